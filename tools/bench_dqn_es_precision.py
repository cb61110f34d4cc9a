#!/usr/bin/env python3
"""float32 against float16 Co-ES update launches of ONE cfg 5-shard generation, from the same base nets, and whole generations
of DQNESEngine against HalfDQNESEngine:

    python tools/bench_dqn_es_precision.py [--repeats 9] [--warmup 3] [--settle-ms 120] [--no-engines] [--out FILE.md]

Update: 2 roles x 250 individuals (C = 4, 18 actions), 8 chunks.  float32: per role coevo_dqn_es_partial (pert - theta over the
perturbed nets coevo_dqn_perturb materialised) + coevo_dqn_es_apply, what DQNESEngine enqueues on one rank; float16: per role
coevo_dqn_es16_partial (the noise drawn again and rounded to fp16; no perturbed net is read) + coevo_dqn_es16_apply, what
HalfDQNESEngine enqueues.  Every parameter of the base nets is an fp16 value and both use the same fitness and noise streams.
After the warm-up the two variants alternate (untimed) until --settle-ms of work has passed, then alternate for --repeats timed
rounds each (device events around the variant's launches); the table has medians and the min .. max spread.

Generations: pop 250, C = 4, 18 actions, T = 200 agent-steps (the cfg 5 shard of bench.py), no fitness sharing, both engines
alternating, host clock around generation() (which ends in a device synchronise).  The float32 engine plays two rollout cohorts
and replays its evaluation games as a graph; the float16 engine plays one cohort and enqueues its evaluation games.

The per-kernel split comes from a run of its own under
    rocprofv3 --kernel-trace --stats -- python tools/bench_dqn_es_precision.py --no-engines --repeats 5
Run it as one GPU step under its own time limit."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from coevonet_amd import lib as L   # noqa: E402

DEV = "cuda"
ROLES = 2
SIGMA, LR = 0.05, 0.1


def half_valued_nets(count, C, n_act, seed):
    """[count][P] fp32 flats whose every entry is an fp16 value; BatchNorm weights near 1"""
    P = int(L.load().coevo_dqn_param_count(C, n_act))
    g = torch.Generator(device=DEV).manual_seed(seed)
    flat = torch.randn(count, P, device=DEV, generator=g) * 0.02
    for lo, hi in ((P - 320, P - 288), (P - 256, P - 192), (P - 128, P - 64)):   # vbn*.weight
        flat[:, lo:hi] += 1.0
    return flat.to(torch.float16).to(torch.float32).contiguous()


def build(precision, flats, fitness, pop, chunks, C, n_act):
    """-> dict(run = enqueue the variant's update launches, bytes read per call, tensors kept alive)"""
    lib = L.load()
    half = precision == "float16"
    stride = int((lib.coevo_dqn16_slab_stride if half else lib.coevo_dqn_slab_stride)(C, n_act))
    floats = int(lib.coevo_dqn_es16_partial_floats(C, n_act)) if half else stride
    zero_idx = torch.zeros(pop, dtype=torch.int32, device=DEV)
    keep = []
    for ri in range(ROLES):   # per role [base | pert x pop]; the float16 update never reads the perturbed nets
        slab = torch.zeros((1 + (0 if half else pop)) * stride, dtype=torch.int32 if half else torch.float32, device=DEV)
        sigma = torch.full((1,), SIGMA, dtype=torch.float32, device=DEV)
        L.call("coevo_dqn16_pack" if half else "coevo_dqn_pack", L._p(flats[ri]), L._p(slab), 1, C, n_act)
        if not half:
            L.call("coevo_dqn_perturb", L._p(slab), L._p(zero_idx), slab.data_ptr() + 4 * stride, 0, pop, C, n_act, L._p(sigma),
                   0, 0, ri, 1, 1, None, 0, None, None)
        keep.append({"slab": slab, "sigma": sigma, "fit": fitness[ri],
                     "part": torch.zeros(chunks * floats, dtype=torch.float32, device=DEV)})
    torch.cuda.synchronize()

    def run():
        for ri, k in enumerate(keep):
            if half:
                L.call("coevo_dqn_es16_partial", C, n_act, L._p(k["fit"]), pop, chunks, L._p(k["sigma"]), 0, 0, ri, L._p(k["part"]))
                L.call("coevo_dqn_es16_apply", L._p(k["slab"]), L._p(k["part"]), chunks, C, n_act, pop, L._p(k["sigma"]), LR)
            else:
                L.call("coevo_dqn_es_partial", L._p(k["slab"]), k["slab"].data_ptr() + 4 * stride, 0, C, n_act, L._p(k["fit"]), pop,
                       chunks, 0, chunks, L._p(k["part"]))
                L.call("coevo_dqn_es_apply", L._p(k["slab"]), L._p(k["part"]), chunks, chunks, chunks * stride, C, n_act, pop,
                       L._p(k["sigma"]), L.C.c_float(LR))
    read = ROLES * 4 * (chunks * floats + (0 if half else pop * stride))
    return {"name": precision, "run": run, "keep": (keep, zero_idx), "ms": [], "bytes": read}


def one(v, timed):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    v["run"]()
    e1.record()
    e1.synchronize()
    if timed:
        v["ms"].append(e0.elapsed_time(e1))


def alternate(variants, a):
    for _ in range(a.warmup):
        for v in variants:
            one(v, False)
    t0, settle = time.perf_counter(), 0
    while (time.perf_counter() - t0) * 1e3 < a.settle_ms:
        for v in variants:
            one(v, False)
        settle += 1
    for _ in range(a.repeats):
        for v in variants:   # alternating: a drift of the clocks lands on both alike
            one(v, True)
    return settle


def verdict(lo, hi):
    if hi < 1.0:
        return "float16 is faster"
    if lo > 1.0:
        return "float16 is slower"
    return "float16 is equal within the spread"


def update(a):
    flats = [half_valued_nets(1, a.C, a.actions, 8 + ri) for ri in range(ROLES)]
    g = torch.Generator(device=DEV).manual_seed(3)
    fitness = [torch.randn(a.pop, device=DEV, generator=g).to(torch.float16).to(torch.float32).contiguous() for _ in range(ROLES)]
    variants = [build(p, flats, fitness, a.pop, a.chunks, a.C, a.actions) for p in ("float32", "float16")]
    settle = alternate(variants, a)
    P = int(L.load().coevo_dqn_param_count(a.C, a.actions))
    lines = ["## Update launches of one generation", "",
             f"{ROLES} roles x {a.pop} individuals (C = {a.C}, {a.actions} actions), {a.chunks} chunks; float32 = per role "
             "coevo_dqn_es_partial (reads the perturbed nets) + coevo_dqn_es_apply, float16 = per role coevo_dqn_es16_partial "
             f"(draws {ROLES} x {a.pop} x {(P - 320) / 1e6:.2f} M normals again, reads no net) + coevo_dqn_es16_apply; warm-up "
             f"{a.warmup}, {settle} settling rounds ({a.settle_ms:.0f} ms), {a.repeats} alternating timed repeats of each variant.",
             "", "| variant | MB read (nets + partials) | median ms | min .. max ms |", "|---|---|---|---|"]
    for v in variants:
        ms = np.array(v["ms"])
        lines.append(f"| {v['name']} | {v['bytes'] / 1e6:.1f} | {np.median(ms):.4f} | {ms.min():.4f} .. {ms.max():.4f} |")
    m32 = float(np.median(variants[0]["ms"]))
    r = np.array(variants[1]["ms"]) / m32
    lines += ["", f"fp16 / fp32 median: {float(np.median(r)):.3f} (fp16 repeats over the fp32 median: {r.min():.3f} .. "
              f"{r.max():.3f}): {verdict(r.min(), r.max())}", ""]
    return lines


def generations(a):
    from coevonet_amd.dqn_es_half import HalfDQNESEngine
    from coevonet_amd.dqn_population import DQNESEngine
    flats = [half_valued_nets(1, a.C, a.actions, 20 + ri).cpu().numpy() for ri in range(ROLES)]
    engines = []
    for name, cls in (("float32 DQNESEngine", DQNESEngine), ("float16 HalfDQNESEngine", HalfDQNESEngine)):
        eng = cls(a.pop, a.C, a.actions, a.T, a.T, device=DEV, chunks=a.chunks)
        for ri, r in enumerate(("first_0", "second_0")):
            eng.upload(r, "base", 0, flats[ri])
        engines.append({"name": name, "eng": eng, "ms": [], "gen": 0})

    def step(e, timed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e["eng"].generation(e["gen"], (SIGMA, SIGMA), LR, False)
        if timed:
            e["ms"].append((time.perf_counter() - t0) * 1e3)
        e["gen"] += 1
    for _ in range(a.warmup):
        for e in engines:
            step(e, False)
    for _ in range(a.repeats):
        for e in engines:
            step(e, True)
    lines = ["## Whole generations", "",
             f"pop {a.pop}, C = {a.C}, {a.actions} actions, T = {a.T} agent-steps ({engines[0]['eng'].steps_per_generation} "
             f"agent-steps per generation), no fitness sharing; warm-up {a.warmup} generations, {a.repeats} alternating timed "
             "generations of each engine, host clock around generation() (ends in a device synchronise).", "",
             "| engine | median ms / generation | min .. max ms | generations/s (median) |", "|---|---|---|---|"]
    for e in engines:
        ms = np.array(e["ms"])
        lines.append(f"| {e['name']} | {np.median(ms):.2f} | {ms.min():.2f} .. {ms.max():.2f} | {1e3 / np.median(ms):.2f} |")
    m32 = float(np.median(engines[0]["ms"]))
    r = np.array(engines[1]["ms"]) / m32
    lines += ["", f"fp16 / fp32 median generation time: {float(np.median(r)):.3f} ({r.min():.3f} .. {r.max():.3f}): "
              f"{verdict(r.min(), r.max())}", ""]
    engines[0]["eng"].ro.close()
    engines[0]["eng"].eval_ro.close()
    engines[1]["eng"].close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pop", type=int, default=250)
    ap.add_argument("--C", type=int, default=4)
    ap.add_argument("--actions", type=int, default=18)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=120.0)
    ap.add_argument("--no-engines", action="store_true", help="the update launches only (the form to run under rocprofv3)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 5, "at least 5 repeats of each variant"
    lines = [f"# float32 vs float16 DeepQN Co-ES update ({torch.cuda.get_device_name(0)})", ""] + update(a)
    torch.cuda.empty_cache()
    if not a.no_engines:
        lines += generations(a)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
