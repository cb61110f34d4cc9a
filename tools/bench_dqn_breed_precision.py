#!/usr/bin/env python3
"""float32 against float16 DeepQN breeding launches of ONE cfg 4-shard generation, from the same elites, and whole generations
of DQNGAEngine against HalfDQNGAEngine:

    python tools/bench_dqn_breed_precision.py [--repeats 9] [--warmup 3] [--settle-ms 120] [--no-engines] [--out FILE.md]

Breeding: 2 roles x 49 children from E = 2 elites (pop 50, C = 4, 6 actions), stale-agent distances fused in.  float32: per role
coevo_dqn_perturb (tiled fc1 layout, what DQNGAEngine enqueues) + coevo_fc_distance_finalize; float16: per role
coevo_dqn16_perturb_dist + coevo_fc16_distance_finalize (what HalfDQNGAEngine enqueues).  Every parameter of the elites is an
fp16 value, so both precisions breed from the same nets with the same noise streams.  After the warm-up the two variants
alternate (untimed) until --settle-ms of work has passed, then alternate for --repeats timed rounds each (device events around
the variant's launches); the table has medians and the min .. max spread.

Generations: pop 50, HoF 10, 2 elites, C = 4, T = 200 agent-steps (the cfg 4 shard of bench.py), both engines replaying their
captured generation, alternating, a device synchronise after each.

The per-kernel split comes from a run of its own under
    rocprofv3 --kernel-trace --stats -- python tools/bench_dqn_breed_precision.py --no-engines --repeats 5
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


def half_valued_nets(count, C, n_act, seed):
    """[count][P] fp32 flats whose every entry is an fp16 value; BatchNorm weights near 1"""
    P = int(L.load().coevo_dqn_param_count(C, n_act))
    g = torch.Generator(device=DEV).manual_seed(seed)
    flat = torch.randn(count, P, device=DEV, generator=g) * 0.02
    for lo, hi in ((P - 320, P - 288), (P - 256, P - 192), (P - 128, P - 64)):   # vbn*.weight
        flat[:, lo:hi] += 1.0
    return flat.to(torch.float16).to(torch.float32).contiguous()


def build(precision, flats, pop, E, C, n_act):
    """-> dict(run = enqueue the variant's launches, child bytes written per call, tensors kept alive)"""
    lib = L.load()
    half = precision == "float16"
    Cw = C if half else C | L.DQN_FC1_TILED
    stride = int((lib.coevo_dqn16_slab_stride if half else lib.coevo_dqn_slab_stride)(C, n_act))
    nb = int((lib.coevo_dqn16_perturb_blocks if half else lib.coevo_dqn_perturb_blocks)(Cw, n_act))
    idx = torch.tensor([c % E for c in range(pop - 1)], dtype=torch.int32, device=DEV)
    keep = []
    for ri in range(ROLES):   # per role [elite E | stale 1 | pop]
        slab = torch.zeros((E + 1 + pop) * stride, dtype=torch.int32 if half else torch.float32, device=DEV)
        L.call("coevo_dqn16_pack" if half else "coevo_dqn_pack", L._p(flats[ri]), L._p(slab), E + 1, Cw, n_act)
        keep.append({"slab": slab, "part": torch.zeros((pop - 1) * nb, dtype=torch.float64, device=DEV),
                     "dist": torch.zeros(pop, dtype=torch.float32, device=DEV),
                     "head": torch.zeros(1, dtype=torch.float32, device=DEV),
                     "sigma": torch.full((1,), 0.05, dtype=torch.float32, device=DEV)})
    at = lambda k, net: k["slab"].data_ptr() + 4 * net * stride   # noqa: E731

    def run():
        for ri, k in enumerate(keep):
            if half:
                L.call("coevo_dqn16_perturb_dist", at(k, 0), L._p(idx), at(k, E + 1), 1, pop - 1, C, n_act, L._p(k["sigma"]), 0, 0,
                       ri, 0, None, 0, at(k, E), L._p(k["part"]))
                L.call("coevo_fc16_distance_finalize", L._p(k["part"]), nb, pop - 1, L._p(k["dist"]), 1, L._p(k["head"]))
            else:
                L.call("coevo_dqn_perturb", at(k, 0), L._p(idx), at(k, E + 1), 1, pop - 1, Cw, n_act, L._p(k["sigma"]), 0, 0, ri,
                       0, E, None, 0, at(k, E), L._p(k["part"]))
                L.call("coevo_fc_distance_finalize", L._p(k["part"]), nb, pop - 1, L._p(k["dist"]), 1, L._p(k["head"]))
    return {"name": precision, "run": run, "keep": (keep, idx), "ms": [], "bytes": ROLES * 4 * stride * (pop - 1),
            "dist": [k["dist"] for k in keep]}


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


def verdict(ratio, lo, hi):
    if hi < 1.0:
        return "float16 is faster"
    if lo > 1.0:
        return "float16 is slower"
    return "float16 is equal within the spread"


def breeding(a):
    flats = [half_valued_nets(a.elites + 1, a.C, a.actions, 8 + ri) for ri in range(ROLES)]
    variants = [build(p, flats, a.pop, a.elites, a.C, a.actions) for p in ("float32", "float16")]
    settle = alternate(variants, a)
    d32 = np.concatenate([d.cpu().numpy()[1:] for d in variants[0]["dist"]])
    d16 = np.concatenate([d.cpu().numpy()[1:] for d in variants[1]["dist"]])
    rel = float(np.max(np.abs(d16 - d32) / d32))
    lines = ["## Breeding launches of one generation", "",
             f"{ROLES} roles x {a.pop - 1} children from {a.elites} elites (C = {a.C}, {a.actions} actions), stale-agent distances "
             "fused in; float32 = per role coevo_dqn_perturb (tiled fc1) + coevo_fc_distance_finalize, float16 = per role "
             f"coevo_dqn16_perturb_dist + coevo_fc16_distance_finalize; warm-up {a.warmup}, {settle} settling rounds "
             f"({a.settle_ms:.0f} ms), {a.repeats} alternating timed repeats of each variant.", "",
             "| variant | child MB written | median ms | min .. max ms | median GB/s written |", "|---|---|---|---|---|"]
    for v in variants:
        ms = np.array(v["ms"])
        med = float(np.median(ms))
        lines.append(f"| {v['name']} | {v['bytes'] / 1e6:.1f} | {med:.4f} | {ms.min():.4f} .. {ms.max():.4f} | "
                     f"{v['bytes'] / med / 1e6:.0f} |")
    m32 = float(np.median(variants[0]["ms"]))
    r = np.array(variants[1]["ms"]) / m32
    lines += ["", f"fp16 / fp32 median: {float(np.median(r)):.3f} (fp16 repeats over the fp32 median: {r.min():.3f} .. "
              f"{r.max():.3f}): {verdict(float(np.median(r)), r.min(), r.max())}",
              f"largest relative difference between the fp16 and the fp32 children's distances: {rel:.2e} "
              "(the fp16 children are the rounded fp32 children)", ""]
    return lines


def generations(a):
    from coevonet_amd.dqn_ga_half import HalfDQNGAEngine
    from coevonet_amd.dqn_population import DQNGAEngine
    pop_flat = {r: half_valued_nets(a.pop, a.C, a.actions, 20 + i).cpu().numpy() for i, r in enumerate(("first_0", "second_0"))}
    hof_flat = {r: half_valued_nets(a.hof, a.C, a.actions, 30 + i).cpu().numpy() for i, r in enumerate(("first_0", "second_0"))}
    engines = []
    for name, cls in (("float32 DQNGAEngine", DQNGAEngine), ("float16 HalfDQNGAEngine", HalfDQNGAEngine)):
        eng = cls(a.pop, a.hof, a.elites, a.C, a.actions, a.T, a.T, device=DEV, capacity=4096)
        eng.load_initial(pop_flat, hof_flat)
        engines.append({"name": name, "eng": eng, "ms": []})

    def step(e, timed):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e["eng"].step(use_graph=True)
        torch.cuda.synchronize()
        if timed:
            e["ms"].append((time.perf_counter() - t0) * 1e3)
    for _ in range(a.warmup):
        for e in engines:
            step(e, False)
    for _ in range(a.repeats):
        for e in engines:
            step(e, True)
    for e in engines:
        L.raise_on_status(e["eng"].ro.status)
    lines = ["## Whole generations", "",
             f"pop {a.pop}, HoF {a.hof}, {a.elites} elites, C = {a.C}, {a.actions} actions, T = {a.T} agent-steps "
             f"({engines[0]['eng'].steps_per_generation} agent-steps per generation), the captured generation replayed; warm-up "
             f"{a.warmup} generations, {a.repeats} alternating timed generations of each engine, host clock around replay + "
             "device synchronise.", "", "| engine | median ms / generation | min .. max ms | generations/s (median) |",
             "|---|---|---|---|"]
    for e in engines:
        ms = np.array(e["ms"])
        lines.append(f"| {e['name']} | {np.median(ms):.2f} | {ms.min():.2f} .. {ms.max():.2f} | {1e3 / np.median(ms):.2f} |")
    m32 = float(np.median(engines[0]["ms"]))
    r = np.array(engines[1]["ms"]) / m32
    lines += ["", f"fp16 / fp32 median generation time: {float(np.median(r)):.3f} ({r.min():.3f} .. {r.max():.3f}): "
              f"{verdict(float(np.median(r)), r.min(), r.max())}", ""]
    for e in engines:
        e["eng"].ro.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pop", type=int, default=50)
    ap.add_argument("--hof", type=int, default=10)
    ap.add_argument("--elites", type=int, default=2)
    ap.add_argument("--C", type=int, default=4)
    ap.add_argument("--actions", type=int, default=6)
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=120.0)
    ap.add_argument("--no-engines", action="store_true", help="the breeding launches only (the form to run under rocprofv3)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 5, "at least 5 repeats of each variant"
    lines = [f"# float32 vs float16 DeepQN breeding ({torch.cuda.get_device_name(0)})", ""] + breeding(a)
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
