#!/usr/bin/env python3
"""Population sharing over float16 nets (include/coevo_sharing16.h): what the fp16 pairwise launch and HalfGAEngine's two
extension modes cost.

    python tools/bench_sharing16.py [--repeats 9] [--warmup 3] [--settle-ms 120] [--out profiles/r28_fp16_population_sharing.md]

Kernel: all pairwise distances of the same 200 nets (fp16-valued Linear entries, D = 10 and 8) by coevo_fc16_pairwise_distance
on their fp16 slab against coevo_fc_pairwise_distance on their fp32 slab (two launches each).  Device events around each call.

Generation: HalfGAEngine at the cfg 2 shape (pop 200, HoF 5, elites 2, T 200; fp16-valued random nets, sigma 0.05) with the
switches off, with hof_mean, and with both: host clock around rollout + select + breed, ending in a device synchronise.

Both tables: warm-up 3 rounds, then the variants alternate untimed until --settle-ms of work has passed, then alternate for
--repeats timed rounds each; median and min .. max.  Run it as one GPU step under its own time limit."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from coevonet_amd import lib as L                   # noqa: E402
from coevonet_amd.ga_half import HalfGAEngine       # noqa: E402
from tools.bench_precision import ROLE_D, ROLES, random_flat   # noqa: E402

DEV = "cuda"


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def protocol(variants, a):
    """variants: [(name, fn() -> ms)] -> {name: [ms] of the timed rounds}, settling rounds"""
    for _ in range(a.warmup):
        for _, fn in variants:
            fn()
    t0, settle = time.perf_counter(), 0
    while (time.perf_counter() - t0) * 1e3 < a.settle_ms:
        for _, fn in variants:
            fn()
        settle += 1
    times = {name: [] for name, _ in variants}
    for _ in range(a.repeats):
        for name, fn in variants:   # alternating: a drift of the clocks lands on every variant alike
            times[name].append(fn())
    return times, settle


def row(name, ms, fmt="{:.4f}"):
    ms = np.asarray(ms)
    return f"| {name} | {fmt.format(float(np.median(ms)))} | {fmt.format(float(ms.min()))} .. {fmt.format(float(ms.max()))} |"


def kernel_lines(a, n=200):
    lines = []
    for D in (10, 8):
        flats = np.stack([random_flat(np.random.default_rng(28 + D + i), D) for i in range(n)])
        src = torch.from_numpy(flats).to(DEV)
        s32 = torch.zeros(n * L.fc_slab_stride(D), dtype=torch.float32, device=DEV)
        s16 = torch.zeros(n * L.fc16_slab_stride(D), dtype=torch.int32, device=DEV)
        L.call("coevo_fc_pack", L._p(src), L._p(s32), n, D)
        L.call("coevo_fc16_pack", L._p(src), L._p(s16), n, D)
        lib = L.load()
        sc32 = torch.zeros(int(lib.coevo_fc_pairwise_scratch_doubles(n, D)), dtype=torch.float64, device=DEV)
        sc16 = torch.zeros(int(lib.coevo_fc16_pairwise_scratch_doubles(n, D)), dtype=torch.float64, device=DEV)
        d32, d16 = (torch.zeros(n, n, dtype=torch.float32, device=DEV) for _ in range(2))
        variants = [("coevo_fc_pairwise_distance (fp32 slab)", lambda: event_ms(
                        lambda: L.call("coevo_fc_pairwise_distance", L._p(s32), n, D, L._p(sc32), L._p(d32)))),
                    ("coevo_fc16_pairwise_distance (fp16 slab)", lambda: event_ms(
                        lambda: L.call("coevo_fc16_pairwise_distance", L._p(s16), n, D, L._p(sc16), L._p(d16))))]
        times, settle = protocol(variants, a)
        m32, m16 = (float(np.median(times[name])) for name, _ in variants)
        mb32, mb16 = 4 * n * L.fc_slab_stride(D) / 1e6, 4 * n * L.fc16_slab_stride(D) / 1e6
        lines += [f"### n = {n}, D = {D} ({settle} settling rounds)", "", "| launch pair | median ms | min .. max ms |",
                  "|---|---|---|"]
        lines += [row(name, times[name]) for name, _ in variants]
        rel = float(torch.max(torch.abs(d16 - d32) / torch.clamp(d32, min=1e-30)).item())
        lines += ["", f"fp16 median / fp32 median: {m16 / m32:.3f}; slab {mb32:.1f} MB (fp32) / {mb16:.1f} MB (fp16); largest "
                  f"relative gap between the two matrices {rel:.2e} (the fp16 contract rounds each term and the root)", ""]
        print("\n".join(lines[-8:]), file=sys.stderr, flush=True)
    return lines


def generation_lines(a, pop=200, hof=5, elites=2, T=200):
    rng = np.random.default_rng(0)
    pop_flat = {r: np.stack([random_flat(rng, ROLE_D[r]) for _ in range(pop)]) for r in ROLES}
    hof_flat = {r: np.stack([random_flat(rng, ROLE_D[r]) for _ in range(hof)]) for r in ROLES}
    sigmas = {r: 0.05 for r in ROLES}
    modes = (("switches off", {}), ("hof_mean", dict(hof_mean=True)),
             ("hof_mean + population_sharing", dict(hof_mean=True, population_sharing=True)))
    variants = []
    for name, kw in modes:
        eng = HalfGAEngine(pop, hof, elites, T, T, **kw)
        eng.load_initial(pop_flat, hof_flat)
        state = {"gen": 0}

        def step(eng=eng, state=state):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.rollout(state["gen"])
            eng.select()
            eng.breed(state["gen"], sigmas)
            torch.cuda.synchronize()
            state["gen"] += 1
            return (time.perf_counter() - t0) * 1e3
        variants.append((name, step))
    times, settle = protocol(variants, a)
    base = float(np.median(times[modes[0][0]]))
    lines = ["", f"## HalfGAEngine generation, pop {pop}, HoF {hof}, elites {elites}, T {T} ({settle} settling rounds)", "",
             "| variant | median ms | min .. max ms | against switches off, ms |", "|---|---|---|---|"]
    for name, _ in modes:
        lines.append(row(name, times[name], "{:.3f}") + f" {float(np.median(times[name])) - base:+.3f} |")
    print("\n".join(lines), file=sys.stderr, flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-ms", type=float, default=120.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r28_fp16_population_sharing.md"))
    a = ap.parse_args()
    assert a.repeats >= 5 and a.warmup >= 1, "at least 5 repeats and one warm-up round"
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    lines = [f"# fp16 population sharing: the pairwise launch and HalfGAEngine's modes ({torch.cuda.get_device_name(0)})", "",
             f"Warm-up {a.warmup}, {a.settle_ms:.0f} ms of settling, {a.repeats} alternating timed repeats of each variant.", "",
             "## The pairwise launch pair on the same 200 nets", ""]
    lines += kernel_lines(a)
    lines += generation_lines(a)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
