#!/usr/bin/env python3
"""Population sharing (include/coevo_sharing.h): what the pairwise-distance kernels and the two Co-GA extension modes cost.

    python tools/bench_sharing.py [--repeats 7] [--warmup 2] [--generations 12] [--kernel-only] [--out FILE.md]

Kernel: all pairwise distances of n = 200 nets (D = 10 and 8) by ``coevo_fc_pairwise_distance`` (two launches) against the only
route the library had to the same matrix: 200 ``coevo_fc_distance`` launches, one per reference net, into the rows of one
buffer.  The words that differ between the routes are counted (random nets are not order-proof).  Device events around each
whole route, warm-up, then --repeats alternating rounds; median (min .. max).

Generation: the host-driven trainer (``args.coevo_device_loop = False``, device_philox, collect off) at the cfg 2 shape (pop 200,
HoF 5, T 200), with the switches off, with ``coevo_hof_mean``, and with both switches: milliseconds per generation over
--generations generations in two rounds over the variants, each block behind --warmup untimed generations.  The difference is
what the modes cost; the headline loop (host-free, pipelined) does not carry them."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from coevonet_amd import genetic_algorithm as ga   # noqa: E402
from coevonet_amd import lib as L   # noqa: E402
from coevonet_amd.game_logic import initialize_env   # noqa: E402
from tests.util import Bag   # noqa: E402

DEV = "cuda"


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(v, fmt="{:.3f}"):
    v = np.asarray(v)
    return f"{fmt.format(float(np.median(v)))} ({fmt.format(float(v.min()))} .. {fmt.format(float(v.max()))})"


def kernel_rows(a, n=200):
    rows = []
    for D in (10, 8):
        stride = L.fc_slab_stride(D)
        g = torch.Generator(device=DEV).manual_seed(D)
        slab = torch.randn(n, stride, generator=g, device=DEV, dtype=torch.float32) * 0.1
        scratch = torch.zeros(int(L.load().coevo_fc_pairwise_scratch_doubles(n, D)), dtype=torch.float64, device=DEV)
        new, old = (torch.zeros(n, n, dtype=torch.float32, device=DEV) for _ in range(2))

        def pairwise():
            L.call("coevo_fc_pairwise_distance", L._p(slab), n, D, L._p(scratch), L._p(new))

        def row_by_row():
            for i in range(n):
                L.call("coevo_fc_distance", slab.data_ptr() + 4 * i * stride, L._p(slab), n, D, old.data_ptr() + 4 * i * n)
        for _ in range(a.warmup):
            pairwise()
            row_by_row()
        torch.cuda.synchronize()
        # (random nets are not order-proof: the two routes add their fp64 terms in other orders, so a word in a few thousand
        # may round the other way - counted, with the largest gap in fp32 ulps; tests/test_sharing_gpu.py has the equalities)
        gap = (new.view(torch.int32).long() - old.view(torch.int32).long()).abs()
        words = f"{int((gap != 0).sum())} of {n * n} differ, by at most {int(gap.max())} ulp"
        t_new, t_old = [], []
        for _ in range(a.repeats):
            t_new.append(event_ms(pairwise))
            t_old.append(event_ms(row_by_row))
        below = max(t_new) < min(t_old)
        rows.append(f"| {n} | {D} | {spread(t_new)} | {spread(t_old)} | {np.median(t_old) / np.median(t_new):.1f}x | "
                    f"{'wholly below' if below else 'OVERLAP'} | {words} |")
        print(rows[-1], file=sys.stderr, flush=True)
    return rows


def generation_rows(a):
    variants = (("switches off", {}), ("coevo_hof_mean", dict(coevo_hof_mean=True)),
                ("coevo_hof_mean + coevo_population_sharing", dict(coevo_hof_mean=True, coevo_population_sharing=True)))
    trainers = []
    for name, kw in variants:
        torch.manual_seed(1)
        args = Bag(algorithm="GA", generations=a.generations + 2 * a.warmup, population=200, hof_size=5, elites_number=2,
                   max_timesteps_per_episode=200, max_evaluation_steps=200, fitness_sharing=True, coevo_device_loop=False, **kw)
        env = initialize_env(args)
        trainers.append((name, ga.GATrainer(env, args, rng="device_philox", env_mode="device", collect=False)))
    times = {name: [] for name, _ in trainers}
    for _ in range(2):   # two rounds over the variants; within a round a variant keeps the chip (and its cache) to itself
        for name, tr in trainers:
            for g in range(a.warmup + a.generations // 2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.step()
                torch.cuda.synchronize()
                if g >= a.warmup:
                    times[name].append((time.perf_counter() - t0) * 1e3)
    base = float(np.median(times[variants[0][0]]))
    rows = []
    for name, _ in trainers:
        med = float(np.median(times[name]))
        rows.append(f"| {name} | {spread(times[name], '{:.2f}')} | {med - base:+.2f} | {1e3 / med:.1f} |")
        print(rows[-1], file=sys.stderr, flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--generations", type=int, default=12)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true", help="the kernel table alone (for a run under a kernel trace)")
    a = ap.parse_args()
    assert a.repeats >= 3 and a.warmup >= 1 and a.generations >= 5
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    lines = [f"# Population sharing: the pairwise kernels and the modes' cost ({torch.cuda.get_device_name(0)})", "",
             f"Kernel: warm-up {a.warmup}, then {a.repeats} alternating rounds, device events around each whole route; median "
             "(min .. max) in ms.", "",
             "| n | D | coevo_fc_pairwise_distance, ms | n x coevo_fc_distance, ms | ratio | new range vs old | words |",
             "|---|---|---|---|---|---|---|"]
    lines += kernel_rows(a)
    if not a.kernel_only:
        lines += generation_lines(a)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


def generation_lines(a):
    lines = ["", "Generation: host-driven trainer, pop 200, HoF 5, T 200, device_philox, collect off; two rounds over the "
              f"variants, in each {a.warmup} warm-up then {a.generations // 2} timed generations per variant; host clock around a "
              "step that ends in a device synchronise; median (min .. max) in ms.", "",
              "| variant | generation, ms | against switches off, ms | generations/s |", "|---|---|---|---|"]
    return lines + generation_rows(a)


if __name__ == "__main__":
    main()
