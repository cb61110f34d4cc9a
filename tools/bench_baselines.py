#!/usr/bin/env python3
"""Cross-play against baseline opponents (coevonet_amd.baselines): what a table costs when a seat is not an evolved net.

    python tools/bench_baselines.py [--repeats 5] [--warmup 1] [--out FILE.md]

1. 20 agent_0 x 20 agent_1 evolved nets x {random, periodic, constant, PPO adversary} x 10 episodes: one ``BaselineCrossPlay``
   whose adversary list holds the four baselines (16 000 games), and one table per baseline alone (4 000 games each).
2. The all-net 20 x 20 x 20 x 10 table (80 000 games) through ``BaselineCrossPlay`` - the unfused route, one policy launch per
   task table plus coevo_mpe_step per env-cycle - next to ``CrossPlay`` (the fused rollout) on the same nets; the results are
   compared word for word.
3. The policy-net launch alone (coevo_mlp_forward_argmax) at 80 000 rows of one net.

Protocol (one process): every variant is warmed up, then the variants of a group ALTERNATE for --repeats rounds, one whole
``run()`` each, timed with the host clock around work that ends in a device synchronise; medians with the min .. max spread.
A ``run()`` includes the reset, every env-cycle, the reduction and the copies back.  The lone launch is timed with device
events over 20 launches per round."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from coevonet_amd import baselines as bl   # noqa: E402
from coevonet_amd import crossplay as xp   # noqa: E402
from coevonet_amd import lib as L   # noqa: E402

FIRST = 1


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def alternate(variants, a):
    """{name: object with run()} -> {name: (times in ms, last result)}"""
    for cp in variants.values():
        for _ in range(a.warmup):
            cp.run(FIRST)
    ms, last = {k: [] for k in variants}, {}
    for _ in range(a.repeats):
        for k, cp in variants.items():
            last[k], t = timed(lambda: cp.run(FIRST))
            ms[k].append(t)
    return {k: (np.array(v), last[k]) for k, v in ms.items()}


def row(name, n_games, t):
    med = float(np.median(t))
    return f"| {name} | {n_games} | {med:.2f} ({t.min():.2f} .. {t.max():.2f}) | {n_games / med * 1e3:,.0f} |"


def ppo_adversary():
    z = np.load(os.path.join(REPO, "tests", "golden", "ppo_baseline.npz"))
    return bl.MLPBaseline(z["adversary_0.flat"], 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 3, "at least 3 alternating rounds"
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    from coevonet_amd.fcnetwork import FCNetwork
    torch.manual_seed(1)
    nets = [[FCNetwork(D, 5, "float32") for _ in range(20)] for D in (10, 10, 8)]
    E = 10
    lines = [f"# Cross-play against baseline opponents ({torch.cuda.get_device_name(0)})", "",
             f"warm-up {a.warmup}, then {a.repeats} alternating rounds of one whole `run()` per variant; host clock around work that "
             "ends in a device synchronise; median (min .. max).  20 agent_0 x 20 agent_1 evolved float32 nets, 10 episodes, 25 "
             "env-cycles.", "", "| table | games | one run(), ms | games/s |", "|---|---|---|---|"]
    kinds = {"random": bl.RandomBaseline(0), "periodic": bl.PeriodicBaseline(0), "constant": bl.ConstantBaseline(1),
             "PPO adversary": ppo_adversary()}
    variants = {f"adversary = {k}": bl.BaselineCrossPlay(nets[0], nets[1], [b], episodes=E) for k, b in kinds.items()}
    variants["adversary = [random, periodic, constant, PPO]"] = bl.BaselineCrossPlay(nets[0], nets[1], list(kinds.values()), episodes=E)
    for k, (t, _) in alternate(variants, a).items():
        lines.append(row(k, variants[k].n_games, t))
        print(lines[-1], file=sys.stderr, flush=True)
    del variants
    torch.cuda.empty_cache()
    pair = {"all nets, BaselineCrossPlay (unfused route)": bl.BaselineCrossPlay(*nets, episodes=E),
            "all nets, CrossPlay (fused rollout)": xp.CrossPlay(*nets, episodes=E)}
    got = alternate(pair, a)
    for k, (t, _) in got.items():
        lines.append(row(k, 80000, t))
        print(lines[-1], file=sys.stderr, flush=True)
    (_, ra), (_, rb) = got.values()
    same = all(np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64))
               for x, y in ((ra.rewards, rb.rewards), (ra.payoff, rb.payoff)))
    lines += ["", f"The two routes' rewards and payoffs are {'equal word for word' if same else 'NOT equal'}."]
    del pair, got
    torch.cuda.empty_cache()
    # ---- the policy-net launch alone
    n, D = 80000, 8
    net = ppo_adversary()
    slab = torch.zeros(bl.mlp_stride(D), dtype=torch.float32, device="cuda")
    slab[:net.flat.size].copy_(torch.from_numpy(net.flat))
    tile = bl.MLP_ROW_TILE
    tasks = torch.tensor([(0, lo, min(tile, n - lo), D) for lo in range(0, n, tile)], dtype=torch.int32, device="cuda")
    obs = (torch.rand(n, L.OBS_STRIDE, device="cuda") * 4 - 2).contiguous()
    actions = torch.zeros(n, dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")

    def launch():
        L.call("coevo_mlp_forward_argmax", L._p(slab), slab.numel(), L._p(tasks), len(tasks), L._p(obs), n, L._p(actions), None,
               L._p(status))
    for _ in range(5):
        launch()
    us = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            launch()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / 20 * 1e3)
    us = np.array(us)
    assert status.item() == 0
    lines += ["", f"coevo_mlp_forward_argmax alone, {n} rows of one width-{D} net ({len(tasks)} workgroups of {tile} rows), device "
              f"events over 20 back-to-back launches: {np.median(us):.1f} us per launch ({us.min():.1f} .. {us.max():.1f}) - "
              f"{n / np.median(us):,.0f} rows/us."]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    assert same, "the unfused and the fused route differ"


if __name__ == "__main__":
    main()
