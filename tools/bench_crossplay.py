#!/usr/bin/env python3
"""Cross-play as ONE device rollout (coevonet_amd.crossplay) against the only route the package had for the same games: a
Python loop over the façade ``play_game``, one game per call.

    python tools/bench_crossplay.py [--repeats 5] [--sample 200] [--warmup 1] [--out FILE.md]

``CrossPlay`` at (A, B, C, E) = (20, 20, 20, 10) - 80 000 simple_adversary games - in float32 and float16, and ``DQNCrossPlay``
at (8, 8, 4), C = 4 / 6 actions, limit 200, in float32 and float16.  The loop is timed over a seeded sample of --sample of
those games (at least 200) and scaled to the count; every sampled game's rewards are compared, bit for bit, with the rollout's.

Protocol (one process, one command): both variants are warmed up, then they ALTERNATE for --repeats rounds - one whole
``run()`` of the rollout, then one chunk of the sample through ``play_game`` - each timed with the host clock around work that
ends in a device synchronise (``run()`` and ``play_game`` both end in a device-to-host copy of their results).  Medians with
the min .. max spread.  The rollout's time includes everything ``run()`` does: limits, reset, rollout, reduction, copies back."""
import argparse
import os
import sys
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from coevonet_amd import crossplay as xp   # noqa: E402
from coevonet_amd import game_logic as gl   # noqa: E402

FIRST = 1   # the first reset ordinal behind initialize_env's own


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def bench(name, cp, dims, E, sample, play, a):
    """cp.run(FIRST) against play(index tuple, episode) over `sample`: -> (markdown row, all sampled games equal?)"""
    n = int(np.prod(dims)) * E
    chunks = np.array_split(np.arange(len(sample)), a.repeats)
    for _ in range(a.warmup):
        cp.run(FIRST)
        for g in sample[:10]:
            play(g)
    run_ms, loop_ms, same = [], [], True
    for chunk in chunks:
        res, ms = timed(lambda: cp.run(FIRST))
        run_ms.append(ms)
        got, ms = timed(lambda: [play(sample[i]) for i in chunk])
        loop_ms.append(ms / len(chunk))
        for i, r in zip(chunk, got):
            want = res.rewards[tuple(sample[i])]
            same = same and np.array_equal(np.array(r, dtype=np.float64).view(np.uint64),
                                           np.ascontiguousarray(want[:len(r)]).view(np.uint64))
    run_ms, loop_ms = np.array(run_ms), np.array(loop_ms) * n
    med_run, med_loop = float(np.median(run_ms)), float(np.median(loop_ms))
    row = (f"| {name} | {n} | {med_run:.1f} ({run_ms.min():.1f} .. {run_ms.max():.1f}) | {n / med_run * 1e3:,.0f} | "
           f"{med_loop:,.0f} ({loop_ms.min():,.0f} .. {loop_ms.max():,.0f}) | {n / med_loop * 1e3:,.0f} | "
           f"{med_loop / med_run:,.0f}x | {'equal' if same else 'NOT equal'} |")
    return row, same


def mpe(precision, a):
    from coevonet_amd.fcnetwork import FCNetwork, FCNetworkHalf
    dims, E = (20, 20, 20), 10
    args = types.SimpleNamespace(game="simple_adversary_v3", precision=precision, max_evaluation_steps=None,
                                 max_timesteps_per_episode=None, render=False)
    env = gl.initialize_env(args)
    torch.manual_seed(1)
    net = FCNetworkHalf if precision == "float16" else FCNetwork
    nets = [[net(D, 5, precision) for _ in range(n)] for n, D in zip(dims, (10, 10, 8))]
    cp = xp.CrossPlay(*nets, episodes=E, precision=precision, env_seed=env.seed_value)
    g = np.random.Generator(np.random.PCG64(3))
    sample = np.stack([g.integers(0, d, a.sample) for d in (*dims, E)], axis=1)

    def play(idx):
        i, j, k, e = (int(x) for x in idx)
        env.n_resets = FIRST + e          # play_game's own env.reset() then takes this ordinal
        return gl.play_game(env, nets[0][i], nets[1][j], nets[2][k], args, eval=True)
    return bench(f"CrossPlay {dims} x {E}, {precision}", cp, dims, E, sample, play, a)


def dqn(precision, a):
    from coevonet_amd.deepqn import DeepQN, DeepQNHalf
    dims, E, C, n_act, limit = (8, 8), 4, 4, 6, 200
    args = types.SimpleNamespace(game="pong_v3", precision=precision, max_evaluation_steps=limit,
                                 max_timesteps_per_episode=limit, coevo_channels=C)
    env = gl.initialize_env(args)
    torch.manual_seed(2)
    net = DeepQNHalf if precision == "float16" else DeepQN
    nets = [[net(C, n_act, precision) for _ in range(n)] for n in dims]
    cp = xp.DQNCrossPlay(*nets, C, n_act, episodes=E, limit=limit, precision=precision, env_seed=env.seed_value)
    g = np.random.Generator(np.random.PCG64(4))
    sample = np.stack([g.integers(0, d, a.sample) for d in (*dims, E)], axis=1)

    def play(idx):
        i, j, e = (int(x) for x in idx)
        env.n_resets = FIRST + e
        return gl.play_game(env, nets[0][i], nets[1][j], args=args, eval=True)
    return bench(f"DQNCrossPlay {dims} x {E}, C = {C} / {n_act} actions, limit {limit}, {precision}", cp, dims, E, sample, play, a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.sample >= 200 and a.repeats >= 3, "a sample of at least 200 games, at least 3 alternating rounds"
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    lines = [f"# Cross-play: one device rollout against the play_game loop ({torch.cuda.get_device_name(0)})", "",
             f"warm-up {a.warmup}, then {a.repeats} alternating rounds: one whole `run()` of the rollout, then a chunk of the seeded "
             f"sample of {a.sample} games through the façade `play_game` (scaled to the game count); host clock around work that ends "
             "in a device synchronise; median (min .. max).", "",
             "| workload | games | one rollout, ms | games/s | play_game loop, ms (scaled) | games/s | ratio | sampled rewards |",
             "|---|---|---|---|---|---|---|---|"]
    ok = True
    for fn, precision in ((mpe, "float32"), (mpe, "float16"), (dqn, "float32"), (dqn, "float16")):
        row, same = fn(precision, a)
        lines.append(row)
        print(row, file=sys.stderr, flush=True)   # (as it goes; the table follows on stdout)
        ok = ok and same
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    assert ok, "a sampled play_game differs from the rollout's game"


if __name__ == "__main__":
    main()
