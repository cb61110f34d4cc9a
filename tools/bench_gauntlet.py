#!/usr/bin/env python3
"""The baseline gauntlet (coevonet_amd.gauntlet): what a generation's absolute score costs.

    python tools/bench_gauntlet.py [--repeats 5] [--warmup 2] [--generations 10] [--out profiles/r30_gauntlet.md]

1. The reference table - the champion pair (agent_0, agent_1) against [Random, Periodic, AlwaysFire, the PPO adversary] and
   [(PPO, PPO), (Random, Random)] against the champion adversary, 10 episodes: 60 games - through one ``Gauntlet.run()`` (four
   launches) and through ``BaselineCrossPlay``, the per-cycle route: one 1 x 1 x 4 table and one 1 x 1 x 1 table per agent pair
   (a 2 x 2 x 1 table would play the cross product, 40 games instead of 20).  The results are compared word for word.
2. The policy net alone: coevo_mlp_forward_argmax_wave (one wave per row) against coevo_mlp_forward_argmax (one thread per row)
   at 1, 60, 4 000 and 80 000 rows of one net.
3. A host-driven float32 generation at the cfg 2 shape (pop 200, HoF 5, T 200, device_philox, collect off) with the gauntlet
   off, on, and replaced by the same tables rebuilt as ``BaselineCrossPlay`` objects every generation from downloaded champions.

Protocol (one process): every variant is warmed up, then the variants of a group ALTERNATE for --repeats rounds; median
(min .. max).  Device time: device events around the enqueued work.  Host time: the host clock around work that ends in a device
synchronise.  Enqueue time: the host clock around the enqueue alone.  A profile (rocprofv3 --kernel-trace --stats) is a run of
its own: --table-only plays the table alone."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from coevonet_amd import baselines as bl   # noqa: E402
from coevonet_amd import gauntlet as gt   # noqa: E402
from coevonet_amd import genetic_algorithm as ga   # noqa: E402
from coevonet_amd import lib as L   # noqa: E402
from coevonet_amd.game_logic import initialize_env   # noqa: E402
from tests.util import Bag   # noqa: E402

FIRST, E = 1, 10


def ppo(role):
    z = np.load(os.path.join(REPO, "tests", "golden", "ppo_baseline.npz"))
    return bl.MLPBaseline(z[f"{role}.flat"], 8 if role == "adversary_0" else 10)


def reference_spec():
    return gt.GauntletSpec(adversaries=[bl.RandomBaseline(1), bl.PeriodicBaseline(0), bl.AlwaysFire, ppo("adversary_0")],
                           agent_pairs=[(ppo("agent_0"), ppo("agent_1")), (bl.RandomBaseline(2), bl.RandomBaseline(3))], episodes=E)


def spread(v, fmt="{:.3f}"):
    v = np.asarray(v, dtype=np.float64)
    return f"{fmt.format(float(np.median(v)))} ({fmt.format(float(v.min()))} .. {fmt.format(float(v.max()))})"


def verdict(new, old):
    """the README's wording: a speed-up only where the ranges are disjoint"""
    new, old = np.asarray(new), np.asarray(old)
    if new.max() < old.min():
        return f"faster, ranges disjoint ({np.median(old) / np.median(new):.2f}x)"
    if new.min() > old.max():
        return f"slower, ranges disjoint ({np.median(new) / np.median(old):.2f}x the time)"
    return "equal within the spread"


def crossplay_tables(spec, champ):
    """the per-cycle route to the spec's games: BaselineCrossPlay objects whose concatenated trios are spec.matches()"""
    tables = [bl.BaselineCrossPlay([champ["agent_0"]], [champ["agent_1"]], spec.adversaries, episodes=spec.episodes)] \
        if spec.adversaries else []
    return tables + [bl.BaselineCrossPlay([p], [q], [champ["adversary_0"]], episodes=spec.episodes) for p, q in spec.agent_pairs]


def measure(fn, enqueue_only=None):
    """(device ms by events, host ms around fn + synchronise, host ms of the enqueue alone or None)"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    host = (time.perf_counter() - t0) * 1e3
    enq = None
    if enqueue_only is not None:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enqueue_only()
        enq = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
    return out, e0.elapsed_time(e1), host, enq


def table_lines(a):
    from coevonet_amd.fcnetwork import FCNetwork
    torch.manual_seed(1)
    champ = {r: FCNetwork(D, 5, "float32").flat() for r, D in (("agent_0", 10), ("agent_1", 10), ("adversary_0", 8))}
    spec = reference_spec()
    g = gt.Gauntlet(spec.matches(), episodes=E)
    for r in spec.champion_roles():
        g.set_champion(r, champ[r])
    tables = crossplay_tables(spec, champ)

    def run_tables():
        return [t.run(FIRST) for t in tables]

    def enqueue_tables():   # the launches of run() without its readback
        for t in tables:
            n = t.n_games
            t.status.zero_()
            L.call("coevo_mpe_reset_episodes", L._p(t.state), n, 0, n, t.rng, FIRST, t.episodes)
            for c in range((t.T + 2) // 3):
                t.enqueue_cycle(c, FIRST)
            L.call("coevo_mpe_rewards", L._p(t.state), n, L._p(t.rewards))
    variants = {"Gauntlet.run(): one launch for all env-cycles": (lambda: g.run(FIRST), lambda: g.enqueue(FIRST)),
                f"BaselineCrossPlay x {len(tables)}: four launches per env-cycle and table": (run_tables, enqueue_tables)}
    for fn, _ in variants.values():
        for _ in range(a.warmup):
            fn()
    ms = {k: ([], [], []) for k in variants}
    last = {}
    for _ in range(a.repeats):
        for k, (fn, enq) in variants.items():
            last[k], dev, host, e = measure(fn, enq)
            for lst, v in zip(ms[k], (dev, host, e)):
                lst.append(v)
    res, cps = last.values()
    want = np.concatenate([c.rewards.reshape(-1, E, 3) for c in cps])
    same = np.array_equal(res.rewards.view(np.uint64), np.ascontiguousarray(want).view(np.uint64)) and \
        np.array_equal(res.mean.view(np.uint64), np.ascontiguousarray(np.concatenate([c.payoff.reshape(-1, 3) for c in cps])).view(np.uint64))
    lines = ["", f"## 1. The reference table: {g.n_games} games, 25 env-cycles", "",
             "| route | device, ms | host incl. synchronise and readback, ms | host enqueue alone, ms |", "|---|---|---|---|"]
    for k, (dev, host, enq) in ms.items():
        lines.append(f"| {k} | {spread(dev)} | {spread(host)} | {spread(enq)} |")
        print(lines[-1], file=sys.stderr, flush=True)
    (d_new, h_new, _), (d_old, h_old, _) = ms.values()
    lines += ["", f"Device time, one launch against the per-cycle route: {verdict(d_new, d_old)}; host time: {verdict(h_new, h_old)}.  "
              f"The two routes' rewards and means are {'equal word for word' if same else 'NOT equal'}."]
    return lines, same


def forward_lines(a):
    D, net = 8, ppo("adversary_0")
    slab = torch.zeros(bl.mlp_stride(D), dtype=torch.float32, device="cuda")
    slab[:net.flat.size].copy_(torch.from_numpy(net.flat))
    lines = ["", "## 2. The policy net alone: one wave per row against one thread per row", "",
             "device events over 20 back-to-back launches of one width-8 net, tasks of at most 256 rows; us per launch", "",
             "| rows | coevo_mlp_forward_argmax_wave | coevo_mlp_forward_argmax | wave form against thread form |", "|---|---|---|---|"]
    for n in (1, 60, 4000, 80000):
        tasks = torch.tensor([(0, lo, min(256, n - lo), D) for lo in range(0, n, 256)], dtype=torch.int32, device="cuda")
        obs = (torch.rand(n, L.OBS_STRIDE, device="cuda") * 4 - 2).contiguous()
        acts = {k: torch.zeros(n, dtype=torch.int32, device="cuda") for k in ("wave", "thread")}
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        names = {"wave": "coevo_mlp_forward_argmax_wave", "thread": "coevo_mlp_forward_argmax"}

        def launch(k):
            L.call(names[k], L._p(slab), slab.numel(), L._p(tasks), len(tasks), L._p(obs), n, L._p(acts[k]), None, L._p(status))
        us = {k: [] for k in names}
        for k in names:
            for _ in range(5):
                launch(k)
        for _ in range(a.repeats):
            for k in names:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    launch(k)
                e1.record()
                torch.cuda.synchronize()
                us[k].append(e0.elapsed_time(e1) / 20 * 1e3)
        assert status.item() == 0 and torch.equal(acts["wave"], acts["thread"])
        lines.append(f"| {n} | {spread(us['wave'], '{:.1f}')} | {spread(us['thread'], '{:.1f}')} | {verdict(us['wave'], us['thread'])} |")
        print(lines[-1], file=sys.stderr, flush=True)
    return lines


class CrossPlayEveryGeneration:
    """what the trainer would have to do without the gauntlet: download the champions after a step and rebuild the tables"""

    def __init__(self, tr, spec):
        self.tr, self.spec, self.scores = tr, spec, []

    def step(self):
        self.tr.step()
        eng = self.tr.eng
        champ = {r: eng.download(r, "hof", eng.hof - 1, 1)[0] for r in ga.ROLES}
        self.scores.append([p for t in crossplay_tables(self.spec, champ) for p in t.run(self.spec.first_ordinal).payoff.reshape(-1, 3)])


def generation_lines(a):
    spec = reference_spec()
    steppers = []
    for name, kind in (("gauntlet off", None), ("gauntlet on (GATrainer(gauntlet=...))", "on"),
                       ("BaselineCrossPlay rebuilt every generation", "cp")):
        torch.manual_seed(0)
        args = Bag(algorithm="GA", generations=2 * (a.generations + a.warmup), population=200, hof_size=5, elites_number=2,
                   max_timesteps_per_episode=200, max_evaluation_steps=200, fitness_sharing=True, coevo_device_loop=False)
        env = initialize_env(args)
        tr = ga.GATrainer(env, args, rng="device_philox", env_mode="device", collect=False, gauntlet=spec if kind == "on" else None)
        steppers.append((name, CrossPlayEveryGeneration(tr, spec) if kind == "cp" else tr))
    times = {name: [] for name, _ in steppers}
    for _ in range(2):   # two rounds over the variants; within a round a variant keeps the chip (and its cache) to itself
        for name, st in steppers:
            for g in range(a.warmup + a.generations // 2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                st.step()
                torch.cuda.synchronize()
                if g >= a.warmup:
                    times[name].append((time.perf_counter() - t0) * 1e3)
    base = times[steppers[0][0]]
    lines = ["", "## 3. A host-driven float32 generation at the cfg 2 shape", "",
             f"pop 200, HoF 5, T 200, device_philox, coevo_device_loop off, collect off; two rounds over the variants, in each "
             f"{a.warmup} warm-up then {a.generations // 2} timed generations per variant; host clock around a step that ends in a "
             "device synchronise; median (min .. max) in ms.", "",
             "| variant | generation, ms | against gauntlet off, ms | generations/s | against gauntlet off |", "|---|---|---|---|---|"]
    for name, _ in steppers:
        med = float(np.median(times[name]))
        lines.append(f"| {name} | {spread(times[name], '{:.2f}')} | {med - float(np.median(base)):+.2f} | {1e3 / med:.1f} | "
                     f"{'-' if times[name] is base else verdict(times[name], base)} |")
        print(lines[-1], file=sys.stderr, flush=True)
    on, cp = steppers[1][1], steppers[2][1]
    on.finish()
    n = min(len(on.res.gauntlet), len(cp.scores))
    same = all(np.array_equal(np.array(on.res.gauntlet[g]).view(np.uint64), np.array(cp.scores[g]).view(np.uint64)) for g in range(n))
    lines += ["", f"The trainer's scores of the first {n} generations and the rebuilt tables' payoffs are "
              f"{'equal word for word' if same else 'NOT equal'}."]
    return lines, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--generations", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--table-only", action="store_true", help="section 1 alone (for a run under a kernel trace)")
    a = ap.parse_args()
    assert a.repeats >= 5 and a.warmup >= 1 and a.generations >= 4
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    lines = [f"# Baseline gauntlet: one launch per generation's score ({torch.cuda.get_device_name(0)})", "",
             f"warm-up {a.warmup}, then {a.repeats} alternating rounds per group; median (min .. max).  A speed-up is claimed only "
             "where the ranges are disjoint."]
    t_lines, ok = table_lines(a)
    lines += t_lines
    if not a.table_only:
        lines += forward_lines(a)
        g_lines, ok2 = generation_lines(a)
        lines += g_lines
        ok = ok and ok2
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    assert ok, "the one-launch route and the per-cycle route differ"


if __name__ == "__main__":
    main()
