#!/usr/bin/env python3
"""Cross-play over the paddle duel with a scripted seat (coevonet_amd.duel_crossplay): what the seat costs inside the env-step
launch, against the launches the library had before, and against the host loop.

    python tools/bench_duel_crossplay.py [--repeats 5] [--warmup 1] [--sample 24] [--out FILE.md]

1. The seat route: 8 float32 nets x {random, constant} x 10 episodes at limit 200 (160 games) through ``DuelCrossPlay``
   (coevo_dqn_out_duel_seat_step: three launches per two agent-steps), next to the SAME games played with the earlier launches
   only - coevo_baseline_actions + coevo_duel_step on the seat's step, coevo_dqn_out_duel_step on the net's (five launches per
   two agent-steps).  State words and returns are compared word for word.
2. The tracker table: 8 nets x ``TrackerSeat`` x 10 episodes at limit 200 through ``DuelCrossPlay``, next to the façade
   ``play_game`` loop with ``DuelTracker`` over a seeded sample of its games, scaled to the count; every sampled game's returns
   and points are compared with the table's.
3. The env launch alone at the tracker table's 80 games: coevo_dqn_out_duel_seat_step against coevo_dqn_out_duel_step, device events over 20
   back-to-back launches.

Protocol (one process): every variant is warmed up, then the variants of a group ALTERNATE for --repeats rounds, timed with
the host clock around work that ends in a device synchronise; medians with the min .. max spread.  A speed-up is claimed only
where the two ranges are disjoint."""
import argparse
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from coevonet_amd import atari_duel as ad   # noqa: E402
from coevonet_amd import baselines as bl   # noqa: E402
from coevonet_amd import duel_crossplay as dx   # noqa: E402
from coevonet_amd import game_logic as gl   # noqa: E402
from coevonet_amd import lib as L   # noqa: E402
from coevonet_amd.deepqn import DeepQN   # noqa: E402

FIRST, C, N_ACT, LIMIT, E = 1, 4, 6, 200, 10


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


class EarlierLaunches:
    """the games of a ``DuelCrossPlay`` with seats as second_0, enqueued with the launches that existed before the seat launch,
    over the same buffers: coevo_dqn_out_duel_step books the net's step, coevo_baseline_actions + plain coevo_duel_step book the
    seat's and render the net's next frame"""

    def __init__(self, cp, seats):
        self.cp, ro = cp, cp.ro
        assert ro.script_parity == 1
        n, B = ro.n_games, len(seats)
        g = np.arange(n)
        words = np.zeros((n, L.K_BL["COEVO_BL_SEAT_WORDS"]), dtype=np.int32)
        for i, b in enumerate(seats):
            games = np.nonzero((g // E) % B == i)[0]
            words[games] = bl._seat_words(games, games, b, 1)
        self.seats = torch.from_numpy(words).to("cuda")
        self.identity = torch.arange(n, dtype=torch.int32, device="cuda")
        self.seat_actions = torch.zeros(n, dtype=torch.int32, device="cuda")

    def enqueue(self, T):
        ro, lib, stream = self.cp.ro, L.load(), L._stream()
        n = ro.n_games
        head = (L._p(ro.dstate), L._p(ro.acc), n, L._p(ro.ordinal0), None, 0)
        tail = (ro.C, ro.n_actions, ro.env_seed, ro.points_to_win, ro.flags)
        for t in range(T + 1):
            net_next = t < T and (t & 1) == 0
            cur = (L._p(ro.rows), L._p(ro.frames)) if net_next else (None, None)
            if t == 0:
                L._check(lib.coevo_duel_step(*head, t, L._p(ro.limit), None, None, *cur, *tail, stream), "coevo_duel_step")
            elif (t - 1) & 1 == 0:   # the net's step t - 1: its output layer rides in the env-step launch
                L._check(lib.coevo_dqn_out_duel_step(*head, t, L._p(ro.limit), L._p(ro.rows), L._p(ro.actions), *cur, *tail,
                                                     L._p(ro.slab), L._p(ro.tasks), ro.n_tasks, n, L._p(ro.ws), L._p(ro.status),
                                                     stream), "coevo_dqn_out_duel_step")
            else:                    # the seat's step t - 1
                L._check(lib.coevo_baseline_actions(L._p(self.seats), n, L._p(ro.ordinal0), 0, n, (t - 2) // 2, ro.n_actions,
                                                    L._p(self.seat_actions), n, stream), "coevo_baseline_actions")
                L._check(lib.coevo_duel_step(*head, t, L._p(ro.limit), L._p(self.identity), L._p(self.seat_actions), *cur, *tail,
                                             stream), "coevo_duel_step")
            if net_next:
                ro._forward(lib, stream)

    def run(self, first):
        cp, ro = self.cp, self.cp.ro
        ro.status.zero_()
        ro.ordinal0.copy_(torch.from_numpy(int(first) + cp._episode))
        ro.set_limits(np.full(ro.n_games, cp.T, dtype=np.int32))
        self.enqueue(cp.T)
        torch.cuda.synchronize()
        L.raise_on_status(ro.status)
        cp._reduce(ro.acc, marg_c=False)   # (what DuelCrossPlay.run does behind its rollout: the reduction and the copies back)
        tables = [x.cpu().numpy() for x in (cp.payoff, *cp.marg[:2])]
        return ro.acc.cpu().numpy().copy(), ro.dstate.cpu().numpy().copy(), tables


def spread(t):
    return f"{np.median(t):.2f} ({t.min():.2f} .. {t.max():.2f})"


def verdict(a, b, what_a, what_b):
    if a.max() < b.min():
        return f"{what_a} is faster: the ranges are disjoint (median ratio {np.median(b) / np.median(a):.2f}x)."
    if b.max() < a.min():
        return f"{what_b} is faster: the ranges are disjoint (median ratio {np.median(a) / np.median(b):.2f}x)."
    return "The ranges overlap: no faster, no slower."


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sample", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 3, "at least 3 alternating rounds"
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    torch.manual_seed(1)
    nets = [DeepQN(C, N_ACT, "float32") for _ in range(8)]
    lines = [f"# Duel cross-play with scripted seats ({torch.cuda.get_device_name(0)})", "",
             f"warm-up {a.warmup}, then {a.repeats} alternating rounds per group; host clock around work that ends in a device "
             f"synchronise; median (min .. max).  8 float32 DeepQN nets as first_0, C = {C} / {N_ACT} actions, {E} episodes, limit "
             f"{LIMIT}, points_to_win 21.", ""]
    # ---- 1. the seat route against the earlier launches
    seats = [bl.RandomBaseline(0), bl.ConstantBaseline(3)]
    cp = dx.DuelCrossPlay(nets, seats, C, N_ACT, episodes=E, limit=LIMIT)
    old = EarlierLaunches(cp, seats)
    n = cp.ro.n_games
    for _ in range(a.warmup):
        cp.run(FIRST)
        old.run(FIRST)
    ms = {"seat": [], "old": []}
    for _ in range(a.repeats):
        res, t = timed(lambda: cp.run(FIRST))
        ms["seat"].append(t)
        new_words = (cp.ro.acc.cpu().numpy().copy(), cp.ro.dstate.cpu().numpy().copy())
        old_words, t = timed(lambda: old.run(FIRST))
        ms["old"].append(t)
    ms = {k: np.array(v) for k, v in ms.items()}
    same1 = all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(new_words, old_words[:2]))
    lines += [f"## 1. {n} games against {{random, constant}} seats", "", "| route | launches per two agent-steps | one run, ms | games/s |",
              "|---|---|---|---|",
              f"| seat launch (coevo_dqn_out_duel_seat_step) | 3 | {spread(ms['seat'])} | {n / np.median(ms['seat']) * 1e3:,.0f} |",
              f"| earlier launches (coevo_baseline_actions + coevo_duel_step + coevo_dqn_out_duel_step) | 5 | {spread(ms['old'])} | "
              f"{n / np.median(ms['old']) * 1e3:,.0f} |", "",
              verdict(ms["seat"], ms["old"], "The seat launch", "The earlier route"),
              f"State words and returns of the two routes are {'equal word for word' if same1 else 'NOT equal'}; "
              f"{int(res.points.sum())} points were scored in the table.", ""]
    del cp, old
    torch.cuda.empty_cache()
    # ---- 2. the tracker table against the play_game loop
    cp = dx.DuelCrossPlay(nets, [dx.TrackerSeat()], C, N_ACT, episodes=E, limit=LIMIT)
    n = cp.ro.n_games
    g = np.random.default_rng(5)
    sample = np.stack([g.integers(0, 8, a.sample), g.integers(0, E, a.sample)], axis=1)
    gl_args = SimpleNamespace(game="pong_v3", max_evaluation_steps=LIMIT, max_timesteps_per_episode=1)

    def play(i, e):
        env = ad.DuelAEC("pong_v3", channels=C)
        env.reset(seed=cp.ro.env_seed)
        env.n_resets = FIRST + int(e)
        r = gl.play_game(env=env, player1=nets[int(i)], player2=ad.DuelTracker(1), args=gl_args, eval=True)
        return (float(r[0]), float(r[1])), tuple(env.state.score)

    for _ in range(a.warmup):
        cp.run(FIRST)
        play(*sample[0])
    chunks = np.array_split(np.arange(len(sample)), a.repeats)
    t_roll, t_loop, same2 = [], [], True
    for chunk in chunks:
        res, t = timed(lambda: cp.run(FIRST))
        t_roll.append(t)
        got, t = timed(lambda: [play(*sample[i]) for i in chunk])
        t_loop.append(t / len(chunk) * n)
        for i, (r, pts) in zip(chunk, got):
            a_, e_ = sample[i]
            same2 &= tuple(res.rewards[a_, 0, e_]) == r and tuple(res.points[a_, 0, e_]) == pts
    t_roll, t_loop = np.array(t_roll), np.array(t_loop)
    lines += [f"## 2. {n} games against the tracker", "", "| route | one table, ms | games/s |", "|---|---|---|",
              f"| DuelCrossPlay, TrackerSeat in the env-step launch | {spread(t_roll)} | {n / np.median(t_roll) * 1e3:,.0f} |",
              f"| play_game loop with DuelTracker ({a.sample} sampled games, scaled to {n}) | {spread(t_loop)} | "
              f"{n / np.median(t_loop) * 1e3:,.0f} |", "",
              verdict(t_roll, t_loop, "The device table", "The host loop"),
              f"Returns and points of every sampled game are {'equal' if same2 else 'NOT equal'} to the table's; the nets conceded "
              f"{int(res.points[..., 1].sum())} points and scored {int(res.points[..., 0].sum())}.", ""]
    # ---- 3. the env launch alone
    ro, lib, stream = cp.ro, L.load(), L._stream()
    cp.run(FIRST)   # leaves a workspace and frames behind
    n = ro.n_games
    lib.coevo_duel_step(L._p(ro.dstate), L._p(ro.acc), n, L._p(ro.ordinal0), None, 0, 0, L._p(ro.limit), None, None, None, None,
                        ro.C, ro.n_actions, ro.env_seed, ro.points_to_win, ro.flags, stream)
    fresh = ro.dstate.clone()   # every game just reset: each burst starts from here
    head = (L._p(ro.dstate), L._p(ro.acc), n, L._p(ro.ordinal0), None, 0, 1, L._p(ro.limit))
    tail = (ro.C, ro.n_actions, ro.env_seed, ro.points_to_win, ro.flags, L._p(ro.slab), L._p(ro.tasks), ro.n_tasks, n, L._p(ro.ws),
            L._p(ro.status), stream)

    def seat_launch():
        ro.dstate.copy_(fresh)
        return lambda: L._check(lib.coevo_dqn_out_duel_seat_step(*head, L._p(ro.seats), 1, L._p(ro.rows), L._p(ro.actions),
                                                                 L._p(ro.script_actions), L._p(ro.rows), L._p(ro.frames), *tail),
                                "coevo_dqn_out_duel_seat_step")

    def plain_launch():
        ro.dstate.copy_(fresh)
        return lambda: L._check(lib.coevo_dqn_out_duel_step(*head, L._p(ro.rows), L._p(ro.actions), L._p(ro.rows), L._p(ro.frames),
                                                            *tail), "coevo_dqn_out_duel_step")
    us = {"seat": [], "plain": []}
    for _ in range(a.repeats + a.warmup):
        for k, make in (("seat", seat_launch), ("plain", plain_launch)):
            fn = make()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) / 20 * 1e3)
    us = {k: np.array(v[a.warmup:]) for k, v in us.items()}
    lines += [f"## 3. the env launch alone, {n} games", "",
              "Device events over 20 back-to-back launches at t = 1 on live games (every launch computes the output row, books and "
              "renders one frame per game; the seat form also plays and books the seat's step).", "",
              "| launch | us per launch |", "|---|---|",
              f"| coevo_dqn_out_duel_seat_step | {spread(us['seat'])} |", f"| coevo_dqn_out_duel_step | {spread(us['plain'])} |", "",
              verdict(us["seat"], us["plain"], "The seat form", "The plain form")
              + "  (One seat launch does the env side of two agent-steps, one plain launch of one.)"]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    assert same1, "the seat route and the earlier launches differ"
    assert same2, "a sampled play_game differs from the table's game"


if __name__ == "__main__":
    main()
