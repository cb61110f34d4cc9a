"""Baseline opponents on the GPU, equalities of bits only: coevo_baseline_actions against scripted_action, the PPO policy
kernels against the C checker (tests/checker16/mlp_checker.c), BaselineCrossPlay / DQNBaselineCrossPlay game by game against
host loops over the oracle's own pieces (tests/baseline_cases.py), the all-net BaselineCrossPlay against CrossPlay word for
word, runs repeated on one object against fresh objects, the faults' ValueError, and test_agents with an opponent."""
import functools

import numpy as np
import pytest
import torch

from coevonet_amd import baselines as bl
from coevonet_amd import crossplay as xp
from coevonet_amd import game_logic as gl
from coevonet_amd import io_utils
from coevonet_amd import lib as L
from coevonet_amd.atari_synthetic import SYNTH_SEED
from coevonet_amd.population import ROLES, ROLES2
from oracle import ref_port as rp
from tests import baseline_cases as bc
from tests import crossplay_cases as cc
from tests.test_crossplay_gpu import assert_result, dqn_nets, fc_nets, mpe_checkpoints, results_equal, same_bits
from tests.util import Bag

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE = L.K_BL["COEVO_MLP_ROW_TILE"]
SENTINEL = -77


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def call(name, *args):
    """L.call over tensors and numpy arrays: every array goes to the device and lives until the launch is enqueued (two
    temporaries in one argument list would otherwise share one freed block)"""
    held = [dev(a) if isinstance(a, np.ndarray) else a for a in args]
    L.call(name, *[L._p(h) if torch.is_tensor(h) else h for h in held])


# ------------------------------------------------------------------------------------------- 1. coevo_baseline_actions
ORDINALS = (0, 2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1)


@pytest.mark.parametrize("n_seats", [1, 63, 64, 65])
def test_baseline_actions_equal_the_statement(n_seats):
    g = np.random.default_rng(n_seats)
    n_rows = 3 * n_seats + 5
    rows = g.permutation(n_rows)[:n_seats]                      # scattered, every row at most once
    games = np.arange(n_seats) % len(ORDINALS)
    kinds = (np.arange(n_seats) // 2) % 3
    seeds = [0 if i % 2 else 2 ** 64 - 1 for i in range(n_seats)]
    slots = g.integers(0, 3, n_seats)
    ordinals = dev(np.array(ORDINALS, dtype=np.uint64).view(np.int64))
    for n_actions in (1, 5, 6, 18, 32):
        args = [int(g.integers(0, n_actions)) if kinds[i] == bl.CONSTANT else int(g.integers(0, 2 ** 31)) for i in range(n_seats)]
        words = np.zeros((n_seats, 8), dtype=np.int64)
        words[:, 0], words[:, 1], words[:, 2], words[:, 3], words[:, 6] = games, rows, kinds, args, slots
        words[:, 4], words[:, 5] = [s & 0xFFFFFFFF for s in seeds], [s >> 32 for s in seeds]
        seats = dev(words.astype(np.uint32).view(np.int32))
        for k in (0, 24, 2 ** 31 - 1):
            for add in (0, 2 ** 63 + 5):
                actions = torch.full((n_rows,), SENTINEL, dtype=torch.int32, device=DEV)
                L.call("coevo_baseline_actions", L._p(seats), n_seats, L._p(ordinals), add, len(ORDINALS), k, n_actions,
                       L._p(actions), n_rows)
                got = actions.cpu().numpy()
                want = np.full(n_rows, SENTINEL, dtype=np.int32)
                for i in range(n_seats):
                    want[rows[i]] = bl.scripted_action(int(kinds[i]), args[i], seeds[i], (ORDINALS[games[i]] + add) % 2 ** 64,
                                                       int(slots[i]), k, n_actions)
                assert np.array_equal(got, want), (n_actions, k, add)
                assert ((want[rows] >= 0) & (want[rows] < n_actions)).all()


def test_baseline_actions_skip_what_they_cannot_serve():
    """a seat outside the tables, of no kind, or a constant outside the action range writes nothing"""
    words = np.zeros((6, 8), dtype=np.int32)
    words[:, 1] = np.arange(6)
    words[0, 0] = 2                                   # game 2 of 2
    words[1, 1] = 9                                   # row 9 of 8
    words[2, 2] = 3                                   # no such kind
    words[3, 2:4] = (bl.CONSTANT, 5)                  # constant 5 of 5 actions
    words[4, 2:4] = (bl.PERIODIC, -1)
    words[5, 2:4] = (bl.CONSTANT, 4)                  # the one that is served
    actions = torch.full((8,), SENTINEL, dtype=torch.int32, device=DEV)
    call("coevo_baseline_actions", words, 6, np.zeros(2, dtype=np.int64), 0, 2, 0, 5, actions, 8)
    want = np.full(8, SENTINEL, dtype=np.int32)
    want[5] = 4
    assert np.array_equal(actions.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------- 2. the policy kernels
def mlp_slab(nets):
    """[(flat, D)] -> (device slab, offsets)"""
    offs, off = [], 0
    for flat, D in nets:
        offs.append(off)
        off += bl.mlp_stride(D)
    host = np.zeros(off, dtype=np.float32)
    for (flat, D), o in zip(nets, offs):
        host[o:o + flat.size] = flat
    return dev(host), offs


def tile_tasks(nets, offs, counts):
    """the rows of net i are counts[i] consecutive rows, cut into tasks of at most TILE rows"""
    tasks, first = [], 0
    for (flat, D), o, n in zip(nets, offs, counts):
        for lo in range(0, n, TILE):
            tasks.append((o, first + lo, min(TILE, n - lo), D))
        first += n
    return np.array(tasks, dtype=np.int32)


def device_forward(nets, counts, obs):
    slab, offs = mlp_slab(nets)
    tasks = tile_tasks(nets, offs, counts)
    n = int(sum(counts))
    assert obs.shape == (n, L.OBS_STRIDE)
    actions = torch.full((n,), SENTINEL, dtype=torch.int32, device=DEV)
    logits = torch.full((n, L.LOGIT_STRIDE), 7.0, dtype=torch.float32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    call("coevo_mlp_forward_argmax", slab, slab.numel(), tasks, len(tasks), obs, n, actions, logits, status)
    lo = logits.cpu().numpy()
    assert (lo[:, bc.NACT:] == 7.0).all()          # the padding floats of a logits row are not written
    return actions.cpu().numpy(), lo[:, :bc.NACT], int(status.item())


def checker_forward(nets, counts, obs):
    a, lo, st, first = [], [], 0, 0
    for (flat, D), n in zip(nets, counts):
        ai, li, si = bc.mlp_rows(flat, D, obs[first:first + n])
        a.append(ai)
        lo.append(li)
        st |= int(np.bitwise_or.reduce(si)) if n else 0
        first += n
    return np.concatenate(a), np.concatenate(lo), st


def same_floats(a, b):
    """bit equality, any NaN equal to any NaN (a NaN's payload is not part of the contract)"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | nan).all())


def fixture_nets():
    return [(bc.fixture()[r]["flat"], bc.ROLE_D[r]) for r in bc.ROLES]


@pytest.mark.parametrize("n_rows", [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_forward_equals_the_checker_around_the_row_tile(n_rows):
    for flat, D in (fixture_nets()[0], fixture_nets()[2]):
        obs = bc.uniform_obs(n_rows, seed=n_rows + D)
        got = device_forward([(flat, D)], [n_rows], obs)
        want = checker_forward([(flat, D)], [n_rows], obs)
        assert got[2] == want[2] == 0
        assert np.array_equal(got[0], want[0]) and same_floats(got[1], want[1])
        assert len(set(got[0].tolist())) > 1 or n_rows == 1


def test_forward_three_fixture_nets_and_both_widths_in_one_call():
    nets, counts = fixture_nets() + [(bc.random_net(8, 1), 8), (bc.random_net(10, 2), 10)], [300, 7, TILE, 1, 65]
    obs = bc.uniform_obs(sum(counts), seed=9)
    got, want = device_forward(nets, counts, obs), checker_forward(nets, counts, obs)
    assert got[2] == want[2] == 0 and np.array_equal(got[0], want[0]) and same_floats(got[1], want[1])
    # the stored fixture rows: the device plays what torch played wherever the margin allows (all of them, as recorded)
    for role in bc.ROLES:
        f, D = bc.fixture()[role], bc.ROLE_D[role]
        o = np.zeros((len(f["obs"]), L.OBS_STRIDE), dtype=np.float32)
        o[:, :D] = f["obs"]
        a, lo, st = device_forward([(f["flat"], D)], [len(o)], o)
        top = np.sort(lo.astype(np.float64), axis=1)
        clear = top[:, -1] - top[:, -2] >= 8 * float(f["max_dlogit"])
        assert st == 0 and (~clear).sum() <= 0.01 * len(clear) and np.array_equal(a[clear], f["actions"][clear])


@pytest.mark.parametrize("D", [8, 10])
def test_forward_crafted_nets(D):
    n = 70
    obs = bc.uniform_obs(4 * n, seed=D)
    nets = [(bc.crafted(name, D), D) for name in ("all_zero", "tie", "dead", "neg_zero")]
    a, lo, st = device_forward(nets, [n] * 4, obs)
    want = checker_forward(nets, [n] * 4, obs)
    assert st == want[2] == 0 and np.array_equal(a, want[0]) and same_floats(lo, want[1])
    assert not a[:n].any() and not lo[:n].view(np.uint32).any()                                    # all zero: +0 logits, action 0
    assert (a[n:2 * n] == 2).all() and np.array_equal(lo[n:2 * n], np.tile(np.float32([0, 0, 1, 0, 1]), (n, 1)))   # the tie
    assert np.array_equal(lo[2 * n:3 * n], np.tile(np.float32([0.25, -1.5, 0.75, 3.0, 0.0]), (n, 1)))   # the head's bias
    assert (a[2 * n:3 * n] == 3).all() and len(set(a[3 * n:].tolist())) > 1


@pytest.mark.parametrize("fault", ["fc1", "fc2", "out", "input"])
def test_forward_faults_raise_their_bit_and_play_zero(fault):
    D, n = 10, 40
    good = bc.random_net(D, 5)
    bad = good.copy()
    obs = bc.uniform_obs(3 * n, seed=4)
    if fault == "input":
        obs[n + 3, 2] = np.inf
    else:
        view, at = {"fc1": (0, (3, 2)), "fc2": (2, (9, 9)), "out": (4, (4, 0))}[fault]
        bc.parts(D, bad)[1][view][at] = np.nan
    nets = [(good, D), (bad, D), (good, D)]
    a, lo, st = device_forward(nets, [n] * 3, obs)
    wa, wlo, wst = checker_forward(nets, [n] * 3, obs)
    assert st == wst and st & bc.ST[fault]
    assert np.array_equal(a, wa) and same_floats(lo, wlo)
    hit = [n + 3] if fault == "input" else list(range(n, 2 * n))
    assert not a[hit].any()
    rest = np.setdiff1d(np.arange(3 * n), hit)
    clean = checker_forward([(good, D)], [3 * n], np.where(np.isinf(obs), 0, obs))        # the other rows are unharmed
    assert np.array_equal(a[rest], clean[0][rest]) and same_floats(lo[rest], clean[1][rest]) and len(set(a[rest].tolist())) > 1


def test_forward_skips_a_bad_task():
    flat = bc.random_net(8, 3)
    slab, _ = mlp_slab([(flat, 8)])
    obs = dev(bc.uniform_obs(4, seed=1))
    for task in ((0, 0, 4, 9), (0, 0, 0, 8), (0, 0, TILE + 1, 8), (0, 2, 4, 8), (2, 0, 4, 8), (4, 0, 4, 8), (-4, 0, 4, 8), (0, -1, 4, 8)):
        actions = torch.full((4,), SENTINEL, dtype=torch.int32, device=DEV)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        call("coevo_mlp_forward_argmax", slab, slab.numel(), np.array([task], dtype=np.int32), 1, obs, 4, actions, None, status)
        assert status.item() == L.K["COEVO_ST_BAD_TASK"] and (actions.cpu().numpy() == SENTINEL).all(), task


def test_policy_cycle_equals_observe_and_the_obs_fed_twin():
    n_games = 130
    nets = [fixture_nets()[2], fixture_nets()[0], fixture_nets()[1]]           # by slot: adversary_0, agent_0, agent_1
    slab, offs = mlp_slab(nets)
    st = torch.zeros(L.MPE_STATE_DOUBLES, n_games, dtype=torch.float64, device=DEV)
    L.call("coevo_mpe_reset", L._p(st), n_games, 0, n_games, L.PCG64State.from_seed(rp.ENV_SEED), 5)
    n_rows = 3 * n_games + 4
    rows = np.random.default_rng(2).permutation(n_rows)[:3 * n_games]
    seat_game = np.tile(np.arange(n_games), 3)
    seat_slot = np.repeat(np.arange(3), n_games)
    seats = np.stack([seat_game, rows, seat_slot, np.zeros_like(rows)], axis=1).astype(np.int32)
    tasks = tile_tasks(nets, offs, [n_games] * 3)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    actions = torch.full((n_rows,), SENTINEL, dtype=torch.int32, device=DEV)
    logits = torch.zeros(3 * n_games, L.LOGIT_STRIDE, dtype=torch.float32, device=DEV)
    call("coevo_mpe_mlp_policy_cycle", slab, slab.numel(), tasks, len(tasks), seats, 3 * n_games, st, n_games, actions, n_rows,
         logits, status)
    obs = torch.zeros(3 * n_games, L.OBS_STRIDE, dtype=torch.float32, device=DEV)
    call("coevo_mpe_observe", st, n_games, seat_game.astype(np.int32), seat_slot.astype(np.int32), 3 * n_games, obs)
    twin_a = torch.zeros(3 * n_games, dtype=torch.int32, device=DEV)
    twin_l = torch.zeros(3 * n_games, L.LOGIT_STRIDE, dtype=torch.float32, device=DEV)
    call("coevo_mlp_forward_argmax", slab, slab.numel(), tasks, len(tasks), obs, 3 * n_games, twin_a, twin_l, status)
    assert status.item() == 0
    got = actions.cpu().numpy()
    assert np.array_equal(got[rows], twin_a.cpu().numpy()) and same_floats(logits.cpu().numpy(), twin_l.cpu().numpy())
    assert (np.delete(got, rows) == SENTINEL).all() and len(set(got[rows].tolist())) > 1
    want = checker_forward(nets, [n_games] * 3, obs.cpu().numpy())
    assert np.array_equal(got[rows], want[0])
    # a seat whose width is not its task's is skipped with COEVO_ST_BAD_TASK
    seats[0, 2] = 1
    call("coevo_mpe_mlp_policy_cycle", slab, slab.numel(), tasks, len(tasks), seats, 3 * n_games, st, n_games, actions, n_rows, None,
         status)
    assert status.item() == L.K["COEVO_ST_BAD_TASK"]


# --------------------------------------------------------------------------------------------------- 3. BaselineCrossPlay
@functools.lru_cache(maxsize=None)
def mixed_lists():
    """dims (2, 2, 3): every role's list holds an evolved net, and every kind of baseline sits somewhere"""
    nets = fc_nets(2, 2, 3)
    return {"agent_0": [nets["agent_0"][0], bc.fixture_baseline("agent_0")],
            "agent_1": [bl.RandomBaseline(3), nets["agent_1"][1]],
            "adversary_0": [nets["adversary_0"][0], bl.PeriodicBaseline(2), bl.ConstantBaseline(3)]}


def make_cp(lists, **kw):
    return bl.BaselineCrossPlay(lists["agent_0"], lists["agent_1"], lists["adversary_0"], **kw)


@pytest.mark.parametrize("limit", [None, 7, 1])
def test_baseline_crossplay_equals_the_host_loop_game_by_game(limit):
    lists, dims, E = mixed_lists(), (2, 2, 3), 2
    cp = make_cp(lists, episodes=E, limit=limit)
    assert cp.n_mlp_seats == 12 and cp.n_script == 12 + 8 + 8 and cp.n_rows == 72
    for first in (1, 2 ** 40):
        want = bc.crossplay_rewards(lists, E, first, limit)
        assert_result(cp.run(first), want, dims, E)          # rewards, payoff and marginals (tests/crossplay_cases.py)
        assert want.any() or limit == 1


def test_two_adversary_policies_and_a_random_pair():
    """the PPO adversary in the table, two random seats in one game, an all-baseline trio beside evolved nets"""
    nets = fc_nets(2, 2, 3)
    lists = {"agent_0": [bl.RandomBaseline(1), nets["agent_0"][1]], "agent_1": [bl.RandomBaseline(1), bc.fixture_baseline("agent_1")],
             "adversary_0": [bc.fixture_baseline("adversary_0"), nets["adversary_0"][2]]}
    cp = make_cp(lists, episodes=3, limit=31)
    assert_result(cp.run(6), bc.crossplay_rewards(lists, 3, 6, 31), (2, 2, 2), 3)


# ------------------------------------------------------------------------------------------------------ 4. route equality
def test_all_net_baseline_crossplay_equals_crossplay_word_for_word():
    nets = fc_nets(3, 1, 2)         # agent_0: per-individual tasks, agent_1: shared-opponent tasks
    for limit in (None, 31):
        a = bl.BaselineCrossPlay(nets["agent_0"], nets["agent_1"], nets["adversary_0"], episodes=2, limit=limit)
        b = xp.CrossPlay(nets["agent_0"], nets["agent_1"], nets["adversary_0"], episodes=2, limit=limit)
        assert len(a.heavy_np) and len(a.light_np) and not a.n_mlp_tasks and not a.n_script
        for first in (1, 6):
            assert results_equal(a.run(first), b.run(first))


# --------------------------------------------------------------------------------------------------- 5. re-use and faults
def test_runs_and_uploads_on_one_object_equal_fresh_objects():
    lists = mixed_lists()
    other = fc_nets(2, 2, 3, seed=50)
    cp = make_cp(lists, episodes=2, limit=31)
    first = cp.run(1)
    assert results_equal(cp.run(6), make_cp(lists, episodes=2, limit=31).run(6))
    assert results_equal(cp.run(1), first)
    cp.upload("agent_1", 1, other["agent_1"][0])
    cp.upload("agent_0", 1, bc.fixture()["agent_1"]["flat"])          # the other width-10 policy into agent_0's policy seat
    swapped = {**lists, "agent_1": [lists["agent_1"][0], other["agent_1"][0]],
               "agent_0": [lists["agent_0"][0], bc.fixture_baseline("agent_1")]}
    after = cp.run(6)
    assert results_equal(after, make_cp(swapped, episodes=2, limit=31).run(6))
    assert not results_equal(after, make_cp(lists, episodes=2, limit=31).run(6))
    for bad in (lambda: cp.upload("agent_1", 0, other["agent_1"][0]),            # a scripted seat has no weights
                lambda: cp.upload("agent_0", 1, bc.fixture()["adversary_0"]["flat"]),
                lambda: cp.upload("agent_0", 0, other["adversary_0"][0]), lambda: cp.upload("agent_0", 2, other["agent_0"][0]),
                lambda: cp.upload("first_0", 0, other["agent_1"][0])):
        with pytest.raises(ValueError):
            bad()


def test_a_nan_net_and_a_nan_policy_raise_play_games_value_error():
    lists = mixed_lists()
    bad_fc = lists["agent_0"][0].copy()
    bad_fc[100] = np.nan
    with pytest.raises(ValueError, match="NaN") as fc:
        make_cp({**lists, "agent_0": [bad_fc, lists["agent_0"][1]]}, episodes=2, limit=7).run(1)
    bad_mlp = bc.fixture()["agent_0"]["flat"].copy()
    bad_mlp[3] = np.nan
    cp = make_cp({**lists, "agent_0": [lists["agent_0"][0], bl.MLPBaseline(bad_mlp, 10)]}, episodes=2, limit=7)
    with pytest.raises(ValueError, match="after fc1") as mlp:
        cp.run(1)
    assert "Warning" in str(fc.value) and "Warning" in str(mlp.value)
    cp.upload("agent_0", 1, bc.fixture()["agent_0"]["flat"])         # repaired: the status word does not stick
    assert_result(cp.run(1), bc.crossplay_rewards(lists, 2, 1, 7), (2, 2, 3), 2)


# ------------------------------------------------------------------------------------------------ 6. DQNBaselineCrossPlay
def test_dqn_baseline_crossplay_equals_the_host_loop_on_both_sides():
    C, n, E, first, limit = 4, 6, 2, 3, 7
    nets = list(dqn_nets(C, n, 4, False)[:2])
    scripted = [bl.RandomBaseline(9), bl.PeriodicBaseline(4), bl.ConstantBaseline(1)]
    for a, b in ((nets, scripted), (scripted, nets)):
        want = bc.dqn_crossplay_rewards(a, b, C, n, E, first, limit, SYNTH_SEED)
        cp = bl.DQNBaselineCrossPlay(a, b, C, n, episodes=E, limit=limit)
        assert_result(cp.run(first), want, (len(a), len(b), 1), E, roles=ROLES2)
        assert want.any()
    again = cp.run(first + 5)                     # the object is reusable, and the tiled fc1 layout plays the same words
    tiled = bl.DQNBaselineCrossPlay(scripted, nets, C, n, episodes=E, limit=limit, fc1_layout="tiled").run(first + 5)
    assert results_equal(again, tiled)


# ------------------------------------------------------------------------------------------------------- 7. test_agents
def test_test_agents_against_a_random_opponent_atari(tmp_path):
    args = Bag(algorithm="GA", game="pong_v3", max_evaluation_steps=6, play_against_yourself=False, test=True)
    env = gl.initialize_env(args)
    torch.manual_seed(8)
    agent = gl.create_agent(env, args)
    agent.mutate(0.02)
    path = str(tmp_path / "hof.pth")
    io_utils.save_model([agent], path)
    for attr in ("GA_hof_to_test_agent_0", "GA_hof_to_test_agent_1", "GA_hof_to_test_adversary"):
        setattr(args, attr, path)
    env.reset()
    start = env.n_resets
    opponent = bl.RandomBaseline()
    got = xp.test_agents(env, args, episodes=10, opponent=opponent)
    want = bc.dqn_crossplay_rewards([agent.model.flat()], [opponent], env.C, env.n_actions, 10, start, 6, env.seed_value)
    assert same_bits(got, cc.reduce_ref(want, 1, 1, 1, 10)[0][0, :2]) and isinstance(got, tuple) and len(got) == 2
    assert env.n_resets == start + 10 and want.any()


def test_test_agents_against_the_ppo_adversary_mpe(tmp_path):
    args, agents = mpe_checkpoints(tmp_path, "float32")
    env = gl.initialize_env(args)
    for _ in range(3):
        env.reset()
    start = env.n_resets
    opponent = {"adversary_0": bc.fixture_baseline("adversary_0")}
    got = xp.test_agents(env, args, episodes=10, opponent=opponent)
    lists = {"agent_0": [agents["agent_0"][-1].model.flat()], "agent_1": [agents["agent_1"][-1].model.flat()],
             "adversary_0": [opponent["adversary_0"]]}
    want = bc.crossplay_rewards(lists, 10, start, 31, env.max_cycles, env.seed_value)
    assert same_bits(got, cc.reduce_ref(want, 1, 1, 1, 10)[0][0]) and env.n_resets == start + 10 and want.any()
