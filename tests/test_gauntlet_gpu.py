"""The baseline gauntlet on the GPU, equalities of bits only.  The yardsticks are what existed before it: BaselineCrossPlay,
coevo_mlp_forward_argmax and its C checker, coevo_mpe_observe / coevo_fc_forward_argmax / coevo_baseline_actions /
coevo_mpe_step run in sequence, and the host loop of tests/baseline_cases.py.  The kernels under test are never their own
reference."""
import functools
import json

import numpy as np
import pytest
import torch

from coevonet_amd import baselines as bl
from coevonet_amd import gauntlet as gt
from coevonet_amd import genetic_algorithm as ga
from coevonet_amd import lib as L
from coevonet_amd.game_logic import initialize_env
from oracle import ref_port as rp
from tests import baseline_cases as bc
from tests import gauntlet_cases as gc
from tests.test_baselines_gpu import (SENTINEL, call, checker_forward, dev, fixture_nets, make_cp, mixed_lists, mlp_slab,
                                      same_floats)
from tests.test_crossplay_gpu import same_bits
from tests.util import Bag, sha

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAD_TASK = L.K["COEVO_ST_BAD_TASK"]
GUARD = 64          # guard words in front of and behind every buffer a kernel under test writes


class Guarded:
    """a device buffer of n words between two runs of GUARD sentinel words"""

    def __init__(self, n, dtype, fill, guard):
        self.full = torch.full((n + 2 * GUARD,), guard, dtype=dtype, device=DEV)
        self.t = self.full[GUARD:GUARD + n]
        self.t.fill_(fill)
        self.guard = self.full.clone()
        self.guard[GUARD:GUARD + n] = 0

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        now = self.full.clone()
        now[GUARD:GUARD + self.t.numel()] = 0
        return bool((now.view(torch.uint8) == self.guard.view(torch.uint8)).all())


# ------------------------------------------------------------------------------------------ 1. the wave-form PPO forward
def forward_both(nets, counts, obs, with_logits=True):
    """coevo_mlp_forward_argmax_wave and coevo_mlp_forward_argmax on the same tasks: one task per net (counts <= 256) ->
    ((actions, logits, status) of the wave form, of the thread form); buffers sentinel-filled, the words outside checked"""
    slab, offs = mlp_slab(nets)
    tasks, first = [], 0
    for (flat, D), o, n in zip(nets, offs, counts):
        tasks.append((o, first, n, D))
        first += n
    n = int(sum(counts))
    tasks_dev, obs_dev = dev(np.array(tasks, dtype=np.int32)), dev(obs)      # (held: two temporaries would share one freed block)
    out = []
    for name in ("coevo_mlp_forward_argmax_wave", "coevo_mlp_forward_argmax"):
        actions = Guarded(n, torch.int32, SENTINEL, -5)
        logits = Guarded(n * L.LOGIT_STRIDE, torch.float32, 7.0, -9.0)
        status = Guarded(1, torch.int32, 0, -5)
        L.call(name, L._p(slab), slab.numel(), L._p(tasks_dev), len(tasks), L._p(obs_dev), n, actions.ptr(),
               logits.ptr() if with_logits else None, status.ptr())
        lo = logits.t.cpu().numpy().reshape(n, L.LOGIT_STRIDE)
        assert (lo[:, bc.NACT:] == 7.0).all() and (with_logits or (lo == 7.0).all())    # the padding floats are not written
        assert actions.intact() and logits.intact() and status.intact()
        out.append((actions.t.cpu().numpy(), lo[:, :bc.NACT], int(status.t.item())))
    return out


@pytest.mark.parametrize("n_rows", [1, 3, 4, 5, 9])
def test_wave_forward_equals_the_thread_form_and_the_checker_around_four_rows(n_rows):
    """five nets of both widths in one call, n_rows each: the edges of four rows per pass"""
    nets = fixture_nets() + [(bc.random_net(8, 1), 8), (bc.random_net(10, 2), 10)]
    counts = [n_rows] * 5
    obs = bc.uniform_obs(sum(counts), seed=n_rows)
    wave, thread = forward_both(nets, counts, obs)
    want = checker_forward(nets, counts, obs)
    assert wave[2] == thread[2] == want[2] == 0
    assert np.array_equal(wave[0], thread[0]) and np.array_equal(wave[0], want[0])
    assert same_floats(wave[1], thread[1]) and same_floats(wave[1], want[1])
    assert np.array_equal(forward_both(nets, counts, obs, with_logits=False)[0][0], want[0])


@pytest.mark.parametrize("D", [8, 10])
def test_wave_forward_crafted_nets_and_faults(D):
    n = 9
    names = ("all_zero", "tie", "dead", "neg_zero")
    nets = [(bc.crafted(name, D), D) for name in names]
    obs = bc.uniform_obs(4 * n, seed=D)
    wave, thread = forward_both(nets, [n] * 4, obs)
    want = checker_forward(nets, [n] * 4, obs)
    assert wave[2] == thread[2] == want[2] == 0 and np.array_equal(wave[0], want[0]) and same_floats(wave[1], want[1])
    assert same_floats(wave[1], thread[1])
    assert not wave[0][:n].any() and not wave[1][:n].view(np.uint32).any()                 # all zero: +0 logits, action 0
    assert (wave[0][n:2 * n] == 2).all() and (wave[0][2 * n:3 * n] == 3).all()              # the tie's first maximum; the bias
    good = bc.random_net(D, 5)
    for fault, view, at in (("fc1", 0, (3, 2)), ("fc2", 2, (9, 9)), ("out", 4, (4, 0)), ("input", None, None)):
        bad, o = good.copy(), bc.uniform_obs(3 * n, seed=4)
        if fault == "input":
            o[n + 3, 2] = np.inf
        else:
            bc.parts(D, bad)[1][view][at] = np.nan
        nets = [(good, D), (bad, D), (good, D)]
        wave, thread = forward_both(nets, [n] * 3, o)
        want = checker_forward(nets, [n] * 3, o)
        assert wave[2] == thread[2] == want[2] and wave[2] & bc.ST[fault], fault
        assert np.array_equal(wave[0], want[0]) and same_floats(wave[1], want[1]) and same_floats(wave[1], thread[1]), fault
        assert not wave[0][[n + 3] if fault == "input" else list(range(n, 2 * n))].any()


def test_wave_forward_plays_the_fixture_rows_and_skips_a_bad_task():
    for role in bc.ROLES:
        f, D = bc.fixture()[role], bc.ROLE_D[role]
        o = np.zeros((len(f["obs"]), L.OBS_STRIDE), dtype=np.float32)
        o[:, :D] = f["obs"]
        wave, thread = forward_both([(f["flat"], D)], [len(o)], o)
        top = np.sort(wave[1].astype(np.float64), axis=1)
        clear = top[:, -1] - top[:, -2] >= 8 * float(f["max_dlogit"])      # the margin rule of the thread form's test
        assert wave[2] == 0 and (~clear).sum() <= 0.01 * len(clear) and np.array_equal(wave[0][clear], f["actions"][clear])
        assert np.array_equal(wave[0], thread[0]) and same_floats(wave[1], thread[1])
    slab, _ = mlp_slab([(bc.random_net(8, 3), 8)])
    obs = dev(bc.uniform_obs(4, seed=1))
    for task in ((0, 0, 4, 9), (0, 0, 0, 8), (0, 0, 257, 8), (0, 2, 4, 8), (2, 0, 4, 8), (4, 0, 4, 8), (-4, 0, 4, 8), (0, -1, 4, 8)):
        actions = torch.full((4,), SENTINEL, dtype=torch.int32, device=DEV)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        call("coevo_mlp_forward_argmax_wave", slab, slab.numel(), np.array([task], dtype=np.int32), 1, obs, 4, actions, None, status)
        assert status.item() == BAD_TASK and (actions.cpu().numpy() == SENTINEL).all(), task


# ------------------------------------------------------------------------------------------------ the per-cycle reference
@functools.lru_cache(maxsize=None)
def seven():
    """the seven-match table with every kind in every slot as a Gauntlet (its slabs and game words) - never run as one"""
    matches, kinds = gc.every_kind_matches()
    return gt.Gauntlet(matches, episodes=1), kinds


ORDINALS = np.array([2 ** 63 - 1, 0, 2 ** 32 - 1, 2 ** 32, 5, 2 ** 40, 1], dtype=np.int64)


def start_state(n):
    """n games after their reset and one cycle of constant actions: positions and velocities that are not zero"""
    st = torch.zeros(L.MPE_STATE_DOUBLES, n, dtype=torch.float64, device=DEV)
    L.call("coevo_mpe_reset", L._p(st), n, 0, n, L.PCG64State.from_seed(rp.ENV_SEED), 7)
    rows = dev(np.arange(3 * n, dtype=np.int32))
    L.call("coevo_mpe_step", L._p(st), n, L._p(rows), L._p(dev((np.arange(3 * n) % 5).astype(np.int32))), 0, None, 1)
    return st


def reference_cycle(g7, words, n, state, ordinals, add, limits, c, obs, actions, status):
    """the launches of BaselineCrossPlay.enqueue_cycle for the game words `words`, with the entry points that existed before
    the gauntlet: observe, the evolved nets, the policy nets, the scripted seats, the world cycle"""
    rows = np.arange(3 * n, dtype=np.int32)
    call("coevo_mpe_observe", state, n, rows // 3, rows % 3, 3 * n, obs)
    fc, mlp, script = [], [], []
    for g in range(n):
        for s in range(3):
            kind, arg, lo, hi = (int(x) for x in words[g, 4 * s:4 * s + 4])
            D = 8 if s == 0 else 10
            if kind == gt.GT_FC:
                fc.append((arg, 3 * g + s, 1, D, 0))
            elif kind == gt.GT_MLP:
                mlp.append((arg, 3 * g + s, 1, D))
            else:
                script.append((g, 3 * g + s, kind, arg, lo, hi, s, 0))
    if fc:
        tasks = L.tasks_to_device(np.array(fc, dtype=L.TASK_DTYPE), DEV)
        L.call("coevo_fc_forward_argmax", L._p(g7.slab), L._p(tasks), len(fc), 1, L._p(obs), L._p(actions), None, L._p(status))
    if mlp:
        call("coevo_mlp_forward_argmax", g7.mlp_slab, g7.mlp_slab.numel(), np.array(mlp, dtype=np.int32), len(mlp), obs, 3 * n,
             actions, None, status)
    if script:
        call("coevo_baseline_actions", np.array(script, dtype=np.int32), len(script), ordinals, add, n, c, 5, actions, 3 * n)
    call("coevo_mpe_step", state, n, rows, actions, c, limits, 1)


def gauntlet_call(g7, words, n, state, ordinals, add, limits, c0, nc, obs, actions, status, slab_floats=None):
    L.call("coevo_mpe_gauntlet", L._p(g7.slab), g7.slab.numel() if slab_floats is None else slab_floats, L._p(g7.mlp_slab),
           g7.mlp_slab.numel(), L._p(words), n, L._p(ordinals), add, state if isinstance(state, int) else L._p(state), L._p(limits),
           c0, nc, 1, obs if isinstance(obs, int) else L._p(obs), actions if isinstance(actions, int) else L._p(actions),
           status if isinstance(status, int) else L._p(status))


# ------------------------------------------------------------------------------------------------------- 2. one cycle
@pytest.mark.parametrize("n_games", [1, 2, 7])
@pytest.mark.parametrize("cycle_first", [0, 3])
def test_one_cycle_equals_the_existing_entry_points_in_sequence(n_games, cycle_first):
    g7, kinds = seven()
    n, c = n_games, cycle_first
    pick = {1: [0], 2: [2, 5], 7: list(range(7))}[n]          # 2: the game without a net and the one with three evolved nets
    words_np = g7.plan.words[pick]
    words, ordinals = dev(words_np), dev(ORDINALS[:n])
    add = 2 ** 63 + 5 if c else 0                               # the sum wraps in 64 bits
    limits = dev(np.array([3 * c + 1, 3 * c + 2, 3 * c + 3, 75, 3 * c, 3 * c + 3, 2][:n], dtype=np.int32))
    s_ref, o_ref = start_state(n), torch.full((3 * n, L.OBS_STRIDE), 3.0, dtype=torch.float32, device=DEV)
    a_ref, st_ref = torch.full((3 * n,), SENTINEL, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    reference_cycle(g7, words_np, n, s_ref, ordinals, add, limits, c, o_ref, a_ref, st_ref)
    state = Guarded(L.MPE_STATE_DOUBLES * n, torch.float64, 0.0, -1.5)
    state.t.copy_(start_state(n).reshape(-1))
    obs = Guarded(3 * n * L.OBS_STRIDE, torch.float32, float("nan"), -9.0)
    actions = Guarded(3 * n, torch.int32, SENTINEL, -5)
    status = Guarded(1, torch.int32, 0, -5)
    gauntlet_call(g7, words, n, state.ptr(), ordinals, add, limits, c, 1, obs.ptr(), actions.ptr(), status.ptr())
    assert status.t.item() == st_ref.item() == 0
    assert np.array_equal(actions.t.cpu().numpy(), a_ref.cpu().numpy()) and (a_ref.cpu().numpy() != SENTINEL).all()
    assert same_bits(obs.t.cpu().numpy(), o_ref.cpu().numpy().reshape(-1))
    assert same_bits(state.t.cpu().numpy(), s_ref.cpu().numpy().reshape(-1))
    assert state.intact() and obs.intact() and actions.intact() and status.intact()
    if n == 7:
        for s in range(3):
            assert set(words_np[:, 4 * s]) == {0, 1, 2, 3, 4}


# ------------------------------------------------------------------------------------------------------ 3. whole games
def table_gauntlet(lists, **kw):
    return gt.Gauntlet(gc.table_matches(lists), **kw)


def assert_equals_crossplay(res, cp_res):
    """rewards word for word, the mean equal to the payoff"""
    M, E = res.rewards.shape[:2]
    assert same_bits(res.rewards, cp_res.rewards.reshape(M, E, 3)) and same_bits(res.mean, cp_res.payoff.reshape(M, 3))


@pytest.mark.parametrize("limit", [1, 2, 3, 4, 5, 73, 74, 75, None])
def test_whole_games_equal_baseline_crossplay_word_for_word(limit):
    """dims (2, 2, 3) x 2 episodes with every kind present: the three branches of the partial last cycle and the cut at
    max_cycles"""
    lists = mixed_lists()
    for max_cycles in (2, 25):
        res = table_gauntlet(lists, episodes=2, limit=limit, max_cycles=max_cycles).run(6)
        want = make_cp(lists, episodes=2, limit=limit, max_cycles=max_cycles).run(6)
        assert res.rewards.shape == (12, 2, 3) and res.mean.shape == (12, 3) and res.n_games == 24
        assert_equals_crossplay(res, want)
        assert want.rewards.any() or limit in (1, 2)          # (no world step before the third agent-step: nothing to credit)


def test_one_match_and_the_host_loop():
    lists = {"agent_0": [gc.fc_flat(10, 1)], "agent_1": [bc.fixture_baseline("agent_1")], "adversary_0": [bl.RandomBaseline(2 ** 64 - 1)]}
    for limit in (None, 31):
        res = table_gauntlet(lists, episodes=3, limit=limit).run(2 ** 40)
        assert_equals_crossplay(res, make_cp(lists, episodes=3, limit=limit).run(2 ** 40))
    lists = mixed_lists()
    want = bc.crossplay_rewards(lists, 2, 1, 7)                    # the oracle's own pieces on the host
    res = table_gauntlet(lists, episodes=2, limit=7).run(1)
    assert same_bits(res.rewards, want.reshape(12, 2, 3)) and want.any()


# ----------------------------------------------------------------------------------------------------- 4. split launches
def test_split_launches_equal_one_launch():
    g7, _ = seven()
    n = 7
    words, ordinals = dev(g7.plan.words), dev(ORDINALS)
    limits = dev(np.array([75, 74, 73, 31, 75, 30, 29], dtype=np.int32))
    out = []
    for spans in (((0, 25),), ((0, 10), (10, 15))):
        state = start_state(n)
        obs = torch.zeros(3 * n, L.OBS_STRIDE, dtype=torch.float32, device=DEV)
        actions, status = torch.zeros(3 * n, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        for c0, nc in spans:
            gauntlet_call(g7, words, n, state, ordinals, 3, limits, c0, nc, obs, actions, status)
        rewards = torch.zeros(n, 3, dtype=torch.float64, device=DEV)
        L.call("coevo_mpe_rewards", L._p(state), n, L._p(rewards))
        assert status.item() == 0
        out.append([t.cpu().numpy() for t in (state, rewards, obs, actions)])
    for a, b in zip(*out):
        assert same_bits(a, b)
    assert out[0][1].any()


# ------------------------------------------------------------------------------------------------------------ 5. poison
def test_poisoned_scratch_and_back_to_back_runs_give_the_same_words():
    g = table_gauntlet(mixed_lists(), episodes=2, limit=31)
    want = make_cp(mixed_lists(), episodes=2, limit=31).run(6)
    words = []
    for poison_f, poison_i in ((float("nan"), 0x7fffffff), (-3e38, -(2 ** 31))):
        g.obs.fill_(poison_f)
        g.actions.fill_(poison_i)
        g.state.fill_(float("nan"))
        g.rewards.fill_(float("nan"))
        g.mean.fill_(float("nan"))
        res = g.run(6)
        assert_equals_crossplay(res, want)
        words.append([t.cpu().numpy().copy() for t in (g.obs, g.actions, g.state, g.rewards, g.mean)])
    for a, b in zip(*words):
        assert same_bits(a, b)


def test_upload_and_set_champion_from_a_flat_array_and_from_a_device_pointer():
    a0, a0b, adv, advb, a1 = gc.fc_flat(10, 1), gc.fc_flat(10, 2), gc.fc_flat(8, 1), gc.fc_flat(8, 2), gc.fc_flat(10, 3)
    ppo, rnd = bc.fixture_baseline("agent_1"), bl.RandomBaseline(4)

    def explicit(champ_a0, champ_adv, seat_a1, seat_mlp):
        return [(champ_a0, seat_a1, rnd), (champ_a0, seat_mlp, champ_adv), (rnd, bl.PeriodicBaseline(1), bl.AlwaysFire)]
    g = gt.Gauntlet(explicit(gt.Champion("agent_0"), gt.Champion("adversary_0"), a1, ppo), episodes=2, limit=31)
    with pytest.raises(ValueError, match="has no weights yet"):
        g.run(1)
    g.set_champion("agent_0", a0)
    g.set_champion("adversary_0", adv)
    first = g.run(1)
    fresh = lambda *seats: gt.Gauntlet(explicit(*seats), episodes=2, limit=31).run(1)   # noqa: E731
    assert same_bits(first.rewards, fresh(a0, adv, a1, ppo).rewards)
    # from a device pointer: the nets lie in another object's slab, in the fc slab layout
    donor = gt.Gauntlet([(a0b, a0b, advb)], episodes=1)
    g.set_champion("agent_0", donor._ptr(donor.plan.fc_off[0]))
    g.set_champion("adversary_0", donor.slab[donor.plan.fc_off[2]:])
    second = g.run(1)
    assert same_bits(second.rewards, fresh(a0b, advb, a1, ppo).rewards) and not same_bits(second.rewards[:2], first.rewards[:2])
    assert same_bits(second.rewards[2], first.rewards[2])                                 # the match without a champion
    # upload: an evolved net from a flat array, then from a device pointer; a policy net
    g.upload(0, "agent_1", a0)
    third = g.run(1)
    assert same_bits(third.rewards, fresh(a0b, advb, a0, ppo).rewards) and same_bits(third.rewards[1:], second.rewards[1:])
    assert not same_bits(third.rewards[0], second.rewards[0])
    g.upload(0, "agent_1", donor._ptr(donor.plan.fc_off[1]))
    other_ppo = bl.MLPBaseline(bc.random_net(10, 9), 10)
    g.upload(1, "agent_1", other_ppo)
    fourth = g.run(1)
    assert same_bits(fourth.rewards, fresh(a0b, advb, a0b, other_ppo).rewards) and same_bits(fourth.rewards[2], first.rewards[2])
    for bad in (lambda: g.upload(2, "agent_0", a0), lambda: g.upload(0, "agent_0", a0), lambda: g.upload(3, "agent_1", a0),
                lambda: g.upload(0, "agent_1", adv), lambda: g.upload(1, "agent_1", bc.fixture()["adversary_0"]["flat"]),
                lambda: g.set_champion("agent_1", a0), lambda: g.set_champion("agent_0", adv), lambda: g.upload(0, "first_0", a0)):
        with pytest.raises(ValueError):
            bad()


# --------------------------------------------------------------------------------------------------------- 6. bad words
def test_a_game_with_a_bad_word_is_skipped_and_the_others_play():
    """data faults reported in the status word: the bad game's state is not touched, nothing is read through its words"""
    g7, _ = seven()
    n, bad_game = 7, 3
    ordinals, limits = dev(ORDINALS), dev(np.full(n, 31, dtype=np.int32))

    def play(words_np, slab_floats=None):
        state = start_state(n)
        obs = torch.full((3 * n, L.OBS_STRIDE), 3.0, dtype=torch.float32, device=DEV)
        actions = torch.full((3 * n,), SENTINEL, dtype=torch.int32, device=DEV)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        gauntlet_call(g7, dev(words_np), n, state, ordinals, 0, limits, 0, 11, obs, actions, status, slab_floats)
        return state.cpu().numpy(), obs.cpu().numpy(), actions.cpu().numpy(), int(status.item())
    clean = play(g7.plan.words)
    before = start_state(n).cpu().numpy()
    assert clean[3] == 0 and not same_bits(clean[0][:, bad_game], before[:, bad_game])
    w = g7.plan.words
    assert [w[bad_game, 4 * s] for s in (1, 2, 0)] == [bl.PERIODIC, bl.CONSTANT, gt.GT_FC]      # match 3: periodic, constant, fc
    fc_seat = next((g, s) for g in range(n) for s in range(3) if w[g, 4 * s] == gt.GT_FC and w[g, 4 * s + 1] > 0)
    cases = [(bad_game, 4, 9, None), (bad_game, 4, -1, None),                      # an unknown kind
             (bad_game, 1, w[bad_game, 1] + 2, None), (bad_game, 1, -64, None),    # an unaligned / a negative net offset
             (bad_game, 1, int(g7.slab.numel()) - 64, None),                       # an offset whose net leaves the slab
             (bad_game, 9, 5, None), (bad_game, 5, -1, None)]                      # a constant of 5, a periodic start of -1
    for game, word, value, slab_floats in cases + [(fc_seat[0], None, None, int(w[fc_seat[0], 4 * fc_seat[1] + 1]) + 100)]:
        words_np = w.copy()
        if word is not None:
            words_np[game, word] = value
        got = play(words_np, slab_floats)     # (the last case: a slab too short for the net of game fc_seat[0] and of later nets)
        assert got[3] == BAD_TASK, (word, value)
        skipped = [g for g in range(n) if any(words_np[g, 4 * s] == gt.GT_FC and slab_floats is not None and
                                              words_np[g, 4 * s + 1] + 138757 > slab_floats for s in range(3))] or [game]
        assert game in skipped
        for g in range(n):
            if g in skipped:
                assert same_bits(got[0][:, g], before[:, g]) and (got[2][3 * g:3 * g + 3] == SENTINEL).all() and (got[1][3 * g:3 * g + 3] == 3.0).all()
            else:
                assert same_bits(got[0][:, g], clean[0][:, g]) and np.array_equal(got[2][3 * g:3 * g + 3], clean[2][3 * g:3 * g + 3])
                assert same_bits(got[1][3 * g:3 * g + 3], clean[1][3 * g:3 * g + 3])


def test_nan_weights_raise_the_bits_of_the_per_cycle_route():
    lists = mixed_lists()
    bad_fc = lists["agent_0"][0].copy()
    bad_fc[100] = np.nan
    bad_mlp = bc.fixture()["agent_0"]["flat"].copy()
    bad_mlp[3] = np.nan
    for broken, msg in (({**lists, "agent_0": [bad_fc, lists["agent_0"][1]]}, "NaN"),
                        ({**lists, "agent_0": [lists["agent_0"][0], bl.MLPBaseline(bad_mlp, 10)]}, "after fc1")):
        cp, g = make_cp(broken, episodes=2, limit=7), table_gauntlet(broken, episodes=2, limit=7)
        with pytest.raises(ValueError, match=msg):
            cp.run(1)
        with pytest.raises(ValueError, match=msg) as e:
            g.run(1)
        assert "Warning" in str(e.value) and int(g.status.item()) == int(cp.status.item()) != 0
    for m in range(6, 12):          # the matches (1, b, c) seat the policy net, each its own copy
        g.upload(m, "agent_0", bc.fixture()["agent_0"]["flat"])
    assert_equals_crossplay(g.run(1), make_cp(lists, episodes=2, limit=7).run(1))     # repaired: the status word does not stick


# ------------------------------------------------------------------------------------------------------------ 7. trainer
def trainer_args(**kw):
    return Bag(algorithm="GA", generations=3, population=8, hof_size=3, elites_number=2, max_timesteps_per_episode=20,
               max_evaluation_steps=20, **kw)


def run_trainer(rng, spec, tmp_path=None):
    torch.manual_seed(5)
    np.random.seed(5)
    args = trainer_args(coevo_device_loop=False)
    env = initialize_env(args)
    if tmp_path is not None:
        res = ga.genetic_algorithm_train(env, env.agents[0], args, str(tmp_path), rng=rng, gauntlet=spec)
        return res, env, None
    tr = ga.GATrainer(env, args, rng=rng, gauntlet=spec)
    champions = []
    for _ in range(args.generations):
        tr.step()
        champions.append({r: tr.eng.download(r, "hof", args.hof_size - 1, 1)[0] for r in ga.ROLES})
    return tr.finish(), env, champions


@pytest.mark.parametrize("rng", ["host_reference", "device_philox"])
def test_trainer_scores_every_generation_and_changes_nothing_else(rng, tmp_path):
    spec = gc.reference_spec(episodes=2, first_ordinal=4)
    off, env_off, _ = run_trainer(rng, None)
    on, env_on, champions = run_trainer(rng, spec)
    for field in ("elite_ids", "fitness", "sigma_after", "diversity"):
        assert getattr(on, field) == getattr(off, field), field
    assert on.rewards == off.rewards and env_on.n_resets == env_off.n_resets
    assert all(same_bits(a, b) for a, b in zip(on.game_rewards, off.game_rewards))
    for r in ga.ROLES:      # what a checkpoint saves
        for region, k in (("hof", 3), ("elite", 2)):
            assert [sha(x) for x in on.engine.download(r, region, 0, k)] == [sha(x) for x in off.engine.download(r, region, 0, k)]
    assert off.gauntlet is None and off.gauntlet_matches is None
    assert on.gauntlet_matches == spec.names() and len(on.gauntlet) == 3
    for g, champ in enumerate(champions):      # a fresh BaselineCrossPlay over the champions downloaded after step g
        want = []
        for a0, a1, adv in spec.matches():
            seat = lambda x, r: champ[r] if isinstance(x, gt.Champion) else x      # noqa: E731
            cp = bl.BaselineCrossPlay([seat(a0, "agent_0")], [seat(a1, "agent_1")], [seat(adv, "adversary_0")], episodes=2, limit=20)
            want.append(cp.run(4).payoff[0, 0, 0])
        assert same_bits(np.array(on.gauntlet[g]), np.array(want)), g
    assert on.gauntlet[0] != on.gauntlet[2]
    res, _, _ = run_trainer(rng, spec, tmp_path)
    lines = [json.loads(x) for x in open(tmp_path / "metrics.jsonl")]
    assert len(lines) == 3 and [x["gauntlet"] for x in lines] == on.gauntlet == res.gauntlet
