"""The MPE environment's host entry points (the env kernels' own bodies compiled for the host cores: csrc/mpe_env.hip,
mpe_obs_from_game / mpe_load_game of csrc/coevo_common.hip.h), the oracle's env and the fp16 checker's stepwise game against
the plain numpy reference of tests/env_cases.py: resets at deep ordinals (the 64-bit overflow point of the jump-ahead
distance, 2^63 - 1), crafted states (far fields, exact ties, float32 / fp64 subnormals, signed zeros, run-away and non-finite
values), both integration orders, actions outside 0 .. 4, ragged limits and shuffled row tables.  Equalities of bit patterns
only (NaN matches NaN).  No GPU."""
import ctypes as C

import numpy as np
import pytest

from coevonet_amd import lib as L
from coevonet_amd.mpe import simple_adversary as sa
from oracle import ref_port as rp
from tests import env_cases as ec
from tests import fp16_checker as ck
from tests.util import load_golden

N, CYCLES = 64, 7
NAN = float("nan")


def seed_rng():
    return L.PCG64State.from_seed(ec.ENV_SEED)


def test_constants_and_ref_reset_is_the_reset_stream():
    assert (ec.STATE_DOUBLES, ec.OBS_STRIDE) == (L.MPE_STATE_DOUBLES, L.OBS_STRIDE)
    goal, apos, lpos = sa.ResetStream(skip_initial=False).take(50)
    for o in range(50):
        g, a, l = ec.ref_reset(o)
        assert g == goal[o] and np.array_equal(a, apos[o]) and np.array_equal(l, lpos[o]), o
    assert len(ec.ORDINALS) == 4 + 7 + 21 + 4 + 1 and max(ec.ORDINALS) == 2 ** 63 - 1


@pytest.mark.parametrize("ordinal", ec.ORDINALS)
def test_host_reset_jump_ahead(ordinal):
    """one game alone (no predecessor: pcg_advance over (ordinal >> 1) * 21 outputs) into a NaN state: all 24 fields written"""
    st = np.full((L.MPE_STATE_DOUBLES, 1), NAN)
    o = np.array([ordinal], dtype=np.int64)
    assert L.load().coevo_mpe_host_reset(st.ctypes.data, 1, seed_rng(), o.ctypes.data) == 0
    ec.assert_same(st, ec.reset_states([ordinal]), f"coevo_mpe_host_reset at ordinal {ordinal}")


def test_host_reset_list_continues_and_jumps():
    """ORDINALS ascending in one call: consecutive ordinals continue the stream (the run of 7 from an odd one, the triples
    around every power of two, the pair across the overflow point), the others jump; then descending: every game jumps"""
    lib = L.load()
    for ords in (ec.ORDINALS, ec.ORDINALS[::-1]):
        o = np.array(ords, dtype=np.int64)
        st = np.full((L.MPE_STATE_DOUBLES, len(o)), NAN)
        assert lib.coevo_mpe_host_reset(st.ctypes.data, len(o), seed_rng(), o.ctypes.data) == 0
        ec.assert_same(st, ec.reset_states(ords), "coevo_mpe_host_reset over ORDINALS")


def test_host_reset_games_both_paths_and_untouched_games():
    """coevo_mpe_host_reset_games over a slice of a game list: ascending game ids (continuation wherever ordinals follow each
    other) and a shuffled list (jump-ahead nearly everywhere); games outside the slice keep their NaN"""
    lib = L.load()
    o = np.array(ec.ORDINALS, dtype=np.int64)
    n = len(o)
    want = ec.reset_states(ec.ORDINALS)
    for games in (np.arange(n, dtype=np.int32), np.random.default_rng(3).permutation(n).astype(np.int32)):
        lo, hi = 3, n - 2
        st = np.full((L.MPE_STATE_DOUBLES, n), NAN)
        assert lib.coevo_mpe_host_reset_games(st.ctypes.data, n, seed_rng(), o.ctypes.data, games.ctypes.data, lo, hi) == 0
        inside = np.zeros(n, dtype=bool)
        inside[games[lo:hi]] = True
        ec.assert_same(st[:, inside], want[:, inside], "coevo_mpe_host_reset_games")
        assert np.isnan(st[:, ~inside]).all() and (~inside).sum() == 5


@pytest.mark.parametrize("ordinal", ec.DEVICE_ORDINALS)
def test_oracle_reset(ordinal):
    s = rp.MpeState()
    s.goal = -1
    rp.lib().oracle_mpe_reset(*rp.Stream().st, ordinal, C.byref(s))
    goal, apos, lpos = ec.ref_reset(ordinal)
    assert s.goal == goal
    ec.assert_same(np.array(s.ppos), apos, f"oracle_mpe_reset positions at {ordinal}")
    ec.assert_same(np.array(s.lm), lpos, f"oracle_mpe_reset landmarks at {ordinal}")
    assert not np.array(s.pvel).view(np.uint64).any()


# ------------------------------------------------------------------------------------------------- crafted states
_REF = {}


def reference(pos_first, ragged):
    """(batch, actions, limits, game_rows, row_game, row_slot, ref_play's cycles): computed once, read only"""
    key = (pos_first, ragged)
    if key not in _REF:
        b = ec.Batch(N, seed=1)
        acts = ec.actions_by_game(N, CYCLES, seed=2)
        limits = ec.ragged_limits(N, CYCLES, seed=3) if ragged else None
        _REF[key] = (b, acts, limits, *ec.shuffled_rows(N, seed=4), ec.ref_play(b, acts, limits, pos_first))
    return _REF[key]


def test_every_class_is_in_the_batch():
    b = reference(1, True)[0]
    assert set(ec.CLASSES) <= set(b.names) and b.names.count("ordinary") == N - len(ec.CLASSES)
    lim = reference(1, True)[2]
    c = CYCLES - 2
    assert set(lim.tolist()) == {0, 1, 2, 3, 4, 3 * c - 1, 3 * c, 3 * c + 1, ec.HUGE}


def rows_of(acts_c, game_rows):
    a = np.full(3 * len(acts_c) + 5, -9, dtype=np.int32)   # (rows past 3n: words no game points to)
    a[game_rows.reshape(-1)] = acts_c.reshape(-1)
    return a


@pytest.mark.parametrize("ragged", [True, False], ids=["ragged", "no_limit"])
@pytest.mark.parametrize("pos_first", [1, 0])
def test_host_observe_and_step(pos_first, ragged):
    """coevo_mpe_host_observe into a NaN buffer (all 12 columns of every row written, columns >= D +0.0) and
    coevo_mpe_host_step, seven cycles: every observation row and all 24 state fields after every cycle"""
    lib = L.load()
    b, acts, limits, game_rows, row_game, row_slot, ref = reference(pos_first, ragged)
    st = b.state.copy()
    lim_p = limits.ctypes.data if limits is not None else None
    for c in range(CYCLES):
        obs = np.full((3 * N, L.OBS_STRIDE), NAN, dtype=np.float32)
        assert lib.coevo_mpe_host_observe(st.ctypes.data, N, row_game.ctypes.data, row_slot.ctypes.data, 3 * N, obs.ctypes.data) == 0
        ec.assert_same(obs, ec.obs_rows(ref[c]["obs"], row_game, row_slot), f"observations of cycle {c}")
        a = rows_of(acts[c], game_rows)
        assert lib.coevo_mpe_host_step(st.ctypes.data, N, game_rows.ctypes.data, a.ctypes.data, len(a), c, lim_p, pos_first) == 0
        ec.assert_same(st, ref[c]["state"], f"state after cycle {c} (pos_first {pos_first})")
    ec.assert_same(st[[12, 13, 14, 15, 16, 17, 22, 23]], b.state[[12, 13, 14, 15, 16, 17, 22, 23]], "constant fields")


@pytest.mark.parametrize("ragged", [True, False], ids=["ragged", "no_limit"])
@pytest.mark.parametrize("pos_first", [1, 0])
def test_host_step_games(pos_first, ragged):
    """coevo_mpe_host_step_games: step cycle c - 1 (none at c = 0) then observe, over two slices of a shuffled game list that
    leaves three games out: those keep their state and their NaN observation rows"""
    lib = L.load()
    b, acts, limits, game_rows, row_game, row_slot, ref = reference(pos_first, ragged)
    games = np.random.default_rng(5).permutation(N).astype(np.int32)
    out, games = games[-3:], games[:-3].copy()
    inside = np.ones(N, dtype=bool)
    inside[out] = False
    st = b.state.copy()
    lim_p = limits.ctypes.data if limits is not None else None
    for c in range(CYCLES + 1):
        obs = np.full((3 * N, L.OBS_STRIDE), NAN, dtype=np.float32)
        a = rows_of(acts[c - 1], game_rows) if c > 0 else None
        for lo, hi in ((0, 20), (20, len(games))):
            assert lib.coevo_mpe_host_step_games(st.ctypes.data, N, game_rows.ctypes.data, a.ctypes.data if c > 0 else None,
                                                 c - 1, lim_p, pos_first, games.ctypes.data, lo, hi, 1 if c < CYCLES else 0,
                                                 obs.ctypes.data) == 0
        if c > 0:
            ec.assert_same(st[:, inside], ref[c - 1]["state"][:, inside], f"state after cycle {c - 1}")
        ec.assert_same(st[:, ~inside], b.state[:, ~inside], "games outside the list")
        rows_in = inside[row_game]
        if c < CYCLES:
            ec.assert_same(obs[rows_in], ec.obs_rows(ref[c]["obs"], row_game, row_slot)[rows_in], f"observations of cycle {c}")
            assert np.isnan(obs[~rows_in]).all()
        else:
            assert np.isnan(obs).all()


def oracle_state(b, g):
    s = rp.MpeState()
    for a in range(3):
        for k in range(2):
            s.ppos[a][k], s.pvel[a][k] = b.apos[g, a, k], b.vel[g, a, k]
    for l in range(2):
        for k in range(2):
            s.lm[l][k] = b.lpos[g, l, k]
    s.goal = int(b.goal[g])
    return s


@pytest.mark.parametrize("pos_first", [1, 0])
def test_oracle_observe_and_world_step(pos_first):
    """oracle_mpe_observe / oracle_mpe_world_step under oracle_mpe_set_pos_first on every game of the batch, seven cycles:
    observations, positions, velocities and both rewards - what lets the whole-game tests trust play_game_steps(poke=...)"""
    O = rp.lib()
    b, acts, _, _, _, _, ref = reference(pos_first, False)
    O.oracle_mpe_set_pos_first(pos_first)
    try:
        for g in range(N):
            s = oracle_state(b, g)
            acc_adv, rg_prev = 0.0, 0.0
            for c in range(CYCLES):
                for slot, D in enumerate((8, 10, 10)):
                    obs = np.full(10, NAN, dtype=np.float32)
                    O.oracle_mpe_observe(C.byref(s), slot, rp._fp(obs))
                    ec.assert_same(obs[:D], ref[c]["obs"][slot][g], f"{b.names[g]} game {g} cycle {c} slot {slot}")
                rg, ra = C.c_double(0), C.c_double(0)
                O.oracle_mpe_world_step(C.byref(s), (C.c_int * 3)(*[int(x) for x in acts[c][g]]), C.byref(rg), C.byref(ra))
                acc_adv, rg_prev = acc_adv + ra.value, rg.value
                what = f"{b.names[g]} game {g} after cycle {c}"
                ec.assert_same(np.array(s.ppos).reshape(6), ref[c]["state"][0:6, g], what + " positions")
                ec.assert_same(np.array(s.pvel).reshape(6), ref[c]["state"][6:12, g], what + " velocities")
                ec.assert_same(np.array([rg_prev, acc_adv]), ref[c]["state"][[18, 21], g], what + " rewards")
    finally:
        O.oracle_mpe_set_pos_first(1)


def test_checker_play_game_steps_is_play_game():
    """tests/fp16_checker.play_game_steps with no poke == play_game (fc16_play_game) on the 18 games of play_game_f16.json"""
    from tests.test_fp16_cpu import fixture_agents
    n = 0
    for c in load_golden("play_game_f16.json")["cases"]:
        _, _, ags = fixture_agents(c)
        flats = [a.model.flat() for a in ags]
        s1, s2 = rp.Stream(), rp.Stream()
        for _ in c["games"]:
            want = ck.play_game(s1, *flats, c["limit"], c["max_cycles"])
            got = ck.play_game_steps(s2, *flats, c["limit"], c["max_cycles"])
            for k in ("rewards", "steps", "actions", "status", "ordinal"):
                assert got[k] == want[k], (c["torch_seed"], k)
            n += 1
    assert n == 18
