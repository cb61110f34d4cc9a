"""The MPE environment kernels (csrc/mpe_env.hip; mpe_world_step / mpe_world_move / mpe_obs_from_game / mpe_fused_observe of
csrc/coevo_common.hip.h) on the device against the plain numpy reference of tests/env_cases.py, the oracle and the fp16
checker: resets at deep ordinals through every reset entry point, crafted states through coevo_mpe_observe / coevo_mpe_step /
coevo_mpe_final_step[_pack], and the finite crafted states through every fused fp32 rollout form and the fp16 cycle kernel.
Every comparison is an equality of bit patterns (NaN matches NaN); buffers start poisoned and carry guard words.

Sizes: n = 1, 127, 128, 129 games for the 128-thread kernels; 1, 21, 22, 43 rows for the observe kernel (256 threads over
12 columns a row: 21 rows end inside the first block, 22 rows start the second)."""
import ctypes as C

import numpy as np
import pytest
import torch

from coevonet_amd import lib as L
from oracle import ref_port as rp
from tests import env_cases as ec
from tests import fp16_checker as ck
from tests import test_fc_forward_edges_gpu as fe
from tests import test_fp16_rollout_gpu as f16

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
NS = (1, 127, 128, 129)
CYCLES = 6
MAX_JOBS = L.K["COEVO_MAX_JOBS"]
ERR_ARG = L.K["COEVO_ERR_ARG"]


def seed_rng():
    return L.PCG64State.from_seed(ec.ENV_SEED)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def opt_dev(a):
    return None if a is None else dev(a)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def nan_state(n):
    return torch.full((L.MPE_STATE_DOUBLES, n), NAN, dtype=torch.float64, device=DEV)


def runs_of(ordinals):
    """consecutive ordinals grouped -> [(first ordinal, count)]"""
    out = []
    for o in ordinals:
        if out and out[-1][0] + out[-1][1] == o:
            out[-1][1] += 1
        else:
            out.append([o, 1])
    return [tuple(r) for r in out]


def seg_array(segs):
    return (L.ResetSeg * len(segs))(*[L.ResetSeg(int(a), int(b), int(c)) for a, b, c in segs])


# ============================================================================================================ a. resets
class Arm:
    """stamp pairs and sync words for the arming reset forms, a guard word on both sides of each array"""

    def __init__(self, n_stamps, n_zero):
        self.n_stamps, self.n_zero = n_stamps, n_zero
        self.stamps = torch.full((2 * n_stamps + 2,), 5, dtype=torch.int64, device=DEV)
        self.words = torch.full((n_zero + 2,), 0x5a5a5a5a, dtype=torch.int32, device=DEV)

    def stamps_p(self):
        return self.stamps.data_ptr() + 8

    def words_p(self):
        return self.words.data_ptr() + 4

    def check(self, stamps_armed, words_zeroed, what):
        s, w = host(self.stamps), host(self.words)
        assert s[0] == 5 and s[-1] == 5 and w[0] == 0x5a5a5a5a and w[-1] == 0x5a5a5a5a, f"{what}: a guard word was written"
        pairs = s[1:-1].reshape(-1, 2)
        if stamps_armed:
            assert (pairs[:, 0] == -1).all() and (pairs[:, 1] == 0).all(), f"{what}: stamp pairs not re-armed to (UINT64_MAX, 0)"
        else:
            assert (pairs == 5).all(), f"{what}: stamps written"
        assert (w[1:-1] == (0 if words_zeroed else 0x5a5a5a5a)).all(), f"{what}: sync words"


def reset_call(entry, st, n, segs, arm=None):
    """one launch of a multi form -> return code.  arm: an Arm whose arrays the form takes (multi_arm: the stamps;
    multi_prep: both)"""
    lib, arr = L.load(), seg_array(segs)
    p = C.cast(arr, C.c_void_p)
    if entry == "multi":
        return lib.coevo_mpe_reset_multi(L._p(st), n, p, len(segs), seed_rng(), L._stream())
    if entry == "multi_arm":
        return lib.coevo_mpe_reset_multi_arm(L._p(st), n, p, len(segs), seed_rng(), arm.stamps_p(), arm.n_stamps, L._stream())
    return lib.coevo_mpe_reset_multi_prep(L._p(st), n, p, len(segs), seed_rng(), arm.stamps_p(), arm.n_stamps, arm.words_p(),
                                          arm.n_zero, L._stream())


@pytest.mark.parametrize("entry", ["reset", "multi", "multi_arm", "multi_prep"])
def test_resets_at_deep_ordinals(entry):
    """DEVICE_ORDINALS (0 .. 3, 2^k - 1 .. 2^k + 1 up to k = 62, a run of 7 from an odd ordinal, the 64-bit overflow point of
    (ordinal >> 1) * 21, 2^63 - 1, 2^63 + 2, 2^64 - 1): one game each in a NaN state, consecutive ordinals as one range - all 24
    fields of every reset game written with numpy's values, the games around them still NaN"""
    ords = ec.DEVICE_ORDINALS
    n = len(ords) + 3
    st, at, segs = nan_state(n), 2, []
    for first, count in runs_of(ords):
        segs.append((at, count, first))
        at += count
    assert at == n - 1 and (2 ** 64 - 1, 1) in [(s[2], s[1]) for s in segs]
    if entry == "reset":
        for game_first, count, first in segs:
            L.call("coevo_mpe_reset", L._p(st), n, game_first, count, seed_rng(), first)
    else:
        arm = Arm(3, 5)
        for i in range(0, len(segs), MAX_JOBS):
            assert reset_call(entry, st, n, segs[i:i + MAX_JOBS], arm) == 0
        arm.check(entry != "multi", entry == "multi_prep", entry)
    got = host(st)
    ec.assert_same(got[:, 2:n - 1], ec.reset_states(ords), f"coevo_mpe_{entry} at DEVICE_ORDINALS")
    assert np.isnan(got[:, [0, 1, n - 1]]).all(), "a game outside the ranges was written"


@pytest.mark.parametrize("first_ordinal,gens", [(-3000, (0, 1, 1000)), (2 ** 40 + 7, (0, 1000)), (ec.OVERFLOW_EDGE - 3040000, (1000,))])
def test_reset_gen(first_ordinal, gens):
    """coevo_mpe_reset_gen: first ordinal = first_ordinal + *gen_dev * 3040 clamped at 0 - a negative first ordinal resets
    generation 0 from ordinal 0 on and later generations from the sum; 129 games (two blocks) inside a NaN state; equal to
    numpy and to coevo_mpe_reset at the summed ordinal"""
    n, game_first, count, per_gen = 140, 3, 129, 3040
    for gen in gens:
        gen_dev = torch.tensor([gen], dtype=torch.int32, device=DEV)
        first = max(first_ordinal + gen * per_gen, 0)
        assert (first == 0) == (first_ordinal < 0 and gen == 0)
        st, st2 = nan_state(n), nan_state(n)
        L.call("coevo_mpe_reset_gen", L._p(st), n, game_first, count, seed_rng(), first_ordinal, L._p(gen_dev), per_gen)
        L.call("coevo_mpe_reset", L._p(st2), n, game_first, count, seed_rng(), first)
        got, got2 = host(st), host(st2)
        ec.assert_same(got[:, game_first:game_first + count], ec.reset_states(range(first, first + count)), f"reset_gen, gen {gen}")
        ec.assert_same(got, got2, f"reset_gen vs coevo_mpe_reset at ordinal {first}")
        assert np.isnan(got[:, :game_first]).all() and np.isnan(got[:, game_first + count:]).all()
        assert int(gen_dev.item()) == gen


SEG_CASES = {   # counts of the segments of one launch (COEVO_MAX_JOBS = 4 a launch: the five counts 0, 1, 127, 128, 129 take two)
    "0_1_127_129": (0, 1, 127, 129), "128_0_129_1": (128, 0, 129, 1), "one_segment": (129,), "one_empty_segment": (0,),
    "all_empty": (0, 0, 0, 0)}


@pytest.mark.parametrize("entry", ["multi", "multi_arm", "multi_prep"])
@pytest.mark.parametrize("case", list(SEG_CASES))
def test_reset_multi_shapes(case, entry):
    """segment counts 0, 1, 127, 128, 129 side by side, n_segs = 1 (the first and the last block row are the same) and
    COEVO_MAX_JOBS, all counts 0 (still one launch when there are stamps or sync words); n_stamps and n_zero larger than the
    launch's thread count (one block of 128 threads a row, or two), so the grid-stride loops go round; guard words keep"""
    counts = SEG_CASES[case]
    assert len(counts) in (1, MAX_JOBS)
    n = sum(counts) + 2 * len(counts) + 1
    st, segs, at, ords = nan_state(n), [], 1, []
    for i, cnt in enumerate(counts):
        first = (7, 2 ** 33 + 1, ec.OVERFLOW_EDGE, 10 ** 6)[i]
        segs.append((at, cnt, first))
        ords.append((at, cnt, first))
        at += cnt + 2
    arm = Arm(2 * 128 + 71, 3 * 128 + 5)
    assert reset_call(entry, st, n, segs, arm) == 0
    arm.check(entry != "multi", entry == "multi_prep", f"{entry} {case}")
    got, written = host(st), np.zeros(n, dtype=bool)
    for game_first, cnt, first in ords:
        if cnt:
            ec.assert_same(got[:, game_first:game_first + cnt], ec.reset_states(range(first, first + cnt)), f"{entry} {case}")
        written[game_first:game_first + cnt] = True
    assert np.isnan(got[:, ~written]).all(), "a game outside the segments was written"


def test_reset_multi_prep_one_array_each():
    """coevo_mpe_reset_multi_prep with stamps only and with sync words only (the other pointer NULL, its count ignored), over
    empty segments: one launch that resets nothing"""
    lib, n = L.load(), 8
    for stamps, words in ((True, False), (False, True)):
        st, arm = nan_state(n), Arm(300, 700)
        arr = seg_array([(0, 0, 5), (3, 0, 9)])
        rc = lib.coevo_mpe_reset_multi_prep(L._p(st), n, C.cast(arr, C.c_void_p), 2, seed_rng(), arm.stamps_p() if stamps else None,
                                            arm.n_stamps if stamps else -4, arm.words_p() if words else None,
                                            arm.n_zero if words else -4, L._stream())
        assert rc == 0
        arm.check(stamps, words, f"prep stamps={stamps} words={words}")
        assert np.isnan(host(st)).all()


def test_reset_refusals_leave_every_buffer_unchanged():
    """the argument combinations the reset entry points refuse (COEVO_ERR_ARG): state, stamps and sync words keep their bits"""
    lib, n = L.load(), 20
    st, arm, rng, s = nan_state(n), Arm(40, 60), seed_rng(), L._stream()
    ok = [(2, 5, 11), (9, 3, 4)]

    def multi(segs, n_games=n, state=True, n_segs=None, null_segs=False):
        arr = seg_array(segs)
        return (L._p(st) if state else None, n_games, None if null_segs else C.cast(arr, C.c_void_p),
                len(segs) if n_segs is None else n_segs, rng), arr

    bad_tables = [dict(segs=ok, state=False), dict(segs=ok, n_games=0), dict(segs=ok, null_segs=True), dict(segs=ok, n_segs=0),
                  dict(segs=ok * 3, n_segs=MAX_JOBS + 1), dict(segs=[(-1, 2, 0)]), dict(segs=[(0, -1, 0)]),
                  dict(segs=ok + [(n - 2, 3, 0)])]
    for kw in bad_tables:
        head, keep = multi(**kw)
        assert lib.coevo_mpe_reset_multi(*head, s) == ERR_ARG, kw
        assert lib.coevo_mpe_reset_multi_arm(*head, arm.stamps_p(), arm.n_stamps, s) == ERR_ARG, kw
        assert lib.coevo_mpe_reset_multi_prep(*head, arm.stamps_p(), arm.n_stamps, arm.words_p(), arm.n_zero, s) == ERR_ARG, kw
    head, keep = multi(ok)
    assert lib.coevo_mpe_reset_multi_arm(*head, None, arm.n_stamps, s) == ERR_ARG
    assert lib.coevo_mpe_reset_multi_arm(*head, arm.stamps_p(), 0, s) == ERR_ARG
    assert lib.coevo_mpe_reset_multi_prep(*head, arm.stamps_p(), 0, arm.words_p(), arm.n_zero, s) == ERR_ARG
    assert lib.coevo_mpe_reset_multi_prep(*head, arm.stamps_p(), arm.n_stamps, arm.words_p(), -1, s) == ERR_ARG
    for fn, tail in ((lib.coevo_mpe_reset, (5,)), (lib.coevo_mpe_reset_gen, (5, None, 0))):
        for state, n_games, game_first, count in ((False, n, 0, 4), (True, 0, 0, 0), (True, n, -1, 4), (True, n, 0, -1),
                                                  (True, n, n - 3, 4)):
            assert fn(L._p(st) if state else None, n_games, game_first, count, rng, *tail, s) == ERR_ARG
    arm.check(False, False, "refused calls")
    assert np.isnan(host(st)).all()


# ========================================================================================================== b. observe
@pytest.mark.parametrize("n_rows", [1, 21, 22, 43])
def test_observe_crafted_states(n_rows):
    """every (class, seat) pair of the crafted batch at shuffled rows, the 43rd row a repeat (n_rows < 43: the first rows of
    the same table) into a NaN buffer: all 12 columns of every row written, columns >= D +0.0, the float32-subnormal class
    subnormal as numpy's cast has it, the rows behind the last one untouched"""
    n = 29
    b = ec.Batch(n, seed=21)
    g = np.random.Generator(np.random.PCG64(22))
    pairs = [(b.index(name), slot) for name in ec.CLASSES for slot in range(3)]
    pairs = [pairs[i] for i in g.permutation(len(pairs))]
    sub = (b.index("subnormal_obs"), 1)
    pairs.remove(sub)
    pairs = ([sub] + pairs + [pairs[4]])[:n_rows]   # (the subnormal seat first: in every row count)
    assert len(pairs) == n_rows
    row_game, row_slot = (np.array([p[k] for p in pairs], dtype=np.int32) for k in (0, 1))
    with np.errstate(all="ignore"):
        want = ec.obs_rows(b.env().observe(), row_game, row_slot)
    tiny = np.abs(want[0])
    assert ((tiny > 0) & (tiny < 2.0 ** -126)).any()
    obs = torch.full((n_rows + 2, L.OBS_STRIDE), NAN, dtype=torch.float32, device=DEV)
    d_st, d_game, d_slot = dev(b.state), dev(row_game), dev(row_slot)   # (held across the launch)
    L.call("coevo_mpe_observe", L._p(d_st), n, L._p(d_game), L._p(d_slot), n_rows, L._p(obs))
    got = host(obs)
    ec.assert_same(got[:n_rows], want, f"coevo_mpe_observe, {n_rows} rows")
    D = np.where(row_slot == 0, 8, 10)
    for r in range(n_rows):
        assert not got[r, D[r]:].view(np.uint32).any(), f"row {r}: columns >= {D[r]} are not +0.0"
    assert np.isnan(got[n_rows:]).all(), "rows past n_rows were written"


# ============================================================================================================= c. step
_PLAY = {}


def played(n, pos_first, ragged):
    """(batch, actions [c][n][3], limits or None, game_rows, ref_play's cycles) - computed once, read only"""
    key = (n, pos_first, ragged)
    if key not in _PLAY:
        b = ec.Batch(n, seed=31)
        acts = ec.actions_by_game(n, CYCLES, seed=32)
        limits = ec.ragged_limits(n, CYCLES, seed=33) if ragged else None
        _PLAY[key] = (b, acts, limits, ec.shuffled_rows(n, seed=34)[0], ec.ref_play(b, acts, limits, pos_first))
    return _PLAY[key]


@pytest.mark.parametrize("ragged", [True, False], ids=["ragged", "no_limit"])
@pytest.mark.parametrize("pos_first", [1, 0])
@pytest.mark.parametrize("n", NS)
def test_step_crafted_states(n, pos_first, ragged):
    """coevo_mpe_step, six cycles: actions -1 .. 6 and a game of 0x7f7f7f7f words read through a shuffled game_rows, ragged
    limits (or game_limit = NULL), both integration orders - all 24 fields of every game after every cycle, the constant
    fields (12 .. 17, 22, 23) unchanged, then coevo_mpe_rewards"""
    b, acts, limits, game_rows, ref = played(n, pos_first, ragged)
    if n >= 127:
        assert set(ec.CLASSES) <= set(b.names)
    st, d_rows = dev(b.state), dev(game_rows)
    d_lim = dev(limits) if ragged else None
    const = [12, 13, 14, 15, 16, 17, 22, 23]
    for c in range(CYCLES):
        a = np.full(3 * n + 5, -9, dtype=np.int32)
        a[game_rows.reshape(-1)] = acts[c].reshape(-1)
        d_a = dev(a)
        L.call("coevo_mpe_step", L._p(st), n, L._p(d_rows), L._p(d_a), c, L._p(d_lim), pos_first)
        got = host(st)
        ec.assert_same(got, ref[c]["state"], f"n {n} pos_first {pos_first} after cycle {c}")
        ec.assert_same(got[const], b.state[const], "constant fields")
    rew = torch.full((n + 1, 3), NAN, dtype=torch.float64, device=DEV)
    L.call("coevo_mpe_rewards", L._p(st), n, L._p(rew))
    got = host(rew)
    ec.assert_same(got[:n], ec.triples(ref[-1]["acc"]), "coevo_mpe_rewards")
    assert np.isnan(got[n]).all()


# ======================================================================================================= d. final step
def final_cases(n, pos_first):
    """(state before, cycle, actions by game or None, limits or None, wanted triples): the books of cycle -1 (as they stand), of
    the cycles c - 1 and c around which the ragged limits 3c - 1, 3c, 3c + 1 put t0, t0 + 1 and t0 + 2 on both sides, and of
    cycle c without limits"""
    c = CYCLES - 2
    b, acts, limits, _, ref = played(n, pos_first, True)
    _, _, _, _, free = played(n, pos_first, False)
    if n > 8:
        for k in (c - 1, c):
            sides = {(3 * k < v, 3 * k + 1 < v, 3 * k + 2 < v) for v in limits.tolist()}
            assert {(False, False, False), (True, True, True)} <= sides
        assert {(3 * (c - 1) + 2 < v, 3 * c + 1 < v) for v in limits.tolist()} >= {(False, False), (True, False), (True, True)}
    return [(ref[c - 1]["state"], -1, None, limits, ec.triples(ref[c - 1]["acc"])),
            (ref[c - 2]["state"], c - 1, acts[c - 1], limits, ec.triples(ref[c - 1]["acc"])),
            (ref[c - 1]["state"], c, acts[c], limits, ec.triples(ref[c]["acc"])),
            (free[c - 1]["state"], c, acts[c], None, ec.triples(free[c]["acc"]))]


@pytest.mark.parametrize("pos_first", [1, 0])
@pytest.mark.parametrize("n", NS)
def test_final_step_closing_credits(n, pos_first):
    """coevo_mpe_final_step against the reference's books after the same cycle (its world step is the device-only
    mpe_world_step: every crafted class, both integration orders); the state buffer keeps its bits"""
    for state, cycle, acts, limits, want in final_cases(n, pos_first):
        st = dev(state)
        rew = torch.full((n + 1, 3), NAN, dtype=torch.float64, device=DEV)
        d_act, d_lim = opt_dev(acts), opt_dev(limits)   # (held across the launch)
        L.call("coevo_mpe_final_step", L._p(st), n, L._p(d_act), cycle, L._p(d_lim), pos_first, L._p(rew))
        got = host(rew)
        ec.assert_same(got[:n], want, f"coevo_mpe_final_step n {n} cycle {cycle} pos_first {pos_first}")
        assert np.isnan(got[n]).all()
        ec.assert_same(host(st), state, "the state after coevo_mpe_final_step")


@pytest.mark.parametrize("hof,n_local", [(1, 40), (3, 14)])
@pytest.mark.parametrize("pos_first", [1, 0])
def test_final_step_pack(pos_first, hof, n_local):
    """coevo_mpe_final_step_pack, 129 games of which the first 3 * n_local * hof are [role][individual][hof game]: rewards as
    the reference's, pack[role][j] = the triple of the individual's LAST hof game + its distance read at dist_first + j of a
    row of dist_pitch > dist_first + n_local floats; guard doubles around pack, the state keeps its bits"""
    n, n_roles, pitch, first = 129, 3, n_local + 9, 4
    assert n_roles * n_local * hof < n
    dist = np.random.default_rng(41).random((n_roles, pitch)).astype(np.float32) * 3
    for state, cycle, acts, limits, want in final_cases(n, pos_first):
        st = dev(state)
        rew = torch.full((n + 1, 3), NAN, dtype=torch.float64, device=DEV)
        pack = torch.full((2 + n_roles * n_local * 4 + 2,), -7.0, dtype=torch.float64, device=DEV)
        d_act, d_lim, d_dist = opt_dev(acts), opt_dev(limits), dev(dist)   # (held across the launch)
        L.call("coevo_mpe_final_step_pack", L._p(st), n, L._p(d_act), cycle, L._p(d_lim), pos_first, L._p(rew),
               pack.data_ptr() + 16, L._p(d_dist), n_roles, n_local, hof, pitch, first)
        got, gp = host(rew), host(pack)
        ec.assert_same(got[:n], want, f"coevo_mpe_final_step_pack rewards, cycle {cycle}")
        assert np.isnan(got[n]).all() and (gp[:2] == -7.0).all() and (gp[-2:] == -7.0).all()
        want_pack = np.zeros((n_roles, n_local, 4))
        want_pack[..., :3] = want[:n_roles * n_local * hof].reshape(n_roles, n_local, hof, 3)[:, :, hof - 1]
        want_pack[..., 3] = dist[:, first:first + n_local].astype(np.float64)
        ec.assert_same(gp[2:-2].reshape(n_roles, n_local, 4), want_pack, f"pack, cycle {cycle} hof {hof}")
        ec.assert_same(host(st), state, "the state after coevo_mpe_final_step_pack")


# ================================================================================================ e. fused fp32 routes
def crafted_games(n_games, seed):
    """{game: (class, goal, apos, vel, lpos)} for one game of every three, the finite classes in turn; the game's place in its
    triple moves on with every round of the classes, so a class meets another limit of a g % 3 pattern each time"""
    g = np.random.Generator(np.random.PCG64(seed))
    out = {}
    for i in range(n_games // 3):
        name = ec.FUSED_CLASSES[i % len(ec.FUSED_CLASSES)]
        out[3 * i + (i + i // len(ec.FUSED_CLASSES)) % 3] = (name, *ec.craft(name, g))
    return out


def columns_of(crafted):
    """{game: the [STATE_DOUBLES] state column of its crafted state}"""
    return {game: ec.lay_out([goal], apos[None], lpos[None], vel[None])[:, 0] for game, (_, goal, apos, vel, lpos) in crafted.items()}


def pokes_of(crafted):
    """{game: f(MpeState)}: the same states for rp.play_game_steps / ck.play_game_steps"""
    def poke(goal, apos, vel, lpos):
        def f(s):
            for a in range(3):
                for k in range(2):
                    s.ppos[a][k], s.pvel[a][k] = apos[a, k], vel[a, k]
            for l in range(2):
                for k in range(2):
                    s.lm[l][k] = lpos[l, k]
            s.goal = goal
        return f
    return {game: poke(goal, apos, vel, lpos) for game, (_, goal, apos, vel, lpos) in crafted.items()}


def fused_limits(n_games, n_cycles):
    """agent-step limits of a whole-game run of n cycles, shuffled: ends inside the last cycle (3n, 3n - 1, 3n - 2), on the
    boundary in front of it (3n - 3), and limits 2, 5, 3n - 4 = 3k + 2, at which agent_1 of cycle k is the first seat that no
    longer acts: the `t0 + 2 < limit` edge of mpe_fused_observe's `stepped` in a cycle that is still observed; 1 and 4 beside"""
    n = n_cycles
    choices = np.array([3 * n, 3 * n - 1, 3 * n - 2, 3 * n - 4, 5, 2, 3 * n - 3, 1, 4])
    assert (choices >= 1).all() and {2, 5, 3 * n - 4} <= {3 * k + 2 for k in range(n - 1)}
    g = np.random.Generator(np.random.PCG64([n_games, n_cycles]))
    return choices[np.arange(n_games) % len(choices)][g.permutation(n_games)]


@pytest.mark.parametrize("pos_first", [1, 0])
@pytest.mark.parametrize("form", fe.FORMS)
def test_fused_routes_play_crafted_states(form, pos_first):
    """every fp32 rollout form (mpe_fused_observe -> mpe_world_step / mpe_world_move in the fused ones): a third of the games
    start from a finite crafted state (far field x 1e4, agent on the goal, mirrored agents, coincident agents, subnormal
    observations, subnormal velocities, -0.0, velocity 1e3), ragged limits (fused_limits), both integration orders - status, rewards of every
    game and the last action words are the oracle's.  pos_first = 0 runs without the cached graphs (captured with 1)"""
    s = fe.setup(form)
    fe.install(s)
    crafted = crafted_games(s.plan.n_games, seed=51)
    first, limits = 61, fused_limits(s.plan.n_games, s.n_cycles)
    met = {name: {int(limits[g]) for g, c in crafted.items() if c[0] == name} for name in ec.FUSED_CLASSES}
    assert all(len(v) >= 2 for v in met.values()), met
    O, ro = rp.lib(), s.ro
    keep = (ro.pos_first, ro.desc.pos_first, ro.use_graph)
    try:
        if pos_first == 0:
            O.oracle_mpe_set_pos_first(0)
            ro.pos_first, ro.desc.pos_first, ro.use_graph = 0, 0, False
            # every game step by step: the module's game cache holds pos_first = 1 games and must not take these
            want, want_status, acts = fe.oracle_games(s, first, limits, s.n_cycles, poke=pokes_of(crafted),
                                                      choose=lambda g, slot, lg, a: a, affected=lambda g: True)
        else:
            want, want_status, acts = fe.oracle_games(s, first, limits, s.n_cycles, poke=pokes_of(crafted))
        assert want_status == 0 and np.isfinite(want).all()
        got, status, last = fe.run(s, form, first, limits, poke_game=columns_of(crafted))
    finally:
        O.oracle_mpe_set_pos_first(1)
        ro.pos_first, ro.desc.pos_first, ro.use_graph = keep
    what = f"{form} crafted states pos_first {pos_first}"
    assert status == want_status, f"{what}: status word {status:#x}"
    fe.assert_games(got, want, what)
    reached = [g for g, a in enumerate(acts) if a]   # the games whose limit lets a seat act in the last cycle
    assert len(reached) >= s.plan.n_games // 3
    fe.assert_last_actions(last[reached], [acts[g] for g in reached], what)


# ================================================================================================ f. fp16 cycle kernel
@pytest.mark.parametrize("pos_first", [1, 0])
def test_fp16_cycle_kernel_plays_crafted_states(pos_first):
    """coevo_mpe16_policy_cycle stepped cycle by cycle (tests/test_fp16_rollout_gpu.Stepper): the finite crafted states
    written into the first state buffer after construction, limits None, 1, 2, 3, 4, T - 1, T side by side - every action of
    every game and the final rewards against the checker's stepwise game; canary game and padding rows as the Stepper asserts"""
    flats, flats10, flats8, tasks, games = f16.build_mixed(13)
    T = 3 * f16.MAXC
    choices = (None, 1, 2, 3, 4, T - 1, T)
    limits = [choices[(3 * g + g // 7) % len(choices)] for g in range(len(games))]
    assert set(limits) == set(choices)
    crafted = crafted_games(len(games), seed=71)
    for i, g in enumerate(sorted(crafted)):   # every class plays a whole game, then one that ends inside the last cycle
        limits[g] = (None, T - 1, 4)[i // len(ec.FUSED_CLASSES)]
    assert set(limits) == set(choices)
    assert {(c[0], limits[g]) for g, c in crafted.items()} >= {(name, lim) for name in ec.FUSED_CLASSES for lim in (None, T - 1)}
    first, pokes, stream = 19, pokes_of(crafted), rp.Stream()
    rp.lib().oracle_mpe_set_pos_first(pos_first)
    try:
        want = []
        for g, (adv, a0, a1) in enumerate(games):
            if g in pokes:
                want.append(ck.play_game_steps(stream, flats[a0], flats[a1], flats[adv], limits[g], f16.MAXC, ordinal=first + g,
                                               poke=pokes[g]))
            else:
                want.append(ck.play_game(stream, flats[a0], flats[a1], flats[adv], limits[g], f16.MAXC, ordinal=first + g))
    finally:
        rp.lib().oracle_mpe_set_pos_first(1)
    assert all(w["status"] == 0 for w in want)
    slab, off, Ds = f16.pack16(flats10, flats8)
    s = f16.Stepper(slab, off, Ds, tasks, len(games), limits, first, pos_first)
    cols = columns_of(crafted)
    idx = torch.tensor(sorted(cols), dtype=torch.int64, device=DEV)
    s.state2[0].index_copy_(1, idx, dev(np.stack([cols[g] for g in sorted(cols)], axis=1)))
    s.play_and_compare(want, f16.MAXC)
    assert int(s.status.item()) == 0
