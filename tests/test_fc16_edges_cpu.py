"""The float16 adversarial net library (tests/fc16_edge_nets.py) against the C checker alone (tests/checker16/fc16_checker.c):
what fc16_forward and the checker's games say about ties, signed zeros, infinities, NaN, a variance of zero, fp16 subnormal
weights, the fp16 rounding points of LayerNorm and of the output chain, and the net that faults only on a padding row.  These
are the expected values of tests/test_fc16_forward_edges_gpu.py, and per class the teeth: what a plausible wrong kernel (last
maximum, flushed subnormals, another rounding, a padding row in the status) would answer instead.  No GPU."""
import numpy as np
import pytest

from oracle import ref_port as rp
from tests import fc16_edge_nets as E
from tests import fp16_checker as ck


def rng(*key):
    return np.random.Generator(np.random.PCG64(list(key)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_checker_rounding_is_numpys():
    """the judge's own f16(): every rounding point the library leans on, and 20000 random words, against numpy"""
    g = rng(1)
    x = np.concatenate([E.LN_VALS, E.LN_VALS_INF, -E.LN_VALS, np.float32([0.0, -0.0, 65504, 65519.99, 65520, 70000, 2.0 ** -14,
                        2.0 ** -14 - 2.0 ** -26, 2.0 ** -24, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, np.inf, -np.inf]),
                        g.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    x = x[~np.isnan(x)]
    with np.errstate(over="ignore"):
        assert np.array_equal(ck.f16_bits(x), x.astype(np.float16).view(np.uint16))


@pytest.mark.parametrize("D", [8, 10])
@pytest.mark.parametrize("name", sorted(E.CLASSES))
def test_class_has_its_property(name, D):
    """status word and action of every class, for several nets and observations"""
    want_st, want_a = E.PROPERTY[name]
    for seed in range(3):
        w = E.make(name, D, seed)
        m = E.linear_mask(D)
        assert E.same_bits_up_to_nan(w[m], E.f16(w[m])), "Linear entries are fp16 values"
        for obs in rng(D, seed).uniform(-2, 2, size=(5, D)).astype(np.float32):
            a, lg, st = ck.forward(w, D, obs)
            assert st == want_st, (name, D, seed, st)
            if want_a is not None:
                assert a == want_a, (name, D, seed, a, lg)
            if name in E.TIES:   # teeth: a `>=` scan would answer another action
                top = bits(lg)[lg == lg.max()]
                assert len(top) == E.TIES[name] and len(set(top.tolist())) == 1
                assert E.last_maximum(lg) != a == int(np.argmax(lg))
            if name == "signed_zeros":
                assert np.array_equal(bits(lg), bits([-0.0, 0.0, -0.0, 0.0, 0.0]))
            if name == "all_neg_inf":
                assert np.all(lg == -np.inf)
            if name == "one_pos_inf":
                assert lg[2] == np.inf and np.isfinite(np.delete(lg, 2)).all()
            if name == "one_nan_logit":   # teeth: a scan that let NaN win (or stop it) would not find the maximum of the four
                rest = np.delete(lg, 2)
                assert np.isnan(lg[2]) and np.isfinite(rest).all() and a == (0, 1, 3, 4)[int(np.argmax(rest))]
            if name == "ln_rounding_inf":
                assert np.isnan(lg[:4]).all() and lg[4] == np.inf
            if name == "ln_rounding":
                with np.errstate(over="ignore"):
                    want = E.LN_VALS.astype(np.float16)
                assert np.array_equal(lg.astype(np.float16).view(np.uint16), want.view(np.uint16))
                assert np.array_equal(bits(lg), bits(np.float32([1.0, 1 + 2.0 ** -9, 0.0, 2.0 ** -23, 65504.0])))
            if want_st & (E.BAD_FC1 | E.BAD_FC2) and name != "ln_rounding_inf" or name == "all_nan_logits":
                assert np.isnan(lg).all()


@pytest.mark.parametrize("D", [8, 10])
def test_bare_gamma_inf_would_not_be_a_fault_class(D):
    """why gamma_inf pins feature 7 above the mean: with ln1.weight[7] = inf alone the fault depends on the sign of
    x[7] - mean, and the ReLU swallows -inf - the class would be healthy on about half of the rows"""
    seen = set()
    for seed in range(6):
        w = E.make("plain", D, seed)
        E.view(w, D, "ln1.weight")[7] = np.inf
        for obs in rng(D, seed, 1).uniform(-2, 2, size=(4, D)).astype(np.float32):
            seen.add(ck.forward(w, D, obs)[2])
    assert seen == {0, E.PROPERTY["gamma_inf"][0]}


@pytest.mark.parametrize("D", [8, 10])
@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan, 65520.0])
def test_non_finite_observation(D, bad):
    """one input column that is not finite AFTER the fp16 rounding: every bit of the status word; columns past D are no inputs"""
    w = E.make("plain", D)
    obs = rng(D).uniform(-2, 2, size=D).astype(np.float32)
    for k in (0, D // 2, D - 1):
        o = obs.copy()
        o[k] = bad
        a, lg, st = ck.forward(w, D, o)
        assert (a, st) == (-1, E.BAD_OBS_STATUS) and np.isnan(lg).all()
    wide = np.concatenate([obs, np.full(12 - D, bad, dtype=np.float32)])
    a, lg, st = ck.forward(w, D, wide)
    a0, lg0, st0 = ck.forward(w, D, obs)
    assert st == st0 == 0 and a == a0 and np.array_equal(bits(lg), bits(lg0))


@pytest.mark.parametrize("D", [8, 10])
@pytest.mark.parametrize("name", sorted(E.SUBNORMAL))
def test_subnormal_classes_have_teeth(name, D):
    """a unit that flushed the class' fp16 subnormal weights to zero would give other logit bits on the rows the GPU file uses"""
    w = E.make(name, D)
    t = E.view(w, D, E.SUBNORMAL[name])
    assert (np.abs(t) < E.MIN_NORMAL16).all() and (t != 0).all() and np.array_equal(bits(t), bits(E.f16(t)))
    wf = E.flushed(w, D, name)
    obs = E.observations(rng(D, 3), 6, D, name, w)
    assert obs.shape == (6, D)
    for o in obs:
        (a, lg, st), (af, lf, sf) = ck.forward(w, D, o), ck.forward(wf, D, o)
        assert st == sf == 0 and not np.array_equal(bits(lg), bits(lf)) and np.isfinite(lg).all()


def test_rounding_helpers():
    x = np.float32([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 1.5 * 2.0 ** -11, 1.0, -1 - 2.0 ** -11, 2.0 ** -25, 3 * 2.0 ** -25,
                    65519.996, 0.3])
    assert np.array_equal(E.f16(x), np.float32([1, 1 + 2.0 ** -9, 1 + 2.0 ** -10, 1, -1, 0, 2.0 ** -23, 65504, np.float16(0.3)]))
    assert np.array_equal(E.round_toward_zero16(x), np.float32([1, 1 + 2.0 ** -10, 1, 1, -1, 0, 2.0 ** -24, 65504,
                                                                np.nextafter(np.float16(0.3), np.float16(0))]))
    assert np.array_equal(E.round_half_up16(x), np.float32([1 + 2.0 ** -10, 1 + 2.0 ** -9, 1 + 2.0 ** -10, 1, -1 - 2.0 ** -10,
                                                            2.0 ** -24, 2.0 ** -23, 65504, np.float16(0.3)]))


def test_rounding_classes_have_teeth():
    """ln_rounding: its logits ARE f16(LN_VALS), and truncation / half-up give other words.  out_rounding: logit 1 is
    f16(1 + k 2^-11) beside logit 0 = 1, and the first maximum of that pair is the action - half-up flips k = 1, truncation
    flips k = 1.5 (and only changes the logit of k = 3)"""
    rne = E.f16(E.LN_VALS)
    assert not np.array_equal(bits(E.round_toward_zero16(E.LN_VALS)), bits(rne))
    assert not np.array_equal(bits(E.round_half_up16(E.LN_VALS)), bits(rne))
    got = {}
    for name, k in (("out_rounding", 1), ("out_rounding_up", 3), ("out_rounding_near", 1.5)):
        x = np.float32(1.0) + np.float32(k * 2.0 ** -11)   # exact in fp32: what the fmaf chain holds before the rounding
        for D in (8, 10):
            w = E.make(name, D)
            assert E.view(w, D, "output.weight")[1][0] == np.float32(k * 2.0 ** -11)
            a, lg, st = ck.forward(w, D, rng(D, 2).uniform(-2, 2, D).astype(np.float32))
            assert st == 0 and lg[0] == 1 and bits(lg[1]) == bits(E.f16(x)) and (lg[2:] == -1000).all()
            assert a == int(lg[1] > lg[0]) == E.PROPERTY[name][1]
        got[name] = tuple(int(r(x) > 1) for r in (E.f16, E.round_toward_zero16, E.round_half_up16))
    assert got == {"out_rounding": (0, 0, 1), "out_rounding_up": (1, 1, 1), "out_rounding_near": (1, 0, 1)}
    assert E.round_toward_zero16(np.float32(1 + 3 * 2.0 ** -11)) != E.f16(np.float32(1 + 3 * 2.0 ** -11))


@pytest.mark.parametrize("D", [8, 10])
@pytest.mark.parametrize("name", sorted(E.PAD_FAULT_ZERO_ROW))
def test_pad_fault_faults_on_the_zero_row_only(name, D):
    """teeth: the all-zero observation that pads a partial pass raises BAD_FC2 | BAD_OUT | NO_ACTION (pad_fault_fc1: BAD_FC1 as
    well, out of LayerNorm(512)); observations of 200 draws each of uniform(-a, a), a = 3, 1, 0.1, 0.01, are all clean; at
    a = 1e-3 every draw of pad_fault is faulty (so: no tiny rows)"""
    for seed in range(2):
        w = E.make(name, D, seed)
        assert ck.forward(w, D, np.zeros(D, dtype=np.float32))[2] == E.PAD_FAULT_ZERO_ROW[name] != 0
        for a in (3, 1, 0.1, 0.01):
            n = 200 if seed == 0 else 20
            assert all(ck.forward(w, D, o)[2] == 0 for o in rng(D, seed, 7).uniform(-a, a, size=(n, D)).astype(np.float32)), a
        tiny = [ck.forward(w, D, o)[2] != 0 for o in rng(D, seed, 8).uniform(-1e-3, 1e-3, size=(20, D)).astype(np.float32)]
        assert all(tiny) if name == "pad_fault" else not any(tiny)   # (pad_fault_fc1 turns faulty only below about 1e-4)


def test_same_bits_up_to_nan():
    f = np.float32
    a = np.array([0.0, -0.0, np.inf, np.nan, 1.5], dtype=f)
    assert E.same_bits_up_to_nan(a, a.copy())
    other_nan = a.copy()
    other_nan.view(np.uint32)[3] = 0xFFC00001
    assert np.isnan(other_nan[3]) and E.same_bits_up_to_nan(a, other_nan)
    for i, v in ((0, -0.0), (1, 0.0), (2, -np.inf), (3, 1.0), (4, np.nan), (4, np.nextafter(f(1.5), f(2)))):
        b = a.copy()
        b[i] = v
        assert not E.same_bits_up_to_nan(a, b), (i, v)
    assert E.last_maximum([1.0, 3.0, np.nan, 3.0, 2.0]) == 3 and E.last_maximum([np.nan] * 5) == -1


@pytest.mark.parametrize("limit,max_cycles", [(13, 5), (None, 4), (1, 25), (7, 25)])
def test_play_game_steps_equals_the_c_loop(limit, max_cycles):
    """the Python restatement of fc16_play_game's loop (the hook for a poked state) is that loop, faulted seats included"""
    stream = rp.Stream()
    for trio in (("plain", "plain", "plain"), ("tie2", "tie5", "tie2_04"), ("plain", "all_nan_logits", "out_rounding"),
                 ("one_nan_logit", "pad_fault", "gamma_inf"), ("pad_fault_fc1", "plain", "pad_fault_fc1")):
        a0, a1, adv = E.make(trio[0], 10, 1), E.make(trio[1], 10, 2), E.make(trio[2], 8, 3)
        x = ck.play_game(stream, a0, a1, adv, limit, max_cycles, ordinal=9)
        y = ck.play_game_steps(stream, a0, a1, adv, limit, max_cycles, ordinal=9)
        for k in ("rewards", "steps", "actions", "status"):
            assert x[k] == y[k], (trio, k, x[k], y[k])
        assert np.isfinite(x["rewards"]).all()   # a faulted seat plays action 0 or its surviving maximum: physics stays finite


@pytest.mark.parametrize("bad", [np.inf, np.nan])
def test_a_poked_state_raises_bad_input_in_the_checkers_game(bad):
    """one entry of a game's state set to inf / NaN after the reset: the checker's own game reports BAD_INPUT (and, the rows that
    observe it being NaN throughout, the four bits behind it); without the poke the same game is clean"""
    stream = rp.Stream()
    a0, a1, adv = E.make("plain", 10, 1), E.make("tie2", 10, 2), E.make("plain", 8, 3)

    def poke(s):
        s.ppos[0][0] = bad

    clean = ck.play_game_steps(stream, a0, a1, adv, None, 3, ordinal=4)
    got = ck.play_game_steps(stream, a0, a1, adv, None, 3, ordinal=4, poke=poke)
    assert clean["status"] == 0 and got["status"] & E.BAD_INPUT and got["status"] == E.BAD_OBS_STATUS
    assert got["steps"] == clean["steps"] == 9


def test_tie_and_rounding_games_show_the_first_maximum():
    """in a game the tie / out_rounding seats play their class' action at every step: the checker's action list shows it"""
    stream = rp.Stream()
    g = ck.play_game(stream, E.make("tie2_23", 10, 1), E.make("out_rounding", 10, 2), E.make("tie3", 8, 3), None, 4, ordinal=2)
    assert g["status"] == 0 and set(g["actions"][0::3]) == {1} and set(g["actions"][1::3]) == {2} and set(g["actions"][2::3]) == {0}
