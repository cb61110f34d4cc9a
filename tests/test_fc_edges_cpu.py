"""The adversarial net library (tests/fc_edge_nets.py) against the CPU oracle alone: what oracle_fc_forward and
oracle_play_game say about ties, signed zeros, infinities, NaN, a variance of zero and subnormal weights.  These are the
expected values of tests/test_fc_forward_edges_gpu.py; the reference raises ValueError on the fault classes
(MPE/fcnetwork.py:39-65, 87).  No GPU."""
import numpy as np
import pytest

from oracle import ref_port as rp
from tests import fc_edge_nets as E


def rng(*key):
    return np.random.Generator(np.random.PCG64(list(key)))


@pytest.mark.parametrize("D", [8, 10])
@pytest.mark.parametrize("name", sorted(E.CLASSES))
def test_class_has_its_property(name, D):
    """status word and action of every class, for several nets and observations"""
    want_st, want_a = E.PROPERTY[name]
    for seed in range(3):
        w = E.make(name, D, seed)
        for obs in rng(D, seed).uniform(-2, 2, size=(5, D)).astype(np.float32):
            a, lg, st = rp.fc_forward(w, D, obs)
            assert st == want_st, (name, D, seed, st)
            if want_a is not None:
                assert a == want_a, (name, D, seed, a, lg)
            if name in E.TIES:
                top = lg.view(np.uint32)[lg == lg.max()]
                assert len(top) == (5 if name == "tie5" else 2) and len(set(top.tolist())) == 1
                assert E.last_maximum(lg) != a == int(np.argmax(lg))
            if name == "signed_zeros":
                assert np.array_equal(lg.view(np.uint32), np.array([-0.0, 0.0, -0.0, 0.0, 0.0], np.float32).view(np.uint32))
            if name == "all_neg_inf":
                assert np.all(lg == -np.inf)
            if name == "one_pos_inf":
                assert lg[2] == np.inf and np.isfinite(np.delete(lg, 2)).all()
            if name == "one_nan_logit":
                assert np.isnan(lg[0]) and a == 1 + int(np.argmax(lg[1:]))
            if E.PROPERTY[name][0] & (E.BAD_FC1 | E.BAD_FC2) or name == "all_nan_logits":
                assert np.isnan(lg).all()


@pytest.mark.parametrize("D", [8, 10])
@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_non_finite_observation(D, bad):
    """one non-finite input column: every bit of the status word; the columns past D are not inputs"""
    w = E.make("plain", D)
    obs = rng(D).uniform(-2, 2, size=D).astype(np.float32)
    for k in (0, D // 2, D - 1):
        o = obs.copy()
        o[k] = bad
        a, lg, st = rp.fc_forward(w, D, o)
        assert (a, st) == (-1, E.BAD_OBS_STATUS) and np.isnan(lg).all()
    wide = np.concatenate([obs, np.full(12 - D, bad, dtype=np.float32)])
    a, lg, st = rp.fc_forward(w, D, wide)
    a0, lg0, st0 = rp.fc_forward(w, D, obs)
    assert st == st0 == 0 and a == a0 and np.array_equal(lg.view(np.uint32), lg0.view(np.uint32))


@pytest.mark.parametrize("D", [8, 10])
@pytest.mark.parametrize("name", sorted(E.SUBNORMAL))
def test_subnormal_classes_have_teeth(name, D):
    """a unit that flushed the class' subnormal weights to zero would give other logits and another action"""
    w = E.make(name, D)
    t = E.view(w, D, E.SUBNORMAL[name])
    assert (np.abs(t) < E.MIN_NORMAL).all() and np.count_nonzero(t) > 0.99 * t.size
    wf = E.flushed(w, D, name)
    obs = E.observations(rng(D, 3), 6, D, name, w)
    assert obs.shape == (6, D)
    for o in obs:
        (a, lg, st), (af, lf, sf) = rp.fc_forward(w, D, o), rp.fc_forward(wf, D, o)
        assert st == sf == 0 and a != af and not np.array_equal(lg.view(np.uint32), lf.view(np.uint32))
        assert np.isfinite(lg).all() and lg.any()
    if name == "subnormal_fc2":   # flushed: fc2 gives exact zeros, so does everything after it
        assert not lf.any() and af == 0 and np.abs(lg).max() < 1e-5


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


@pytest.mark.parametrize("limit,max_cycles", [(13, 5), (None, 4), (0, 3), (1, 25), (7, 25)])
def test_play_game_steps_equals_the_c_loop(limit, max_cycles):
    """the Python restatement of oracle_play_game's loop (the hook for a poked state / another argmax rule) is that loop"""
    stream = rp.Stream()
    for trio in (("plain", "plain", "plain"), ("tie2", "tie5", "tie2_04"), ("plain", "all_nan_logits", "plain"),
                 ("one_nan_logit", "plain", "nan_in_fc1")):
        a0, a1, adv = E.make(trio[0], 10, 1), E.make(trio[1], 10, 2), E.make(trio[2], 8, 3)
        x = rp.play_game_status(stream, a0, a1, adv, limit, max_cycles, ordinal=9)
        y = rp.play_game_steps(stream, a0, a1, adv, limit, max_cycles, ordinal=9)
        for k in ("rewards", "steps", "actions", "status"):
            assert x[k] == y[k], (trio, k, x[k], y[k])
        assert np.isfinite(x["rewards"]).all()   # a faulted seat plays action 0 or its surviving maximum: physics stays finite


def test_play_game_status_and_the_raising_form():
    stream = rp.Stream()
    a0, a1, adv = E.make("plain", 10, 1), E.make("nan_in_fc2", 10, 2), E.make("one_pos_inf", 8, 3)
    g = rp.play_game_status(stream, a0, a1, adv, 13, 5, ordinal=4)
    assert g["status"] == E.PROPERTY["nan_in_fc2"][0] | E.PROPERTY["one_pos_inf"][0]
    assert g["actions"][0::3] == [2] * 5 and g["actions"][2::3] == [0] * 4   # +inf logit 2 survives; no action -> 0
    with pytest.raises(ValueError, match=f"status {g['status']}"):
        rp.play_game(stream, a0, a1, adv, 13, 5, ordinal=4)
    ok = rp.play_game(stream, a0, a0, E.make("plain", 8, 3), 13, 5, ordinal=4)
    assert "status" not in ok and ok["steps"] == 13
    assert rp.play_game_status(stream, a0, a1, adv, 1, 5, ordinal=4)["status"] == E.BAD_OUT   # only the adversary acted


def test_tie_games_tell_the_first_maximum_from_the_last():
    """a game with a tie net in a seat takes another course when that seat takes the LAST maximum"""
    stream = rp.Stream()
    plain10, plain8 = E.make("plain", 10, 1), E.make("plain", 8, 2)
    for slot, name in ((0, "tie2"), (0, "tie5"), (1, "tie2_04"), (2, "tie2_23"), (2, "tie5")):
        nets = [plain8, plain10, plain10]
        nets[slot] = E.make(name, 8 if slot == 0 else 10, 5)
        adv, a0, a1 = nets
        first = rp.play_game_steps(stream, a0, a1, adv, 40, 25, ordinal=6)
        last = rp.play_game_steps(stream, a0, a1, adv, 40, 25, ordinal=6,
                                  choose=lambda s, lg, a: E.last_maximum(lg) if s == slot else a)
        assert first["status"] == last["status"] == 0
        assert first["actions"][slot::3] != last["actions"][slot::3] and first["rewards"] != last["rewards"], (slot, name)
