"""The adversarial float16 DeepQN net library (tests/dqn16_edge_nets.py) against the C checker alone (tests/checker16/
dqn16_checker.c): what every class means on the checker's stages, that every (site, mode) rounding pair has teeth - the checker
with ONE conversion site rounding wrongly differs from the contract in a word the GPU leaves behind - that the three quotient
pairs which cannot differ really cannot, and that dqn16_forward_stages without a variant is dqn16_forward.  These are the
expected values of tests/test_dqn16_forward_edges_gpu.py and the conditions without which that file could pass vacuously.  The
variants are wrong kernels on paper; nothing on a GPU is mutated.  No GPU.

About 13 ms per checker forward; the file makes some 700 of them, a part on a few threads."""
import numpy as np
import pytest

from tests import dqn16_checker as ck
from tests import dqn16_edge_nets as E
from tests import fc16_edge_nets as F16

FULL = [(4, 6), (6, 18)]
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def release_nets():
    yield
    E.release()


def u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def differ(a, b):
    return not E.same_bits_up_to_nan(np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32))


# ------------------------------------------------------------------------------------------- the checker's new entry point
def test_rounding_modes_value_by_value():
    """the five conversions on the values the constructions rest on"""
    x = F32([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -12, 2.0 ** -15, 2.0 ** -25, 3 * 2.0 ** -25, 65519.0, 65520.0, 70000.0,
             -65520.0, -(1 + 2.0 ** -11), -(2.0 ** -15), np.inf, -np.inf, 0.0, -0.0, 1.0009765625])
    want = {"nearest_even": [1, 1 + 2.0 ** -9, 1, 2.0 ** -15, 0, 2.0 ** -23, 65504, np.inf, np.inf, -np.inf, -1, -(2.0 ** -15), np.inf,
                             -np.inf, 0.0, -0.0, 1.0009765625],
            "toward_zero": [1, 1 + 2.0 ** -10, 1, 2.0 ** -15, 0, 2.0 ** -24, 65504, 65504, 65504, -65504, -1, -(2.0 ** -15), np.inf,
                            -np.inf, 0.0, -0.0, 1.0009765625],
            "ties_away": [1 + 2.0 ** -10, 1 + 2.0 ** -9, 1, 2.0 ** -15, 2.0 ** -24, 2.0 ** -23, 65504, np.inf, np.inf, -np.inf,
                          -(1 + 2.0 ** -10), -(2.0 ** -15), np.inf, -np.inf, 0.0, -0.0, 1.0009765625],
            "flush_results": [1, 1 + 2.0 ** -9, 1, 0.0, 0, 0.0, 65504, np.inf, np.inf, -np.inf, -1, -0.0, np.inf, -np.inf, 0.0, -0.0,
                              1.0009765625],
            "saturate": [1, 1 + 2.0 ** -9, 1, 2.0 ** -15, 0, 2.0 ** -23, 65504, 65504, 65504, -65504, -1, -(2.0 ** -15), np.inf,
                         -np.inf, 0.0, -0.0, 1.0009765625]}
    for mode in ck.MODES:
        assert np.array_equal(u32(ck.round_mode(x, mode)), u32(F32(want[mode]))), mode
    assert all(np.isnan(ck.round_mode(F32([np.nan]), mode)[0]) for mode in ck.MODES)
    with np.errstate(over="ignore"):
        g = np.random.default_rng(1).normal(0, 1, 2000).astype(np.float32) * F32(10.0) ** np.random.default_rng(2).integers(-9, 6, 2000)
        assert np.array_equal(u32(ck.round_mode(g, "nearest_even")), u32(g.astype(np.float16).astype(np.float32)))
        assert np.array_equal(u32(ck.round_mode(g, "toward_zero")), u32(F16.round_toward_zero16(g)))
        assert np.array_equal(u32(ck.round_mode(g, "ties_away")), u32(F16.round_half_up16(g)))


def test_the_three_quotient_pairs_are_vacuous():
    """all 256 bytes: the fp32 quotient u8 / 255 is never an fp16 midpoint, never rounds to a subnormal or past 65504, so
    ties_away, flush_results and saturate at the quotient equal the contract for every frame there is; toward_zero does not.
    The fp32 quotient also rounds to the half the exact quotient rounds to; 254 of the 256 quotients are inexact halves"""
    q = (np.arange(256, dtype=np.float32) / F32(255.0)).astype(np.float32)
    contract = ck.round_mode(q, "nearest_even")
    for site, mode in E.VACUOUS:
        assert site == "quotient" and np.array_equal(u32(ck.round_mode(q, mode)), u32(contract)), mode
    assert len(E.VACUOUS) == 3 and differ(ck.round_mode(q, "toward_zero"), contract)
    assert (contract[1:] >= E.MIN_NORMAL16).all() and contract.max() == 1.0
    exact = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float16).astype(np.float32)
    assert np.array_equal(u32(exact), u32(contract))
    assert int((contract.astype(np.float64) * 255.0 != np.arange(256)).sum()) == 254
    mid = (contract.astype(np.float64) + np.nextafter(contract.astype(np.float16), np.float16(2)).astype(np.float64)) / 2
    assert not (q.astype(np.float64) == mid).any()


@pytest.mark.parametrize("C,n", E.SHAPES)
def test_plain_stages_equal_dqn16_forward(C, n):
    """no variant selected: logits, action and status of dqn16_forward bit for bit, on healthy and faulty rows; the stages hold fp16
    values, the rectified ones nothing negative"""
    for name, fname in (("plain", "random"), ("plain", "zeros"), ("tie2", "full"), ("nan_conv2.weight", "random"),
                        ("all_neg_inf", "planes"), ("fc1_rounding", "hot_last"), ("conv1_saturate", "lit")):
        w, f = E.make(name, C, n), E.frame(C, fname)
        a, lg, st = ck.forward(w, C, n, f)
        s = ck.stages(w, C, n, f)
        assert (s["action"], s["status"]) == (a, st) and np.array_equal(u32(s["logits"]), u32(lg)), (name, fname)
        assert s is not None and np.array_equal(u32(E.checker(w, f, C, n)["logits"]), u32(lg))
        with np.errstate(over="ignore", invalid="ignore"):
            for k in ck.STAGES:
                assert np.array_equal(u32(s[k]), u32(s[k].astype(np.float16).astype(np.float32))) or np.isnan(s[k]).any(), k
        if st == 0 and name == "plain":
            assert all((s[k] >= 0).all() for k in ("x", "a1", "a2", "a3", "hid")) and (s["s1"] < 0).any()


# ------------------------------------------------------------------------------------------- the classes
@pytest.mark.parametrize("C,n", FULL)
def test_class_has_its_property(C, n):
    """every class on the random frame (the conv1 one-tap classes on the lit frame as well): the action where PROPERTY fixes it, the
    NaN pattern of the logits, the status, and what makes the class an edge; every entry of every net an fp16 value"""
    names = sorted(E.CLASSES)
    assert set(E.PROPERTY) == set(names) and len(names) >= 60
    got = E.checker_many([(E.make(name, C, n), E.frame(C, "random")) for name in names], C, n)
    for name, s in zip(names, got):
        w = E.make(name, C, n)
        with np.errstate(over="ignore", invalid="ignore"):
            assert E.same_bits_up_to_nan(w, w.astype(np.float16).astype(np.float32)), f"{name}: an entry that is no fp16 value"
        want_a, want_nan, want_st = E.PROPERTY[name]
        a, lg, st = (-1 if s["status"] & E.NO_ACTION else s["action"]), s["logits"], s["status"]
        what = (name, C, n, a, lg, st)
        if want_a is not None:
            assert a == (want_a if want_a >= -1 else n + want_a), what
        if want_st is not None:
            assert st == want_st, what
        assert st in (0, E.NO_ACTION) and (st == 0 or s["action"] == 0), what
        nans = int(np.isnan(lg).sum())
        if want_nan is not None:
            assert nans == {"all": n, "one": 1, "none": 0}[want_nan], what
        if want_nan == "one":
            rest = np.where(np.isnan(lg), -np.inf, lg)
            assert a == int(np.argmax(rest)) and not np.isnan(lg[a]), what
        if name in E.TIES:
            top = u32(lg)[lg == lg.max()]
            assert len(top) == (n if name == "tie_all" else 2) and len(set(top.tolist())) == 1, what
            assert E.last_maximum(lg) != a == int(np.argmax(lg)), what
        if name == "signed_zeros":
            assert np.array_equal(u32(lg), u32(np.where(np.arange(n) % 2 == 0, -0.0, 0.0))), what
        if name == "all_neg_inf":
            assert np.all(lg == -np.inf), what
        if name == "one_pos_inf":
            assert lg[2] == np.inf and np.isfinite(np.delete(lg, 2)).all(), what
        if name == "inf_output.weight":
            assert not np.isfinite(lg).all(), what
        if name.endswith("_below"):
            assert np.isfinite(lg).all() and np.isfinite(s["act"]).all(), what
    assert all(E.PROPERTY[name][2] == 0 for name in E.QUIET if E.PROPERTY[name][2] is not None) and len(E.FAULTY) >= 24
    assert set(E.OUTPUT_SENSITIVE) <= set(names)


@pytest.mark.parametrize("C,n", FULL)
def test_exact_constructions_of_fc1_and_the_output_layer(C, n):
    """fc1_rounding: a3 is 0.5 everywhere and every group's six hidden words are 1, 1 + 2^-9, 2^-15, 0, inf, 65504, whatever the
    frame; out_rounding[_first]: the same six words as logits, from hid = 0.5; each wrong mode changes exactly the words
    CHANGED_BY names; out_last_step and the rounding ties are what their docstrings say"""
    for fname in ("random", "full"):
        f = E.frame(C, fname)
        w = E.make("fc1_rounding", C, n)
        s = ck.stages(w, C, n, f)
        assert (s["a3"] == E.HALF_IN).all()
        for j0, k in E.FC1_GROUPS:
            assert np.array_equal(u32(s["hid"][j0:j0 + 6]), u32(E.GROUP_WORDS)), (j0, k)
        assert s["logits"][2] == np.inf and (np.delete(s["logits"], 2) == -np.inf).all()
        for mode, changed in E.CHANGED_BY.items():
            v = ck.stages(w, C, n, f, "fc1", mode)
            for j0, _ in E.FC1_GROUPS:
                assert sorted(np.flatnonzero(u32(v["hid"][j0:j0 + 6]) != u32(E.GROUP_WORDS)).tolist()) == list(changed), (mode, j0)
    f = E.frame(C, "random")
    for name in ("out_rounding", "out_rounding_first"):
        w = E.make(name, C, n)
        s = ck.stages(w, C, n, f)
        assert set(np.unique(s["hid"]).tolist()) == {0.0, 0.5} and len(E.out_groups(n)) == n // 6
        for i0, _ in E.out_groups(n):
            assert np.array_equal(u32(s["logits"][i0:i0 + 6]), u32(E.GROUP_WORDS)), (name, i0)
        for mode, changed in E.CHANGED_BY.items():
            v = ck.stages(w, C, n, f, "out", mode)
            for i0, _ in E.out_groups(n):
                assert sorted(np.flatnonzero(u32(v["logits"][i0:i0 + 6]) != u32(E.GROUP_WORDS)).tolist()) == list(changed), (mode, i0)
    # the critical weights sit where the issue of a fused conversion was: the chain's last step (k = 511), and at its first
    Wo = E.view(E.make("out_rounding", C, n), C, n, "output.weight")
    assert Wo[0, 511] != 0 and not Wo[0, :510].any() and E.view(E.make("out_rounding_first", C, n), C, n, "output.weight")[0, 0] != 0
    W1 = E.view(E.make("fc1_rounding", C, n), C, n, "fc1.weight")
    assert W1[0, 0] and W1[63, 3135] and W1[448, 1567] and W1[511, 3135] and np.count_nonzero(W1) == 7 * len(E.FC1_GROUPS)
    # out_last_step: the exact sum is above the midpoint, its fp32 rounding is the midpoint
    s = ck.stages(E.make("out_last_step", C, n), C, n, f)
    exact = 1.0 + float(E.LAST_STEP_HID) * float(E.LAST_STEP_W)
    assert s["hid"][511] == E.LAST_STEP_HID and exact == 1 + 2.0 ** -11 + 2.0 ** -25 and F32(exact) == F32(1 + 2.0 ** -11)
    assert np.float16(exact) == np.float16(1 + 2.0 ** -10) and s["logits"][1] == 1.0 == s["logits"][0] and s["action"] == 0
    # the rounding ties and the two wrong scans
    for name, scan_wrong, last_wrong in (("rounding_tie", 3, 3), ("rounding_tie_rev", 1, 3)):
        w = E.make(name, C, n)
        assert ck.stages(w, C, n, f)["action"] == 1
        assert ck.stages(w, C, n, f, scan="scan_before_rounding")["action"] == scan_wrong
        assert ck.stages(w, C, n, f, scan="last_maximum")["action"] == last_wrong
    for name in ("tie_all", "tie2", "tie2_0_last", "tie2_last2"):
        w = E.make(name, C, n)
        assert ck.stages(w, C, n, f, scan="last_maximum")["action"] != ck.stages(w, C, n, f)["action"], name


@pytest.mark.parametrize("C,n", FULL)
def test_conv1_one_tap_classes(C, n):
    """on the lit frame channels 3 and 19 hold f16(b) off the six lit positions and f16(b + w) on them - a proper subset, among
    them positions 0, 15 | 16, 383 | 384 and 399; on a frame without a lit tap the channels are constant and every mode is hidden"""
    f = E.frame(C, "lit")
    assert sorted(set(f.reshape(-1).tolist())) == [0, 255] and int((f == 255).sum()) == len(E.LIT_POSITIONS) == 6
    lit = np.zeros(400, dtype=bool)
    lit[list(E.LIT_POSITIONS)] = True
    want_lit = {"conv1_ties_away": 1.0, "conv1_flush": 2.0 ** -15, "conv1_saturate": np.inf, "conv1_below": 65504.0}
    for name, (b, wt) in E.CONV1_BW.items():
        w = E.make(name, C, n)
        s = ck.stages(w, C, n, f)
        for ch in E.LIT_CHANNELS:
            assert (s["s1"][ch][~lit] == F32(b)).all() and (s["s1"][ch][lit] == F32(want_lit[name])).all(), (name, ch)
        assert min(E.LIT_CHANNELS) < 16 <= max(E.LIT_CHANNELS)
        if name in ("conv1_ties_away", "conv1_below"):      # a constant channel: BatchNorm returns relu(beta)
            beta = E.view(w, C, n, "vbn1.bias")
            for ch in E.LIT_CHANNELS:
                assert (s["a1"][ch] == max(beta[ch], 0)).all()
        if name == "conv1_saturate":
            assert np.isnan(s["logits"]).all() and s["status"] == E.NO_ACTION
            z = ck.stages(w, C, n, E.frame(C, "zeros"))
            assert z["status"] == 0 and not differ(z["logits"], ck.stages(w, C, n, E.frame(C, "zeros"), "conv1", "saturate")["logits"])


@pytest.mark.parametrize("C,n", FULL + [(3, 6)])
def test_overflow_on_full_faults_on_one_frame_only(C, n):
    """healthy on the 16 ragged frames (conv1 channel 7 stays far below 65504), all NaN without an action on the all-255 frame"""
    w = E.make("overflow_on_full", C, n)
    got = E.checker_many([(w, f) for f in E.ragged_frames(C)] + [(w, E.frame(C, "full"))], C, n)
    assert all(s["status"] == 0 and np.isfinite(s["logits"]).all() and np.isfinite(s["act"]).all() for s in got[:16])
    assert got[16]["status"] == E.NO_ACTION and np.isnan(got[16]["logits"]).all() and np.isnan(got[16]["hid"]).all()
    s1 = ck.stages(w, C, n, E.ragged_frames(C)[7])["s1"][E.FULL_CHANNEL]
    assert 20000 < s1.min() and s1.max() < 60000
    assert np.isposinf(ck.stages(w, C, n, E.frame(C, "full"))["s1"][E.FULL_CHANNEL]).all()
    assert len({u32(s["logits"]).tobytes() for s in got}) == 17


@pytest.mark.parametrize("C,n", FULL)
def test_subnormal_classes_differ_from_their_flushed_twins(C, n):
    """each sub_* net against the same net with the subnormal tensor set to zero - what a unit that flushes subnormal operands
    would compute: other GPU-visible words on the random frame.  The conv classes also hold subnormal RESULTS"""
    f = E.frame(C, "random")
    for name, tensor in E.SUBNORMAL.items():
        w, wf = E.make(name, C, n), E.flushed(name, C, n)
        t = E.view(w, C, n, tensor)
        assert (np.abs(t) < E.MIN_NORMAL16).all() and np.count_nonzero(t) > 0.5 * t.size and not E.view(wf, C, n, tensor).any()
        a, b = E.checker_many([(w, f), (wf, f)], C, n)
        assert a["status"] == b["status"] == 0 and np.isfinite(a["logits"]).all() and a["logits"].any()
        assert differ(a["logits"], b["logits"]) and (name == "sub_out" or differ(a["hid"], b["hid"])), name
        if name in E.SUB_SCALE:
            s = ck.stages(w, C, n, f)["s" + name[-1]]
            assert ((s != 0) & (np.abs(s) < E.MIN_NORMAL16)).mean() > 0.1, name


@pytest.mark.parametrize("C,n", FULL)
def test_dead_and_switched_off_channels(C, n):
    """dead_conv<k>: the channel's conv sums are the bias everywhere and its BatchNorm output is EXACTLY relu(beta) - with the bias
    0.013 as with bias 0: in this format a constant channel cannot show the summation order (up to 400 copies of one fp16 value
    add up exactly in fp32 in any order, so the mean is the value and d = 0; the fp32 catalogue's dead channels do show it).  The
    order itself is pinned by every random row, whose sums are inexact.  gamma0_*: the frame cannot show; beta_off_conv3: a3 = 0"""
    f = E.frame(C, "random")
    plain = E.checker(E.make("plain", C, n), f, C, n)
    for k in (1, 2, 3):
        w = E.make(f"dead_conv{k}", C, n)
        ch = E.dead_channel(E.make("plain", C, n), C, n, k)
        beta = E.view(w, C, n, f"vbn{k}.bias")[ch]
        assert not E.view(w, C, n, f"conv{k}.weight")[ch].any() and E.view(w, C, n, f"conv{k}.bias")[ch] == E.DEAD_BIAS and beta > 0
        s, z = ck.stages(w, C, n, f), ck.stages(E.dead_with_bias(k, C, n, 0.0), C, n, f)
        assert (s[f"s{k}"][ch] == E.DEAD_BIAS).all() and (s[f"a{k}"][ch] == beta).all() and (z[f"a{k}"][ch] == beta).all()
        assert not differ(s["logits"], z["logits"]) and differ(s["logits"], plain["logits"])
    for name in ("gamma0_conv1", "gamma0_conv2", "gamma0_conv3", "beta_off_conv3"):
        w = E.make(name, C, n)
        a, b = E.checker_many([(w, f), (w, E.frame(C, "full"))], C, n)
        assert not differ(a["logits"], b["logits"]) and differ(a["logits"], plain["logits"]), name
    assert not E.checker(E.make("beta_off_conv3", C, n), f, C, n)["act"].any()
    for k in (1, 2, 3):
        assert differ(E.checker(E.make(f"gamma_neg_conv{k}", C, n), f, C, n)["logits"], plain["logits"])


# ------------------------------------------------------------------------------------------- teeth
@pytest.mark.parametrize("C,n", E.SHAPES)
def test_every_rounding_pair_has_teeth(C, n):
    """33 pairs = nine sites x four wrong modes less the three vacuous quotient pairs, none skipped: on at least one of the
    pair's rows the checker with that ONE conversion wrong differs from the contract in conv3 activations, hidden row, logits or
    action - the words a launch leaves behind.  A kernel with that conversion wrong cannot pass the GPU file.  The ties_away
    frames of the conv / BatchNorm sites are the recorded first frames of the seeded sequence"""
    rows = E.rounding_rows(C, n)
    assert set(rows) == {(s, m) for s in ck.SITES for m in E.WRONG_MODES} - set(E.VACUOUS) and len(rows) == 33
    for (site, mode), rr in rows.items():
        teeth = []
        for name, fname in rr:
            w, f = E.make(name, C, n), E.frame(C, fname)
            want = ck.stages(w, C, n, f)
            teeth.append(E.shows(want, ck.stages(w, C, n, f, site, mode)))
            assert not differ(want["logits"], E.checker(w, f, C, n)["logits"])
        assert any(teeth), f"({site}, {mode}) at C = {C}, n = {n}: no row of {rr} notices the variant"
        assert all(teeth) or (site, mode) == ("conv1", "flush_results"), (site, mode, rr, teeth)
    assert all(0 <= i < 64 for i in E.TIES_AWAY_FRAME[(C, n)].values())


def test_recorded_tie_frames_are_the_first_of_the_sequence():
    """C = 4, n = 6: the recorded index of each conv / BatchNorm site is what the search over the seeded sequence returns (no
    earlier frame shows); the other shapes' indices are asserted to show by the teeth test"""
    for site, i in E.TIES_AWAY_FRAME[(4, 6)].items():
        assert E.first_tie_frame(4, 6, site, limit=i + 1) == i, site


def test_the_two_wrong_scans_have_teeth_and_the_rows_are_all_listed():
    C, n = 4, 6
    rows = E.class_rows(C, n)
    assert len(rows) == len(set(rows)) and {name for name, _ in rows} == set(E.CLASSES)
    assert all(r in rows for rr in E.rounding_rows(C, n).values() for r in rr)
    f = E.frame(C, "random")
    for scan in ck.ACTION_SCANS[1:]:
        assert any(ck.stages(E.make(name, C, n), C, n, f, scan=scan)["action"] != E.checker(E.make(name, C, n), f, C, n)["action"]
                   for name in E.TIES), scan


@pytest.mark.parametrize("C,n", FULL)
def test_filler_rows_are_pairwise_different(C, n):
    """the 4 healthy nets x 16 random frames of the ragged and filler rows: 64 different logit vectors, none a class row's, so a
    row or task mix-up on the device cannot return a matching vector"""
    got = E.checker_many([(E.healthy(C, n, k), E.ragged_frames(C)[i]) for k in range(4) for i in range(16)], C, n)
    vecs = {u32(s["logits"]).tobytes() for s in got}
    assert len(vecs) == 64 and all(np.isfinite(s["logits"]).all() and s["status"] == 0 for s in got)
    assert u32(E.checker(E.make("plain", C, n), E.frame(C, "random"), C, n)["logits"]).tobytes() not in vecs
    assert len({s["action"] for s in got}) > 1


def test_cache_task_tiling_and_expected_status():
    C, n = 4, 6
    w, f = E.make("plain", C, n), E.frame(C, "zeros")
    E.checker(w, f, C, n)
    before = E.N_CHECKER_CALLS
    again = E.checker_many([(w, f)] * 3 + [(w.copy(), f.copy())], C, n)
    assert E.N_CHECKER_CALLS == before and all(not differ(s["logits"], again[0]["logits"]) for s in again)
    tasks, rows = E.tile_rows([(1, 3), (0, 17), (1, 0), (0, 16)])
    assert tasks == [(1, 0, 3), (0, 3, 17), (1, 20, 0), (0, 21, 16)] and rows == 37
    assert E.served_rows(tasks, rows) == [1] * 3 + [None] * 18 + [0] * 16
    nets = [w, E.make("all_neg_inf", C, n)]
    want, st = E.expected([(0, 0, 1), (1, 1, 1), (0, 2, 0)], nets, np.stack([f, f, f]), C, n)
    assert st == E.NO_ACTION | E.BAD_TASK and want[2] is None and want[1]["status"] == E.NO_ACTION and want[1]["action"] == 0
    assert E.expected([(0, 0, 2)], nets, np.stack([f, f]), C, n)[1] == 0


def test_edge_nets_of_the_older_files_are_unchanged():
    """edge_nets moved here from tests/test_fp16_dqn_gpu.py: the same five nets (their construction draws from fixed seeds)"""
    C, n = 4, 6
    sub, zero, big, tie, over = E.edge_nets(C, n)
    t = E.view(sub, C, n, "fc1.weight")
    assert (np.abs(t) < E.MIN_NORMAL16).all() and t.all() and not E.view(zero, C, n, "fc1.weight").any()
    assert (E.view(big, C, n, "fc1.weight")[0] == 60000.0).all() and np.isfinite(E.view(big, C, n, "fc1.weight")[1:]).all()
    assert E.view(tie, C, n, "output.bias").tolist() == [0.125, 0.25, 0.5, 0.375, 0.5, 0.125] and not E.view(tie, C, n, "output.weight").any()
    assert (E.view(over, C, n, "conv1.weight") == 60000.0).all()
    for a in (zero, big, tie, over):
        assert np.array_equal(u32(E.view(a, C, n, "conv2.weight")), u32(E.view(sub, C, n, "conv2.weight")))
