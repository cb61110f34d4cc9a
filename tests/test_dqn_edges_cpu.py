"""The adversarial DeepQN net library (tests/dqn_edge_nets.py) against the CPU oracle alone: what oracle_dqn_forward says about
ties, signed zeros, infinities, NaN or overflow in each of the 16 parameter tensors, constant conv channels, a BatchNorm scale
of zero or below, and subnormal weights in every layer.  These are the expected values of tests/test_dqn_forward_edges_gpu.py,
and the conditions on its inputs without which that file could pass vacuously: a subnormal class must differ from its flushed
twin, a dead channel from the summation-order-free variant, the 64 filler rows from each other.  No GPU.

385 distinct oracle forwards per (C, n) - 300 of them the 50 classes on the six named frames - about 4 s each on a handful of
threads (dqn_edge_nets.oracle_many: the C call releases the interpreter lock)."""
import numpy as np
import pytest

from tests import dqn_edge_nets as E

SHAPES = [(4, 6), (6, 18)]


@pytest.fixture(scope="module", autouse=True)
def release_nets():
    yield
    E.release()


def u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def differ(a, b):
    return not np.array_equal(u32(a), u32(b))


@pytest.mark.parametrize("C,n", SHAPES)
def test_offsets_are_the_oracles(C, n):
    """the flat order the library pokes is the one oracle_dqn_forward reads: a NaN written through view() into each tensor
    reaches the logits (the CLASSES test) and the offsets add up to oracle_dqn_param_count (asserted in offsets())"""
    off = E.offsets(C, n)
    assert list(off) == list(E.TENSORS) and off["conv1.weight"][0] == 0
    assert off["vbn1.weight"][0] == off["output.bias"][0] + n and len(E.base_net(C, n, 3)) == off["vbn3.bias"][0] + 64
    w = E.base_net(C, n, 3)
    assert abs(E.view(w, C, n, "vbn2.weight") - 1).max() < 0.2 and abs(E.view(w, C, n, "vbn3.bias")).max() < 0.2   # affine ~ (1, 0)


@pytest.mark.parametrize("C,n", SHAPES)
def test_class_has_its_property(C, n):
    """every class on every named frame: the action where PROPERTY fixes it, the NaN pattern of the logits, and per class
    what makes it an edge (bit-equal top logits, the sign of each zero, -inf everywhere, finite 1e37-sized logits, ...)"""
    F = E.FRAMES(C)
    names = sorted(E.CLASSES)
    got = E.oracle_many([(E.make(name, C, n), f) for name in names for f in F.values()], C, n)
    assert set(E.PROPERTY) == set(names) and len(names) >= 48
    it = iter(got)
    for name in names:
        want_a, want_nan = E.PROPERTY[name]
        for fname in F:
            a, lg = next(it)
            what = (name, C, n, fname, a, lg)
            if want_a is not None:
                assert a == (want_a if want_a >= -1 else n + want_a), what
            else:
                assert -1 <= a < n, what
            nans = int(np.isnan(lg).sum())
            if want_nan is not None:
                assert nans == {"all": n, "one": 1, "none": 0}[want_nan], what
            if want_nan == "all":
                assert a == -1, what
            if want_nan == "one":
                rest = np.where(np.isnan(lg), -np.inf, lg)
                assert a == int(np.argmax(rest)) and 0 <= a and not np.isnan(lg[a]), what
            if name in E.TIES:
                top = u32(lg)[lg == lg.max()]
                assert len(top) == (n if name == "tie_all" else 2) and len(set(top.tolist())) == 1, what
                assert E.last_maximum(lg) != a == int(np.argmax(lg)), what
            if name == "signed_zeros":
                assert np.array_equal(u32(lg), u32(np.where(np.arange(n) % 2 == 0, -0.0, 0.0).astype(np.float32))), what
            if name == "all_neg_inf":
                assert np.all(lg == -np.inf), what
            if name == "one_pos_inf":
                assert lg[2] == np.inf and np.isfinite(np.delete(lg, 2)).all(), what
            if name == "overflow_fc1":
                assert np.isfinite(lg).all() and 1e33 < np.abs(lg).max() < 1e38, what
            if name in ("inf_fc1.weight", "inf_output.weight"):
                assert not np.isfinite(lg).all(), what
            if name == "sub_out":
                assert (np.abs(lg) < E.MIN_NORMAL).all() and (lg != 0).all(), what
    # the faults split as the GPU file's launches assume: NO_FAULT classes never come without an action
    assert all(E.PROPERTY[name][0] != -1 for name in E.NO_FAULT) and len(E.MAY_FAULT) >= 24


@pytest.mark.parametrize("C,n", SHAPES)
def test_beta_off_and_gamma0_cut_the_frame_off(C, n):
    """beta_off_conv3: the logits are those of fc1.bias alone, whatever the frame; gamma0_*: the frame cannot show either,
    but the layers behind still run on relu(beta)"""
    F = E.FRAMES(C)
    for name in ("beta_off_conv3", "gamma0_conv1", "gamma0_conv2", "gamma0_conv3"):
        w = E.make(name, C, n)
        lgs = [lg for _, lg in E.oracle_many([(w, f) for f in F.values()], C, n)]
        assert all(not differ(lg, lgs[0]) for lg in lgs), name
        if name == "beta_off_conv3":
            other = w.copy()   # another conv stack and another fc1 matrix behind the same fc1.bias: the same logits
            for tensor in ("conv1.weight", "conv2.bias", "fc1.weight"):
                E.view(other, C, n, tensor)[:] *= -0.5
            assert not differ(lgs[0], E.oracle(other, F["random"], C, n)[1])
            other = other.copy()   # (the oracle cache froze the first one)
            E.view(other, C, n, "fc1.bias")[:] *= -0.5
            assert differ(lgs[0], E.oracle(other, F["random"], C, n)[1])
    plain = E.oracle(E.make("plain", C, n), F["random"], C, n)[1]
    for name in ("gamma_neg_conv1", "gamma_neg_conv2", "gamma_neg_conv3", "gamma0_conv1", "beta_off_conv3"):
        assert differ(E.oracle(E.make(name, C, n), F["random"], C, n)[1], plain), name


@pytest.mark.parametrize("C,n", SHAPES)
def test_subnormal_classes_are_observable(C, n):
    """each sub_* net against the same net with the scaled tensor set to zero - what a unit that flushes subnormal operands or
    results would compute: other logits on the frames the GPU file shows them (random, and the two hot bytes for the conv
    layers: on a constant frame a conv1 image is constant either way)"""
    F = E.FRAMES(C)
    for name, (tensor, scale) in E.SUB_SCALE.items():
        w, wf = E.make(name, C, n), E.flushed(name, C, n)
        t = E.view(w, C, n, tensor)
        assert (np.abs(t) < E.MIN_NORMAL).all() and np.count_nonzero(t) > 0.99 * t.size and not E.view(wf, C, n, tensor).any()
        for fname in ("random", "hot_first", "hot_last"):
            (a, lg), (af, lf) = E.oracle_many([(w, F[fname]), (wf, F[fname])], C, n)
            assert differ(lg, lf) and np.isfinite(lg).all() and np.isfinite(lf).all() and lg.any(), (name, fname, lg, lf)
            if name == "sub_out":
                assert not lf.any() and af == 0 and (np.abs(lg) < E.MIN_NORMAL).all() and (lg != 0).all()


@pytest.mark.parametrize("C,n", SHAPES)
def test_dead_channels_show_the_summation_order(C, n):
    """a conv channel with all-zero weights is its bias at every position: d = x - S / N is what the canonical strided-sum and
    tree order leave of it, times 1/sqrt(1e-5).  Each dead_conv<k> differs from plain AND from the same net with the channel's
    bias at 0 (d exactly 0: nothing of the order shows) - a kernel that summed in another order would get other logits here.
    0.0125 is the counter-example the constants were picked against: its sums are exact and the class would test nothing"""
    f = E.FRAMES(C)["random"]
    plain = E.oracle(E.make("plain", C, n), f, C, n)[1]
    for k in (1, 2, 3):
        w = E.make(f"dead_conv{k}", C, n)
        ch = E.dead_channel(E.make("plain", C, n), C, n, k)
        assert not E.view(w, C, n, f"conv{k}.weight")[ch].any() and E.view(w, C, n, f"conv{k}.bias")[ch] == E.DEAD_BIAS[k]
        lg = E.oracle(w, f, C, n)[1]
        zero = E.oracle(E.dead_with_bias(k, C, n, 0.0), f, C, n)[1]
        assert differ(lg, plain) and differ(lg, zero), (k, lg, zero)
    exact = E.oracle(E.dead_with_bias(1, C, n, 0.0125), f, C, n)[1]
    assert not differ(exact, E.oracle(E.dead_with_bias(1, C, n, 0.0), f, C, n)[1])


@pytest.mark.parametrize("C,n", SHAPES)
def test_filler_rows_are_pairwise_different(C, n):
    """the 4 healthy nets x 16 random frames of the ragged and filler rows: 64 different logit vectors, none of them a class
    row's, so a row or task mix-up on the device cannot return a matching vector"""
    pairs = [(E.healthy(C, n, k), E.ragged_frames(C)[i]) for k in range(4) for i in range(16)]
    got = E.oracle_many(pairs, C, n)
    vecs = {u32(lg).tobytes() for _, lg in got}
    assert len(vecs) == 64 and all(np.isfinite(lg).all() and 0 <= a < n for a, lg in got)
    assert u32(E.oracle(E.make("plain", C, n), E.FRAMES(C)["random"], C, n)[1]).tobytes() not in vecs
    assert len({a for a, _ in got}) > 1   # the frames steer the action


def test_oracle_cache_counts_distinct_pairs_only():
    C, n = 4, 6
    w, f = E.make("plain", C, n), E.FRAMES(C)["zeros"]
    E.oracle(w, f, C, n)
    before = E.N_ORACLE_CALLS
    again = E.oracle_many([(w, f)] * 5 + [(w.copy(), f.copy())], C, n)      # equal content, other objects
    assert E.N_ORACLE_CALLS == before and all(not differ(lg, again[0][1]) for _, lg in again)
    assert not again[0][1].flags.writeable and not w.flags.writeable


def test_task_table_and_expected_status():
    tasks, net_of_row = E.task_table([(2, 3), (0, 1), (2, 16)], 1000)
    assert net_of_row == [2] * 3 + [0] + [2] * 16
    assert [(int(t["net_off"]), int(t["row_begin"]), int(t["n_rows"])) for t in tasks] == [(2000, 0, 3), (0, 3, 1), (2000, 4, 16)]
    C, n = 4, 6
    nets, f = [E.make("plain", C, n), E.make("all_neg_inf", C, n)], E.FRAMES(C)["zeros"]
    want, st = E.expected([(0, 1), (1, 1)], nets, np.stack([f, f]), C, n)
    assert st == E.NO_ACTION and [a for a, _ in want] == [want[0][0], -1]
    assert E.expected([(0, 2)], nets, np.stack([f, f]), C, n)[1] == 0
