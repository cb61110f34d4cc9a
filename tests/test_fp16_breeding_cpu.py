"""Float16 Co-GA breeding without a GPU: the CPU restatement (tests/ga16_checker.py) against torch's half update and against
numpy's float16 evaluation of the reference's distance formula, the rounding edges and HalfGAEngine's refusals (the new C-ABI
symbols in the header and the binding: tests/test_abi.py)."""
import numpy as np
import pytest
import torch

from coevonet_amd import lib as L
from coevonet_amd.fcnetwork import FCNetworkHalf, LINEAR_KEYS
from oracle import ref_port as rp
from tests import ga16_checker as gk

# largest gap, in fp16 ulps of the reference's value, between the contract's distance (fp64 sum of the squared fp16
# differences, one rounding of the square root) and numpy's float16 np.linalg.norm (sequential fp32 dot rounded to half before
# the square root) over the 272 pairs of distance_pairs(): measured with numpy 2.x on x86-64
MEASURED_MAX_ULPS = 1.0


def test_checker_mutation_is_torchs_half_update():
    """ga16_checker.add_noise == half_param.data += noise (Linear) / fp32 param += noise (LayerNorm) on the same noise"""
    for D, seed in ((10, 5), (8, 6)):
        torch.manual_seed(seed)
        net = FCNetworkHalf(D, 5)
        parent = net.flat()
        rng = np.random.default_rng(seed)
        noise, off = np.zeros(len(parent), dtype=np.float32), 0
        for k, p in net._params.items():
            n = p.numel()
            # ordinary noise, plus values that land exactly between two halves and beyond the half range
            z = (rng.normal(0, 0.3, n) * 10.0 ** rng.integers(-6, 3, n)).astype(np.float32)
            noise[off:off + n] = z
            p.data += torch.from_numpy(z.reshape(tuple(p.shape)))
            off += n
        got = gk.add_noise(parent, D, noise)
        want = net.flat()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        keys = np.array([k in LINEAR_KEYS for k, p in net._params.items() for _ in range(p.numel())])
        assert np.array_equal(keys, gk.linear_mask(D))


def test_rounding_edges_overflow_and_subnormals():
    D = 8
    m = gk.linear_mask(D)
    P = rp.param_count(D)
    big = np.where(m, np.float32(65504), np.float32(1.0)).astype(np.float32)
    up = gk.add_noise(big, D, np.full(P, 40.0, dtype=np.float32))
    assert np.isposinf(up[m]).all() and (up[~m] == np.float32(41.0)).all()
    down = gk.add_noise(-big, D, np.full(P, -40.0, dtype=np.float32))
    assert np.isneginf(down[m]).all()
    # 65504 + 15.99 still rounds back to 65504 (the tie to 65536 = inf starts at 65520)
    assert (gk.add_noise(big, D, np.full(P, 15.99, dtype=np.float32))[m] == np.float32(65504)).all()
    # subnormal parents keep their bits under sigma = 0, through the philox route as well
    sub = (np.arange(P) % 1023 + 1).astype(np.uint16).view(np.float16).astype(np.float32)
    assert (np.abs(sub) < 6.2e-5).all() and (sub != 0).all()
    assert np.array_equal(gk.add_noise(sub, D, np.zeros(P, dtype=np.float32)).view(np.uint32), sub.view(np.uint32))
    assert np.array_equal(gk.mutate(sub, D, 0.0, 1, 2, 3).view(np.uint32), sub.view(np.uint32))


def distance_pairs():
    """272 (D, net, other) pairs of both widths: initial nets, children at sigma 0.005 / 0.05 / 0.5 against their parent and
    against another net, and a net against itself"""
    out = []
    for D in (10, 8):
        torch.manual_seed(100 + D)
        for n in range(17):
            a = gk.round_linear(rp.init_net(D), D)
            b = gk.round_linear(rp.init_net(D), D)
            out.append((D, a, b))
            for s_i, sigma in enumerate((0.005, 0.05, 0.5)):
                c = gk.mutate(a, D, sigma, 3, n, s_i)
                out.append((D, c, a))
                out.append((D, c, b))
            out.append((D, a, a))
    return out


def test_distance_against_the_reference_formula_in_numpy_float16():
    """The contract's distance against what the reference executes, np.linalg.norm(a16 - b16) on float16 get_weights_ES()
    vectors.  Measured on the 272 pairs: the largest difference is 1.0 fp16 ulp of the reference's value (a child at sigma 0.5
    against its parent, width 10: 185.375 against 185.25); a net against itself gives 0 in both.  The bound is that measured
    maximum plus one ulp, for numpy builds that order the half dot differently."""
    pairs = distance_pairs()
    assert len(pairs) >= 200
    worst, zeros = 0.0, 0
    for D, a, b in pairs:
        m = gk.linear_mask(D)
        ref = np.linalg.norm(a[m].astype(np.float16) - b[m].astype(np.float16))
        assert ref.dtype == np.float16
        got = np.float16(gk.distance(a, b, D))
        if a is b:
            assert got == 0 and ref == 0
            zeros += 1
            continue
        worst = max(worst, abs(float(got) - float(ref)) / float(np.spacing(np.abs(ref))))
    print(f"largest difference to numpy's float16 norm: {worst} fp16 ulps over {len(pairs)} pairs")
    assert zeros == 34
    assert worst <= MEASURED_MAX_ULPS + 1.0


def test_sharing_score_route_matches_the_reference_expression():
    """the oracle's sharing arithmetic on handed-over distances (fp16 values) against numpy's own expression"""
    rng = np.random.default_rng(2)
    d = (rng.random(37) * 3).astype(np.float16).astype(np.float32)
    d[5] = 0.0
    got = gk.sharing_score(d)
    want = np.sum(np.maximum(0, 1 - d / np.mean(d)))
    assert got.dtype == np.float32 and abs(float(got) - float(want)) <= 1e-5 * float(want)
    assert gk.rank_desc([1.0, 3.0, 3.0, 2.0]) == [2, 1, 3, 0]


def test_half_engine_refuses_out_of_scope_arguments_before_the_library_is_loaded(monkeypatch):
    import coevonet_amd
    from coevonet_amd.ga_half import HalfGAEngine

    assert coevonet_amd.HalfGAEngine is HalfGAEngine

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(L, "load", no_load)
    for kw, msg in ((dict(adaptive=True), "adaptive"), (dict(shard=(1, 2)), "one rank"), (dict(shard=(0, 2)), "one rank"),
                    (dict(env="host"), "device env"), (dict(rng="host_reference"), "device_philox")):
        with pytest.raises(ValueError, match=msg):
            HalfGAEngine(6, 2, 2, **kw)
    for bad in ((1, 1, 1), (6, 0, 2), (6, 17, 2), (6, 2, 9), (4, 1, 5), (5000, 1, 1)):
        with pytest.raises(ValueError, match="out of range"):
            HalfGAEngine(*bad)


def test_the_trainers_still_refuse_float16():
    from tests.test_fp16_cpu import test_out_of_scope_float16_combinations_raise
    test_out_of_scope_float16_combinations_raise()
