"""Float16 DeepQN breeding without a GPU: the refusals of the entry points and of HalfDQNGAEngine, the CPU restatement
(tests/dqn_ga16_checker.py) against torch's half update and against numpy's float16 evaluation of the reference's distance
formula, and the one named deviation from it.  (The new C-ABI symbols in the header and the binding: tests/test_abi.py.)"""
import numpy as np
import pytest
import torch

from coevonet_amd import lib as L
from oracle import ref_port as rp
from tests import dqn_ga16_checker as dk

SHAPES = ((4, 6), (3, 18), (6, 6))
# largest gap, in fp16 ulps of the reference's value, between the contract's distance (fp64 sum of the squared fp16 differences,
# one rounding of the square root) and numpy's float16 np.linalg.norm over the 15 pairs of distance_pairs(): measured with
# numpy 2.x on x86-64
MEASURED_MAX_ULPS = 1.0
ERR_ARG = L.K["COEVO_ERR_ARG"]
SKIP_BN, ANTITHETIC, FROM_ORDER, COPY = (L.K["COEVO_DQP_" + n] for n in ("SKIP_BN", "ANTITHETIC", "FROM_ORDER", "COPY"))


def test_perturb_blocks_is_one_block_per_256_pieces():
    lib = L.load()
    for C, n in SHAPES + ((1, 1), (6, 32)):
        stride = int(lib.coevo_dqn16_slab_stride(C, n))
        assert stride % 64 == 0
        assert lib.coevo_dqn16_perturb_blocks(C, n) == -(-(stride // 4) // 256)
    for C, n in ((0, 6), (7, 6), (4, 0), (4, 33), (4 | L.DQN_FC1_TILED, 6), (4 | 0x1000, 6)):
        assert lib.coevo_dqn16_perturb_blocks(C, n) == ERR_ARG


def _perturb_args(**kw):
    """a well-formed argument list over made-up 16-byte aligned addresses: a refusal reads none of them"""
    a = dict(parent=0x10000, idx=0x20000, child=0x30000, first=0, n=1, C=4, n_actions=6, sigma=0x40000, seed=1, slo=0, shi=0,
             flags=0, gen=None, bias=0, ref=0x50000, partial=0x60000)
    a.update(kw)
    return [a[k] for k in ("parent", "idx", "child", "first", "n", "C", "n_actions", "sigma", "seed", "slo", "shi", "flags",
                           "gen", "bias", "ref", "partial")] + [None]


BAD_PERTURB = [dict(parent=None), dict(idx=None), dict(child=None), dict(sigma=None), dict(child=None, flags=COPY, ref=None,
                                                                                           partial=None),
               dict(C=0), dict(C=7), dict(n_actions=0), dict(n_actions=33), dict(C=4 | L.DQN_FC1_TILED), dict(C=4 | 0x200),
               dict(parent=0x10004), dict(child=0x30008), dict(ref=0x50002), dict(n=-1), dict(first=-1), dict(ref=None),
               dict(partial=None), dict(flags=ANTITHETIC), dict(flags=FROM_ORDER), dict(flags=16), dict(flags=SKIP_BN | 32),
               dict(flags=-1)]


@pytest.mark.parametrize("bad", BAD_PERTURB, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD_PERTURB])
def test_perturb_dist_refuses(bad):
    assert L.load().coevo_dqn16_perturb_dist(*_perturb_args(**bad)) == ERR_ARG


def test_distance_refuses_and_empty_calls_are_ok():
    lib = L.load()
    good = dict(ref=0x10000, pop=0x20000, n=1, C=4, n_actions=6, partial=0x30000)
    for bad in (dict(ref=None), dict(pop=None), dict(partial=None), dict(C=0), dict(C=7), dict(C=4 | L.DQN_FC1_TILED),
                dict(n_actions=0), dict(n_actions=33), dict(ref=0x10008), dict(pop=0x20004), dict(n=-1)):
        a = dict(good, **bad)
        assert lib.coevo_dqn16_distance(a["ref"], a["pop"], a["n"], a["C"], a["n_actions"], a["partial"], None) == ERR_ARG, bad
    assert lib.coevo_dqn16_distance(0x10000, 0x20000, 0, 4, 6, 0x30000, None) == 0
    assert lib.coevo_dqn16_perturb_dist(*_perturb_args(n=0)) == 0
    assert lib.coevo_dqn16_perturb_dist(*_perturb_args(n=0, flags=SKIP_BN, ref=None, partial=None)) == 0


def test_half_dqn_engine_refuses_out_of_scope_arguments_before_the_library_is_loaded(monkeypatch):
    import coevonet_amd
    from coevonet_amd.build import SOURCES
    from coevonet_amd.dqn_ga_half import HalfDQNGAEngine, HalfSynthRollout

    assert coevonet_amd.HalfDQNGAEngine is HalfDQNGAEngine and coevonet_amd.HalfSynthRollout is HalfSynthRollout
    assert {"HalfDQNGAEngine", "HalfSynthRollout"} <= set(coevonet_amd.__all__)
    assert "dqn16_offspring.hip" in SOURCES

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(L, "load", no_load)
    for kw, msg in ((dict(shard=(1, 2)), "one rank"), (dict(shard=(0, 2)), "one rank"), (dict(frames="host"), "on the device"),
                    (dict(gather=lambda eng: None), "gather")):
        with pytest.raises(ValueError, match=msg):
            HalfDQNGAEngine(3, 2, 2, 4, 6, 4, 3, **kw)
    for bad in ((3, 2, 4), (3, 0, 1), (3, 2, 0)):
        with pytest.raises(ValueError, match="out of range"):
            HalfDQNGAEngine(*bad, 4, 6, 4, 3)


def test_the_trainers_still_refuse_float16():
    from tests.test_fp16_cpu import test_out_of_scope_float16_combinations_raise
    test_out_of_scope_float16_combinations_raise()


def test_checker_mutation_is_torchs_half_update():
    """dqn_ga16_checker.add_noise == half_param.data += noise on a half tensor with the same noise array: every parameter,
    BatchNorm affine included"""
    torch.manual_seed(5)
    flat, shapes = rp.dqn_init(3, 6)
    parent = dk.to_half(flat)
    rng = np.random.default_rng(5)
    # ordinary noise, plus values that land exactly between two halves and beyond the half range
    noise = (rng.normal(0, 0.3, len(parent)) * 10.0 ** rng.integers(-6, 6, len(parent))).astype(np.float32)
    want, off = np.zeros(len(parent), dtype=np.float16), 0
    for shp in shapes:
        n = int(np.prod(shp))
        p = torch.from_numpy(parent[off:off + n].astype(np.float16).reshape(shp))
        assert p.dtype == torch.float16
        p += torch.from_numpy(noise[off:off + n].reshape(shp))   # torch.normal(0, sigma, size) is a float32 tensor
        want[off:off + n] = p.numpy().ravel()
        off += n
    assert off == len(parent)
    got = dk.add_noise(parent, noise)
    assert np.isinf(got).any() and np.array_equal(got.astype(np.float16).view(np.uint16), want.view(np.uint16))
    assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32))


def test_rounding_edges_overflow_and_subnormals():
    P = rp.lib().oracle_dqn_param_count(3, 6)
    big = np.full(P, 65504, dtype=np.float32)
    assert np.isposinf(dk.add_noise(big, np.full(P, 40.0, dtype=np.float32))).all()
    assert np.isneginf(dk.add_noise(-big, np.full(P, -40.0, dtype=np.float32))).all()
    # 65504 + 15.99 still rounds back to 65504 (the tie to 65536 = inf starts at 65520)
    assert (dk.add_noise(big, np.full(P, 15.99, dtype=np.float32)) == np.float32(65504)).all()
    # subnormal parents keep their bits under sigma = 0, through the philox route as well
    sub = (np.arange(P) % 1023 + 1).astype(np.uint16).view(np.float16).astype(np.float32)
    assert (np.abs(sub) < 6.2e-5).all() and (sub != 0).all()
    assert np.array_equal(dk.add_noise(sub, np.zeros(P, dtype=np.float32)).view(np.uint32), sub.view(np.uint32))
    assert np.array_equal(dk.mutate(sub, 3, 6, 0.0, 1, 2, 3).view(np.uint32), sub.view(np.uint32))
    # COEVO_DQP_SKIP_BN: the 320 BatchNorm entries come last and stay
    kid = dk.mutate(sub, 3, 6, 0.05, 1, 2, 3, skip_bn=True)
    assert np.array_equal(kid[P - 320:].view(np.uint32), sub[P - 320:].view(np.uint32)) and (kid[:P - 320] != sub[:P - 320]).mean() > 0.99


def distance_pairs():
    """15 (net, other) pairs: per shape the two initial nets, and Philox children of one of them at sigma 0.005 and 0.05 against
    the other (a stale net) and against their parent"""
    out = []
    for C, n in SHAPES:
        torch.manual_seed(100 + C + n)
        a, b = dk.to_half(rp.dqn_init(C, n)[0]), dk.to_half(rp.dqn_init(C, n)[0])
        out.append((a, b))
        for s_i, sigma in enumerate((0.005, 0.05)):
            c = dk.mutate(a, C, n, sigma, 3, 7, s_i)
            out += [(c, b), (c, a)]
    return out


def test_distance_against_the_reference_formula_in_numpy_float16():
    """The contract's distance against what the reference executes, np.linalg.norm(a16 - b16) on float16 get_weights_ES() vectors
    (all parameters).  Measured on the 15 pairs: the largest difference is 1.0 fp16 ulp of the reference's value.  The bound is
    that measured maximum plus one ulp, for numpy builds that order the half dot differently."""
    worst = 0.0
    for a, b in distance_pairs():
        ref = np.linalg.norm(a.astype(np.float16) - b.astype(np.float16))
        assert ref.dtype == np.float16 and np.isfinite(ref) and ref > 0
        got = np.float16(dk.distance(a, b))
        gap = abs(float(got) - float(ref)) / float(np.spacing(np.abs(ref)))
        print(f"contract {float(got)!r} numpy {float(ref)!r} gap {gap} fp16 ulps")
        worst = max(worst, gap)
    print(f"largest difference to numpy's float16 norm: {worst} fp16 ulps")
    assert worst <= MEASURED_MAX_ULPS + 1.0
    a = distance_pairs()[0][0]
    assert dk.distance(a, a) == 0 and np.linalg.norm(a.astype(np.float16) - a.astype(np.float16)) == 0


def test_named_deviation_numpy_half_norm_overflows_at_max_mutation_power():
    """At sigma = 0.2 (max_mutation_power) the sum of the squared differences of a child to its parent passes 65504; numpy
    rounds that sum to half BEFORE the square root, so the reference's distance is inf.  The contract sums in fp64 and rounds
    the square root once: a finite 260 .. 261 (six channels, six actions: 0.2 * sqrt(1 691 622 parameters) = 260.1, and the
    spread of a chi distribution with that many degrees of freedom is 0.2 / sqrt(2) = 0.14).  Both facts are pinned; neither is
    to be "fixed"."""
    torch.manual_seed(104)
    a = dk.to_half(rp.dqn_init(6, 6)[0])
    assert len(a) == 1691622
    c = dk.mutate(a, 6, 6, 0.2, 3, 7, 2)
    assert dk.distance_sum(c, a) > 65504
    ref = np.linalg.norm(c.astype(np.float16) - a.astype(np.float16))
    assert ref.dtype == np.float16 and np.isposinf(ref)
    got = float(dk.distance(c, a))
    assert 260.0 <= got <= 261.0
