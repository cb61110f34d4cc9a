"""Float16 Co-ES without a GPU: the CPU restatement (tests/es16_checker.py) against numpy's own half arithmetic for what the
reference executes - np.dot(noises16.T, fit16), scale * dot, base16 += upd -, the one-step fitness rounding, the new kernels
and partial sizes in the library, and HalfESEngine's export and refusals.  (The new C-ABI symbols in the library, the header
and the binding: tests/test_abi.py.)"""
import ctypes

import numpy as np
import pytest

from coevonet_amd import lib as L
from oracle import ref_port as rp
from tests import es16_checker as ek
from tests import ga16_checker as gk

NEW_KERNELS = ("fc16_es_partial_kernel", "fc16_es_apply_kernel", "es16_fitness_kernel")
# largest gap, in fp16 ulps of numpy's value, between dot16 with the canonical ES_CHUNKS = 8 chunk sums and numpy's sequential
# half np.dot over the inputs of half_inputs() (D = 8 and 10, n = 16, sigma 0.05): measured with numpy 2.x on x86-64
MEASURED_MAX_ULPS_CHUNKS8 = 4.0
N, SIGMA, LR, SEED = 16, 0.05, 0.1, 77


def bits16(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16).view(np.uint16)


def half_inputs(D):
    """-> (base16 [P_linear], noises16 [n][P_linear], fit16 [n]) as numpy float16 arrays, over the Linear entries"""
    m = gk.linear_mask(D)
    rng = np.random.default_rng(D)
    base = (rng.uniform(-0.3, 0.3, int(m.sum()))).astype(np.float16)
    noises = np.stack([ek.noise16(D, SIGMA, SEED, 3 + j, 6)[m] for j in range(N)]).astype(np.float16)
    fit = rng.normal(-20.0, 15.0, N).astype(np.float16)
    return base, noises, fit


@pytest.mark.parametrize("D", [8, 10])
def test_chunks_1_is_numpys_half_arithmetic_bit_for_bit(D):
    base, noises, fit = half_inputs(D)
    m = gk.linear_mask(D)
    P = rp.param_count(D)
    full = np.zeros((N, P), dtype=np.float32)
    full[:, m] = noises.astype(np.float32)
    theta = np.ones(P, dtype=np.float32)
    theta[m] = base.astype(np.float32)
    dot = ek.dot16(ek.chunk_partials(full, fit.astype(np.float32), 1))
    new, upd = ek.apply(theta, D, dot, LR, N, SIGMA)
    # what the reference executes on half arrays (evolutionary_strategy.py:137-148, 259-265)
    ref_dot = np.dot(noises.T, fit)
    scale = LR / (N * float(np.float32(SIGMA)))
    ref_upd = scale * ref_dot
    ref_base = base.copy()
    ref_base += ref_upd
    assert ref_dot.dtype == np.float16 and ref_upd.dtype == np.float16 and ref_base.dtype == np.float16
    assert np.array_equal(bits16(dot[m]), ref_dot.view(np.uint16))
    assert np.array_equal(bits16(upd[m]), ref_upd.view(np.uint16))
    assert np.array_equal(bits16(new[m]), ref_base.view(np.uint16))
    assert np.array_equal(new[~m], theta[~m]) and not dot[~m].any()
    assert np.count_nonzero(ref_base != base) > 1000, "the update must move the net for the comparison to mean anything"


def test_chunks_8_stays_within_the_measured_gap_to_numpy():
    """The canonical summation (ES_CHUNKS = 8 chunk sums added left to right) against numpy's sequential half dot on the same
    inputs.  Measured: D = 8: 31 of 137 221 entries differ, the largest difference 4.0 fp16 ulps of numpy's value; D = 10: 23
    of 138 245, at most 2.0 ulps.  The gaps above one ulp sit at entries whose terms (|fit16 * noise16| up to 2.5) cancel to a
    sum near 6e-5, where an fp16 ulp is 6e-8 - the size of ONE fp32 rounding of a running sum -, so the order of the fp32
    additions shows; no entry above 1e-3 in magnitude differs by more than one ulp.  The bound is the measured maximum plus
    one ulp."""
    worst = 0.0
    for D in (8, 10):
        base, noises, fit = half_inputs(D)
        m = gk.linear_mask(D)
        full = np.zeros((N, rp.param_count(D)), dtype=np.float32)
        full[:, m] = noises.astype(np.float32)
        dot = ek.dot16(ek.chunk_partials(full, fit.astype(np.float32), ek.ES_CHUNKS))[m]
        ref = np.dot(noises.T, fit)
        gap = np.abs(dot.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)
        print(f"D = {D}: {np.count_nonzero(gap)} of {gap.size} entries differ, largest gap {gap.max()} fp16 ulps")
        worst = max(worst, float(gap.max()))
        assert gap[np.abs(ref.astype(np.float64)) > 1e-3].max() <= 1.0
    assert worst <= MEASURED_MAX_ULPS_CHUNKS8 + 1.0


def test_fitness_is_rounded_from_fp64_in_one_step():
    x = 1.0 + 2.0 ** -11 + 2.0 ** -30
    assert float(np.float32(x)) == 1.0 + 2.0 ** -11 and np.float16(np.float32(x)) == np.float16(1.0)   # two steps: the tie
    fit = ek.fitness16([x, -x, 70000.0, 65519.9, 1e-9, -3.0])
    assert fit.dtype == np.float32
    assert fit[0] == np.float32(1.0 + 2.0 ** -10) and fit[1] == -fit[0]
    assert np.isposinf(fit[2]) and fit[3] == np.float32(65504.0) and fit[4] == 0 and fit[5] == -3.0
    shared = ek.fitness16([x, 10.0], np.float32(0.7))
    assert shared[0] == np.float32(np.float16(np.float32(1.0 + 2.0 ** -10) / np.float32(1.7)))
    assert shared[1] == np.float32(np.float16(np.float32(10.0) / np.float32(1.7)))


def test_noise_is_the_rounded_fp32_noise_of_the_perturbed_net():
    """a zero parent perturbed with stream j has the stored noise in its Linear entries; LayerNorm entries have none"""
    for D in (8, 10):
        zero = np.zeros(rp.param_count(D), dtype=np.float32)
        n = ek.noise16(D, 0.5, SEED, 4, 9)
        assert np.array_equal(n.view(np.uint32), gk.mutate(zero, D, 0.5, SEED, 4, 9, skip_layernorm=True).view(np.uint32))
        tiny = ek.noise16(D, 1e-6, SEED, 4, 9)[gk.linear_mask(D)]
        assert (tiny == 0).any() and (tiny != 0).any() and (np.abs(tiny) < 6.1e-5).all(), "subnormal and zero noise16"


def test_library_has_the_es16_kernels_and_partial_sizes():
    """(the entry points in the header, the library and the binding: tests/test_abi.py)"""
    from coevonet_amd.build import build
    build()
    dll = ctypes.CDLL(L.LIB_PATH)
    blob = open(L.LIB_PATH, "rb").read()
    for kernel in NEW_KERNELS:
        assert kernel.encode() in blob, f"{kernel} is not in libcoevo.so"
    dll.coevo_es16_partial_floats.restype = ctypes.c_int64
    assert dll.coevo_es16_partial_floats(9) == -1
    for D in (8, 10):   # one float per Linear weight, then one per word of the fp32 tail up to the stride
        weights = D * 512 + 512 * 256 + 5 * 256
        dll.coevo_fc16_slab_stride.restype = ctypes.c_int64
        assert dll.coevo_es16_partial_floats(D) == weights + dll.coevo_fc16_slab_stride(D) - weights // 2


def test_half_es_engine_is_exported_and_refuses_before_the_library_is_loaded(monkeypatch):
    import coevonet_amd
    from coevonet_amd.es_half import HalfESEngine

    assert coevonet_amd.HalfESEngine is HalfESEngine and "HalfESEngine" in coevonet_amd.__all__

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(L, "load", no_load)
    for kw, msg in ((dict(rng="host_reference"), "device_philox"), (dict(env="host"), "device env"),
                    (dict(shard=(1, 2)), "one rank"), (dict(shard=(0, 2)), "one rank"), (dict(antithetic=True), "antithetic"),
                    (dict(centered_rank=True), "centered-rank")):
        with pytest.raises(ValueError, match=msg):
            HalfESEngine(6, **kw)
    for kw in (dict(pop=0), dict(pop=6, chunks=0), dict(pop=6, chunks=65)):
        with pytest.raises(ValueError, match="out of range"):
            HalfESEngine(**kw)


def test_the_trainers_still_refuse_float16():
    from tests.test_fp16_cpu import test_out_of_scope_float16_combinations_raise
    test_out_of_scope_float16_combinations_raise()
