"""Float16 Co-ES over DeepQN without a GPU: the CPU restatement (tests/dqn_es16_checker.py) against numpy's own half arithmetic
for what the reference executes - np.dot(noises16.T, fit16), scale * dot, base16 += upd -, which entries move, the stored noise
against the perturbed net of an all-zero parent, the new kernels and partial sizes in the library, and HalfDQNESEngine's export
and refusals.  (The new C-ABI symbols in the library, the header and the binding: tests/test_abi.py.)"""
import ctypes
import functools
import os

import numpy as np
import pytest

from coevonet_amd import lib as L
from oracle import ref_port as rp
from tests import dqn_es16_checker as xk
from tests import dqn_ga16_checker as dk
from tests import es16_checker as ek

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_KERNELS = ("dqn16_es_partial_kernel", "dqn16_es_apply_kernel")
# largest gap, in fp16 ulps of numpy's value, between dot16 with the canonical ES_CHUNKS = 8 chunk sums and numpy's sequential
# half np.dot over the inputs of half_inputs() ((C, n) = (3, 6), 8 and 16 individuals, sigma 0.05): measured with numpy 2.x on
# x86-64 (8 individuals: 0.0, one individual per chunk; 16 individuals: 8.0)
MEASURED_MAX_ULPS_CHUNKS8 = 8.0
C_, N_ACT = 3, 6
N, SIGMA, LR, SEED = 8, 0.05, 0.1, 77


def bits16(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16).view(np.uint16)


@functools.lru_cache(maxsize=None)
def half_inputs(n_ind=N):
    """-> (base16 [P_moving], noises16 [n_ind][P_moving], fit16 [n_ind]) as numpy float16 arrays, over the entries an update
    moves"""
    m = xk.moving_mask(C_, N_ACT)
    rng = np.random.default_rng(C_ + N_ACT + n_ind)
    base = (rng.uniform(-0.3, 0.3, int(m.sum()))).astype(np.float16)
    noises = np.stack([xk.noise16(C_, N_ACT, SIGMA, SEED, 3 + j, 6)[m] for j in range(n_ind)]).astype(np.float16)
    fit = rng.normal(-20.0, 15.0, n_ind).astype(np.float16)
    for a in (base, noises, fit):
        a.setflags(write=False)
    return base, noises, fit


@functools.lru_cache(maxsize=None)
def numpy_half_update(n_ind=N):
    """what the reference executes on half arrays (evolutionary_strategy.py:137-148, 259-265) -> (dot, upd, base) float16"""
    base, noises, fit = half_inputs(n_ind)
    ref_dot = np.dot(noises.T, fit)
    scale = LR / (n_ind * float(np.float32(SIGMA)))
    ref_upd = scale * ref_dot
    ref_base = base.copy()
    ref_base += ref_upd
    assert ref_dot.dtype == np.float16 and ref_upd.dtype == np.float16 and ref_base.dtype == np.float16
    return ref_dot, ref_upd, ref_base


def checker_update(chunks, n_ind=N):
    base, noises, fit = half_inputs(n_ind)
    m = xk.moving_mask(C_, N_ACT)
    P = xk.n_params(C_, N_ACT)
    full = np.zeros((n_ind, P), dtype=np.float32)
    full[:, m] = noises.astype(np.float32)
    theta = np.full(P, 0.75, dtype=np.float32)   # (the BatchNorm entries: any value, they must come back as they are)
    theta[m] = base.astype(np.float32)
    dot = ek.dot16(ek.chunk_partials(full, fit.astype(np.float32), chunks))
    new, upd = xk.apply(theta, C_, N_ACT, dot, LR, n_ind, SIGMA)
    return theta, dot, upd, new


def test_chunks_1_is_numpys_half_arithmetic_bit_for_bit():
    base, _, _ = half_inputs()
    m = xk.moving_mask(C_, N_ACT)
    ref_dot, ref_upd, ref_base = numpy_half_update()
    theta, dot, upd, new = checker_update(1)
    assert np.array_equal(bits16(dot[m]), ref_dot.view(np.uint16))
    assert np.array_equal(bits16(upd[m]), ref_upd.view(np.uint16))
    assert np.array_equal(bits16(new[m]), ref_base.view(np.uint16))
    assert np.count_nonzero(ref_base != base) > 1000000, "the update must move the net for the comparison to mean anything"


def test_chunks_8_stays_within_the_measured_gap_to_numpy():
    """The canonical summation (ES_CHUNKS = 8 chunk sums added left to right) against numpy's sequential half dot on the same
    inputs.  With 8 individuals every chunk holds ONE individual, so a chunk sum is fmaf(fit, noise, 0) - the exact product - and
    the left-to-right addition of the chunk sums is the sequential fp32 sum over j itself; 16 individuals (two to a chunk) are
    measured beside them so that the order of the fp32 additions does differ.  Measured: 8 individuals: 0 of 1 685 158 entries
    differ, 0.0 ulps; 16 individuals: 287 of 1 685 158 differ, the largest difference 8.0 fp16 ulps of numpy's value, and no
    entry above 1e-3 in magnitude differs by more than 1.0 ulp - as for the FC nets (tests/test_fp16_es_cpu.py), the gaps above
    one ulp sit at entries whose terms cancel to a sum near the fp16 subnormal range, where an fp16 ulp is the size of one fp32
    rounding of a running sum.  The bound is the measured maximum plus one ulp."""
    m = xk.moving_mask(C_, N_ACT)
    worst = 0.0
    for n_ind in (N, 16):
        ref = numpy_half_update(n_ind)[0]
        dot = checker_update(ek.ES_CHUNKS, n_ind)[1][m]
        gap = np.abs(dot.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)
        print(f"(C, n) = ({C_}, {N_ACT}), {n_ind} individuals: {np.count_nonzero(gap)} of {gap.size} entries differ, largest gap "
              f"{gap.max()} fp16 ulps; above 1e-3 in magnitude {gap[np.abs(ref.astype(np.float64)) > 1e-3].max()}")
        worst = max(worst, float(gap.max()))
    assert worst <= MEASURED_MAX_ULPS_CHUNKS8 + 1.0


def test_the_batchnorm_affine_and_nothing_else_stays_untouched():
    m = xk.moving_mask(C_, N_ACT)
    P = xk.n_params(C_, N_ACT)
    assert int((~m).sum()) == 320 and not m[P - 320:].any() and m[:P - 320].all()   # vbn1 .. vbn3 gamma / beta come last
    theta, dot, upd, new = checker_update(ek.ES_CHUNKS)
    assert np.array_equal(new[~m].view(np.uint32), theta[~m].view(np.uint32)) and not dot[~m].any()
    off = 0
    for shape in rp.dqn_init(C_, N_ACT)[1][:10]:   # conv1 .. conv3, fc1, output: weight and bias each
        n = int(np.prod(shape))
        assert (new[off:off + n] != theta[off:off + n]).mean() > 0.9, shape
        off += n
    assert off == P - 320


def test_noise_is_the_rounded_fp32_noise_of_the_perturbed_net():
    """a zero parent perturbed with stream j has the stored noise in its conv and Linear entries; BatchNorm entries have none"""
    for C, n in ((3, 6), (4, 18)):
        zero = np.zeros(xk.n_params(C, n), dtype=np.float32)
        m = xk.moving_mask(C, n)
        got = xk.noise16(C, n, 0.5, SEED, 4, 9)
        assert np.array_equal(got.view(np.uint32), dk.mutate(zero, C, n, 0.5, SEED, 4, 9, skip_bn=True).view(np.uint32))
        assert np.count_nonzero(got[m]) > 0.99 * m.sum() and not got[~m].any()
        tiny = xk.noise16(C, n, 1e-6, SEED, 4, 9)[m]
        assert (tiny == 0).any() and (tiny != 0).any() and (np.abs(tiny) < 6.1e-5).all(), "subnormal and zero noise16"


def test_library_has_the_dqn_es16_kernels_and_partial_sizes():
    """(the entry points in the header, the library and the binding: tests/test_abi.py)"""
    from coevonet_amd.build import SOURCES, build
    assert "dqn16_es.hip" in SOURCES
    build()
    dll = ctypes.CDLL(L.LIB_PATH)
    text = open(os.path.join(REPO, "include", "coevo.h")).read()
    assert "evolutionary_strategy.py:120-148" in text and "Atari/deepqn.py:158-172" in text
    blob = open(L.LIB_PATH, "rb").read()
    for kernel in NEW_KERNELS:
        assert kernel.encode() in blob, f"{kernel} is not in libcoevo.so"
    dll.coevo_dqn_es16_partial_floats.restype = ctypes.c_int64
    dll.coevo_dqn16_slab_stride.restype = ctypes.c_int64
    for C, n in ((0, 6), (7, 6), (4, 0), (4, 33), (4 | L.DQN_FC1_TILED, 6), (4 | 0x1000, 6)):
        assert dll.coevo_dqn_es16_partial_floats(C, n) == -1
    for C, n in ((4, 6), (3, 18), (1, 1), (6, 32)):   # one float per half of fc1, one per word everywhere else
        assert dll.coevo_dqn_es16_partial_floats(C, n) == dll.coevo_dqn16_slab_stride(C, n) + 512 * 3136 // 2


def _args(**kw):
    """well-formed argument lists over made-up 16-byte aligned addresses: a refusal reads none of them"""
    a = dict(C=4, n_actions=6, fit=0x10000, n=4, chunks=2, sig=0x20000, part=0x30000, theta=0x40000)
    a.update(kw)
    return a


BAD_PARTIAL = [dict(fit=None), dict(sig=None), dict(part=None), dict(C=0), dict(C=7), dict(n_actions=0), dict(n_actions=33),
               dict(C=4 | L.DQN_FC1_TILED), dict(C=4 | 0x200), dict(n=0), dict(n=-1), dict(chunks=0), dict(chunks=65),
               dict(chunks=-1), dict(part=0x30004), dict(part=0x30008)]
BAD_APPLY = [dict(theta=None), dict(sig=None), dict(part=None), dict(C=0), dict(C=7), dict(n_actions=0), dict(n_actions=33),
             dict(C=4 | L.DQN_FC1_TILED), dict(C=4 | 0x200), dict(n=0), dict(n=-1), dict(chunks=0), dict(chunks=65),
             dict(theta=0x40004), dict(theta=0x40008), dict(part=0x30004)]


def test_the_entry_points_refuse_bad_arguments():
    lib = L.load()
    for bad in BAD_PARTIAL:
        a = _args(**bad)
        assert lib.coevo_dqn_es16_partial(a["C"], a["n_actions"], a["fit"], a["n"], a["chunks"], a["sig"], SEED, 0, 0, a["part"],
                                          None) == -1, bad
    for bad in BAD_APPLY:
        a = _args(**bad)
        assert lib.coevo_dqn_es16_apply(a["theta"], a["part"], a["chunks"], a["C"], a["n_actions"], a["n"], a["sig"], 0.1,
                                        None) == -1, bad


def test_half_dqn_es_engine_is_exported_and_refuses_before_the_library_is_loaded(monkeypatch):
    import coevonet_amd
    from coevonet_amd.dqn_es_half import HalfDQNESEngine

    assert coevonet_amd.HalfDQNESEngine is HalfDQNESEngine and "HalfDQNESEngine" in coevonet_amd.__all__

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(L, "load", no_load)
    for kw, msg in ((dict(shard=(1, 2)), "one rank"), (dict(shard=(0, 2)), "one rank"), (dict(gather=lambda *a: None), "gather"),
                    (dict(frames="host"), "on the device only"), (dict(antithetic=True), "antithetic"),
                    (dict(centered_rank=True), "centered-rank")):
        with pytest.raises(ValueError, match=msg):
            HalfDQNESEngine(6, 4, 6, 3, 3, **kw)
    for kw in (dict(pop=0), dict(pop=65536), dict(pop=6, chunks=0), dict(pop=6, chunks=65)):
        with pytest.raises(ValueError, match="out of range"):
            HalfDQNESEngine(C=4, n_actions=6, T_train=3, T_eval=3, **kw)
