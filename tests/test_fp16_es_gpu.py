"""The float16 Co-ES update on the GPU against the CPU restatement tests/es16_checker.py, equalities only: the fitness rounding
(coevo_es16_fitness), every word of the noise-regenerating chunk partials (coevo_es16_partial), the regenerated noise against
the perturbed nets' own, every word of the updated base net (coevo_es16_apply), the argument checks, and whole HalfESEngine
generations (rewards, fit16, distances and scores, every net, evaluation means, run() against the single steps)."""
import functools

import numpy as np
import pytest
import torch

from coevonet_amd import lib as L
from coevonet_amd.es_half import HalfESEngine
from oracle import ref_port as rp
from tests import es16_checker as ek
from tests import ga16_checker as gk
from tests.test_fp16_breeding_gpu import POISON, SEED, bits, dev_f32, dev_i32, pack16, unpack16, used_words
from tests.test_fp16_gpu import random_flat
from tests.util import sha

pytestmark = pytest.mark.gpu
DEV = "cuda"
STREAM_HI = 9
SLO_FIRST = 5


def eq64(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


@functools.lru_cache(maxsize=None)
def partial_map(D):
    """canonical parameters() index of every float of a chunk partial (-1: a word of the stride's padding), asked of the
    library: two nets whose entries spell their own index (p % 2048, p // 2048: both exact in fp16) are packed, and a partial
    is the slab order with every half entry widened to one float"""
    P = L.fc_param_count(D)
    p = np.arange(P)
    slab = pack16([(p % 2048).astype(np.float32), (p // 2048).astype(np.float32)], D).cpu().numpy()
    stride = L.fc16_slab_stride(D)
    n_half_words = (D * 512 + 512 * 256 + 5 * 256) // 2
    nets = []
    for w in slab.reshape(2, stride):
        halves = w[:n_half_words].view(np.float16).astype(np.int64)
        tail = w[n_half_words:].view(np.float32).astype(np.int64)
        nets.append(np.concatenate([halves, tail]))
    canon = nets[0] + 2048 * nets[1]
    canon[2 * n_half_words + (used_words(D) - n_half_words):] = -1
    assert len(canon) == L.es16_partial_floats(D) and np.array_equal(np.sort(canon[canon >= 0]), p)
    return canon


def to_partial_layout(want_flat, D):
    """[chunks][P] canonical values -> the partial words: Linear entries at their float, 0 at LayerNorm and padding words"""
    canon = partial_map(D)
    m = gk.linear_mask(D)
    keep = (canon >= 0) & m[np.maximum(canon, 0)]
    out = np.zeros((len(want_flat), len(canon)), dtype=np.float32)
    out[:, keep] = np.asarray(want_flat, dtype=np.float32)[:, canon[keep]]
    return out


def from_partial_layout(words, D):
    """partial words [chunks][floats] -> [chunks][P] canonical"""
    canon = partial_map(D)
    out = np.zeros((len(words), L.fc_param_count(D)), dtype=np.float32)
    out[:, canon[canon >= 0]] = words[:, canon >= 0]
    return out


# ---------------------------------------------------------------------------------------------- coevo_es16_fitness
@pytest.mark.parametrize("with_score", [False, True])
def test_fitness_rounds_the_fp64_reward_in_one_step(with_score):
    rng = np.random.default_rng(3)
    G = 40
    table = rng.normal(-30.0, 25.0, (G, 3))
    x = 1.0 + 2.0 ** -11 + 2.0 ** -30   # through an RNE fp32 this is the tie 1 + 2^-11 -> 1.0; in one step 1 + 2^-10
    table[3] = [x, -x, 1.0 + 2.0 ** -11]
    table[7] = [70000.0, -70000.0, 65519.999]
    table[9] = [3e-8, 2.9e-8, -6.2e-5]        # half of the smallest subnormal rounds to 0 / just above it; a subnormal
    idx = rng.permutation(G)[:23].astype(np.int32)
    idx[:3] = [3, 7, 9]
    rew = torch.from_numpy(table).to(DEV)
    score = dev_f32(0.7314) if with_score else None
    for slot in range(3):
        fit = torch.full((len(idx) + 2,), float("nan"), dtype=torch.float32, device=DEV)
        L.call("coevo_es16_fitness", L._p(rew), L._p(dev_i32(idx)), slot, len(idx), L._p(score), fit.data_ptr() + 4)
        got = fit.cpu().numpy()
        assert np.isnan(got[0]) and np.isnan(got[-1])
        want = ek.fitness16(table[idx, slot], np.float32(0.7314) if with_score else None)
        assert np.array_equal(bits(got[1:-1]), bits(want)), slot
        assert np.array_equal(bits(got[1:-1]), bits(got[1:-1].astype(np.float16).astype(np.float32))), "fp16 values"
        if not with_score and slot == 0:
            assert got[1] == np.float32(1.0 + 2.0 ** -10) and np.isposinf(got[2]) and got[3] == np.float32(2.0 ** -24)
        if not with_score and slot == 1:
            assert got[1] == -np.float32(1.0 + 2.0 ** -10) and np.isneginf(got[2]) and got[3] == 0
        if not with_score and slot == 2:
            assert got[1] == np.float32(1.0) and got[2] == np.float32(65504.0)


# ---------------------------------------------------------------------------------------------- coevo_es16_partial
N_MAX = 16


@functools.lru_cache(maxsize=None)
def noises(D, sigma):
    """the stored noise of individuals 0 .. N_MAX - 1 (streams SLO_FIRST + j), computed once per (D, sigma)"""
    out = np.stack([ek.noise16(D, sigma, SEED, SLO_FIRST + j, STREAM_HI) for j in range(N_MAX)])
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("sigma", [1e-6, 0.05, 0.5])
@pytest.mark.parametrize("D", [10, 8])
def test_partial_every_word_against_the_checker(D, sigma):
    rng = np.random.default_rng(int(D + 1000 * sigma))
    nz = noises(D, sigma)
    m = gk.linear_mask(D)
    if sigma == 1e-6:
        lin = nz[:, m]
        assert (lin == 0).any() and ((lin != 0) & (np.abs(lin) < 6.1e-5)).any(), "subnormal and zero noise16"
    fit = ek.f16(rng.normal(-25.0, 20.0, N_MAX))
    fit_dev = torch.from_numpy(fit).to(DEV)
    sig = dev_f32(sigma)
    F = L.es16_partial_floats(D)
    for n in (1, 2, 7, 16):
        for chunks in (1, 2, 8):
            buf = torch.full(((chunks + 1) * F,), float("nan"), dtype=torch.float32, device=DEV)
            L.call("coevo_es16_partial", D, L._p(fit_dev), n, chunks, L._p(sig), SEED, SLO_FIRST, STREAM_HI, L._p(buf))
            got = buf.cpu().numpy().reshape(chunks + 1, F)
            assert np.isnan(got[chunks]).all(), "words past the last chunk changed"
            want = to_partial_layout(ek.chunk_partials(nz[:n], fit[:n], chunks), D)
            assert np.array_equal(got[:chunks].view(np.uint32), want.view(np.uint32)), (n, chunks)
            for c in range(chunks):
                if c * n // chunks == (c + 1) * n // chunks:
                    assert not got[c].view(np.uint32).any(), "a chunk without an individual is a zero partial"
    if sigma != 1e-6:
        assert np.count_nonzero(got[:chunks]) > 100000


@pytest.mark.parametrize("D", [10, 8])
def test_regenerated_noise_is_the_perturbed_nets_noise(D):
    """a zero parent perturbed with stream j holds noise16[j] in its Linear entries (and nothing elsewhere), and the partial
    of n = 1, fitness 1.0 on the same stream is the same numbers"""
    sigma = 0.3
    P = L.fc_param_count(D)
    m = gk.linear_mask(D)
    par = pack16([np.zeros(P, dtype=np.float32)], D)
    stride = L.fc16_slab_stride(D)
    child = torch.full((4 * stride,), POISON, dtype=torch.int32, device=DEV)
    sig = dev_f32(sigma)
    L.call("coevo_fc16_perturb_dist", L._p(par), L._p(dev_i32([0, 0, 0])), L._p(child), 0, 3, D, L._p(sig), SEED, SLO_FIRST + 2,
           STREAM_HI, 1, None, None, None)
    kids = unpack16(child, 0, 3, D)
    F = L.es16_partial_floats(D)
    one = dev_f32(1.0)
    for c in range(3):
        j = 2 + c
        assert np.array_equal(bits(kids[c]), bits(ek.noise16(D, sigma, SEED, SLO_FIRST + j, STREAM_HI)))
        assert not kids[c][~m].any() and np.count_nonzero(kids[c][m]) > 0.99 * m.sum()
        buf = torch.full((F,), float("nan"), dtype=torch.float32, device=DEV)
        L.call("coevo_es16_partial", D, L._p(one), 1, 1, L._p(sig), SEED, SLO_FIRST + j, STREAM_HI, L._p(buf))
        got = from_partial_layout(buf.cpu().numpy()[None], D)[0]
        # (fmaf(1, x, +0) turns a -0 into +0: compare values where the noise is a zero)
        assert np.array_equal(got == 0, kids[c] == 0)
        nzero = kids[c] != 0
        assert np.array_equal(bits(got[nzero]), bits(kids[c][nzero]))


# ---------------------------------------------------------------------------------------------- coevo_es16_apply
@pytest.mark.parametrize("chunks", [1, 3, 8])
@pytest.mark.parametrize("D", [10, 8])
def test_apply_every_word_and_nothing_else(D, chunks):
    rng = np.random.default_rng(10 * D + chunks)
    P = L.fc_param_count(D)
    m = gk.linear_mask(D)
    theta = random_flat(rng, D)
    sub = np.flatnonzero(m)[::97]
    theta[sub] = (np.arange(len(sub)) % 1023 + 1).astype(np.uint16).view(np.float16).astype(np.float32)   # subnormal entries
    stride = L.fc16_slab_stride(D)
    slab = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, size=3 * stride, dtype=np.int64).astype(np.int32)).to(DEV)
    L.call("coevo_fc16_pack", L._p(torch.from_numpy(theta[None]).to(DEV)), slab.data_ptr() + 4 * stride, 1, D)
    before = slab.cpu().numpy().copy()
    # chunk sums of every size class: ordinary, enough to carry dot16 past 65504, small enough for a subnormal upd16, zero
    flat = (rng.normal(0, 1, (chunks, P)) * 10.0 ** rng.integers(-7, 3, (chunks, P))).astype(np.float32)
    flat[:, ::11] = rng.normal(0, 40000.0, (chunks, len(range(0, P, 11)))).astype(np.float32)
    flat[:, ::13] = 0
    words = to_partial_layout(flat, D)
    canon = partial_map(D)
    unused = ~((canon >= 0) & m[np.maximum(canon, 0)])
    words[:, unused] = np.float32("nan")   # LayerNorm and padding floats of a partial are never used
    n, sigma, lr = 16, 0.05, 0.1
    sig = dev_f32(sigma)
    part = torch.from_numpy(words).to(DEV)
    L.call("coevo_es16_apply", slab.data_ptr() + 4 * stride, L._p(part), chunks, D, n, L._p(sig), lr)
    torch.cuda.synchronize()
    after = slab.cpu().numpy()
    assert np.array_equal(after[:stride], before[:stride]) and np.array_equal(after[2 * stride:], before[2 * stride:])
    assert np.array_equal(after[stride + used_words(D):2 * stride], before[stride + used_words(D):2 * stride])
    got = unpack16(slab, 1, 1, D)[0]
    dot = ek.dot16(np.where(m, flat, np.float32(0)))
    want, upd = ek.apply(theta, D, dot, lr, n, sigma)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(got[~m]), bits(theta[~m])), "LayerNorm gamma / beta changed"
    assert np.isinf(dot[m]).sum() > 100 and np.isinf(got[m]).sum() > 100, "dot16 past 65504 is inf, and so is the entry"
    tiny = (upd[m] != 0) & (np.abs(upd[m]) < 6.1e-5)
    assert tiny.sum() > 100 and (got[m][tiny] != theta[m][tiny]).any(), "subnormal upd16 were flushed"
    assert np.array_equal(bits(part.cpu().numpy()), bits(words)) and float(sig.item()) == np.float32(sigma)


def apply_in_a_poisoned_slab(theta, flat, D, n, sigma, lr, rng):
    """coevo_es16_apply on `theta` packed between two nets' worth of random words, from the chunk sums `flat` [chunks][P]
    (canonical order; the LayerNorm and padding floats of the partials are NaN: never used) -> the updated net, unpacked;
    the words around the net and its stride's padding are checked here"""
    m = gk.linear_mask(D)
    stride = L.fc16_slab_stride(D)
    slab = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, size=3 * stride, dtype=np.int64).astype(np.int32)).to(DEV)
    L.call("coevo_fc16_pack", L._p(torch.from_numpy(theta[None].copy()).to(DEV)), slab.data_ptr() + 4 * stride, 1, D)
    before = slab.cpu().numpy().copy()
    words = to_partial_layout(flat, D)
    canon = partial_map(D)
    words[:, ~((canon >= 0) & m[np.maximum(canon, 0)])] = np.float32("nan")
    part = torch.from_numpy(words).to(DEV)
    L.call("coevo_es16_apply", slab.data_ptr() + 4 * stride, L._p(part), len(flat), D, n, L._p(dev_f32(sigma)), lr)
    torch.cuda.synchronize()
    after = slab.cpu().numpy()
    assert np.array_equal(after[:stride], before[:stride]) and np.array_equal(after[2 * stride:], before[2 * stride:])
    assert np.array_equal(after[stride + used_words(D):2 * stride], before[stride + used_words(D):2 * stride])
    return unpack16(slab, 1, 1, D)[0]


@pytest.mark.parametrize("D", [10, 8])
def test_apply_edges_overflow_to_inf_and_subnormals_are_kept(D):
    """the twin of tests/test_fp16_dqn_es_gpu.py's test of the same name for the FC nets: every word against
    tests/es16_checker.py, bit for bit, and the LayerNorm entries untouched"""
    rng = np.random.default_rng(50 + D)
    P = L.fc_param_count(D)
    m = gk.linear_mask(D)
    even = np.arange(P) % 2 == 0
    n, sigma, lr = 16, 0.05, 0.1
    assert ek.scale16(lr, n, sigma) == np.float32(0.125)
    # theta at +-65504, a finite update of 500 in its direction: past the last finite half
    big = np.where(even, np.float32(65504.0), np.float32(-65504.0))
    flat = np.where(even, np.float32(4000.0), np.float32(-4000.0))[None]
    got = apply_in_a_poisoned_slab(big, flat, D, n, sigma, lr, rng)
    want, upd = ek.apply(big, D, ek.dot16(np.where(m, flat, np.float32(0))), lr, n, sigma)
    assert np.array_equal(bits(got), bits(want)) and (np.abs(upd[m]) == 500).all()
    assert np.isposinf(got[m & even]).all() and np.isneginf(got[m & ~even]).all()
    assert np.array_equal(bits(got[~m]), bits(big[~m])), "LayerNorm gamma / beta changed"
    # an all-subnormal theta and a subnormal update (dot16 = f16(4e-6), upd16 = 8 * 2^-24): moved, never flushed
    sub = (np.arange(P) % 1015 + 1).astype(np.uint16).view(np.float16).astype(np.float32)
    sub[~even] *= -1
    flat = np.full((1, P), 4e-6, dtype=np.float32)
    got = apply_in_a_poisoned_slab(sub, flat, D, n, sigma, lr, rng)
    want, upd = ek.apply(sub, D, ek.dot16(np.where(m, flat, np.float32(0))), lr, n, sigma)
    assert (upd[m] == np.float32(8 * 2.0 ** -24)).all()
    assert np.array_equal(bits(got), bits(want)) and (got[m] != sub[m]).all() and np.array_equal(bits(got[~m]), bits(sub[~m]))
    assert (np.abs(got) < 6.2e-5).all() and (got[m] != 0).mean() > 0.99
    # chunk sums whose total passes 65504 only together: dot16 is inf, and so is the entry (theta finite)
    theta = random_flat(rng, D)
    flat = np.where(even, np.float32(30000.0), np.float32(-30000.0))[None].repeat(3, axis=0)
    got = apply_in_a_poisoned_slab(theta, flat, D, n, sigma, lr, rng)
    dot = ek.dot16(np.where(m, flat, np.float32(0)))
    want, _ = ek.apply(theta, D, dot, lr, n, sigma)
    assert np.isfinite(flat[0] + flat[1]).all() and np.abs(flat[0] + flat[1]).max() < 65504 and np.isinf(dot[m]).all()
    assert np.array_equal(bits(got), bits(want))
    assert np.isposinf(got[m & even]).all() and np.isneginf(got[m & ~even]).all()
    assert np.array_equal(bits(got[~m]), bits(theta[~m])), "LayerNorm gamma / beta changed"


def test_apply_scale_is_rounded_once_from_the_fp64_quotient():
    """lr / (n sigma) = 1 + 2^-11 + 2^-30 in fp64 (n = 1, sigma = 1): through an fp32 quotient scale16 would be 1.0"""
    D = 8
    P = L.fc_param_count(D)
    m = gk.linear_mask(D)
    theta = np.zeros(P, dtype=np.float32)
    slab = pack16([theta], D)
    flat = np.where(m, np.float32(1.0), np.float32(0))[None].astype(np.float32)
    part = torch.from_numpy(to_partial_layout(flat, D)).to(DEV)
    lr = 1.0 + 2.0 ** -11 + 2.0 ** -30
    L.call("coevo_es16_apply", L._p(slab), L._p(part), 1, D, 1, L._p(dev_f32(1.0)), lr)
    got = unpack16(slab, 0, 1, D)[0]
    assert ek.scale16(lr, 1, 1.0) == np.float32(1.0 + 2.0 ** -10)
    assert (got[m] == np.float32(1.0 + 2.0 ** -10)).all() and not got[~m].any()


def test_bad_arguments_return_err_arg_and_write_nothing():
    D = 10
    lib = L.load()
    stride = L.fc16_slab_stride(D)
    F = L.es16_partial_floats(D)
    theta = torch.full((stride + 4,), POISON, dtype=torch.int32, device=DEV)
    part = torch.full((2 * F + 4,), float("nan"), dtype=torch.float32, device=DEV)
    fit = torch.full((4,), float("nan"), dtype=torch.float32, device=DEV)
    rew = torch.zeros(4, 3, dtype=torch.float64, device=DEV)
    idx, sig = dev_i32([0, 1, 2, 3]), dev_f32(0.1)
    s = L._stream()
    assert lib.coevo_es16_partial_floats(9) == -1 and lib.coevo_es16_partial_floats(0) == -1
    assert F == stride + (D * 512 + 512 * 256 + 5 * 256) // 2
    good = dict(D=D, fit=L._p(fit), n=4, chunks=2, sig=L._p(sig), part=L._p(part), theta=L._p(theta))

    def partial(**kw):
        a = dict(good, **kw)
        return lib.coevo_es16_partial(a["D"], a["fit"], a["n"], a["chunks"], a["sig"], SEED, 0, 0, a["part"], s)

    def apply(**kw):
        a = dict(good, **kw)
        return lib.coevo_es16_apply(a["theta"], a["part"], a["chunks"], a["D"], a["n"], a["sig"], 0.1, s)

    for kw in (dict(fit=None), dict(sig=None), dict(part=None), dict(D=9), dict(D=0), dict(n=0), dict(n=-1), dict(chunks=0),
               dict(chunks=65), dict(chunks=-1), dict(part=L._p(part) + 4), dict(part=L._p(part) + 8)):
        assert partial(**kw) == -1, kw
    for kw in (dict(theta=None), dict(sig=None), dict(part=None), dict(D=9), dict(D=0), dict(n=0), dict(n=-1), dict(chunks=0),
               dict(chunks=65), dict(theta=L._p(theta) + 4), dict(theta=L._p(theta) + 8), dict(part=L._p(part) + 4)):
        assert apply(**kw) == -1, kw
    def fitness(**kw):
        a = dict(dict(rew=L._p(rew), idx=L._p(idx), slot=0, n=4, score=None, fit=L._p(fit)), **kw)
        return lib.coevo_es16_fitness(a["rew"], a["idx"], a["slot"], a["n"], a["score"], a["fit"], s)

    for kw in (dict(rew=None), dict(idx=None), dict(fit=None), dict(slot=-1), dict(slot=3), dict(n=0), dict(n=-1)):
        assert fitness(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (theta.cpu().numpy().view(np.uint32) == POISON).all() and torch.isnan(part).all() and torch.isnan(fit).all()


# ---------------------------------------------------------------------------------------------- whole generations
SIGMAS = {"agent_0": 0.05, "agent_1": 0.02, "adversary_0": 0.1}
LR = 0.1
CONFIGS = {"pop6": dict(pop=6, limit_train=6, limit_eval=6, max_cycles=25, torch_seed=3, philox_seed=11),
           "pop16": dict(pop=16, limit_train=None, limit_eval=None, max_cycles=3, torch_seed=4, philox_seed=5)}
GENERATIONS = 2


def initial_base(cfg):
    torch.manual_seed(cfg["torch_seed"])
    return {r: gk.round_linear(rp.init_net(gk.ROLE_D[r]), gk.ROLE_D[r]) for r in gk.ROLES}


@functools.lru_cache(maxsize=None)
def checker_run(name, sharing):
    cfg = CONFIGS[name]
    base = initial_base(cfg)
    out = []
    for gen in range(GENERATIONS):
        rec = ek.generation(base, gen, SIGMAS, LR, sharing, cfg["pop"], cfg["limit_train"], cfg["limit_eval"], cfg["max_cycles"],
                            cfg["philox_seed"])
        rec["base_sha"] = {r: sha(base[r]) for r in gk.ROLES}
        rec["pert_sha"] = {r: [sha(w) for w in rec["pert"][r]] for r in gk.ROLES}
        out.append(rec)
    return out


def engine(cfg):
    eng = HalfESEngine(cfg["pop"], cfg["limit_train"], cfg["limit_eval"], cfg["max_cycles"], philox_seed=cfg["philox_seed"])
    base = initial_base(cfg)
    keep = [eng.upload(r, "base", 0, base[r][None]) for r in gk.ROLES]
    torch.cuda.current_stream().synchronize()
    del keep
    return eng


@pytest.mark.parametrize("sharing", [False, True])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_whole_generations_against_the_checker(name, sharing):
    cfg = CONFIGS[name]
    want = checker_run(name, sharing)
    eng = engine(cfg)
    evs, divs = [], []
    for gen, rec in enumerate(want):
        eng.perturb(gen, SIGMAS)   # without the fused distances: update() computes them; run() below fuses them
        for r in gk.ROLES:
            assert [sha(w) for w in eng.download(r, "pert", 0, cfg["pop"])] == rec["pert_sha"][r], (gen, r, "perturbed nets")
        eng.rollout(gen)
        torch.cuda.synchronize()
        assert eq64(eng.rewards_host(), rec["games"]), (gen, "training games")
        eng.update(gen, LR, sharing)
        for r in gk.ROLES:
            assert np.array_equal(bits(eng.fitness[r].cpu().numpy()), bits(rec["fit16"][r])), (gen, r, "fit16")
            if sharing:
                assert np.array_equal(bits(eng.dist[r].cpu().numpy()), bits(rec["dist"][r])), (gen, r, "distances")
                assert bits(eng.diversity()[r]) == bits(rec["score"][r]), (gen, r, "sharing score")
            assert sha(eng.download(r, "base", 0, 1)[0]) == rec["base_sha"][r], (gen, r, "base net after the update")
        ev = eng.evaluate(gen)
        assert eq64(eng.eval_ro.rewards.cpu().numpy(), rec["eval_games"]) and ev == rec["eval_rewards"], (gen, "evaluation")
        evs.append(ev)
        divs.append(eng.diversity() if sharing else None)
    first = initial_base(cfg)
    for r in gk.ROLES:
        assert sha(first[r]) != want[0]["base_sha"][r] != want[1]["base_sha"][r], "the update must move the base nets"
    # a second engine with the same seeds, driven by run(): the same arrays
    eng2 = engine(cfg)
    res = eng2.run(GENERATIONS, SIGMAS, LR, sharing)
    assert res["eval_rewards"] == evs
    if sharing:
        assert [{r: int(bits(d[r])[0]) for r in gk.ROLES} for d in res["diversity"]] == \
            [{r: int(bits(d[r])[0]) for r in gk.ROLES} for d in divs]
    else:
        assert res["diversity"] == [None] * GENERATIONS
    torch.cuda.synchronize()
    assert np.array_equal(eng2.slab.cpu().numpy(), eng.slab.cpu().numpy())
    for r in gk.ROLES:
        assert np.array_equal(bits(eng2.fitness[r].cpu().numpy()), bits(eng.fitness[r].cpu().numpy()))
