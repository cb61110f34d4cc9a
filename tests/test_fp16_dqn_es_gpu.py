"""The float16 Co-ES update over DeepQN on the GPU against the CPU restatement tests/dqn_es16_checker.py, equalities only: every
word of the noise-regenerating chunk partials (coevo_dqn_es16_partial), the regenerated noise against the perturb launch's own,
every word of the updated base net (coevo_dqn_es16_apply) and nothing else, the one-step rounding of scale16, the argument
checks, and whole HalfDQNESEngine generations (reward pairs, distances, scores, fit16, every net, evaluation means, run() against
the single steps)."""
import functools

import numpy as np
import pytest
import torch

from coevonet_amd import lib as L
from coevonet_amd.dqn_es_half import HalfDQNESEngine
from coevonet_amd.population import mean_eval
from oracle import ref_port as rp
from tests import dqn_es16_checker as xk
from tests import dqn_ga16_checker as dk
from tests import es16_checker as ek
from tests.test_fp16_dqn_breeding_gpu import (POISON, SEED, SKIP_BN, bits, dev_f32, dev_i32, n_params, pack16, poisoned,
                                              stride16, unpack16, used_words)
from tests.util import sha

pytestmark = pytest.mark.gpu
DEV = "cuda"
ERR_ARG = -1
SHAPES = ((4, 6), (3, 18))   # between them they move every section boundary and the padded last quad
IDS = dict(ids=lambda s: f"C{s[0]}n{s[1]}")
STREAM_HI = 9
SLO_FIRST = 5
FC1_HALVES = 512 * 3136
GUARD = 4   # floats in front of and behind a partial buffer (16 bytes: the buffer stays aligned)


def partial_floats(C, n):
    return int(L.load().coevo_dqn_es16_partial_floats(C, n))


@functools.lru_cache(maxsize=None)
def partial_map(C, n):
    """canonical parameters() index of every float of a chunk partial (-1: a word of the stride's padding), asked of the
    library: two nets whose entries spell their own index (p % 2048, p // 2048: both exact in fp16) are packed, and a partial
    is the slab order with every half of the fc1 block (which starts 2048 C + 70112 words into a net) widened to one float"""
    P = n_params(C, n)
    p = np.arange(P)
    slab = pack16([(p % 2048).astype(np.float32), (p // 2048).astype(np.float32)], C, n).cpu().numpy()
    stride, wf = stride16(C, n), 2048 * C + 70112
    nets = []
    for w in slab.reshape(2, stride):
        head = w[:wf].view(np.float32).astype(np.int64)
        halves = w[wf:wf + FC1_HALVES // 2].view(np.float16).astype(np.int64)
        tail = w[wf + FC1_HALVES // 2:].view(np.float32).astype(np.int64)
        nets.append(np.concatenate([head, halves, tail]))
    canon = nets[0] + 2048 * nets[1]
    canon[used_words(C, n) + FC1_HALVES // 2:] = -1
    assert len(canon) == partial_floats(C, n) and np.array_equal(np.sort(canon[canon >= 0]), p)
    canon.setflags(write=False)
    return canon


def used_floats(C, n):
    """-> mask over a partial's floats: True where an update reads and writes (a parameter that is not BatchNorm affine)"""
    canon = partial_map(C, n)
    return (canon >= 0) & xk.moving_mask(C, n)[np.maximum(canon, 0)]


def to_partial_layout(want_flat, C, n):
    """[chunks][P] canonical values -> the partial words: moving entries at their float, 0 at BatchNorm and padding words"""
    canon, keep = partial_map(C, n), used_floats(C, n)
    out = np.zeros((len(want_flat), len(canon)), dtype=np.float32)
    out[:, keep] = np.asarray(want_flat, dtype=np.float32)[:, canon[keep]]
    return out


def from_partial_layout(words, C, n):
    """partial words [chunks][floats] -> [chunks][P] canonical"""
    canon = partial_map(C, n)
    out = np.zeros((len(words), n_params(C, n)), dtype=np.float32)
    out[:, canon[canon >= 0]] = words[:, canon >= 0]
    return out


def same_words_or_both_nan(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


# ---------------------------------------------------------------------------------------------- coevo_dqn_es16_partial
N_IND = 5
# a zero, a negative, the largest finite half, a word whose products with a noise of 2 or more leave fp32 (2^127 is a power of
# two: every product that stays finite is exact, as the product of two halves is, so fmaf and multiply-then-add agree), and an
# ordinary value behind it
FIT = np.array([0.0, -3.5, 65504.0, 2.0 ** 127, 1.25], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def noises(C, n, sigma):
    """the stored noise of individuals 0 .. N_IND - 1 (streams SLO_FIRST + j), computed once per (shape, sigma)"""
    out = np.stack([xk.noise16(C, n, sigma, SEED, SLO_FIRST + j, STREAM_HI) for j in range(N_IND)])
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("sigma", [1e-6, 0.05, 0.5])
@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_partial_every_word_against_the_checker(shape, sigma):
    C, n = shape
    nz = noises(C, n, sigma)
    m = xk.moving_mask(C, n)
    if sigma == 1e-6:
        assert (nz[:, m] == 0).any() and ((nz[:, m] != 0) & (np.abs(nz[:, m]) < 6.1e-5)).any(), "subnormal and zero noise16"
        assert (np.abs(nz) < 6.1e-5).all()
    fit_dev = torch.from_numpy(FIT).to(DEV)
    sig = dev_f32(sigma)
    F = partial_floats(C, n)
    unused = ~used_floats(C, n)
    for chunks in (3, 8):   # unequal chunks; more chunks than individuals
        buf = torch.full((chunks * F + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
        L.call("coevo_dqn_es16_partial", C, n, L._p(fit_dev), N_IND, chunks, L._p(sig), SEED, SLO_FIRST, STREAM_HI,
               buf.data_ptr() + 4 * GUARD)
        got = buf.cpu().numpy()
        assert np.isnan(got[:GUARD]).all() and np.isnan(got[-GUARD:]).all(), "guard words changed"
        got = got[GUARD:-GUARD].reshape(chunks, F)
        want = to_partial_layout(ek.chunk_partials(nz, FIT, chunks), C, n)
        assert same_words_or_both_nan(got, want), chunks
        assert not got[:, unused].view(np.uint32).any(), "BatchNorm and padding positions read 0"
        empty = [c for c in range(chunks) if c * N_IND // chunks == (c + 1) * N_IND // chunks]
        assert len(empty) == (3 if chunks == 8 else 0)
        for c in empty:
            assert not got[c].view(np.uint32).any(), "a chunk without an individual is a zero partial"
        if sigma == 0.5:   # the chunk of individual 3 holds products past fp32: inf on both sides
            assert np.isinf(got).sum() > 10 and np.array_equal(np.isinf(got), np.isinf(want))
        if sigma != 1e-6:
            assert np.count_nonzero(got) > 1000000


@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_regenerated_noise_is_the_perturb_launchs_noise(shape):
    """a zero parent perturbed with stream j holds noise16[j] in its conv and Linear entries (and nothing in BatchNorm), and the
    partial of one individual with fitness 1.0 on the same stream is the same numbers - at every piece: the conv pieces that
    straddle Philox blocks, the last partial quad, the first and last fc1 piece"""
    C, n = shape
    sigma = 0.3
    P = n_params(C, n)
    m = xk.moving_mask(C, n)
    par = pack16([np.zeros(P, dtype=np.float32)], C, n)
    child = poisoned(4 * stride16(C, n))
    sig = dev_f32(sigma)
    L.call("coevo_dqn16_perturb_dist", L._p(par), L._p(dev_i32([0, 0, 0])), L._p(child), 0, 3, C, n, L._p(sig), SEED,
           SLO_FIRST + 2, STREAM_HI, SKIP_BN, None, 0, None, None)
    kids = unpack16(child, 0, 3, C, n)
    F = partial_floats(C, n)
    one = dev_f32(1.0)
    for c in range(3):
        j = 2 + c
        assert np.array_equal(bits(kids[c]), bits(xk.noise16(C, n, sigma, SEED, SLO_FIRST + j, STREAM_HI)))
        assert not kids[c][~m].any() and np.count_nonzero(kids[c][m]) > 0.99 * m.sum()
        buf = torch.full((F,), float("nan"), dtype=torch.float32, device=DEV)
        L.call("coevo_dqn_es16_partial", C, n, L._p(one), 1, 1, L._p(sig), SEED, SLO_FIRST + j, STREAM_HI, L._p(buf))
        got = from_partial_layout(buf.cpu().numpy()[None], C, n)[0]
        # (fmaf(1, x, +0) turns a -0 into +0: compare values where the noise is a zero)
        assert np.array_equal(got == 0, kids[c] == 0)
        nzero = kids[c] != 0
        assert np.array_equal(bits(got[nzero]), bits(kids[c][nzero]))


# ---------------------------------------------------------------------------------------------- coevo_dqn_es16_apply
def random_theta(rng, C, n):
    """a generic fp16-valued net with a stripe of subnormal entries"""
    theta = dk.to_half(rng.normal(0, 0.1, n_params(C, n)))
    sub = np.arange(0, len(theta), 97)
    theta[sub] = (np.arange(len(sub)) % 1023 + 1).astype(np.uint16).view(np.float16).astype(np.float32)
    return theta


def apply_in_a_poisoned_slab(theta, words, chunks, C, n, n_total, sigma, lr, rng):
    """the base net as net 1 of a three-net slab of random words -> (the updated net, flat; slab words before; after)"""
    stride = stride16(C, n)
    slab = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, size=3 * stride, dtype=np.int64).astype(np.int32)).to(DEV)
    L.call("coevo_dqn16_pack", L._p(torch.from_numpy(theta[None]).to(DEV)), slab.data_ptr() + 4 * stride, 1, C, n)
    torch.cuda.synchronize()
    before = slab.cpu().numpy().copy()
    sig = dev_f32(sigma)
    part = torch.from_numpy(words).to(DEV)
    L.call("coevo_dqn_es16_apply", slab.data_ptr() + 4 * stride, L._p(part), chunks, C, n, n_total, L._p(sig), lr)
    torch.cuda.synchronize()
    assert np.array_equal(bits(part.cpu().numpy()), bits(words)) and float(sig.item()) == np.float32(sigma)
    return unpack16(slab, 1, 1, C, n)[0], before, slab.cpu().numpy()


@pytest.mark.parametrize("chunks", [1, 3, 8])
@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_apply_every_word_and_nothing_else(shape, chunks):
    C, n = shape
    rng = np.random.default_rng(100 * C + n + chunks)
    P, stride = n_params(C, n), stride16(C, n)
    m = xk.moving_mask(C, n)
    theta = random_theta(rng, C, n)
    # chunk sums of every size class: ordinary, enough to carry dot16 past 65504, small enough for a subnormal upd16, zero
    flat = (rng.normal(0, 1, (chunks, P)) * 10.0 ** rng.integers(-7, 3, (chunks, P))).astype(np.float32)
    flat[:, ::11] = rng.normal(0, 40000.0, (chunks, len(range(0, P, 11)))).astype(np.float32)
    flat[:, ::13] = 0
    words = to_partial_layout(flat, C, n)
    words[:, ~used_floats(C, n)] = np.float32("nan")   # BatchNorm and padding floats of a partial are never used
    n_total, sigma, lr = 16, 0.05, 0.1
    got, before, after = apply_in_a_poisoned_slab(theta, words, chunks, C, n, n_total, sigma, lr, rng)
    assert np.array_equal(after[:stride], before[:stride]) and np.array_equal(after[2 * stride:], before[2 * stride:])
    assert np.array_equal(after[stride + used_words(C, n):2 * stride], before[stride + used_words(C, n):2 * stride])
    dot = ek.dot16(np.where(m, flat, np.float32(0)))
    want, upd = xk.apply(theta, C, n, dot, lr, n_total, sigma)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(got[~m]), bits(theta[~m])), "BatchNorm gamma / beta changed"
    # (six of the ten decades of the chunk sums, 1e-3 and up, give an update above half an ulp of a theta near 0.1)
    assert (got[m] != theta[m]).mean() > 0.5
    assert np.isinf(dot[m]).sum() > 100 and np.isinf(got[m]).sum() > 100, "dot16 past 65504 is inf, and so is the entry"
    tiny = (upd[m] != 0) & (np.abs(upd[m]) < 6.1e-5)
    assert tiny.sum() > 100 and (got[m][tiny] != theta[m][tiny]).any(), "subnormal upd16 were flushed"


def test_apply_edges_overflow_to_inf_and_subnormals_are_kept():
    C, n = 3, 18
    rng = np.random.default_rng(5)
    P = n_params(C, n)
    m = xk.moving_mask(C, n)
    n_total, sigma, lr = 16, 0.05, 0.1   # scale16 = 0.125
    # theta at +-65504, a finite update of 500 in its direction: past the last finite half
    big = np.full(P, 65504, dtype=np.float32)
    big[1::2] *= -1
    flat = np.where(big > 0, np.float32(4000.0), np.float32(-4000.0))[None].astype(np.float32)
    got, _, _ = apply_in_a_poisoned_slab(big, to_partial_layout(flat, C, n), 1, C, n, n_total, sigma, lr, rng)
    want, upd = xk.apply(big, C, n, ek.dot16(np.where(m, flat, np.float32(0))), lr, n_total, sigma)
    assert np.array_equal(bits(got), bits(want)) and (np.abs(upd[m]) == 500).all()
    assert np.isposinf(got[m][big[m] > 0]).all() and np.isneginf(got[m][big[m] < 0]).all() and (np.abs(got[~m]) == 65504).all()
    # an all-subnormal theta and a subnormal update (dot16 = f16(4e-6), upd16 = 8 * 2^-24): moved, never flushed
    sub = (np.arange(P) % 1015 + 1).astype(np.uint16).view(np.float16).astype(np.float32)
    sub[1::2] *= -1
    flat = np.full((1, P), 4e-6, dtype=np.float32)
    got, _, _ = apply_in_a_poisoned_slab(sub, to_partial_layout(flat, C, n), 1, C, n, n_total, sigma, lr, rng)
    want, upd = xk.apply(sub, C, n, ek.dot16(np.where(m, flat, np.float32(0))), lr, n_total, sigma)
    assert (upd[m] == np.float32(8 * 2.0 ** -24)).all()
    assert np.array_equal(bits(got), bits(want)) and (got[m] != sub[m]).all() and np.array_equal(bits(got[~m]), bits(sub[~m]))
    assert (np.abs(got) < 6.2e-5).all() and (got[m] != 0).mean() > 0.99
    # chunk sums whose total passes 65504 only together: dot16 is inf, and so is the entry (theta finite)
    theta = random_theta(rng, C, n)
    flat = np.full((3, P), 30000.0, dtype=np.float32)
    flat[:, 1::2] *= -1
    got, _, _ = apply_in_a_poisoned_slab(theta, to_partial_layout(flat, C, n), 3, C, n, n_total, sigma, lr, rng)
    dot = ek.dot16(np.where(m, flat, np.float32(0)))
    want, _ = xk.apply(theta, C, n, dot, lr, n_total, sigma)
    assert np.isinf(dot[m]).all() and np.array_equal(bits(got), bits(want))
    assert np.isposinf(got[m][0::2]).all() and np.isneginf(got[m][1::2]).all() and np.isfinite(got[~m]).all()


# lr / (n sigma) whose fp64 quotient 0.00672340415513262 rounds to another fp16 word when it passes through fp32 first: found by
# a numpy search over lr = k / 1000, n < 600 and sigma = fp32(0.05)
SCALE_TRIPLE = (0.079, 235, 0.05)


def test_apply_scale_is_rounded_once_from_the_fp64_quotient():
    C, n = 4, 6
    lr, n_total, sigma = SCALE_TRIPLE
    q = lr / (n_total * float(np.float32(sigma)))
    once, twice = np.float16(q), np.float16(np.float32(q))
    assert once != twice and ek.scale16(lr, n_total, sigma) == np.float32(once)
    P = n_params(C, n)
    m = xk.moving_mask(C, n)
    slab = pack16([np.zeros(P, dtype=np.float32)], C, n)
    flat = np.where(m, np.float32(1.0), np.float32(0))[None].astype(np.float32)
    part = torch.from_numpy(to_partial_layout(flat, C, n)).to(DEV)
    L.call("coevo_dqn_es16_apply", L._p(slab), L._p(part), 1, C, n, n_total, L._p(dev_f32(sigma)), lr)
    got = unpack16(slab, 0, 1, C, n)[0]
    assert (got[m] == np.float32(once)).all() and not got[~m].any()


def test_bad_arguments_return_err_arg_and_write_nothing():
    C, n = 3, 18
    lib = L.load()
    stride, F = stride16(C, n), partial_floats(C, n)
    theta = poisoned(stride + 4)
    part = torch.full((2 * F + 4,), float("nan"), dtype=torch.float32, device=DEV)
    fit = torch.ones(4, dtype=torch.float32, device=DEV)
    sig = dev_f32(0.1)
    s = L._stream()
    assert lib.coevo_dqn_es16_partial_floats(7, n) == ERR_ARG and lib.coevo_dqn_es16_partial_floats(C, 33) == ERR_ARG
    assert lib.coevo_dqn_es16_partial_floats(C | L.DQN_FC1_TILED, n) == ERR_ARG
    assert F == stride + FC1_HALVES // 2
    good = dict(C=C, n_actions=n, fit=L._p(fit), n=4, chunks=2, sig=L._p(sig), part=L._p(part), theta=L._p(theta))

    def partial(**kw):
        a = dict(good, **kw)
        return lib.coevo_dqn_es16_partial(a["C"], a["n_actions"], a["fit"], a["n"], a["chunks"], a["sig"], SEED, 0, 0, a["part"],
                                          s)

    def apply(**kw):
        a = dict(good, **kw)
        return lib.coevo_dqn_es16_apply(a["theta"], a["part"], a["chunks"], a["C"], a["n_actions"], a["n"], a["sig"], 0.1, s)

    shapes = (dict(C=0), dict(C=7), dict(n_actions=0), dict(n_actions=33), dict(C=C | L.DQN_FC1_TILED), dict(C=C | 0x200))
    for kw in (dict(fit=None), dict(sig=None), dict(part=None), dict(n=0), dict(n=-1), dict(chunks=0), dict(chunks=65),
               dict(chunks=-1), dict(part=L._p(part) + 4), dict(part=L._p(part) + 8)) + shapes:
        assert partial(**kw) == ERR_ARG, kw
    for kw in (dict(theta=None), dict(sig=None), dict(part=None), dict(n=0), dict(n=-1), dict(chunks=0), dict(chunks=65),
               dict(theta=L._p(theta) + 4), dict(theta=L._p(theta) + 8), dict(part=L._p(part) + 4)) + shapes:
        assert apply(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()
    assert (theta.cpu().numpy().view(np.uint32) == POISON).all() and torch.isnan(part).all()
    # ... and the good calls do write
    assert partial() == 0 and apply() == 0
    torch.cuda.synchronize()
    assert not torch.isnan(part[:2 * F]).any() and torch.isnan(part[2 * F:]).all()
    assert (theta.cpu().numpy().view(np.uint32)[stride:] == POISON).all()


# ---------------------------------------------------------------------------------------------- whole generations
# torch_seed / philox_seed: chosen on the CPU so that no forward of the checker's games has two equal largest logits (counted
# in checker_run; fp16 logits do tie - one of twelve candidate seed pairs had a tie - these have none) and every role sees a
# nonzero reward in generation 0 (C4n6: in both generations; C3n18: first_0 in both), so that both base nets move and
# generation 1 starts from moved nets
CONFIGS = {"C4n6_pop3": dict(pop=3, C=4, n=6, torch_seed=42, philox_seed=7),
           "C3n18_pop4": dict(pop=4, C=3, n=18, torch_seed=52, philox_seed=7)}
T_TRAIN = T_EVAL = 3
GENERATIONS = 2
CHUNKS = 8
SIGMAS = (0.05, 0.08)
LR = 0.1
ENV_SEED = 123


def initial_base(cfg):
    """two generic fp16-valued nets: initial nets after one mutation of every parameter (the BatchNorm affine then differs from
    1 / 0)"""
    torch.manual_seed(cfg["torch_seed"])
    return {r: dk.mutate(dk.to_half(rp.dqn_init(cfg["C"], cfg["n"])[0]), cfg["C"], cfg["n"], 0.02, 77, ri, 0)
            for ri, r in enumerate(xk.ROLES)}


@functools.lru_cache(maxsize=None)
def checker_run(name, sharing):
    """the sequential restatement, computed once per configuration -> per generation the record + the sha256 of every net"""
    cfg = CONFIGS[name]
    base = initial_base(cfg)
    forward, ties = dk.ck.forward, []

    def counting_forward(flat, C, n, frame):
        a, logits, st = forward(flat, C, n, frame)
        ties.append(int(np.sum(logits == logits.max()) > 1))
        return a, logits, st
    out = []
    dk.ck.forward = counting_forward
    try:
        for gen in range(GENERATIONS):
            rec = xk.generation(base, gen, SIGMAS, LR, sharing, cfg["pop"], cfg["C"], cfg["n"], T_TRAIN, T_EVAL, ENV_SEED,
                                cfg["philox_seed"], chunks=CHUNKS)
            rec["base_sha"] = {r: sha(base[r]) for r in xk.ROLES}
            rec["pert_sha"] = {r: [sha(w) for w in rec["pert"][r]] for r in xk.ROLES}
            out.append(rec)
    finally:
        dk.ck.forward = forward
    assert len(ties) == GENERATIONS * (2 * cfg["pop"] + xk.N_EVAL) * T_TRAIN and not any(ties), "a logit tie in the checker's games"
    return out


def engine(cfg):
    eng = HalfDQNESEngine(cfg["pop"], cfg["C"], cfg["n"], T_TRAIN, T_EVAL, device=DEV, env_seed=ENV_SEED,
                          philox_seed=cfg["philox_seed"], chunks=CHUNKS)
    base = initial_base(cfg)
    for r in xk.ROLES:
        eng.upload(r, "base", 0, base[r][None])
    return eng


def acc_pairs(ro):
    return ro.acc.cpu().numpy()[:, :2].tolist()


@pytest.mark.parametrize("sharing", [False, True], ids=["plain", "sharing"])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_whole_generations_against_the_checker(name, sharing):
    cfg = CONFIGS[name]
    want = checker_run(name, sharing)
    eng, eng2 = engine(cfg), engine(cfg)
    try:
        evs, divs = [], []
        for gen, rec in enumerate(want):
            # without the fused distances in generation 1: update() computes them; run() below fuses them in both
            eng.perturb(gen, SIGMAS, sharing and gen == 0)
            for r in xk.ROLES:
                assert [sha(w) for w in eng.download(r, "pert", 0, cfg["pop"])] == rec["pert_sha"][r], (gen, r, "perturbed nets")
            eng.rollout(gen)
            torch.cuda.synchronize()
            assert acc_pairs(eng.ro) == rec["games"], (gen, "training reward pairs")
            eng.update(gen, LR, sharing)
            for ri, r in enumerate(xk.ROLES):
                assert np.array_equal(bits(eng.fitness[ri].cpu().numpy()), bits(rec["fit16"][r])), (gen, r, "fit16")
                if sharing:
                    assert np.array_equal(bits(eng.dist[ri].cpu().numpy()), bits(rec["dist"][r])), (gen, r, "distances")
                    assert bits(eng.diversity()[ri]) == bits(rec["score"][r]), (gen, r, "sharing score")
                assert sha(eng.download(r, "base", 0, 1)[0]) == rec["base_sha"][r], (gen, r, "base net after the update")
            eng.evaluate(gen)
            torch.cuda.synchronize()
            ev = mean_eval(eng.eval_ro.acc.cpu().numpy(), 2)
            assert acc_pairs(eng.eval_ro) == rec["eval_games"] and ev == rec["eval_rewards"], (gen, "evaluation")
            assert int(eng.ro.status.item()) == 0 and int(eng.eval_ro.status.item()) == 0
            evs.append(ev)
            divs.append(eng.diversity() if sharing else None)
        first = initial_base(cfg)
        for r in xk.ROLES:   # (three agent-steps a game: hits are rare, and without a reward the update is zero)
            assert np.any(want[0]["fit16"][r] != 0), (r, "no reward in generation 0: the update would not move the net")
            assert sha(first[r]) != want[0]["base_sha"][r], "the update must move the base nets"
        # a second engine with the same seeds, driven by run(): the same arrays
        res = eng2.run(GENERATIONS, SIGMAS, LR, sharing)
        assert res["eval_rewards"] == evs
        if sharing:
            assert [[int(bits(x)[0]) for x in d] for d in res["diversity"]] == [[int(bits(x)[0]) for x in d] for d in divs]
        else:
            assert res["diversity"] == [None] * GENERATIONS
        torch.cuda.synchronize()
        assert np.array_equal(eng2.slab.cpu().numpy(), eng.slab.cpu().numpy())
        for ri in range(2):
            assert np.array_equal(bits(eng2.fitness[ri].cpu().numpy()), bits(eng.fitness[ri].cpu().numpy()))
    finally:
        eng.close()
        eng2.close()


def test_an_upload_invalidates_the_fused_distances():
    """perturb() with fitness sharing leaves the distances of its generation behind; an upload into the slab makes them stale, and
    the next update() computes them again from the nets that are there"""
    cfg = CONFIGS["C4n6_pop3"]
    eng = engine(cfg)
    try:
        base = initial_base(cfg)
        eng.perturb(0, SIGMAS, True)
        assert eng._dist_gen == 0
        torch.cuda.synchronize()
        fused = [eng.dist[ri].cpu().numpy().copy() for ri in range(2)]
        assert all((d > 0).all() for d in fused)
        eng.upload("second_0", "pert", 1, base["second_0"][None])   # perturbed net 1 of second_0 := its base net
        assert eng._dist_gen is None
        eng.update(0, LR, True)
        torch.cuda.synchronize()
        again = [eng.dist[ri].cpu().numpy() for ri in range(2)]
        assert np.array_equal(bits(again[0]), bits(fused[0]))
        assert again[1][1] == 0 and np.array_equal(bits(again[1][[0, 2]]), bits(fused[1][[0, 2]]))
        assert eng._dist_gen is None   # the base nets moved
    finally:
        eng.close()
