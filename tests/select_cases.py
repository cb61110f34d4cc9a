"""Named inputs and plain references for the selection kernels (csrc/select.hip) at their edges: NaN, zero spread, ties and
the 256-wide ranking slices.

The references are numpy / math.fsum restatements of the reference project's expressions (diversity_penalty,
utils/game_logic_functions.py:12-37; the GA fitness, genetic_algorithm.py:140-146; np.argsort(fitness)[::-1], :223-225).
They never go through oracle_diversity, tests/ga16_checker or libcoevo: tests/test_select_edges_cpu.py holds the checkers to
them, tests/test_select_edges_gpu.py the kernels.  No GPU and no libcoevo needed here.

The device comparisons are equalities although the kernels add their fp64 terms in an order of their own (lane-strided, then
a shuffle tree).  So every finite case is *order-proof*: the fp64 sum taken forwards, backwards and by fsum rounds to the
same fp32 word, and - stronger, and what makes an equality legitimate for ANY order - the whole interval fsum +- n * 2^-53 *
sum|x| (the worst error of n fp64 additions in any order) rounds to that word.  A draw that is not order-proof is redrawn
with the next seed, MAX_REDRAWS times at the most."""
import functools
import math

import numpy as np
import torch

from oracle import ref_port as rp

F32 = np.float32
MAX_REDRAWS = 3
RANDOM_N = (2, 23, 255, 256, 257, 511, 513, 4096)
SUBNORMAL = F32(1e-40)
_quiet = dict(over="ignore", invalid="ignore", divide="ignore", under="ignore")


# ------------------------------------------------------------------------------------------- comparing
def same_f32(a, b):
    """finite and infinite values as bits, NaN by NaN-ness (a NaN's payload is nobody's contract)"""
    a = np.atleast_1d(np.asarray(a, dtype=np.float32)).ravel()
    b = np.atleast_1d(np.asarray(b, dtype=np.float32)).ravel()
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))


# ------------------------------------------------------------------------------------------- order-proof sums
def _orders(x):
    x = np.asarray(x, dtype=np.float64)
    if len(x) == 0:
        return 0.0, 0.0, 0.0
    return float(np.cumsum(x)[-1]), float(np.cumsum(x[::-1])[-1]), math.fsum(x.tolist())


def order_proof(x, post, rel_slack=0.0):
    """post: fp64 sum -> fp32 word.  True when forwards, backwards, fsum and both ends of the any-order error interval
    (widened by rel_slack, for a step of `post` that may be a few fp64 ulps off, such as a device sqrt) give one word"""
    x = np.asarray(x, dtype=np.float64)
    if not np.isfinite(x).all():
        return True   # an inf or NaN term gives inf or NaN in every order (these inputs hold no inf of the other sign)
    fwd, bwd, exact = _orders(x)
    err = len(x) * 2.0 ** -53 * math.fsum(np.abs(x).tolist())
    lo, hi = (exact - err) * (1 - rel_slack), (exact + err) * (1 + rel_slack)
    with np.errstate(**_quiet):
        words = {np.float32(post(v)).view(np.uint32).item() for v in (fwd, bwd, exact, lo, hi)}
    return len(words) == 1


def _sqrt32(s):
    return F32(math.sqrt(max(s, 0.0)))


# ------------------------------------------------------------------------------------------- the sharing score
def np_score(d):
    """numpy's expression on an fp32 array, as the reference (and game_logic.diversity_penalty) writes it"""
    d = np.asarray(d, dtype=np.float32)
    with np.errstate(**_quiet):
        return np.sum(np.maximum(0, 1 - d / np.mean(d)))


def contract_sigma(d):
    return F32(math.fsum(float(x) for x in d) / len(d))


def contract_shares(d):
    d = np.asarray(d, dtype=np.float32)
    with np.errstate(**_quiet):
        return (F32(1) - d / contract_sigma(d)).astype(np.float32)


def contract_score(d):
    """sigma = f32(fsum(d) / n); sh_i = f32(1) - d_i / sigma in float32; f32(fsum(sh_i > 0)); NaN if any sh_i is NaN"""
    sh = contract_shares(d)
    if np.isnan(sh).any():
        return F32(np.nan)
    return F32(math.fsum(float(s) for s in sh if s > 0))


def score_order_proof(d):
    """sigma and the score of `d` do not depend on the order of their fp64 sums (NaN scores: nothing to round)"""
    d = np.asarray(d, dtype=np.float32)
    n = len(d)
    # (a / n in fp64 is one more correctly rounded, monotonic step: it maps the interval's ends to the ends)
    if not order_proof(d.astype(np.float64), lambda s: F32(s / n)):
        return False
    sh = contract_shares(d)
    if np.isnan(sh).any():
        return True
    return order_proof(sh[sh > 0].astype(np.float64), F32)


def _redraw(make, ok, seed):
    for k in range(MAX_REDRAWS + 1):
        x = make(seed + 1000 * k)
        if ok(x):
            return x, k
    raise AssertionError(f"no order-proof draw within {MAX_REDRAWS} redraws (seed {seed})")


def random_dist(n, seed):
    """uniform [0, 3) distances, order-proof -> (fp32 array, redraws used)"""
    def make(s):
        return (np.random.Generator(np.random.PCG64(s)).random(n) * 3).astype(np.float32)
    return _redraw(make, score_order_proof, seed)


def dist_kind(kind, n, seed=0):
    """the score cases as shapes that exist at any n (the fused kernel needs them at pop = 1 ... 4096); positions are spread
    so that at n > 256 the special entries sit in different 256-strides of the kernels' loops"""
    base, _ = random_dist(n, 7000 + 13 * n + seed)
    d = base.copy()
    last, mid = n - 1, n // 2
    if kind == "random":
        pass
    elif kind == "zeros":
        d[:] = 0
    elif kind == "one_zero":
        d[mid] = 0
    elif kind == "one_inf":
        d[mid] = np.inf
    elif kind == "one_nan":
        d[last] = np.nan
    elif kind == "two_inf":
        d[0] = d[last] = np.inf
    elif kind == "all_equal":
        d[:] = F32(1.37)
    elif kind == "subnormal":
        d[mid] = SUBNORMAL
    elif kind == "overflow":
        d[:] = F32(1)
        d[0] = d[mid] = F32(3e38)   # n >= 3: the fp32 sum overflows, the fp64 sum does not
    else:
        raise KeyError(kind)
    if not score_order_proof(d):   # the injected entry moved sigma: take the next base
        assert seed < MAX_REDRAWS, (kind, n)
        return dist_kind(kind, n, seed + 1)
    return d


@functools.lru_cache(maxsize=None)
def score_cases():
    """name -> (fp32 distances, redraws).  The rows of the issue's list, in its order."""
    a = lambda *v: np.array(v, dtype=np.float32)
    cases = {
        "zeros_9": a(*[0] * 9),
        "one_zero_4": a(0, 1.5, 0.25, 2.0),
        "one_inf_4": a(1, 2, np.inf, 3),
        "one_nan_4": a(1, 2, np.nan, 3),
        "two_inf_5": a(1, np.inf, 2, np.inf, 3),
        "single_1": a(0.7),
        "all_equal_7": a(*[1.37] * 7),
        "equals_sigma_4": a(1, 2, 3, 2),          # sigma = 2 exactly: sh = 0 for the two 2s, which must not count
        "subnormal_4": a(1e-40, 1.25, 2.0, 0.75),   # (1, 2, 0.5 beside it: the score 1 + f32(3/7) is an exact tie)
        "overflow_3": a(3e38, 3e38, 1),
    }
    out = {k: (v, 0) for k, v in cases.items()}
    for n in RANDOM_N:
        out[f"random_{n}"] = random_dist(n, 100 + n)
    return out


# the fixed rows whose score is NaN (NaN propagates as in numpy), and the ones whose value can be said without arithmetic
NAN_SCORE = ("zeros_9", "one_inf_4", "one_nan_4", "two_inf_5")
PINNED_SCORE = {"single_1": 0.0, "all_equal_7": 0.0, "equals_sigma_4": 0.5, "subnormal_4": 1.25,
                "overflow_3": 1.0}   # overflow_3: numpy's fp32 mean overflows and gives 3.0; the fp64 mean stays (deviation)


# ------------------------------------------------------------------------------------------- distances
def _dist_terms(ref, net, D):
    with np.errstate(**_quiet):
        diff = np.concatenate([np.asarray(net, dtype=np.float32)[o:o + n] - np.asarray(ref, dtype=np.float32)[o:o + n]
                               for o, n in rp.linear_segments(D)]).astype(np.float32)
        return diff.astype(np.float64) ** 2   # exact: 48 significant bits at the most


def contract_dist(ref, net, D):
    """f32(sqrt(fsum(f32(a - b)^2))) over the Linear entries of flat parameter vectors; inf stays inf, NaN stays NaN"""
    t = _dist_terms(ref, net, D)
    return _sqrt32(math.fsum(t.tolist())) if np.isfinite(t).all() else F32(np.sqrt(np.sum(t)))


def dist_order_proof(ref, net, D):
    return order_proof(_dist_terms(ref, net, D), _sqrt32, rel_slack=2.0 ** -50)   # sqrt halves it: 2 ulp of fp64 sqrt slack


@functools.lru_cache(maxsize=None)
def dist_nets(D, n, seed=0):
    """-> (ref [P], nets [n][P], redraws): FCNetwork initialisations, the nets mutated by sigma 0.05, every distance
    order-proof, and their sharing score too"""
    def make(s):
        torch.manual_seed(s)
        ref = rp.init_net(D)
        return ref, np.stack([rp.mutate_torch(rp.init_net(D), D, 0.05) for _ in range(n)])

    def ok(x):   # ... and so is the sharing score of these distances (coevo_fc_diversity)
        return all(dist_order_proof(x[0], w, D) for w in x[1]) and \
            score_order_proof(np.array([contract_dist(x[0], w, D) for w in x[1]], dtype=np.float32))
    (ref, nets), k = _redraw(make, ok, 500 + 31 * D + n + seed)
    return ref, nets, k


def subnormal_nets(D, n):
    """nets whose Linear entries differ from the reference's by subnormal amounts only (both operands subnormal, so the fp32
    difference is exact): a kernel that flushes subnormals sees distance 0"""
    P = rp.param_count(D)
    g = np.random.Generator(np.random.PCG64(77 + D))
    ref = (g.integers(0, 1 << 20, size=P).astype(np.uint32)).view(np.float32).copy()          # < 2^-129
    nets = np.stack([(g.integers(0, 1 << 22, size=P).astype(np.uint32)).view(np.float32) for _ in range(n)])
    return ref, nets


# ------------------------------------------------------------------------------------------- partial sums (finalize)
@functools.lru_cache(maxsize=None)
def partial_case(n, n_blocks, seed=0):
    """[n][n_blocks] fp64 partial sums of squares, each row order-proof under f32(sqrt(.)); rows rotate through plain, with
    zeros, with an inf and with a NaN among the partials when there is room"""
    def make(s):
        p = np.random.Generator(np.random.PCG64(s)).random((n, n_blocks)) * 4
        for c in range(n):
            k = (c * 7 + 3) % n_blocks
            if c % 4 == 1:
                p[c, k] = 0.0
            elif c % 4 == 2:
                p[c, k] = np.inf
            elif c % 4 == 3:
                p[c, k] = np.nan
        return p

    def ok(p):
        return all(order_proof(row, _sqrt32, rel_slack=2.0 ** -50) for row in p)
    return _redraw(make, ok, 900 + 17 * n + n_blocks + seed)


def contract_finalize(partial):
    """f32(sqrt(fsum(row))) per row; inf stays inf, NaN stays NaN"""
    with np.errstate(**_quiet):
        return np.array([_sqrt32(math.fsum(row.tolist())) if np.isfinite(row).all() else F32(np.sqrt(np.sum(row)))
                         for row in partial], dtype=np.float32)


# ------------------------------------------------------------------------------------------- fitness and ranking
def np_fitness(rewards, game_first, pop, gpi, hof, slot, div):
    """genetic_algorithm.py:140-146 as numpy >= 2 evaluates it (quirk Q2: only the individual's LAST game counts, divided by
    hof all the same): the expression of tests/test_kernels_gpu.py test_diversity_fitness_rank"""
    div = np.float32(div)
    with np.errstate(**_quiet):
        return np.array([np.float32(rewards[game_first + i * gpi + gpi - 1, slot] / hof) / (1 + div) for i in range(pop)],
                        dtype=np.float32)


def np_order(f):
    return np.argsort(np.asarray(f, dtype=np.float32), kind="stable")[::-1]


RANK_N = (1, 2, 256, 257, 4096)
CENTERED_N = (1, 2, 7, 257, 5000)


@functools.lru_cache(maxsize=None)
def rank_vectors(n):
    """name -> fp32 fitness vector of length n: the ranking edges that exist at this n over distinct normals"""
    g = np.random.Generator(np.random.PCG64(4000 + n))
    base = g.permutation(n).astype(np.float32) / F32(8) - F32(n / 16)   # distinct, exact in fp32, both signs
    out = {"distinct": base}

    def put(name, need, fn):
        if n >= need:
            f = base.copy()
            fn(f)
            out[name] = f
    put("nan_first", 1, lambda f: f.__setitem__(0, np.nan))
    put("nan_middle", 3, lambda f: f.__setitem__(n // 2, np.nan))
    put("nan_last", 2, lambda f: f.__setitem__(n - 1, np.nan))
    put("nan_three", 3, lambda f: f.__setitem__([0, n // 2, n - 1], np.nan))
    put("nan_straddles_slice", 257, lambda f: f.__setitem__([255, 256], np.nan))
    put("all_nan", 1, lambda f: f.__setitem__(slice(None), np.nan))
    put("pos_neg_inf", 2, lambda f: (f.__setitem__(0, -np.inf), f.__setitem__(n - 1, np.inf)))
    put("inf_tie", 4, lambda f: (f.__setitem__([1, n - 2], np.inf), f.__setitem__([0, n // 2], -np.inf)))
    # -0 and +0 are one value: the index decides, whichever sign comes first
    put("signed_zeros", 2, lambda f: (f.__setitem__(0, -0.0), f.__setitem__(n - 1, 0.0)))
    put("signed_zeros_rev", 7, lambda f: (f.__setitem__([1, 5], 0.0), f.__setitem__([3, 6], -0.0)))
    put("tie5", 7, lambda f: f.__setitem__([0, 2, 3, n // 2, n - 1], F32(0.0625)))
    put("tie_255_256", 257, lambda f: f.__setitem__([255, 256], F32(0.0625)))
    put("tie_511_512", 513, lambda f: f.__setitem__([511, 512], F32(0.0625)))
    put("tie_0_last", 2, lambda f: f.__setitem__([0, n - 1], F32(0.0625)))
    put("all_equal", 1, lambda f: f.__setitem__(slice(None), F32(-2.5)))
    put("subnormals", 4, lambda f: f.__setitem__([0, 1, 2, 3], [1e-45, -1e-45, 0.0, 1e-45]))
    return out
