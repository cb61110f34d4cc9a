"""Named inputs and plain references for the fp32 breeding, promotion and ES-update kernels (csrc/offspring.hip) at their
edges: segment ends, the one-element last quad, stream and generation wraps, planted non-finite values, the 16-deep ES loop.

The noise VALUES are the oracle's (oracle_philox_normals, the bit-level definition of the noise contract; its transform is
held against a float64 Box-Muller in tests/test_breed_edges_cpu.py).  Everything the kernels DO with the noise is restated
here in plain numpy on canonical flat arrays - agent.py:25-29 and :51-53 (child = parent + noise, noise rounded first),
genetic_algorithm.py:232-275 (elites, Hall of Fame, children), evolutionary_strategy.py:120-148 (the update) - and never goes
through oracle_perturb_philox or oracle_es_update_from_pert: tests/test_breed_edges_cpu.py holds those two to these
restatements, tests/test_breed_edges_gpu.py the kernels.  No GPU and no libcoevo needed here.

Comparisons: finite and infinite results as bits, NaN by position only (x86 and gfx950 give different NaN signs and payloads
for inf * 0 and inf - inf).

The ES accumulation is one fused multiply-add per term in float32.  This interpreter has no math.fma, so a term is emulated
as f32(f64(f) * f64(d) + f64(acc)): the product of two float32 is exact in float64 (48 bits), the sum is rounded to 53 bits
and then to 24.  That double rounding differs from the single rounding of a real fma only when the 53-bit sum is exactly
half way between two float32 AND the float64 addition was inexact; es_accumulate counts such terms (TwoSum error term and
an exact half-way test) and both test files assert the count is zero for every input they use, so no input had to be
restricted to few significant bits."""
import functools
import math

import numpy as np
import torch

from oracle import ref_port as rp

F32 = np.float32
M32 = 0xffffffff
H1, H2 = 512, 256
BLOCK = 1024                      # slab positions per workgroup of the breeding kernels = per distance partial
_quiet = dict(over="ignore", invalid="ignore", divide="ignore", under="ignore")


def bits(u):
    return np.array([u], dtype=np.uint32).view(np.float32)[0]


FLT_MAX, SUB_MIN, SUB_MAX = bits(0x7f7fffff), bits(0x00000001), bits(0x007fffff)
FINITE_PLANTS = [F32(0.0), F32(-0.0), SUB_MIN, SUB_MAX, -SUB_MIN, FLT_MAX, -FLT_MAX]
ALL_PLANTS = FINITE_PLANTS + [F32(np.inf), F32(-np.inf), bits(0x7fc00123), bits(0xffa00001)]   # two NaNs with payloads


# ------------------------------------------------------------------------------------------- comparing
def same_f32(a, b):
    """finite and infinite values as bits, NaN by position"""
    a = np.atleast_1d(np.asarray(a, dtype=np.float32)).ravel()
    b = np.atleast_1d(np.asarray(b, dtype=np.float32)).ravel()
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))


def first_diff(a, b):
    """for assertion messages: the first few positions where same_f32 fails"""
    a, b = np.asarray(a, dtype=np.float32).ravel(), np.asarray(b, dtype=np.float32).ravel()
    bad = np.flatnonzero((np.isnan(a) != np.isnan(b)) | (~np.isnan(a) & ~np.isnan(b) & (a.view(np.uint32) != b.view(np.uint32))))
    return [(int(i), a[i], b[i]) for i in bad[:4]], len(bad)


def same_bits(a, b):
    return bool(np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32),
                               np.ascontiguousarray(b, dtype=np.float32).view(np.uint32)))


# ------------------------------------------------------------------------------------------- layout
def params(D):
    return rp.param_count(D)


def stride(D):
    return (params(D) + 63) // 64 * 64


def n_blocks(D):
    return (stride(D) + BLOCK - 1) // BLOCK


@functools.lru_cache(maxsize=None)
def slab_to_flat(D):
    """int64 [stride]: the canonical flat index held by each slab position, -1 for the padding words.  Only the two weight
    matrices are re-tiled (include/coevo.h): W1t[k][j] = fc1.w[j][k]; W2q[jb][kq][l][c] = fc2.w[64 jb + l][4 kq + c]."""
    P, o_b1 = params(D), D * H1
    o_w2 = o_b1 + 3 * H1
    o_b2 = o_w2 + H1 * H2
    s = np.arange(stride(D), dtype=np.int64)
    out = s.copy()
    w1 = s < o_b1
    out[w1] = (s[w1] % H1) * D + s[w1] // H1
    w2 = (s >= o_w2) & (s < o_b2)
    t = s[w2] - o_w2
    out[w2] = o_w2 + ((t >> 15) * 64 + ((t >> 2) & 63)) * H1 + ((t >> 8) & 127) * 4 + (t & 3)
    out[P:] = -1
    return out


@functools.lru_cache(maxsize=None)
def ln_mask(D):
    m = np.zeros(params(D), dtype=bool)
    for o, n in rp.ln_segments(D):
        m[o:o + n] = True
    return m


def segments(D):
    """(offset, length) of the ten parameter tensors in canonical order"""
    out, off = [], 0
    for _, shp in rp.param_shapes(D):
        n = int(np.prod(shp))
        out.append((off, n))
        off += n
    return out


def to_slab_rows(flat, D, padding):
    """numpy image of a packed net: flat [P] -> [stride] with `padding` in the words past P"""
    m = slab_to_flat(D)
    out = np.full(stride(D), padding, dtype=np.float32)
    out[m >= 0] = np.asarray(flat, dtype=np.float32)[m[m >= 0]]
    return out


# ------------------------------------------------------------------------------------------- noise
@functools.lru_cache(maxsize=64)
def _normals(seed, stream_lo, stream_hi, P):
    z = rp.philox_normals(seed, stream_lo, stream_hi, 0, (P + 3) // 4).reshape(-1)[:P].copy()
    z.setflags(write=False)
    return z


def normals(seed, stream_lo, stream_hi, P):
    """fp32 [P]: entry p = element p % 4 of quad p // 4 of stream (stream_lo, stream_hi)"""
    return _normals(int(seed), int(stream_lo) & M32, int(stream_hi) & M32, int(P))


def stream_of(ind, flags):
    """individual `ind` (mod 2^32) -> (stream_lo, negate): antithetic pairs (flag bit 1) share stream ind >> 1"""
    ind &= M32
    return (ind >> 1, bool(ind & 1)) if flags & 2 else (ind, False)


def noise(sigma, seed, ind, stream_hi, flags, P):
    """f32(sigma * z), negated for the odd partner of an antithetic pair"""
    slo, neg = stream_of(ind, flags)
    with np.errstate(**_quiet):
        nz = (F32(sigma) * normals(seed, slo, stream_hi, P)).astype(np.float32)
    return -nz if neg else nz


def child(parent, D, sigma, seed, ind, stream_hi, flags=0, gen=None):
    """child = parent + f32(sigma * z) in float32; flag bit 0 keeps the LayerNorm entries (the parent's bits); with a
    generation counter the stream is stream_hi + 4 gen (mod 2^32)"""
    parent = np.asarray(parent, dtype=np.float32)
    shi = (stream_hi + (4 * gen if gen is not None else 0)) & M32
    with np.errstate(**_quiet):
        out = (parent + noise(sigma, seed, ind, shi, flags, len(parent))).astype(np.float32)
    if flags & 1:
        out[ln_mask(D)] = parent[ln_mask(D)]
    return out


def rebuilt_elite(old_elites, D, ident, sigma, seed, stream_hi_prev, gen=None):
    """id 0 -> old elite 0 unchanged; id >= 1 -> old elite (id - 1) % E + sigma * noise(stream id - 1); with a generation
    counter g the children were bred with stream_hi_prev + 4 (g - 1)"""
    if ident == 0:
        return np.array(old_elites[0], dtype=np.float32, copy=True)
    c = ident - 1
    shi = (stream_hi_prev + (4 * (gen - 1) if gen is not None else 0)) & M32
    return child(old_elites[c % len(old_elites)], D, sigma, seed, c, shi, 0)


def promote(pop, hof, elite, order, E, from_pop, to_pop0):
    """genetic_algorithm.py:232-275 as list operations on rows (any row type) -> (pop, hof, elite)"""
    pop, hof, elite = list(pop), list(hof), list(elite)
    if from_pop:
        elite = [pop[order[k]] for k in range(E)]
    hof.pop(0)
    hof.append(elite[0])
    if to_pop0:
        pop[0] = elite[0]
    return pop, hof, elite


# ------------------------------------------------------------------------------------------- fused distance
def dist_partials(child_flat, ref_flat, D):
    """fp64 [n_blocks]: per block of 1024 slab positions, fsum of f64(f32(child - ref))^2 over the Linear entries below P;
    a block whose terms are not all finite gets numpy's sum (inf or NaN: compared by class)"""
    m = slab_to_flat(D)
    lin = (m >= 0) & ~ln_mask(D)[np.maximum(m, 0)]
    with np.errstate(**_quiet):
        d = (np.asarray(child_flat, dtype=np.float32) - np.asarray(ref_flat, dtype=np.float32)).astype(np.float32)
        sq = np.zeros(n_blocks(D) * BLOCK)
        sq[:len(m)][lin] = d[m[lin]].astype(np.float64) ** 2
        out = np.empty(n_blocks(D))
        for b, row in enumerate(sq.reshape(-1, BLOCK)):
            out[b] = math.fsum(row.tolist()) if np.isfinite(row).all() else np.sum(row)
    return out


def same_partials(got, want, rtol=1e-12):
    """the kernel's fixed fp64 tree against fsum: relative 1024 * 2^-53 ~ 1.2e-13, asserted at 1e-12; NaN and inf by class"""
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    if not np.array_equal(np.isinf(got), np.isinf(want)):
        return False
    f = np.isfinite(want)
    return bool((np.abs(got[f] - want[f]) <= rtol * np.abs(want[f])).all())


def final_distance(partials):
    """f32(sqrt(fsum(partials))); inf stays inf, NaN stays NaN"""
    p = np.asarray(partials, dtype=np.float64)
    with np.errstate(**_quiet):
        return F32(math.sqrt(math.fsum(p.tolist()))) if np.isfinite(p).all() else F32(np.sqrt(np.sum(p)))


def within_one_ulp(got, want):
    got, want = F32(got), F32(want)
    if np.isnan(want) or np.isinf(want):
        return bool(np.isnan(got)) if np.isnan(want) else bool(got == want)
    return bool(abs(int(got.view(np.int32)) - int(want.view(np.int32))) <= 1)


# ------------------------------------------------------------------------------------------- the ES update
def es_accumulate(f, d, lo, hi):
    """acc = 0; for i in lo..hi-1: acc = fma32(f[i], d[i], acc) -> (fp32 [P], number of terms whose emulation is not provably
    the fused result: see the module docstring)"""
    acc = np.zeros(d.shape[1], dtype=np.float32)
    unsafe = 0
    with np.errstate(**_quiet):
        for i in range(lo, hi):
            a = np.float64(f[i]) * d[i].astype(np.float64)      # exact
            b = acc.astype(np.float64)
            y = a + b
            y32 = y.astype(np.float32)
            fin = np.isfinite(y) & np.isfinite(y32)
            bb = y - a
            err = (a - (y - bb)) + (b - bb)                      # TwoSum: y + err = a + b exactly
            away = np.where(y > y32.astype(np.float64), F32(np.inf), F32(-np.inf)).astype(np.float32)
            nb = np.nextafter(y32, away).astype(np.float64)
            tie = (y != y32.astype(np.float64)) & ((y - y32.astype(np.float64)) == (nb - y))
            unsafe += int(np.count_nonzero(fin & tie & (err != 0)))
            acc = y32
    return acc, unsafe


def es_chunk_bounds(n, chunks):
    return [(c * n // chunks, (c + 1) * n // chunks) for c in range(chunks)]


def es_update(theta, pert, fit, D, sigma, lr, chunks=1):
    """theta' = theta + scale * sum_i f_i (pert_i - theta) over the Linear entries: differences in float32, one fused
    multiply-add per term from 0 with i ascending inside a chunk, chunk sums added left to right,
    scale = f32(lr) / (f32(n) * sigma) -> (theta' fp32 [P], unsafe term count, float64 reference, its error bound)"""
    theta = np.asarray(theta, dtype=np.float32)
    pert = np.asarray(pert, dtype=np.float32)
    f = np.asarray(fit, dtype=np.float32)
    n = len(f)
    with np.errstate(**_quiet):
        d = (pert - theta[None]).astype(np.float32)
        tot, unsafe = None, 0
        for lo, hi in es_chunk_bounds(n, chunks):
            acc, u = es_accumulate(f, d, lo, hi)
            unsafe += u
            tot = acc if tot is None else (tot + acc).astype(np.float32)
        scale = F32(lr) / (F32(n) * F32(sigma))
        out = (theta + (scale * tot).astype(np.float32)).astype(np.float32)
        keep = ln_mask(D)
        out[keep] = theta[keep]
        terms = f.astype(np.float64)[:, None] * d.astype(np.float64)
        ref64 = theta.astype(np.float64) + np.float64(scale) * terms.sum(axis=0)
        bound = (n + 2) * 2.0 ** -24 * abs(np.float64(scale)) * np.abs(terms).sum(axis=0) + 2.0 ** -24 * np.abs(ref64)
        ref64[keep], bound[keep] = theta[keep], 0.0
    return out, unsafe, ref64, bound


ES_N = (1, 15, 16, 17, 32, 33)
ES_CHUNKED = ((50, 3), (5, 8), (33, 64))
ES_FITNESS = ("random", "zeros", "neg_zero", "one_inf", "one_nan", "subnormal", "alt_flt_max")
ES_SIGMAS = (F32(0.05), F32(1e-38))
ES_LR = F32(0.1)
ES_LR_BIG = F32(1000.0)      # with sigma 1e-38 the scale overflows


def es_fitness(kind, n, seed=0):
    f = np.random.Generator(np.random.PCG64(600 + n + seed)).normal(size=n).astype(np.float32)
    if kind == "zeros":
        f[:] = 0
    elif kind == "neg_zero":
        f[::2] = F32(-0.0)
    elif kind == "one_inf":
        f[n // 2] = np.inf
    elif kind == "one_nan":
        f[n - 1] = np.nan
    elif kind == "subnormal":
        f[n // 3] = F32(1e-40)
    elif kind == "alt_flt_max":
        f[:] = FLT_MAX
        f[1::2] = -FLT_MAX
    else:
        assert kind == "random", kind
    return f


ES_SEED, ES_SHI = 99, 3


def es_cases():
    """(D, n, chunks, fitness kind, sigma, lr): the 16 boundary in one launch, chunks that straddle 16 / are empty /
    outnumber the individuals, every fitness vector, and the subnormal sigma 1e-38 with a scale lr / (n sigma) that is huge
    (lr 0.1: 5.9e35) and one that overflows to inf (lr 1000)"""
    s0, s1 = ES_SIGMAS
    out = [((8, 10)[j % 2], n, 1, "random", s0, ES_LR) for j, n in enumerate(ES_N)]
    out += [((10, 8)[j % 2], n, c, "random", s0, ES_LR) for j, (n, c) in enumerate(ES_CHUNKED)]
    out += [((8, 10)[j % 2], 33, 1, kind, s0, ES_LR) for j, kind in enumerate(ES_FITNESS[1:])]
    out += [(10, 17, 1, "random", s1, ES_LR), (8, 50, 3, "random", s1, ES_LR_BIG), (10, 33, 3, "alt_flt_max", s0, ES_LR)]
    return out


@functools.lru_cache(maxsize=4)
def es_inputs(D, n, sigma, kind):
    """-> (theta [P], pert [n][P], fitness [n]): a planted theta (finite plants) and its children bred with LayerNorm kept"""
    theta = planted_parents(D, 1)[0]
    pert = np.stack([child(theta, D, F32(sigma), ES_SEED, i, ES_SHI, 1) for i in range(n)])
    return theta, pert, es_fitness(kind, n)


# ------------------------------------------------------------------------------------------- planted parents
def plant_positions(D):
    """sorted canonical indices: the first and last entry of each of the ten segments, the four entries on each side of
    every segment boundary, and the last (one-element) quad"""
    P, pos = params(D), set()
    for o, n in segments(D):
        pos |= {o, o + n - 1}
        if o:
            pos |= set(range(o - 4, o + 4))
    pos |= {0, 1, 2, 3, P - 1}
    return sorted(p for p in pos if 0 <= p < P)


@functools.lru_cache(maxsize=None)
def planted_parents(D, n, seed=0):
    """fp32 [n][P], read-only: seeded initialisations mutated by sigma 0.05 (as the kernel tests' make_nets), with planted
    values at plant_positions - net 0 takes the finite ones only (+-0, the smallest and largest subnormal, +-FLT_MAX), the
    others +-inf and NaN as well, each net starting somewhere else in the list"""
    torch.manual_seed(9100 + 17 * D + seed)
    nets = np.stack([rp.mutate_torch(rp.init_net(D), D, 0.05) for _ in range(n)]).astype(np.float32)
    pos = plant_positions(D)
    for k in range(n):
        vals = FINITE_PLANTS if k == 0 else ALL_PLANTS
        for j, p in enumerate(pos):
            nets[k, p] = vals[(j + 3 * k) % len(vals)]
    nets.setflags(write=False)
    return nets


def padding_of(net):
    """the finite sentinel planted in net `net`'s padding words"""
    return F32(1000.5 + net)


def plain_nets(D, n, seed):
    torch.manual_seed(9300 + 13 * D + seed)
    return np.stack([rp.mutate_torch(rp.init_net(D), D, 0.05) for _ in range(n)]).astype(np.float32)


# ------------------------------------------------------------------------------------------- perturb cases
SIGMAS = (F32(0.0), F32(1e-41), F32(0.05), F32(3e38), F32(np.inf), F32(np.nan))
WRAP_FIRST = 2 ** 32 - 2        # stream_lo_first of the wrap cases: 4 children take individuals 2^32-2, 2^32-1, 0, 1
GENS = (0, 1, 5, 2 ** 30)       # 4 * 2^30 wraps to 0


SEED = 0x1234567890ABCDEF
N_PARENTS = 3
PIDX = (2, 0, 2, 1, 0)          # unordered and repeated


def perturb_cases():
    """name -> dict(D, sigma, flags, entry, slo_first, shi, gen, pidx): entry "flags" = coevo_fc_perturb_flags, "plain" =
    coevo_fc_perturb, "gen" = coevo_fc_perturb_gen with the generation counter on the device"""
    out = {}

    def add(name, D, sigma=F32(0.05), flags=0, entry="flags", slo_first=1000, shi=7, gen=None, pidx=PIDX):
        out[name] = dict(D=D, sigma=F32(sigma), flags=flags, entry=entry, slo_first=slo_first, shi=shi, gen=gen,
                         pidx=tuple(pidx))
    for i, s in enumerate(SIGMAS):
        for flags in range(4):
            add(f"sigma{i}_flags{flags}", (8, 10)[(i + flags) % 2], sigma=s, flags=flags, slo_first=1000 + 8 * i)
    add("plain_ga", 10, flags=0, entry="plain")
    add("plain_es", 8, flags=1, entry="plain")
    for flags in range(4):      # individuals 2^32-2, 2^32-1, 0, 1: streams wrap through 0, with and without pairing
        add(f"wrap_flags{flags}", (10, 8)[flags % 2], flags=flags, slo_first=WRAP_FIRST, pidx=(1, 0, 2, 0))
    for j, g in enumerate(GENS):
        add(f"gen{j}", (8, 10)[j % 2], flags=j % 4, entry="gen", shi=2 ** 32 - 3, gen=g)   # g = 1, 5: stream_hi wraps too
    return out


def perturb_want(case, parents):
    """the children of a case, canonical order: fp32 [n_children][P]"""
    c = case
    return np.stack([child(parents[p], c["D"], c["sigma"], SEED, c["slo_first"] + k, c["shi"], c["flags"], c["gen"])
                     for k, p in enumerate(c["pidx"])])


# ------------------------------------------------------------------------------------------- Box-Muller
def box_muller64(a, b):
    """float64 Box-Muller of raw words: u1 = (2 (a >> 9) + 1) 2^-24, u2 = (b >> 8) 2^-24 -> [n][2].  cos and sin of
    2 pi u2 are taken after an exact reduction to the first octant so that the float64 result is good to its last bits"""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    u1 = (2 * (a >> np.uint64(9)) + 1).astype(np.float64) * 2.0 ** -24
    k = (b >> np.uint64(8)).astype(np.int64)                    # u2 = k / 2^24
    r = np.sqrt(-2.0 * np.log(u1))
    q, rem = k >> 22, k & (2 ** 22 - 1)                          # quadrant, position inside it (exact)
    x = rem.astype(np.float64) * (2.0 ** -22) * (np.pi / 2)
    c0, s0 = np.cos(x), np.sin(x)
    c = np.select([q == 0, q == 1, q == 2], [c0, -s0, -c0], s0)
    s = np.select([q == 0, q == 1, q == 2], [s0, c0, -s0], -c0)
    return np.stack([r * c, r * s], axis=1)


def log_threshold_mantissas():
    """a >> 9 values whose u1 = (2 m + 1) 2^-24 sits on either side of the mantissa threshold 0.7071... of canon_logf, for each
    exponent -1 ... -24 that has room for one"""
    out = []
    for e in range(1, 25):                         # u1 in [2^-e, 2^-e+1)
        x = math.sqrt(0.5) * 2.0 ** (1 - e)        # the threshold in this binade
        w = x * 2.0 ** 24                          # 2 m + 1 ~ w
        m0 = int((w - 1) // 2)
        for m in (m0 - 1, m0, m0 + 1, m0 + 2):
            if 0 <= m < 2 ** 23:
                out.append(m)
    return sorted(set(out))


def box_muller_edges():
    """-> (a, b) uint32 arrays: the cross product of the edge sets of a >> 9 and b >> 8, placed in the words' top bits"""
    ms = sorted(set([0, 1, 2, 2 ** 22 - 1, 2 ** 22, 2 ** 23 - 2, 2 ** 23 - 1] + log_threshold_mantissas()))
    ks = set([0, 2 ** 24 - 1])
    for j in range(9):
        ks |= {j * 2 ** 21 - 1, j * 2 ** 21, j * 2 ** 21 + 1}
    ks = sorted(k for k in ks if 0 <= k < 2 ** 24)
    a = np.repeat(np.array(ms, dtype=np.uint64) << np.uint64(9), len(ks))
    b = np.tile(np.array(ks, dtype=np.uint64) << np.uint64(8), len(ms))
    return a.astype(np.uint32), b.astype(np.uint32)


def box_muller_sweep(n=1 << 20, seed=2024):
    g = np.random.Generator(np.random.PCG64(seed))
    return (g.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32),
            g.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32))


# the Box-Muller error of the oracle against float64, measured by tests/test_breed_edges_cpu.py over the edge set and the
# 2^20-pair sweep (see its docstring); the test asserts twice these
BM_MAX_ABS = 5.87e-7     # max |z - z64|            (edge set 5.83e-7, sweep 5.86e-7)
BM_MAX_ULP = 3.28        # max |z - z64| / ulp(z64) (edge set 2.44, sweep 3.28); the largest relative error is 2.4e-7
