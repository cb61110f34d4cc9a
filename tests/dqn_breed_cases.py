"""Named inputs and plain references for the fp32 DeepQN population kernels at their edges: dqn_perturb_kernel with its four
code paths per quad, the pack / unpack / relayout moves (csrc/dqn_engine.hip, csrc/deepqn.hip), the chunked ES update with the
three-range BatchNorm skip (coevo_dqn_es_partial / coevo_dqn_es_apply, csrc/offspring.hip) and the synthetic env
(synth_step_kernel).

The slab map is restated here in numpy from the layout comments of csrc/dqn_common.hip.h and calls nothing.  What is not
keyed by the FCNetwork width comes from tests/breed_cases.py: the comparisons, the plant values, the noise table (the oracle's
Philox normals), the fma-emulating ES accumulation and its unsafe-term count, the partial and distance bounds.  Where a
helper there takes D only for its LayerNorm mask, its twin here takes the keep-mask itself.  tests/test_dqn_breed_edges_cpu.py
holds these restatements to the oracle's C code, tests/test_dqn_breed_edges_gpu.py the kernels to the restatements.  No GPU
and no libcoevo needed here."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from coevonet_amd import lib as L
from oracle import ref_port as rp
from tests import breed_cases as bc

F32 = np.float32
M32 = bc.M32
BLOCK = bc.BLOCK                  # slab positions per workgroup of dqn_perturb_kernel = per distance partial
TILED = L.DQN_FC1_TILED           # COEVO_DQN_FC1_TILED, or-ed into the channel argument
FC1_IN, FC1_OUT = 3136, 512
_quiet = dict(over="ignore", invalid="ignore", divide="ignore", under="ignore")

# (C, n_actions): (1, 1) the smallest net, the last quad one live word + three padding words, F_g1 % 4 == 1 (every BatchNorm /
# output-bias Philox block straddles slab quads by one); (3, 5) offset 1 beside a full last quad; (5, 3) offset 3; (6, 32)
# total % 64 == 0: no padding at all, the largest accepted shape
SHAPES = ((1, 1), (3, 5), (5, 3), (6, 32))
LAYOUTS = (0, TILED)
PAIRS = tuple((s, t) for t in LAYOUTS for s in SHAPES)      # index j: shape j % 4, tiled for j >= 4


# ------------------------------------------------------------------------------------------- layout
@functools.lru_cache(maxsize=None)
def layout(C, n):
    """slab offsets: conv weights in MFMA lane order, each followed by its (bias, gamma, beta) triple, the fc1 block, then
    fc1.b, output.w, output.b; stride = total rounded up to 64 words"""
    b1 = C * 64 * 32
    w2 = b1 + 96
    b2 = w2 + 512 * 64
    w3 = b2 + 192
    b3 = w3 + 576 * 64
    wf = b3 + 192
    bf = wf + FC1_OUT * FC1_IN
    wo = bf + FC1_OUT
    bo = wo + n * FC1_OUT
    total = bo + n
    return SimpleNamespace(w1=0, b1=b1, w2=w2, b2=b2, w3=w3, b3=b3, wf=wf, bf=bf, wo=wo, bo=bo, total=total,
                           stride=(total + 63) // 64 * 64)


TENSORS = ("conv1.w", "conv1.b", "conv2.w", "conv2.b", "conv3.w", "conv3.b", "fc1.w", "fc1.b", "output.w", "output.b",
           "vbn1.w", "vbn1.b", "vbn2.w", "vbn2.b", "vbn3.w", "vbn3.b")


def segments(C, n):
    """(offset, length) of the 16 parameter tensors in canonical (torch parameters()) order"""
    sizes = [32 * C * 64, 32, 64 * 512, 64, 64 * 576, 64, FC1_OUT * FC1_IN, FC1_OUT, FC1_OUT * n, n, 32, 32, 64, 64, 64, 64]
    out, off = [], 0
    for s in sizes:
        out.append((off, s))
        off += s
    return out


def params(C, n):
    o, s = segments(C, n)[-1]
    return o + s


def stride(C, n):
    return layout(C, n).stride


def shift(C, n, tiled):
    """quads by which dqn_perturb_kernel shifts its thread -> slab map in the tiled layout: the fc1 block's first quad then
    falls on lane 0 of a wave"""
    return (64 - ((layout(C, n).wf >> 2) & 63)) & 63 if tiled else 0


def n_blocks(C, n, tiled):
    return (stride(C, n) // 4 + shift(C, n, tiled) + 255) // 256


def _conv(i, cout, taps):
    """position i of a conv block holds W[co = 32 np + 16 (e & 1) + lane % 16][tap = 4 (2 qp + e / 2) + lane / 16] with
    i = ((qp * NP + np) * 64 + lane) * 4 + e, NP = cout / 32 -> co * taps + tap"""
    npc = cout // 32
    e, lane, blk = i & 3, (i >> 2) & 63, i >> 8
    np_, qp = blk % npc, blk // npc
    co = 32 * np_ + 16 * (e & 1) + (lane & 15)
    tap = 4 * (2 * qp + (e >> 1)) + (lane >> 4)
    return co * taps + tap


def _fc1(i, tiled):
    """streamed wfq[ob][kq][l][c] = fc1.w[64 ob + l][4 kq + c]; tiled wft[ob][Q][T][l][j] = fc1.w[64 ob + 16 T + l % 16]
    [16 Q + 4 j + l / 16] -> out * 3136 + k"""
    if tiled:
        j, l, T, Q, ob = i & 3, (i >> 2) & 63, (i >> 8) & 3, (i >> 10) % 196, (i >> 10) // 196
        return (ob * 64 + 16 * T + (l & 15)) * FC1_IN + 16 * Q + 4 * j + (l >> 4)
    c, l, kq, ob = i & 3, (i >> 2) & 63, (i >> 8) % 784, (i >> 8) // 784
    return (ob * 64 + l) * FC1_IN + 4 * kq + c


@functools.lru_cache(maxsize=None)
def slab_to_flat(C, n, tiled):
    """int64 [stride]: the canonical flat index held by each slab position, -1 for the padding words"""
    L = layout(C, n)
    F = dict(zip(TENSORS, (o for o, _ in segments(C, n))))
    m = np.full(L.stride, -1, dtype=np.int64)
    ar = lambda k: np.arange(k, dtype=np.int64)
    m[L.w1:L.b1] = F["conv1.w"] + _conv(ar(L.b1), 32, C * 64)
    m[L.w2:L.b2] = F["conv2.w"] + _conv(ar(512 * 64), 64, 512)
    m[L.w3:L.b3] = F["conv3.w"] + _conv(ar(576 * 64), 64, 576)
    for at, k, names in ((L.b1, 32, ("conv1.b", "vbn1.w", "vbn1.b")), (L.b2, 64, ("conv2.b", "vbn2.w", "vbn2.b")),
                         (L.b3, 64, ("conv3.b", "vbn3.w", "vbn3.b"))):
        for j, name in enumerate(names):
            m[at + j * k:at + (j + 1) * k] = F[name] + ar(k)
    m[L.wf:L.bf] = F["fc1.w"] + _fc1(ar(FC1_OUT * FC1_IN), bool(tiled))
    m[L.bf:L.total] = F["fc1.b"] + ar(L.total - L.bf)       # fc1.b, output.w, output.b: contiguous in both orders
    m.setflags(write=False)
    return m


def bn_slab_ranges(C, n):
    """the three [lo, hi) slab ranges of BatchNorm gamma / beta: behind each conv bias"""
    L = layout(C, n)
    return ((L.b1 + 32, L.w2), (L.b2 + 64, L.w3), (L.b3 + 64, L.wf))


@functools.lru_cache(maxsize=None)
def bn_slab_mask(C, n):
    m = np.zeros(stride(C, n), dtype=bool)
    for lo, hi in bn_slab_ranges(C, n):
        m[lo:hi] = True
    return m


@functools.lru_cache(maxsize=None)
def bn_mask(C, n):
    """canonical: the six vbn tensors (they come last)"""
    m = np.zeros(params(C, n), dtype=bool)
    for o, s in segments(C, n)[10:]:
        m[o:o + s] = True
    return m


def to_slab_rows(flat, C, n, tiled, padding):
    """numpy image of a packed net: flat [P] -> [stride] with `padding` in the padding words"""
    m = slab_to_flat(C, n, tiled)
    out = np.full(len(m), padding, dtype=np.float32)
    live = m >= 0
    out[live] = np.asarray(flat, dtype=np.float32)[m[live]]
    return out


def from_slab_row(row, C, n, tiled):
    """-> flat [P]"""
    m = slab_to_flat(C, n, tiled)
    out = np.empty(params(C, n), dtype=np.float32)
    live = m >= 0
    out[m[live]] = np.asarray(row, dtype=np.float32)[live]
    return out


def bit_pattern_rows(C, n, n_nets, seed=5):
    """uint32 [n_nets][stride]: arbitrary bit patterns for the word-moving kernels - random words with two NaN payloads, +-0,
    both subnormal extremes and +-FLT_MAX sprinkled in and at both ends of the fc1 block, a distinct sentinel in each net's
    padding words"""
    L = layout(C, n)
    g = np.random.Generator(np.random.PCG64(seed + 100 * C + n))
    rows = g.integers(0, 2 ** 32, size=(n_nets, L.stride), dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7fc00123, 0xffa00001, 0x00000000, 0x80000000, 0x00000001, 0x007fffff, 0x7f7fffff, 0xff7fffff],
                       dtype=np.uint32)
    for k in range(n_nets):
        at = g.integers(0, L.total, size=4096)
        rows[k, at] = special[np.arange(4096) % len(special)]
        edge = [0, L.b1 - 1, L.b1, L.wf - 1, L.wf, L.wf + 1, L.bf - 2, L.bf - 1, L.bf, L.total - 1]
        rows[k, edge] = special[(np.arange(len(edge)) + k) % len(special)]
        rows[k, L.total:] = 0xdead0000 + k
    return rows


# ------------------------------------------------------------------------------------------- planted parents
N_PARENTS = 3
PIDX = (2, 0, 2, 1, 0)          # unordered and repeated
SEED = 0x1234567890ABCDEF
SMALL_PLANTS = [F32(0.0), F32(-0.0), bc.SUB_MIN, bc.SUB_MAX, -bc.SUB_MIN]


def bn_edge_positions(C, n):
    """canonical indices of the words on both sides of every BatchNorm range boundary in SLAB order (the same in both fc1
    layouts: the first fc1 word is fc1.w[0][0] in either)"""
    m = slab_to_flat(C, n, 0)
    return [int(m[s]) for lo, hi in bn_slab_ranges(C, n) for s in (lo - 1, lo, hi - 1, hi)]


def plant_positions(C, n):
    """sorted canonical indices: the first and last entry of each of the 16 tensors, the four entries on each side of every
    tensor boundary, the first and last word of the fc1 block in slab order (both layouts), both sides of every BatchNorm range
    boundary in slab order"""
    P, pos = params(C, n), set()
    for o, s in segments(C, n):
        pos |= {o, o + s - 1}
        if o:
            pos |= set(range(o - 4, o + 4))
    L = layout(C, n)
    for tiled in LAYOUTS:
        m = slab_to_flat(C, n, tiled)
        pos |= {int(m[L.wf]), int(m[L.bf - 1])}
    pos |= set(bn_edge_positions(C, n))
    return sorted(p for p in pos if 0 <= p < P)


@functools.lru_cache(maxsize=None)
def planted_parents(C, n):
    """fp32 [3][P], read-only: seeded DeepQN initialisations mutated by sigma 0.05 with planted values at plant_positions - net
    0 takes the finite ones only, the others +-inf and the two NaNs as well, each net starting somewhere else in the list.  The
    words on both sides of every BatchNorm range boundary (slab order) then take a small plant (+-0 or a subnormal) in every
    net: +-FLT_MAX there would swallow the noise and hide a skip range that is off by one word"""
    torch.manual_seed(9500 + 100 * C + n)
    nets = []
    for _ in range(N_PARENTS):
        flat, shapes = rp.dqn_init(C, n)
        nets.append(rp.dqn_mutate_torch(flat, shapes, 0.05))
    nets = np.stack(nets).astype(np.float32)
    pos = plant_positions(C, n)
    for k in range(N_PARENTS):
        vals = bc.FINITE_PLANTS if k == 0 else bc.ALL_PLANTS
        for j, p in enumerate(pos):
            nets[k, p] = vals[(j + 3 * k) % len(vals)]
        for j, p in enumerate(bn_edge_positions(C, n)):
            nets[k, p] = SMALL_PLANTS[(j + k) % len(SMALL_PLANTS)]
    nets.setflags(write=False)
    return nets


padding_of = bc.padding_of      # the finite sentinel planted in net k's padding words


@functools.lru_cache(maxsize=None)
def plain_net(C, n, seed):
    torch.manual_seed(9700 + 100 * C + n + 1000 * seed)
    flat, shapes = rp.dqn_init(C, n)
    out = rp.dqn_mutate_torch(flat, shapes, 0.05).astype(np.float32)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------- perturb
def child(parent, C, n, sigma, seed, ind, stream_hi, flags=0, gen=None, gen_bias=0):
    """child = parent + f32(sigma * z[p]) at canonical index p, negated for the odd partner under flag bit 1 (ANTITHETIC); flag
    bit 0 (SKIP_BN) keeps the BatchNorm words (the parent's bits); with a generation counter the stream is
    stream_hi + 4 (gen + gen_bias) mod 2^32"""
    parent = np.asarray(parent, dtype=np.float32)
    shi = (stream_hi + (4 * (gen + gen_bias) if gen is not None else 0)) & M32
    with np.errstate(**_quiet):
        out = (parent + bc.noise(sigma, seed, ind, shi, flags, len(parent))).astype(np.float32)
    if flags & 1:
        keep = bn_mask(C, n)
        out[keep] = parent[keep]
    return out


def perturb_cases():
    """name -> dict(shape, tiled, sigma, flags, slo_first, shi, gen, gen_bias, pidx)"""
    out = {}

    def add(name, pair, sigma=F32(0.05), flags=0, slo_first=1000, shi=7, gen=None, gen_bias=0, pidx=PIDX):
        shape, tiled = pair
        out[name] = dict(shape=shape, tiled=tiled, sigma=F32(sigma), flags=flags, slo_first=slo_first, shi=shi, gen=gen,
                         gen_bias=gen_bias, pidx=tuple(pidx))
    # the 24 sigma / flag combinations: pair (i + 2 flags) % 8 - three per pair, with three different flag values
    for i, s in enumerate(bc.SIGMAS):
        for flags in range(4):
            add(f"sigma{i}_flags{flags}", PAIRS[(i + 2 * flags) % 8], sigma=s, flags=flags, slo_first=1000 + 8 * i)
    # individuals 2^32-2, 2^32-1, 0, 1: streams wrap through 0, with and without pairing
    for flags in range(4):
        for t in range(2):
            add(f"wrap_flags{flags}_layout{t}", PAIRS[4 * t + (flags + t) % 4], flags=flags, slo_first=bc.WRAP_FIRST,
                pidx=(1, 0, 2, 0))
    # the generation counter on the device: stream_hi + 4 (gen + gen_bias) wraps for every gen but 0 with bias 0
    for j, g in enumerate(bc.GENS):
        for b, bias in enumerate((0, -1)):
            for t in range(2):
                add(f"gen{j}_bias{b}_layout{t}", PAIRS[4 * t + (j + b + t) % 4], flags=(j + 2 * b) % 4, shi=2 ** 32 - 3, gen=g,
                    gen_bias=bias, pidx=(1, 0, 2, 0))
    return out


DIST_PIDX = (0, 2, 0, 1)
IN_PLACE = ((1, 1, 0, 1), (5, 3, TILED, 2), (6, 32, TILED, 0), (3, 5, 0, 3))      # (C, n_actions, layout, flags)


def plain_case(shape, tiled, flags, pidx):
    """the children of the distance and in-place tests: sigma 0.05, individuals 1000 ..., stream_hi 7"""
    return dict(shape=tuple(shape), tiled=tiled, sigma=F32(0.05), flags=flags, slo_first=1000, shi=7, gen=None, gen_bias=0,
                pidx=tuple(pidx))


def perturb_want(c):
    """the children of a case, canonical order: fp32 [n_children][P]"""
    (C, n), parents = c["shape"], planted_parents(*c["shape"])
    return np.stack([child(parents[p], C, n, c["sigma"], SEED, c["slo_first"] + k, c["shi"], c["flags"], c["gen"], c["gen_bias"])
                     for k, p in enumerate(c["pidx"])])


# FROM_ORDER (flag 4): child e is individual order[e] of the population bred from the E elites - id 0 the plain copy of elite 0,
# id >= 1 elite (id - 1) % E + noise of stream id - 1.  Each order holds id 0, every residue of (id - 1) % E and an id >= E + 1
ORDERS = {1: (2, 0, 1, 3), 2: (3, 0, 2, 1, 4), 3: (0, 4, 2, 3, 7)}
ORDER_GEN, ORDER_GEN_BIAS, ORDER_SHI = 3, -1, 2 ** 32 - 6


def order_want(C, n, E, with_gen, flags=0):
    parents = planted_parents(C, n)
    gen = ORDER_GEN if with_gen else None
    return np.stack([parents[0].copy() if i == 0 else
                     child(parents[(i - 1) % E], C, n, F32(0.05), SEED, i - 1, ORDER_SHI, flags, gen, ORDER_GEN_BIAS)
                     for i in ORDERS[E]])


# ------------------------------------------------------------------------------------------- fused distance
def dist_partials(child_flat, ref_flat, C, n, tiled):
    """fp64 [n_blocks]: per workgroup of dqn_perturb_kernel, fsum of f64(f32(child - ref))^2 over its LIVE words (BatchNorm
    counts, padding never does).  Workgroup b holds the slab quads 256 b - shift ... 256 b - shift + 255: in the tiled layout
    the block boundaries sit shift(C, n) quads earlier.  A block whose terms are not all finite gets numpy's sum (inf or NaN:
    compared by class)"""
    m = slab_to_flat(C, n, tiled)
    live = m >= 0
    nb, sh = n_blocks(C, n, tiled), 4 * shift(C, n, tiled)
    with np.errstate(**_quiet):
        d = (np.asarray(child_flat, dtype=np.float32) - np.asarray(ref_flat, dtype=np.float32)).astype(np.float32)
        sq = np.zeros(nb * BLOCK)
        sq[sh:sh + len(m)][live] = d[m[live]].astype(np.float64) ** 2
        rows = sq.reshape(nb, BLOCK)
        fin = np.isfinite(rows).all(axis=1)
        out = np.empty(nb)
        for b in range(nb):
            out[b] = math.fsum(rows[b].tolist()) if fin[b] else np.sum(rows[b])
    return out


def dist_ref(C, n, kind):
    """-> (canonical reference net, its padding word): an unrelated net with NaN padding, or one with an inf on an fc1 weight,
    an output weight and a BatchNorm gamma, with a finite sentinel of its own"""
    ref = plain_net(C, n, 6).copy()
    if kind == "inf":
        seg = segments(C, n)
        ref[seg[6][0] + 700001], ref[seg[8][0] + 1], ref[seg[12][0] + 5] = np.inf, -np.inf, np.inf
        return ref, F32(-3000.25)
    assert kind == "unrelated", kind
    return ref, F32(np.nan)


# ------------------------------------------------------------------------------------------- the ES update
def es_update(theta, pert, fit, keep, sigma, lr, chunks=1):
    """breed_cases.es_update with an explicit keep-mask: theta' = theta + scale * sum_i f_i (pert_i - theta) outside `keep`,
    differences in float32, one fused multiply-add per term from 0 with i ascending inside a chunk, chunk sums added left to
    right, scale = f32(lr) / (f32(n) * sigma) -> (theta' fp32 [P], unsafe term count, float64 reference, its error bound)"""
    theta = np.asarray(theta, dtype=np.float32)
    pert = np.asarray(pert, dtype=np.float32)
    f = np.asarray(fit, dtype=np.float32)
    n = len(f)
    with np.errstate(**_quiet):
        d = (pert - theta[None]).astype(np.float32)
        tot, unsafe = None, 0
        for lo, hi in bc.es_chunk_bounds(n, chunks):
            acc, u = bc.es_accumulate(f, d, lo, hi)
            unsafe += u
            tot = acc if tot is None else (tot + acc).astype(np.float32)
        scale = F32(lr) / (F32(n) * F32(sigma))
        out = (theta + (scale * tot).astype(np.float32)).astype(np.float32)
        out[keep] = theta[keep]
        s, sa = np.zeros(len(theta)), np.zeros(len(theta))
        for i in range(n):                         # (term by term: [n][P] float64 would be 450 MB)
            t = np.float64(f[i]) * d[i].astype(np.float64)
            s += t
            sa += np.abs(t)
        ref64 = theta.astype(np.float64) + np.float64(scale) * s
        bound = (n + 2) * 2.0 ** -24 * abs(np.float64(scale)) * sa + 2.0 ** -24 * np.abs(ref64)
        ref64[keep], bound[keep] = theta[keep], 0.0
    return out, unsafe, ref64, bound


ES_SHAPES = ((1, 1), (6, 32))
ES_SIGMAS = bc.ES_SIGMAS            # 0.05 and 1e-38
ES_PERT_NAN = 2                     # the perturbed net whose padding words are NaN (when there are that many)


def es_pert_padding(i):
    return F32(np.nan) if i == ES_PERT_NAN else F32(2000.5 + i)


def es_cases():
    """(shape, n, chunks, fitness kind, sigma, lr, form).  form "one": one partial launch into one block; "two_launch": the
    partials of chunk 0 and of chunks 1 ... by two launches, the second on its shard of the nets; "two_block": two chunks per
    block, the blocks 8 NaN words further apart than their chunks need.  n = 1, 16, 17, 33 in one chunk (below, at and past the
    16-deep loop); chunks that are empty, outnumber the individuals, or split 33 in three; a NaN fitness and alternating
    +-FLT_MAX; sigma 1e-38 with a huge scale (lr 0.1) and one that overflows to inf (lr 1000)"""
    a, b = ES_SHAPES
    s0, s1 = ES_SIGMAS
    lr = bc.ES_LR
    return [(a, 1, 1, "random", s0, lr, "one"), (b, 16, 1, "random", s0, lr, "one"), (a, 17, 1, "random", s0, lr, "one"),
            (b, 33, 1, "random", s0, lr, "one"), (a, 33, 1, "random", s0, lr, "one"),
            (a, 33, 3, "random", s0, lr, "one"), (b, 5, 8, "random", s0, lr, "one"), (a, 33, 64, "random", s0, lr, "one"),
            (b, 33, 3, "random", s0, lr, "two_launch"), (a, 33, 3, "random", s0, lr, "two_block"),
            (b, 5, 8, "random", s0, lr, "two_block"),
            (a, 33, 1, "one_nan", s0, lr, "one"), (b, 33, 1, "alt_flt_max", s0, lr, "one"),
            (a, 17, 1, "random", s1, lr, "one"), (b, 33, 3, "random", s1, bc.ES_LR_BIG, "one")]


def es_id(case):
    (C, n_act), n, chunks, kind, sigma, lr, form = case
    return f"C{C}n{n_act}-n{n}-chunks{chunks}-{kind}-sigma{float(sigma):g}-lr{float(lr):g}-{form}"


@functools.lru_cache(maxsize=1)
def es_inputs(shape, n, sigma):
    """-> (theta [P], pert [n][P]): planted net 0 (finite plants) and n children bred with flags 0 - their BatchNorm words
    DIFFER from theta's, so the skip has something to skip"""
    C, n_act = shape
    theta = planted_parents(C, n_act)[0]
    pert = np.stack([child(theta, C, n_act, F32(sigma), bc.ES_SEED, i, bc.ES_SHI, 0) for i in range(n)])
    pert.setflags(write=False)
    return theta, pert


@functools.lru_cache(maxsize=4)
def es_want(shape, n, chunks, kind, sigma, lr):
    """-> (theta, fitness, theta' fp32, unsafe count, float64 reference, bound); the perturbed nets are es_inputs(...)[1]"""
    theta, pert = es_inputs(shape, n, float(sigma))
    fit = bc.es_fitness(kind, n)
    out, unsafe, ref64, bound = es_update(theta, pert, fit, bn_mask(*shape), F32(sigma), F32(lr), chunks)
    return theta, fit, out, unsafe, ref64, bound


# ------------------------------------------------------------------------------------------- the synthetic env
SYNTH_SEED = 0x5EED1234ABCD
SYNTH_GEN = 3
SYNTH_T = 8
# (effective ordinal or None = game_ordinal0 -10, limit): the counter turns -10 into -10 + 3 ordinals_per_gen = -1 (disabled)
# or 2; a game with a given effective ordinal gets game_ordinal0 = ordinal - 3 ordinals_per_gen
SYNTH_GAMES = ((1, 5), (2 ** 32 + 5, 8), (2 ** 40 + 1, 2), (-1, 5), (None, 8), (None, 1), (0, 0), (2 ** 31, 1))
SYNTH_ROWS = 11                 # frame rows: more than games, so some are never anybody's


def synth_ordinal0(per_gen):
    return np.array([-10 if o is None else o - SYNTH_GEN * per_gen for o, _ in SYNTH_GAMES], dtype=np.int64)


def synth_limits():
    return np.array([l for _, l in SYNTH_GAMES], dtype=np.int32)


def synth_rows(t):
    """game -> frame row at step t: a permutation that changes with every step, so row_prev (that of t - 1) != row_cur"""
    G = len(SYNTH_GAMES)
    return np.array([(5 * g + 3 * t + 1) % SYNTH_ROWS for g in range(G)], dtype=np.int32)


def synth_action(g, t, target, n_actions):
    """the scripted action of game g at step t: the target on every other step, another action in between"""
    return int(target) if (g + t) % 2 == 0 else (int(target) + 1 + g % 3) % n_actions


class SynthRef:
    """The env in plain Python.  t = 0 zeroes the three accumulators and sets last = 0xFF, prev_hit = 0; while t - 1 < limit,
    step t >= 1 books the action of step t - 1 on acc[(t - 1) & 1] += prev_hit - hit; the frame of step t is
    synth_frame(seed, ordinal, t, last, C), written only while t < limit; a negative ordinal disables the game (limit 0)"""

    def __init__(self, ordinal0, limits, gen, per_gen, C, n_actions, seed, gstate, acc):
        self.ordinal = [int(o) + (gen * per_gen if gen is not None else 0) for o in ordinal0]
        self.lim = [0 if o < 0 else int(l) for o, l in zip(self.ordinal, limits)]
        self.C, self.n_actions, self.seed = C, n_actions, seed
        self.gstate, self.acc = np.array(gstate, dtype=np.int32), np.array(acc, dtype=np.float64)

    def target(self, g, t):
        return rp.synth_target(self.seed, self.ordinal[g], t, self.n_actions)

    def step(self, t, row_prev, actions_prev, row_cur, frames):
        """updates state, accumulators and `frames` ([rows][84][84][C] uint8) in place"""
        for g in range(len(self.ordinal)):
            last, prev_hit = int(self.gstate[g, 0]), int(self.gstate[g, 1])
            if t == 0:
                last, prev_hit = 0xFF, 0
                self.acc[g] = 0.0
            elif t - 1 < self.lim[g]:
                a = int(actions_prev[row_prev[g]])
                hit = 1 if a == self.target(g, t - 1) else 0
                self.acc[g, (t - 1) & 1] += float(prev_hit - hit)
                prev_hit, last = hit, a
            self.gstate[g, 0], self.gstate[g, 1] = last, prev_hit
            if t < self.lim[g]:
                frames[row_cur[g]] = rp.synth_frame(self.seed, self.ordinal[g], t, last, self.C)
