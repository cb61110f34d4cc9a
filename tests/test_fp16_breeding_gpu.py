"""Float16 Co-GA breeding on the GPU against the CPU restatement tests/ga16_checker.py, equalities only: the offspring kernel
word for word (coevo_fc16_perturb_dist), its fused distance partials against the standalone kernel's, the finalized
distances, net copies and the promotion against numpy, and whole HalfGAEngine generations (rewards, elite ids, diversity
scores, every net)."""
import functools

import numpy as np
import pytest
import torch

from coevonet_amd import lib as L
from coevonet_amd.ga_half import HalfGAEngine
from oracle import ref_port as rp
from tests import breed_cases as bc
from tests import ga16_checker as gk
from tests.test_fp16_gpu import random_flat
from tests.util import sha

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0x7fc07e00   # NaN as an fp32 word and in both of its halves
SEED = 0x1234567890abcdef


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def pack16(flats, D):
    flats = np.ascontiguousarray(np.stack(flats), dtype=np.float32)
    slab = torch.full((len(flats) * L.fc16_slab_stride(D),), POISON, dtype=torch.int32, device=DEV)
    L.call("coevo_fc16_pack", L._p(torch.from_numpy(flats).to(DEV)), L._p(slab), len(flats), D)
    return slab


def unpack16(slab, first, n, D):
    out = torch.zeros(n, L.fc_param_count(D), dtype=torch.float32, device=DEV)
    L.call("coevo_fc16_unpack", slab.data_ptr() + 4 * first * L.fc16_slab_stride(D), L._p(out), n, D)
    return out.cpu().numpy()


def dev_f32(x):
    return torch.tensor([x], dtype=torch.float32, device=DEV)


def dev_i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def used_words(D):
    """words of a net's stride that hold parameters, asked of the library: a net of ones packs to nonzero words followed by
    the stride's zeroed padding"""
    w = pack16([np.ones(L.fc_param_count(D), dtype=np.float32)], D).cpu().numpy()
    used = int(np.flatnonzero(w)[-1]) + 1
    assert (w[:used] != 0).all() and 0 <= len(w) - used < 64
    return used


CALLS = ((1, 1, 5), (2, 3, 0), (5, 7, 100))   # (child_first, n_children, stream_lo_first): nets 1 .. 11 of 13, parents repeat
STREAM_HI = 9


def breed(parents, D, sigma, flags, with_dist=None):
    """three launches into one poisoned 13-net child slab -> (child slab, parent slab, partials per call)"""
    par = pack16(parents, D)
    stride = L.fc16_slab_stride(D)
    child = torch.full((13 * stride,), POISON, dtype=torch.int32, device=DEV)
    sig = dev_f32(sigma)
    nb = L.fc16_perturb_blocks(D)
    partials = []
    for first, n, slo in CALLS:
        idx = dev_i32([c % len(parents) for c in range(n)])
        part = torch.full((n * nb,), float("nan"), dtype=torch.float64, device=DEV) if with_dist is not None else None
        L.call("coevo_fc16_perturb_dist", L._p(par), L._p(idx), L._p(child), first, n, D, L._p(sig), SEED, slo, STREAM_HI,
               flags, None, L._p(with_dist) if with_dist is not None else None, L._p(part) if part is not None else None)
        partials.append(part)
    torch.cuda.synchronize()
    return child, par, partials


def want_children(parents, D, sigma, flags):
    return {first + c: gk.mutate(parents[c % len(parents)], D, sigma, SEED, slo + c, STREAM_HI, skip_layernorm=bool(flags))
            for first, n, slo in CALLS for c in range(n)}


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("sigma", [0.0, 0.005, 0.5])
@pytest.mark.parametrize("D", [10, 8])
def test_perturb_every_word_against_the_checker(D, sigma, flags):
    rng = np.random.default_rng(100 * D + flags)
    parents = [random_flat(rng, D), random_flat(rng, D, scale=0.15)]
    child, par, _ = breed(parents, D, sigma, flags)
    stride = L.fc16_slab_stride(D)
    words = child.cpu().numpy().view(np.uint32).reshape(13, stride)
    assert (words[0] == POISON).all() and (words[12] == POISON).all(), "a net outside the written range changed"
    got = unpack16(child, 1, 11, D)
    want = want_children(parents, D, sigma, flags)
    m = gk.linear_mask(D)
    pwords = par.cpu().numpy().view(np.uint32).reshape(2, stride)
    # the fp32 child of the upcast parent with the same seed and stream (coevo_fc_perturb)
    par32 = torch.zeros(2 * L.fc_slab_stride(D), dtype=torch.float32, device=DEV)
    L.call("coevo_fc_pack", L._p(torch.from_numpy(np.stack(parents)).to(DEV)), L._p(par32), 2, D)
    child32 = torch.zeros(13 * L.fc_slab_stride(D), dtype=torch.float32, device=DEV)
    sig = dev_f32(sigma)
    for first, n, slo in CALLS:
        L.call("coevo_fc_perturb", L._p(par32), L._p(dev_i32([c % 2 for c in range(n)])), L._p(child32), first, n, D,
               L._p(sig), SEED, slo, STREAM_HI, flags)
    flat32 = torch.zeros(13, L.fc_param_count(D), dtype=torch.float32, device=DEV)
    L.call("coevo_fc_unpack", L._p(child32), L._p(flat32), 13, D)
    flat32 = flat32.cpu().numpy()
    owner = {first + c: c % 2 for first, n, slo in CALLS for c in range(n)}   # the parent of each written net
    for net in range(1, 12):
        assert np.array_equal(bits(got[net - 1]), bits(want[net])), (net, "differs from the checker")
        assert (words[net, used_words(D):] == 0).all(), "the stride's padding words are the parent's zeros"
        with np.errstate(over="ignore"):
            assert np.array_equal(bits(got[net - 1][m]), bits(flat32[net][m].astype(np.float16).astype(np.float32)))
        assert np.array_equal(bits(got[net - 1][~m]), bits(flat32[net][~m]))
        if sigma == 0.0:
            assert np.array_equal(words[net], pwords[owner[net]]), "sigma 0 must reproduce the parent's words"
        if flags:
            assert np.array_equal(bits(got[net - 1][~m]), bits(parents[owner[net]][~m]))


@pytest.mark.parametrize("D", [10, 8])
def test_generation_counter_on_the_device_shifts_the_noise_stream(D):
    """gen_dev: the launch reads the generation g from device memory and draws from stream_hi + 4 g"""
    rng = np.random.default_rng(40 + D)
    parents = [random_flat(rng, D), random_flat(rng, D, scale=0.1)]
    par = pack16(parents, D)
    stride = L.fc16_slab_stride(D)
    idx, sig, g = dev_i32([0, 1, 0]), dev_f32(0.05), dev_i32([3])
    slabs = []
    for stream_hi, gen_dev in ((2, L._p(g)), (2 + 4 * 3, None)):
        child = torch.full((5 * stride,), POISON, dtype=torch.int32, device=DEV)
        L.call("coevo_fc16_perturb_dist", L._p(par), L._p(idx), L._p(child), 1, 3, D, L._p(sig), SEED, 7, stream_hi, 0, gen_dev,
               None, None)
        slabs.append(child)
    torch.cuda.synchronize()
    assert torch.equal(slabs[0], slabs[1]) and int(g.item()) == 3
    got = unpack16(slabs[0], 1, 3, D)
    for c in range(3):
        assert np.array_equal(bits(got[c]), bits(gk.mutate(parents[c % 2], D, 0.05, SEED, 7 + c, 14)))
    words = slabs[0].cpu().numpy().view(np.uint32).reshape(5, stride)
    assert (words[0] == POISON).all() and (words[4] == POISON).all()


@pytest.mark.parametrize("D", [10, 8])
def test_noise_is_the_philox_normal_of_the_canonical_index(D):
    """zero parents and sigma 1: a LayerNorm entry of the child IS eps(p), a Linear entry is f16(eps(p)); spot checks in W2h,
    W1h, W3h, each bias and gamma / beta"""
    P = rp.param_count(D)
    child, _, _ = breed([np.zeros(P, dtype=np.float32)], D, 1.0, 0)
    got = unpack16(child, 1, 11, D)
    o_b1, o_w2 = D * 512, D * 512 + 1536
    o_b2 = o_w2 + 512 * 256
    o_w3, o_b3 = o_b2 + 768, o_b2 + 768 + 1280
    spots = [0, 1, D - 1, D, 511 * D + D - 1, 2500,                         # fc1.weight -> W1h
             o_b1, o_b1 + 511, o_b1 + 512, o_b1 + 1023, o_b1 + 1024, o_b1 + 1535,   # fc1.bias, ln1 gamma, ln1 beta
             o_w2, o_w2 + 7, o_w2 + 8, o_w2 + 513, o_w2 + 70001, o_b2 - 1,   # fc2.weight -> W2h
             o_b2, o_b2 + 255, o_b2 + 256, o_b2 + 511, o_b2 + 512, o_b2 + 767,
             o_w3, o_w3 + 9, o_b3 - 1, o_b3, o_b3 + 3, o_b3 + 4]
    assert spots[-1] == P - 1
    m = gk.linear_mask(D)
    z = torch.zeros(4, dtype=torch.float32, device=DEV)
    for net, (first, c, slo) in ((1, (1, 0, 5)), (4, (2, 2, 0)), (11, (5, 6, 100))):
        for p in spots:
            L.call("coevo_philox_normals", SEED, slo + c, STREAM_HI, p // 4, 1, L._p(z))
            eps = z.cpu().numpy()[p % 4]
            want = np.float32(np.float16(eps)) if m[p] else eps
            assert bits(got[net - 1][p]) == bits(want), (net, p)


def test_overflow_and_subnormal_parents():
    D = 8
    m = gk.linear_mask(D)
    P = rp.param_count(D)
    rng = np.random.default_rng(1)
    big = np.where(m, np.float32(65504) * np.where(np.arange(P) % 2, -1, 1), rng.normal(1, 0.1, P)).astype(np.float32)
    sub = np.where(m, (np.arange(P) % 1023 + 1).astype(np.uint16).view(np.float16).astype(np.float32), np.float32(1.0)).astype(np.float32)
    for parent, sigma in ((big, 30.0), (sub, 0.0), (sub, 2e-6)):
        child, par, _ = breed([parent], D, sigma, 0)
        got = unpack16(child, 1, 11, D)
        want = want_children([parent], D, sigma, 0)
        for net in range(1, 12):
            assert np.array_equal(bits(got[net - 1]), bits(want[net])), (sigma, net)
        if parent is big:
            assert np.isinf(got[:, m]).sum() > 1000 and np.array_equal(np.isinf(got[0]), np.isinf(want[1]))
        else:
            tiny = (np.abs(got[:, m]) < 6.1e-5) & (got[:, m] != 0)
            assert tiny.mean() > 0.9, "fp16 subnormals were flushed"


def test_bad_arguments_return_err_arg_and_write_nothing():
    D = 10
    rng = np.random.default_rng(2)
    par = pack16([random_flat(rng, D)], D)
    stride = L.fc16_slab_stride(D)
    child = torch.full((3 * stride,), POISON, dtype=torch.int32, device=DEV)
    idx, sig = dev_i32([0, 0]), dev_f32(0.1)
    nb = L.fc16_perturb_blocks(D)
    part = torch.full((2 * nb,), float("nan"), dtype=torch.float64, device=DEV)
    lib = L.load()
    assert nb == -(-stride // 4 // 256) and lib.coevo_fc16_perturb_blocks(9) == -1
    good = dict(parent=L._p(par), idx=L._p(idx), child=L._p(child), first=1, n=2, D=D, sig=L._p(sig), flags=0, ref=L._p(par),
                part=L._p(part))

    def call(**kw):
        a = dict(good, **kw)
        return lib.coevo_fc16_perturb_dist(a["parent"], a["idx"], a["child"], a["first"], a["n"], a["D"], a["sig"], SEED, 0, 0,
                                           a["flags"], None, a["ref"], a["part"], L._stream())

    bad = [dict(parent=None), dict(idx=None), dict(child=None), dict(sig=None), dict(D=9), dict(D=0), dict(n=-1), dict(n=65536),
           dict(first=-1), dict(parent=L._p(par) + 4), dict(child=L._p(child) + 8), dict(ref=L._p(par) + 4), dict(ref=None),
           dict(part=None), dict(flags=2), dict(flags=-1)]
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(n=0) == 0 and call(n=0, ref=None, part=None) == 0
    assert lib.coevo_fc16_distance(None, L._p(par), 1, D, L._p(part), L._stream()) == -1
    assert lib.coevo_fc16_distance(L._p(par), L._p(par) + 4, 1, D, L._p(part), L._stream()) == -1
    assert lib.coevo_fc16_distance(L._p(par), L._p(par), 1, 9, L._p(part), L._stream()) == -1
    assert lib.coevo_fc16_distance(L._p(par), L._p(par), 1, D, None, L._stream()) == -1
    assert lib.coevo_fc16_distance(L._p(par), L._p(par), 0, D, L._p(part), L._stream()) == 0
    assert lib.coevo_fc16_distance_finalize(None, nb, 1, L._p(sig), 0, None, L._stream()) == -1
    assert lib.coevo_fc16_distance_finalize(L._p(part), nb, 1, L._p(sig), 0, L._p(sig), L._stream()) == -1   # head needs first >= 1
    assert lib.coevo_fc16_gather(L._p(par), L._p(idx), L._p(child) + 4, 0, 1, D, L._stream()) == -1
    assert lib.coevo_fc16_gather(L._p(par), None, L._p(child), 0, 1, D, L._stream()) == -1
    assert lib.coevo_fc16_gather(L._p(par), L._p(idx), L._p(child), 0, 0, D, L._stream()) == 0
    role = (L.GaPromoteRole * 1)(L.GaPromoteRole(L._p(child), L._p(child), L._p(child), L._p(idx), D, 1, 1, 0))
    assert lib.coevo_ga16_promote(role, 1, 9, 1, L._stream()) == -1 and lib.coevo_ga16_promote(role, 1, 1, 17, L._stream()) == -1
    assert lib.coevo_ga16_promote(role, 4, 1, 1, L._stream()) == -1 and lib.coevo_ga16_promote(None, 1, 1, 1, L._stream()) == -1
    role[0].order = None
    assert lib.coevo_ga16_promote(role, 1, 1, 1, L._stream()) == -1
    role[0].order, role[0].hof = L._p(idx), L._p(child) + 4
    assert lib.coevo_ga16_promote(role, 1, 1, 1, L._stream()) == -1
    torch.cuda.synchronize()
    assert (child.cpu().numpy().view(np.uint32) == POISON).all() and torch.isnan(part).all()
    assert float(sig.item()) == np.float32(0.1)


@pytest.mark.parametrize("D", [10, 8])
def test_fused_partials_equal_the_standalone_kernel_and_distances_equal_the_checker(D):
    rng = np.random.default_rng(7 + D)
    parents = [random_flat(rng, D), random_flat(rng, D, scale=0.1)]
    stale = random_flat(rng, D)
    ref = pack16([stale], D)
    sigma = 0.05
    child, _, fused = breed(parents, D, sigma, 0, with_dist=ref)
    nb = L.fc16_perturb_blocks(D)
    stride = L.fc16_slab_stride(D)
    alone = torch.full((11 * nb,), float("nan"), dtype=torch.float64, device=DEV)
    L.call("coevo_fc16_distance", L._p(ref), child.data_ptr() + 4 * stride, 11, D, L._p(alone))
    torch.cuda.synchronize()
    got = torch.cat(fused).cpu().numpy()
    assert np.array_equal(got.view(np.uint64), alone.cpu().numpy().view(np.uint64))
    assert np.isfinite(got).all() and (got > 0).sum() > 10 * nb
    want = want_children(parents, D, sigma, 0)
    dist = torch.full((13,), float("nan"), dtype=torch.float32, device=DEV)
    head = dev_f32(np.float32(np.float16(3.14159)))
    L.call("coevo_fc16_distance_finalize", L._p(alone), nb, 11, L._p(dist), 1, L._p(head))
    # a net against itself and against a one-entry neighbour, through the standalone kernel
    near = stale.copy()
    near[3] = np.float32(np.float16(near[3]) + np.float16(0.25))
    two = pack16([stale, near], D)
    p2 = torch.zeros(2 * nb, dtype=torch.float64, device=DEV)
    d2 = torch.full((2,), float("nan"), dtype=torch.float32, device=DEV)
    L.call("coevo_fc16_distance", L._p(ref), L._p(two), 2, D, L._p(p2))
    L.call("coevo_fc16_distance_finalize", L._p(p2), nb, 2, L._p(d2), 0, None)
    torch.cuda.synchronize()
    dist = dist.cpu().numpy()
    assert bits(dist[0]) == bits(head.cpu().numpy()[0]) and np.isnan(dist[12])
    for net in range(1, 12):
        w = gk.distance(want[net], stale, D)
        assert bits(dist[net]) == bits(w) and np.float32(np.float16(w)) == w, (net, dist[net], w)
    d2 = d2.cpu().numpy()
    assert bits(d2[0]) == bits(np.float32(0)) and bits(d2[1]) == bits(gk.distance(near, stale, D)) and d2[1] > 0


@pytest.mark.parametrize("hof", [1, 2, 3])
@pytest.mark.parametrize("E", [1, 2])
def test_gather_and_promote_against_numpy(E, hof):
    rng = np.random.default_rng(10 * E + hof)
    pop = 5
    Ds = (10, 10, 8)
    counts = (("guard0", 1), ("pop", pop), ("hof", hof), ("elite", E), ("guard1", 1))
    slabs, before, orders = [], [], []
    roles = (L.GaPromoteRole * 3)()
    for ri, D in enumerate(Ds):
        stride = L.fc16_slab_stride(D)
        n = sum(c for _, c in counts)
        w = rng.integers(-2 ** 31, 2 ** 31, size=(n, stride), dtype=np.int64).astype(np.int32)
        t = torch.from_numpy(w).to(DEV)
        order = np.concatenate([[pop - 1], rng.permutation(pop - 1)]).astype(np.int32)   # elite[0] = the last individual
        od = torch.from_numpy(order).to(DEV)
        at = {}
        k = 0
        for name, c in counts:
            at[name] = k
            k += c
        roles[ri] = L.GaPromoteRole(t.data_ptr() + 4 * stride * at["pop"], t.data_ptr() + 4 * stride * at["hof"],
                                    t.data_ptr() + 4 * stride * at["elite"], L._p(od), D, 1, 1, 0)
        slabs.append((t, at, od))
        before.append(w)
        orders.append(order)
    L.call("coevo_ga16_promote", roles, 3, E, hof)
    torch.cuda.synchronize()
    for (t, at, _), w, order in zip(slabs, before, orders):
        got = t.cpu().numpy()
        want = w.copy()
        p, h, e = at["pop"], at["hof"], at["elite"]
        for k in range(E):
            want[e + k] = w[p + order[k]]
        for i in range(hof - 1):
            want[h + i] = w[h + i + 1]
        want[h + hof - 1] = w[p + order[0]]
        want[p] = w[p + order[0]]
        assert np.array_equal(got, want)
        assert np.array_equal(got[p + 1:p + pop], w[p + 1:p + pop]) and np.array_equal(got[[0, -1]], w[[0, -1]])
        if hof == 1:
            assert np.array_equal(got[h], w[p + pop - 1])
    # coevo_fc16_gather: dst[2 + i] = src[idx[i]]
    for D in (10, 8):
        stride = L.fc16_slab_stride(D)
        src = rng.integers(-2 ** 31, 2 ** 31, size=(4, stride), dtype=np.int64).astype(np.int32)
        dst = rng.integers(-2 ** 31, 2 ** 31, size=(6, stride), dtype=np.int64).astype(np.int32)
        ts, td = torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV)
        L.call("coevo_fc16_gather", L._p(ts), L._p(dev_i32([3, 0, 3])), L._p(td), 2, 3, D)
        want = dst.copy()
        want[2:5] = src[[3, 0, 3]]
        assert np.array_equal(td.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------- promotion and gather, corners
# coevo_ga16_promote is coevo_ga_promote on 16-byte pieces of fp16 slabs (the same compile-time recursions, role selection and
# host checks: csrc/promote_roles.hip.h; tests/test_breed_edges_gpu.py holds the fp32 launch), and coevo_fc16_gather runs the
# copy kernel of coevo_net_gather: the fp32 suite's corners here, on raw 32-bit words compared as integers, against list
# operations - never against the fp32 launch.
ROLE_D16 = (10, 10, 8)
GUARD = 0x5A5A5A5A


class Region16:
    """n fp16-slab nets of raw words between one guard net on each side.  Net i carries, besides random words, an fp32 NaN
    whose halves are an fp16 NaN and an fp16 subnormal (0x7fc00001 + i), a negative one (0xffc00000 + i), an fp32 subnormal
    (1 + i) and a pair of fp16 NaN halves (0x7e007e01 + i), each in every fifth word."""

    def __init__(self, n, D, rng):
        self.n, self.stride = n, L.fc16_slab_stride(D)
        w = rng.integers(0, 2 ** 32, size=(n + 2, self.stride), dtype=np.uint64).astype(np.uint32)
        for i in range(n):
            for k, pattern in enumerate((0x7FC00001, 0xFFC00000, 1, 0x7E007E01)):
                w[1 + i, k::5] = pattern + i
        w[0] = w[-1] = GUARD
        self.t = torch.from_numpy(w.view(np.int32)).to(DEV)
        self.p = self.t.data_ptr() + 4 * self.stride
        self.before = w[1:-1].copy()

    def rows(self):
        """-> the n nets as uint32 rows, after asserting the guard nets"""
        a = self.t.cpu().numpy().view(np.uint32)
        assert (a[0] == GUARD).all() and (a[-1] == GUARD).all(), "a guard net was written"
        return a[1:-1]


def promote16_case(E, hof, n_roles, variant):
    n_pop = 10
    rng = np.random.default_rng(1000 * E + 10 * hof + n_roles)
    roles, checks = (L.GaPromoteRole * n_roles)(), []
    for r in range(n_roles):
        D = ROLE_D16[r]
        kind = (r + variant) % 3
        pop, hofs, elite = Region16(n_pop, D, rng), Region16(hof, D, rng), Region16(E, D, rng)
        if kind == 0:      # the best already sits in pop[0] and is written back onto itself; the rest distinct
            ids, from_pop, to_pop0 = [0] + list(1 + rng.permutation(n_pop - 1)[:E - 1]), 1, 1
        elif kind == 1:    # pop's last net is the best, an id repeats, pop[0] is left alone
            ids, from_pop, to_pop0 = [n_pop - 1] + [3] * (E - 1), 1, 0
            if E > 2:
                ids[2] = n_pop - 1
        else:              # the elites are in place already: read, not written; no order at all
            ids, from_pop, to_pop0 = None, 0, 1
        order = dev_i32(ids) if ids is not None else None
        roles[r] = L.GaPromoteRole(pop.p, hofs.p, elite.p, L._p(order), D, from_pop, to_pop0, 0)
        checks.append((ids, from_pop, to_pop0, pop, hofs, elite, order))
    L.call("coevo_ga16_promote", roles, n_roles, E, hof)
    torch.cuda.synchronize()
    for r, (ids, from_pop, to_pop0, pop, hofs, elite, _) in enumerate(checks):
        want_p, want_h, want_e = bc.promote(list(pop.before), list(hofs.before), list(elite.before), ids, E, from_pop, to_pop0)
        for name, got, want in (("pop", pop.rows(), want_p), ("hof", hofs.rows(), want_h), ("elite", elite.rows(), want_e)):
            assert len(got) == len(want)
            for k in range(len(want)):
                assert np.array_equal(got[k], want[k]), (variant, r, name, k)


@pytest.mark.parametrize("n_roles", [1, 2, 3])
@pytest.mark.parametrize("E,hof", [(1, 1), (1, 16), (8, 1), (8, 16), (3, 2)])
def test_promote16_corners_vs_list_operations(E, hof, n_roles):
    """every (E, hof) corner of the compile-time recursions on fp16 slabs, one to three roles of mixed width (the D = 8 role's
    surplus workgroup leaves without writing: its regions end in guard nets), the three aliasing kinds of the fp32 suite's
    promote_case; words that are NaN or subnormal as fp32 and as fp16 halves travel as integers"""
    for variant in range(3 if n_roles == 1 else 2):
        promote16_case(E, hof, n_roles, variant)


@pytest.mark.parametrize("D", [10, 8])
def test_gather16_edges(D):
    """coevo_fc16_gather: n = 0 writes nothing, a repeated index, dst_first > 0, every destination region between guard nets;
    bad arguments return ERR_ARG and write nothing"""
    rng = np.random.default_rng(40 + D)
    lib, st = L.load(), L._stream()
    src, dst = Region16(4, D, rng), Region16(6, D, rng)
    idx = dev_i32([3, 0, 3, 1])
    assert lib.coevo_fc16_gather(src.p, L._p(idx), dst.p, 2, 0, D, st) == 0
    bad = [(None, L._p(idx), dst.p, 0, 1, D), (src.p, None, dst.p, 0, 1, D), (src.p, L._p(idx), None, 0, 1, D),
           (src.p, L._p(idx), dst.p, 0, 1, 9), (src.p, L._p(idx), dst.p, 0, -1, D), (src.p, L._p(idx), dst.p, 0, 65536, D),
           (src.p, L._p(idx), dst.p, -1, 1, D), (src.p + 4, L._p(idx), dst.p, 0, 1, D), (src.p, L._p(idx), dst.p + 8, 0, 1, D)]
    for args in bad:
        assert lib.coevo_fc16_gather(*args, st) == -1, args
    torch.cuda.synchronize()
    assert np.array_equal(dst.rows(), dst.before) and np.array_equal(src.rows(), src.before)
    L.call("coevo_fc16_gather", src.p, L._p(idx), dst.p, 2, 4, D)      # dst[2 .. 5] = src[3, 0, 3, 1]: up to the guard net
    L.call("coevo_fc16_gather", src.p, idx.data_ptr() + 4, dst.p, 0, 1, D)   # dst[0] = src[0]
    torch.cuda.synchronize()
    want = dst.before.copy()
    want[2:6] = src.before[[3, 0, 3, 1]]
    want[0] = src.before[0]
    assert np.array_equal(dst.rows(), want) and np.array_equal(src.rows(), src.before)


# ---------------------------------------------------------------------------------------------- whole generations
SIGMAS = {"agent_0": 0.05, "agent_1": 0.02, "adversary_0": 0.1}
CONFIGS = {"pop6": dict(pop=6, hof=2, elites=2, limit_train=6, limit_eval=6, max_cycles=25, torch_seed=3, philox_seed=11),
           "pop4": dict(pop=4, hof=1, elites=1, limit_train=None, limit_eval=None, max_cycles=3, torch_seed=4, philox_seed=5)}
GENERATIONS = 2


def initial_nets(cfg):
    torch.manual_seed(cfg["torch_seed"])
    hof, popu = rp.ga_initial(cfg["pop"], cfg["hof"])
    rnd = lambda d: {r: np.stack([gk.round_linear(w, gk.ROLE_D[r]) for w in d[r]]) for r in gk.ROLES}   # noqa: E731
    return rnd(popu), rnd(hof)


@functools.lru_cache(maxsize=None)
def checker_run(name):
    """the checker's two generations of a configuration, computed once: per generation the record and the nets after it"""
    cfg = CONFIGS[name]
    pop_flat, hof_flat = initial_nets(cfg)
    st = gk.State(pop_flat, hof_flat)
    out = []
    for gen in range(GENERATIONS):
        rec = gk.generation(st, gen, SIGMAS, cfg["elites"], cfg["limit_train"], cfg["limit_eval"], cfg["max_cycles"],
                            cfg["philox_seed"])
        rec["nets"] = {(r, region): [sha(w) for w in nets[r]] for r in gk.ROLES
                       for region, nets in (("pop", st.popu), ("hof", st.hof), ("elite", st.elites))}
        out.append(rec)
    return out


def engine(cfg):
    eng = HalfGAEngine(cfg["pop"], cfg["hof"], cfg["elites"], cfg["limit_train"], cfg["limit_eval"], cfg["max_cycles"],
                       philox_seed=cfg["philox_seed"])
    eng.load_initial(*initial_nets(cfg))
    return eng


def engine_nets(eng):
    counts = {"pop": eng.pop, "hof": eng.hof, "elite": eng.E}
    return {(r, region): [sha(w) for w in eng.download(r, region, 0, n)] for r in gk.ROLES for region, n in counts.items()}


def eq64(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_whole_generations_against_the_checker(name):
    cfg = CONFIGS[name]
    want = checker_run(name)
    ties = sum(rec["tie"][r] for n in CONFIGS for rec in checker_run(n) for r in gk.ROLES)   # over BOTH configurations
    assert ties <= 1, "choose seeds whose fitnesses do not tie: at most one role-generation may skip the elite-id comparison"
    eng = engine(cfg)
    steps = {"elite_ids": [], "eval_rewards": [], "diversity": []}
    for gen, rec in enumerate(want):
        eng.rollout(gen)
        rew = eng.rewards_host()
        assert eq64(rew[:eng.n_main], rec["games"]), (gen, "main games")
        if gen > 0:
            assert eq64(rew[eng.n_main:], want[gen - 1]["eval_games"]), (gen, "evaluation games of the generation before")
            ev = eng.eval_rewards()
            assert ev == want[gen - 1]["eval_rewards"]
            steps["eval_rewards"].append(ev)
        eng.select()
        ids, div = eng.elite_ids(), eng.diversity()
        for r in gk.ROLES:
            assert bits(div[r]) == bits(rec["diversity"][r]), (gen, r, div[r], rec["diversity"][r])
            assert np.array_equal(bits(eng.fitness[r].cpu().numpy()), bits(rec["fitness"][r])), (gen, r)
            if not rec["tie"][r]:
                assert ids[r] == rec["elite_ids"][r], (gen, r)
        steps["elite_ids"].append(ids)
        steps["diversity"].append(div)
        eng.breed(gen, SIGMAS)
        assert engine_nets(eng) == rec["nets"], (gen, "nets after breeding")
    ev = eng.eval_only(GENERATIONS - 1)
    assert eq64(eng.rewards_host()[eng.n_main:], want[-1]["eval_games"]) and ev == want[-1]["eval_rewards"]
    steps["eval_rewards"].append(ev)
    # a second engine with the same seeds, driven by run(): the same arrays
    eng2 = engine(cfg)
    res = eng2.run(GENERATIONS, SIGMAS)
    assert res["elite_ids"] == steps["elite_ids"] and res["eval_rewards"] == steps["eval_rewards"]
    assert [{r: int(bits(d[r])[0]) for r in gk.ROLES} for d in res["diversity"]] == \
        [{r: int(bits(d[r])[0]) for r in gk.ROLES} for d in steps["diversity"]]
    assert engine_nets(eng2) == engine_nets(eng)
    assert np.array_equal(eng2.slab.cpu().numpy(), eng.slab.cpu().numpy())
    for r in gk.ROLES:
        assert np.array_equal(bits(eng2.dist[r].cpu().numpy()), bits(eng.dist[r].cpu().numpy()))
