"""The selection kernels (csrc/select.hip) through the C ABI at NaN, zero spread, ties and the 256-wide ranking slices,
against the plain numpy / fsum references of tests/select_cases.py - never against another kernel, the oracle's C code or a
checker.  Equalities only: finite values as bits, NaN by NaN-ness (the inputs are order-proof, see select_cases).  Every
output buffer starts as a sentinel with guard words on both sides, and what a launch must not touch is asserted untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

from coevonet_amd import genetic_algorithm as ga
from coevonet_amd import lib as L
from oracle import ref_port as rp
from tests import select_cases as sc
from tests.util import Bag

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
PAD = 4
SENT = {torch.float32: -7.25, torch.float64: -7.25, torch.int32: -99}
SIG = ("mutation_power_agent_0", "mutation_power_agent_1", "mutation_power_adversary")
KINDS = ("random", "zeros", "one_zero", "one_inf", "one_nan", "two_inf", "all_equal", "subnormal", "overflow")
FUSED_POPS = (1, 2, 256, 257, 513, 4096)


# ------------------------------------------------------------------------------------------- plumbing
def dev(a):
    """a device copy; the caller holds it in a name until the launch's results are read (a temporary's block is handed out again
    by the caching allocator as soon as the next tensor is made)"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Out:
    """an output buffer of n words between PAD guard words, all of it the dtype's sentinel"""

    def __init__(self, n, dtype=torch.float32):
        self.n, self.sent = n, SENT[dtype]
        self.buf = torch.full((n + 2 * PAD,), self.sent, dtype=dtype, device=DEV)
        self.t = self.buf[PAD:PAD + n]
        self.p = L._p(self.t)

    def get(self):
        """-> the n words, after asserting the guards"""
        a = self.buf.cpu().numpy()
        assert (a[:PAD] == self.sent).all() and (a[PAD + self.n:] == self.sent).all(), "a guard word was written"
        return a[PAD:PAD + self.n]

    def untouched(self):
        return bool((self.get() == self.sent).all())


def to_slab(flat_np, D, poison_padding=True):
    n = flat_np.shape[0]
    slab = torch.zeros(n, L.fc_slab_stride(D), dtype=torch.float32, device=DEV)
    flat = dev(flat_np.astype(np.float32))
    L.call("coevo_fc_pack", L._p(flat), L._p(slab), n, D)
    if poison_padding:   # nothing past fc_param_count(D) belongs to the net
        slab[:, L.fc_param_count(D):] = float("nan")
    return slab


def refused(name, *args):
    with pytest.raises(L.CoevoError):
        L.call(name, *args)


# ------------------------------------------------------------------------------------------- distances
def _ln_poison(nets, D):
    """LayerNorm gamma / beta of the nets set to 1e30 and NaN: the distance is over the Linear entries only"""
    out = np.array(nets, dtype=np.float32, copy=True)
    for o, n in rp.ln_segments(D):
        out[..., o:o + n:2] = 1e30
        out[..., o + 1:o + n:2] = np.nan
    return out


def _first_linear(D, k):
    """the k-th Linear segment's offset (fc1.weight, fc1.bias, fc2.weight, fc2.bias, output.weight, output.bias)"""
    return rp.linear_segments(D)[k][0]


@pytest.mark.parametrize("n", [1, 3, 23])
@pytest.mark.parametrize("D", [8, 10])
def test_fc_distance_and_diversity_vs_fsum(D, n):
    ref, nets, _ = sc.dist_nets(D, n)
    assert L.fc_slab_stride(D) > L.fc_param_count(D) == rp.param_count(D)
    want = np.array([sc.contract_dist(ref, w, D) for w in nets], dtype=np.float32)
    # the population, then the reference itself (exact +0) and a net with one infinite fc2 weight (inf) - all with wild LayerNorms
    hot = nets[0].copy()
    hot[_first_linear(D, 2) + 70001] = np.inf
    pop = _ln_poison(np.concatenate([nets, ref[None], hot[None]]), D)
    ref_slab, slab = to_slab(ref[None], D), to_slab(pop, D)
    dist, dist2, score = Out(n + 2), Out(n), Out(1)
    L.call("coevo_fc_distance", L._p(ref_slab), L._p(slab), n + 2, D, dist.p)
    L.call("coevo_fc_diversity", L._p(ref_slab), L._p(slab), n, D, dist2.p, score.p)
    got, got2, got_s = dist.get(), dist2.get(), score.get()
    print(D, n, "dist", got[:3], "want", want[:3], "score", got_s, sc.contract_score(want))
    assert sc.same_f32(got[:n], want) and sc.same_f32(got2, want)
    assert got[n].view(np.uint32) == 0 and got[n + 1] == np.inf
    assert sc.same_f32(got_s, sc.contract_score(want))


@pytest.mark.parametrize("D", [8, 10])
def test_fc_distance_inf_minus_inf_and_subnormal_differences(D):
    ref, nets, _ = sc.dist_nets(D, 3)
    k = _first_linear(D, 4) + 3   # an output.weight entry
    ref = ref.copy()
    ref[k] = np.inf
    pop = nets.copy()
    pop[0, k], pop[1, k] = np.inf, -np.inf            # inf - inf = NaN; -inf - inf = -inf, squared inf; finite - inf: inf
    dist = Out(3)
    ref_slab, slab = to_slab(ref[None], D), to_slab(pop, D)
    L.call("coevo_fc_distance", L._p(ref_slab), L._p(slab), 3, D, dist.p)
    got = dist.get()
    assert np.isnan(got[0]) and got[1] == np.inf and got[2] == np.inf
    assert sc.same_f32(got, [sc.contract_dist(ref, w, D) for w in pop])
    sref, snets = sc.subnormal_nets(D, 3)
    want = np.array([sc.contract_dist(sref, w, D) for w in snets], dtype=np.float32)
    assert (want > 0).all() and (want < 1e-30).all()
    dist = Out(3)
    ref_slab, slab = to_slab(sref[None], D), to_slab(snets, D)
    L.call("coevo_fc_distance", L._p(ref_slab), L._p(slab), 3, D, dist.p)
    assert sc.same_f32(dist.get(), want)


# ------------------------------------------------------------------------------------------- finishing partial sums
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("n_blocks", [1, 63, 64, 65, 130])
def test_distance_finalize_vs_fsum(n_blocks, n):
    partial, _ = sc.partial_case(n, n_blocks)
    want = sc.contract_finalize(partial)
    d_part = dev(partial)
    plain, headed = Out(n), Out(3 + n)
    head = dev(np.array([4.5], dtype=np.float32))
    L.call("coevo_fc_distance_finalize", L._p(d_part), n_blocks, n, plain.p, 0, None)
    L.call("coevo_fc_distance_finalize", L._p(d_part), n_blocks, n, headed.p, 3, L._p(head))
    assert sc.same_f32(plain.get(), want)
    got = headed.get()
    assert sc.same_f32(got[3:], want) and got[2] == 4.5 and (got[:2] == headed.sent).all()


@pytest.mark.parametrize("tick", [False, True])
def test_distance_finalize_multi_vs_fsum(tick):
    """three jobs of different n (one of them 0) and n_blocks in one launch, against the fsum reference"""
    shapes = [(5, 65, 3, True), (0, 7, 1, True), (1, 130, 0, False)]   # n, n_blocks, first, head
    jobs, keep, outs = (L.FinalizeJob * 3)(), [], []
    head = dev(np.array([0.375], dtype=np.float32))
    for j, (n, nb, first, with_head) in enumerate(shapes):
        partial = sc.partial_case(max(n, 1), nb)[0]
        d_part, out = dev(partial), Out(first + n)
        jobs[j] = L.FinalizeJob(L._p(d_part), out.p, L._p(head) if with_head else None, nb, n, first, 0)
        keep.append(d_part)
        outs.append((out, sc.contract_finalize(partial[:n]) if n else np.zeros(0, dtype=np.float32)))
    cnt = Out(1, torch.int32)
    cnt.t.fill_(41)
    if tick:
        L.call("coevo_fc_distance_finalize_multi_tick", C.cast(jobs, C.c_void_p), 3, cnt.p)
    else:
        L.call("coevo_fc_distance_finalize_multi", C.cast(jobs, C.c_void_p), 3)
    torch.cuda.synchronize()
    assert cnt.get()[0] == (42 if tick else 41)
    for (out, want), (n, nb, first, with_head) in zip(outs, shapes):
        got = out.get()
        if n == 0:
            assert (got == out.sent).all()   # not even the head
            continue
        assert sc.same_f32(got[first:], want)
        if with_head:
            assert got[first - 1] == 0.375 and (got[:first - 1] == out.sent).all()


# ------------------------------------------------------------------------------------------- score, fitness, rank: one by one
def reward_column(n, flavour, seed):
    """the last-game reward of each of n individuals, with what makes ranking hard: 0 - ties across the slice borders and
    between the ends; 1 - a NaN, +inf and -inf; 2 - a five-way tie and signed zeros"""
    r = np.random.Generator(np.random.PCG64(seed)).normal(size=n) * 10

    def put(idx, val, need=1):
        if n >= need:
            r[[i for i in idx if 0 <= i < n]] = val
    if flavour == 0:
        put([255, 256], 1.5, need=257)
        put([511, 512], -2.5, need=513)
        put([0, n - 1], 0.75)
    elif flavour == 1:
        put([n // 3], np.nan)
        put([0], np.inf, need=2)
        put([n - 1], -np.inf, need=3)
    else:
        put([0, 2, 3, n // 2, n - 1], 3.25)
        put([1], -0.0, need=3)
        put([n - 2], 0.0, need=4)
    return r


def rewards_array(cols, game_first, gpi, n, rows, seed):
    """[rows][3] fp64 noise with cols[slot][i] at the last game of individual i (quirk Q2): row game_first + i * gpi + gpi - 1"""
    a = np.random.Generator(np.random.PCG64(seed)).normal(size=(rows, 3)) * 10
    for slot, col in cols.items():
        a[game_first + np.arange(n) * gpi + gpi - 1, slot] = col
    return a


@pytest.mark.parametrize("name", list(sc.score_cases()))
def test_sharing_score_fitness_rank_vs_numpy(name):
    d, _ = sc.score_cases()[name]
    n, gpi, hof, game_first = len(d), 3, 5, 4
    want_s = sc.contract_score(d)
    score = Out(1)
    d_dist = dev(d)
    L.call("coevo_sharing_score", L._p(d_dist), n, score.p)
    got_s = score.get()
    print(name, "score", got_s, "contract", want_s, "numpy", sc.np_score(d))
    assert sc.same_f32(got_s, want_s)
    if name in sc.NAN_SCORE:
        assert np.isnan(got_s[0])
    # fitness for every slot: games_per_individual != hof; the buffer has rows enough for any mix-up of the two to stay inside it
    cols = {s: reward_column(n, s, 11 * n + s) for s in range(3)}
    rewards = rewards_array(cols, game_first, gpi, n, game_first + n * 8 + 8, seed=n)
    d_rew, d_div = dev(rewards), dev(np.array([want_s], dtype=np.float32))
    fits, orders = [Out(n) for _ in range(3)], [Out(n, torch.int32) for _ in range(3)]
    for s in range(3):
        L.call("coevo_ga_fitness", L._p(d_rew), game_first, n, gpi, hof, s, L._p(d_div), fits[s].p)
        L.call("coevo_rank_desc", fits[s].p, n, orders[s].p)
    for s in range(3):
        want_f = sc.np_fitness(rewards, game_first, n, gpi, hof, s, want_s)
        assert sc.same_f32(fits[s].get(), want_f), s
        assert np.array_equal(orders[s].get(), sc.np_order(want_f)), s
        if np.isnan(want_s):
            assert np.array_equal(orders[s].get(), np.arange(n)[::-1])


@pytest.mark.parametrize("n", sc.RANK_N)
def test_rank_desc_ties_nan_and_slices(n):
    vecs = sc.rank_vectors(n)
    outs, ins = {}, {name: dev(f) for name, f in vecs.items()}
    for name in vecs:
        outs[name] = Out(n, torch.int32)
        L.call("coevo_rank_desc", L._p(ins[name]), n, outs[name].p)
    for name, f in vecs.items():
        got = outs[name].get()
        assert sorted(got.tolist()) == list(range(n)), name
        assert np.array_equal(got, sc.np_order(f)), name


@pytest.mark.parametrize("n", sc.CENTERED_N)
def test_centered_ranks_ties_nan_and_blocks(n):
    vecs = sc.rank_vectors(n)
    outs, ins = {}, {name: dev(f) for name, f in vecs.items()}
    for name in vecs:
        outs[name] = Out(n)
        L.call("coevo_centered_ranks", L._p(ins[name]), n, outs[name].p)
    for name, f in vecs.items():
        assert np.array_equal(outs[name].get().view(np.uint32), rp.centered_ranks(f).view(np.uint32)), name


@pytest.mark.parametrize("n", [1, 127, 128, 129])
def test_gather_f32(n):
    g = np.random.Generator(np.random.PCG64(n))
    src = g.normal(size=300).astype(np.float32)
    src[5], src[6] = np.nan, -0.0
    d_src = dev(src)
    for idx in (np.arange(n)[::-1] * 2, np.arange(n) * 7 % 5 + 3, np.full(n, 299)):
        out, d_idx = Out(n), dev(idx.astype(np.int32))
        L.call("coevo_gather_f32", out.p, L._p(d_src), L._p(d_idx), n)
        assert sc.same_f32(out.get(), src[idx]) and np.array_equal(np.signbit(out.get()), np.signbit(src[idx]))


# ------------------------------------------------------------------------------------------- the fused launch
def adapt_reference(hist, ev, first, g, s64, smin, smax, cap, adaptive=1):
    """ga_adapt_kernel's contract: evaluate_current_weights' means of generation g - 1 into hist, then the reference's rule as
    numpy evaluates it (ga.adapt_mutation_power, as in test_adapt_sigma_kernel_vs_numpy_rule) -> hist, sig_hist column, sigma64"""
    hist, s, col = hist.copy(), [float(x) for x in s64], None
    if 0 < g <= cap:
        e = g - 1
        for k in range(3):
            tot = 0.0
            for i in range(10):
                tot += float(ev[first + i, k])
            hist[k, e] = tot / 10
        if adaptive:
            args = Bag(max_mutation_power=smax, min_mutation_power=smin, **dict(zip(SIG, s)))
            with np.errstate(invalid="ignore"):
                ga.adapt_mutation_power(args, e, {r: hist[k, :e + 1].tolist() for k, r in enumerate(ga.ROLES)})
            s = [getattr(args, a) for a in SIG]
        col = (e, s)
    return hist, col, s


class Adapt:
    """device state of the sigma rule around generation g, everything it may write pre-filled"""

    def __init__(self, g, cap=40, nan_at=None, seed=5, first=6):
        rng = np.random.default_rng(seed)
        self.g, self.cap, self.first, self.smin, self.smax = g, cap, first, 0.02, 0.1
        self.hist0 = np.full((3, cap), SENT[torch.float64])
        self.hist0[:, :max(min(g - 1, cap), 0)] = rng.normal(size=(3, max(min(g - 1, cap), 0)))
        self.hist0[0, :max(min(g - 1, cap), 0)] -= 0.3 * np.arange(max(min(g - 1, cap), 0))   # agent_0 gets worse: the increase branch
        if nan_at is not None:
            self.hist0[:, nan_at] = np.nan
        self.ev = rng.normal(size=(first + 10 + 3, 3))
        self.s64_0 = np.array([0.05, 0.08, 0.03])
        self.hist, self.sigh = dev(self.hist0), torch.full((3, cap), SENT[torch.float64], dtype=torch.float64, device=DEV)
        self.d_ev, self.s64 = dev(self.ev), dev(self.s64_0)
        self.s32 = dev(self.s64_0.astype(np.float32))
        self.s32p = Out(3)
        self.gen = dev(np.array([g], dtype=np.int32))

    def args(self):
        return L.GaAdaptArgs(L._p(self.d_ev), L._p(self.gen), L._p(self.hist), L._p(self.sigh), L._p(self.s64), L._p(self.s32),
                             self.s32p.p, self.smin, self.smax, self.first, self.cap, 1, 0)

    def check(self, through_select):
        hist, col, s = adapt_reference(self.hist0, self.ev, self.first, self.g, self.s64_0, self.smin, self.smax, self.cap)
        sigh = np.full((3, self.cap), SENT[torch.float64])
        if col:
            sigh[:, col[0]] = col[1]
        assert np.array_equal(self.hist.cpu().numpy(), hist, equal_nan=True)
        assert np.array_equal(self.sigh.cpu().numpy(), sigh)
        assert self.s64.cpu().tolist() == s
        assert self.s32.cpu().tolist() == [float(F32(x)) for x in s]
        if through_select:   # what the children of this generation were bred with
            assert self.s32p.get().tolist() == [float(F32(x)) for x in self.s64_0]
        else:
            assert self.s32p.untouched()
        return s


class Roles:
    """three roles' inputs and sentinel outputs for one fused launch, and the numpy reference of each"""

    def __init__(self, pop, kinds, gpi, hof, seed):
        self.pop, self.gpi, self.hof = pop, gpi, hof
        self.dist = [sc.dist_kind(k if (k != "overflow" or pop >= 3) else "random", pop) for k in kinds]
        self.cols = [reward_column(pop, r, seed + r) for r in range(3)]
        self.outs = [(Out(1), Out(pop), Out(pop, torch.int32), Out(1)) for _ in range(3)]
        self.keep = []

    def plain(self):
        """roles' own dist / rewards pointers: role r's games begin at 2 + r * pop * gpi, its slot is (r + 1) % 3"""
        pop, gpi = self.pop, self.gpi
        self.first = [2 + r * pop * gpi for r in range(3)]
        self.slot = [(r + 1) % 3 for r in range(3)]
        self.rewards = np.random.default_rng(pop).normal(size=(2 + 3 * pop * gpi + 4, 3)) * 10
        for r in range(3):
            self.rewards[self.first[r] + np.arange(pop) * gpi + gpi - 1, self.slot[r]] = self.cols[r]
        d_rew = dev(self.rewards)
        sel = (L.GaSelectRole * 3)()
        for r in range(3):
            d = dev(self.dist[r])
            self.keep += [d, d_rew]
            div, fit, order, best = self.outs[r]
            sel[r] = L.GaSelectRole(L._p(d), L._p(d_rew), div.p, fit.p, order.p, best.p, self.first[r], self.slot[r])
        return sel

    def gathered(self, world, n_local):
        """[world][3][n_local][4] fp64 records {reward triple of the last game, distance}; the roles carry no input pointers"""
        assert world * n_local == self.pop
        self.first, self.slot, self.gpi = [0, 0, 0], [(r + 1) % 3 for r in range(3)], 1
        buf = np.random.default_rng(self.pop).normal(size=(world, 3, n_local, 4)) * 10
        self.rewards = []
        for r in range(3):
            buf[:, r, :, self.slot[r]] = self.cols[r].reshape(world, n_local)
            buf[:, r, :, 3] = self.dist[r].astype(np.float64).reshape(world, n_local)
        d_buf = dev(buf)
        self.keep.append(d_buf)
        sel = (L.GaSelectRole * 3)()
        for r in range(3):
            div, fit, order, best = self.outs[r]
            sel[r] = L.GaSelectRole(None, None, div.p, fit.p, order.p, best.p, 0, self.slot[r])
        return sel, d_buf

    def check(self, n_roles=3):
        for r in range(n_roles):
            d, (div, fit, order, best) = self.dist[r], self.outs[r]
            want_s = sc.contract_score(d)
            rew = np.zeros((self.pop, 3))
            rew[:, self.slot[r]] = self.cols[r]
            want_f = sc.np_fitness(rew, 0, self.pop, 1, self.hof, self.slot[r], want_s)
            want_o = sc.np_order(want_f)
            got_o = order.get()
            assert sc.same_f32(div.get(), want_s), r
            assert sc.same_f32(fit.get(), want_f), r
            assert sorted(got_o.tolist()) == list(range(self.pop)), r
            assert np.array_equal(got_o, want_o), r
            assert sc.same_f32(best.get(), d[want_o[0]]), r
            if np.isnan(want_s):   # every fitness NaN: the order is n-1 ... 0 and the best is the last individual
                assert np.isnan(fit.get()).all() and np.array_equal(got_o, np.arange(self.pop)[::-1])


@pytest.mark.parametrize("kinds", [KINDS[0:3], KINDS[3:6], KINDS[6:9]])
@pytest.mark.parametrize("pop", FUSED_POPS)
def test_ga_select_vs_numpy(pop, kinds):
    """a different case in each role of one launch (nothing leaks through the shared LDS), at one slice, the slice border and
    the LDS cap - alone and with the sigma rule's block beside it"""
    gpi, hof = 3, 5
    for with_adapt in (False, True):
        roles = Roles(pop, kinds, gpi, hof, seed=pop)
        sel = roles.plain()
        if with_adapt:
            ad = Adapt(g=14)
            L.call("coevo_ga_select_adapt", sel, 3, pop, gpi, hof, None, 0, C.byref(ad.args()))
        else:
            L.call("coevo_ga_select", sel, 3, pop, gpi, hof)
        torch.cuda.synchronize()
        roles.check()
        if with_adapt:
            s = ad.check(through_select=True)
            assert s[0] == min(0.08 * 1.2, 0.1)   # agent_0 worse: the increase from agent_1's sigma (quirk Q5) was taken


@pytest.mark.parametrize("kinds", [KINDS[0:3], KINDS[3:6], KINDS[6:9]])
@pytest.mark.parametrize("world,n_local", [(3, 86), (1, 257), (257, 1)])
def test_ga_select_gathered_vs_numpy(world, n_local, kinds):
    pop, hof = world * n_local, 5
    for with_adapt in (False, True):
        roles = Roles(pop, kinds, 1, hof, seed=pop + 1)
        sel, d_buf = roles.gathered(world, n_local)
        if with_adapt:
            ad = Adapt(g=14)
            L.call("coevo_ga_select_adapt", sel, 3, pop, 1, hof, L._p(d_buf), n_local, C.byref(ad.args()))
        else:
            L.call("coevo_ga_select_gathered", sel, 3, pop, hof, L._p(d_buf), n_local)
        torch.cuda.synchronize()
        roles.check()
        if with_adapt:
            ad.check(through_select=True)


def test_ga_select_one_and_two_roles_leave_the_rest_alone():
    roles = Roles(257, KINDS[0:3], 3, 5, seed=9)
    sel = roles.plain()
    L.call("coevo_ga_select", sel, 2, 257, 3, 5)
    torch.cuda.synchronize()
    assert all(o.untouched() for o in roles.outs[2])
    roles.check(n_roles=2)


# ------------------------------------------------------------------------------------------- the sigma rule's corners
@pytest.mark.parametrize("g,nan_at", [(0, None), (41, None), (45, None), (40, None), (14, 9), (25, 12)])
def test_adapt_sigma_corners(g, nan_at):
    """*gen_dev = 0 and *gen_dev - 1 >= cap: nothing recorded, sigma32 = f32(sigma64); the last generation that fits (40);
    a NaN evaluation mean inside the newer (9 of 4..13) or the older (12 of 5..14) window: the comparison is false, sigma decays"""
    ad = Adapt(g=g, nan_at=nan_at)
    a = ad.args()
    L.call("coevo_ga_adapt_sigma", a.rewards, a.eval_first_game, a.gen_dev, a.hist, a.sig_hist, a.cap, a.sigma64, a.sigma32,
           a.sig_min, a.sig_max, 1)
    torch.cuda.synchronize()
    s = ad.check(through_select=False)
    if g in (0, 41, 45):
        assert s == ad.s64_0.tolist()
    if nan_at is not None:
        assert s == [max(x * 0.95, 0.02) for x in ad.s64_0.tolist()]


# ------------------------------------------------------------------------------------------- refusals
def test_refused_arguments_write_nothing():
    """only what the entry points check on the host; each raises and leaves every output as it was"""
    n = 8
    d = dev(sc.random_dist(n, 1)[0])
    f32o, i32o, one = Out(4097), Out(4097, torch.int32), Out(1)
    rewards = dev(np.zeros((4097 * 3 + 8, 3)))
    idx = dev(np.zeros(n, dtype=np.int32))
    part = dev(np.ones((n, 4)))
    head = dev(np.array([1.0], dtype=np.float32))
    ref, nets, _ = sc.dist_nets(8, 1)
    slab = to_slab(nets, 8)
    refused("coevo_sharing_score", L._p(d), 0, one.p)
    refused("coevo_rank_desc", L._p(d), 0, i32o.p)
    refused("coevo_rank_desc", f32o.p, 4097, i32o.p)
    refused("coevo_centered_ranks", L._p(d), 0, f32o.p)
    refused("coevo_centered_ranks", f32o.p, n, f32o.p)                      # in place
    refused("coevo_gather_f32", f32o.p, L._p(d), L._p(idx), 0)
    refused("coevo_fc_distance", L._p(slab), L._p(slab), 0, 8, f32o.p)
    refused("coevo_fc_distance", L._p(slab), L._p(slab), 1, 9, f32o.p)      # no such observation width
    refused("coevo_fc_diversity", L._p(slab), L._p(slab), 0, 8, f32o.p, one.p)
    refused("coevo_fc_distance_finalize", L._p(part), 4, 0, f32o.p, 0, None)
    refused("coevo_fc_distance_finalize", L._p(part), 0, n, f32o.p, 0, None)
    refused("coevo_fc_distance_finalize", L._p(part), 4, n, f32o.p, 0, L._p(head))   # a head needs first >= 1
    refused("coevo_ga_fitness", L._p(rewards), 0, 0, 3, 5, 0, L._p(d), f32o.p)
    refused("coevo_ga_fitness", L._p(rewards), 0, n, 3, 5, 3, L._p(d), f32o.p)      # slot 3
    refused("coevo_ga_fitness", L._p(rewards), 0, n, 3, 0, 0, L._p(d), f32o.p)
    jobs = (L.FinalizeJob * 1)(L.FinalizeJob(L._p(part), f32o.p, L._p(head), 4, n, 0, 0))
    cnt = Out(1, torch.int32)
    refused("coevo_fc_distance_finalize_multi", C.cast(jobs, C.c_void_p), 1)        # head with first = 0
    refused("coevo_fc_distance_finalize_multi", C.cast(jobs, C.c_void_p), 0)        # n_jobs = 0
    refused("coevo_fc_distance_finalize_multi_tick", C.cast(jobs, C.c_void_p), 0, cnt.p)

    def role(**kw):
        a = dict(dist=f32o.p, rewards=L._p(rewards), diversity=one.p, fitness=f32o.p, order=i32o.p, best_dist=one.p,
                 game_first=0, slot=0)
        a.update(kw)
        return (L.GaSelectRole * 1)(L.GaSelectRole(*[a[k] for k, _ in L.GaSelectRole._fields_]))
    gathered = dev(np.zeros((2, 1, 4, 4)))
    refused("coevo_ga_select", role(), 1, 0, 3, 5)
    refused("coevo_ga_select", role(), 1, 4097, 3, 5)
    refused("coevo_ga_select", role(), 0, n, 3, 5)
    refused("coevo_ga_select", role(slot=3), 1, n, 3, 5)
    refused("coevo_ga_select", role(diversity=None), 1, n, 3, 5)
    refused("coevo_ga_select", role(order=None), 1, n, 3, 5)
    refused("coevo_ga_select", role(dist=None), 1, n, 3, 5)                       # no gathered buffer: dist is needed
    refused("coevo_ga_select_gathered", role(), 1, 7, 5, L._p(gathered), 4)       # pop % n_local
    refused("coevo_ga_select_gathered", role(), 1, n, 5, None, 4)
    refused("coevo_ga_select_adapt", role(), 1, n, 3, 5, None, 0, None)           # no sigma-rule arguments
    torch.cuda.synchronize()
    assert f32o.untouched() and i32o.untouched() and one.untouched() and cnt.untouched()
