"""The fp32 breeding, promotion and ES-update kernels (csrc/offspring.hip) through the C ABI at their edges, against the plain
numpy / fsum references of tests/breed_cases.py (proven on the CPU by tests/test_breed_edges_cpu.py) - never against a sibling
launch, except where one index path is held against the other on purpose.  Finite and infinite results as bits, NaN by
position.  Every buffer a launch writes lies between guard rows / words of a sentinel, and what a launch must not touch is
asserted untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

from coevonet_amd import lib as L
from oracle import ref_port as rp
from tests import breed_cases as bc, tile_major_cases as tm

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
SENT = -7.25
PAD = 4
ERR_ARG = -1


# ------------------------------------------------------------------------------------------- plumbing
def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


class Slab:
    """n slab rows of width D between one guard row on each side, everything the sentinel at first"""

    def __init__(self, n, D):
        self.n, self.D, self.stride, self.P = n, D, L.fc_slab_stride(D), L.fc_param_count(D)
        self.buf = torch.full((n + 2, self.stride), SENT, dtype=torch.float32, device=DEV)
        self.t = self.buf[1:n + 1]
        self.p = self.t.data_ptr()
        self.keep = []

    def row(self, i):
        return self.p + 4 * i * self.stride

    def load(self, flat, first=0, padding=bc.padding_of):
        """pack canonical nets into rows first..., then plant each net's padding words directly"""
        d = dev(np.asarray(flat, dtype=np.float32))
        self.keep.append(d)
        L.call("coevo_fc_pack", L._p(d), self.row(first), len(flat), self.D)
        for k in range(len(flat)):
            self.t[first + k, self.P:] = float(padding(k))
        return self

    def put(self, rows, first=0):
        self.t[first:first + len(rows)] = dev(np.asarray(rows, dtype=np.float32))
        return self

    def rows(self):
        """-> the n raw rows, after asserting the guard rows"""
        a = self.buf.cpu().numpy()
        assert (a[0] == SENT).all() and (a[-1] == SENT).all(), "a guard row was written"
        return a[1:-1]

    def flat(self, first=0, n=None):
        n = self.n - first if n is None else n
        back = torch.zeros(n, self.P, dtype=torch.float32, device=DEV)
        L.call("coevo_fc_unpack", self.row(first), L._p(back), n, self.D)
        return back.cpu().numpy()


class Words:
    """n words between PAD guard words, all of it `fill`"""

    def __init__(self, n, dtype=torch.float32, fill=SENT):
        self.n, self.fill = n, fill
        self.buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=DEV)
        self.t = self.buf[PAD:PAD + n]
        self.p = self.t.data_ptr()

    def get(self):
        a = self.buf.cpu().numpy()
        g = np.concatenate([a[:PAD], a[PAD + self.n:]])
        assert (np.isnan(g).all() if np.isnan(self.fill) else (g == self.fill).all()), "a guard word was written"
        return a[PAD:PAD + self.n]

    def untouched(self):
        a = self.get()
        return bool(np.isnan(a).all() if np.isnan(self.fill) else (a == self.fill).all())


def is_sent(rows):
    return bool((np.asarray(rows) == SENT).all())


def rc(name, *args):
    """the entry point's return code (no exception)"""
    return getattr(L.load(), name)(*args, L._stream())


def parent_slab(D, nets=None):
    nets = bc.planted_parents(D, bc.N_PARENTS) if nets is None else nets
    return Slab(len(nets), D).load(nets), nets


def ln_poison(flat, D):
    """LayerNorm entries of a canonical net set to 1e30 and NaN"""
    out = np.array(flat, dtype=np.float32, copy=True)
    for o, n in rp.ln_segments(D):
        out[..., o:o + n:2] = 1e30
        out[..., o + 1:o + n:2] = np.nan
    return out


# ------------------------------------------------------------------------------------------- 0. the layout the references use
@pytest.mark.parametrize("D", [8, 10])
def test_slab_map_is_the_pack_kernels(D):
    assert (L.fc_param_count(D), L.fc_slab_stride(D)) == (bc.params(D), bc.stride(D))
    assert int(L.load().coevo_fc_perturb_blocks(D)) == bc.n_blocks(D)
    s = Slab(1, D).load(np.arange(bc.params(D), dtype=np.float32)[None], padding=lambda k: -1.0)
    assert np.array_equal(s.rows()[0].astype(np.int64), bc.slab_to_flat(D))


# ------------------------------------------------------------------------------------------- 1. noise in bulk
# What the two windows hold, computed on the CPU from the raw Philox words (oracle_philox4x32) of their 2^21 (a, b) pairs:
#   (seed 3, stream (17, 5), q_first 0):                    a >> 9 from 13 to 8388603 (of 0 ... 8388607); b >> 8 hits 1 of the
#                                                           8 octant edges k * 2^21 of u2
#   (seed 2^40 + 3, stream (2^31, 3), q_first 2^32 - 2^19): a >> 9 from 4 to 8388606; none of the 8 octant edges hit
# (an octant edge is one b >> 8 value in 2^24: 2^21 draws hit each with probability 1/8).  The transform's edges proper are
# the CPU test's job (test_box_muller_edges_and_sweep_vs_float64); this test pins the kernel to the oracle in bulk.
NOISE_WINDOWS = ((3, 17, 5, 0), ((1 << 40) + 3, 2 ** 31, 3, 2 ** 32 - 2 ** 19))


@pytest.mark.parametrize("seed,lo,hi,q_first", NOISE_WINDOWS)
def test_noise_bulk_equals_oracle(seed, lo, hi, q_first):
    n = 1 << 20
    z = Words(4 * n)
    L.call("coevo_philox_normals", seed, lo, hi, q_first, n, z.p)
    got, want = z.get(), rp.philox_normals(seed, lo, hi, q_first, n).reshape(-1)
    assert np.isfinite(want).all() and bc.same_bits(got, want), bc.first_diff(got, want)


# ------------------------------------------------------------------------------------------- 2. perturb, every word
def launch_perturb(c, parents, d_pidx, child, child_first, sigma, gen_dev):
    n = len(c["pidx"])
    head = (parents.p, L._p(d_pidx), child.p, child_first, n, c["D"], L._p(sigma), bc.SEED, c["slo_first"] & bc.M32, c["shi"])
    if c["entry"] == "flags":
        L.call("coevo_fc_perturb_flags", *head, c["flags"])
    elif c["entry"] == "plain":
        L.call("coevo_fc_perturb", *head, c["flags"])
    else:
        L.call("coevo_fc_perturb_gen", *head, c["flags"], L._p(gen_dev))


def check_children(c, nets, rows, flat, what):
    """flat / rows: the children only, in launch order"""
    D, P = c["D"], bc.params(c["D"])
    want = bc.perturb_want(c, nets)
    ln = bc.ln_mask(D)
    for k, p in enumerate(c["pidx"]):
        assert bc.same_f32(flat[k], want[k]), (what, k, bc.first_diff(flat[k], want[k]))
        assert bc.same_bits(rows[k][P:], np.full(bc.stride(D) - P, bc.padding_of(p))), (what, k, "padding")
        if c["flags"] & 1:
            assert bc.same_bits(flat[k][ln], nets[p][ln]), (what, k, "LayerNorm bits")
        elif 1e-3 < c["sigma"] < 1e30:
            moved = flat[k][ln] != nets[p][ln]
            assert moved[np.isfinite(nets[p][ln]) & (np.abs(nets[p][ln]) < 1e30)].mean() > 0.9, (what, k, "LayerNorm perturbed")


@pytest.mark.parametrize("name", list(bc.perturb_cases()))
def test_perturb_every_word(name):
    c = bc.perturb_cases()[name]
    D, n = c["D"], len(c["pidx"])
    parents, nets = parent_slab(D)
    child = Slab(1 + n + 1, D)                       # a net before child_first and one after the last child
    d_pidx = dev(np.array(c["pidx"], dtype=np.int32))
    sigma = dev(np.array([c["sigma"]], dtype=np.float32))
    gen_dev = dev(np.array([c["gen"] or 0], dtype=np.int32))
    launch_perturb(c, parents, d_pidx, child, 1, sigma, gen_dev)
    rows, flat = child.rows(), child.flat(1, n)
    assert is_sent(rows[0]) and is_sent(rows[1 + n]), "a net outside [child_first, child_first + n) was written"
    check_children(c, nets, rows[1:1 + n], flat, name)
    pr = parents.rows()
    for k in range(bc.N_PARENTS):
        assert bc.same_bits(pr[k], bc.to_slab_rows(nets[k], D, bc.padding_of(k))), "a parent changed"


@pytest.mark.parametrize("D,flags", [(8, 1), (10, 2)])
def test_perturb_in_place_after_the_parents(D, flags):
    """child_slab == parent_slab, the children placed after the parents (the ES form)"""
    c = dict(bc.perturb_cases()["plain_es"], D=D, flags=flags, entry="flags", pidx=(2, 0, 2, 1))
    nets = bc.planted_parents(D, bc.N_PARENTS)
    s = Slab(bc.N_PARENTS + 4 + 1, D).load(nets)
    d_pidx, sigma = dev(np.array(c["pidx"], dtype=np.int32)), dev(np.array([c["sigma"]], dtype=np.float32))
    launch_perturb(c, s, d_pidx, s, bc.N_PARENTS, sigma, None)
    rows = s.rows()
    for k in range(bc.N_PARENTS):
        assert bc.same_bits(rows[k], bc.to_slab_rows(nets[k], D, bc.padding_of(k)))
    assert is_sent(rows[-1])
    check_children(c, nets, rows[bc.N_PARENTS:bc.N_PARENTS + 4], s.flat(bc.N_PARENTS, 4), "in place")


def test_perturb_no_children_writes_nothing():
    D = 8
    parents, _ = parent_slab(D)
    child, part = Slab(2, D), Words(2 * bc.n_blocks(D), torch.float64)
    d_pidx, sigma = dev(np.zeros(2, dtype=np.int32)), dev(np.array([0.05], dtype=np.float32))
    args = (parents.p, L._p(d_pidx), child.p, 0, 0, D, L._p(sigma), bc.SEED, 0, 0)
    assert rc("coevo_fc_perturb", *args, 0) == 0 and rc("coevo_fc_perturb_flags", *args, 3) == 0
    assert rc("coevo_fc_perturb_dist", *args, 0, None, parents.p, part.p) == 0
    torch.cuda.synchronize()
    assert is_sent(child.rows()) and part.untouched()


# ------------------------------------------------------------------------------------------- 3. fused distance
def hot_entry(D):
    """a canonical fc2.weight entry and the distance block that holds it"""
    e = bc.segments(D)[4][0] + 70001
    return e, int(np.flatnonzero(bc.slab_to_flat(D) == e)[0]) // bc.BLOCK


def dist_parents(D):
    """planted net 0 (finite), a plain net with +inf on one fc2 weight, planted net 2 (inf and NaN plants)"""
    pl = bc.planted_parents(D, bc.N_PARENTS)
    hot = bc.plain_nets(D, 1, 5)[0].copy()
    hot[hot_entry(D)[0]] = np.inf
    return np.stack([pl[0], hot, pl[2]])


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("ref_kind", ["parent", "unrelated", "inf"])
@pytest.mark.parametrize("D", [8, 10])
def test_fused_distance_vs_fsum(D, ref_kind, flags):
    nets = dist_parents(D)
    parents, _ = parent_slab(D, nets)
    c = dict(bc.perturb_cases()["plain_ga"], D=D, flags=flags, pidx=(0, 1, 0, 2, 1))
    n, nb = len(c["pidx"]), bc.n_blocks(D)
    e, blk = hot_entry(D)
    if ref_kind == "parent":
        ref_flat, ref_ptr = nets[0], parents.row(0)
    else:
        ref_flat = bc.plain_nets(D, 1, 6)[0].copy()
        if ref_kind == "inf":
            ref_flat[e] = np.inf
        # 1e30 and NaN in the reference's LayerNorm and padding words: excluded, even with flag 0 where LayerNorm is perturbed
        ref_slab = Slab(1, D).load(ln_poison(ref_flat, D)[None], padding=lambda k: np.nan)
        ref_slab.t[0, bc.params(D)::2] = 1e30
        ref_ptr = ref_slab.p
    child, part, dist = Slab(n, D), Words(n * nb, torch.float64), Words(n)
    d_pidx, sigma = dev(np.array(c["pidx"], dtype=np.int32)), dev(np.array([c["sigma"]], dtype=np.float32))
    L.call("coevo_fc_perturb_dist", parents.p, L._p(d_pidx), child.p, 0, n, D, L._p(sigma), bc.SEED, c["slo_first"], c["shi"],
           flags, None, ref_ptr, part.p)
    L.call("coevo_fc_distance_finalize", part.p, nb, n, dist.p, 0, None)
    rows, flat = child.rows(), child.flat()
    check_children(c, nets, rows, flat, ref_kind)
    got_p, got_d = part.get().reshape(n, nb), dist.get()
    want = bc.perturb_want(c, nets)
    for k, p in enumerate(c["pidx"]):
        want_p = bc.dist_partials(want[k], ref_flat, D)
        assert bc.same_partials(got_p[k], want_p), (k, np.flatnonzero(~np.isclose(got_p[k], want_p, rtol=1e-12, atol=0, equal_nan=True)))
        assert bc.within_one_ulp(got_d[k], bc.final_distance(want_p)), (k, got_d[k], bc.final_distance(want_p))
        if p == 0:     # the finite parent
            assert np.isfinite(want_p).all() == (ref_kind != "inf")
            if ref_kind == "parent":    # the distance is the norm of the noise over the Linear entries
                nz = bc.noise(c["sigma"], bc.SEED, c["slo_first"] + k, c["shi"], flags, bc.params(D))[~bc.ln_mask(D)]
                big = np.abs(nets[0][~bc.ln_mask(D)]) > 1e30             # (+-FLT_MAX + noise = +-FLT_MAX: difference 0)
                assert abs(float(got_d[k]) / np.linalg.norm(nz[~big].astype(np.float64)) - 1) < 1e-3
        if p == 1 and ref_kind == "inf":   # inf - inf: a NaN partial in exactly that block
            assert np.flatnonzero(np.isnan(got_p[k])).tolist() == [blk] and np.isfinite(np.delete(got_p[k], blk)).all()


# ------------------------------------------------------------------------------------------- 4. the multi-job launch
@pytest.mark.parametrize("n_jobs", [1, 4])
def test_multi_job_launch_vs_numpy(n_jobs):
    Ds, ns = ((8, 10, 10, 8), (0, 1, 5, 2)) if n_jobs == 4 else ((10,), (5,))
    flags, gen = (0, None) if n_jobs == 4 else (3, 5)
    sig = np.array([0.05, 0.02, 0.11, 0.3], dtype=np.float32)
    d_sig = dev(sig)
    gen_dev = dev(np.array([gen or 0], dtype=np.int32))
    jobs, keep, checks = (L.PerturbJob * n_jobs)(), [], []
    for j, (D, n) in enumerate(zip(Ds, ns)):
        parents, nets = parent_slab(D)
        pidx = tuple((2 * k + j) % bc.N_PARENTS for k in range(n))
        d_pidx = dev(np.array(pidx + (0,), dtype=np.int32))
        with_dist = not (n_jobs == 4 and j == 3)                     # one job without distance beside jobs with it
        ref_flat = bc.plain_nets(D, 1, 20 + j)[0]
        ref_slab = Slab(1, D).load(ln_poison(ref_flat, D)[None], padding=lambda k: np.nan)
        child, part = Slab(1 + max(n, 1) + 1, D), Words(max(n, 1) * bc.n_blocks(D), torch.float64)
        slo, shi = [WRAP, 7, WRAP - 1, 3][j], [5, 2 ** 32 - 1, 9, 0][j]   # streams wrap inside a job
        jobs[j] = L.PerturbJob(parents.p, L._p(d_pidx), child.p, d_sig.data_ptr() + 4 * j, ref_slab.p if with_dist else None,
                               part.p if with_dist else None, 1, n, D, slo & bc.M32, shi, 0)
        keep += [parents, d_pidx, ref_slab]
        checks.append((dict(D=D, sigma=sig[j], flags=flags, slo_first=slo, shi=shi, gen=gen, pidx=pidx), nets, child, part,
                       ref_flat, with_dist))
    L.call("coevo_fc_perturb_dist_multi", C.cast(jobs, C.c_void_p), n_jobs, bc.SEED, flags, L._p(gen_dev) if gen is not None else None)
    torch.cuda.synchronize()
    for c, nets, child, part, ref_flat, with_dist in checks:
        n, nb = len(c["pidx"]), bc.n_blocks(c["D"])
        rows = child.rows()
        assert is_sent(rows[0]) and is_sent(rows[1 + n:])
        if n == 0:
            assert part.untouched()
            continue
        check_children(c, nets, rows[1:1 + n], child.flat(1, n), "multi")
        if not with_dist:
            assert part.untouched()
            continue
        got_p, want = part.get().reshape(n, nb), bc.perturb_want(c, nets)
        for k in range(n):
            assert bc.same_partials(got_p[k], bc.dist_partials(want[k], ref_flat, c["D"])), k


WRAP = bc.WRAP_FIRST


# ------------------------------------------------------------------------------------------- 5. elite rebuild
REBUILD_ORDERS = {
    1: ((0,), (5,), (1,)),
    3: ((0, 4, 2), (3, 1, 2), (7, 0, 7)),          # id 0 first; the cyclic parent map (2, 0, 1), id 0 absent; repeats, ids > E
    8: ((9, 0, 3, 3, 17, 1, 8, 2), (0, 1, 2, 3, 4, 5, 6, 7), (16, 15, 14, 13, 12, 11, 10, 9)),
}
REBUILD_SIGMA = np.array([0.05, 0.031, 0.07], dtype=np.float32)
ROLE_D = (8, 10, 10)


def materialised(old, D, ids, sigma_ptr, seed, shi):
    """the child coevo_fc_perturb builds for each id >= 1 from parent (id - 1) % E with stream id - 1: raw rows"""
    E = old.n
    out = Slab(len(ids), D)
    for k, ident in enumerate(ids):
        if ident == 0:
            continue
        d_pidx = dev(np.array([(ident - 1) % E], dtype=np.int32))
        out.keep.append(d_pidx)
        L.call("coevo_fc_perturb", old.p, L._p(d_pidx), out.p, k, 1, D, sigma_ptr, seed, ident - 1, shi, 0)
    return out.rows()


@pytest.mark.parametrize("gen", [None, 1, 3])
@pytest.mark.parametrize("E", [1, 3, 8])
def test_rebuild_elites_vs_numpy_and_vs_the_materialised_child(E, gen):
    seed, shi_prev, D = 77, 2 ** 32 - 2, (8, 10)[E % 2 ^ (gen is None)]
    nets = bc.planted_parents(D, E)
    d_sig = dev(REBUILD_SIGMA)
    gen_dev = dev(np.array([gen or 0], dtype=np.int32))
    shi_eff = (shi_prev + (4 * (gen - 1) if gen is not None else 0)) & bc.M32
    for ids in REBUILD_ORDERS[E]:
        old, new = Slab(E, D).load(nets), Slab(E, D)
        order = dev(np.array(ids, dtype=np.int32))
        L.call("coevo_fc_rebuild_elites", old.p, L._p(order), new.p, E, D, d_sig.data_ptr() + 4, seed, shi_prev,
               L._p(gen_dev) if gen is not None else None)
        rows, flat = new.rows(), new.flat()
        child_rows = materialised(old, D, ids, d_sig.data_ptr() + 4, seed, shi_eff)
        old_rows = old.rows()
        for k, ident in enumerate(ids):
            want = bc.rebuilt_elite(nets, D, ident, REBUILD_SIGMA[1], seed, shi_prev, gen)
            assert bc.same_f32(flat[k], want), (ids, k, bc.first_diff(flat[k], want))
            src = 0 if ident == 0 else (ident - 1) % E
            assert bc.same_bits(rows[k][bc.params(D):], old_rows[src][bc.params(D):])
            # the two index paths: the generic one here, the fc2 fast path in the breeding kernel - bit for bit, padding too
            assert bc.same_bits(rows[k], old_rows[0] if ident == 0 else child_rows[k]), (ids, k)
        for k in range(E):
            assert bc.same_bits(old_rows[k], bc.to_slab_rows(nets[k], D, bc.padding_of(k)))


@pytest.mark.parametrize("gen", [None, 3])
@pytest.mark.parametrize("E,hof,n_roles", [(1, 1, 1), (3, 2, 3), (8, 16, 2), (3, 16, 1)])
def test_promote_rebuild_in_place_vs_numpy(E, hof, n_roles, gen):
    """coevo_ga_promote_rebuild: the new elites rebuilt in place from the old ones (every new elite of the cyclic order reads an
    old elite that another level overwrites), the Hall of Fame pushed and pop[0] written in the same launch; a role with
    elites_from_pop promoted as usual beside the rebuilt ones"""
    seed, shi_prev = 77, 2 ** 32 - 3
    d_sig = dev(REBUILD_SIGMA)
    gen_dev = dev(np.array([gen or 0], dtype=np.int32))
    roles, checks = (L.GaPromoteRole * n_roles)(), []
    g = torch.Generator(device=DEV).manual_seed(E * 100 + hof)
    for r in range(n_roles):
        D = ROLE_D[r]
        ids = REBUILD_ORDERS[E][(r + 1) % 3]       # role 0 of E = 3 takes the cycle (3, 1, 2)
        nets = bc.planted_parents(D, E)
        from_pop = n_roles == 3 and r == 2
        elite = Slab(E, D).load(nets)
        pop, hofs = Slab(max(ids) + 1 if from_pop else 2, D), Slab(hof, D)
        pop.t.copy_(torch.randn(pop.t.shape, generator=g, device=DEV))
        hofs.t.copy_(torch.randn(hofs.t.shape, generator=g, device=DEV))
        order = dev(np.array(ids, dtype=np.int32))
        roles[r] = L.GaPromoteRole(pop.p, hofs.p, elite.p, L._p(order), D, int(from_pop), 1, 0)
        checks.append((D, ids, nets, from_pop, pop, hofs, elite, pop.rows().copy(), hofs.rows().copy(), elite.rows().copy(), order))
    L.call("coevo_ga_promote_rebuild", roles, n_roles, E, hof, L._p(d_sig), seed, shi_prev, L._p(gen_dev) if gen is not None else None)
    torch.cuda.synchronize()
    for r, (D, ids, nets, from_pop, pop, hofs, elite, pop0, hof0, elite0, _) in enumerate(checks):
        got_e, got_h, got_p = elite.rows(), hofs.rows(), pop.rows()
        if from_pop:
            want_p, want_h, want_e = bc.promote(list(pop0), list(hof0), list(elite0), ids, E, True, True)
            for k in range(E):
                assert bc.same_bits(got_e[k], want_e[k]), (r, k)
        else:
            flat = elite.flat()
            for k, ident in enumerate(ids):
                want = bc.rebuilt_elite(nets, D, ident, REBUILD_SIGMA[r], seed, shi_prev + r, gen)
                assert bc.same_f32(flat[k], want), (r, ids, k, bc.first_diff(flat[k], want))
                src = 0 if ident == 0 else (ident - 1) % E
                assert bc.same_bits(got_e[k][bc.params(D):], elite0[src][bc.params(D):]), (r, k, "padding")
            want_p, want_h, _ = bc.promote(list(pop0), list(hof0), list(got_e), None, E, False, True)
        for k in range(hof):
            assert bc.same_bits(got_h[k], want_h[k]), (r, "hof", k)
        for k in range(len(pop0)):
            assert bc.same_bits(got_p[k], want_p[k]), (r, "pop", k)


# ------------------------------------------------------------------------------------------- 6. promotion
def promote_roles_of(E, hof, n_roles, variant, raw_w2=False):
    """n_roles roles of mixed width with random nets in pop / hof / elite (raw_w2: tm.raw_words in the fc2.weight block of
    every net - NaN payloads, infinities, -0.0, subnormals) -> (roles, per role: ids, from_pop, to_pop0, the three slabs, their
    rows before the launch, the order tensor)"""
    n_pop = 10
    g = torch.Generator(device=DEV).manual_seed(1000 * E + 10 * hof + n_roles)
    rng = np.random.default_rng(E + hof)
    raw = np.random.Generator(np.random.PCG64([E, hof, n_roles, variant]))
    roles, checks = (L.GaPromoteRole * n_roles)(), []
    for r in range(n_roles):
        D = ROLE_D[r]
        kind = (r + variant) % 3
        pop, hofs, elite = Slab(n_pop, D), Slab(hof, D), Slab(E, D)
        for s in (pop, hofs, elite):
            s.t.copy_(torch.randn(s.t.shape, generator=g, device=DEV))
            if raw_w2:
                o = tm.w2_offset(D)
                s.t[:, o:o + L.W2_FLOATS] = dev(tm.raw_words(raw, s.n * L.W2_FLOATS).reshape(s.n, -1))
        pop.t[0, 5], pop.t[n_pop - 1, 7], elite.t[0, 9] = float("nan"), float("inf"), -0.0
        if kind == 0:      # the best already sits in pop[0] and is written back onto itself; the rest distinct
            ids, from_pop, to_pop0 = [0] + list(1 + rng.permutation(n_pop - 1)[:E - 1]), 1, 1
        elif kind == 1:    # pop's last net is the best, an id repeats, pop[0] is left alone
            ids, from_pop, to_pop0 = [n_pop - 1] + [3] * (E - 1), 1, 0
            if E > 2:
                ids[2] = n_pop - 1
        else:              # the elites are in place already: read, not written
            ids, from_pop, to_pop0 = None, 0, 1
        order = dev(np.array(ids, dtype=np.int32)) if ids is not None else None
        roles[r] = L.GaPromoteRole(pop.p, hofs.p, elite.p, L._p(order), D, from_pop, to_pop0, 0)
        checks.append((ids, from_pop, to_pop0, pop, hofs, elite, pop.rows().copy(), hofs.rows().copy(), elite.rows().copy(), order))
    return roles, checks


def assert_regions(r, slabs, want):
    for name, got, rows in zip(("pop", "hof", "elite"), (s.rows() for s in slabs), want):
        assert len(got) == len(rows)
        for k in range(len(rows)):
            assert bc.same_bits(got[k], rows[k]), (r, name, k)


def promote_case(E, hof, n_roles, tick, variant):
    roles, checks = promote_roles_of(E, hof, n_roles, variant)
    cnt = Words(1, torch.int32, fill=41)
    if tick:
        L.call("coevo_ga_promote_tick", roles, n_roles, E, hof, cnt.p)
    else:
        L.call("coevo_ga_promote", roles, n_roles, E, hof)
    torch.cuda.synchronize()
    assert cnt.get()[0] == (42 if tick else 41)
    for r, (ids, from_pop, to_pop0, pop, hofs, elite, pop0, hof0, elite0, _) in enumerate(checks):
        assert_regions(r, (pop, hofs, elite), bc.promote(list(pop0), list(hof0), list(elite0), ids, E, from_pop, to_pop0))


@pytest.mark.parametrize("n_roles", [1, 2, 3])
@pytest.mark.parametrize("E,hof", [(1, 1), (1, 16), (8, 1), (8, 16), (3, 2)])
def test_promote_vs_list_operations(E, hof, n_roles):
    """every (E, hof) corner of the compile-time recursions, one to three roles of mixed width (the D = 8 role's surplus
    workgroups leave without writing: its regions end in guard rows), with and without the tick"""
    for variant in range(3 if n_roles == 1 else 2):
        promote_case(E, hof, n_roles, tick=(variant + n_roles) % 2 == 1, variant=variant)


# ------------------------------------------------------------------------------------------- 6b. promotion with the twins
class Twins:
    """[n_roles][hof][W2_FLOATS] twin slots between PAD guard words (16 bytes: the slots stay 16-byte aligned), one further
    role's worth of words behind the last role, all of it tm.raw_words: every slot distinct random bits with NaN payloads,
    -0.0 and subnormals - NOT the twins of the Hall of Fame's nets, so that a slot that was recomputed instead of moved, or
    moved the wrong way, shows"""

    def __init__(self, n_roles, hof, seed):
        self.n_roles, self.hof = n_roles, hof
        n = (n_roles + 1) * hof * L.W2_FLOATS
        self.before = tm.raw_words(np.random.Generator(np.random.PCG64([seed, n_roles, hof])), n + 2 * PAD)
        self.buf = dev(self.before)
        self.p = self.buf.data_ptr() + 4 * PAD
        assert self.p % 16 == 0

    def slots(self, a=None):
        """-> [n_roles + 1][hof][W2_FLOATS] uint32 (of `a`, or of the device buffer after asserting its guard words)"""
        if a is None:
            a = self.buf.cpu().numpy()
            assert bc.same_bits(a[:PAD], self.before[:PAD]) and bc.same_bits(a[-PAD:], self.before[-PAD:]), "a guard word was written"
        return a[PAD:-PAD].view(np.uint32).reshape(self.n_roles + 1, self.hof, L.W2_FLOATS)

    def untouched(self):
        return bc.same_bits(self.buf.cpu().numpy(), self.before)


def promote_tiled_case(E, hof, n_roles, variant, launches=1):
    """coevo_ga_promote_tick_tiled, `launches` times back to back on the same buffers: pop / hof / elite and the counter as
    coevo_ga_promote_tick leaves them (bc.promote), the twins as tm.promote_tiled's FIFO - the old slots moved as the words
    they are, the last one twin_of the best's fc2.weight as it was before that launch"""
    roles, checks = promote_roles_of(E, hof, n_roles, variant, raw_w2=True)
    twins, cnt = Twins(n_roles, hof, seed=7 + variant), Words(1, torch.int32, fill=41)
    old = twins.slots(twins.before.copy())
    for _ in range(launches):
        L.call("coevo_ga_promote_tick_tiled", roles, n_roles, E, hof, cnt.p, twins.p)
    torch.cuda.synchronize()
    assert cnt.get()[0] == 41 + launches
    got = twins.slots()
    for r, (ids, from_pop, to_pop0, pop, hofs, elite, pop0, hof0, elite0, _) in enumerate(checks):
        D = ROLE_D[r]
        state = (list(pop0), list(hof0), list(elite0), [old[r, j] for j in range(hof)])
        for _ in range(launches):
            state = tm.promote_tiled(*state, ids, E, from_pop, to_pop0, lambda row: tm.w2_of_slab_row(row, D))
        assert_regions(r, (pop, hofs, elite), state[:3])
        for j, want in enumerate(state[3]):
            bad = np.flatnonzero(got[r, j] != want.view(np.uint32))
            assert not len(bad), (r, "twin slot", j, "of", hof, len(bad), bad[:4])
    assert np.array_equal(got[n_roles], old[n_roles]), "words behind the last role's twins were written"


@pytest.mark.parametrize("n_roles", [1, 2, 3])
@pytest.mark.parametrize("E,hof", [(1, 1), (1, 16), (8, 1), (8, 16), (3, 2)])
def test_promote_tiled_vs_list_operations(E, hof, n_roles):
    """the corners of test_promote_vs_list_operations through ga_promote_tiled_kernel: promote_twin_shift<1..15> at hof 1 (no
    level stores), 2 and 16 (every level does), the clamped loads of the surplus levels, the D = 8 role's surplus workgroups
    beside a D = 10 role, the best in pop[0] written onto itself, elites_from_pop = 0"""
    for variant in range(3 if n_roles == 1 else 2):
        promote_tiled_case(E, hof, n_roles, variant)


@pytest.mark.parametrize("E,hof,n_roles", [(3, 2, 3), (1, 1, 2), (8, 16, 1)])
def test_promote_tiled_twice_is_the_two_step_fifo(E, hof, n_roles):
    for variant in range(2):
        promote_tiled_case(E, hof, n_roles, variant, launches=2)


def test_promote_tiled_refusals_write_nothing():
    E, hof, n_roles = 2, 2, 2
    roles, checks = promote_roles_of(E, hof, n_roles, 0, raw_w2=True)
    twins, cnt = Twins(n_roles, hof, seed=3), Words(1, torch.int32, fill=41)
    lib, st = L.load(), L._stream()

    def call(roles=roles, n_roles=n_roles, E=E, hof=hof, counter=cnt.p, tw=twins.p):
        return lib.coevo_ga_promote_tick_tiled(roles, n_roles, E, hof, counter, tw, st)

    def edited(**fields):
        """the roles with fields of role 1 replaced (a region moved 4 bytes: still inside its slab's allocation)"""
        out = (L.GaPromoteRole * n_roles)()
        for r in range(n_roles):
            out[r] = L.GaPromoteRole(*(getattr(roles[r], f) for f, _ in L.GaPromoteRole._fields_))
        for f, v in fields.items():
            setattr(out[1], f, v(getattr(roles[1], f)) if callable(v) else v)
        return out

    assert call(counter=None) == ERR_ARG and call(tw=None) == ERR_ARG
    assert call(tw=twins.p + 4) == ERR_ARG                                   # 4 bytes off 16-byte alignment
    for region in ("pop", "hof", "elite"):
        assert call(roles=edited(**{region: lambda p: p + 4})) == ERR_ARG, region
    assert call(hof=17) == ERR_ARG and call(hof=0) == ERR_ARG
    assert call(E=9) == ERR_ARG and call(E=0) == ERR_ARG
    assert call(n_roles=0) == ERR_ARG and call(n_roles=4) == ERR_ARG
    assert call(roles=edited(D=9)) == ERR_ARG
    assert call(roles=edited(order=None, elites_from_pop=1)) == ERR_ARG       # elites_from_pop without an order
    torch.cuda.synchronize()
    assert cnt.get()[0] == 41 and twins.untouched()
    for r, (_, _, _, pop, hofs, elite, pop0, hof0, elite0, _) in enumerate(checks):
        assert_regions(r, (pop, hofs, elite), (pop0, hof0, elite0))


# ------------------------------------------------------------------------------------------- 7. the ES update
def es_setup(D, n, sigma, kind):
    """theta in row 0 with its own padding, the n perturbed nets bred by coevo_fc_perturb behind it, then NaN planted in the
    LayerNorm and padding words of the perturbed nets"""
    theta, pert, fit = bc.es_inputs(D, n, float(sigma), kind)
    s = Slab(1 + n, D).load(theta[None])
    zero, d_sigma = dev(np.zeros(n, dtype=np.int32)), dev(np.array([sigma], dtype=np.float32))
    L.call("coevo_fc_perturb", s.p, L._p(zero), s.p, 1, n, D, L._p(d_sigma), bc.ES_SEED, 0, bc.ES_SHI, 1)
    got = s.flat(1, n)
    assert bc.same_f32(got, pert), "the perturbed nets are not the reference's: see test_perturb_every_word"
    m = bc.slab_to_flat(D)
    dead = dev((m < 0) | bc.ln_mask(D)[np.maximum(m, 0)])
    s.t[1:, dead] = float("nan")
    return s, theta, pert, fit, d_sigma, dev(fit)


def check_theta(s, theta, want, D, what):
    row, flat = s.rows()[0], s.flat(0, 1)[0]
    ln = bc.ln_mask(D)
    assert bc.same_bits(row[bc.params(D):], np.full(bc.stride(D) - bc.params(D), bc.padding_of(0))), (what, "padding")
    assert bc.same_bits(flat[ln], theta[ln]), (what, "LayerNorm")
    assert bc.same_f32(flat, want), (what, bc.first_diff(flat, want))
    return flat


@pytest.mark.parametrize("D,n,chunks,kind,sigma,lr", bc.es_cases())
def test_es_update_vs_numpy(D, n, chunks, kind, sigma, lr):
    s, theta, pert, fit, d_sigma, d_fit = es_setup(D, n, sigma, kind)
    stride = s.stride
    want, unsafe, ref64, bound = bc.es_update(theta, pert, fit, D, sigma, lr, chunks)
    assert unsafe == 0
    theta_row = s.t[0].clone()
    if chunks == 1:     # the one-launch form, then chunks_total = 1 of the two-step form: the same bits
        L.call("coevo_es_update", s.p, s.row(1), D, L._p(d_fit), n, L._p(d_sigma), C.c_float(lr))
        one = check_theta(s, theta, want, D, "es_update")
        s.t[0].copy_(theta_row)
    # the two-step form in a two-block layout with 8 NaN gap words after each block that nobody may read
    cpb = (chunks + 1) // 2 if chunks > 1 else 1
    n_blk = (chunks + cpb - 1) // cpb
    bstride = cpb * stride + 8
    parts = Words(n_blk * bstride, fill=float("nan"))
    for b in range(n_blk):
        first, cnt = b * cpb, min(cpb, chunks - b * cpb)
        lo = first * n // chunks
        L.call("coevo_es_partial", s.p, s.row(1 + lo), lo, D, L._p(d_fit), n, chunks, first, cnt, parts.p + 4 * b * bstride)
    L.call("coevo_es_apply", s.p, parts.p, chunks, cpb, bstride, D, n, L._p(d_sigma), C.c_float(lr))
    two = check_theta(s, theta, want, D, "es_partial + es_apply")
    if chunks == 1:
        assert bc.same_bits(one, two)
    pw = parts.get().reshape(n_blk, bstride)
    assert np.isnan(pw[:, cpb * stride:]).all(), "a gap word was written"
    for c, (lo, hi) in enumerate(bc.es_chunk_bounds(n, chunks)):
        chunk = pw[c // cpb, (c % cpb) * stride:(c % cpb + 1) * stride]
        if lo == hi:
            assert not chunk.view(np.uint32).any(), ("an empty chunk is not zeros", c)
    if kind == "random" and sigma == bc.ES_SIGMAS[0]:
        assert (np.abs(two.astype(np.float64) - ref64) <= bound).all()
    # the perturbed nets were only read
    assert bc.same_f32(s.flat(1, n)[:, ~bc.ln_mask(D)], pert[:, ~bc.ln_mask(D)])


# ------------------------------------------------------------------------------------------- 8. refused arguments
def test_refused_arguments_write_nothing():
    D = 8
    parents, _ = parent_slab(D)
    nb = bc.n_blocks(D)
    child, part, f32o = Slab(3, D), Words(3 * nb, torch.float64), Words(64)
    idx, sigma = dev(np.zeros(8, dtype=np.int32)), dev(np.array([0.05, 0.05, 0.05], dtype=np.float32))
    fit = dev(np.ones(8, dtype=np.float32))
    lib, st = L.load(), L._stream()

    def perturb_dist(n_children=2, child_first=0, D=D, flags=0, ref=parents.p, partial=part.p):
        return lib.coevo_fc_perturb_dist(parents.p, L._p(idx), child.p, child_first, n_children, D, L._p(sigma), 1, 0, 0, flags,
                                         None, ref, partial, st)
    assert perturb_dist(n_children=-1) == ERR_ARG and perturb_dist(n_children=65536) == ERR_ARG
    assert perturb_dist(child_first=-1) == ERR_ARG
    assert perturb_dist(flags=4) == ERR_ARG and perturb_dist(flags=-1) == ERR_ARG
    assert perturb_dist(ref=None) == ERR_ARG and perturb_dist(partial=None) == ERR_ARG
    # D = 9 at every entry point
    assert perturb_dist(D=9) == ERR_ARG
    head = (parents.p, L._p(idx), child.p, 0, 2, 9, L._p(sigma), 1, 0, 0)
    assert lib.coevo_fc_perturb(*head, 0, st) == ERR_ARG and lib.coevo_fc_perturb_flags(*head, 0, st) == ERR_ARG
    assert lib.coevo_fc_perturb_gen(*head, 0, L._p(idx), st) == ERR_ARG
    assert lib.coevo_fc_perturb_flags(*head[:5], D, *head[6:], 4, st) == ERR_ARG
    assert lib.coevo_fc_perturb_blocks(9) == ERR_ARG and lib.coevo_fc_param_count(9) == ERR_ARG
    assert lib.coevo_fc_pack(parents.p, child.p, 1, 9, st) == ERR_ARG and lib.coevo_fc_unpack(parents.p, child.p, 1, 9, st) == ERR_ARG
    job = (L.PerturbJob * 1)(L.PerturbJob(parents.p, L._p(idx), child.p, L._p(sigma), None, None, 0, 2, 9, 0, 0, 0))
    assert lib.coevo_fc_perturb_dist_multi(C.cast(job, C.c_void_p), 1, 1, 0, None, st) == ERR_ARG
    job[0].D = D
    assert lib.coevo_fc_perturb_dist_multi(C.cast(job, C.c_void_p), 0, 1, 0, None, st) == ERR_ARG
    assert lib.coevo_fc_perturb_dist_multi(C.cast(job, C.c_void_p), 5, 1, 0, None, st) == ERR_ARG
    assert lib.coevo_fc_perturb_dist_multi(C.cast(job, C.c_void_p), 1, 1, 4, None, st) == ERR_ARG
    assert lib.coevo_fc_rebuild_elites(parents.p, L._p(idx), child.p, 2, 9, L._p(sigma), 1, 0, None, st) == ERR_ARG
    assert lib.coevo_es_update(child.p, parents.p, 9, L._p(fit), 2, L._p(sigma), 0.1, st) == ERR_ARG
    assert lib.coevo_es_partial(child.p, parents.p, 0, 9, L._p(fit), 2, 1, 0, 1, child.row(1), st) == ERR_ARG
    assert lib.coevo_es_apply(child.p, child.row(1), 1, 1, 0, 9, 2, L._p(sigma), 0.1, st) == ERR_ARG
    # rebuild
    assert lib.coevo_fc_rebuild_elites(parents.p, L._p(idx), child.p, 0, D, L._p(sigma), 1, 0, None, st) == ERR_ARG
    assert lib.coevo_fc_rebuild_elites(child.p, L._p(idx), child.p, 2, D, L._p(sigma), 1, 0, None, st) == ERR_ARG
    # promotion
    pop, hof, elite = Slab(2, D), Slab(2, D), Slab(2, D)

    def role(D=D, order=L._p(idx), from_pop=1):
        return (L.GaPromoteRole * 1)(L.GaPromoteRole(pop.p, hof.p, elite.p, order, D, from_pop, 1, 0))
    for E, h, n_roles in ((0, 2, 1), (9, 2, 1), (2, 0, 1), (2, 17, 1), (2, 2, 0), (2, 2, 4)):
        assert lib.coevo_ga_promote(role(), n_roles, E, h, st) == ERR_ARG, (E, h, n_roles)
    assert lib.coevo_ga_promote(role(order=None), 1, 2, 2, st) == ERR_ARG          # elites_from_pop with no order
    assert lib.coevo_ga_promote(role(D=9), 1, 2, 2, st) == ERR_ARG
    assert lib.coevo_ga_promote_tick(role(), 1, 2, 2, None, st) == ERR_ARG
    assert lib.coevo_ga_promote_rebuild(role(from_pop=0), 1, 2, 2, None, 1, 0, None, st) == ERR_ARG        # no sigma
    assert lib.coevo_ga_promote_rebuild(role(order=None, from_pop=0), 1, 2, 2, L._p(sigma), 1, 0, None, st) == ERR_ARG
    assert lib.coevo_ga_promote_rebuild(role(D=9, from_pop=0), 1, 2, 2, L._p(sigma), 1, 0, None, st) == ERR_ARG
    # ES
    assert lib.coevo_es_partial(child.p, parents.p, 1, D, L._p(fit), 8, 4, 0, 2, child.row(1), st) == ERR_ARG   # chunk 0 starts at 0
    assert lib.coevo_es_partial(child.p, parents.p, 4, D, L._p(fit), 8, 4, 2, 3, child.row(1), st) == ERR_ARG   # 2 + 3 > 4 chunks
    assert lib.coevo_es_apply(child.p, child.row(1), 2, 1, L.fc_slab_stride(D) + 2, D, 8, L._p(sigma), 0.1, st) == ERR_ARG
    assert lib.coevo_es_update(child.p, parents.p, D, L._p(fit), 0, L._p(sigma), 0.1, st) == ERR_ARG
    assert lib.coevo_philox_normals(1, 0, 0, 0, 0, f32o.p, st) == ERR_ARG
    torch.cuda.synchronize()
    assert is_sent(child.rows()) and part.untouched() and f32o.untouched()
    assert is_sent(pop.rows()) and is_sent(hof.rows()) and is_sent(elite.rows())
