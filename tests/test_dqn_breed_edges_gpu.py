"""The fp32 DeepQN population kernels through the C ABI at their edges, against the plain numpy / fsum / Python references of
tests/dqn_breed_cases.py (proven on the CPU by tests/test_dqn_breed_edges_cpu.py): the word-moving kernels coevo_dqn_pack /
_unpack / _relayout on raw bit patterns, every word of every child of coevo_dqn_perturb in both fc1 layouts (streamed, tiled,
generic and copy paths; the fused distance partials with their shifted block boundaries), the chunked ES update
coevo_dqn_es_partial / _apply with its three-range BatchNorm skip, and coevo_synth_step with scripted actions.  Slabs are built
on the host from the numpy slab map, so a perturb or ES failure is that kernel's and not the pack kernel's.  Finite and infinite
results as bits, NaN by position; moves as raw bits.  Every buffer a launch writes lies between guard rows / words, and what a
launch must not touch is asserted untouched."""
import numpy as np
import pytest
import torch

from coevonet_amd import lib as L
from tests import breed_cases as bc
from tests import dqn_breed_cases as dc

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
SENT = -7.25
PAD = 4
ERR_ARG = -1
COPY, FROM_ORDER = 8, 4


# ------------------------------------------------------------------------------------------- plumbing
def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


class Rows:
    """n rows of `width` fp32 words between one guard row on each side, everything the sentinel at first"""

    def __init__(self, n, width):
        self.n, self.width = n, width
        self.buf = torch.full((n + 2, width), SENT, dtype=torch.float32, device=DEV)
        self.t = self.buf[1:n + 1]
        self.p = self.t.data_ptr()

    def row(self, i):
        return self.p + 4 * i * self.width

    def put(self, rows, first=0):
        """fp32 rows, or uint32 rows taken as bit patterns"""
        rows = np.ascontiguousarray(rows)
        if rows.dtype == np.uint32:
            self.t.view(torch.int32)[first:first + len(rows)] = dev(rows.view(np.int32))
        else:
            self.t[first:first + len(rows)] = dev(rows.astype(np.float32, copy=False))
        return self

    def rows(self):
        """-> the n raw rows, after asserting the guard rows"""
        a = self.buf.cpu().numpy()
        assert (a[0] == SENT).all() and (a[-1] == SENT).all(), "a guard row was written"
        return a[1:-1]


def slab(n, C, n_act):
    """(the numpy layout sizes every buffer here: it must be the library's before anything is launched on them)"""
    lib = L.load()
    assert (int(lib.coevo_dqn_slab_stride(C, n_act)), int(lib.coevo_dqn_param_count(C, n_act))) == (dc.stride(C, n_act), dc.params(C, n_act))
    for tiled in dc.LAYOUTS:
        assert int(lib.coevo_dqn_perturb_blocks(C | tiled, n_act)) == dc.n_blocks(C, n_act, tiled)
    return Rows(n, dc.stride(C, n_act))


class Words:
    """n words between PAD guard words, all of it `fill`"""

    def __init__(self, n, dtype=torch.float32, fill=SENT):
        self.n, self.fill = n, fill
        self.buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=DEV)
        self.t = self.buf[PAD:PAD + n]
        self.p = self.t.data_ptr()

    def _is_fill(self, a):
        return bool(torch.isnan(a).all() if isinstance(self.fill, float) and np.isnan(self.fill) else (a == self.fill).all())

    def guards_ok(self):
        return self._is_fill(self.buf[:PAD]) and self._is_fill(self.buf[PAD + self.n:])

    def get(self):
        assert self.guards_ok(), "a guard word was written"
        return self.t.cpu().numpy()

    def untouched(self):
        return self.guards_ok() and self._is_fill(self.t)


def is_sent(rows):
    return bool((np.asarray(rows) == SENT).all())


def rc(name, *args):
    """the entry point's return code (no exception)"""
    return getattr(L.load(), name)(*args, L._stream())


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def parent_rows(C, n_act, tiled, count=dc.N_PARENTS):
    nets = dc.planted_parents(C, n_act)[:count]
    return nets, np.stack([dc.to_slab_rows(nets[k], C, n_act, tiled, dc.padding_of(k)) for k in range(count)])


def perturb(parents_p, pidx, child_p, child_first, n, carg, n_act, sigma, slo_first, shi, flags, E=1, gen=None, gen_bias=0,
            ref=None, part=None):
    L.call("coevo_dqn_perturb", parents_p, L._p(pidx), child_p, child_first, n, carg, n_act, L._p(sigma), dc.SEED,
           slo_first & bc.M32, shi, flags, E, L._p(gen), gen_bias, ref, part)


def check_children(rows, want, pidx, prow, C, n_act, tiled, flags, what):
    """rows: the children's slab rows in launch order; want: canonical [n][P]; prow: the parents' slab rows"""
    total, bn = dc.layout(C, n_act).total, dc.bn_slab_mask(C, n_act)
    for k, p in enumerate(pidx):
        want_row = dc.to_slab_rows(want[k], C, n_act, tiled, dc.padding_of(p))
        assert bc.same_f32(rows[k], want_row), (what, k, bc.first_diff(rows[k], want_row))
        assert bc.same_bits(rows[k][total:], prow[p][total:]), (what, k, "padding")
        if flags & 1:
            assert bc.same_bits(rows[k][bn], prow[p][bn]), (what, k, "BatchNorm bits")


# ------------------------------------------------------------------------------------------- 1. the slab map and the moves
@pytest.mark.parametrize("tiled", dc.LAYOUTS)
@pytest.mark.parametrize("C,n_act", dc.SHAPES)
def test_pack_is_the_numpy_slab_map(C, n_act, tiled):
    assert L.DQN_FC1_TILED == dc.TILED
    lib = L.load()
    P, m = dc.params(C, n_act), dc.slab_to_flat(C, n_act, tiled)
    assert (int(lib.coevo_dqn_param_count(C, n_act)), int(lib.coevo_dqn_slab_stride(C, n_act))) == (P, len(m))
    assert int(lib.coevo_dqn_perturb_blocks(C | tiled, n_act)) == dc.n_blocks(C, n_act, tiled)
    assert P < 2 ** 24                                   # float(p) is exact
    flat = np.stack([np.arange(P, dtype=np.float32), np.arange(P, dtype=np.float32)[::-1]])
    d_flat = dev(flat)
    s = slab(2, C, n_act)
    L.call("coevo_dqn_pack", L._p(d_flat), s.p, 2, C | tiled, n_act)
    rows = s.rows()
    want = np.where(m >= 0, m, 0).astype(np.float32)
    assert bc.same_bits(rows[0], want), bc.first_diff(rows[0], want)
    assert bc.same_bits(rows[1], np.where(m >= 0, P - 1 - m, 0).astype(np.float32))      # padding: +0


@pytest.mark.parametrize("tiled", dc.LAYOUTS)
@pytest.mark.parametrize("C,n_act", dc.SHAPES)
def test_relayout_moves_raw_bits(C, n_act, tiled):
    """source layout `tiled`: -> the other layout -> back, and -> the same layout; padding travels with the net"""
    other = dc.TILED - tiled
    src = dc.bit_pattern_rows(C, n_act, 2)
    a, b, c, same = (slab(2, C, n_act) for _ in range(4))
    a.put(src)
    L.call("coevo_dqn_relayout", a.p, b.p, 2, C | tiled, C | other, n_act)
    L.call("coevo_dqn_relayout", b.p, c.p, 2, C | other, C | tiled, n_act)
    L.call("coevo_dqn_relayout", a.p, same.p, 2, C | tiled, C | tiled, n_act)
    assert np.array_equal(u32(a.rows()), src), "the source changed"
    assert np.array_equal(u32(c.rows()), src), "round trip"
    assert np.array_equal(u32(same.rows()), src), "same layout"
    # the twin against the two numpy maps: canonical word by canonical word, padding in place
    m_src, m_dst = dc.slab_to_flat(C, n_act, tiled), dc.slab_to_flat(C, n_act, other)
    live = m_src >= 0
    got = u32(b.rows())
    for k in range(2):
        canon = np.empty(dc.params(C, n_act), dtype=np.uint32)
        canon[m_src[live]] = src[k][live]
        want = src[k].copy()
        want[live] = canon[m_dst[live]]
        assert np.array_equal(got[k], want), k
    assert not np.array_equal(got, src)


@pytest.mark.parametrize("tiled", dc.LAYOUTS)
@pytest.mark.parametrize("C,n_act", dc.SHAPES)
def test_unpack_writes_the_live_words_as_bits_and_nothing_else(C, n_act, tiled):
    P, m = dc.params(C, n_act), dc.slab_to_flat(C, n_act, tiled)
    src = dc.bit_pattern_rows(C, n_act, 2, seed=6)
    s, out = slab(2, C, n_act).put(src), Rows(3, P)            # row 2 of the output: a canary behind the last net
    L.call("coevo_dqn_unpack", s.p, out.p, 2, C | tiled, n_act)
    got = out.rows()
    assert is_sent(got[2]), "written past the last net"
    live = m >= 0
    for k in range(2):
        want = np.empty(P, dtype=np.uint32)
        want[m[live]] = src[k][live]
        assert np.array_equal(u32(got[k]), want), k
    assert np.array_equal(u32(s.rows()), src)
    # ... and pack o unpack is the identity on canonical bits
    back = slab(2, C, n_act)
    L.call("coevo_dqn_pack", out.p, back.p, 2, C | tiled, n_act)
    rows = u32(back.rows())
    assert np.array_equal(rows[:, live], src[:, live]) and not rows[:, ~live].any()


# ------------------------------------------------------------------------------------------- 2. perturb, every word
@pytest.mark.parametrize("name", list(dc.perturb_cases()))
def test_perturb_every_word(name):
    c = dc.perturb_cases()[name]
    (C, n_act), tiled, n = c["shape"], c["tiled"], len(c["pidx"])
    nets, prow = parent_rows(C, n_act, tiled)
    parents = slab(dc.N_PARENTS, C, n_act).put(prow)
    child = slab(1 + n + 1, C, n_act)                    # a net before child_first and one after the last child
    d_pidx, sigma = dev(np.array(c["pidx"], dtype=np.int32)), dev(np.array([c["sigma"]], dtype=np.float32))
    gen = dev(np.array([c["gen"]], dtype=np.int32)) if c["gen"] is not None else None
    perturb(parents.p, d_pidx, child.p, 1, n, C | tiled, n_act, sigma, c["slo_first"], c["shi"], c["flags"], gen=gen,
            gen_bias=c["gen_bias"])
    rows = child.rows()
    assert is_sent(rows[0]) and is_sent(rows[1 + n]), "a net outside [child_first, child_first + n) was written"
    check_children(rows[1:1 + n], dc.perturb_want(c), c["pidx"], prow, C, n_act, tiled, c["flags"], name)
    assert bc.same_bits(parents.rows(), prow), "a parent changed"


@pytest.mark.parametrize("with_gen", [False, True])
@pytest.mark.parametrize("tiled", dc.LAYOUTS)
@pytest.mark.parametrize("E", [1, 2, 3])
def test_from_order_vs_numpy_and_vs_the_materialised_child(E, tiled, with_gen):
    C, n_act = dc.SHAPES[(E + with_gen + (tiled != 0)) % 4]
    order = dc.ORDERS[E]
    n = len(order)
    nets, prow = parent_rows(C, n_act, tiled)
    old = slab(E, C, n_act).put(prow[:E])
    new, plain = slab(1 + n + 1, C, n_act), slab(n, C, n_act)
    d_order, sigma = dev(np.array(order, dtype=np.int32)), dev(np.array([0.05], dtype=np.float32))
    gen = dev(np.array([dc.ORDER_GEN], dtype=np.int32)) if with_gen else None
    perturb(old.p, d_order, new.p, 1, n, C | tiled, n_act, sigma, 12345, dc.ORDER_SHI, FROM_ORDER, E=E, gen=gen,
            gen_bias=dc.ORDER_GEN_BIAS)
    keep = []
    for k, ident in enumerate(order):      # the plain launch with stream_lo_first = id - 1 from parent (id - 1) % E
        if ident:
            keep.append(dev(np.array([(ident - 1) % E], dtype=np.int32)))
            perturb(old.p, keep[-1], plain.p, k, 1, C | tiled, n_act, sigma, ident - 1, dc.ORDER_SHI, 0, gen=gen,
                    gen_bias=dc.ORDER_GEN_BIAS)
    rows, prows = new.rows(), plain.rows()
    assert is_sent(rows[0]) and is_sent(rows[1 + n])
    src = [0 if i == 0 else (i - 1) % E for i in order]
    check_children(rows[1:1 + n], dc.order_want(C, n_act, E, with_gen), src, prow, C, n_act, tiled, 0, (E, order))
    for k, ident in enumerate(order):
        assert bc.same_bits(rows[1 + k], prow[0] if ident == 0 else prows[k]), (order, k)
    assert bc.same_bits(old.rows(), prow[:E])


@pytest.mark.parametrize("tiled", dc.LAYOUTS)
@pytest.mark.parametrize("C,n_act", dc.SHAPES)
def test_copy_flag_copies_bits_or_only_measures(C, n_act, tiled):
    nets, prow = parent_rows(C, n_act, tiled)
    parents = slab(dc.N_PARENTS, C, n_act).put(prow)
    n, nb = len(dc.PIDX), dc.n_blocks(C, n_act, tiled)
    d_pidx = dev(np.array(dc.PIDX, dtype=np.int32))
    child = slab(1 + n + 1, C, n_act)
    perturb(parents.p, d_pidx, child.p, 1, n, C | tiled, n_act, None, 7, 7, COPY | 3)     # no sigma, bits 0 and 1 beside COPY
    rows = child.rows()
    assert is_sent(rows[0]) and is_sent(rows[1 + n])
    for k, p in enumerate(dc.PIDX):
        assert bc.same_bits(rows[1 + k], prow[p]), (k, "NaN payloads, padding and all")
    # no child slab: the distance of the existing nets to a reference, nothing else written
    ref_flat, ref_pad = dc.dist_ref(C, n_act, "unrelated")
    ref = slab(1, C, n_act).put(dc.to_slab_rows(ref_flat, C, n_act, tiled, ref_pad)[None])
    part = Words(n * nb, torch.float64)
    perturb(parents.p, d_pidx, None, 0, n, C | tiled, n_act, None, 7, 7, COPY, ref=ref.p, part=part.p)
    got = part.get().reshape(n, nb)
    for k, p in enumerate(dc.PIDX):
        assert bc.same_partials(got[k], dc.dist_partials(nets[p], ref_flat, C, n_act, tiled)), k
    assert bc.same_bits(parents.rows(), prow) and bc.same_bits(child.rows()[1:1 + n], rows[1:1 + n])


DIST_PIDX = dc.DIST_PIDX


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("ref_kind", ["parent", "unrelated", "inf"])
@pytest.mark.parametrize("tiled", dc.LAYOUTS)
@pytest.mark.parametrize("C,n_act", dc.SHAPES)
def test_fused_distance_vs_fsum(C, n_act, tiled, ref_kind, flags):
    """the partials of every workgroup (shifted by dqn_perturb_shift quads in the tiled layout) against fsum over its live
    words: BatchNorm words count even when they are not perturbed, padding never does - the parents carry 1000.5 + k there, the
    references NaN or -3000.25"""
    nets, prow = parent_rows(C, n_act, tiled)
    parents = slab(dc.N_PARENTS, C, n_act).put(prow)
    c = dc.plain_case((C, n_act), tiled, flags, DIST_PIDX)
    n, nb = len(DIST_PIDX), dc.n_blocks(C, n_act, tiled)
    if ref_kind == "parent":
        ref_flat, ref_ptr = nets[0], parents.row(0)
    else:
        ref_flat, ref_pad = dc.dist_ref(C, n_act, ref_kind)
        ref = slab(1, C, n_act).put(dc.to_slab_rows(ref_flat, C, n_act, tiled, ref_pad)[None])
        ref_ptr = ref.p
    child, part, dist = slab(n, C, n_act), Words(n * nb, torch.float64), Words(n)
    d_pidx, sigma = dev(np.array(DIST_PIDX, dtype=np.int32)), dev(np.array([0.05], dtype=np.float32))
    perturb(parents.p, d_pidx, child.p, 0, n, C | tiled, n_act, sigma, c["slo_first"], c["shi"], flags, ref=ref_ptr, part=part.p)
    L.call("coevo_fc_distance_finalize", part.p, nb, n, dist.p, 0, None)
    want = dc.perturb_want(c)
    check_children(child.rows(), want, DIST_PIDX, prow, C, n_act, tiled, flags, ref_kind)
    got_p, got_d = part.get().reshape(n, nb), dist.get()
    for k, p in enumerate(DIST_PIDX):
        want_p = dc.dist_partials(want[k], ref_flat, C, n_act, tiled)
        bad = np.flatnonzero(~np.isclose(got_p[k], want_p, rtol=1e-12, atol=0, equal_nan=True))
        assert bc.same_partials(got_p[k], want_p), (k, bad[:8], got_p[k][bad[:4]], want_p[bad[:4]])
        assert bc.within_one_ulp(got_d[k], bc.final_distance(want_p)), (k, got_d[k], bc.final_distance(want_p))
        if p == 0:      # the finite parent
            assert np.isfinite(want_p).all() == (ref_kind != "inf")
            if ref_kind == "parent":      # the norm of the noise over every word that took some (+-FLT_MAX + noise = +-FLT_MAX)
                nz = bc.noise(F32(0.05), dc.SEED, c["slo_first"] + k, c["shi"], flags, dc.params(C, n_act))
                took = np.abs(nets[0]) < 1e30
                if flags & 1:
                    took &= ~dc.bn_mask(C, n_act)
                assert abs(float(got_d[k]) / np.linalg.norm(nz[took].astype(np.float64)) - 1) < 1e-3
                assert np.isfinite(got_d[k])


@pytest.mark.parametrize("C,n_act,tiled,flags", dc.IN_PLACE)
def test_perturb_in_place_after_the_parents(C, n_act, tiled, flags):
    """child_slab == parent_slab, the children placed after the parents (the ES form)"""
    c = dc.plain_case((C, n_act), tiled, flags, (2, 0, 2, 1))
    nets, prow = parent_rows(C, n_act, tiled)
    s = slab(dc.N_PARENTS + 4 + 1, C, n_act).put(prow)
    d_pidx, sigma = dev(np.array(c["pidx"], dtype=np.int32)), dev(np.array([0.05], dtype=np.float32))
    perturb(s.p, d_pidx, s.p, dc.N_PARENTS, 4, C | tiled, n_act, sigma, c["slo_first"], c["shi"], flags)
    rows = s.rows()
    assert bc.same_bits(rows[:dc.N_PARENTS], prow) and is_sent(rows[-1])
    check_children(rows[dc.N_PARENTS:dc.N_PARENTS + 4], dc.perturb_want(c), c["pidx"], prow, C, n_act, tiled, flags, "in place")


def test_perturb_no_children_writes_nothing():
    C, n_act = 1, 1
    _, prow = parent_rows(C, n_act, 0)
    parents = slab(dc.N_PARENTS, C, n_act).put(prow)
    child, part = slab(2, C, n_act), Words(2 * dc.n_blocks(C, n_act, dc.TILED), torch.float64)
    d_pidx, sigma = dev(np.zeros(2, dtype=np.int32)), dev(np.array([0.05], dtype=np.float32))
    for carg in (C, C | dc.TILED):
        assert rc("coevo_dqn_perturb", parents.p, L._p(d_pidx), child.p, 0, 0, carg, n_act, L._p(sigma), 1, 0, 0, 0, 1, None, 0,
                  parents.p, part.p) == 0
    torch.cuda.synchronize()
    assert is_sent(child.rows()) and part.untouched()


def test_perturb_refusals_write_nothing():
    C, n_act = 3, 5
    _, prow = parent_rows(C, n_act, 0)
    parents = slab(dc.N_PARENTS, C, n_act).put(prow)
    child, part = slab(3, C, n_act), Words(3 * dc.n_blocks(C, n_act, dc.TILED), torch.float64)
    idx, sigma = dev(np.zeros(8, dtype=np.int32)), dev(np.array([0.05], dtype=np.float32))
    base = dict(parent=parents.p, pidx=L._p(idx), child=child.p, first=0, n=2, carg=C, n_act=n_act, sigma=L._p(sigma), flags=0,
                E=1, ref=parents.p, part=part.p)

    def call(**kw):
        a = dict(base, **kw)
        return rc("coevo_dqn_perturb", a["parent"], a["pidx"], a["child"], a["first"], a["n"], a["carg"], a["n_act"], a["sigma"],
                  1, 0, 0, a["flags"], a["E"], None, 0, a["ref"], a["part"])
    refused = dict(
        ref_without_partial=dict(part=None), partial_without_ref=dict(ref=None), neither_output=dict(child=None, ref=None, part=None),
        flags_16=dict(flags=16), flags_negative=dict(flags=-1), no_sigma=dict(sigma=None), no_parent=dict(parent=None),
        order_without_idx=dict(flags=FROM_ORDER, pidx=None), order_E0=dict(flags=FROM_ORDER, E=0),
        order_in_place=dict(flags=FROM_ORDER, child=parents.p), too_many=dict(n=65536), negative_n=dict(n=-1),
        negative_first=dict(first=-1), stray_bit=dict(carg=C | 0x200), stray_high_bit=dict(carg=C | dc.TILED | 0x10000),
        C0=dict(carg=0), C7=dict(carg=7), C0_tiled=dict(carg=dc.TILED), n0=dict(n_act=0), n33=dict(n_act=33))
    for what, kw in refused.items():
        assert call(**kw) == ERR_ARG, what
    lib = L.load()
    for carg, n in ((0, 5), (7, 5), (3, 0), (3, 33), (3 | 0x200, 5)):
        assert lib.coevo_dqn_perturb_blocks(carg, n) == ERR_ARG
        assert lib.coevo_dqn_unpack(parents.p, child.p, 1, carg, n, L._stream()) == ERR_ARG
        assert lib.coevo_dqn_pack(parents.p, child.p, 1, carg, n, L._stream()) == ERR_ARG
        assert lib.coevo_dqn_relayout(parents.p, child.p, 1, carg, carg, n, L._stream()) == ERR_ARG
    assert lib.coevo_dqn_relayout(parents.p, child.p, 1, 3, 4 | dc.TILED, 5, L._stream()) == ERR_ARG     # other channel count
    assert lib.coevo_dqn_relayout(parents.p, parents.p, 1, 3, 3 | dc.TILED, 5, L._stream()) == ERR_ARG   # in place
    assert call(flags=COPY, sigma=None, n=0) == 0                                                          # (accepted: no sigma under COPY)
    torch.cuda.synchronize()
    assert is_sent(child.rows()) and part.untouched() and bc.same_bits(parents.rows(), prow)


# ------------------------------------------------------------------------------------------- 3. the ES update
def es_layout(chunks, form, stride):
    """-> (chunks_per_block, blocks, block stride in floats, launches [(chunk_first, n_chunks)])"""
    if form == "two_block":
        cpb = 2
        n_blk = (chunks + cpb - 1) // cpb
        return cpb, n_blk, cpb * stride + 8, [(b * cpb, min(cpb, chunks - b * cpb)) for b in range(n_blk)]
    launches = [(0, chunks)] if form == "one" else [(0, 1), (1, chunks - 1)]
    return chunks, 1, chunks * stride, launches


@pytest.mark.parametrize("case", dc.es_cases(), ids=dc.es_id)
def test_es_update_vs_numpy(case):
    shape, n, chunks, kind, sigma, lr, form = case
    C, n_act = shape
    theta, fit, want, unsafe, ref64, bound = dc.es_want(shape, n, chunks, kind, sigma, lr)
    assert unsafe == 0, "an emulated fma term that is not provably the fused result: choose another seed"
    pert = dc.es_inputs(shape, n, float(sigma))[1]
    stride, total, bn = dc.stride(C, n_act), dc.layout(C, n_act).total, dc.bn_slab_mask(C, n_act)
    theta_row = dc.to_slab_rows(theta, C, n_act, 0, dc.padding_of(0))
    ts = slab(1, C, n_act).put(theta_row[None])
    ps = slab(n, C, n_act).put(np.stack([dc.to_slab_rows(pert[i], C, n_act, 0, dc.es_pert_padding(i)) for i in range(n)]))
    before = ps.buf.clone()
    d_fit, d_sigma = dev(fit), dev(np.array([sigma], dtype=np.float32))
    cpb, n_blk, bstride, launches = es_layout(chunks, form, stride)
    parts = Words(n_blk * bstride, fill=float("nan"))
    bounds = bc.es_chunk_bounds(n, chunks)
    for first, cnt in launches:             # each launch on its own shard of the nets: pert_slab_local = net `lo`
        lo = bounds[first][0]
        dest = parts.p + 4 * ((first // cpb) * bstride + (first % cpb) * stride)
        L.call("coevo_dqn_es_partial", ts.p, ps.row(lo), lo, C, n_act, L._p(d_fit), n, chunks, first, cnt, dest)
    L.call("coevo_dqn_es_apply", ts.p, parts.p, chunks, cpb, bstride, C, n_act, n, L._p(d_sigma), float(lr))
    row = ts.rows()[0]
    assert bc.same_bits(row[total:], theta_row[total:]), "padding"
    assert bc.same_bits(row[bn], theta_row[bn]), "BatchNorm words"
    flat = dc.from_slab_row(row, C, n_act, 0)
    assert bc.same_f32(flat, want), bc.first_diff(flat, want)
    if kind == "random" and sigma == dc.ES_SIGMAS[0]:
        assert (np.abs(flat.astype(np.float64) - ref64) <= bound).all()
    # the partial buffer: guards and gap words still NaN, an empty chunk all zero bits
    assert parts.guards_ok()
    pw = parts.t.view(n_blk, bstride)
    assert bool(torch.isnan(pw[:, cpb * stride:]).all()), "a gap word was written"
    for c, (lo, hi) in enumerate(bounds):
        if lo == hi:
            chunk = pw[c // cpb, (c % cpb) * stride:(c % cpb + 1) * stride]
            assert not bool(chunk.view(torch.int32).any()), ("an empty chunk is not zeros", c)
    assert torch.equal(ps.buf.view(torch.int32), before.view(torch.int32)), "the perturbed nets were written"


def test_es_refusals_write_nothing():
    C, n_act = 1, 1
    stride = dc.stride(C, n_act)
    ts, ps, parts = slab(1, C, n_act), slab(8, C, n_act), Words(4 * stride + 8)
    fit, sigma = dev(np.ones(8, dtype=np.float32)), dev(np.array([0.05], dtype=np.float32))
    lib, st = L.load(), L._stream()

    def partial(ind_first=0, C=C, n_act=n_act, n=8, chunks=4, first=0, cnt=2, theta=ts.p, pert=ps.p, f=L._p(fit), out=parts.p):
        return lib.coevo_dqn_es_partial(theta, pert, ind_first, C, n_act, f, n, chunks, first, cnt, out, st)

    def apply(chunks=4, cpb=2, bstride=2 * stride + 8, C=C, n_act=n_act, n=8, theta=ts.p, p=parts.p, s=L._p(sigma)):
        return lib.coevo_dqn_es_apply(theta, p, chunks, cpb, bstride, C, n_act, n, s, 0.1, st)
    assert partial(ind_first=1) == ERR_ARG                          # chunk 0 starts at individual 0
    assert partial(first=1, ind_first=0) == ERR_ARG                 # chunk 1 of 4 over 8 starts at individual 2
    assert partial(first=1, ind_first=3) == ERR_ARG
    assert partial(first=2, ind_first=4, cnt=3) == ERR_ARG          # 2 + 3 > 4 chunks
    assert partial(cnt=0) == ERR_ARG and partial(n=0) == ERR_ARG and partial(chunks=0) == ERR_ARG and partial(first=-1) == ERR_ARG
    assert partial(theta=None) == ERR_ARG and partial(pert=None) == ERR_ARG and partial(f=None) == ERR_ARG and partial(out=None) == ERR_ARG
    assert apply(bstride=2 * stride + 2) == ERR_ARG and apply(bstride=-4) == ERR_ARG
    assert apply(cpb=0) == ERR_ARG and apply(chunks=0) == ERR_ARG and apply(n=0) == ERR_ARG
    assert apply(theta=None) == ERR_ARG and apply(p=None) == ERR_ARG and apply(s=None) == ERR_ARG
    for bad in (dict(C=0), dict(C=7), dict(n_act=0), dict(n_act=33)):
        assert partial(**bad) == ERR_ARG and apply(**bad) == ERR_ARG, bad
    torch.cuda.synchronize()
    assert is_sent(ts.rows()) and is_sent(ps.rows()) and parts.untouched()


# ------------------------------------------------------------------------------------------- 4. the synthetic env
POISON = 0xA5


class SynthDevice:
    """game state (77 everywhere), accumulators (5.5) and frame rows (0xA5) between guards"""

    def __init__(self, G, n_rows, C):
        self.G, self.nbytes = G, 84 * 84 * C
        self.gs, self.acc = Words(4 * G, torch.int32, fill=77), Words(3 * G, torch.float64, fill=5.5)
        self.frames = torch.full((n_rows + 2, self.nbytes), POISON, dtype=torch.uint8, device=DEV)
        self.frames_p = self.frames[1:].data_ptr()

    def read(self):
        f = self.frames.cpu().numpy()
        assert (f[0] == POISON).all() and (f[-1] == POISON).all(), "a guard frame row was written"
        return self.gs.get().reshape(self.G, 4), self.acc.get().reshape(self.G, 3), f[1:-1]


@pytest.mark.parametrize("C,n_act,per_gen", [(1, 5, 3), (4, 18, 4), (1, 18, 4), (4, 5, 3)])
def test_synth_steps_vs_plain_python(C, n_act, per_gen):
    """eight games stepped t = 0 ... 7 with scripted actions: ordinals 1, 2^32 + 5, 2^40 + 1, -1, two at -10 + 3 per_gen (-1:
    disabled, or 2), 0 and 2^31; limits 0, 1, 2, 5, 8; the frame rows permuted anew at every step"""
    G, R = len(dc.SYNTH_GAMES), dc.SYNTH_ROWS
    ord0, lim = dc.synth_ordinal0(per_gen), dc.synth_limits()
    d = SynthDevice(G, R, C)
    ref = dc.SynthRef(ord0, lim, dc.SYNTH_GEN, per_gen, C, n_act, dc.SYNTH_SEED, np.full((G, 4), 77), np.full((G, 3), 5.5))
    d_ord0, d_lim, d_gen = dev(ord0), dev(lim), dev(np.array([dc.SYNTH_GEN], dtype=np.int32))
    booked = 0
    for t in range(dc.SYNTH_T):
        row_cur = dc.synth_rows(t)
        row_prev = dc.synth_rows(t - 1) if t else None
        actions = np.full(R, -9, dtype=np.int32)
        if t:
            for g in range(G):
                actions[row_prev[g]] = dc.synth_action(g, t - 1, ref.target(g, t - 1), n_act)
        want_frames = np.full((R, 84, 84, C), POISON, dtype=np.uint8)
        acc_before = ref.acc.copy()
        ref.step(t, row_prev, actions, row_cur, want_frames)
        booked += int((ref.acc != acc_before).any(axis=1).sum()) if t else 0
        d.frames.fill_(POISON)
        d_prev, d_act = (dev(row_prev), dev(actions)) if t else (None, None)
        d_cur = dev(row_cur)
        L.call("coevo_synth_step", d.gs.p, d.acc.p, G, L._p(d_ord0), L._p(d_gen), per_gen, t, L._p(d_lim), L._p(d_prev),
               L._p(d_act), L._p(d_cur), d.frames_p, C, n_act, dc.SYNTH_SEED)
        gs, acc, frames = d.read()
        assert np.array_equal(gs, ref.gstate), (t, gs.tolist(), ref.gstate.tolist())
        assert np.array_equal(acc.view(np.uint64), ref.acc.view(np.uint64)), (t, acc.tolist(), ref.acc.tolist())
        written = sorted(int(row_cur[g]) for g in range(G) if t < ref.lim[g])
        for r in range(R):
            assert np.array_equal(frames[r], want_frames[r].reshape(-1)), (t, r, r in written)
            assert (r in written) or (frames[r] == POISON).all()
        if t == 0:
            assert written and not ref.acc.any() and (ref.gstate[:, 0] == 0xFF).all()
    assert booked >= 6 and (ref.gstate[:, 2:] == 77).all()      # hits and misses moved the returns; the spare words stay


def test_synth_largest_step_and_refusals():
    C, n_act, t = 4, 18, 65535
    ord0, lim = np.array([7, 2 ** 33 + 1], dtype=np.int64), np.array([65536, 65535], dtype=np.int32)
    d = SynthDevice(2, 3, C)
    gs0 = np.array([[3, 1, 77, 77], [4, 0, 77, 77]], dtype=np.int32)
    d.gs.t.copy_(dev(gs0.reshape(-1)))
    ref = dc.SynthRef(ord0, lim, None, 0, C, n_act, dc.SYNTH_SEED, gs0, np.full((2, 3), 5.5))
    rows_prev, rows_cur = np.array([2, 0], dtype=np.int32), np.array([1, 2], dtype=np.int32)
    actions = np.array([ref.target(1, t - 1), -9, (ref.target(0, t - 1) + 1) % n_act], dtype=np.int32)     # game 1 hits, game 0 misses
    want_frames = np.full((3, 84, 84, C), POISON, dtype=np.uint8)
    ref.step(t, rows_prev, actions, rows_cur, want_frames)
    d_ord0, d_lim, d_prev, d_act, d_cur = dev(ord0), dev(lim), dev(rows_prev), dev(actions), dev(rows_cur)
    args = [d.gs.p, d.acc.p, 2, L._p(d_ord0), None, 0, t, L._p(d_lim), L._p(d_prev), L._p(d_act), L._p(d_cur), d.frames_p, C,
            n_act, dc.SYNTH_SEED]

    def refused(**kw):
        a = list(args)
        for k, v in kw.items():
            a[dict(t=6, limit=7, row_prev=8, actions=9, row_cur=10, n_games=2, C=12, n_act=13, ord0=3)[k]] = v
        return rc("coevo_synth_step", *a)
    assert refused(t=65536) == ERR_ARG and refused(t=-1) == ERR_ARG and refused(limit=None) == ERR_ARG
    assert refused(actions=None) == ERR_ARG and refused(row_prev=None) == ERR_ARG and refused(row_cur=None) == ERR_ARG
    assert refused(n_games=0) == ERR_ARG and refused(ord0=None) == ERR_ARG
    assert refused(C=0) == ERR_ARG and refused(C=7) == ERR_ARG and refused(n_act=0) == ERR_ARG and refused(n_act=33) == ERR_ARG
    torch.cuda.synchronize()
    gs, acc, frames = d.read()
    assert np.array_equal(gs, gs0) and (acc == 5.5).all() and (frames == POISON).all(), "a refused call wrote"
    L.call("coevo_synth_step", *args)
    gs, acc, frames = d.read()
    assert np.array_equal(gs, ref.gstate) and np.array_equal(acc.view(np.uint64), ref.acc.view(np.uint64))
    assert ref.acc[0].tolist() == [6.5, 5.5, 5.5] and ref.acc[1].tolist() == [4.5, 5.5, 5.5]     # step 65534 is actor 0's
    assert ref.gstate[:, :2].tolist() == [[int(actions[2]), 0], [int(actions[0]), 1]]
    assert np.array_equal(frames, want_frames.reshape(3, -1))
    # game 0 gets the frame of step 65535 in row 1; game 1 has reached its limit: booked, no frame
    assert (frames[1] != POISON).any() and (frames[0] == POISON).all() and (frames[2] == POISON).all()
