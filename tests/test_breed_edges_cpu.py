"""The references of tests/breed_cases.py proven on the CPU before tests/test_breed_edges_gpu.py judges a kernel by them: the
numpy restatements against the oracle's C code on the inputs the GPU suite uses, the oracle's Box-Muller against a float64
Box-Muller, and the cases against what they claim to hold.

Box-Muller, oracle (float32, fmaf-only polynomials) against sqrt(-2 ln u1) (cos, sin)(2 pi u2) in float64, measured here over
the edge set (2208 pairs: the extremes of u1, both sides of the 0.7071 mantissa threshold in every binade, the quadrant
edges, the f = 0.5 swap, u2 = 0) and a seeded sweep of 2^20 random pairs:
    max |z - z64|            5.83e-7 (edges)   5.86e-7 (sweep)
    max |z - z64| / ulp(z64) 2.44    (edges)   3.28    (sweep)
    max relative error       1.8e-7  (edges)   2.4e-7  (sweep)      - rounding, no wrong coefficient (that would be > 1e-5)
The test asserts twice the measured maxima (breed_cases.BM_MAX_ABS, BM_MAX_ULP)."""
import math

import numpy as np
import pytest

from oracle import ref_port as rp
from tests import breed_cases as bc

F32 = np.float32


# ------------------------------------------------------------------------------------------- the restatements agree
def test_noise_table_is_the_oracles_quads():
    P = bc.params(8)
    z = bc.normals(7, 199, 41, P)
    assert z.dtype == np.float32 and z.shape == (P,) and P % 4 == 1
    buf = np.zeros(4, dtype=np.float32)
    for q in (0, 1, 1000, P // 4):      # the last quad holds one element
        rp.lib().oracle_philox_normal4(7, 199, 41, q, rp._fp(buf))
        assert bc.same_bits(z[4 * q:4 * q + 4], buf[:len(z[4 * q:4 * q + 4])])
    w = rp.philox_normals(7, 199, 41, 2 ** 32 - 2, 4)   # the quad counter wraps
    for i, q in enumerate((2 ** 32 - 2, 2 ** 32 - 1, 0, 1)):
        rp.lib().oracle_philox_normal4(7, 199, 41, q, rp._fp(buf))
        assert bc.same_bits(w[i], buf)


@pytest.mark.parametrize("name", list(bc.perturb_cases()))
def test_child_restatement_equals_oracle_perturb(name):
    c = bc.perturb_cases()[name]
    D = c["D"]
    parents = bc.planted_parents(D, bc.N_PARENTS)
    want = bc.perturb_want(c, parents)
    shi = (c["shi"] + 4 * (c["gen"] or 0)) & bc.M32
    for k, p in enumerate(c["pidx"]):
        slo, neg = bc.stream_of(c["slo_first"] + k, c["flags"])
        ref = rp.mutate_philox(parents[p], D, c["sigma"], bc.SEED, slo, shi, skip_layernorm=bool(c["flags"] & 1), negate=neg)
        assert bc.same_f32(want[k], ref), (name, k, bc.first_diff(want[k], ref))
        if c["flags"] & 1:   # LayerNorm keeps the parent's bits, NaN payloads included
            assert bc.same_bits(want[k][bc.ln_mask(D)], parents[p][bc.ln_mask(D)])


def test_sigma_sweep_reaches_subnormal_and_infinite_noise():
    """the reference alone: sigma 1e-41 gives subnormal noise, 3e38 overflows to +-inf, inf * z and NaN * z as IEEE has them"""
    P = bc.params(10)
    tiny = bc.noise(F32(1e-41), bc.SEED, 1000, 7, 0, P)
    assert np.count_nonzero((tiny != 0) & (np.abs(tiny) < np.finfo(np.float32).tiny)) > 1000
    big = bc.noise(F32(3e38), bc.SEED, 1000, 7, 0, P)
    assert np.isinf(big).any() and (big == np.inf).any() and (big == -np.inf).any() and np.isfinite(big).any()
    assert np.isinf(bc.noise(F32(np.inf), bc.SEED, 1000, 7, 0, P)).sum() > P - 8
    assert np.isnan(bc.noise(F32(np.nan), bc.SEED, 1000, 7, 0, P)).all()
    assert not bc.noise(F32(0.0), bc.SEED, 1000, 7, 0, P).any()
    a, b = bc.noise(F32(0.05), bc.SEED, 10, 7, 2, P), bc.noise(F32(0.05), bc.SEED, 11, 7, 2, P)
    assert bc.same_bits(a, -b) and np.abs(a).max() > 0.1      # an antithetic pair


def test_rebuild_rule_is_the_materialised_child():
    D, E = 8, 3
    old = bc.planted_parents(D, E)
    for ident, gen in ((0, None), (1, None), (4, 3), (9, 1)):
        got = bc.rebuilt_elite(old, D, ident, F32(0.05), 77, 5, gen)
        if ident == 0:
            assert bc.same_bits(got, old[0])
            continue
        c = ident - 1
        shi = (5 + (4 * (gen - 1) if gen is not None else 0)) & bc.M32
        assert bc.same_f32(got, rp.mutate_philox(old[c % E], D, F32(0.05), 77, c, shi))


def test_promote_list_operations():
    pop, hof, elite = list("abcde"), list("xyz"), list("pq")
    assert bc.promote(pop, hof, elite, [3, 0], 2, True, True) == (list("dbcde"), list("yzd"), list("da"))
    assert bc.promote(pop, hof, elite, None, 2, False, False) == (pop, list("yzp"), elite)
    assert bc.promote(pop, ["x"], elite, [4, 4], 2, True, False) == (pop, ["e"], ["e", "e"])


@pytest.mark.parametrize("D,n,chunks,kind,sigma,lr", bc.es_cases())
def test_es_restatement_equals_oracle_update(D, n, chunks, kind, sigma, lr):
    theta, pert, fit = bc.es_inputs(D, n, float(sigma), kind)
    got, unsafe, ref64, bound = bc.es_update(theta, pert, fit, D, sigma, lr, chunks)
    assert unsafe == 0, "an emulated fma term that is not provably the fused result: choose another seed"
    for ch in sorted({chunks, 1, 3, 8}):
        mine = got if ch == chunks else bc.es_update(theta, pert, fit, D, sigma, lr, ch)[0]
        with np.errstate(over="ignore"):
            ref = rp.es_update_from_pert(theta, D, pert, fit, sigma, lr, chunks=ch)
        assert bc.same_f32(mine, ref), (ch, bc.first_diff(mine, ref))
    keep = bc.ln_mask(D)
    assert bc.same_bits(got[keep], theta[keep])
    if kind == "random" and sigma == bc.ES_SIGMAS[0]:
        fin = np.isfinite(ref64)
        assert fin.all() and (np.abs(got[fin] - ref64[fin]) <= bound[fin]).all()
        assert (got != theta)[~keep].mean() > 0.9      # it moved
    if kind == "zeros":
        assert bc.same_f32(got[~keep], (theta + F32(0.0)).astype(np.float32)[~keep])   # (-0 becomes +0: theta + 0)
    if kind in ("one_inf", "one_nan"):
        assert np.isnan(got[~keep]).any()
    if sigma == bc.ES_SIGMAS[1]:
        with np.errstate(over="ignore"):
            scale = F32(lr) / (F32(n) * sigma)
        assert 0 < F32(n) * sigma < np.finfo(np.float32).tiny * 64 and scale > 1e35
        assert np.isinf(scale) == (lr == bc.ES_LR_BIG)        # the scale overflows


def test_es_emulated_fma_matches_c_fmaf_on_rounding_ties():
    """the emulation against the oracle's fmaf on terms built to land half way between two float32 (where double rounding
    would show): exact ties must agree, inexact ones are counted as unsafe"""
    x = F32(1 + 2.0 ** -12)                       # x * x = 1 + 2^-11 + 2^-24: half way between two float32
    f = np.array([1.0, x], dtype=np.float32)
    # col 0: acc = 0, the tie is exact (to even: 1 + 2^-11); col 1: acc = 2^-80 is a sticky bit a real fma rounds up on
    d = np.array([[0.0, 2.0 ** -80], [x, x]], dtype=np.float32)
    P = bc.params(8)
    th = np.zeros(P, dtype=np.float32)
    pert = np.zeros((2, P), dtype=np.float32)
    pert[:, :2] = d
    ref = rp.es_update_from_pert(th, 8, pert, f, 0.5, 1.0, chunks=1)     # theta = 0, scale = 1 (lr = n * sigma)
    mine, unsafe, _, _ = bc.es_update(th, pert, f, 8, 0.5, 1.0, 1)
    assert ref[0] == F32(1 + 2.0 ** -11) and ref[1] == F32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert mine[0] == ref[0] and unsafe == 1      # the one term the emulation cannot vouch for is the one it gets wrong
    assert mine[1] != ref[1] and bc.same_bits(mine[2:], ref[2:])


# ------------------------------------------------------------------------------------------- Box-Muller against float64
def _bm_check(a, b):
    z = rp.box_muller(a, b)
    z64 = bc.box_muller64(a, b)
    assert np.isfinite(z).all()                      # never NaN from a negative radicand, never inf
    lim = F32(math.sqrt(-2.0 * math.log(2.0 ** -24)))
    assert np.abs(z).max() <= np.nextafter(lim, F32(np.inf))
    k = (b.astype(np.int64) >> 8)
    q, rem = k >> 22, k & (2 ** 22 - 1)
    # signs per quadrant (cos, sin): (+,+) (-,+) (-,-) (+,-); on an edge one of the two is a signed zero
    cs, ss = np.array([1, -1, -1, 1])[q], np.array([1, 1, -1, -1])[q]
    inside = rem != 0
    assert (np.sign(z[inside, 0]) == cs[inside]).all() and (np.sign(z[inside, 1]) == ss[inside]).all()
    edge = ~inside
    zero_col = np.where(q[edge] % 2 == 0, 1, 0)      # sin is 0 at u2 = 0, 1/2; cos at 1/4, 3/4
    rows = np.flatnonzero(edge)
    assert (z[rows, zero_col] == 0).all() and (z[rows, 1 - zero_col] != 0).all()
    sin0 = edge & (q % 2 == 0)
    assert (z[sin0, 1] == 0).all() and (z[~sin0, 1] != 0).all()          # z1 = +-0 exactly where sin is 0
    err = np.abs(z.astype(np.float64) - z64)
    ulp = np.spacing(np.abs(z64).astype(np.float32)).astype(np.float64)
    nz = z64 != 0
    rel = (err[nz] / np.abs(z64[nz])).max()
    return err.max(), (err / ulp).max(), rel


def test_box_muller_edges_and_sweep_vs_float64():
    a, b = bc.box_muller_edges()
    ms, ks = set((a >> 9).tolist()), set((b >> 8).tolist())
    assert {0, 1, 2, 2 ** 22 - 1, 2 ** 22, 2 ** 23 - 2, 2 ** 23 - 1} <= ms and {0, 2 ** 24 - 1, 2 ** 21, 2 ** 21 + 1} <= ks
    # both sides of the 0.7071 mantissa threshold in every binade that has two odd numerators around it
    sides = {}
    for m in bc.log_threshold_mantissas():
        mant, e = math.frexp((2 * m + 1) * 2.0 ** -24)
        sides.setdefault(e, set()).add(mant < math.sqrt(0.5))
    assert all(s == {True, False} for e, s in sides.items() if e >= -20) and min(sides) <= -22 and max(sides) == 0
    e_abs, e_ulp, e_rel = _bm_check(a, b)
    s_abs, s_ulp, s_rel = _bm_check(*bc.box_muller_sweep())
    print("box-muller vs float64: edges abs %.3g ulp %.3g rel %.3g; sweep abs %.3g ulp %.3g rel %.3g"
          % (e_abs, e_ulp, e_rel, s_abs, s_ulp, s_rel))
    assert max(e_rel, s_rel) < 1e-5, "a wrong polynomial coefficient, not rounding"
    assert max(e_abs, s_abs) <= 2 * bc.BM_MAX_ABS and max(e_ulp, s_ulp) <= 2 * bc.BM_MAX_ULP


def test_box_muller_single_call_equals_bulk():
    a, b = bc.box_muller_edges()
    bulk = rp.box_muller(a[:50], b[:50])
    for i in range(50):
        assert bc.same_bits(rp.box_muller(a[i:i + 1], b[i:i + 1])[0], bulk[i])


# ------------------------------------------------------------------------------------------- the cases hold what they claim
@pytest.mark.parametrize("D", [8, 10])
def test_planted_positions_are_the_segment_edges(D):
    P = bc.params(D)
    assert P == {8: 138757, 10: 139781}[D] and bc.stride(D) % 64 == 0 and 0 < bc.stride(D) - P < 64
    pos = set(bc.plant_positions(D))
    segs = bc.segments(D)
    assert len(segs) == 10 and segs[-1][0] + segs[-1][1] == P
    assert sorted(rp.ln_segments(D) + rp.linear_segments(D)) == segs
    for o, n in segs:
        assert {o, o + n - 1} <= pos
        if o:
            assert set(range(o - 4, o + 4)) <= pos
    assert P - 1 in pos and (P - 1) % 4 == 0        # the last quad holds one element
    nets = bc.planted_parents(D, bc.N_PARENTS)
    assert np.isfinite(nets[0]).all() and np.isnan(nets[1]).any() and np.isinf(nets[2]).any()
    for k in range(bc.N_PARENTS):
        vals = nets[k][sorted(pos)]
        want = bc.FINITE_PLANTS if k == 0 else bc.ALL_PLANTS
        assert {v.view(np.uint32).item() for v in vals} == {F32(v).view(np.uint32).item() for v in want}
    # planted values fall on LayerNorm and on Linear entries, and on re-tiled and plain slab positions
    ln = bc.ln_mask(D)
    assert ln[sorted(pos)].any() and (~ln[sorted(pos)]).any()
    m = bc.slab_to_flat(D)
    assert sorted(m[m >= 0].tolist()) == list(range(P)) and (m[P:] == -1).all()
    assert m[3 * 512 + 77] == 77 * D + 3
    o_w2 = D * 512 + 1536
    assert m[o_w2 + ((2 * 128 + 17) * 64 + 5) * 4 + 3] == o_w2 + (2 * 64 + 5) * 512 + 17 * 4 + 3


def test_wrap_cases_cross_two_to_the_32():
    cases = bc.perturb_cases()
    for flags in range(4):
        c = cases[f"wrap_flags{flags}"]
        inds = [c["slo_first"] + k for k in range(len(c["pidx"]))]
        assert inds[0] < 2 ** 32 <= inds[-1]
        streams = [bc.stream_of(i, flags) for i in inds]
        if flags & 2:
            assert streams == [(2 ** 31 - 1, False), (2 ** 31 - 1, True), (0, False), (0, True)]
        else:
            assert streams == [(2 ** 32 - 2, False), (2 ** 32 - 1, False), (0, False), (1, False)]
    for j, g in enumerate(bc.GENS):
        c = cases[f"gen{j}"]
        assert (c["shi"] + 4 * g >= 2 ** 32) == (g != 0)
    assert (4 * bc.GENS[-1]) & bc.M32 == 0
    assert {c["flags"] for c in cases.values()} == {0, 1, 2, 3} and {c["D"] for c in cases.values()} == {8, 10}


def test_es_cases_cover_the_sixteen_boundary():
    ns = {n for _, n, ch, *_ in bc.es_cases() if ch == 1}
    assert {1, 15, 16, 17, 32, 33} <= ns
    assert bc.es_chunk_bounds(50, 3) == [(0, 16), (16, 33), (33, 50)]
    assert sum(lo == hi for lo, hi in bc.es_chunk_bounds(5, 8)) == 3
    assert max(hi - lo for lo, hi in bc.es_chunk_bounds(33, 64)) == 1
    assert {k for _, _, _, k, *_ in bc.es_cases()} == set(bc.ES_FITNESS) and {D for D, *_ in bc.es_cases()} == {8, 10}
    f = bc.es_fitness("neg_zero", 33)
    assert np.signbit(f[0]) and f[0] == 0


def test_dist_partials_reference():
    D = 10
    nets = bc.plain_nets(D, 2, 1)
    p = bc.dist_partials(nets[0], nets[1], D)
    assert p.shape == (bc.n_blocks(D),) == (137,)
    lin = ~bc.ln_mask(D)
    d = (nets[0] - nets[1]).astype(np.float32)[lin].astype(np.float64)
    assert math.isclose(math.fsum(p.tolist()), math.fsum((d * d).tolist()), rel_tol=1e-15)
    assert not bc.dist_partials(nets[0], nets[0], D).any()
    hot = nets[1].copy()
    hot[bc.segments(D)[4][0] + 70001] = np.inf
    ph = bc.dist_partials(nets[0], hot, D)
    assert np.isinf(ph).sum() == 1 and bc.same_partials(ph, ph) and not bc.same_partials(p, ph)
    assert bc.within_one_ulp(bc.final_distance(p), F32(np.linalg.norm(d)))
