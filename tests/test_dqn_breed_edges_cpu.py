"""The references of tests/dqn_breed_cases.py proven on the CPU before tests/test_dqn_breed_edges_gpu.py judges a kernel by
them: the numpy slab map against what csrc/dqn_common.hip.h promises of it, the child and ES restatements against the oracle's
C code (oracle_perturb_philox, oracle_es_update_from_pert with the BatchNorm segments) on the very inputs the GPU file uses,
the plain-Python env against oracle_dqn_play_game, and the cases against what they claim to hold."""
import math

import numpy as np
import pytest

from oracle import ref_port as rp
from tests import breed_cases as bc
from tests import dqn_breed_cases as dc

F32 = np.float32


# ------------------------------------------------------------------------------------------- the slab map
@pytest.mark.parametrize("C,n", dc.SHAPES)
def test_slab_map_is_a_bijection_with_the_batchnorm_words_in_three_ranges(C, n):
    L, P = dc.layout(C, n), dc.params(C, n)
    assert P == rp.lib().oracle_dqn_param_count(C, n) == L.total and L.stride % 64 == 0 and 0 <= L.stride - L.total < 64
    (o_bn, n_bn), = rp.dqn_bn_segments(C, n)
    assert (o_bn, n_bn) == (dc.segments(C, n)[10][0], 320) and dc.bn_mask(C, n).sum() == 320
    maps = [dc.slab_to_flat(C, n, t) for t in dc.LAYOUTS]
    for m in maps:
        assert m.shape == (L.stride,) and (m[L.total:] == -1).all() and (m[:L.total] >= 0).all()
        assert np.array_equal(np.sort(m[:L.total]), np.arange(P))                 # onto [0, P), each index once
        assert sorted(m[dc.bn_slab_mask(C, n)].tolist()) == list(range(o_bn, o_bn + n_bn))
        assert dc.bn_slab_mask(C, n).sum() == 320
        assert np.array_equal(dc.from_slab_row(dc.to_slab_rows(np.arange(P), C, n, 0, -1.0), C, n, 0), np.arange(P))
    differs = np.flatnonzero(maps[0] != maps[1])
    assert len(differs) and differs.min() >= L.wf and differs.max() < L.bf           # tiled moves fc1 words only
    o_fc1, n_fc1 = dc.segments(C, n)[6]
    for m in maps:
        assert m[L.wf:L.bf].min() == o_fc1 and m[L.wf:L.bf].max() == o_fc1 + n_fc1 - 1
    # entries worked out by hand from the layout comments
    s, t = maps
    assert s[0] == 0 and s[4 * 17 + 3] == (16 + 1) * (64 * C) + 4 * 1 + 1      # conv1: lane 17, e 3: co 16 + 1, tap 4 * 1 + 1
    o_w2 = dc.segments(C, n)[2][0]
    assert s[L.w2 + ((3 * 2 + 1) * 64 + 35) * 4 + 2] == o_w2 + (32 + 3) * 512 + 4 * (2 * 3 + 1) + 2   # qp 3, np 1, lane 35, e 2
    assert s[L.wf + ((2 * 784 + 9) * 64 + 5) * 4 + 3] == o_fc1 + (128 + 5) * 3136 + 39               # ob 2, kq 9, l 5, c 3
    assert t[L.wf + (((1 * 196 + 7) * 4 + 2) * 64 + 37) * 4 + 1] == o_fc1 + (64 + 32 + 5) * 3136 + 16 * 7 + 4 + 2
    assert s[L.b1 + 31] == dc.segments(C, n)[1][0] + 31 and s[L.b1 + 32] == o_bn and s[L.w2 - 1] == o_bn + 63
    assert s[L.b3 + 64] == o_bn + 192 and s[L.wf - 1] == P - 1 and s[L.total - 1] == o_bn - 1


def test_shapes_are_the_edges_they_claim():
    tot = [dc.layout(C, n).total for C, n in dc.SHAPES]
    assert [x % 4 for x in tot] == [1, 1, 3, 0]            # = (P - 320) % 4: how the BatchNorm / bias Philox blocks straddle quads
    assert [dc.stride(C, n) - x for (C, n), x in zip(dc.SHAPES, tot)] == [31, 27, 29, 0]
    assert tot[1] % 8 == 5                                 # a full quad of live words, then one live word and three padding
    for C, n in dc.SHAPES:
        L = dc.layout(C, n)
        sh = dc.shift(C, n, dc.TILED)
        assert (L.wf // 4 + sh) % 64 == 0 and 0 < sh < 64 and dc.shift(C, n, 0) == 0
        assert dc.n_blocks(C, n, 0) == (L.stride + 1023) // 1024 and dc.n_blocks(C, n, dc.TILED) >= dc.n_blocks(C, n, 0)
    # the slab's triples start on quads, their canonical tensors at these offsets inside a Philox block
    assert all(dc.layout(C, n).b1 % 4 == 0 and dc.layout(C, n).bo % 4 == 0 for C, n in dc.SHAPES)
    assert [dc.segments(C, n)[10][0] % 4 for C, n in dc.SHAPES] == [1, 1, 3, 0]


@pytest.mark.parametrize("C,n", dc.SHAPES)
def test_planted_positions_are_the_tensor_and_range_edges(C, n):
    P, pos = dc.params(C, n), set(dc.plant_positions(C, n))
    segs = dc.segments(C, n)
    assert len(segs) == 16 and segs[-1][0] + segs[-1][1] == P
    for o, s in segs:
        assert {o, o + s - 1} <= pos
        if o:
            assert set(range(max(o - 4, 0), o + 4)) <= pos
    L = dc.layout(C, n)
    for tiled in dc.LAYOUTS:
        m = dc.slab_to_flat(C, n, tiled)
        assert {int(m[L.wf]), int(m[L.bf - 1])} <= pos
        for lo, hi in dc.bn_slab_ranges(C, n):
            assert {int(m[lo - 1]), int(m[lo]), int(m[hi - 1]), int(m[hi])} <= pos
    nets = dc.planted_parents(C, n)
    assert nets.shape == (3, P) and np.isfinite(nets[0]).all() and np.isnan(nets[1]).any() and np.isinf(nets[2]).any()
    for k in range(dc.N_PARENTS):
        got = {v.view(np.uint32).item() for v in nets[k][sorted(pos)]}
        want = {F32(v).view(np.uint32).item() for v in (bc.FINITE_PLANTS if k == 0 else bc.ALL_PLANTS)}
        assert got == want
        edge = nets[k][dc.bn_edge_positions(C, n)]
        assert (np.abs(edge) < np.finfo(np.float32).tiny).all()          # +-0 or subnormal: any noise moves them
    bn = dc.bn_mask(C, n)
    assert bn[sorted(pos)].any() and (~bn[sorted(pos)]).any()


# ------------------------------------------------------------------------------------------- perturb
def test_perturb_cases_cover_what_they_claim():
    cases = dc.perturb_cases()
    combos = {}
    for name, c in cases.items():
        if name.startswith("sigma"):
            combos.setdefault((c["shape"], c["tiled"]), []).append((int(name[5]), c["flags"]))
    assert set(combos) == set(dc.PAIRS) and all(len(v) >= 3 for v in combos.values())
    assert sorted(x for v in combos.values() for x in v) == [(i, f) for i in range(6) for f in range(4)]
    assert all(len({f for _, f in v}) == 3 for v in combos.values())
    for t in dc.LAYOUTS:       # each layout meets every sigma
        assert {i for (s, tt), v in combos.items() if tt == t for i, _ in v} == set(range(6))
    for group, count in (("wrap", 8), ("gen", 16)):
        sub = [c for name, c in cases.items() if name.startswith(group)]
        assert len(sub) == count and {c["tiled"] for c in sub} == set(dc.LAYOUTS) and {c["shape"] for c in sub} == set(dc.SHAPES)
        assert {c["flags"] for c in sub} == {0, 1, 2, 3}
    for name, c in cases.items():
        assert 4 <= len(c["pidx"]) <= 5 and len(set(c["pidx"])) < len(c["pidx"]) and list(c["pidx"]) != sorted(c["pidx"])
        if name.startswith("wrap"):
            inds = [c["slo_first"] + k for k in range(len(c["pidx"]))]
            assert inds[0] < 2 ** 32 <= inds[-1]
        if name.startswith("gen"):
            assert c["shi"] == 2 ** 32 - 3 and c["gen"] in bc.GENS and c["gen_bias"] in (0, -1)
    assert {(c["gen"], c["gen_bias"]) for n_, c in cases.items() if n_.startswith("gen")} == {(g, b) for g in bc.GENS for b in (0, -1)}
    for E, order in dc.ORDERS.items():
        assert 0 in order and {(i - 1) % E for i in order if i} == set(range(E)) and max(order) >= E + 1
        assert 4 <= len(order) <= 5


OTHER_CHILDREN = {f"dist_C{C}n{n}_flags{f}": dc.plain_case((C, n), 0, f, dc.DIST_PIDX) for C, n in dc.SHAPES for f in (0, 1)}
OTHER_CHILDREN.update({f"in_place_C{C}n{n}_flags{f}": dc.plain_case((C, n), t, f, (2, 0, 2, 1)) for C, n, t, f in dc.IN_PLACE})


@pytest.mark.parametrize("name", list(dc.perturb_cases()) + list(OTHER_CHILDREN))
def test_child_restatement_equals_oracle_perturb(name):
    """every case of test_perturb_every_word, and the children of the distance and in-place tests (the same in both layouts)"""
    c = dc.perturb_cases().get(name) or OTHER_CHILDREN[name]
    C, n = c["shape"]
    parents, want = dc.planted_parents(C, n), dc.perturb_want(c)
    shi = (c["shi"] + (4 * (c["gen"] + c["gen_bias"]) if c["gen"] is not None else 0)) & bc.M32
    bn = rp.dqn_bn_segments(C, n)
    for k, p in enumerate(c["pidx"]):
        slo, neg = bc.stream_of(c["slo_first"] + k, c["flags"])
        ref = rp.perturb_philox_flat(parents[p], c["sigma"], dc.SEED, slo, shi, bn if c["flags"] & 1 else (), negate=neg)
        assert bc.same_f32(want[k], ref), (name, k, bc.first_diff(want[k], ref))
        if c["flags"] & 1:   # BatchNorm keeps the parent's bits, NaN payloads included
            assert bc.same_bits(want[k][dc.bn_mask(C, n)], parents[p][dc.bn_mask(C, n)])
    if c["sigma"] == bc.SIGMAS[1]:      # 1e-41: every noise word subnormal or zero, and the children differ from the parents
        nz = bc.noise(c["sigma"], dc.SEED, c["slo_first"], shi, c["flags"], dc.params(C, n))
        assert (np.abs(nz) < np.finfo(np.float32).tiny).all() and np.count_nonzero(nz) > 1000
        small = np.abs(parents[c["pidx"][0]]) < 1e-37
        assert (want[0][small] != parents[c["pidx"][0]][small]).any()


@pytest.mark.parametrize("E", [1, 2, 3])
def test_order_rule_is_the_materialised_child(E):
    C, n = dc.SHAPES[E % 4]
    parents = dc.planted_parents(C, n)
    for with_gen in (False, True):
        want = dc.order_want(C, n, E, with_gen)
        shi = (dc.ORDER_SHI + (4 * (dc.ORDER_GEN + dc.ORDER_GEN_BIAS) if with_gen else 0)) & bc.M32
        for k, ident in enumerate(dc.ORDERS[E]):
            ref = parents[0] if ident == 0 else rp.perturb_philox_flat(parents[(ident - 1) % E], F32(0.05), dc.SEED, ident - 1, shi)
            assert bc.same_f32(want[k], ref) and (ident != 0 or bc.same_bits(want[k], ref))


# ------------------------------------------------------------------------------------------- distance
@pytest.mark.parametrize("tiled", dc.LAYOUTS)
def test_dist_partials_reference(tiled):
    C, n = 3, 5
    a, b = dc.plain_net(C, n, 1), dc.plain_net(C, n, 2)
    p = dc.dist_partials(a, b, C, n, tiled)
    assert p.shape == (dc.n_blocks(C, n, tiled),)
    d = (a - b).astype(np.float32).astype(np.float64)
    assert math.isclose(math.fsum(p.tolist()), math.fsum((d * d).tolist()), rel_tol=1e-15)     # every live word once, BatchNorm too
    assert not dc.dist_partials(a, a, C, n, tiled).any()
    # one hot word lands in the block the shifted thread map gives it
    L, m = dc.layout(C, n), dc.slab_to_flat(C, n, tiled)
    for s in (0, L.wf - 1, L.wf, L.total - 1):
        hot = np.array(b, copy=True)
        hot[m[s]] = np.inf
        ph = dc.dist_partials(a, hot, C, n, tiled)
        assert np.flatnonzero(np.isinf(ph)).tolist() == [(s // 4 + dc.shift(C, n, tiled)) // 256]
    if tiled:
        assert p[0] < dc.dist_partials(a, b, C, n, 0)[0]       # block 0 holds 256 - shift quads only
    ref, pad = dc.dist_ref(C, n, "inf")
    assert np.isinf(ref).sum() == 3 and np.isfinite(pad) and np.isnan(dc.dist_ref(C, n, "unrelated")[1])


# ------------------------------------------------------------------------------------------- the ES update
def _es_unique():
    seen, out = set(), []
    for shape, n, chunks, kind, sigma, lr, _ in dc.es_cases():
        key = (shape, n, chunks, kind, float(sigma), float(lr))
        if key not in seen:
            seen.add(key)
            out.append((shape, n, chunks, kind, sigma, lr))
    return out


@pytest.mark.parametrize("shape,n,chunks,kind,sigma,lr", _es_unique(), ids=[dc.es_id(c + ("update",)) for c in _es_unique()])
def test_es_restatement_equals_oracle_update(shape, n, chunks, kind, sigma, lr):
    C, n_act = shape
    theta, fit, got, unsafe, ref64, bound = dc.es_want(shape, n, chunks, kind, sigma, lr)
    pert = dc.es_inputs(shape, n, float(sigma))[1]
    assert unsafe == 0, "an emulated fma term that is not provably the fused result: choose another seed"
    with np.errstate(over="ignore"):
        ref = rp.dqn_es_update_from_pert(theta, pert, fit, sigma, lr, C, n_act, chunks=chunks)
    assert bc.same_f32(got, ref), bc.first_diff(got, ref)
    keep = dc.bn_mask(C, n_act)
    assert bc.same_bits(got[keep], theta[keep])
    assert (pert[:, keep] != theta[keep]).mean() > 0.9 or sigma != dc.ES_SIGMAS[0]      # the skip has teeth
    edge = np.array(dc.bn_edge_positions(C, n_act))
    if sigma == dc.ES_SIGMAS[0]:
        assert (pert[0, edge] != theta[edge]).all()           # both sides of every range boundary differ in the perturbed net
        if kind != "one_nan":
            assert (got[edge] != theta[edge]).tolist() == [True, False, False, True] * 3    # outside moves, inside stays
    if kind == "random" and sigma == dc.ES_SIGMAS[0]:
        assert np.isfinite(ref64).all() and (np.abs(got - ref64) <= bound).all()
        assert (got != theta)[~keep].mean() > 0.9
    if kind == "one_nan":
        assert np.isnan(got[~keep]).all()
    if sigma == dc.ES_SIGMAS[1]:
        with np.errstate(over="ignore"):
            scale = F32(lr) / (F32(n) * sigma)
        assert scale > 1e35 and np.isinf(scale) == (lr == bc.ES_LR_BIG)


def test_es_cases_cover_the_sixteen_boundary_and_both_shapes():
    cases = dc.es_cases()
    assert {n for _, n, ch, *_ in cases if ch == 1} >= {1, 16, 17, 33}
    assert {(n, ch) for _, n, ch, *_ in cases if ch > 1} == {(33, 3), (5, 8), (33, 64)}
    assert {f for *_, f in cases} == {"one", "two_launch", "two_block"} and {s for s, *_ in cases} == set(dc.ES_SHAPES)
    assert {k for _, _, _, k, *_ in cases} == {"random", "one_nan", "alt_flt_max"}
    for shape in dc.ES_SHAPES:       # each shape: the 16-deep loop entered, and a chunked sum
        assert any(s == shape and n >= 16 and ch == 1 for s, n, ch, *_ in cases) and any(s == shape and ch > 1 for s, _, ch, *_ in cases)
    assert bc.es_chunk_bounds(33, 3) == [(0, 11), (11, 22), (22, 33)]
    assert sum(lo == hi for lo, hi in bc.es_chunk_bounds(5, 8)) == 3 and max(hi - lo for lo, hi in bc.es_chunk_bounds(33, 64)) == 1
    assert np.isnan(dc.es_pert_padding(dc.ES_PERT_NAN)) and np.isfinite(dc.es_pert_padding(0))
    assert len({dc.es_id(c) for c in cases}) == len(cases)


# ------------------------------------------------------------------------------------------- the synthetic env
def test_synth_reference_books_what_the_oracle_game_returns():
    """the scripted reference fed with the actions of oracle_dqn_play_game: the same returns, and the frames the game's nets saw"""
    C, n_act, seed = 1, 5, dc.SYNTH_SEED
    a, b = dc.plain_net(C, n_act, 3), dc.plain_net(C, n_act, 4)
    for ordinal, limit in ((1, 5), (2 ** 32 + 5, 2), (2 ** 40 + 1, 1)):
        game = rp.dqn_play_game(a, b, C, n_act, seed, ordinal, limit)
        assert game["steps"] == limit
        ref = dc.SynthRef([ordinal], [limit], None, 0, C, n_act, seed, [[7, 7, 7, 7]], [[5.5, 5.5, 5.5]])
        frames = np.full((2, 84, 84, C), 0xA5, dtype=np.uint8)
        actions = np.zeros(2, dtype=np.int32)
        for t in range(limit + 2):
            if 1 <= t <= limit:
                actions[(t - 1) & 1] = game["actions"][t - 1]
            ref.step(t, [(t - 1) & 1], actions, [t & 1], frames)
            if t < limit:      # the frame the oracle's net acts on at step t gives the oracle's action
                net = b if t & 1 else a
                assert rp.dqn_forward(net, C, n_act, frames[t & 1])[0] == game["actions"][t]
        assert ref.acc[0].tolist() == [game["rewards"][0], game["rewards"][1], 0.0]
        assert ref.gstate[0].tolist() == [game["actions"][-1], ref.gstate[0, 1], 7, 7]


def test_synth_cases_hit_and_miss_and_cover_the_limits():
    assert len(dc.SYNTH_GAMES) == 8 and {l for _, l in dc.SYNTH_GAMES} == {0, 1, 2, 5, 8}
    assert {o for o, _ in dc.SYNTH_GAMES} >= {1, 2 ** 32 + 5, 2 ** 40 + 1, -1, None}
    assert dc.synth_ordinal0(3)[4] + 3 * dc.SYNTH_GEN == -1 and dc.synth_ordinal0(4)[4] + 4 * dc.SYNTH_GEN == 2
    for t in range(1, dc.SYNTH_T):
        r0, r1 = dc.synth_rows(t - 1), dc.synth_rows(t)
        assert len(set(r1.tolist())) == 8 and (r0 != r1).all() and r1.max() < dc.SYNTH_ROWS
    for per_gen, n_act in ((3, 5), (4, 18)):
        ref = dc.SynthRef(dc.synth_ordinal0(per_gen), dc.synth_limits(), dc.SYNTH_GEN, per_gen, 1, n_act, dc.SYNTH_SEED,
                          np.zeros((8, 4)), np.zeros((8, 3)))
        assert (ref.lim[4] == 0) == (per_gen == 3) and ref.lim[3] == 0 and ref.ordinal[1] == 2 ** 32 + 5
        for g in range(8):
            if ref.lim[g] >= 2:
                hits = [dc.synth_action(g, t, ref.target(g, t), n_act) == ref.target(g, t) for t in range(ref.lim[g])]
                assert any(hits) and not all(hits), (g, hits)
