"""The float16 twin of tests/sharing_cases.py: the all-pairs distance of fp16-valued nets (include/coevo_sharing16.h) as a numpy
statement, its inputs, and the Co-GA generation of HalfGAEngine under the extension modes hof_mean / population_sharing
restated on the CPU (tests/ga16_checker.py's games and breeding, sharing_cases' fitness and niche counts).  No GPU needed here.

The float16 distance contract (DESIGN.md "float16 nets"): per Linear entry d = f16(f32(a) - f32(b)), d * d summed in fp64,
dist = f16(sqrt(sum)) rounded once.  The device adds its fp64 terms in an order of its own, so, as in sharing_cases, a finite
input is *order-proof*: the worst-case interval of the sum under any order rounds, after the root, to one fp16 word.  The
drawn nets are sharing_cases.nets(D) rounded with ga16_checker.round_linear, redrawn (sharing_cases.MAX_NET_REDRAWS times at
the most) where a pair is not; that is a property of the input, never of what a kernel answered."""
import functools

import numpy as np

from oracle import ref_port as rp
from tests import fp16_checker as ck
from tests import ga16_checker as gk
from tests import sharing_cases as S

F32 = np.float32
_quiet = S._quiet
# the crafted pair whose per-entry rounding shows: ROUNDING_ENTRIES Linear entries of ROUNDING_PAIR, every other entry equal
ROUNDING_PAIR = (1.3828125, 0.041290283203125)
ROUNDING_ENTRIES = 100
ROUNDING_CONTRACT, ROUNDING_UNROUNDED = 13.421875, 13.4140625


def _square_sums(flats, D):
    """[n][n] fp64: sum over the Linear entries of f64(f16(f32(w_j - w_i)))^2 (np.sum's order); the upper triangle is
    computed, the lower one mirrors it (round to nearest even is symmetric: f16(a - b) = -f16(b - a))"""
    w = np.ascontiguousarray(np.asarray(flats, dtype=np.float32)[:, gk.linear_mask(D)])
    out = np.zeros((len(w), len(w)), dtype=np.float64)
    with np.errstate(**_quiet):
        for i in range(len(w)):
            d = (w[i:] - w[i]).astype(np.float32).astype(np.float16).astype(np.float64)
            out[i, i:] = np.sum(d * d, axis=1)   # the squares are exact: 22 significant bits at the most
            out[i:, i] = out[i, i:]
    return out


def _f16_word(x):
    """fp64 -> the fp16 value (one rounding, nearest even: numpy converts double to half directly) as float32"""
    with np.errstate(**_quiet):
        return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float32)


def pairwise(flats, D):
    """dist[i][j] = f16(sqrt(sum_p f64(d)^2)), d = f16(f32(w_j[p] - w_i[p])) over gk.linear_mask(D), as float32 words; the
    diagonal is +0.0 by the contract, also for a net that holds inf (whose inf - inf would say NaN)"""
    with np.errstate(**_quiet):
        d = _f16_word(np.sqrt(_square_sums(flats, D)))
    np.fill_diagonal(d, F32(0))
    return d


def _sums_order_proof(s, n_terms):
    """sharing_cases._sums_order_proof with fp16 output: the interval s +- 2 n 2^-53 s, widened by 2^-50 for the root, rounds
    to one fp16 word"""
    with np.errstate(**_quiet):
        err = 2 * n_terms * 2.0 ** -53 * s
        lo = _f16_word(np.sqrt(np.maximum(s - err, 0) * (1 - 2.0 ** -50)))
        hi = _f16_word(np.sqrt((s + err) * (1 + 2.0 ** -50)))
    return (S.bits32(lo) == S.bits32(hi)) | ~np.isfinite(s)


def pairwise_order_proof(flats, D, rows=None):
    """every finite distance of pairwise(flats, D) (rows: of those rows only) is the same fp16 word under any order of its
    fp64 sum: the interval test, or - a pair that it refuses - a sum that is exact in any order (sharing_cases.
    _exact_in_any_order on its squares, which are fp32 values).  The second matters for the rounding pair, whose root is an
    exact fp16 tie that no order can move."""
    w = np.asarray(flats, dtype=np.float32)
    mask = gk.linear_mask(D)
    if rows is None:
        sums, rows = _square_sums(w, D), range(len(w))
    else:
        x = np.ascontiguousarray(w[:, mask])
        with np.errstate(**_quiet):
            sums = np.stack([np.sum((x - x[k]).astype(np.float16).astype(np.float64) ** 2, axis=1) for k in rows])
    bad = np.argwhere(~_sums_order_proof(sums, int(mask.sum())))
    with np.errstate(**_quiet):
        for r, j in bad:
            i = list(rows)[r]
            if i == j:   # (the diagonal is +0.0 by the contract)
                continue
            d = (w[j, mask] - w[i, mask]).astype(np.float16).astype(np.float32)
            if not S._exact_in_any_order(d * d):
                return False
    return True


@functools.lru_cache(maxsize=None)
def nets(D):
    """-> ([n][P] sharing_cases.nets(D) with the Linear entries rounded to fp16, redrawn nets): every pairwise fp16 distance
    order-proof, and the niche counts of every leading n' x n' block with n' in PAIRWISE_N too"""
    base = S.nets(D)[0]
    P, mask = base.shape[1], gk.linear_mask(D)
    w = np.stack([gk.round_linear(x, D) for x in base])
    n_terms = int(mask.sum())
    redrawn = 0
    while True:
        bad = np.argwhere(~_sums_order_proof(_square_sums(w, D), n_terms))
        if len(bad) == 0:
            break
        redrawn += 1
        assert redrawn <= S.MAX_NET_REDRAWS, f"no order-proof fp16 population within {S.MAX_NET_REDRAWS} redrawn nets (D {D})"
        k = int(bad.max())
        x = (np.random.Generator(np.random.PCG64(4600 + D + 100 * k + 7 * redrawn)).standard_normal(P) * 0.1).astype(np.float32)
        x[~mask] = 1.0
        w[k] = gk.round_linear(x, D)
    d = pairwise(w, D)
    assert all(S.niche_order_proof(d[:m, :m]) for m in S.PAIRWISE_N if m <= len(w)), "a niche count is not order-proof"
    return w, redrawn


@functools.lru_cache(maxsize=None)
def expected(D):
    return pairwise(nets(D)[0], D)


CRAFTED = ("identical", "layernorm", "inf", "extreme", "subnormal", "rounding")
CRAFTED_N = (3, S.TILE + 1)   # one tile pair; three, and a net past the first tile


def _with_rows(w, D, base, changed):
    """pairwise(w, D) where only the nets `changed` differ from those of the matrix `base`: their rows and columns computed
    again, by pairwise()'s own arithmetic"""
    want = base.copy()
    x = np.ascontiguousarray(np.asarray(w, dtype=np.float32)[:, gk.linear_mask(D)])
    with np.errstate(**_quiet):
        for k in changed:
            d = (x - x[k]).astype(np.float32).astype(np.float16).astype(np.float64)
            want[k, :] = want[:, k] = _f16_word(np.sqrt(np.sum(d * d, axis=1)))
    np.fill_diagonal(want, F32(0))
    return want


def changed_nets(kind, n):
    """the nets that crafted(D, kind, n) changes"""
    return {"plain": (), "layernorm": (0, n // 2, n - 1), "inf": (n // 2,)}.get(kind, (0, n - 1))


def crafted(D, kind, n):
    """the first n nets of nets(D) (a copy) with one edge put in -> (flats [n][P], expected distances [n][n] from pairwise())"""
    w = nets(D)[0][:n].copy()
    base = expected(D)[:n, :n]
    ln = np.flatnonzero(~gk.linear_mask(D))
    lin = np.flatnonzero(gk.linear_mask(D))
    if kind == "plain":
        return w, base.copy()
    if kind == "identical":          # an off-diagonal +0.0
        w[n - 1] = w[0]
    elif kind == "layernorm":        # LayerNorm entries never count, whatever they hold
        w[0, ln[::2]], w[0, ln[1::2]] = 1e30, -1e30
        w[n - 1, ln] = np.nan
        w[n // 2, ln[:7]] = np.inf
    elif kind == "inf":              # one inf Linear entry: the net's row and column are inf, its diagonal +0.0
        w[n // 2, lin[len(lin) // 3]] = np.inf
    elif kind == "extreme":          # one entry 65504 in net 0 and -65504 in net n - 1: d = f16(131008) = inf between them
        w[0, lin[5]], w[n - 1, lin[5]] = 65504.0, -65504.0
    elif kind == "subnormal":        # net n - 1 = net 0 but for 50 entries whose differences are fp16 subnormals
        w[n - 1] = w[0]
        w[0, lin[:50]] = 0.0
        w[n - 1, lin[:50]] = 3 * 2.0 ** -24
    elif kind == "rounding":         # net n - 1 = net 0 but for the rounding pair's entries
        w[n - 1] = w[0]
        w[0, lin[-ROUNDING_ENTRIES:]], w[n - 1, lin[-ROUNDING_ENTRIES:]] = ROUNDING_PAIR
    else:
        raise KeyError(kind)
    return w, _with_rows(w, D, base, changed_nets(kind, n))


# ------------------------------------------------------------------------------------------- the engine's generation
def engine_initial():
    """sharing_cases.engine_initial with every net's Linear entries rounded to fp16 -> (hof, population) {role: [k][P]}"""
    hof, pop = S.engine_initial()
    rnd = lambda d: {r: np.stack([gk.round_linear(w, rp.ROLE_D[r]) for w in d[r]]) for r in rp.ROLES}   # noqa: E731
    return rnd(hof), rnd(pop)


def play_generation_games(st, gen, limit_train, first_ordinal=1, max_cycles=25):
    """the 3 * pop * hof training games of generation `gen` on the checker's state, in HalfGAEngine's order -> [3 pop hof][3]"""
    stream = rp.Stream()
    pop, hof_n = len(st.popu[gk.ROLES[0]]), len(st.hof[gk.ROLES[0]])
    o = first_ordinal + gen * (3 * pop * hof_n + gk.N_EVAL)
    out = []
    for role in gk.ROLES:
        for i in range(pop):
            for k in range(hof_n):
                a0, a1, adv = rp.ga_game_nets(role, st.popu[role][i], st.hof, k, hof_n)
                g = ck.play_game(stream, a0, a1, adv, limit_train, max_cycles, ordinal=o)
                assert g["status"] == 0
                o += 1
                out.append(g["rewards"])
    return np.array(out, dtype=np.float64), stream, o


def generation_tail(rewards, pop_flat, stale_dist, D, ri, gen, hof, E, sigma, seed, hof_mean, population_sharing):
    """sharing_cases.generation_tail in the float16 contract: the share over pairwise() of this module (niche counts) or the
    sharing score of the fp16 stale-agent distances, sharing_cases.fitness, the ranking, and the fp16 children
    (ga16_checker.mutate)"""
    pop_flat = np.asarray(pop_flat, dtype=np.float32)
    pop = len(pop_flat)
    out = {}
    if population_sharing:
        out["pair_dist"] = pairwise(pop_flat, D)
        out["niche"] = share = S.niche(out["pair_dist"])
    else:
        out["diversity"] = gk.sharing_score(stale_dist)
        share = np.array([out["diversity"]], dtype=np.float32)
    flags = (S.HOF_MEAN if hof_mean else 0) | (S.PER_INDIVIDUAL if population_sharing else 0)
    fit = S.fitness(np.asarray(rewards)[:pop * hof], hof, hof, S.RET_SLOT[ri], flags, share)
    order = gk.rank_desc(fit)
    elites = [pop_flat[i] for i in order[:E]]
    out.update(fitness=fit, order=order, elite_ids=order[:E], best_dist=F32(stale_dist[order[0]]),
               children=[gk.mutate(elites[c % E], D, sigma, seed, c, 4 * gen + ri) for c in range(pop - 1)])
    return out


def generation(st, gen, sigma, E, limit, philox_seed, hof_mean, population_sharing):
    """one HalfGAEngine generation under the modes on the checker's state (updated in place) -> dict(games, tails {role:
    generation_tail}, eval_games)"""
    rewards, stream, o = play_generation_games(st, gen, limit)
    pop, hof_n = len(st.popu[gk.ROLES[0]]), len(st.hof[gk.ROLES[0]])
    per = pop * hof_n
    if st.dist is None:
        st.dist = {r: np.array([gk.distance(w, st.stale[r], gk.ROLE_D[r]) for w in st.popu[r]], dtype=np.float32)
                   for r in gk.ROLES}
    rec = {"games": rewards, "tails": {}, "eval_games": []}
    new_dist = {}
    for ri, r in enumerate(gk.ROLES):
        D = gk.ROLE_D[r]
        t = rec["tails"][r] = generation_tail(rewards[ri * per:(ri + 1) * per], np.stack(st.popu[r]), st.dist[r], D, ri, gen,
                                              hof_n, E, sigma, philox_seed, hof_mean, population_sharing)
        t["stale_dist"] = st.dist[r].copy()
        elites = [st.popu[r][i] for i in t["elite_ids"]]
        st.elites[r] = elites
        st.hof[r].append(elites[0])
        st.hof[r].pop(0)
        new_dist[r] = np.array([st.dist[r][t["order"][0]]] + [gk.distance(w, st.stale[r], D) for w in t["children"]],
                               dtype=np.float32)
        st.popu[r] = [elites[0]] + list(t["children"])
    st.dist = new_dist
    for _ in range(gk.N_EVAL):
        g = ck.play_game(stream, st.hof["agent_0"][-1], st.hof["agent_1"][-1], st.hof["adversary_0"][-1], limit, 25, ordinal=o)
        assert g["status"] == 0
        o += 1
        rec["eval_games"].append(g["rewards"])
    return rec
