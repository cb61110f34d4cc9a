"""The Co-GA extension modes hof_mean / population_sharing (include/coevo_sharing.h) as plain numpy statements,
and the inputs of tests/test_sharing_cpu.py and tests/test_sharing_gpu.py.  No GPU and no libcoevo needed here.

The device comparisons are equalities although the kernels add their fp64 terms in an order of their own (a thread's run of
parameters, then the slabs; lane-strided and a shuffle tree for the niche counts).  As in tests/select_cases.py every finite
input is therefore *order-proof*: the whole interval sum +- n * 2^-53 * sum|x|, the worst error of n fp64 additions in ANY
order, rounds to one fp32 word.  A draw that is not order-proof is redrawn with the next seed, select_cases.MAX_REDRAWS times
at the most; that is a property of the input, never of what a kernel answered."""
import functools

import numpy as np

from oracle import ref_port as rp
from tests import ga16_checker as gk
from tests import select_cases as sc

F32 = np.float32
HOF_MEAN, PER_INDIVIDUAL = 1, 2          # COEVO_FIT_HOF_MEAN, COEVO_FIT_PER_INDIVIDUAL
TILE = 32                                # the pairwise kernel's net tile (csrc/sharing.hip PW_TILE)
RET_SLOT = (0, 1, 2)                     # reward slot of role ri in a play_game triple: population.RET_SLOT in ROLES order
PAIRWISE_N = (1, 2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
_quiet = dict(over="ignore", invalid="ignore", divide="ignore", under="ignore")


def bits32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------- the statements
def _square_sums(flats, D):
    """[n][n] fp64: sum over the Linear entries of f64(f32(w_j - w_i))^2 (np.sum's order)"""
    w = np.ascontiguousarray(np.asarray(flats, dtype=np.float32)[:, gk.linear_mask(D)])
    out = np.zeros((len(w), len(w)), dtype=np.float64)
    with np.errstate(**_quiet):
        for i in range(len(w)):
            df = (w - w[i]).astype(np.float32)
            out[i] = np.sum(df.astype(np.float64) ** 2, axis=1)   # the squares are exact: 48 significant bits at the most
    return out


def pairwise(flats, D):
    """dist[i][j] = f32(sqrt(sum_p f64(df)^2)), df = w_j[p] - w_i[p] in fp32 over gk.linear_mask(D) of the flat parameters()
    vectors; the diagonal is +0.0 by the contract, also for a net that holds inf or NaN (whose inf - inf would say NaN)"""
    with np.errstate(**_quiet):
        d = np.sqrt(_square_sums(flats, D)).astype(np.float32)
    np.fill_diagonal(d, F32(0))
    return d


def _sums_order_proof(s, n_terms):
    """[n][n] bool over fp64 sums of n_terms squares: the interval s +- 2 n 2^-53 s (n for the any-order bound, n more for
    np.sum's own error; all terms are >= 0), widened by 2^-50 for a square root that may be an fp64 ulp or two off, rounds to
    one fp32 word after the root.  An inf or NaN sum is inf or NaN in every order."""
    with np.errstate(**_quiet):
        err = 2 * n_terms * 2.0 ** -53 * s
        lo = np.sqrt(np.maximum(s - err, 0) * (1 - 2.0 ** -50)).astype(np.float32)
        hi = np.sqrt((s + err) * (1 + 2.0 ** -50)).astype(np.float32)
    return (bits32(lo) == bits32(hi)) | ~np.isfinite(s)


def pairwise_order_proof(flats, D):
    """every finite distance of pairwise(flats, D) is the same fp32 word under any order of its fp64 sum"""
    return bool(_sums_order_proof(_square_sums(flats, D), int(gk.linear_mask(D).sum())).all())


def niche(d):
    """row by row through ga16_checker.sharing_score = the oracle's oracle_diversity arithmetic, the self term d[i][i] included"""
    d = np.asarray(d, dtype=np.float32)
    return np.array([gk.sharing_score(row) for row in d], dtype=np.float32)


def _exact_in_any_order(x):
    """the fp64 sum of these fp32 values has no rounding in ANY order: they are all multiples of the spacing q of the smallest
    one, and so is every partial sum, none of which exceeds sum|x| <= 2^52 q"""
    x = np.abs(np.asarray(x, dtype=np.float32))
    x = x[x != 0]
    if len(x) == 0:
        return True
    if not np.isfinite(x).all():
        return False
    return float(np.sum(x.astype(np.float64))) <= 2.0 ** 52 * float(np.spacing(x.min()))


def _row_order_proof(row):
    """select_cases.score_order_proof, which asks that the worst-case interval of each fp64 sum rounds to one fp32 word - or
    the sum is exact in any order.  (The second matters: the mean of 32 distances of one binade is an exact fp32 TIE once in
    32 rows, which the interval test must refuse although no order can move it.)"""
    row = np.asarray(row, dtype=np.float32)
    n = len(row)
    if not (_exact_in_any_order(row) or sc.order_proof(row.astype(np.float64), lambda s: F32(s / n))):
        return False
    sh = sc.contract_shares(row)
    if np.isnan(sh).any():
        return True
    return _exact_in_any_order(sh[sh > 0]) or sc.order_proof(sh[sh > 0].astype(np.float64), F32)


def niche_order_proof(d):
    return all(_row_order_proof(row) for row in np.asarray(d, dtype=np.float32))


def fitness(rewards, gpi, hof, slot, flags, share, game_first=0):
    """individual i's games are rewards[game_first + i gpi + k][slot]; HOF_MEAN: f32((+0.0 + r_0 + r_1 + ...) / hof), k
    ascending in fp64, else the last game (Q2); PER_INDIVIDUAL: / (1 + share[i]) in fp32, else / (1 + share[0])"""
    rewards = np.asarray(rewards, dtype=np.float64)
    share = np.atleast_1d(np.asarray(share, dtype=np.float32))
    pop = (len(rewards) - game_first) // gpi if flags & PER_INDIVIDUAL == 0 else len(share)
    out = np.zeros(pop, dtype=np.float32)
    with np.errstate(**_quiet):
        for i in range(pop):
            r = rewards[game_first + i * gpi:game_first + (i + 1) * gpi, slot]
            if flags & HOF_MEAN:
                num = np.float64(0.0)
                for x in r:
                    num = num + x
            else:
                num = r[-1]
            total = F32(num / np.float64(hof))
            out[i] = total / (F32(1) + share[i if flags & PER_INDIVIDUAL else 0])
    return out


def fitness_reversed(rewards, gpi, hof, slot, share):
    """fitness(..., HOF_MEAN | PER_INDIVIDUAL, ...) with each individual's sum taken from its last game down"""
    r = np.asarray(rewards, dtype=np.float64).reshape(-1, gpi, 3)[:, ::-1].reshape(-1, 3)
    return fitness(r, gpi, hof, slot, HOF_MEAN | PER_INDIVIDUAL, share)


def stale_distances(pop_flat, stale, D):
    """the distances to the stale agent (Q3) that the engine keeps beside either mode: select_cases.contract_dist"""
    return np.array([sc.contract_dist(stale, w, D) for w in pop_flat], dtype=np.float32)


def generation_tail(rewards, pop_flat, stale_dist, D, ri, gen, hof, E, sigma, seed, hof_mean, population_sharing):
    """The tail of one role's generation under the modes, from its games' reward triples [pop * hof][3] (individual-major),
    the population [pop][P] and the stale-agent distances [pop]: the share (niche counts over pairwise(), or the one sharing
    score against the stale agent), fitness(), ga16_checker.rank_desc, the elite ids, the best's stale-agent distance and the
    children rp.mutate_philox(elite[c % E], sigma, seed, c, 4 gen + ri)."""
    pop_flat = np.asarray(pop_flat, dtype=np.float32)
    pop = len(pop_flat)
    out = {}
    if population_sharing:
        out["pair_dist"] = pairwise(pop_flat, D)
        out["niche"] = share = niche(out["pair_dist"])
    else:
        out["diversity"] = gk.sharing_score(stale_dist)
        share = np.array([out["diversity"]], dtype=np.float32)
    flags = (HOF_MEAN if hof_mean else 0) | (PER_INDIVIDUAL if population_sharing else 0)
    fit = fitness(np.asarray(rewards)[:pop * hof], hof, hof, RET_SLOT[ri], flags, share)
    order = gk.rank_desc(fit)
    elites = [pop_flat[i] for i in order[:E]]
    out.update(fitness=fit, order=order, elite_ids=order[:E], best_dist=F32(stale_dist[order[0]]),
               children=[rp.mutate_philox(elites[c % E], D, F32(sigma), seed, c, 4 * gen + ri) for c in range(pop - 1)])
    return out


# ------------------------------------------------------------------------------------------- inputs
_PATTERN = (1e16, 1.0, -1e16, 0.5, 3.0, -1e16, 1e16, 2.0 ** -30)


def cancellation_rewards(pop, gpi):
    """[pop * gpi][3]: huge terms that cancel around small ones (1e16 + 1.0 is 1e16), each individual starting elsewhere in
    the pattern: the sum of an individual's games depends on the order of its terms"""
    g, s = np.meshgrid(np.arange(pop * gpi), np.arange(3), indexing="ij")
    return np.asarray(_PATTERN)[(g % gpi + g // gpi + 3 * s) % len(_PATTERN)]


MAX_NET_REDRAWS = 8


@functools.lru_cache(maxsize=None)
def nets(D, n=max(PAIRWISE_N)):
    """-> ([n][P] fp32 normals x 0.1 with LayerNorm gamma 1 / beta 0, nets redrawn): every pairwise distance order-proof, and
    the niche counts of every leading n' x n' block with n' in PAIRWISE_N too.  About one pair in 5000 is not order-proof
    under the worst-case bound; the later net of such a pair is drawn again, MAX_NET_REDRAWS times at the most."""
    P = rp.param_count(D)
    mask = gk.linear_mask(D)
    n_terms = int(mask.sum())

    def make(seed):
        w = (np.random.Generator(np.random.PCG64(seed)).standard_normal(P) * 0.1).astype(np.float32)
        w[~mask] = 1.0
        return w
    w = np.stack([make(2600 + D + 100 * i) for i in range(n)])
    redrawn = 0
    while True:
        bad = np.argwhere(~_sums_order_proof(_square_sums(w, D), n_terms))
        if len(bad) == 0:
            break
        redrawn += 1
        assert redrawn <= MAX_NET_REDRAWS, f"no order-proof population within {MAX_NET_REDRAWS} redrawn nets (D {D})"
        k = int(bad.max())
        w[k] = make(2600 + D + 100 * k + 7 * redrawn)
    d = pairwise(w, D)
    assert all(niche_order_proof(d[:m, :m]) for m in PAIRWISE_N if m <= n), "a niche count of the drawn nets is not order-proof"
    return w, redrawn


@functools.lru_cache(maxsize=None)
def expected(D):
    """pairwise() of nets(D), computed once: the distances of the first n' nets are its leading n' x n' block"""
    return pairwise(nets(D)[0], D)


def crafted(D, kind, n):
    """the first n nets of nets(D) (a copy) with one edge put in -> (flats [n][P], expected distances [n][n])"""
    w = nets(D)[0][:n].copy()
    want = expected(D)[:n, :n].copy()
    ln = np.flatnonzero(~gk.linear_mask(D))
    lin = np.flatnonzero(gk.linear_mask(D))
    if kind == "plain":
        return w, want
    if kind == "identical":          # an off-diagonal +0.0
        w[n - 1] = w[0]
        want[n - 1, :], want[:, n - 1] = want[0, :], want[:, 0]
        want[n - 1, n - 1] = want[0, n - 1] = want[n - 1, 0] = 0
    elif kind == "layernorm":        # LayerNorm entries never count, whatever they hold
        w[0, ln[::2]], w[0, ln[1::2]] = 1e30, -1e30
        w[n - 1, ln] = np.nan
        w[n // 2, ln[:7]] = np.inf
    elif kind == "inf":              # one inf Linear entry: the net's row and column are inf, its diagonal +0.0
        k = n // 2
        w[k, lin[len(lin) // 3]] = np.inf
        want[k, :], want[:, k] = np.inf, np.inf
        want[k, k] = 0
    else:
        raise KeyError(kind)
    return w, want


NICHE_CRAFTED = ("single", "zeros", "one_inf", "n257")


@functools.lru_cache(maxsize=None)
def niche_matrix(kind):
    """crafted symmetric 'distance' matrices without nets -> [n][n] fp32, every row order-proof"""
    if kind == "single":
        return np.zeros((1, 1), dtype=np.float32)
    if kind == "zeros":              # identical nets: 0 / 0, NaN everywhere
        return np.zeros((5, 5), dtype=np.float32)
    n = 257 if kind == "n257" else 6

    def make(s):
        u = (np.random.Generator(np.random.PCG64(s)).random((n, n)) * 3).astype(np.float32)
        d = np.triu(u, 1)
        d = d + d.T
        if kind == "one_inf":
            d[1, 4] = d[4, 1] = np.inf
        return d
    return sc._redraw(make, niche_order_proof, 3300 + n)[0]


# ------------------------------------------------------------------------------------------- the engine test's configuration
ENGINE = dict(pop=8, hof=3, elites=2, limit=9, seed=3, sigma=0.05, philox_seed=0)
MODES = ((True, False), (False, True), (True, True))   # (hof_mean, population_sharing): the three non-default pairs


CLUSTER = (2, 3, 4)        # these individuals start as close copies of individual 0 (sigma CLUSTER_SIGMA): a niche of four
CLUSTER_SIGMA = 0.02


def engine_initial():
    """-> (hof {role: [hof][P]}, population {role: [pop][P]}): the reference's creation order under the engine test's seed,
    then a niche: fresh nets are all but equidistant, so that every niche count is 1.00x and sharing could not move a rank"""
    import torch
    torch.manual_seed(ENGINE["seed"])
    hof, popu = rp.ga_initial(ENGINE["pop"], ENGINE["hof"])
    for ri, r in enumerate(rp.ROLES):
        for c in CLUSTER:
            popu[r][c] = rp.mutate_philox(popu[r][0], rp.ROLE_D[r], F32(CLUSTER_SIGMA), 99, c, ri)
    return {r: np.stack(hof[r]) for r in rp.ROLES}, {r: np.stack(popu[r]) for r in rp.ROLES}


def oracle_generation0_rewards(hof_flat, pop_flat):
    """the 3 * pop * hof training games of generation 0 through oracle.ref_port.play_game -> [3 pop hof][3] fp64"""
    stream = rp.Stream()
    hof = {r: list(hof_flat[r]) for r in rp.ROLES}
    out = []
    for role in rp.ROLES:
        for i in range(ENGINE["pop"]):
            for k in range(ENGINE["hof"]):
                a0, a1, adv = rp.ga_game_nets(role, pop_flat[role][i], hof, k, ENGINE["hof"])
                out.append(rp.play_game(stream, a0, a1, adv, ENGINE["limit"])["rewards"])
    return np.array(out, dtype=np.float64)
