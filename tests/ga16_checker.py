"""The float16 Co-GA generation restated sequentially on the CPU (the contract of DESIGN.md "float16 nets", breeding part):
mutation = the oracle's counter-based fp32 child of the upcast parent with its Linear entries rounded to fp16; distance =
f16(sqrt(sum in fp64 of f16(a - b)^2)) over the Linear entries; games through tests/fp16_checker.play_game; sharing score
through the oracle's own oracle_diversity, fitness and rank as the oracle port writes them; generation() composes them in
HalfGAEngine's order (GAEngine.breed_device on one GPU)."""
import ctypes as C

import numpy as np

from oracle import ref_port as rp
from tests import fp16_checker as ck

ROLES = rp.ROLES
ROLE_D = rp.ROLE_D
N_EVAL = 10

_masks = {}


def linear_mask(D):
    """True at the Linear weights and biases of the flat parameters() vector (= get_weights_ES()'s entries)"""
    if D not in _masks:
        m = np.zeros(rp.param_count(D), dtype=bool)
        for o, n in rp.linear_segments(D):
            m[o:o + n] = True
        _masks[D] = m
    return _masks[D]


def round_linear(flat32, D):
    """fp16 rounding (nearest even, past 65504 inf, subnormals kept) of the Linear entries; LayerNorm entries as they are"""
    out = np.array(flat32, dtype=np.float32, copy=True)
    m = linear_mask(D)
    with np.errstate(over="ignore"):
        out[m] = out[m].astype(np.float16).astype(np.float32)
    return out


def add_noise(parent, D, noise):
    """child = f16(f32(parent) + noise) on Linear entries, parent + noise on LayerNorm entries; noise is fp32"""
    parent = np.asarray(parent, dtype=np.float32)
    with np.errstate(over="ignore"):
        return round_linear(parent + np.asarray(noise, dtype=np.float32), D)


def mutate(parent, D, sigma, seed, stream_lo, stream_hi, skip_layernorm=False):
    """the float16 child of noise stream (stream_lo, stream_hi): the fp32 child of the upcast parent, Linear entries rounded"""
    child32 = rp.mutate_philox(np.ascontiguousarray(parent, dtype=np.float32), D, np.float32(sigma), seed, stream_lo,
                               stream_hi, skip_layernorm=skip_layernorm)
    return round_linear(child32, D)


def distance_sum(a, b, D):
    """sum over the Linear entries of f16(f32(a) - f32(b))^2 in fp64"""
    m = linear_mask(D)
    with np.errstate(over="ignore", invalid="ignore"):
        d = (np.asarray(a, dtype=np.float32)[m] - np.asarray(b, dtype=np.float32)[m]).astype(np.float16)
        d = d.astype(np.float64)
        return np.sum(d * d)


def distance(a, b, D):
    """-> the distance as a float32 that holds an fp16 value"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.float32(np.float16(np.sqrt(distance_sum(a, b, D))))


def f16_bits(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16).view(np.uint16)


# Selection.  oracle/ref_port.py has the Co-GA sharing / fitness / rank arithmetic only inline in ga_train (div =
# diversity(...) at :322, fit.append(last / hof_n / (1 + div)) at :337, np.argsort(fitness)[::-1] at :343), on distances it
# computes itself from fp32 nets.  Here the distances are given (fp16 values), so: the score goes through the oracle's C
# sharing code (oracle_diversity, coevo_oracle.c:318-342) with each distance handed over as a one-entry net, and fitness()
# and rank_desc() restate lines :337 and :343 in the float32 arithmetic numpy >= 2 gives them (tests/test_kernels_gpu.py
# test_diversity_fitness_rank pins the device kernels to the same expressions).
def sharing_score(dist):
    """the oracle's sharing arithmetic (oracle_diversity) on given distances: each distance is handed over as a one-entry
    'net' against a zero individual, whose fp64 sqrt(d * d) is d again.  A NaN share (all distances 0, a NaN or two infinite
    distances) makes the score NaN, as np.maximum does in the reference's expression"""
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    zero = np.zeros(1, dtype=np.float32)
    so, sl = np.array([0], dtype=np.int32), np.array([1], dtype=np.int32)
    back = np.zeros(len(dist), dtype=np.float32)
    fn = rp.lib().oracle_diversity
    fn.restype = C.c_double
    score = fn(rp._fp(zero), rp._fp(dist), len(dist), C.c_size_t(1), rp._ip(so), rp._ip(sl), 1, rp._fp(back))
    assert np.array_equal(back.view(np.uint32), np.abs(dist).view(np.uint32)) or np.isnan(dist).any()
    return np.float32(score)


def fitness(last_rewards, hof_n, div):
    """genetic_algorithm.py:140-146 in float32, as oracle/ref_port.py and numpy >= 2 evaluate it (quirk Q2: the last game)"""
    return np.array([np.float32(r / hof_n) / (np.float32(1) + np.float32(div)) for r in last_rewards], dtype=np.float32)


def rank_desc(fit):
    """argsort(fitness)[::-1] on a stable ascending sort (Q13)"""
    return [int(x) for x in np.argsort(np.asarray(fit, dtype=np.float32), kind="stable")[::-1]]


class State:
    """population, Hall of Fame and stale agent of the three roles as flat float32 vectors of fp16-valued nets, plus the
    stale-agent distances the last breeding left behind (None: compute them from the nets)"""

    def __init__(self, pop_flat, hof_flat):
        self.popu = {r: [np.array(w, dtype=np.float32) for w in pop_flat[r]] for r in ROLES}
        self.hof = {r: [np.array(w, dtype=np.float32) for w in hof_flat[r]] for r in ROLES}
        self.stale = {r: self.popu[r][-1].copy() for r in ROLES}   # Q3
        self.elites = {r: [] for r in ROLES}
        self.dist = None


def generation(st, gen, sigmas, E, limit_train=None, limit_eval=None, max_cycles=25, philox_seed=0, first_ordinal=1):
    """one generation on `st` (updated in place) -> dict(games: main games' reward triples, eval_games: the N_EVAL triples,
    eval_rewards, elite_ids, diversity {role: float32}, fitness, tie {role: the role's fitness values are not all distinct})"""
    stream = rp.Stream()
    pop, hof_n = len(st.popu[ROLES[0]]), len(st.hof[ROLES[0]])
    M = 3 * pop * hof_n
    o = first_ordinal + gen * (M + N_EVAL)
    rec = {"games": [], "eval_games": [], "elite_ids": {}, "diversity": {}, "fitness": {}, "tie": {}}
    last = {r: [] for r in ROLES}
    for ph, role in enumerate(ROLES):
        for i in range(pop):
            for k in range(hof_n):
                a0, a1, adv = rp.ga_game_nets(role, st.popu[role][i], st.hof, k, hof_n)
                g = ck.play_game(stream, a0, a1, adv, limit_train, max_cycles, ordinal=o)
                assert g["status"] == 0
                o += 1
                rec["games"].append(g["rewards"])
            last[role].append(g["rewards"][ph])   # Q2: only the last HoF game counts
    if st.dist is None:
        st.dist = {r: np.array([distance(w, st.stale[r], ROLE_D[r]) for w in st.popu[r]], dtype=np.float32) for r in ROLES}
    new_dist = {}
    for ri, role in enumerate(ROLES):
        D = ROLE_D[role]
        div = sharing_score(st.dist[role])
        fit = fitness(last[role], hof_n, div)
        order = rank_desc(fit)
        rec["diversity"][role], rec["fitness"][role], rec["elite_ids"][role] = div, fit, order[:E]
        rec["tie"][role] = len(set(fit.tolist())) < len(fit)
        elites = [st.popu[role][i] for i in order[:E]]
        st.elites[role] = elites
        st.hof[role].append(elites[0])
        st.hof[role].pop(0)
        children = [mutate(elites[c % E], D, sigmas[role], philox_seed, c, 4 * gen + ri) for c in range(pop - 1)]
        new_dist[role] = np.array([st.dist[role][order[0]]] + [distance(w, st.stale[role], D) for w in children],
                                  dtype=np.float32)
        st.popu[role] = [elites[0]] + children
    st.dist = new_dist
    ev = [0.0, 0.0, 0.0]
    for _ in range(N_EVAL):
        g = ck.play_game(stream, st.hof["agent_0"][-1], st.hof["agent_1"][-1], st.hof["adversary_0"][-1], limit_eval,
                         max_cycles, ordinal=o)
        assert g["status"] == 0
        o += 1
        rec["eval_games"].append(g["rewards"])
        for s in range(3):
            ev[s] += g["rewards"][s]
    rec["eval_rewards"] = [e / 10 for e in ev]
    return rec
