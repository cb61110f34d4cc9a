"""The float16 Co-ES generation restated sequentially on the CPU (the contract of DESIGN.md 6a "Float16 Co-ES"): the stored
noise = the oracle's counter-based fp32 child of an all-zero parent (0 + noise32) rounded to fp16 with numpy; perturbed nets
through tests/ga16_checker.mutate; games through tests/fp16_checker.play_game; distances and the sharing score through
ga16_checker.distance / sharing_score; the fitness rounding, the chunked fp32 sum and the three roundings of the apply rule
in numpy; generation() composes them in HalfESEngine's order."""
import numpy as np

from oracle import ref_port as rp
from tests import fp16_checker as ck
from tests import ga16_checker as gk

ROLES = rp.ROLES
ROLE_D = rp.ROLE_D
RET_SLOT = {"agent_0": 0, "agent_1": 1, "adversary_0": 2}   # the role's slot of play_game's triple
N_EVAL = 10
ES_CHUNKS = 8


def f16(x):
    """round to fp16 (nearest even, subnormals kept, past 65504 inf) -> float32 holding the fp16 value; from fp64 input this
    is ONE rounding"""
    with np.errstate(over="ignore"):
        return np.asarray(x).astype(np.float16).astype(np.float32)


def noise16(D, sigma, seed, stream_lo, stream_hi):
    """the stored noise of one individual over the flat parameters() vector: f16(sigma * eps) on Linear entries, 0 elsewhere"""
    zero = np.zeros(rp.param_count(D), dtype=np.float32)
    n32 = rp.mutate_philox(zero, D, np.float32(sigma), seed, stream_lo, stream_hi, skip_layernorm=True)
    out = f16(n32)
    assert not out[~gk.linear_mask(D)].any()
    return out


def fitness16(rewards, score=None):
    """fit16 = f16(reward) in one rounding from fp64; with a sharing score f16(f32(fit16) / (1.0f + score))"""
    fit = f16(np.asarray(rewards, dtype=np.float64))
    if score is not None:
        with np.errstate(over="ignore", invalid="ignore"):
            fit = f16(fit / (np.float32(1.0) + np.float32(score)))
    return fit.astype(np.float32)


def chunk_partials(noises16, fit16, chunks):
    """[chunks][P] float32: chunk c = individuals [c n / C, (c + 1) n / C), j ascending, acc = fmaf(fit, noise, acc) from 0.
    The product of two fp16 values is exact in float32, so multiply-then-add rounds once, as the fmaf does."""
    noises16 = np.asarray(noises16, dtype=np.float32)
    fit16 = np.asarray(fit16, dtype=np.float32)
    n = len(fit16)
    out = np.zeros((chunks, noises16.shape[1]), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(chunks):
            acc = out[c]
            for j in range(c * n // chunks, (c + 1) * n // chunks):
                prod = fit16[j] * noises16[j]
                acc = (acc + prod).astype(np.float32)
            out[c] = acc
    return out


def dot16(partials):
    """the chunk sums added left to right in float32, rounded once to fp16"""
    tot = np.array(partials[0], dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for p in partials[1:]:
            tot = (tot + p).astype(np.float32)
    return f16(tot)


def scale16(lr, n, sigma):
    """f16(lr / (n sigma)): the fp64 quotient of the double lr and the fp32 sigma, one rounding"""
    with np.errstate(over="ignore"):
        return np.float32(np.float16(float(lr) / (n * float(np.float32(sigma)))))


def apply(theta, D, dot, lr, n, sigma):
    """-> (new theta, upd16): upd16 = f16(scale16 * dot16), theta' = f16(theta + upd16) on Linear entries"""
    m = gk.linear_mask(D)
    theta = np.asarray(theta, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        upd = f16(scale16(lr, n, sigma) * np.asarray(dot, dtype=np.float32))
        out = theta.copy()
        out[m] = f16(theta[m] + upd[m])
    return out, upd


def update(theta, D, fit16, sigma, lr, seed, stream_lo_first, stream_hi, chunks=ES_CHUNKS):
    """the whole update of one role's base net from the fitness"""
    n = len(fit16)
    noises = np.stack([noise16(D, sigma, seed, stream_lo_first + j, stream_hi) for j in range(n)])
    new, _ = apply(theta, D, dot16(chunk_partials(noises, fit16, chunks)), lr, n, sigma)
    return new


def generation(base, gen, sigmas, lr, fitness_sharing, pop, limit_train=None, limit_eval=None, max_cycles=25, philox_seed=0,
               first_ordinal=1, chunks=ES_CHUNKS):
    """one generation on `base` {role: flat fp16-valued net} (updated in place) -> dict(games: the 3 pop reward triples, pert
    {role: perturbed nets}, dist / score / fit16 {role: ...}, eval_games, eval_rewards)"""
    stream = rp.Stream()
    o = first_ordinal + gen * (3 * pop + N_EVAL)
    rec = {"games": [], "eval_games": [], "dist": {}, "score": {}, "fit16": {}}
    pert = {r: [gk.mutate(base[r], ROLE_D[r], sigmas[r], philox_seed, j, 4 * gen + ri, skip_layernorm=True)
                for j in range(pop)] for ri, r in enumerate(ROLES)}
    rec["pert"] = pert
    rewards = {r: [] for r in ROLES}
    for j in range(pop):
        for r in ROLES:
            nets = dict(base)
            nets[r] = pert[r][j]
            g = ck.play_game(stream, nets["agent_0"], nets["agent_1"], nets["adversary_0"], limit_train, max_cycles, ordinal=o)
            assert g["status"] == 0
            o += 1
            rec["games"].append(g["rewards"])
            rewards[r].append(g["rewards"][RET_SLOT[r]])
    for ri, r in enumerate(ROLES):
        D = ROLE_D[r]
        score = None
        if fitness_sharing:
            rec["dist"][r] = np.array([gk.distance(w, base[r], D) for w in pert[r]], dtype=np.float32)
            score = rec["score"][r] = gk.sharing_score(rec["dist"][r])
        fit = rec["fit16"][r] = fitness16(rewards[r], score)
        base[r] = update(base[r], D, fit, sigmas[r], lr, philox_seed, 0, 4 * gen + ri, chunks)
    ev = [0.0, 0.0, 0.0]
    for _ in range(N_EVAL):
        g = ck.play_game(stream, base["agent_0"], base["agent_1"], base["adversary_0"], limit_eval, max_cycles, ordinal=o)
        assert g["status"] == 0
        o += 1
        rec["eval_games"].append(g["rewards"])
        for s in range(3):
            ev[s] += g["rewards"][s]
    rec["eval_rewards"] = [e / 10 for e in ev]
    return rec
