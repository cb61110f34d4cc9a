"""The float16 Co-ES generation over DeepQN restated sequentially on the CPU (the contract of DESIGN.md 6a "Float16 DeepQN
Co-ES"), composed from what the other float16 checkers already state: perturbed nets through tests/dqn_ga16_checker.mutate
(BatchNorm skipped); the stored noise = the oracle's counter-based fp32 child of an all-zero parent (0 + noise32) rounded to
fp16 with numpy; games through dqn_ga16_checker.play_game; distances through dqn_ga16_checker.distance; the sharing score
through ga16_checker.sharing_score; the fitness rounding, the chunked fp32 sum and the roundings of the apply rule through
tests/es16_checker; the apply masked to the non-BatchNorm parameters; generation() composes them in HalfDQNESEngine's order,
game ordinals as oracle/ref_port.py:dqn_es_train numbers them."""
import numpy as np

from oracle import ref_port as rp
from tests import dqn_ga16_checker as dk
from tests import es16_checker as ek
from tests import ga16_checker as gk

ROLES = rp.DQN_ROLES
N_EVAL = 10
ES_CHUNKS = 8

_masks = {}


def n_params(C, n_actions):
    return int(rp.lib().oracle_dqn_param_count(C, n_actions))


def moving_mask(C, n_actions):
    """True at the entries a Co-ES update moves: every parameter but the BatchNorm affine (Atari/deepqn.py:158-172)"""
    key = (C, n_actions)
    if key not in _masks:
        m = np.ones(n_params(C, n_actions), dtype=bool)
        for o, n in rp.dqn_bn_segments(C, n_actions):
            m[o:o + n] = False
        m.setflags(write=False)
        _masks[key] = m
    return _masks[key]


def noise16(C, n_actions, sigma, seed, stream_lo, stream_hi):
    """the stored noise of one individual over the flat parameters() vector: f16(sigma * eps) on conv and Linear entries, 0 at
    the BatchNorm affine"""
    zero = np.zeros(n_params(C, n_actions), dtype=np.float32)
    out = dk.to_half(rp.perturb_philox_flat(zero, np.float32(sigma), seed, stream_lo & 0xffffffff, stream_hi & 0xffffffff,
                                            rp.dqn_bn_segments(C, n_actions)))
    assert not out[~moving_mask(C, n_actions)].any()
    return out


def apply(theta, C, n_actions, dot, lr, n, sigma):
    """-> (new theta, upd16): upd16 = f16(scale16 * dot16), theta' = f16(theta + upd16) on the non-BatchNorm entries"""
    m = moving_mask(C, n_actions)
    theta = np.asarray(theta, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        upd = ek.f16(ek.scale16(lr, n, sigma) * np.asarray(dot, dtype=np.float32))
        out = theta.copy()
        out[m] = ek.f16(theta[m] + upd[m])
    return out, upd


def update(theta, C, n_actions, fit16, sigma, lr, seed, stream_lo_first, stream_hi, chunks=ES_CHUNKS):
    """the whole update of one role's base net from the fitness"""
    n = len(fit16)
    noises = np.stack([noise16(C, n_actions, sigma, seed, stream_lo_first + j, stream_hi) for j in range(n)])
    new, _ = apply(theta, C, n_actions, ek.dot16(ek.chunk_partials(noises, fit16, chunks)), lr, n, sigma)
    return new


def generation(base, gen, sigmas, lr, fitness_sharing, pop, C, n_actions, T_train, T_eval, env_seed, philox_seed=0,
               first_ordinal=1, chunks=ES_CHUNKS):
    """one generation on `base` {role: flat fp16-valued net} (updated in place) -> dict(games: the 2 pop reward pairs, pert
    {role: perturbed nets}, dist / score / fit16 {role: ...}, eval_games, eval_rewards).  sigmas: (first_0, second_0)"""
    o = first_ordinal + gen * (2 * pop + N_EVAL)
    rec = {"games": [], "eval_games": [], "dist": {}, "score": {}, "fit16": {}}
    pert = {r: [dk.mutate(base[r], C, n_actions, sigmas[ri], philox_seed, j, 4 * gen + ri, skip_bn=True) for j in range(pop)]
            for ri, r in enumerate(ROLES)}
    rec["pert"] = pert
    if fitness_sharing:   # against the base nets the perturbed nets were drawn from
        for r in ROLES:
            rec["dist"][r] = np.array([dk.distance(w, base[r]) for w in pert[r]], dtype=np.float32)
            rec["score"][r] = gk.sharing_score(rec["dist"][r])
    rewards = {r: [] for r in ROLES}
    for j in range(pop):
        for ri, r in enumerate(ROLES):
            nets = (pert[r][j], base["second_0"]) if ri == 0 else (base["first_0"], pert[r][j])
            g = dk.play_game(nets[0], nets[1], C, n_actions, env_seed, o + 2 * j + ri, T_train)
            rec["games"].append(g)
            rewards[r].append(g[ri])
    for ri, r in enumerate(ROLES):   # (no update reads the other role's base net: one after the other is all at once)
        fit = rec["fit16"][r] = ek.fitness16(rewards[r], rec["score"][r] if fitness_sharing else None)
        base[r] = update(base[r], C, n_actions, fit, sigmas[ri], lr, philox_seed, 0, 4 * gen + ri, chunks)
    ev = [0.0, 0.0]
    for j in range(N_EVAL):
        g = dk.play_game(base["first_0"], base["second_0"], C, n_actions, env_seed, o + 2 * pop + j, T_eval)
        rec["eval_games"].append(g)
        for s in range(2):
            ev[s] += g[s]
    rec["eval_rewards"] = [e / 10 for e in ev]
    return rec
