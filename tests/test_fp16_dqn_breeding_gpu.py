"""Float16 DeepQN breeding on the GPU against the CPU restatement tests/dqn_ga16_checker.py, equalities only: the offspring
kernel word for word (coevo_dqn16_perturb_dist) and against the fp32 kernel's child, the rounding edges, its fused distance
partials against the standalone kernel's, the finalized distances, the refusals, and whole HalfDQNGAEngine generations (every
reward pair, fitness, diversity, elite ids, sigma, every net)."""
import functools

import numpy as np
import pytest
import torch

from coevonet_amd import lib as L
from coevonet_amd.dqn_ga_half import HalfDQNGAEngine
from coevonet_amd.dqn_population import dqn_initial_population
from oracle import ref_port as rp
from tests import dqn_ga16_checker as dk
from tests.util import Bag, sha

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0x7fc07e00   # NaN as an fp32 word and in both of its halves
SEED = 0x1234567890abcdef
SKIP_BN, COPY = 1, 8
ERR_ARG = -1
SHAPES = ((4, 6), (3, 18))   # between them they move every section boundary and the padded last quad
CALLS = ((1, 1, 5), (3, 3, 100))   # (child_first, n_children, stream_lo_first): nets 1 and 3 .. 5 of 7
NETS = 7
STREAM_HI = 9


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def stride16(C, n):
    return int(L.load().coevo_dqn16_slab_stride(C, n))


def blocks16(C, n):
    return int(L.load().coevo_dqn16_perturb_blocks(C, n))


def n_params(C, n):
    return int(L.load().coevo_dqn_param_count(C, n))


def pack16(flats, C, n):
    flats = np.ascontiguousarray(np.stack(flats), dtype=np.float32)
    slab = torch.full((len(flats) * stride16(C, n),), POISON, dtype=torch.int32, device=DEV)
    L.call("coevo_dqn16_pack", L._p(torch.from_numpy(flats).to(DEV)), L._p(slab), len(flats), C, n)
    return slab


def unpack16(slab, first, count, C, n):
    out = torch.zeros(count, n_params(C, n), dtype=torch.float32, device=DEV)
    L.call("coevo_dqn16_unpack", slab.data_ptr() + 4 * first * stride16(C, n), L._p(out), count, C, n)
    return out.cpu().numpy()


def dev_f32(x):
    return torch.tensor([x], dtype=torch.float32, device=DEV)


def dev_i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


def poisoned(words):
    return torch.full((words,), POISON, dtype=torch.int32, device=DEV)


def nan_partials(count):
    return torch.full((count,), float("nan"), dtype=torch.float64, device=DEV)


@functools.lru_cache(maxsize=None)
def parents_of(C, n):
    """two generic fp16-valued nets: initial nets after one mutation of every parameter (the BatchNorm affine then differs from
    1 / 0), the second on a larger scale"""
    torch.manual_seed(40 + C + n)
    a = dk.mutate(dk.to_half(rp.dqn_init(C, n)[0]), C, n, 0.02, 77, 0, 0)
    b = dk.mutate(dk.to_half(3.0 * rp.dqn_init(C, n)[0]), C, n, 0.1, 77, 1, 0)
    return a, b


@functools.lru_cache(maxsize=None)
def used_words(C, n):
    """words of a net's stride that hold parameters, asked of the library: a net of ones packs to nonzero words followed by the
    stride's zeroed padding"""
    w = pack16([np.ones(n_params(C, n), dtype=np.float32)], C, n).cpu().numpy()
    used = int(np.flatnonzero(w)[-1]) + 1
    assert (w[:used] != 0).all() and 0 <= len(w) - used < 64
    return used


def breed(parents, C, n, sigma, flags, with_dist=None, stream_hi=STREAM_HI, gen_dev=None, gen_bias=0):
    """the launches of CALLS into one poisoned 7-net child slab -> (child slab, parent slab, partials per call)"""
    par = pack16(parents, C, n)
    child = poisoned(NETS * stride16(C, n))
    sig = dev_f32(sigma)
    partials = []
    for first, count, slo in CALLS:
        idx = dev_i32([c % len(parents) for c in range(count)])
        part = nan_partials(count * blocks16(C, n)) if with_dist is not None else None
        L.call("coevo_dqn16_perturb_dist", L._p(par), L._p(idx), L._p(child), first, count, C, n, L._p(sig), SEED, slo, stream_hi,
               flags, L._p(gen_dev) if gen_dev is not None else None, gen_bias,
               L._p(with_dist) if with_dist is not None else None, L._p(part) if part is not None else None)
        partials.append(part)
    torch.cuda.synchronize()
    return child, par, partials


def want_children(parents, C, n, sigma, flags, stream_hi=STREAM_HI):
    return {first + c: dk.mutate(parents[c % len(parents)], C, n, sigma, SEED, slo + c, stream_hi, skip_bn=bool(flags & SKIP_BN))
            for first, count, slo in CALLS for c in range(count)}


def fp32_children(parents, C, n, sigma, flags):
    """what coevo_dqn_perturb (streamed fc1 layout) writes for the upcast parents with the same seed and streams -> flat [7][P]"""
    lib = L.load()
    st32, P = int(lib.coevo_dqn_slab_stride(C, n)), n_params(C, n)
    par32 = torch.zeros(len(parents) * st32, dtype=torch.float32, device=DEV)
    L.call("coevo_dqn_pack", L._p(torch.from_numpy(np.stack(parents)).to(DEV)), L._p(par32), len(parents), C, n)
    child32 = torch.zeros(NETS * st32, dtype=torch.float32, device=DEV)
    sig = dev_f32(sigma)
    for first, count, slo in CALLS:
        L.call("coevo_dqn_perturb", L._p(par32), L._p(dev_i32([c % len(parents) for c in range(count)])), L._p(child32), first,
               count, C, n, L._p(sig), SEED, slo, STREAM_HI, flags, 1, None, 0, None, None)
    flat = torch.zeros(NETS, P, dtype=torch.float32, device=DEV)
    L.call("coevo_dqn_unpack", L._p(child32), L._p(flat), NETS, C, n)
    return flat.cpu().numpy()


@pytest.mark.parametrize("flags", [0, SKIP_BN])
@pytest.mark.parametrize("sigma", [0.0, 0.05, 0.5])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"C{s[0]}n{s[1]}")
def test_perturb_every_word_against_the_checker_and_the_fp32_kernel(shape, sigma, flags):
    C, n = shape
    parents = parents_of(C, n)
    child, par, _ = breed(parents, C, n, sigma, flags)
    stride, P = stride16(C, n), n_params(C, n)
    words = child.cpu().numpy().view(np.uint32).reshape(NETS, stride)
    for untouched in (0, 2, 6):
        assert (words[untouched] == POISON).all(), "a net outside the written range changed"
    pwords = par.cpu().numpy().view(np.uint32).reshape(2, stride)
    want = want_children(parents, C, n, sigma, flags)
    flat32 = fp32_children(parents, C, n, sigma, flags)
    owner = {first + c: c % 2 for first, count, slo in CALLS for c in range(count)}   # the parent of each written net
    assert sorted(want) == [1, 3, 4, 5]
    for net in sorted(want):
        got = unpack16(child, net, 1, C, n)[0]
        assert np.array_equal(bits(got), bits(want[net])), (net, "differs from the checker")
        assert (words[net, used_words(C, n):] == 0).all(), "the stride's padding words are the parent's zeros"
        # every parameter, BatchNorm included: f16() of the fp32 kernel's child of the upcast parent, same seed and stream
        with np.errstate(over="ignore"):
            assert np.array_equal(bits(got), bits(flat32[net].astype(np.float16).astype(np.float32))), (net, "fp32 kernel")
        if sigma == 0.0:
            # bit-equal to the parent - but for a parent entry that is -0 (the first net of C = 3, n = 18 holds one): the
            # noise is +-0, and -0 + +0 is +0 in IEEE arithmetic, torch's and the checker's included
            pflat = parents[owner[net]]
            neg0 = bits(pflat) == 0x80000000
            assert np.array_equal(bits(got)[~neg0], bits(pflat)[~neg0]) and (got[neg0] == 0).all()
            if not neg0.any():
                assert np.array_equal(words[net], pwords[owner[net]]), "sigma 0 must reproduce the parent's words"
        else:
            changed = got != parents[owner[net]]
            bn = changed[P - 320:].mean()
            assert changed[:P - 320].mean() > 0.9 and (bn == 0.0 if flags else bn > 0.9)
        if flags:
            assert np.array_equal(bits(got[P - 320:]), bits(parents[owner[net]][P - 320:]))
    if sigma:   # distinct streams give distinct children of one parent
        assert not np.array_equal(words[3], words[5])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"C{s[0]}n{s[1]}")
def test_generation_counter_on_the_device_shifts_the_noise_stream_and_wraps(shape):
    """gen_dev: the launch reads the generation g from device memory and draws from stream_hi + 4 (g + gen_bias), modulo 2^32"""
    C, n = shape
    parents = parents_of(C, n)
    g = dev_i32([3])
    wrapped, _, _ = breed(parents, C, n, 0.05, 0, stream_hi=0xFFFFFFFE, gen_dev=g, gen_bias=-1)   # + 8 -> 6
    plain, _, _ = breed(parents, C, n, 0.05, 0, stream_hi=6)
    assert torch.equal(wrapped, plain) and int(g.item()) == 3
    want = want_children(parents, C, n, 0.05, 0, stream_hi=6)
    assert np.array_equal(bits(unpack16(wrapped, 4, 1, C, n)[0]), bits(want[4]))
    other, _, _ = breed(parents, C, n, 0.05, 0, stream_hi=2)
    assert not torch.equal(other, plain)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"C{s[0]}n{s[1]}")
def test_copy_flag_copies_and_serves_the_distance_alone(shape):
    C, n = shape
    parents = parents_of(C, n)
    stride, nb = stride16(C, n), blocks16(C, n)
    ref = pack16([parents[1]], C, n)
    child, par, parts = breed(parents, C, n, 0.5, COPY, with_dist=ref)
    words = child.cpu().numpy().view(np.uint32).reshape(NETS, stride)
    pwords = par.cpu().numpy().view(np.uint32).reshape(2, stride)
    for first, count, slo in CALLS:
        for c in range(count):
            assert np.array_equal(words[first + c], pwords[c % 2])
    for untouched in (0, 2, 6):
        assert (words[untouched] == POISON).all()
    # child_slab NULL and sigma NULL: the distance of the parents themselves = coevo_dqn16_distance's partials, bit for bit
    fused, alone = nan_partials(2 * nb), nan_partials(2 * nb)
    L.call("coevo_dqn16_perturb_dist", L._p(par), L._p(dev_i32([0, 1])), None, 0, 2, C, n, None, SEED, 0, 0, COPY, None, 0,
           L._p(ref), L._p(fused))
    L.call("coevo_dqn16_distance", L._p(ref), L._p(par), 2, C, n, L._p(alone))
    torch.cuda.synchronize()
    assert np.array_equal(fused.cpu().numpy().view(np.uint64), alone.cpu().numpy().view(np.uint64))
    assert np.array_equal(parts[1].cpu().numpy().view(np.uint64)[:2 * nb], alone.cpu().numpy().view(np.uint64))
    assert (alone.cpu().numpy()[nb:] == 0).all() and (alone.cpu().numpy()[:nb] > 0).any()   # parents[1] against itself


def test_edges_overflow_to_inf_and_subnormals_are_kept():
    C, n = 3, 18
    P = n_params(C, n)
    big = np.full(P, 65504, dtype=np.float32)
    # sigma 64: a noise of 16 or more (40 % of the entries) carries 65504 past the last finite half
    child, _, _ = breed([big, -big], C, n, 64.0, 0)
    want = want_children([big, -big], C, n, 64.0, 0)
    for net in (1, 4):
        got = unpack16(child, net, 1, C, n)[0]
        assert np.array_equal(bits(got), bits(want[net]))
        inf = np.isposinf(got) if net != 4 else np.isneginf(got)   # net 4 = child 1 of the second call: parent -big
        assert 0.3 < inf.mean() < 0.5 and not np.isnan(got).any()
    sub = (np.arange(P) % 1023 + 1).astype(np.uint16).view(np.float16).astype(np.float32)
    sub[1::2] *= -1
    assert (np.abs(sub) < 6.2e-5).all() and (sub != 0).all()
    for sigma in (0.0, 1e-6):   # untouched, and moved inside the subnormal range: never flushed to zero
        child, par, _ = breed([sub, sub[::-1].copy()], C, n, sigma, 0)
        want = want_children([sub, sub[::-1].copy()], C, n, sigma, 0)
        for net in (1, 3, 4):
            got = unpack16(child, net, 1, C, n)[0]
            assert np.array_equal(bits(got), bits(want[net])), (sigma, net)
            assert ((np.abs(got) < 6.2e-5) & (got != 0)).mean() > 0.95
        if sigma == 0.0:
            stride = stride16(C, n)
            words, pwords = child.cpu().numpy().reshape(NETS, stride), par.cpu().numpy().reshape(2, stride)
            assert np.array_equal(words[1], pwords[0]) and np.array_equal(words[4], pwords[1])


def order_proof_children(C, n, sigma, ref):
    """children of CALLS whose distance to `ref` is order-proof (dqn_ga16_checker.distance_order_proof), redrawn with the next
    stream_hi three times at the most -> (stream_hi, {net: child})"""
    parents = parents_of(C, n)
    for stream_hi in range(STREAM_HI, STREAM_HI + 4):
        want = want_children(parents, C, n, sigma, 0, stream_hi=stream_hi)
        if all(dk.distance_order_proof(w, ref) for w in want.values()):
            return stream_hi, want
    raise AssertionError("no order-proof case in four draws")


@pytest.mark.parametrize("sigma", [0.005, 0.05])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"C{s[0]}n{s[1]}")
def test_fused_partials_equal_the_distance_kernels_and_distances_equal_the_checkers(shape, sigma):
    C, n = shape
    parents = parents_of(C, n)
    stride, nb = stride16(C, n), blocks16(C, n)
    torch.manual_seed(7 + C)
    stale = dk.to_half(rp.dqn_init(C, n)[0])
    stream_hi, want = order_proof_children(C, n, sigma, stale)
    ref = pack16([stale], C, n)
    child, par, parts = breed(parents, C, n, sigma, 0, with_dist=ref, stream_hi=stream_hi)
    for (first, count, slo), part in zip(CALLS, parts):
        alone = nan_partials(count * nb)
        L.call("coevo_dqn16_distance", L._p(ref), child.data_ptr() + 4 * first * stride, count, C, n, L._p(alone))
        dist = torch.full((8,), -1.0, dtype=torch.float32, device=DEV)
        head = dev_f32(123.5)
        L.call("coevo_fc16_distance_finalize", L._p(part), nb, count, L._p(dist), 2, L._p(head))
        torch.cuda.synchronize()
        assert np.isfinite(part.cpu().numpy()).all()
        assert np.array_equal(part.cpu().numpy().view(np.uint64), alone.cpu().numpy().view(np.uint64)), "fused != standalone"
        d = dist.cpu().numpy()
        assert d[0] == -1.0 and d[1] == 123.5 and (d[2 + count:] == -1.0).all(), "head / neighbours"
        for c in range(count):
            w = dk.distance(want[first + c], stale)
            assert bits(d[2 + c])[0] == bits(w)[0], (first + c, d[2 + c], w)
            assert dk.f16_bits(d[2 + c]) == dk.f16_bits(w) and w > 0


def test_a_net_against_itself_is_zero():
    C, n = 4, 6
    nb = blocks16(C, n)
    a, b = parents_of(C, n)
    slab = pack16([a, b, a], C, n)
    part = nan_partials(3 * nb)
    L.call("coevo_dqn16_distance", L._p(slab), L._p(slab), 3, C, n, L._p(part))
    dist = torch.full((3,), -1.0, dtype=torch.float32, device=DEV)
    L.call("coevo_fc16_distance_finalize", L._p(part), nb, 3, L._p(dist), 0, None)
    torch.cuda.synchronize()
    d = dist.cpu().numpy()
    assert d[0] == 0 and d[2] == 0 and d[1] > 0
    if dk.distance_order_proof(b, a):
        assert bits(d[1])[0] == bits(dk.distance(b, a))[0]


def test_every_bad_argument_writes_nothing():
    """sentinels: the child slab and the partials sit between guard words and keep every bit after each refused call"""
    C, n = 3, 18
    lib, stride, nb = L.load(), stride16(C, n), blocks16(C, n)
    par = pack16(list(parents_of(C, n)), C, n)
    ref = pack16([parents_of(C, n)[0]], C, n)
    child = poisoned(3 * stride)          # net 1 is the target, nets 0 and 2 the guards
    part = nan_partials(nb + 2)           # partial 0 and nb + 1 the guards
    idx, sig = dev_i32([1]), dev_f32(0.05)
    good = dict(parent=L._p(par), idx=L._p(idx), child=L._p(child), first=1, n=1, C=C, n_actions=n, sigma=L._p(sig), seed=SEED,
                slo=0, shi=0, flags=0, gen=None, bias=0, ref=L._p(ref), partial=part.data_ptr() + 8)
    order = ("parent", "idx", "child", "first", "n", "C", "n_actions", "sigma", "seed", "slo", "shi", "flags", "gen", "bias", "ref",
             "partial")
    bad = [dict(parent=None), dict(idx=None), dict(child=None), dict(sigma=None), dict(C=0), dict(C=7), dict(n_actions=0),
           dict(n_actions=33), dict(C=C | L.DQN_FC1_TILED), dict(C=C | 0x200), dict(parent=L._p(par) + 4),
           dict(child=L._p(child) + 8), dict(ref=L._p(ref) + 4), dict(n=-1), dict(first=-1), dict(ref=None), dict(partial=None),
           dict(flags=2), dict(flags=4), dict(flags=16), dict(flags=SKIP_BN | 32), dict(flags=COPY | 2),
           dict(child=None, flags=COPY, ref=None, partial=None)]
    for b in bad:
        a = dict(good, **b)
        assert lib.coevo_dqn16_perturb_dist(*[a[k] for k in order], L._stream()) == ERR_ARG, b
    dgood = dict(ref=L._p(ref), pop=L._p(par), n=1, C=C, n_actions=n, partial=part.data_ptr() + 8)
    for b in (dict(ref=None), dict(pop=None), dict(partial=None), dict(C=0), dict(C=C | L.DQN_FC1_TILED), dict(n_actions=33),
              dict(ref=L._p(ref) + 8), dict(pop=L._p(par) + 4), dict(n=-1)):
        a = dict(dgood, **b)
        assert lib.coevo_dqn16_distance(a["ref"], a["pop"], a["n"], a["C"], a["n_actions"], a["partial"], L._stream()) == ERR_ARG, b
    # a count of 0 is fine and writes nothing either
    assert lib.coevo_dqn16_perturb_dist(*[dict(good, n=0)[k] for k in order], L._stream()) == 0
    assert lib.coevo_dqn16_distance(L._p(ref), L._p(par), 0, C, n, part.data_ptr() + 8, L._stream()) == 0
    torch.cuda.synchronize()
    assert (child.cpu().numpy().view(np.uint32) == POISON).all() and np.isnan(part.cpu().numpy()).all()
    # ... and the good call does write: the target and its partials, not the guards
    assert lib.coevo_dqn16_perturb_dist(*[good[k] for k in order], L._stream()) == 0
    torch.cuda.synchronize()
    words = child.cpu().numpy().view(np.uint32).reshape(3, stride)
    p = part.cpu().numpy()
    assert (words[0] == POISON).all() and (words[2] == POISON).all() and (words[1, :used_words(C, n)] != POISON).all()
    assert np.isnan(p[0]) and np.isnan(p[-1]) and np.isfinite(p[1:-1]).all()


# ---------------------------------------------------------------------------------------------------- whole generations
CONFIGS = {
    "pop3_hof2_adaptive": dict(pop=3, hof=2, E=2, C=4, n=6, T_train=4, T_eval=3, adaptive=True, generations=3, seed=21),
    "pop4_hof1_fixed": dict(pop=4, hof=1, E=1, C=3, n=18, T_train=3, T_eval=2, adaptive=False, generations=2, seed=22),
}
ENV_SEED = 123
SIGMAS = (0.05, 0.08)


def initial(cfg):
    torch.manual_seed(cfg["seed"])
    return dqn_initial_population(cfg["pop"], cfg["hof"], cfg["C"], cfg["n"])


def net_shas(popu, hof, elites):
    return {r: {"pop": [sha(w) for w in popu[r]], "hof": [sha(w) for w in hof[r]], "elite": [sha(w) for w in elites[r]]}
            for r in dk.ROLES}


@functools.lru_cache(maxsize=None)
def checker_run(name):
    """the sequential restatement, computed once per configuration -> per generation the record + the sha256 of every net"""
    cfg = CONFIGS[name]
    pop_flat, hof_flat = initial(cfg)
    st = dk.State(pop_flat, hof_flat)
    args = Bag(mutation_power_agent_0=SIGMAS[0], mutation_power_agent_1=SIGMAS[1], mutation_power_adversary=0.0,
               adaptive=cfg["adaptive"], max_timesteps_per_episode=cfg["T_train"], max_evaluation_steps=cfg["T_eval"])
    out = []
    for gen in range(cfg["generations"]):
        rec = dk.generation(st, gen, args, cfg["E"], cfg["C"], cfg["n"], ENV_SEED, philox_seed=SEED)
        rec["shas"] = net_shas(st.popu, st.hof, st.elites)
        rec["dist"] = {r: st.dist[r].copy() for r in dk.ROLES}
        out.append(rec)
    return out


def make_engine(cfg):
    eng = HalfDQNGAEngine(cfg["pop"], cfg["hof"], cfg["E"], cfg["C"], cfg["n"], cfg["T_train"], cfg["T_eval"], device=DEV,
                          env_seed=ENV_SEED, philox_seed=SEED, first_ordinal=1, capacity=16, sigmas=SIGMAS, sig_min=0.001,
                          sig_max=0.2, adaptive=cfg["adaptive"])
    eng.load_initial(*initial(cfg))
    return eng


def engine_state(eng):
    """everything a generation leaves behind, as comparable python values"""
    torch.cuda.synchronize()
    down = {r: {"pop": eng.download(r, "pop", 0, eng.pop), "hof": eng.download(r, "hof", 0, eng.hof),
                "elite": eng.download(r, "elite", 0, eng.E)} for r in dk.ROLES}
    return {"acc": eng.ro.acc.cpu().numpy()[:, :2].tolist(),
            "fitness": [bits(eng.fitness[ri].cpu().numpy()).tolist() for ri in range(2)],
            "diversity": [int(bits(eng.div[ri].cpu().numpy())[0]) for ri in range(2)],
            "elite_ids": [eng.order[ri][:eng.E].cpu().numpy().astype(int).tolist() for ri in range(2)],
            "sigma": eng.sigma64.cpu().numpy()[:2].tolist(),
            "sigma32": bits(eng.sigma32.cpu().numpy()[:2]).tolist(),
            "dist": [bits(eng.dist_all[ri].cpu().numpy()).tolist() for ri in range(2)],
            "shas": {r: {k: [sha(w) for w in v] for k, v in down[r].items()} for r in dk.ROLES},
            "status": int(eng.ro.status.item()), "gen_dev": int(eng.gen_dev.item())}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_whole_generations_equal_the_checker_and_graph_replay_equals_eager(name):
    cfg = CONFIGS[name]
    want = checker_run(name)
    n_main = 2 * cfg["pop"] * cfg["hof"]
    eng, eager = make_engine(cfg), make_engine(cfg)
    try:
        # generation 0's distances to the stale agent: coevo_dqn16_distance + the finalize in load_initial
        pop_flat, hof_flat = initial(cfg)
        st0 = dk.State(pop_flat, hof_flat)
        torch.cuda.synchronize()
        for ri, r in enumerate(dk.ROLES):
            assert np.array_equal(bits(eng.dist_all[ri].cpu().numpy()), bits(st0.dist[r])), r
            assert st0.dist[r][-1] == 0 and (st0.dist[r][:-1] > 0).all()
        for gen, rec in enumerate(want):
            eng.step(use_graph=True)
            eager.step(use_graph=False)
            got, got_eager = engine_state(eng), engine_state(eager)
            assert got == got_eager, (gen, "graph replay differs from the eager generation")
            assert got["status"] == 0 and got["gen_dev"] == gen + 1
            assert got["acc"][:n_main] == rec["games"], (gen, "reward pairs")
            if gen > 0:   # the evaluation games of generation gen - 1 rode along
                assert got["acc"][n_main:] == want[gen - 1]["eval_games"], (gen, "evaluation reward pairs")
            for ri, r in enumerate(dk.ROLES):
                assert got["fitness"][ri] == bits(rec["fitness"][ri]).tolist(), (gen, r, "fitness")
                assert got["diversity"][ri] == int(bits(rec["diversity"][ri])[0]), (gen, r, "diversity")
                assert got["elite_ids"][ri] == rec["elite_ids"][ri], (gen, r, "elite ids")
                assert got["dist"][ri] == bits(rec["dist"][r]).tolist(), (gen, r, "distances")
            # the sigma rule has seen the evaluation of generation gen - 1: what this generation bred with
            assert got["sigma"] == rec["sigma_before"], (gen, "sigma")
            assert got["sigma32"] == bits(np.array(rec["sigma_before"], dtype=np.float32)).tolist()
            assert got["shas"] == rec["shas"], (gen, "nets")
        if cfg["adaptive"]:
            assert want[-1]["sigma_before"] != list(SIGMAS)
        assert any(any(g) for rec in want for g in rec["games"]), "no hit was credited in any game"
        assert eng.eval_only() == want[-1]["eval_rewards"] == eager.eval_only()
        assert int(eng.ro.status.item()) == 0
    finally:
        eng.close()
        eager.close()
