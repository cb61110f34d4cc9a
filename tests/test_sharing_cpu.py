"""The Co-GA extension modes hof_mean / population_sharing without a GPU: the fourth header (include/coevo_sharing.h) and its
binding, every host-side refusal (entry points, engine, trainers - the latter before the library is loaded), the numpy
statements of tests/sharing_cases.py against the oracle and against each other, and the proof that the engine test of
tests/test_sharing_gpu.py can tell the modes apart."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from coevonet_amd import lib as L
from oracle import ref_port as rp
from tests import ga16_checker as gk
from tests import select_cases as sc
from tests import sharing_cases as S
from tests.util import Bag

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SH = ("coevo_fc_pairwise_distance", "coevo_fc_pairwise_scratch_doubles", "coevo_ga_fitness_shared", "coevo_niche_counts")
ERR_ARG = L.K["COEVO_ERR_ARG"]


def header_text(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", name)).read(), flags=re.S)


# ------------------------------------------------------------------------------------------------ header, library, binding
def test_sharing_symbols_are_declared_exported_and_bound():
    text = header_text("coevo_sharing.h")
    assert sorted(set(re.findall(r"\b(coevo_[a-z0-9_]+)\s*\(", text))) == sorted(SH) == L.sharing_symbols()
    assert "typedef" not in text and "struct" not in text
    lib, dll = L.load(), ctypes.CDLL(L.LIB_PATH)
    for name in SH:
        assert hasattr(dll, name), f"{name} is not exported by libcoevo.so"
        res, args = L._SH_SIGS[name]
        assert getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
    i, p = ctypes.c_int, ctypes.c_void_p
    assert L._SH_SIGS == {"coevo_fc_pairwise_scratch_doubles": (ctypes.c_int64, [i, i]),
                          "coevo_fc_pairwise_distance": (i, [p, i, i, p, p, p]),
                          "coevo_niche_counts": (i, [p, i, p, p]),
                          "coevo_ga_fitness_shared": (i, [p] + [i] * 6 + [p, p, p])}
    assert L.K_SH == {"COEVO_SHARING_MAX_POP": 4096, "COEVO_FIT_HOF_MEAN": S.HOF_MEAN, "COEVO_FIT_PER_INDIVIDUAL": S.PER_INDIVIDUAL}
    # coevo_ga_fitness's arguments with `flags` in front of the share
    old = L._SIGS["coevo_ga_fitness"]
    assert L._SH_SIGS["coevo_ga_fitness_shared"] == (old[0], old[1][:6] + [i] + old[1][6:])
    # the three other tables are what they were
    assert len(L.exported_symbols()) == 132 and len(L.STRUCTS) == 17 and len(L.extension_symbols()) == 6
    assert len(L.crossplay_symbols()) == 2
    assert not set(SH) & (set(L._SIGS) | set(L._EXT_SIGS) | set(L._XP_SIGS))
    assert not set(L.K_SH) & (set(L.K) | set(L.K_EXT) | set(L.K_XP))
    assert L.K["COEVO_VERSION"] == 103 == lib.coevo_version()


def test_the_sharing_header_is_plain_c(tmp_path):
    src = tmp_path / "hdr.c"
    src.write_text('#include "coevo_sharing.h"\nint main(void) { return coevo_version() + COEVO_SHARING_MAX_POP + '
                   'COEVO_FIT_HOF_MEAN + COEVO_FIT_PER_INDIVIDUAL ? 0 : 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"),
                    "-c", str(src), "-o", str(tmp_path / "hdr.o")], check=True)


def test_the_sharing_header_may_not_declare_structs_or_repeat_names():
    with pytest.raises(L.CoevoError, match="declares a struct"):
        L._parse_sharing_header("typedef struct { int32_t n; } coevo_new;")
    for taken in ("int coevo_version(void);", "int coevo_dqn16_relayout(void);", "int coevo_crossplay_reduce(void);",
                  "#define COEVO_OK 0", "#define COEVO_DQN16_FC1_SUPER 98", "#define COEVO_CROSSPLAY_MAX_GAMES 5"):
        with pytest.raises(L.CoevoError, match="repeats a name"):
            L._parse_sharing_header(taken)
    from coevonet_amd.build import SOURCES, _headers
    assert "sharing.hip" in SOURCES and any(h.endswith("coevo_sharing.h") for h in _headers())


# ------------------------------------------------------------------------------------------------ refusals
def test_entry_points_refuse_bad_arguments_on_the_host():
    """COEVO_ERR_ARG comes back before any launch, so these calls need no GPU (the pointers are never followed)"""
    lib = L.load()
    buf = np.zeros(4096, dtype=np.float64)
    p = buf.ctypes.data
    assert p % 16 == 0
    assert [lib.coevo_fc_pairwise_scratch_doubles(n, D) for n, D in ((0, 10), (-1, 8), (4097, 10), (8, 9), (8, 0))] == [-1] * 5
    for n in (1, 2, 31, 32, 33, 65, 200, 4096):
        for D in (8, 10):
            m = lib.coevo_fc_pairwise_scratch_doubles(n, D)
            assert m > 0 and m % (n * n) == 0 and 1 <= m // (n * n) <= 64, (n, D)
    assert lib.coevo_fc_pairwise_scratch_doubles(4096, 10) == 4096 * 4096    # one slab: the tile pairs alone fill the device
    ok = dict(slab=p, n=8, D=10, scratch=p + 1024, dist=p + 2048)
    for kw in (dict(slab=None), dict(scratch=None), dict(dist=None), dict(n=0), dict(n=-3), dict(n=4097), dict(D=9), dict(D=0),
               dict(slab=p + 4), dict(slab=p + 8), dict(scratch=p + 1028)):
        a = {**ok, **kw}
        assert lib.coevo_fc_pairwise_distance(a["slab"], a["n"], a["D"], a["scratch"], a["dist"], None) == ERR_ARG, kw
    for kw in (dict(dist=None), dict(niche=None), dict(n=0), dict(n=4097)):
        a = {**dict(dist=p, n=8, niche=p + 1024), **kw}
        assert lib.coevo_niche_counts(a["dist"], a["n"], a["niche"], None) == ERR_ARG, kw
    ok = dict(rewards=p, game_first=0, pop=8, gpi=3, hof=3, slot=1, flags=3, share=p + 1024, fitness=p + 2048)
    big = 2 ** 31 - 1
    for kw in (dict(rewards=None), dict(share=None), dict(fitness=None), dict(pop=0), dict(gpi=0), dict(hof=0), dict(slot=-1),
               dict(slot=3), dict(game_first=-1), dict(flags=4), dict(flags=-1), dict(flags=7), dict(pop=big, gpi=2),
               dict(game_first=big, pop=1, gpi=1)):
        a = {**ok, **kw}
        assert lib.coevo_ga_fitness_shared(a["rewards"], a["game_first"], a["pop"], a["gpi"], a["hof"], a["slot"], a["flags"],
                                           a["share"], a["fitness"], None) == ERR_ARG, kw
    assert not buf.any()


class Ctx:
    """the two attributes and the gather callback of a coevonet_amd.dist context that a trainer reads"""
    rank, world = 0, 2

    def gather_ga(self, eng):
        raise AssertionError("nothing to gather: the trainer refuses first")


def test_engine_and_trainers_refuse_before_the_library_is_loaded(monkeypatch):
    from coevonet_amd import dqn_population as dq
    from coevonet_amd import genetic_algorithm as ga

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(L, "load", no_load)
    for modes in (dict(hof_mean=True), dict(population_sharing=True), dict(hof_mean=True, population_sharing=True)):
        with pytest.raises(ValueError, match=r"one rank only, not shard \(1, 2\)"):
            ga.GAEngine(8, 3, 2, shard=(1, 2), **modes)
        with pytest.raises(ValueError, match=r"one rank only, not shard \(0, 2\)"):
            ga.GAEngine(8, 3, 2, shard=(0, 2), **modes)
        with pytest.raises(ValueError, match="at most 4096 individuals, not 4097"):
            ga.GAEngine(4097, 3, 2, **modes)
    for modes in (dict(population_sharing=True), dict(hof_mean=True, population_sharing=True)):
        with pytest.raises(ValueError, match='population_sharing needs rng="device_philox"'):
            ga.GAEngine(8, 3, 2, rng="host_reference", **modes)
    # hof_mean alone runs over the host's breeding: it gets as far as the library
    with pytest.raises(AssertionError, match="the library was loaded"):
        ga.GAEngine(8, 3, 2, rng="host_reference", hof_mean=True)
    # ... and with both off nothing is refused: a shard, the host's breeding
    with pytest.raises(AssertionError, match="the library was loaded"):
        ga.GAEngine(8, 3, 2, rng="host_reference", shard=(1, 2))
    # the trainer
    for attr in ("coevo_hof_mean", "coevo_population_sharing"):
        args = Bag(population=8, hof_size=3, **{attr: True})
        with pytest.raises(ValueError, match=r"one rank only, not shard \(0, 2\)"):
            ga.GATrainer(None, args, rng="device_philox", dist_ctx=Ctx())
        with pytest.raises(ValueError, match="at most 4096 individuals, not 5000"):
            ga.GATrainer(None, Bag(population=5000, hof_size=3, **{attr: True}), rng="device_philox")
        half = Bag(population=8, hof_size=3, precision="float16", **{attr: True})
        with pytest.raises(ValueError, match=f"Co-GA training with precision float16 is not built with args.{attr}"):
            ga.GATrainer(None, half, rng="device_philox")
        for cls, what in ((dq.DQNGATrainer, "DeepQN Co-GA training"), (dq.DQNESTrainer, "DeepQN Co-ES training")):
            for precision in ("float32", "float16"):
                with pytest.raises(ValueError, match=f"{what} is not built with args.{attr}"):
                    cls(None, Bag(game="pong_v3", precision=precision, **{attr: True}))
    with pytest.raises(ValueError, match='population_sharing needs rng="device_philox"'):
        ga.GATrainer(None, Bag(population=8, hof_size=3, coevo_population_sharing=True))   # (the default rng: host_reference)


# ------------------------------------------------------------------------------------------------ the statements
@pytest.mark.parametrize("D", [8, 10])
def test_pairwise_rows_equal_the_oracles_distances(D):
    """row i of pairwise() = oracle_diversity's distances of every net to net i (its own sequential fp64 sum: the inputs are
    order-proof), bits symmetric, diagonal +0.0"""
    n = 7
    w, want = S.crafted(D, "plain", n)
    assert S.pairwise_order_proof(w, D)
    d = S.pairwise(w, D)
    assert np.array_equal(S.bits32(d), S.bits32(want))
    segs = rp.linear_segments(D)
    so, sl = np.array([s[0] for s in segs], dtype=np.int32), np.array([s[1] for s in segs], dtype=np.int32)
    fn = rp.lib().oracle_diversity
    for i in range(n):
        back = np.zeros(n, dtype=np.float32)
        fn(rp._fp(w[i]), rp._fp(w), n, ctypes.c_size_t(w.shape[1]), rp._ip(so), rp._ip(sl), len(segs), rp._fp(back))
        assert np.array_equal(S.bits32(back), S.bits32(d[i])), i
        # ... and select_cases' fsum statement of the same distance
        assert np.array_equal(S.bits32([sc.contract_dist(w[i], x, D) for x in w]), S.bits32(d[i])), i
    assert np.array_equal(S.bits32(d), S.bits32(d.T)) and not S.bits32(np.diag(d)).any()


@pytest.mark.parametrize("D", [8, 10])
def test_crafted_nets_state_what_they_mean(D):
    n = 5
    plain = S.crafted(D, "plain", n)[1]
    w, want = S.crafted(D, "identical", n)
    assert np.array_equal(S.bits32(S.pairwise(w, D)), S.bits32(want)) and S.bits32(want[0, n - 1]) == 0
    w, want = S.crafted(D, "layernorm", n)        # LayerNorm entries of 1e30 / NaN / inf: the distances of the plain nets
    assert np.isnan(w).any() and np.array_equal(S.bits32(want), S.bits32(plain))
    assert np.array_equal(S.bits32(S.pairwise(w, D)), S.bits32(plain))
    w, want = S.crafted(D, "inf", n)
    k = n // 2
    assert np.array_equal(S.bits32(S.pairwise(w, D)), S.bits32(want))
    assert np.isinf(np.delete(want[k], k)).all() and np.isinf(np.delete(want[:, k], k)).all() and S.bits32(want[k, k]) == 0
    assert np.isfinite(np.delete(np.delete(want, k, 0), k, 1)).all()


def test_niche_statement():
    d = S.expected(10)[:6, :6]
    got = S.niche(d)
    for i in range(6):   # numpy's own expression of diversity_penalty on the row, the self term included
        assert got[i] == pytest.approx(float(sc.np_score(d[i])), rel=1e-6)
        assert sc.same_f32(got[i], sc.contract_score(d[i]))
    assert np.isnan(S.niche(S.niche_matrix("single"))).all() and np.isnan(S.niche(S.niche_matrix("zeros"))).all()
    inf = S.niche(S.niche_matrix("one_inf"))
    assert np.isnan(inf[[1, 4]]).all() and np.isfinite(np.delete(inf, [1, 4])).all()   # inf / inf in the two rows that hold it
    assert S.niche_matrix("n257").shape == (257, 257) and np.isfinite(S.niche(S.niche_matrix("n257"))).all()
    assert all(S.niche_order_proof(S.niche_matrix(k)) for k in S.NICHE_CRAFTED)


def test_fitness_statement_and_the_cancellation_table():
    g = np.random.Generator(np.random.PCG64(5))
    pop, gpi = 6, 3
    r = -g.random((4 + pop * gpi, 3)) * 20
    share = (g.random(pop) * 2).astype(np.float32)
    for hof in (1, 3, 5):
        for slot in range(3):
            # flags 0: the expression every other checker uses for coevo_ga_fitness
            assert np.array_equal(S.bits32(S.fitness(r, gpi, hof, slot, 0, share[:1], game_first=4)),
                                  S.bits32(sc.np_fitness(r, 4, pop, gpi, hof, slot, share[0])))
            assert np.array_equal(S.bits32(S.fitness(r, gpi, hof, slot, 0, share[:1], game_first=4)),
                                  S.bits32(gk.fitness(r[4:].reshape(pop, gpi, 3)[:, -1, slot], hof, share[0])))
            both = S.fitness(r, gpi, hof, slot, S.HOF_MEAN | S.PER_INDIVIDUAL, share, game_first=4)
            want = (r[4:].reshape(pop, gpi, 3)[:, :, slot].sum(axis=1) / hof).astype(np.float32) / (1 + share)
            np.testing.assert_allclose(both, want, rtol=3e-7)
    # the cancellation table: a right-to-left sum gives other bits
    share8 = (g.random(8) * 2).astype(np.float32)   # (eight individuals: every start in the pattern, in every slot)
    for hof in (3, 5):
        c = S.cancellation_rewards(8, hof)
        for slot in range(3):
            fwd = S.fitness(c, hof, hof, slot, S.HOF_MEAN | S.PER_INDIVIDUAL, share8)
            assert (S.bits32(fwd) != S.bits32(S.fitness_reversed(c, hof, hof, slot, share8))).any(), (hof, slot)
    # the issue's own three terms: 1e16 + 1.0 is 1e16, so the ascending chain ends at 0.0 where the exact sum is 1.0
    assert S.fitness([[1e16] * 3, [1.0] * 3, [-1e16] * 3], 3, 3, 0, S.HOF_MEAN, [0.0]).tolist() == [0.0]
    assert S.fitness([[1e16] * 3, [-1e16] * 3, [1.0] * 3], 3, 3, 0, S.HOF_MEAN, [0.0]).tolist() == [np.float32(1 / 3)]
    # a chain that starts from +0.0 ends at +0.0 on games of -0.0
    assert not S.bits32(S.fitness(np.full((3, 3), -0.0), 3, 3, 0, S.HOF_MEAN, [0.0])).any()


def test_the_engine_tests_configuration_tells_the_modes_apart():
    """on generation 0's games, played by the oracle for the engine test's seeded configuration, each of the three mode pairs
    chooses other elites than the reference mode in at least one role"""
    E = S.ENGINE
    hof, pop = S.engine_initial()
    rew = S.oracle_generation0_rewards(hof, pop)
    per = E["pop"] * E["hof"]
    assert rew.shape == (3 * per, 3)
    differs = {m: [] for m in S.MODES}
    for ri, r in enumerate(rp.ROLES):
        D = rp.ROLE_D[r]
        mine = rew[ri * per:(ri + 1) * per]
        stale = S.stale_distances(pop[r], pop[r][-1], D)
        ref = gk.rank_desc(gk.fitness(mine.reshape(E["pop"], E["hof"], 3)[:, -1, ri], E["hof"], gk.sharing_score(stale)))
        for m in S.MODES:
            t = S.generation_tail(mine, pop[r], stale, D, ri, 0, E["hof"], E["elites"], E["sigma"], E["philox_seed"], *m)
            differs[m].append(t["elite_ids"] != ref[:E["elites"]])
            if m[1]:   # a niche of four around individual 0, loners elsewhere
                assert (t["niche"][[0, *S.CLUSTER]] > 2).all() and (np.delete(t["niche"], [0, *S.CLUSTER]) == 1).all()
    assert all(any(v) for v in differs.values()), differs
