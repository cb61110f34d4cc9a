"""Cross-play without a GPU: the game tables against a brute-force loop, every refusal before the library is loaded, the third
header (include/coevo_crossplay.h) and its binding, the host-side refusals of its two entry points, and the proof that the
reward tables of tests/crossplay_cases.py can tell the stated summation order from others."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import coevonet_amd
from coevonet_amd import lib as L
from coevonet_amd import population as P
from tests import crossplay_cases as cc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XP = ("coevo_crossplay_reduce", "coevo_mpe_reset_episodes")
GAME_SHAPES = [(1, 1, 1, 1), (2, 3, 2, 3), (3, 1, 2, 2)]


class Names:
    """a net table that answers with the (role, index) it was asked for"""

    def __call__(self, region, role, i=0):
        assert region == "cross"
        return (role, i)


# ------------------------------------------------------------------------------------------------------------ game tables
@pytest.mark.parametrize("shape", GAME_SHAPES)
def test_cross_games_equal_the_brute_force_loop(shape):
    A, B, C, E = shape
    games, episode = P.cross_games(Names(), A, B, C, E)
    want = cc.brute_games(A, B, C, E)
    assert len(games) == len(episode) == len(want) == A * B * C * E
    for g in range(len(games)):
        assert (*games[g], episode[g]) == want[g], g   # slot order (adversary, agent_0, agent_1): RolloutPlan's
    games2, episode2 = P.cross_games2(Names(), A, B, E)
    want2 = cc.brute_games2(A, B, E)
    assert len(games2) == len(want2) == A * B * E
    for g in range(len(games2)):
        assert (*games2[g], episode2[g]) == want2[g], g


def test_cross_games_number_nets_through_the_shared_net_table():
    stride = {r: 100 + 10 * i for i, r in enumerate(P.ROLES)}
    base = {"agent_0": {"cross": 0}, "agent_1": {"cross": 200}, "adversary_0": {"cross": 1000}}
    table = P.NetTable(base, stride, P.ROLE_D)
    games, _ = P.cross_games(table, 2, 1, 3, 2)
    off = lambda role, i: base[role]["cross"] + i * stride[role]   # noqa: E731
    for g, (adv, a0, a1) in enumerate(games):
        t = g // 2
        assert table.net_off[adv] == off("adversary_0", t % 3) and table.net_D[adv] == 8
        assert table.net_off[a0] == off("agent_0", t // 3) and table.net_off[a1] == off("agent_1", 0)
    assert len(table.net_off) == 2 + 1 + 3   # the same weights in two role lists would be two entries


# ------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_comes_before_the_library_is_loaded(monkeypatch):
    from coevonet_amd import crossplay as xp

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(L, "load", no_load)
    f10, f8 = np.zeros(xp.fc_params(10), dtype=np.float32), np.zeros(xp.fc_params(8), dtype=np.float32)
    for kw, msg in (
            (dict(agent_0=[]), "no net for role agent_0"), (dict(agent_1=[]), "no net for role agent_1"),
            (dict(adversary=[]), "no net for role adversary_0"), (dict(adversary=None), "no net for role adversary_0"),
            (dict(episodes=0), "episodes 0"), (dict(episodes=-3), "episodes -3"),
            (dict(agent_0=[f8]), "net 0 of role agent_0 has 138757 parameters, not 139781"),
            (dict(agent_1=[f10, f10[:-1]]), "net 1 of role agent_1"), (dict(adversary=[f10]), "net 0 of role adversary_0"),
            (dict(precision="bfloat16"), "Unsupported precision: bfloat16"), (dict(precision="half"), "Unsupported precision"),
            (dict(agent_0=[f10] * 1024, agent_1=[f10] * 1024, episodes=2), "2097152 games"),
            (dict(agent_0=[f10] * 1025, agent_1=[f10] * 1024, episodes=1), "1049600 games")):
        with pytest.raises(ValueError, match=msg):
            xp.CrossPlay(**{**dict(agent_0=[f10], agent_1=[f10], adversary=[f8]), **kw})
    P46 = xp.dqn_params(4, 6)
    q = np.zeros(P46, dtype=np.float32)
    for kw, msg in (
            (dict(first=[]), "no net for role first_0"), (dict(second=[]), "no net for role second_0"),
            (dict(episodes=0), "episodes 0"), (dict(first=[q[:-1]]), f"net 0 of role first_0 has {P46 - 1} parameters, not {P46}"),
            (dict(second=[q, np.zeros(xp.dqn_params(6, 18), dtype=np.float32)]), "net 1 of role second_0"),
            (dict(precision="bfloat16"), "Unsupported precision: bfloat16"), (dict(limit=None), "a step limit is required"),
            (dict(fc1_layout="rows"), "fc1_layout"), (dict(C=7), "not a DeepQN shape"),
            (dict(first=[q] * 1024, second=[q] * 1025), "1049600 games")):
        with pytest.raises(ValueError, match=msg):
            xp.DQNCrossPlay(**{**dict(first=[q], second=[q], C=4, n_actions=6, episodes=1, limit=6), **kw})
    # a negative first_ordinal is refused by run() before it touches anything
    for cls in (xp.CrossPlay, xp.DQNCrossPlay):
        with pytest.raises(ValueError, match="negative first_ordinal -1"):
            object.__new__(cls).run(-1)
    half = object.__new__(xp.CrossPlay)
    half.episodes = 3
    with pytest.raises(ValueError, match="leaves the 64-bit ordinals"):
        half.run(2 ** 64 - 2)


def test_parameter_counts_without_the_library_equal_the_librarys():
    from coevonet_amd import crossplay as xp
    lib = L.load()
    assert [xp.fc_params(D) for D in (8, 10)] == [lib.coevo_fc_param_count(D) for D in (8, 10)] == [138757, 139781]
    for C, n in ((4, 6), (6, 18), (1, 1), (3, 32)):
        assert xp.dqn_params(C, n) == lib.coevo_dqn_param_count(C, n), (C, n)
    assert xp.MAX_GAMES == 2 ** 20


def test_public_surface_is_lazy_and_complete():
    for name in ("CrossPlay", "DQNCrossPlay", "test_agents", "cross_play_checkpoints"):
        from coevonet_amd import crossplay as xp
        assert getattr(coevonet_amd, name) is getattr(xp, name) and name in coevonet_amd.__all__
    assert {"HalfGAEngine", "HalfESEngine", "DeepQNHalf", "HalfDQNGAEngine", "HalfSynthRollout",
            "HalfDQNESEngine"} <= set(coevonet_amd.__all__)


# ------------------------------------------------------------------------------------------------ header, library, binding
def header_text(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", name)).read(), flags=re.S)


def test_crossplay_symbols_are_declared_exported_and_bound():
    text = header_text("coevo_crossplay.h")
    assert sorted(set(re.findall(r"\b(coevo_[a-z0-9_]+)\s*\(", text))) == sorted(XP) == L.crossplay_symbols()
    assert "typedef" not in text and "struct" not in text
    lib, dll = L.load(), ctypes.CDLL(L.LIB_PATH)
    for name in XP:
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
        assert hasattr(dll, name), f"{name} is not exported by libcoevo.so"
        res, args = L._XP_SIGS[name]
        assert res is ctypes.c_int and getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
    # coevo_mpe_reset's arguments with `episodes` in front of the stream
    reset = L._SIGS["coevo_mpe_reset"]
    assert L._XP_SIGS["coevo_mpe_reset_episodes"] == (reset[0], reset[1][:-1] + [ctypes.c_int, ctypes.c_void_p])
    assert L._XP_SIGS["coevo_crossplay_reduce"][1] == [ctypes.c_void_p] + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 5
    assert L.K_XP == {"COEVO_CROSSPLAY_MAX_GAMES": 2 ** 20}
    # the two other tables are what they were
    declared = sorted(set(re.findall(r"\b(coevo_[a-z0-9_]+)\s*\(", header_text("coevo.h"))))
    assert L.exported_symbols() == declared and len(declared) == 132 and len(L.STRUCTS) == 17
    assert L.extension_symbols() == sorted(set(re.findall(r"\b(coevo_[a-z0-9_]+)\s*\(", header_text("coevo_ext.h"))))
    assert len(L.extension_symbols()) == 6
    assert not set(XP) & (set(L._SIGS) | set(L._EXT_SIGS)) and not set(L.K_XP) & (set(L.K) | set(L.K_EXT))
    assert L.K["COEVO_VERSION"] == 103 == lib.coevo_version()


def test_the_crossplay_header_is_plain_c(tmp_path):
    src = tmp_path / "hdr.c"
    src.write_text('#include "coevo_crossplay.h"\nint main(void) { return coevo_version() + COEVO_CROSSPLAY_MAX_GAMES ? 0 : 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"),
                    "-c", str(src), "-o", str(tmp_path / "hdr.o")], check=True)


def test_the_crossplay_header_may_not_declare_structs_or_repeat_names():
    with pytest.raises(L.CoevoError, match="declares a struct"):
        L._parse_crossplay_header("typedef struct { int32_t n; } coevo_new;")
    for taken in ("int coevo_version(void);", "int coevo_dqn16_relayout(void);", "#define COEVO_DQN16_FC1_SUPER 98",
                  "#define COEVO_OK 0"):
        with pytest.raises(L.CoevoError, match="repeats a name"):
            L._parse_crossplay_header(taken)
    from coevonet_amd.build import SOURCES, _headers
    assert "crossplay.hip" in SOURCES and any(h.endswith("coevo_crossplay.h") for h in _headers())


def test_entry_points_refuse_bad_arguments_on_the_host():
    """COEVO_ERR_ARG comes back before any launch, so these calls need no GPU (the pointers are never followed)"""
    lib = L.load()
    rng = L.PCG64State.from_seed(1)
    buf = np.zeros(4096, dtype=np.float64)
    p = buf.ctypes.data
    at = lambda words: p + 8 * words   # noqa: E731
    ok_reset = dict(state=p, n_games=8, game_first=3, count=5, first_ordinal=0, episodes=2)
    for kw in (dict(state=None), dict(n_games=0), dict(game_first=-1), dict(count=-1), dict(count=6), dict(game_first=9, count=0),
               dict(episodes=0), dict(episodes=-1), dict(game_first=2 ** 31 - 1, count=2 ** 31 - 1)):
        a = {**ok_reset, **kw}
        assert lib.coevo_mpe_reset_episodes(a["state"], a["n_games"], a["game_first"], a["count"], rng, a["first_ordinal"],
                                            a["episodes"], None) == L.K["COEVO_ERR_ARG"], kw
    assert lib.coevo_mpe_reset_episodes(p, 8, 3, 0, rng, 0, 2, None) == 0   # count == 0: OK without a launch
    # rewards [2 * 3 * 2 * 3 = 36][3] = 108 words at 0; outputs behind them
    ok = dict(rewards=at(0), A=2, B=3, C=2, E=3, payoff=at(200), marg_a=at(300), marg_b=at(320), marg_c=at(340))
    big = 2 ** 31 - 1
    for kw in (dict(rewards=None), dict(payoff=None), dict(A=0), dict(B=0), dict(C=-1), dict(E=0),
               dict(A=big, B=big, C=big, E=big), dict(A=715827883, B=1, C=1, E=1), dict(A=1024, B=1024, C=683, E=1),
               dict(payoff=at(0)), dict(payoff=at(107)), dict(payoff=at(-35)), dict(marg_a=at(50)), dict(marg_b=at(107)),
               dict(marg_c=at(-5)), dict(marg_a=at(-5))):
        a = {**ok, **kw}
        assert lib.coevo_crossplay_reduce(a["rewards"], a["A"], a["B"], a["C"], a["E"], a["payoff"], a["marg_a"], a["marg_b"],
                                          a["marg_c"], None) == L.K["COEVO_ERR_ARG"], kw
    assert not buf.any()


# --------------------------------------------------------------------------------------------- the reduction, stated
@pytest.mark.parametrize("shape", cc.SHAPES)
def test_reduction_statement_on_plain_numbers(shape):
    A, B, C, E = shape
    r = np.arange(A * B * C * E * 3, dtype=np.float64).reshape(-1, 3) % 17 - 4     # small integers: every order is exact
    payoff, ma, mb, mc = cc.reduce_ref(r, A, B, C, E)
    p = r.reshape(A, B, C, E, 3).sum(axis=3) / E
    assert np.array_equal(payoff, p.reshape(-1, 3))
    # integer sums over exact quotients need not be exact: compare the marginals' SUMS, which are
    assert np.allclose(ma, p.mean(axis=(1, 2)), rtol=1e-14) and np.allclose(mb, p.mean(axis=(0, 2)), rtol=1e-14)
    assert np.allclose(mc, p.mean(axis=(0, 1)), rtol=1e-14)
    assert ma.shape == (A, 3) and mb.shape == (B, 3) and mc.shape == (C, 3)


def test_the_cancellation_table_tells_the_orders_apart():
    for A, B, C, E in cc.SHAPES:
        r = cc.cancellation_rewards(A, B, C, E)
        want = cc.bits(cc.reduce_ref(r, A, B, C, E)[0])
        if E >= 8:     # np.sum leaves the left-to-right chain from eight terms on
            assert (cc.bits(cc.numpy_sum_payoff(r, A, B, C, E)) != want).any(), (A, B, C, E)
        if E >= 3:
            assert (cc.bits(cc.reversed_payoff(r, A, B, C, E)) != want).any(), (A, B, C, E)
    # the issue's own three terms: 1e16 + 1.0 is 1e16, so the chain ends at 0.0 where the exact sum is 1.0
    assert cc.reduce_ref([[1e16] * 3, [1.0] * 3, [-1e16] * 3], 1, 1, 1, 3)[0].tolist() == [[0.0, 0.0, 0.0]]
    assert cc.reduce_ref([[1e16] * 3, [-1e16] * 3, [1.0] * 3], 1, 1, 1, 3)[0].tolist() == [[1 / 3] * 3]


def test_negative_zeros_end_at_positive_zero():
    for A, B, C, E in cc.SHAPES:
        for out in cc.reduce_ref(cc.negative_zero_rewards(A, B, C, E), A, B, C, E):
            assert not cc.bits(out).any()    # +0.0 everywhere: the chains start from +0.0, not from their first term
