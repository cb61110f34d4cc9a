"""Baseline opponents without a GPU: the scripted-action statement (known answers of the Philox word, the range map), every
refusal before the library is loaded, the sixth header and its binding, the C checker of the PPO policy net against the torch
results recorded in tests/golden/ppo_baseline.npz, and test_agents' unchanged refusal with no opponent."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import coevonet_amd
from coevonet_amd import baselines as bl
from coevonet_amd import crossplay as xp
from coevonet_amd import lib as L
from coevonet_amd.atari_synthetic import philox4x32_10
from tests import baseline_cases as bc
from tests.util import Bag

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BL = ("coevo_baseline_actions", "coevo_mlp_forward_argmax", "coevo_mlp_param_count", "coevo_mlp_slab_stride",
      "coevo_mpe_mlp_policy_cycle")
N_ACTIONS = (1, 5, 6, 18, 32)


# ------------------------------------------------------------------------------------------------------- scripted_action
def test_philox_word_known_answers():
    """Philox4x32-10's published known-answer vectors (Random123 kat_vectors), then the word scripted_action draws"""
    assert [int(w[()]) for w in philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert [int(w[()]) for w in philox4x32_10(0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff)] == \
        [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert [int(w[()]) for w in philox4x32_10(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0)] == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    # counter = (ordinal low, ordinal high, k, slot), key = (seed low, seed high)
    ordinal, seed, k, slot = 0x85a308d3243f6a88, 0x299f31d0a4093822, 0x13198a2e, 0x03707344
    for n in N_ACTIONS:
        assert bl.scripted_action(bl.RANDOM, 0, seed, ordinal, slot, k, n) == (0xd16cfe09 * n) >> 32
        assert bl.scripted_action(bl.RANDOM, 0, 0, 0, 0, 0, n) == (0x6627e8d5 * n) >> 32
        assert bl.scripted_action(bl.RANDOM, 0, 2 ** 64 - 1, 2 ** 64 - 1, 0xffffffff, 0xffffffff, n) == (0x408f276d * n) >> 32


@pytest.mark.parametrize("n", N_ACTIONS)
def test_range_map(n):
    """(w * n) >> 32 in 64 bits: 0 at w = 0, n - 1 at w = 2**32 - 1, every action reached, never n"""
    seen = set()
    for ordinal in range(40):
        for k in (0, 1, 24, 2 ** 31 - 1):
            for slot in range(3):
                a = bl.scripted_action(bl.RANDOM, 0, 7, ordinal, slot, k, n)
                w = int(philox4x32_10(ordinal, 0, k, slot, 7, 0)[0])
                assert a == w * n // 2 ** 32 and 0 <= a < n
                seen.add(a)
    assert seen == set(range(n))
    assert (0 * n) >> 32 == 0 and ((2 ** 32 - 1) * n) >> 32 == n - 1
    for k in (0, 1, n - 1, n, 24, 2 ** 31 - 1):
        assert bl.scripted_action(bl.PERIODIC, 3, 0, 9, 1, k, n) == (3 + k) % n
        assert bl.PeriodicBaseline(3).action(9, 1, k, n) == (3 + k) % n
    assert bl.scripted_action(bl.CONSTANT, n - 1, 0, 9, 1, 5, n) == n - 1
    for bad in (-1, n):
        with pytest.raises(ValueError, match="constant action"):
            bl.scripted_action(bl.CONSTANT, bad, 0, 0, 0, 0, n)


def test_two_random_seats_of_one_game_differ_through_the_slot_and_not_through_the_table():
    b = bl.RandomBaseline(5)
    a = [[b.action(3, slot, k, 5) for k in range(25)] for slot in range(3)]
    assert a[0] != a[1] != a[2] and a[0] != a[2]
    assert a[1] == [bl.RandomBaseline(5).action(3, 1, k, 5) for k in range(25)]      # the episode alone decides
    assert a[1] != [b.action(4, 1, k, 5) for k in range(25)] and a[1] != [bl.RandomBaseline(6).action(3, 1, k, 5) for k in range(25)]
    assert bl.AlwaysFire.kind == bl.CONSTANT and bl.AlwaysFire.arg == 1 and bl.AlwaysFire.action(0, 0, 7, 6) == 1


# ------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_comes_before_the_library_is_loaded(monkeypatch):
    from coevonet_amd.deepqn import DeepQNHalf
    from coevonet_amd.fcnetwork import FCNetworkHalf
    half_fc, half_q = FCNetworkHalf(10, 5), DeepQNHalf(4, 6)      # (their constructors may load the library: built first)

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(L, "load", no_load)
    f10, f8 = np.zeros(xp.fc_params(10), dtype=np.float32), np.zeros(xp.fc_params(8), dtype=np.float32)
    m10, m8 = bl.MLPBaseline(np.zeros(5189, dtype=np.float32), 10), bl.MLPBaseline(np.zeros(5061, dtype=np.float32), 8)
    for kw, msg in (
            (dict(agent_0=[]), "no seat for role agent_0"), (dict(adversary=None), "no seat for role adversary_0"),
            (dict(episodes=0), "episodes 0"), (dict(precision="float16"), "float32 evolved nets only"),
            (dict(precision="bfloat16"), "float32 evolved nets only"),
            (dict(agent_1=[half_fc]), "seat 0 of role agent_1 is a float16 net"),
            (dict(agent_0=[f8]), "net 0 of role agent_0 has 138757 parameters, not 139781"),
            (dict(agent_1=[bl.RandomBaseline(), f10[:-1]]), "net 1 of role agent_1"),
            (dict(adversary=[m10]), "seat 0 of role adversary_0 is a policy net of width 10, not 8"),
            (dict(agent_0=[f10, m8]), "seat 1 of role agent_0 is a policy net of width 8, not 10"),
            (dict(agent_1=[bl.ConstantBaseline(5)]), "seat 0 of role agent_1: constant action 5 outside 0 .. 4"),
            (dict(agent_0=[bl.RandomBaseline()] * 1024, agent_1=[f10] * 1024, episodes=2), "2097152 games"),
            (dict(agent_0=[m10] * 1025, agent_1=[bl.AlwaysFire] * 1024, episodes=1), "1049600 games")):
        with pytest.raises(ValueError, match=msg):
            bl.BaselineCrossPlay(**{**dict(agent_0=[f10], agent_1=[m10], adversary=[bl.RandomBaseline()]), **kw})
    for args, msg in (((np.zeros(5189), 8), "5189 parameters, not 5061"), ((np.zeros(5061), 10), "not 5189"),
                      ((np.zeros(5189), 12), "observation width 12")):
        with pytest.raises(ValueError, match=msg):
            bl.MLPBaseline(*args)
    for make in (lambda: bl.ConstantBaseline(-1), lambda: bl.ConstantBaseline(32), lambda: bl.PeriodicBaseline(-1),
                 lambda: bl.RandomBaseline(-1), lambda: bl.RandomBaseline(2 ** 64)):
        with pytest.raises(ValueError):
            make()
    P46 = xp.dqn_params(4, 6)
    q, r = np.zeros(P46, dtype=np.float32), bl.RandomBaseline()
    for kw, msg in (
            (dict(first=[]), "no seat for role first_0"), (dict(second=[m10]), "an MLPBaseline is a simple_adversary policy"),
            (dict(second=[r, q]), "role second_0 mixes nets and scripted baselines"), (dict(first=[r]), "both sides are scripted"),
            (dict(second=[q]), "no scripted side"), (dict(episodes=0), "episodes 0"), (dict(limit=None), "a step limit is required"),
            (dict(limit=-1), "negative step limit"), (dict(precision="float16"), "float32 only"), (dict(C=7), "not a DeepQN shape"),
            (dict(n_actions=33), "not a DeepQN shape"), (dict(fc1_layout="rows"), "fc1_layout"),
            (dict(first=[q[:-1]]), f"net 0 of role first_0 has {P46 - 1} parameters, not {P46}"),
            (dict(first=[half_q]), "net 0 of role first_0 is a float16 net"),
            (dict(second=[bl.ConstantBaseline(6)]), "seat 0 of role second_0: constant action 6 outside 0 .. 5"),
            (dict(first=[q] * 1025, second=[r] * 1024), "1049600 games")):
        with pytest.raises(ValueError, match=msg):
            bl.DQNBaselineCrossPlay(**{**dict(first=[q], second=[r], C=4, n_actions=6, episodes=1, limit=6), **kw})
    for cls in (bl.BaselineCrossPlay, bl.DQNBaselineCrossPlay):
        with pytest.raises(ValueError, match="negative first_ordinal -1"):
            object.__new__(cls).run(-1)


def test_test_agents_without_an_opponent_refuses_as_before(monkeypatch):
    """opponent=None is today's behaviour: the Atari path still names play_against_yourself, and a wrong opponent is refused"""
    from coevonet_amd import game_logic as gl
    monkeypatch.setattr(L, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    args = Bag(algorithm="GA", game="pong_v3", max_evaluation_steps=6, play_against_yourself=False, test=True)
    env = gl.initialize_env(args)
    for kw in ({}, dict(opponent=None)):
        with pytest.raises(ValueError) as e:
            xp.test_agents(env, args, **kw)
        assert str(e.value) == ("test_agents: the Atari games are tested with args.play_against_yourself only (the random dummy "
                                "opponent is not built)")
    m10 = bl.MLPBaseline(np.zeros(5189, dtype=np.float32), 10)
    with pytest.raises(ValueError, match="`opponent` is a scripted baseline"):
        xp.test_agents(env, args, opponent=m10)
    mpe_args = Bag(algorithm="GA", max_evaluation_steps=6, test=True)
    mpe_env = gl.initialize_env(mpe_args)
    for bad in (bl.RandomBaseline(), {}, {"first_0": bl.RandomBaseline()}, {"agent_0": 3}):
        with pytest.raises(ValueError, match="role: baseline"):
            xp.test_agents(mpe_env, mpe_args, opponent=bad)
    assert env.n_resets == 1 and mpe_env.n_resets == 1      # refused before a reset was taken


def test_public_surface():
    for name in ("BaselineCrossPlay", "DQNBaselineCrossPlay", "RandomBaseline", "PeriodicBaseline", "ConstantBaseline",
                 "AlwaysFire", "MLPBaseline", "load_ppo_baseline"):
        assert getattr(coevonet_amd, name) is getattr(bl, name) and name in coevonet_amd.__all__
    assert [bl.mlp_params(D) for D in (10, 8)] == [5189, 5061] == [L.load().coevo_mlp_param_count(D) for D in (10, 8)]
    assert [bl.mlp_stride(D) for D in (10, 8)] == [5192, 5064] == [L.load().coevo_mlp_slab_stride(D) for D in (10, 8)]
    assert L.load().coevo_mlp_param_count(9) == L.K["COEVO_ERR_ARG"] == L.load().coevo_mlp_slab_stride(12)


# ------------------------------------------------------------------------------------------------ header, library, binding
def header_text(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", name)).read(), flags=re.S)


def test_baseline_symbols_are_declared_exported_and_bound():
    text = header_text("coevo_baseline.h")
    assert sorted(set(re.findall(r"\b(coevo_[a-z0-9_]+)\s*\(", text))) == sorted(BL) == L.baseline_symbols()
    assert "typedef" not in text and "struct" not in text
    lib, dll = L.load(), ctypes.CDLL(L.LIB_PATH)
    for name in BL:
        assert hasattr(dll, name), f"{name} is not exported by libcoevo.so"
        res, args = L._BL_SIGS[name]
        assert res is ctypes.c_int and getattr(lib, name).restype is res and getattr(lib, name).argtypes == args
    others = set(L._SIGS) | set(L._EXT_SIGS) | set(L._XP_SIGS) | set(L._SH_SIGS) | set(L._SH16_SIGS)
    assert not set(BL) & others and not set(L.K_BL) & (set(L.K) | set(L.K_EXT) | set(L.K_XP) | set(L.K_SH))
    assert L.K_BL == {"COEVO_BL_RANDOM": 0, "COEVO_BL_PERIODIC": 1, "COEVO_BL_CONSTANT": 2, "COEVO_BL_SEAT_WORDS": 8,
                      "COEVO_MLP_H": 64, "COEVO_MLP_NACT": 5, "COEVO_MLP_ROW_TILE": 256, "COEVO_MLP_TASK_WORDS": 4,
                      "COEVO_MLP_SEAT_WORDS": 4}
    # the pinned ABI is what it was
    declared = sorted(set(re.findall(r"\b(coevo_[a-z0-9_]+)\s*\(", header_text("coevo.h"))))
    assert L.exported_symbols() == declared and len(declared) == 132 and len(L.STRUCTS) == 17
    assert L.K["COEVO_VERSION"] == 103 == lib.coevo_version()
    with pytest.raises(L.CoevoError, match="declares a struct"):
        L._parse_baseline_header("typedef struct { int32_t n; } coevo_new;")
    for taken in ("int coevo_version(void);", "int coevo_crossplay_reduce(void);", "#define COEVO_OK 0",
                  "#define COEVO_CROSSPLAY_MAX_GAMES 4"):
        with pytest.raises(L.CoevoError, match="repeats a name"):
            L._parse_baseline_header(taken)
    from coevonet_amd.build import SOURCES, _headers
    assert "baseline.hip" in SOURCES and any(h.endswith("coevo_baseline.h") for h in _headers())


def test_the_baseline_header_is_plain_c(tmp_path):
    src = tmp_path / "hdr.c"
    src.write_text('#include "coevo_baseline.h"\nint main(void) { return coevo_version() + COEVO_MLP_ROW_TILE ? 0 : 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"),
                    "-c", str(src), "-o", str(tmp_path / "hdr.o")], check=True)


def test_entry_points_refuse_bad_arguments_on_the_host():
    """COEVO_ERR_ARG comes back before any launch, so these calls need no GPU (the pointers are never followed)"""
    lib, ERR = L.load(), L.K["COEVO_ERR_ARG"]
    buf = np.zeros(4096, dtype=np.float64)
    p = buf.ctypes.data
    ok = dict(seats=p, n_seats=3, ordinals=p + 1024, add=0, n_games=4, k=0, n_actions=5, actions=p + 2048, n_rows=12)
    for kw in (dict(seats=None), dict(ordinals=None), dict(actions=None), dict(n_seats=-1), dict(n_games=0), dict(n_rows=0),
               dict(n_actions=0), dict(n_actions=33)):
        a = {**ok, **kw}
        assert lib.coevo_baseline_actions(a["seats"], a["n_seats"], a["ordinals"], a["add"], a["n_games"], a["k"], a["n_actions"],
                                          a["actions"], a["n_rows"], None) == ERR, kw
    assert lib.coevo_baseline_actions(p, 0, p, 0, 4, 0, 5, p, 12, None) == 0      # no seat: OK without a launch
    ok = dict(nets=p, floats=5192, tasks=p + 2048, n_tasks=1, obs=p + 4096, n_rows=4, actions=p + 8192, status=p + 9000)
    for kw in (dict(nets=None), dict(nets=p + 4), dict(floats=0), dict(tasks=None), dict(obs=None), dict(actions=None),
               dict(status=None), dict(n_tasks=-1), dict(n_rows=0)):
        a = {**ok, **kw}
        assert lib.coevo_mlp_forward_argmax(a["nets"], a["floats"], a["tasks"], a["n_tasks"], a["obs"], a["n_rows"], a["actions"],
                                            None, a["status"], None) == ERR, kw
        assert lib.coevo_mpe_mlp_policy_cycle(a["nets"], a["floats"], a["tasks"], a["n_tasks"], a["obs"], a["n_rows"], p, 4,
                                              a["actions"], 12, None, a["status"], None) == ERR, kw
    assert lib.coevo_mlp_forward_argmax(p, 5192, p, 0, p, 4, p, None, p, None) == 0
    assert lib.coevo_mpe_mlp_policy_cycle(p, 5192, p, 1, p, 4, None, 4, p, 12, None, p, None) == ERR   # no state
    assert not buf.any()


# ------------------------------------------------------------------------- the checker against the recorded torch results
@pytest.mark.parametrize("role", bc.ROLES)
def test_checker_equals_torch_where_the_margin_allows(role):
    """Actions are equal on every row whose top-two logit margin in the checker is at least 8 x the recorded max |dlogit|; at
    most 1 % of the rows may fall below that margin and be left out.  Recorded over 4096 uniform(-2, 2) rows per role: max
    |dlogit| 1.4e-6 .. 2.9e-6, no row below the margin, no mismatch; the fixture stores the first 256 rows."""
    f = bc.fixture()[role]
    D = bc.ROLE_D[role]
    assert f["flat"].dtype == np.float32 and f["flat"].size == bl.mlp_params(D) and f["obs"].shape == (256, D)
    actions, logits, st = bc.mlp_rows(f["flat"], D, f["obs"])
    assert not st.any()
    dmax = float(f["max_dlogit"])
    assert 0 < dmax < 1e-5
    assert np.abs(logits.astype(np.float64) - f["logits"].astype(np.float64)).max() <= dmax   # the stored rows are among the 4096
    top = np.sort(logits.astype(np.float64), axis=1)
    clear = top[:, -1] - top[:, -2] >= 8 * dmax
    assert (~clear).sum() <= 0.01 * len(clear)
    assert np.array_equal(actions[clear], f["actions"][clear])
    assert np.array_equal(np.argmax(f["logits"], axis=1)[clear], f["actions"][clear])   # argmax(softmax) agrees with first-max


def test_checker_on_the_crafted_nets():
    for D in (8, 10):
        obs = bc.uniform_obs(5, seed=D)
        a, lo, st = bc.mlp_rows(bc.crafted("all_zero", D), D, obs)
        assert not a.any() and not lo.any() and not st.any() and not np.signbit(lo).any()
        a, lo, st = bc.mlp_rows(bc.crafted("tie", D), D, obs)
        assert (a == 2).all() and np.array_equal(lo, np.tile(np.float32([0, 0, 1, 0, 1]), (5, 1))) and not st.any()
        a, lo, st = bc.mlp_rows(bc.crafted("dead", D), D, obs)
        assert (a == 3).all() and np.array_equal(lo, np.tile(np.float32([0.25, -1.5, 0.75, 3.0, 0.0]), (5, 1))) and not st.any()
        flat, (W1, b1, W2, b2, W3, b3) = bc.parts(D, bc.random_net(D, 5))
        for view, at, bit in ((0, (3, 2), "fc1"), (2, (9, 9), "fc2"), (4, (4, 0), "out")):
            net = flat.copy()
            bc.parts(D, net)[1][view][at] = np.nan
            a, lo, st = bc.mlp_rows(net, D, obs)
            assert (st & bc.ST[bit]).all() and not a.any(), bit
        bad = obs.copy()
        bad[2, 1] = np.inf
        a, lo, st = bc.mlp_rows(flat, D, bad)
        assert st[2] & bc.ST["input"] and a[2] == 0 and not st[[0, 1, 3, 4]].any()


def test_from_state_dict_takes_the_policy_and_drops_the_value_head():
    import torch
    f = bc.fixture()["adversary_0"]
    _, (W1, b1, W2, b2, W3, b3) = bc.parts(8, f["flat"].copy())
    sd = {"fc1.weight": torch.from_numpy(W1), "fc1.bias": torch.from_numpy(b1), "fc2.weight": torch.from_numpy(W2),
          "fc2.bias": torch.from_numpy(b2), "policy_head.weight": torch.from_numpy(W3), "policy_head.bias": torch.from_numpy(b3),
          "value_head.weight": torch.zeros(1, 64), "value_head.bias": torch.zeros(1)}
    m = bl.MLPBaseline.from_state_dict(sd)
    assert m.D == 8 and np.array_equal(m.flat, f["flat"])
    with pytest.raises(ValueError, match="no policy_head.bias"):
        bl.MLPBaseline.from_state_dict({k: v for k, v in sd.items() if k != "policy_head.bias"})
    with pytest.raises(ValueError, match="not a D -> 64 -> 64 -> 5 policy"):
        bl.MLPBaseline.from_state_dict({**sd, "fc2.weight": torch.zeros(64, 32)})
