"""Statements for the baseline gauntlet (include/coevo_gauntlet.h, coevonet_amd/gauntlet.py): match lists that hold every
seat kind in every slot, the game words they must give, and the trainer's spec.  No GPU, no device library."""
import functools

import numpy as np

from coevonet_amd import baselines as bl
from coevonet_amd import gauntlet as gt
from coevonet_amd.crossplay import fc_params
from tests import baseline_cases as bc

TRIO = ("agent_0", "agent_1", "adversary_0")
FC, MLP = 3, 4
KINDS = ("fc", "mlp", "random", "periodic", "constant")


@functools.lru_cache(maxsize=None)
def fc_flat(D, seed):
    """a random FCNetwork in flat order: fan-in scaled weights, LayerNorm weights near 1"""
    g = np.random.default_rng(1000 * D + seed)
    h1, h2, nact = 512, 256, 5
    parts = [g.normal(0, 1 / np.sqrt(D), h1 * D), g.normal(0, 0.1, h1), 1 + g.normal(0, 0.1, h1), g.normal(0, 0.1, h1),
             g.normal(0, 1 / np.sqrt(h1), h2 * h1), g.normal(0, 0.1, h2), 1 + g.normal(0, 0.1, h2), g.normal(0, 0.1, h2),
             g.normal(0, 1 / np.sqrt(h2), nact * h2), g.normal(0, 0.1, nact)]
    flat = np.concatenate(parts).astype(np.float32)
    assert flat.size == fc_params(D)
    return flat


def seat(kind, role, i):
    """seat number i of a kind for `role`: the scripted ones carry the edge seeds 0 and 2**64 - 1"""
    D = bc.ROLE_D[role]
    if kind == "fc":
        return fc_flat(D, i)
    if kind == "mlp":
        return bl.MLPBaseline(bc.fixture()[role]["flat"] if i % 2 == 0 else bc.random_net(D, 40 + i), D)
    if kind == "random":
        return bl.RandomBaseline((0, 2 ** 64 - 1, 7)[i % 3])
    if kind == "periodic":
        return bl.PeriodicBaseline((2, 0, 2 ** 31 - 1)[i % 3])
    return bl.ConstantBaseline((3, 0, 4)[i % 3])


def every_kind_matches():
    """seven matches: match i < 5 seats kinds (i, i + 1, i + 2) mod 5 on (agent_0, agent_1, adversary_0) - every kind in every
    slot, match 2 without any net -, match 5 three evolved nets, match 6 three policy nets"""
    rows = [[KINDS[(i + j) % 5] for j in range(3)] for i in range(5)] + [["fc"] * 3, ["mlp"] * 3]
    assert rows[2] == ["random", "periodic", "constant"]
    for j in range(3):
        assert {r[j] for r in rows} == set(KINDS)
    return [tuple(seat(k, role, i) for k, role in zip(row, TRIO)) for i, row in enumerate(rows)], rows


def expected_words(matches, kinds, episodes):
    """the game table of `matches` by the header's statement, with the slab offsets in order of appearance"""
    fc_off = mlp_off = 0
    words = np.zeros((len(matches), 16), dtype=np.int64)
    for m, (trio, row) in enumerate(zip(matches, kinds)):
        for x, kind, role in zip(trio, row, TRIO):
            s = bc.ROLE_SLOT[role]
            D = bc.ROLE_D[role]
            if kind == "fc":
                words[m, 4 * s:4 * s + 4] = (FC, fc_off, 0, 0)
                fc_off += (fc_params(D) + 63) // 64 * 64
            elif kind == "mlp":
                words[m, 4 * s:4 * s + 4] = (MLP, mlp_off, 0, 0)
                mlp_off += bl.mlp_stride(D)
            else:
                words[m, 4 * s:4 * s + 4] = (x.kind, x.arg, x.seed & 0xFFFFFFFF, x.seed >> 32)
    return np.repeat(words, episodes, axis=0).astype(np.uint32).view(np.int32), fc_off, mlp_off


def table_matches(lists):
    """the trios of a BaselineCrossPlay over `lists` in its game order t = (a B + b) C + c"""
    return [(a, b, c) for a in lists["agent_0"] for b in lists["agent_1"] for c in lists["adversary_0"]]


def reference_spec(episodes=10, first_ordinal=1):
    """the reference table of the issue: the champion pair against [Random, Periodic, AlwaysFire, the PPO adversary], and
    [(PPO, PPO), (Random, Random)] against the champion adversary"""
    return gt.GauntletSpec(
        adversaries=[bl.RandomBaseline(1), bl.PeriodicBaseline(0), bl.AlwaysFire, bc.fixture_baseline("adversary_0")],
        agent_pairs=[(bc.fixture_baseline("agent_0"), bc.fixture_baseline("agent_1")), (bl.RandomBaseline(2), bl.RandomBaseline(3))],
        episodes=episodes, first_ordinal=first_ordinal)
