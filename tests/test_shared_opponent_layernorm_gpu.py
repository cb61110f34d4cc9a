"""The two LayerNorms of the lean shared-opponent body (fc_policy_mfma16_body, csrc/fc_body_mfma16.hip.h) against the oracle, bit for bit.

The body takes its row sums from packed butterflies over the 16x16 accumulator tiles and computes a row's mean / rstd in one
lane per row.  Whatever order it adds in must be the canonical one (lane xor 1, 2, 4, 8 inside a 16-lane row, then
(T0 + T1) + (T2 + T3), then the block partials left to right), so the nets and observations here mix magnitudes from 1e-6 to
1e3: with them any other order of the same additions shows in the bits of the logits.  Row counts 1, 4, 5, 15 and 16 (a lone
row, a full register group, a ragged last task, a full tile), D = 8 and 10, a row of variance 0 and a row with a NaN
observation next to healthy ones.

Entry points and helpers are those of tests/test_fc_forward_edges_gpu.py: coevo_fc_forward_merged (MODE_OBS: logits and
actions of every row) and the fused lean cycle launch of a DeviceRollout (MODE_FUSED: whole games, rewards and the last action
words).  Expected values are always the oracle's (rp.fc_forward, rp.play_game_status); no tolerance anywhere.  Before a
launch is trusted the oracle alone must give finite, pairwise distinct logits and status 0 for every healthy row."""
import numpy as np
import pytest
import torch

from coevonet_amd import lib as L
from oracle import ref_port as rp
from tests import fc_edge_nets as E
from tests import test_fc_forward_edges_gpu as G

pytestmark = pytest.mark.gpu
NAN = np.float32(np.nan)
ROWS = [16, 15, 5, 4, 1]


def wide(g, shape):
    """random signs, magnitudes 10^u with u uniform in [-6, 3]"""
    return (g.choice([-1.0, 1.0], size=shape) * 10.0 ** g.uniform(-6.0, 3.0, size=shape)).astype(np.float32)


def wide_net(D, seed, flat_fc1_bias=False):
    """an initialised net whose fc1 / fc2 weights and biases mix magnitudes from 1e-6 to 1e3 (flat_fc1_bias: fc1.bias 0.5
    throughout, so that an all-zero observation gives 512 equal fc1 outputs)"""
    g = G.rng(17, D, seed)
    w = E.base_net(D, 3000 + seed)
    for name in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"):
        t = E.view(w, D, name)
        t[:] = wide(g, t.shape)
    if flat_fc1_bias:
        E.view(w, D, "fc1.bias")[:] = 0.5
    return w


def wide_task(g, D, n, seed, name="wide", net=None):
    return name, wide_net(D, seed) if net is None else net, wide(g, (n, D))


def oracle_is_clean(D, tasks):
    """on the CPU, the oracle alone: every row without a NaN observation has status 0 and five finite, distinct logits"""
    for name, w, obs in tasks:
        for r, o in enumerate(obs):
            if np.isnan(o).any():
                continue
            a, lg, st = rp.fc_forward(w, D, o)
            assert st == 0 and np.isfinite(lg).all() and len(set(lg.view(np.uint32).tolist())) == rp.NACT and a >= 0, \
                f"{name} row {r} (D = {D}): the oracle gives status {st:#x}, logits {lg}"


def order_shows(D, tasks):
    """on the CPU: for most rows the fp32 sum of the 512 fc1 outputs taken left to right differs from the one taken pairwise,
    so a LayerNorm that added in another order than the canonical one would not keep the bits"""
    differ = total = 0
    for _, w, obs in tasks:
        W1, b1 = E.view(w, D, "fc1.weight").astype(np.float64), E.view(w, D, "fc1.bias").astype(np.float64)
        for o in obs:
            if not np.isfinite(o).all() or not o.any():
                continue
            h = (W1 @ o.astype(np.float64) + b1).astype(np.float32)
            seq = np.float32(0.0)
            for x in h:
                seq = np.float32(seq + x)
            tree = h.copy()
            while len(tree) > 1:
                tree = (tree[0::2] + tree[1::2]).astype(np.float32)
            differ, total = differ + (seq != tree[0]), total + 1
    assert total and differ * 2 > total, f"only {differ} of {total} rows tell one summation order from another"


def light_cast(g, D):
    """per-individual tasks of the R = 5 instantiation"""
    return [wide_task(g, D, n, 50 + i, "wide light") for i, n in enumerate([5, 3, 1, 4])]


@pytest.mark.parametrize("D", [8, 10])
@pytest.mark.parametrize("mix", ["same_net", "mixed"])
def test_wide_range_rows_bit_exact(mix, D):
    """same_net: one net as a full 16-row task and a ragged 15-row one, another as 5 + 4 rows, a lone row, beside the one
    per-individual task the entry point requires.  mixed: five nets (16, 15, 5, 4, 1 rows) beside four per-individual tasks
    of wide nets"""
    g = G.rng(5, D, mix == "mixed")
    if mix == "same_net":
        a, b = wide_net(D, 1), wide_net(D, 2)
        heavy = [wide_task(g, D, 16, 0, "wide A", a), wide_task(g, D, 15, 0, "wide A", a), wide_task(g, D, 5, 0, "wide B", b),
                 wide_task(g, D, 4, 0, "wide B", b), wide_task(g, D, 1, 3)]
        light = light_cast(g, D)[:1]
    else:
        heavy = [wide_task(g, D, n, 10 + i) for i, n in enumerate(ROWS)]
        light = light_cast(g, D)
    oracle_is_clean(D, heavy + light)
    order_shows(D, heavy)
    assert G.check("merged", D, {"heavy": (16, heavy), "light": (5, light)}) == 0


@pytest.mark.parametrize("D", [8, 10])
def test_a_row_of_equal_fc1_outputs(D):
    """an all-zero observation under fc1.bias = 0.5: that row's 512 fc1 outputs are equal, its variance is 0 and its
    rstd 1 / sqrt(eps); the other rows of its task (same register group, other groups, the other task of the net) are wide"""
    g = G.rng(6, D)
    net = wide_net(D, 20, flat_fc1_bias=True)
    heavy = []
    for n, zero_rows in ((16, [0, 6]), (15, [14]), (5, [4]), (4, [1]), (1, [0])):
        name, w, obs = wide_task(g, D, n, 0, f"flat bias, zero rows {zero_rows}", net)
        obs[zero_rows] = 0.0
        h = (E.view(w, D, "fc1.weight") @ obs[zero_rows[0]] + E.view(w, D, "fc1.bias")).astype(np.float32)
        assert (h == np.float32(0.5)).all()
        heavy.append((name, w, obs))
    light = light_cast(g, D)[:2]
    oracle_is_clean(D, heavy + light)
    assert G.check("merged", D, {"heavy": (16, heavy), "light": (5, light)}) == 0


@pytest.mark.parametrize("D", [8, 10])
def test_a_nan_observation_in_one_row(D):
    """one NaN observation per task, in rows of different register groups: the status word is exactly the oracle's (all five
    bits from those rows, nothing else), every other row keeps the oracle's bits"""
    g = G.rng(7, D)
    net = wide_net(D, 30)
    heavy = []
    for n, p in ((16, 9), (15, 14), (5, 0), (4, 3), (16, None), (1, None)):
        name, w, obs = wide_task(g, D, n, 0, f"NaN in row {p}", net)
        if p is not None:
            obs[p, p % D] = NAN
        heavy.append((name, w, obs))
    light = light_cast(g, D)[:2]
    oracle_is_clean(D, heavy + light)
    assert G.check("merged", D, {"heavy": (16, heavy), "light": (5, light)}) == E.BAD_OBS_STATUS


def test_fused_cycle_launch_with_wide_shared_opponents():
    """whole games through the fused lean cycle launch (fc_cycle16_kernel<5>: the shared agent_1 opponents and adversaries are
    tasks of fc_policy_mfma16_body<MODE_FUSED>, D = 10 and 8) with wide nets in every shared seat and in three per-individual
    ones: status 0, rewards and the last action words bit-equal to the oracle's games; on the CPU first: the games' actions
    are not all the same, so a wrong logit has something to change"""
    s = G.setup("lean16")
    ind, a1s, advs = G.seats(s, "lean16")
    G.install(s)
    for D, nets, tags, idx in ((10, s.nets10, s.tags10, a1s + ind[:3]), (8, s.nets8, s.tags8, advs)):
        for i in idx:
            nets[i] = wide_net(D, 40 + i)
            tags[i] = ("wide", D, 40 + i)
    for flat, D, at in ((s.nets10, 10, 0), (s.nets8, 8, len(s.nets10) * s.s10)):   # into the slab, as G.install packs them
        src = torch.from_numpy(np.ascontiguousarray(flat)).to(G.DEV)
        L.call("coevo_fc_pack", L._p(src), s.slab.data_ptr() + 4 * at, len(flat), D)
    first, limits = 53, G.limits_of(s, ragged=True)
    want, want_status, acts = G.oracle_games(s, first, limits, s.n_cycles)
    assert want_status == 0 and np.isfinite(want).all()
    assert len({tuple(a) for a in acts}) > 1, "every game ends on the same actions: these nets cannot show a wrong logit"
    got, status, last = G.run(s, "lean16", first, limits)
    assert status == 0, f"status {status:#x}"
    s.ro.check_status()
    G.assert_games(got, want, "lean16 wide shared opponents")
    G.assert_last_actions(last, acts, "lean16 wide shared opponents")
