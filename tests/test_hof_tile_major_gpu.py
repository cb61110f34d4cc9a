"""Tile-major twins of the Hall of Fame's second layer (COEVO_TASK_TILED): the stand-alone builder against its index formula
(tests/tile_major_cases.py, proven on the CPU by tests/test_hof_tile_major_cpu.py) and at its edges - raw words bit for bit,
16 nets, no nets, refusals -, the lean cycle launch through twins against the oracle and against the canonical path, the pipelined one-GPU Co-GA loop with
COEVO_HOF_TILED 1 against 0, and an upload into the Hall of Fame between generations.  Everything bit for bit."""
import numpy as np
import pytest
import torch

from coevonet_amd import genetic_algorithm as ga, lib as L
from coevonet_amd.game_logic import initialize_env
from oracle import ref_port as rp
from tests import fc_edge_nets as en, tile_major_cases as tm
from tests.tile_major_cases import twin_of
from tests.util import Bag

pytestmark = pytest.mark.gpu
DEV = "cuda"
H1, H2 = 512, 256


def test_twin_of_is_the_index_formula():
    W2 = np.arange(H2 * H1, dtype=np.float32).reshape(H2, H1)
    t = twin_of(W2).reshape(4, 128, 64, 4)
    for w, q, l, T in [(0, 0, 0, 0), (3, 127, 63, 3), (2, 17, 37, 1), (1, 5, 16, 2), (0, 64, 15, 3)]:
        lc, lg = l % 16, l // 16
        assert t[w, q, l, T] == W2[64 * w + 16 * T + lc, 4 * q + lg]


def slab_with_twin_room(flat, D, n_twins):
    """nets packed at the slab's start, then room for n_twins twins at a multiple of TASK_TWIN_UNIT -> (slab, twin offset)"""
    n, stride = flat.shape[0], L.fc_slab_stride(D)
    twin0 = -(-n * stride // L.TASK_TWIN_UNIT) * L.TASK_TWIN_UNIT
    slab = torch.zeros(twin0 + n_twins * L.W2_FLOATS, dtype=torch.float32, device=DEV)
    L.call("coevo_fc_pack", L._p(torch.from_numpy(flat).to(DEV)), L._p(slab), n, D)
    return slab, twin0


@pytest.mark.parametrize("D", [8, 10])
@pytest.mark.parametrize("n_nets", [1, 3])
def test_twin_builder_equals_the_index_formula(D, n_nets):
    """W2[j][k] = 512 j + k (+ 131072 per further net: still exact in fp32)"""
    flat = np.zeros((n_nets, L.fc_param_count(D)), dtype=np.float32)
    for i in range(n_nets):
        en.view(flat[i], D, "fc2.weight")[:] = np.arange(H2 * H1, dtype=np.float32).reshape(H2, H1) + H2 * H1 * i
    slab, twin0 = slab_with_twin_room(flat, D, n_nets + 1)
    slab[twin0:] = -1.0
    L.call("coevo_fc_w2_tile_major", L._p(slab), slab.data_ptr() + 4 * twin0, n_nets, D)
    got = slab[twin0:].cpu().numpy().reshape(n_nets + 1, -1)
    for i in range(n_nets):
        assert np.array_equal(got[i], twin_of(en.view(flat[i], D, "fc2.weight"))), i
    assert (got[n_nets] == -1.0).all()   # nothing written behind the last twin
    back = torch.zeros(n_nets, L.fc_param_count(D), dtype=torch.float32, device=DEV)
    L.call("coevo_fc_unpack", L._p(slab), L._p(back), n_nets, D)
    assert np.array_equal(back.cpu().numpy(), flat)   # ... and the nets are what they were


# ---------------------------------------------------------------------------------------------- the builder's edges
SENT = np.float32(-7.25)


class RawCase:
    """n_nets raw-word nets of width D (tm.raw_words: random bits, NaN payloads, infinities, -0.0, subnormals - in fc2.weight
    as everywhere else) between a guard net on each side, and a twin buffer of n_twins + 1 sentinel slots between guard words:
    the last slot is what a launch that wrote one twin too many would hit"""
    PAD = 4   # (16 bytes: the twins stay 16-byte aligned behind the guard words)

    def __init__(self, D, n_nets, n_twins, seed):
        self.D, self.n, self.stride = D, n_nets, L.fc_slab_stride(D)
        g = np.random.Generator(np.random.PCG64([seed, D, n_nets]))
        self.src_np = tm.raw_words(g, (n_nets + 2) * self.stride).reshape(n_nets + 2, self.stride)
        self.src = torch.from_numpy(self.src_np).to(DEV)
        self.dst = torch.full((2 * self.PAD + (n_twins + 1) * L.W2_FLOATS,), float(SENT), dtype=torch.float32, device=DEV)
        self.src_p = self.src.data_ptr() + 4 * self.stride
        self.dst_p = self.dst.data_ptr() + 4 * self.PAD

    def twins(self):
        """-> [n_twins + 1][W2_FLOATS] after asserting the guard words and that the source is bit for bit what it was"""
        torch.cuda.synchronize()
        a = self.dst.cpu().numpy()
        assert (a[:self.PAD] == SENT).all() and (a[-self.PAD:] == SENT).all(), "a guard word of the twin buffer was written"
        assert np.array_equal(self.src.cpu().numpy().view(np.uint32), self.src_np.view(np.uint32)), "the source nets changed"
        return a[self.PAD:-self.PAD].reshape(-1, L.W2_FLOATS)


@pytest.mark.parametrize("D,n_nets", [(8, 16), (10, 3), (8, 1)])
def test_twin_builder_copies_raw_words_bit_for_bit(D, n_nets):
    """NaN (payloads kept), inf, -0.0 and subnormals in fc2.weight come out at their permuted places as the words they are;
    nothing behind the last twin (16 nets of D = 8: the largest launch the engines make), the source left as it was"""
    c = RawCase(D, n_nets, n_nets, seed=21)
    w2 = c.src_np[1:1 + n_nets, tm.w2_offset(D):tm.w2_offset(D) + L.W2_FLOATS]
    assert np.isnan(w2).any() and np.isinf(w2).any() and (w2.view(np.uint32) == 0x80000000).any() \
        and ((w2 != 0) & (np.abs(w2) < en.MIN_NORMAL)).any()
    L.call("coevo_fc_w2_tile_major", c.src_p, c.dst_p, n_nets, D)
    got = c.twins()
    for i in range(n_nets):
        want = twin_of(tm.w2_of_slab_row(c.src_np[1 + i], D))
        assert np.array_equal(got[i].view(np.uint32), want.view(np.uint32)), (i, np.flatnonzero(got[i].view(np.uint32) != want.view(np.uint32))[:4])
    assert (got[n_nets] == SENT).all(), "written behind the last twin"


def test_twin_builder_no_nets_and_refusals_write_nothing():
    D = 8
    c = RawCase(D, 2, 2, seed=22)
    lib, st = L.load(), L._stream()
    assert lib.coevo_fc_w2_tile_major(c.src_p, c.dst_p, 0, D, st) == 0            # no nets: fine, and nothing to do
    for what, args in (("unaligned src", (c.src_p + 4, c.dst_p, 2, D)), ("unaligned dst", (c.src_p, c.dst_p + 4, 2, D)),
                       ("D = 9", (c.src_p, c.dst_p, 2, 9)), ("negative n_nets", (c.src_p, c.dst_p, -1, D)),
                       ("no src", (None, c.dst_p, 2, D)), ("no dst", (c.src_p, None, 2, D))):
        assert lib.coevo_fc_w2_tile_major(*args, st) == L.K["COEVO_ERR_ARG"], what
    assert (c.twins() == SENT).all()


# (net, rows, through its twin?): tasks of 16, 15, 5, 4 and 1 rows, two tasks of net 4, net 0 once through its twin and once not
HEAVY = [(0, 16, True), (1, 15, True), (2, 5, True), (3, 4, True), (4, 1, True), (4, 1, True), (5, 16, False), (0, 15, False)]
LIGHT = [(6, 5), (7, 1), (8, 8)]


@pytest.fixture(scope="module", params=[8, 10])
def merged_case(request):
    """nets, observations (one NaN row per task; the second one-row task of net 4 is healthy) and the oracle's word on every
    row, computed once per D"""
    D = request.param
    torch.manual_seed(300 + D)
    flat = np.stack([rp.mutate_torch(rp.init_net(D), D, 0.05) for _ in range(9)])
    g = np.random.Generator(np.random.PCG64(77 + D))
    rows = sum(n for _, n, _ in HEAVY) + sum(n for _, n in LIGHT)
    obs = np.zeros((rows, L.OBS_STRIDE), dtype=np.float32)
    obs[:, :D] = g.uniform(-2, 2, size=(rows, D)).astype(np.float32)
    net_of_row, r0, nan_rows = [], 0, []
    for t, (net, n) in enumerate([(net, n) for net, n, _ in HEAVY] + LIGHT):
        if t != 5:
            nan_rows.append(r0 + (n - 1) // 2)
        net_of_row += [net] * n
        r0 += n
    obs[nan_rows, D - 1] = np.nan
    want = [rp.fc_forward(flat[net_of_row[r]], D, obs[r, :D]) for r in range(rows)]
    status = 0
    for r, (a, lg, st) in enumerate(want):
        status |= st
        if r in nan_rows:
            assert st == en.BAD_OBS_STATUS
        else:   # a healthy row: finite, distinct logits
            assert st == 0 and np.isfinite(lg).all() and len(set(lg.tolist())) == 5, (r, lg)
    return D, flat, obs, want, status


def run_merged(D, flat, obs, tiled, poison=()):
    """one coevo_fc_forward_merged over HEAVY + LIGHT -> (actions, logits, status).  tiled: the tasks marked so read their
    net's twin; poison: nets whose canonical W2 is overwritten with NaN after the twins were built"""
    stride = L.fc_slab_stride(D)
    slab, twin0 = slab_with_twin_room(flat, D, 6)
    L.call("coevo_fc_w2_tile_major", L._p(slab), slab.data_ptr() + 4 * twin0, 6, D)
    o_w2 = D * H1 + 3 * H1
    for net in poison:
        slab[net * stride + o_w2:net * stride + o_w2 + L.W2_FLOATS] = float("nan")
    heavy, light = np.zeros(len(HEAVY), dtype=L.TASK_DTYPE), np.zeros(len(LIGHT), dtype=L.TASK_DTYPE)
    r0 = 0
    for t, (net, n, tw) in enumerate(HEAVY):
        heavy[t] = (net * stride, r0, n, D, L.task_tiled_flags(twin0 + net * L.W2_FLOATS) if (tw and tiled) else 0)
        r0 += n
    for t, (net, n) in enumerate(LIGHT):
        light[t] = (net * stride, r0, n, D, 0)
        r0 += n
    d_heavy, d_light, d_obs = L.tasks_to_device(heavy), L.tasks_to_device(light), torch.from_numpy(obs).to(DEV)
    actions = torch.full((r0,), -7, dtype=torch.int32, device=DEV)
    logits = torch.zeros(r0, L.LOGIT_STRIDE, dtype=torch.float32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    L.call("coevo_fc_forward_merged", L._p(slab), L._p(d_heavy), len(HEAVY), 16, L._p(d_light), len(LIGHT), 8, L._p(d_obs),
           L._p(actions), L._p(logits), L._p(status))
    return actions.cpu().numpy(), logits.cpu().numpy(), int(status.item())


@pytest.mark.parametrize("path", ["canonical", "tiled", "tiled_canonical_w2_poisoned"])
def test_merged_launch_through_twins_equals_the_oracle(merged_case, path):
    """flagged shared-opponent, unflagged shared-opponent and per-individual tasks in one launch: logits, actions and the status
    word are the oracle's on both paths; with the canonical W2 of the nets that only play through their twins (1 .. 4)
    overwritten by NaN the answer is still the oracle's - the twin is what the flagged tasks read"""
    D, flat, obs, want, status = merged_case
    got_a, got_l, got_st = run_merged(D, flat, obs, tiled=path != "canonical",
                                      poison=(1, 2, 3, 4) if path == "tiled_canonical_w2_poisoned" else ())
    assert got_st == status
    for r, (a, lg, st) in enumerate(want):
        assert en.same_bits_up_to_nan(got_l[r, :5], lg), (r, got_l[r, :5], lg)
        assert got_a[r] == max(a, 0), r   # (no action, -1 in the oracle: the kernels store 0 beside the NO_ACTION bit)


# ---------------------------------------------------------------------------------------------- the pipelined loop
def _trainer(cfg, monkeypatch, tiled):
    monkeypatch.setenv("COEVO_HOF_TILED", "1" if tiled else "0")
    torch.manual_seed(cfg["seed"])
    np.random.seed(cfg["seed"])
    args = Bag(algorithm="GA", **cfg["args"])
    env = initialize_env(args)
    return ga.GATrainer(env, args, rng="device_philox", env_mode="device")


def _twins_match(eng):
    torch.cuda.synchronize()
    twins = eng.hof_twin.cpu().numpy().reshape(3, eng.hof, -1)
    for ri, r in enumerate(ga.ROLES):
        for j, w in enumerate(eng.download(r, "hof", 0, eng.hof)):
            assert np.array_equal(twins[ri, j], twin_of(en.view(w, ga.ROLE_D[r], "fc2.weight"))), (r, j)


def _state(tr):
    eng = tr.eng
    torch.cuda.synchronize()
    return {"rewards": eng.ro.rewards.cpu().numpy().view(np.uint64).copy(),
            "fitness": np.stack([eng.fitness[r].cpu().numpy() for r in ga.ROLES]).view(np.uint32),
            "elites": np.stack([eng.order[r][:eng.E].cpu().numpy() for r in ga.ROLES]),
            "sigma": eng.sigma64.cpu().numpy().view(np.uint64).copy(),
            "hof": np.concatenate([eng.download(r, "hof", 0, eng.hof).view(np.uint32).reshape(-1) for r in ga.ROLES])}


def _same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("pop,hof,elites,pipelined", [(6, 2, 2, False), (4, 1, 1, True), (10, 3, 2, True)])
def test_pipelined_loop_tiled_equals_canonical(monkeypatch, pop, hof, elites, pipelined):
    """three generations of the one-GPU device loop asked for two cohorts: rewards, fitness, elite ids, sigma and Hall-of-Fame
    weights byte-equal with the twins and without; after every generation each twin is the permutation of its net.
    pop 4 / hof 1: no FIFO shift; pop 10 / hof 3: the FIFO shifts two slots.  pop 6 / hof 2 cannot be cut into two cohorts (its
    agent_1 Hall-of-Fame nets play 6 rows, one task: RolloutPlan refuses, the engine falls back to one chain and the
    whole-generation graph), so the mode never turns on there and every task keeps reading the canonical nets."""
    cfg = {"seed": 9, "args": dict(generations=3, population=pop, hof_size=hof, elites_number=elites, fitness_sharing=True,
                                   max_timesteps_per_episode=40, max_evaluation_steps=40, coevo_cohorts=2)}
    a, b = _trainer(cfg, monkeypatch, True), _trainer(cfg, monkeypatch, False)
    assert b.eng.hof_twin is None and a.eng.hof_twin is not None
    assert a.eng.K == b.eng.K == a.eng.ro.n_cohorts == (2 if pipelined else 1)
    for gen in range(3):
        a.step()
        b.step()
        assert a.eng._hof_tiled == pipelined and not b.eng._hof_tiled
        assert (a.eng.plan.heavy_np["reserved"] & L.TASK_TILED).all() == pipelined and not b.eng.plan.heavy_np["reserved"].any()
        _same(_state(a), _state(b), gen)
        if pipelined:
            _twins_match(a.eng)
    ra, rb = a.finish(), b.finish()
    assert ra.elite_ids == rb.elite_ids and [ra.rewards[r] for r in ga.ROLES] == [rb.rewards[r] for r in ga.ROLES]
    assert all(np.array_equal(x, y) for x, y in zip(ra.game_rewards, rb.game_rewards)) and len(ra.game_rewards) == 3


def test_upload_into_the_hall_of_fame_refreshes_the_twins(monkeypatch):
    """new Hall-of-Fame weights between two generations: the next rollout plays THEM on both paths (a stale twin would go on
    playing the old nets without any fault bit)"""
    cfg = {"seed": 4, "args": dict(generations=3, population=10, hof_size=3, elites_number=2, fitness_sharing=True,
                                   max_timesteps_per_episode=40, max_evaluation_steps=40, coevo_cohorts=2)}
    a, b = _trainer(cfg, monkeypatch, True), _trainer(cfg, monkeypatch, False)
    a.step()
    b.step()
    assert a.eng._hof_tiled and not b.eng._hof_tiled
    torch.manual_seed(123)
    fresh = {r: np.stack([rp.init_net(ga.ROLE_D[r]) for _ in range(3)]) for r in ga.ROLES}
    before = _state(a)
    for tr in (a, b):
        torch.cuda.synchronize()
        for r in ga.ROLES:
            tr.eng.upload(r, "hof", 0, fresh[r])
    _twins_match(a.eng)
    a.step()
    b.step()
    after = _state(a)
    _same(after, _state(b), "after the upload")
    _twins_match(a.eng)
    assert not np.array_equal(before["rewards"], after["rewards"])
