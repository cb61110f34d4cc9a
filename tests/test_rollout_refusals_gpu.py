"""coevo_mpe_rollout / coevo_mpe16_rollout refuse a malformed descriptor before they launch anything.

Both entry points share one driver (csrc/rollout_api.hip): a two-cohort rollout of two cycles is handed a copy of its descriptor
with exactly one defect - no context, a missing / ill-formed cohort table, too many cohorts, a context whose cohort streams were
never reserved.  Every call answers COEVO_ERR_ARG, and the poisoned second state buffer, action words, rewards and clock stamps
are bit for bit what they were: no launch ran, not even the one that re-arms the stamps.  The untouched descriptor then plays
the rollout, and equals DeviceRollout.enqueue after the same reset.

Shapes: the smallest GA-shaped batches of tests/test_rollout_reuse_gpu.py and tests/test_fp16_rollout_gpu.py that two cohorts
can split - a shared opponent with <= 8 rows is ONE task and cannot play in two cohorts (RolloutPlan raises), so the float32
batch has 10 individuals (10 rows per opponent) and the float16 one 6 per role (12 rows), Hall of Fame 2."""
import ctypes as C

import numpy as np
import pytest
import torch

from coevonet_amd import lib as L
from tests.test_fp16_rollout_gpu import GaSetup
from tests.test_rollout_reuse_gpu import Setup

pytestmark = pytest.mark.gpu
ERR_ARG = -1
K, N_CYCLES, FIRST = 2, 2, 3
MAXK = L.K["COEVO_MAX_COHORTS"]
DEFECTS = ("ctx_null", "heavy_begin_null", "light_begin_null", "heavy_begin_first", "light_begin_last", "decreasing",
           "too_many_cohorts", "lanes_not_reserved")


@pytest.fixture(scope="module", params=["coevo_mpe_rollout", "coevo_mpe16_rollout"])
def batch(request):
    if request.param == "coevo_mpe_rollout":
        s = Setup(10, 2, 8, K)
        s.load_nets(seed=77)
    else:
        s = GaSetup(6, 2, K, seed=77)
    assert s.ro._entry == request.param and s.ro.n_cohorts == K
    s.ro.set_limits(np.full(s.plan.n_games, 3 * N_CYCLES))
    return s


def descriptor(ro):
    """the descriptor of a whole two-cycle rollout with timed stamps, as DeviceRollout.enqueue would hand it over"""
    d = L.RolloutDesc()
    C.memmove(C.byref(d), C.byref(ro.desc), C.sizeof(d))
    d.n_cycles = N_CYCLES
    d.light_stamps = L._p(ro.stamps)
    return d


def poison(ro):
    ro.state2[1].fill_(float("nan"))
    ro.actions_by_game.fill_(0x7f7f7f7f)
    ro.rewards.fill_(float("nan"))
    ro.stamps.fill_(5)
    torch.cuda.synchronize()
    return {name: t.clone().view(torch.uint8) for name, t in
            (("state2[1]", ro.state2[1]), ("actions_by_game", ro.actions_by_game), ("rewards", ro.rewards),
             ("stamps", ro.stamps))}


@pytest.mark.parametrize("defect", DEFECTS)
def test_defective_descriptor_is_refused_before_any_launch(batch, defect):
    ro, p = batch.ro, batch.plan
    ro.reset(0, p.n_games, FIRST)
    before = poison(ro)
    d, ctx = descriptor(ro), ro.ctx
    # cohort tables long enough for every cohort count tried here, well formed beyond cohort K (empty cohorts)
    hb = np.concatenate([p.heavy_begin_np, np.full(MAXK, p.heavy_begin_np[-1])]).astype(np.int32)
    lb = np.concatenate([p.light_begin_np, np.full(MAXK, p.light_begin_np[-1])]).astype(np.int32)
    assert hb[K] == d.n_heavy > 0 and lb[K] == d.n_light > 0 and hb[1] > 0
    fresh = None
    if defect == "ctx_null":
        ctx = None
    elif defect == "heavy_begin_first":
        hb[0] = 1
    elif defect == "light_begin_last":
        lb[K] -= 1
    elif defect == "decreasing":
        hb[1] = hb[K] + 1
    elif defect == "too_many_cohorts":
        d.n_cohorts = MAXK + 1
    elif defect == "lanes_not_reserved":
        ctx = fresh = L.load().coevo_rollout_ctx_create(0)
        assert fresh
    d.heavy_begin = None if defect == "heavy_begin_null" else hb.ctypes.data
    d.light_begin = None if defect == "light_begin_null" else lb.ctypes.data
    try:
        rc = getattr(L.load(), ro._entry)(C.byref(d), ctx, 0, L._stream())
        torch.cuda.synchronize()
    finally:
        if fresh:
            L.load().coevo_rollout_ctx_destroy(fresh)
    assert rc == ERR_ARG
    after = {"state2[1]": ro.state2[1], "actions_by_game": ro.actions_by_game, "rewards": ro.rewards, "stamps": ro.stamps}
    for name, want in before.items():   # (the stamps last: the launch that re-arms them is the first a rollout enqueues)
        same = torch.equal(after[name].view(torch.uint8), want)
        assert same, f"{defect}: a launch wrote {name}"


def test_untouched_descriptor_plays_what_enqueue_plays(batch):
    ro, p = batch.ro, batch.plan
    ro.reset(0, p.n_games, FIRST)
    poison(ro)
    d = descriptor(ro)
    L._check(getattr(L.load(), ro._entry)(C.byref(d), ro.ctx, 0, L._stream()), ro._entry)
    torch.cuda.synchronize()
    ro.check_status()
    got = ro.rewards.cpu().numpy().copy()
    st = ro.stamps[:K * N_CYCLES].cpu().numpy()
    assert (st != 5).all(), "a clock stamp of a launch that ran still holds the poison"
    ro.reset(0, p.n_games, FIRST)
    poison(ro)
    ro.enqueue(N_CYCLES)
    torch.cuda.synchronize()
    ro.check_status()
    want = ro.rewards.cpu().numpy()
    assert not np.isnan(want).any() and want.any()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
