"""float16 nets on the GPU, bit for bit against the C checker (tests/checker16/fc16_checker.c): the slab's pack / unpack,
coevo_fc16_forward_argmax on thousands of (net, observation) pairs with crafted overflow and exact logit ties, and the
float16 play_game façade.  The nets (random_flat, the three-way tie, the two overflow nets) are tests/fc16_edge_nets.py's; the
full edge suite of this kernel and of the rollout's is tests/test_fc16_forward_edges_gpu.py."""
import numpy as np
import pytest
import torch

from coevonet_amd import lib as L
from coevonet_amd.fcnetwork import FCNetworkHalf
from oracle import ref_port as rp
from tests import fc16_edge_nets as E
from tests import fp16_checker as ck
from tests.fc16_edge_nets import linear_mask, random_flat   # (re-exported: the other fp16 test files import them from here)
from tests.util import Bag, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"


def pack(flats, D):
    n = len(flats)
    stride = L.fc16_slab_stride(D)
    slab = torch.full((n * stride,), -1, dtype=torch.int32, device=DEV)   # padding must come out zeroed
    L.call("coevo_fc16_pack", L._p(torch.from_numpy(np.ascontiguousarray(flats)).to(DEV)), L._p(slab), n, D)
    return slab, stride


def run_forward(slab, tasks, max_rows, obs_np):
    rows = obs_np.shape[0]
    obs = torch.zeros(rows, L.OBS_STRIDE, dtype=torch.float32)
    obs[:, :obs_np.shape[1]] = torch.from_numpy(obs_np)
    obs = obs.to(DEV)
    actions = torch.full((rows,), -1, dtype=torch.int32, device=DEV)
    logits = torch.zeros(rows, L.LOGIT_STRIDE, dtype=torch.float32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    L.call("coevo_fc16_forward_argmax", L._p(slab), L._p(L.tasks_to_device(tasks, DEV)), len(tasks), max_rows,
           L._p(obs), L._p(actions), L._p(logits), L._p(status))
    torch.cuda.synchronize()
    return actions.cpu().numpy(), logits.cpu().numpy()[:, :5], int(status.item())


def test_pack_unpack_exact():
    rng = np.random.default_rng(7)
    for D in (10, 8):
        flats = np.stack([random_flat(rng, D) for _ in range(3)])
        slab, stride = pack(flats, D)
        back = torch.zeros(flats.shape, dtype=torch.float32, device=DEV)
        L.call("coevo_fc16_unpack", L._p(slab), L._p(back), 3, D)
        assert np.array_equal(back.cpu().numpy().view(np.uint32), flats.view(np.uint32))
        used = 65536 + 256 * D + 640 + 3 * 512 + 3 * 256 + 5   # W2h, W1h, W3h (words), then the fp32 section
        assert stride == (used + 63) // 64 * 64
        assert (slab.cpu().numpy().reshape(3, stride)[:, used:] == 0).all()   # the pack zeroes the padding
        # rounding on pack: non-fp16 Linear entries round to nearest even, the fp32 entries are kept
        raw = rng.normal(0, 0.1, flats.shape[1]).astype(np.float32)
        slab1, _ = pack(raw[None], D)
        back1 = torch.zeros((1, raw.size), dtype=torch.float32, device=DEV)
        L.call("coevo_fc16_unpack", L._p(slab1), L._p(back1), 1, D)
        want = raw.copy()
        m = linear_mask(D)
        want[m] = raw[m].astype(np.float16).astype(np.float32)
        assert np.array_equal(back1.cpu().numpy()[0].view(np.uint32), want.view(np.uint32))


def same_bits(a, b):
    """bitwise equal, any NaN matching any NaN (the payload of a generated NaN is the platform's)"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def check_pairs(flats, D, obs, rows_per_task):
    """every net applied to rows_per_task observations; compare bits with the checker"""
    slab, stride = pack(flats, D)
    n = len(flats)
    tasks = np.zeros(n, dtype=L.TASK_DTYPE)
    for i in range(n):
        tasks[i] = (i * stride, i * rows_per_task, rows_per_task, D, 0)
    act, lg, st = run_forward(slab, tasks, rows_per_task, obs)
    want_st = 0
    for i in range(n):
        for r in range(rows_per_task):
            row = i * rows_per_task + r
            a, wl, s = ck.forward(flats[i], D, obs[row])
            want_st |= s
            assert same_bits(lg[row], wl), (i, r, lg[row], wl)
            assert act[row] == max(a, 0), (i, r)
    assert st == want_st
    return act, lg, st


@pytest.mark.parametrize("D,n_nets,rows", [(10, 40, 32), (8, 24, 32), (10, 64, 5), (8, 80, 1)])
def test_forward_random_nets_bitwise(D, n_nets, rows):
    """40x32 + 24x32 + 64x5 + 80x1 = 2448 (net, observation) pairs; 32-row tasks take four passes of 8 rows"""
    rng = np.random.default_rng(1000 + D * n_nets + rows)
    flats = np.stack([random_flat(rng, D, scale=0.05 * (1 + i % 4)) for i in range(n_nets)])
    obs = rng.uniform(-3, 3, size=(n_nets * rows, D)).astype(np.float32)
    obs[::7] *= np.float32(1e-3)   # small inputs: fp16 subnormal-adjacent values
    _, _, st = check_pairs(flats, D, obs, rows)
    assert st == 0


def test_forward_exact_ties_take_the_first_maximum():
    rng = np.random.default_rng(3)
    D = 10
    flat = random_flat(rng, D)
    # actions 1, 3 and 4 get identical output rows and biases, the maximum: exact logit ties, the strict '>' scan keeps action 1
    E.tie3(flat, D)
    obs = rng.uniform(-2, 2, size=(16, D)).astype(np.float32)
    act, lg, st = check_pairs(flat[None], D, obs, 16)
    assert st == 0
    assert (lg[:, 1] == lg[:, 3]).all() and (lg[:, 1] == lg[:, 4]).all() and (act == 1).all()


def test_forward_fp16_overflow_sets_status():
    rng = np.random.default_rng(4)
    D = 10
    # fc2 outputs past 65504 become inf, the LayerNorm then makes NaN: status BAD_FC2 (and the logits follow)
    flat = random_flat(rng, D)
    E.fc2_overflow(flat, D)
    obs = rng.uniform(-2, 2, size=(4, D)).astype(np.float32)
    _, _, st = check_pairs(flat[None], D, obs, 4)
    assert st & 4
    # an observation past the fp16 range is inf after rounding: BAD_INPUT, as the reference's half input check
    flat = random_flat(rng, D)
    obs = rng.uniform(-2, 2, size=(4, D)).astype(np.float32)
    obs[2, 3] = np.float32(70000.0)
    _, _, st = check_pairs(flat[None], D, obs, 4)
    assert st & 1
    # fc1 overflow (huge fc1 bias): BAD_FC1
    flat = random_flat(rng, D)
    E.fc1_overflow(flat, D)
    _, _, st = check_pairs(flat[None], D, obs[:2], 2)
    assert st & 2


def test_fc16_network_forward_and_fixture():
    """FCNetworkHalf.forward / determine_action through the kernel == checker; vs the reference's logits within one fp16
    ulp of the row's largest logit, actions equal where the reference's margin exceeds two ulps"""
    args = Bag(precision="float16")
    for c in load_golden("fc_forward_f16.json")["cases"]:
        torch.manual_seed(c["torch_seed"])
        net = FCNetworkHalf(c["D"], 5)
        if c["mutated"]:
            for p in net.parameters():
                p.data += torch.normal(0, c["mutate_std"], size=p.size())
        for obs, ref, ref_a, m in zip(c["obs"], c["logits"], c["actions"], c["margins"]):
            x = torch.tensor(obs).to(torch.float16)
            got = net.forward(x, args)
            assert got.dtype == torch.float16
            a, want, _ = ck.forward(net.flat(), c["D"], obs)
            assert np.array_equal(got.to(torch.float32).numpy().view(np.uint32), want.view(np.uint32))
            assert net.determine_action(x, args) == a
            tol = ck.ulp16(np.max(np.abs(ref)))
            assert np.max(np.abs(want.astype(np.float64) - np.array(ref))) <= tol
            if m > 2 * ck.ulp16(max(ref)):
                assert a == ref_a


def test_play_game_fp16_facade():
    """game_logic.play_game with float16 agents (nets packed once per game) == the checker's game, bit for bit, and the
    checker's game == the reference's fixture on all 18 games"""
    from coevonet_amd import game_logic as gl
    from coevonet_amd.mpe.simple_adversary import ENV_SEED, SimpleAdversaryAEC
    checked_exact = 0
    for c in load_golden("play_game_f16.json")["cases"]:
        torch.manual_seed(c["torch_seed"])
        np.random.seed(c["torch_seed"])
        env = SimpleAdversaryAEC(max_cycles=c["max_cycles"])
        env.reset(seed=ENV_SEED)
        args = Bag(precision="float16", max_timesteps_per_episode=c["limit"], max_evaluation_steps=c["limit"])
        ags = [gl.create_agent(env, args, r) for r in ("agent_0", "agent_1", "adversary_0")]
        if c["mutated"]:
            for a in ags:
                a.mutate(c["mutate_std"])
        stream = rp.Stream()
        for g in c["games"]:
            got = gl.play_game(env, ags[0].model, ags[1].model, ags[2].model, args, eval=False)
            want = ck.play_game(stream, *[a.model.flat() for a in ags], c["limit"], c["max_cycles"])
            assert want["status"] == 0
            assert list(got) == want["rewards"]
            assert want["actions"] == g["actions"] and want["rewards"] == g["rewards"], (c["torch_seed"], len(g["actions"]))
            checked_exact += 1
    assert checked_exact == 18


def test_forward_rejects_tasks_it_cannot_serve():
    """an unaligned net offset (the 16-byte weight pieces), a bad width or row count: the task is skipped and reported"""
    rng = np.random.default_rng(5)
    D = 10
    slab, stride = pack(random_flat(rng, D)[None], D)
    obs = rng.uniform(-1, 1, size=(1, D)).astype(np.float32)
    for off, rows, width in ((2, 1, D), (0, 0, D), (0, 33, D), (0, 1, 9)):
        tasks = np.zeros(1, dtype=L.TASK_DTYPE)
        tasks[0] = (off, 0, rows, width, 0)
        act, _, st = run_forward(slab, tasks, 1, obs)
        assert st == 64 and act[0] == -1, (off, rows, width)
