"""The float16 DeepQN forward (csrc/dqn16.hip) through the C ABI and the Python surface: every assertion is an equality
against the sequential C checker (tests/dqn16_checker.py) - logits as bits, actions, status."""
import functools

import numpy as np
import pytest
import torch

from coevonet_amd import deepqn as dq
from coevonet_amd import game_logic as gl
from coevonet_amd import lib as L
from coevonet_amd.atari_synthetic import SyntheticAtariAEC
from tests import dqn16_checker as ck
from tests.dqn16_edge_nets import edge_nets   # noqa: F401  (tests/test_fp16_dqn_tiled_gpu.py imports it from here)
from tests.test_fp16_dqn_cpu import fixture_net, offsets
from tests.util import DQN_FRAME_KINDS, Bag, dqn_golden_frames, load_golden

pytestmark = pytest.mark.gpu

ST_NO_ACTION, ST_BAD_TASK = 16, 64
POISON_I32 = 0x7f7f7f7f
DEV = "cuda"


def same_bits(got, want):
    """equal bit patterns; a NaN matches any NaN (the payload of a NaN is not part of the contract)"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


class Slab:
    """nets packed into one fp16 slab on the device"""

    def __init__(self, nets, C, n):
        self.C, self.n = C, n
        self.stride = int(L.load().coevo_dqn16_slab_stride(C, n))
        flat = torch.from_numpy(np.ascontiguousarray(np.stack(nets), dtype=np.float32)).to(DEV)
        self.slab = torch.full((len(nets), self.stride), POISON_I32, dtype=torch.int32, device=DEV)
        L.call("coevo_dqn16_pack", L._p(flat), L._p(self.slab), len(nets), C, n)


def raw_forward(slab, tasks, frames, *, max_rows=None, status0=0, bufs=None, logits=True):
    """coevo_dqn16_forward_argmax on poisoned buffers -> dict(rc, logits [rows, 32], actions, status, bufs)"""
    rows = frames.shape[0]
    t = np.zeros(len(tasks), dtype=L.DQN_TASK_DTYPE)
    for i, task in enumerate(tasks):
        t[i] = task
    d_tasks = L.tasks_to_device(t, DEV)
    d_frames = torch.from_numpy(np.ascontiguousarray(frames)).to(DEV)
    if bufs is None:
        ws = torch.full((int(L.load().coevo_dqn16_workspace_bytes(rows)) // 4,), float("nan"), dtype=torch.float32, device=DEV)
        lg = torch.full((rows, L.DQN_LOGIT_STRIDE), POISON_I32, dtype=torch.int32, device=DEV).view(torch.float32)
        act = torch.full((rows,), POISON_I32, dtype=torch.int32, device=DEV)
        bufs = (ws, lg, act)
    ws, lg, act = bufs
    status = torch.full((1,), status0, dtype=torch.int32, device=DEV)
    if max_rows is None:
        max_rows = min(max(int(x[2]) for x in tasks), L.DQN_MAX_ROWS)
    rc = L.load().coevo_dqn16_forward_argmax(L._p(slab.slab), L._p(d_tasks), len(tasks), max_rows, rows, slab.C, slab.n,
                                             L._p(d_frames), L._p(act), L._p(lg) if logits else None, L._p(status), L._p(ws),
                                             L._stream())
    torch.cuda.synchronize()
    return {"rc": rc, "logits": lg.cpu().numpy(), "actions": act.cpu().numpy(), "status": int(status.item()), "bufs": bufs}


def check_rows(out, n, want, rows=None):
    """rows of `out` against [(action, logits, status)] of the checker; the floats past n_actions keep their poison"""
    rows = range(len(want)) if rows is None else rows
    for r, (a, lg, _) in zip(rows, want):
        assert same_bits(out["logits"][r, :n], lg), (r, out["logits"][r, :n], lg)
        assert out["actions"][r] == a, r
        assert (out["logits"][r, n:].view(np.uint32) == POISON_I32).all(), r


RANDOM_CASES = [(4, 6, (3, 1, 10)), (6, 18, (16, 2)), (3, 6, (2, 5)), (5, 18, (4,)), (1, 1, (1,)), (4, 6, (1,) * 19)]


@functools.lru_cache(maxsize=None)
def random_case(C, n, rows):
    """nets (rp.dqn_init + mutate 0.02, rounded to half), frames and the checker's answers of one task list - computed once"""
    torch.manual_seed(C * 10 + n + len(rows))
    nets = [ck.half_net(C, n, 0.02) for _ in rows]
    g = np.random.Generator(np.random.PCG64(7))
    frames = [g.integers(0, 256, size=(r, 84, 84, C), dtype=np.uint8) for r in rows]
    frames[0][0] = 0                      # constant frames: zero variance in conv1's BatchNorm statistics
    if rows[0] > 1:
        frames[0][1] = 255
    else:
        frames[-1][0] = 255
    want = [ck.forward(net, C, n, fr[r]) for net, fr in zip(nets, frames) for r in range(fr.shape[0])]
    return nets, frames, want


def task_table(slab, rows):
    out, row = [], 0
    for i, r in enumerate(rows):
        out.append((i * slab.stride, row, r))
        row += r
    return out


@pytest.mark.parametrize("C,n,rows", RANDOM_CASES)
def test_forward_equals_the_checker(C, n, rows):
    """rows 1 / 4 / 5 / 16 per task, a row total that is no multiple of 8, 19 tasks (a wave grid rounded up to 24)"""
    nets, frames, want = random_case(C, n, rows)
    slab = Slab(nets, C, n)
    out = raw_forward(slab, task_table(slab, rows), np.concatenate(frames))
    assert out["rc"] == 0 and out["status"] == 0 and all(w[2] == 0 for w in want)
    check_rows(out, n, want)


def test_poisoned_buffers_and_back_to_back_forwards():
    """workspace NaN, logits and actions 0x7f bytes before the call; a second forward on the same (now used) workspace and
    outputs gives the same bits; without a logits buffer the actions are the same"""
    C, n, rows = RANDOM_CASES[2]
    nets, frames, want = random_case(C, n, rows)
    slab = Slab(nets, C, n)
    fr = np.concatenate(frames)
    first = raw_forward(slab, task_table(slab, rows), fr)
    check_rows(first, n, want)
    second = raw_forward(slab, task_table(slab, rows), fr, bufs=first["bufs"])
    assert second["rc"] == 0 and second["status"] == 0
    assert np.array_equal(first["logits"].view(np.uint32), second["logits"].view(np.uint32))
    assert np.array_equal(first["actions"], second["actions"])
    third = raw_forward(slab, task_table(slab, rows), fr, logits=False)
    assert third["rc"] == 0 and np.array_equal(third["actions"], first["actions"])
    assert (third["logits"].view(np.uint32) == POISON_I32).all()


def test_pack_rounds_to_half_and_unpack_returns_it():
    C, n = 3, 6
    torch.manual_seed(1)
    g = np.random.default_rng(2)
    P = int(L.load().coevo_dqn_param_count(C, n))
    flat = g.normal(0, 1, (2, P)).astype(np.float32)
    edges = [65519.9, 65520.0, 3e-8, 2.9802322e-08, 2.9802326e-08, -1e-7, 1.00048828125, 1.00146484375, -70000.0]
    flat[0, :len(edges)] = edges          # not fp16 values, in conv1.weight (stored as upcast words) ...
    o = offsets(C, n)["fc1.weight"][0]
    for at in (o, o + 7, o + 3136 + 8, o + 64 * 3136 + 391 * 8, o + 512 * 3136 - len(edges)):
        flat[1, at:at + len(edges)] = edges   # ... and in fc1.weight (stored as 2-byte values): first, odd, next-block and last places
    slab = Slab(list(flat), C, n)
    back = torch.zeros(2, P, dtype=torch.float32, device=DEV)
    L.call("coevo_dqn16_unpack", L._p(slab.slab), L._p(back), 2, C, n)
    with np.errstate(over="ignore"):
        want = flat.astype(np.float16).astype(np.float32)
    assert np.array_equal(back.cpu().numpy().view(np.uint32), want.view(np.uint32))
    used = 884710 - 8192 - 6 * 513 + C * 2048 + n * 513   # the words of C = 4, n = 6 moved to this shape
    assert (slab.slab[:, used:] == 0).all().item()          # the stride's padding is zeroed
    lib = L.load()
    for args in ((None, L._p(slab.slab), 1, C, n), (L._p(back), None, 1, C, n), (L._p(back), L._p(slab.slab), 0, C, n),
                 (L._p(back), L._p(slab.slab), 1, 7, n), (L._p(back), L._p(slab.slab), 1, C | L.DQN_FC1_TILED, n),
                 (L._p(back), L._p(slab.slab), 1, C, 33)):
        assert lib.coevo_dqn16_pack(*args, L._stream()) == -1


def test_edge_nets_through_the_abi():
    C, n = 4, 6
    sub, zero, big, tie, over = edge_nets(C, n)
    g = np.random.Generator(np.random.PCG64(8))
    frames = g.integers(0, 256, size=(5, 84, 84, C), dtype=np.uint8)
    frames[4] = 255
    slab = Slab([sub, zero, big, tie, over], C, n)
    tasks = task_table(slab, (1, 1, 1, 1))
    out = raw_forward(slab, tasks, frames[:4], status0=0x1000)
    want = [ck.forward(net, C, n, frames[i]) for i, net in enumerate((sub, zero, big, tie))]
    assert out["rc"] == 0 and out["status"] == 0x1000           # a foreign bit survives, nothing is added
    check_rows(out, n, want)
    assert not np.array_equal(out["logits"][0, :n], raw_forward(slab, [tasks[1]], frames[:1])["logits"][0, :n])  # not flushed
    assert not np.isfinite(want[2][1]).all()                    # the inf of fc1 reaches the logits
    assert out["logits"][3, 2] == out["logits"][3, 4] == 0.5 and out["actions"][3] == 2
    # conv overflow: all-NaN logits, COEVO_ST_NO_ACTION, action 0; the foreign bit still survives
    a, lg, st = ck.forward(over, C, n, frames[4])
    assert np.isnan(lg).all() and st == ST_NO_ACTION and a == 0
    out = raw_forward(slab, [(4 * slab.stride, 0, 1)], frames[4:5], status0=0x1000)
    assert out["rc"] == 0 and out["status"] == (0x1000 | ST_NO_ACTION)
    assert np.isnan(out["logits"][0, :n]).all() and out["actions"][0] == 0


def test_bad_tasks_are_skipped_and_reported():
    C, n, rows = RANDOM_CASES[2]            # two nets: 2 and 5 rows
    nets, frames, want = random_case(C, n, rows)
    slab = Slab(nets, C, n)
    g = np.random.Generator(np.random.PCG64(11))
    filler = g.integers(0, 256, size=(18, 84, 84, C), dtype=np.uint8)
    fr = np.concatenate([frames[0], filler, frames[1]])          # rows 0-1 | 2 (unaligned) | 3-19 (17 rows) | 20-24
    tasks = [(0, 0, 2), (slab.stride + 2, 2, 1), (slab.stride, 3, 17), (slab.stride, 20, 5)]
    out = raw_forward(slab, tasks, fr, max_rows=16)
    assert out["rc"] == 0 and out["status"] == ST_BAD_TASK
    check_rows(out, n, want[:2], rows=range(0, 2))
    check_rows(out, n, want[2:], rows=range(20, 25))
    assert (out["logits"][2:20].view(np.uint32) == POISON_I32).all() and (out["actions"][2:20] == POISON_I32).all()
    # n_rows = 0 and a negative count are bad tasks too
    out = raw_forward(slab, [(0, 0, 2), (slab.stride, 2, 0), (slab.stride, 2, -3)], fr[:2], max_rows=2)
    assert out["status"] == ST_BAD_TASK
    check_rows(out, n, want[:2])


def test_argument_errors():
    C, n, rows = RANDOM_CASES[4]
    nets, frames, _ = random_case(C, n, rows)
    slab = Slab(nets, C, n)
    lib = L.load()
    t = np.zeros(1, dtype=L.DQN_TASK_DTYPE)
    t[0] = (0, 0, 1)
    d_tasks = L.tasks_to_device(t, DEV)
    d_frames = torch.from_numpy(frames[0]).to(DEV)
    ws = torch.zeros(int(lib.coevo_dqn16_workspace_bytes(1)) // 4, dtype=torch.float32, device=DEV)
    lg = torch.full((1, L.DQN_LOGIT_STRIDE), 7.0, dtype=torch.float32, device=DEV)
    act = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    good = dict(slab=L._p(slab.slab), tasks=L._p(d_tasks), n_tasks=1, max_rows=1, rows=1, C=C, n=n, frames=L._p(d_frames),
                actions=L._p(act), logits=L._p(lg), status=L._p(st), ws=L._p(ws))

    def call(**kw):
        a = dict(good, **kw)
        return lib.coevo_dqn16_forward_argmax(a["slab"], a["tasks"], a["n_tasks"], a["max_rows"], a["rows"], a["C"], a["n"],
                                              a["frames"], a["actions"], a["logits"], a["status"], a["ws"], L._stream())

    bad = [dict(slab=None), dict(tasks=None), dict(frames=None), dict(actions=None), dict(status=None), dict(ws=None),
           dict(C=0), dict(C=7), dict(n=0), dict(n=33), dict(max_rows=0), dict(max_rows=17), dict(n_tasks=0), dict(rows=0),
           dict(slab=good["slab"] + 4), dict(slab=good["slab"] + 8), dict(C=C | L.DQN_FC1_TILED), dict(C=C | 0x200),
           dict(C=C | (1 << 16))]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert act.item() == 7 and st.item() == 0 and (lg == 7.0).all().item()   # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    assert st.item() == 0 and act.item() == 0


def test_facade_agrees_with_the_checker_on_the_fixture_frames():
    c = load_golden("deepqn_forward_f16.json")["cases"][0]
    C, n = c["C"], c["n_actions"]
    net = fixture_net(c)
    frames = dqn_golden_frames(C, c["frame_pcg_seed"])
    want = [ck.forward(net.flat(), C, n, frames[r]) for r in range(len(DQN_FRAME_KINDS))]
    logits, actions = dq.batched_actions([net.flat()], [frames], C, n, precision="float16")
    assert logits.dtype == np.float32 and logits.shape == (len(DQN_FRAME_KINDS), n)
    for r, (a, lg, st) in enumerate(want):
        assert st == 0 and same_bits(logits[r], lg) and actions[r] == a
    for r in (0, 5, 7):    # a random frame, all-0, constant planes: the [1, C, 84, 84] tensor of preprocess_observation and the raw frame
        x = torch.from_numpy(frames[r]).permute(2, 0, 1).unsqueeze(0).to(torch.float16)
        out = net.forward(x)
        assert out.dtype == torch.float16 and tuple(out.shape) == (1, n)
        assert np.array_equal(out.numpy()[0].view(np.uint16), want[r][1].astype(np.float16).view(np.uint16))
        assert net.determine_action(frames[r], None) == want[r][0]
    with pytest.raises(ValueError):
        dq.batched_actions([net.flat()], [frames], C, n, precision="float16", fc1_tiled=True)
    with pytest.raises(ValueError):
        dq.batched_actions([net.flat()], [frames], C, n, precision="bfloat16")


def test_nan_net_raises_and_a_healthy_net_is_unaffected():
    C, n = 4, 6
    torch.manual_seed(5)
    good = ck.half_net(C, n, 0.02)
    bad = good.copy()
    bad[offsets(C, n)["conv2.weight"][0] + 100] = np.nan
    g = np.random.Generator(np.random.PCG64(3))
    frames = [g.integers(0, 256, size=(2, 84, 84, C), dtype=np.uint8) for _ in range(2)]
    a, lg, st = ck.forward(bad, C, n, frames[1][0])
    assert np.isnan(lg).all() and st == ST_NO_ACTION
    with pytest.raises(ValueError):
        dq.batched_actions([good, bad], frames, C, n, precision="float16")
    logits, actions = dq.batched_actions([good, good], frames, C, n, precision="float16")
    a0, w0, _ = ck.forward(good, C, n, frames[1][1])
    assert actions[3] == a0 and same_bits(logits[3], w0)


def test_play_game_with_two_half_agents_equals_the_checker_loop():
    steps = 6
    args = Bag(game="pong_v3", precision="float16", max_timesteps_per_episode=steps, max_evaluation_steps=steps)
    env = SyntheticAtariAEC("pong_v3", channels=4)
    env.reset(seed=123)
    torch.manual_seed(31)
    p1, p2 = gl.create_agent(env, args), gl.create_agent(env, args)
    for p in (p1, p2):
        p.mutate(0.02)
    got = gl.play_game(env, p1.model, p2.model, args=args)
    twin = SyntheticAtariAEC("pong_v3", channels=4)
    twin.reset(seed=123)
    twin.reset()                                   # play_game's own reset
    rewards = {"first_0": 0, "second_0": 0}
    flats = {"first_0": p1.model.flat(), "second_0": p2.model.flat()}
    for t, agent in zip(range(steps), twin.agent_iter()):
        a, _, st = ck.forward(flats[agent], 4, 6, twin.observe(agent))
        assert st == 0
        twin.step(a)
        rewards[agent] += twin.last()[1]
    assert got == (rewards["first_0"], rewards["second_0"])
    assert env.t == steps and env.last_action == twin.last_action
