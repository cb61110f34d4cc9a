"""The tiled fc1 block of the fp16 DeepQN slab on the GPU (csrc/dqn16_tiled.hip, include/coevo_ext.h), equalities only:
relayout / pack / unpack against the numpy permutation, the tiled forward against the streamed entry points, the C checker and
the order-telling nets' numpy row, the tiled breeding launch against the relayout of the streamed one's children, and whole
HalfDQNGAEngine(fc1_layout="tiled") generations against the checker and the streamed engine."""
import functools

import numpy as np
import pytest
import torch

from coevonet_amd import lib as L
from coevonet_amd.dqn_ga_half import HalfDQNGAEngine
from coevonet_amd.dqn_population import DQNGATrainer
from oracle import ref_port as rp
from tests import dqn16_checker as ck
from tests import dqn16_tiled_cases as tc
from tests import dqn_ga16_checker as dk
from tests import test_fp16_dqn_breeding_gpu as bg
from tests import test_fp16_dqn_trainers_gpu as tg
from tests.test_fp16_dqn_cpu import offsets
from tests.test_fp16_dqn_gpu import edge_nets, same_bits
from tests.util import Bag

pytestmark = pytest.mark.gpu
DEV = "cuda"
POISON = 0x7fc07e00        # NaN as an fp32 word and in both of its halves
POISON_I32 = 0x7f7f7f7f
ST_NO_ACTION, ST_BAD_TASK = 16, 64
ERR_ARG = -1
SHAPES = ((4, 6), (3, 18))


def stride16(C, n):
    return int(L.load().coevo_dqn16_slab_stride(C, n))


def fc1_block(C, n):
    """(first word, words) of the fc1 block in a net's stride: the conv sections in front are the fp32 slab's (w1 2048 C, b1 96,
    w2 32768, b2 192, w3 36864, b3 192 words)"""
    return 2048 * C + 96 + 32768 + 192 + 36864 + 192, 512 * 3136 // 2


def relayout(src, count, C, n, s, d, dst=None):
    """coevo_dqn16_relayout of `count` nets -> a new slab tensor (or into dst)"""
    dst = torch.full_like(src[:count * stride16(C, n)], POISON) if dst is None else dst
    L.call("coevo_dqn16_relayout", L._p(src), L._p(dst), count, C, n, s, d)
    torch.cuda.synchronize()
    return dst


def numpy_tiled(words, C, n):
    """the numpy permutation of a streamed slab [nets, stride] (uint32) -> the tiled one"""
    w0, nw = fc1_block(C, n)
    out = words.copy()
    src, dst = tc.streamed_to_tiled()
    for i in range(len(words)):
        halves = np.ascontiguousarray(words[i, w0:w0 + nw]).view(np.uint16)
        t = np.empty_like(halves)
        t[dst] = halves[src]
        out[i, w0:w0 + nw] = t.view(np.uint32)
    return out


# ---------------------------------------------------------------------------------------------------------------- relayout
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"C{s[0]}n{s[1]}")
def test_relayout_is_the_numpy_permutation_and_touches_nothing_else(shape):
    """nets of raw 16-bit patterns - NaN payloads, subnormals, +-0 and everything else a word can hold - between guard nets"""
    C, n = shape
    stride = stride16(C, n)
    w0, nw = fc1_block(C, n)
    g = np.random.default_rng(C * 100 + n)
    words = g.integers(0, 1 << 32, (2, stride), dtype=np.uint64).astype(np.uint32)
    words[0, w0:w0 + 8] = [0x7e017c01, 0xfe00fc00, 0x00010001, 0x83ff03ff, 0x80000000, 0x00008000, 0x7c00fc00, 0xffff7fff]
    src = torch.from_numpy(words.view(np.int32).reshape(-1)).to(DEV)
    guarded = torch.full((4 * stride,), POISON, dtype=torch.int32, device=DEV)   # nets 0 and 3 are guards
    relayout(src, 2, C, n, 0, 1, dst=guarded[stride:3 * stride])
    got = guarded.cpu().numpy().view(np.uint32).reshape(4, stride)
    assert (got[0] == POISON).all() and (got[3] == POISON).all(), "the words round the destination"
    want = numpy_tiled(words, C, n)
    assert np.array_equal(got[1:3], want), "streamed -> tiled: halves of the fc1 block permuted, every other word as it was"
    assert np.array_equal(got[1:3, :w0], words[:, :w0]) and np.array_equal(got[1:3, w0 + nw:], words[:, w0 + nw:])
    assert not np.array_equal(got[1:3, w0:w0 + nw], words[:, w0:w0 + nw])
    tiled = guarded[stride:3 * stride].clone()
    back = relayout(tiled, 2, C, n, 1, 0)
    assert torch.equal(back, src), "tiled -> streamed is the inverse"
    for flag in (0, 1):
        assert torch.equal(relayout(src, 2, C, n, flag, flag), src), "equal flags copy"
    # bad arguments write nothing
    lib, dst = L.load(), torch.full((2 * stride,), POISON, dtype=torch.int32, device=DEV)
    good = dict(src=L._p(src), dst=L._p(dst), n=2, C=C, n_actions=n, s=0, d=1)
    for b in (dict(src=None), dict(dst=None), dict(dst=L._p(src)), dict(src=L._p(src) + 4), dict(dst=L._p(dst) + 8), dict(n=-1),
              dict(C=0), dict(C=C | L.DQN_FC1_TILED), dict(n_actions=33), dict(s=2), dict(d=-1), dict(d=2)):
        a = dict(good, **b)
        assert lib.coevo_dqn16_relayout(a["src"], a["dst"], a["n"], a["C"], a["n_actions"], a["s"], a["d"], L._stream()) == ERR_ARG, b
    assert lib.coevo_dqn16_relayout(L._p(src), L._p(dst), 0, C, n, 0, 1, L._stream()) == 0
    torch.cuda.synchronize()
    assert (dst == POISON).all().item() and torch.equal(src.cpu(), torch.from_numpy(words.view(np.int32).reshape(-1)))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"C{s[0]}n{s[1]}")
def test_pack_tiled_is_the_relayout_of_pack_and_unpack_tiled_inverts_it(shape):
    C, n = shape
    stride, P = stride16(C, n), bg.n_params(C, n)
    g = np.random.default_rng(5 + C)
    flat = g.normal(0, 1, (3, P)).astype(np.float32)
    o = offsets(C, n)["fc1.weight"][0]
    edges = np.array([65519.9, 65520.0, 3e-8, 2.9802322e-08, 2.9802326e-08, -1e-7, 1.00048828125, -70000.0, -0.0], dtype=np.float32)
    for at in (o, o + 31, o + 3136 + 29, o + 512 * 3136 - len(edges)):
        flat[1, at:at + len(edges)] = edges
    d_flat = torch.from_numpy(flat).to(DEV)
    tiled = torch.full((5 * stride,), POISON, dtype=torch.int32, device=DEV)   # nets 0 and 4 are guards
    L.call("coevo_dqn16_pack_tiled", L._p(d_flat), tiled.data_ptr() + 4 * stride, 3, C, n)
    streamed = bg.pack16(list(flat), C, n)
    assert torch.equal(tiled[stride:4 * stride], relayout(streamed, 3, C, n, 0, 1))
    assert (tiled[:stride] == POISON).all().item() and (tiled[4 * stride:] == POISON).all().item()
    back = torch.full((3, P), float("nan"), dtype=torch.float32, device=DEV)
    L.call("coevo_dqn16_unpack_tiled", tiled.data_ptr() + 4 * stride, L._p(back), 3, C, n)
    with np.errstate(over="ignore"):
        want = flat.astype(np.float16).astype(np.float32)
    assert np.array_equal(back.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(bg.unpack16(streamed, 0, 3, C, n).view(np.uint32), want.view(np.uint32))
    lib = L.load()
    for args in ((None, L._p(tiled), 1, C, n), (L._p(d_flat), None, 1, C, n), (L._p(d_flat), L._p(tiled), 0, C, n),
                 (L._p(d_flat), L._p(tiled), 1, 7, n), (L._p(d_flat), L._p(tiled), 1, C | L.DQN_FC1_TILED, n)):
        assert lib.coevo_dqn16_pack_tiled(*args, L._stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert (tiled[:stride] == POISON).all().item()


# ----------------------------------------------------------------------------------------------------------------- forward
class Slabs:
    """the same nets packed into a streamed and a tiled slab"""

    def __init__(self, nets, C, n):
        self.C, self.n, self.stride = C, n, stride16(C, n)
        self.streamed = bg.pack16(nets, C, n)
        self.tiled = torch.full_like(self.streamed, POISON)
        flat = torch.from_numpy(np.ascontiguousarray(np.stack(nets), dtype=np.float32)).to(DEV)
        L.call("coevo_dqn16_pack_tiled", L._p(flat), L._p(self.tiled), len(nets), C, n)
        torch.cuda.synchronize()


def forward(slabs, tasks, frames, tiled, *, status0=0, bufs=None, hidden_only=False):
    """coevo_dqn16_forward_argmax[_tiled] (or the hidden pair) on poisoned buffers -> dict(rc, hid [rows, 512] and act [rows, 3136]
    of the workspace, logits, actions, status, bufs)"""
    rows = frames.shape[0]
    t = np.zeros(len(tasks), dtype=L.DQN_TASK_DTYPE)
    for i, task in enumerate(tasks):
        t[i] = task
    d_tasks, d_frames = L.tasks_to_device(t, DEV), torch.from_numpy(np.ascontiguousarray(frames)).to(DEV)
    if bufs is None:
        ws = torch.full((int(L.load().coevo_dqn16_workspace_bytes(rows)) // 4,), float("nan"), dtype=torch.float32, device=DEV)
        lg = torch.full((rows, L.DQN_LOGIT_STRIDE), POISON_I32, dtype=torch.int32, device=DEV).view(torch.float32)
        act = torch.full((rows,), POISON_I32, dtype=torch.int32, device=DEV)
        bufs = (ws, lg, act)
    ws, lg, act = bufs
    status = torch.full((1,), status0, dtype=torch.int32, device=DEV)
    slab = slabs.tiled if tiled else slabs.streamed
    head = (L._p(slab), L._p(d_tasks), len(tasks), min(max(1, max(int(x[2]) for x in tasks)), 16), rows, slabs.C, slabs.n,
            L._p(d_frames))
    sfx = "_tiled" if tiled else ""
    if hidden_only:
        rc = getattr(L.load(), "coevo_dqn16_forward_hidden" + sfx)(*head, L._p(status), L._p(ws), L._stream())
    else:
        rc = getattr(L.load(), "coevo_dqn16_forward_argmax" + sfx)(*head, L._p(act), L._p(lg), L._p(status), L._p(ws), L._stream())
    torch.cuda.synchronize()
    w = ws.cpu().numpy()
    return {"rc": rc, "act": w[:rows * 3136].reshape(rows, 3136), "hid": w[rows * 3136:].reshape(rows, 512),
            "logits": lg.cpu().numpy(), "actions": act.cpu().numpy(), "status": int(status.item()), "bufs": bufs}


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_outputs(t, s, what=""):
    """every word the tiled forward left behind equals the streamed one's: all 512 hidden outputs of every row, the conv
    activations, logits (poison past n_actions included), actions, status, return code"""
    assert t["rc"] == s["rc"] == 0, what
    assert np.array_equal(words(t["hid"]), words(s["hid"])), (what, "hidden rows")
    assert np.array_equal(words(t["act"]), words(s["act"])), (what, "conv activations")
    assert np.array_equal(words(t["logits"]), words(s["logits"])), (what, "logits")
    assert np.array_equal(t["actions"], s["actions"]) and t["status"] == s["status"], what


def task_table(stride, spec):
    """[(net, rows)] -> tasks that tile the rows"""
    out, row = [], 0
    for net, r in spec:
        out.append((net * stride, row, r))
        row += r
    return out


# rows 1 / 3 / 4 / 5 / 15 / 16 and a row total that is no multiple of 8; one net in three adjacent tasks (plain loads) beside
# lone nets (non-temporal loads); 19 one-row tasks (a grid rounded up to 24)
TASK_LISTS = {
    "rows_1_3_4_5_15_16": (4, 6, [(0, 1), (1, 3), (2, 4), (3, 5), (4, 15), (5, 16)]),
    "shared_net_beside_lone_nets": (3, 18, [(0, 3), (0, 2), (0, 1), (1, 4), (2, 1)]),
    "nineteen_one_row_tasks": (6, 6, [(i % 3, 1) for i in range(19)]),
}


@functools.lru_cache(maxsize=None)
def random_case(name):
    """nets and frames of one task list - drawn once"""
    C, n, spec = TASK_LISTS[name]
    torch.manual_seed(len(name) + C)
    nets = [ck.half_net(C, n, 0.02) for _ in range(1 + max(net for net, _ in spec))]
    g = np.random.Generator(np.random.PCG64(17))
    frames = g.integers(0, 256, size=(sum(r for _, r in spec), 84, 84, C), dtype=np.uint8)
    frames[0] = 0                                   # a constant frame: zero variance in conv1's BatchNorm statistics
    return nets, frames


@functools.lru_cache(maxsize=None)
def checker_rows(name):
    """the checker's (action, logits, status) per row of random_case(name) - computed once"""
    C, n, spec = TASK_LISTS[name]
    nets, frames = random_case(name)
    want, row = [], 0
    for net, r in spec:
        want += [ck.forward(nets[net], C, n, frames[row + i]) for i in range(r)]
        row += r
    return want


@pytest.mark.parametrize("name", list(TASK_LISTS))
def test_forward_equals_the_streamed_entry_points_and_the_checker(name):
    C, n, spec = TASK_LISTS[name]
    nets, frames = random_case(name)
    slabs = Slabs(nets, C, n)
    tasks = task_table(slabs.stride, spec)
    assert len(frames) % 8 != 0 or name != "rows_1_3_4_5_15_16"
    t, s = forward(slabs, tasks, frames, True), forward(slabs, tasks, frames, False)
    assert_same_outputs(t, s, name)
    assert t["status"] == 0 and np.isfinite(t["hid"]).all() and (t["hid"] >= 0).all() and (t["hid"] > 0).mean() > 0.2
    for r, (a, lg, st) in enumerate(checker_rows(name)):
        assert st == 0 and same_bits(t["logits"][r, :n], lg) and t["actions"][r] == a, (name, r)
        assert (words(t["logits"][r, n:]) == POISON_I32).all()
    # the hidden pair leaves the same workspace and touches neither logits nor actions
    h = forward(slabs, tasks, frames, True, hidden_only=True)
    assert h["rc"] == 0 and h["status"] == 0 and np.array_equal(words(h["hid"]), words(t["hid"]))
    assert (words(h["logits"]) == POISON_I32).all() and (h["actions"] == POISON_I32).all()
    # two forwards back to back on the used buffers: the same words; a foreign status bit survives
    again = forward(slabs, tasks, frames, True, bufs=t["bufs"], status0=0x1000)
    assert again["status"] == 0x1000
    again["status"] = 0
    assert_same_outputs(again, s, name + " (second forward)")


def test_order_telling_nets_give_the_numpy_row():
    """fc1 rows that hold +32768, -32768 and 2^-10: the outputs count which k came before, between and after"""
    C, n = 4, 6
    torch.manual_seed(12)
    base, off = ck.half_net(C, n, 0.02), offsets(C, n)
    gamma = tc.f16(np.random.default_rng(1).normal(1, 0.5, 64))
    nets = [tc.telling_net(base, off, 0, gamma), tc.telling_net(base, off, 1), base]
    slabs = Slabs(nets, C, n)
    frames = np.zeros((1 + 16 + 3, 84, 84, C), dtype=np.uint8)
    frames[17:] = np.random.Generator(np.random.PCG64(2)).integers(0, 256, size=(3, 84, 84, C), dtype=np.uint8)
    tasks = task_table(slabs.stride, [(0, 1), (1, 16), (2, 3)])
    t, s = forward(slabs, tasks, frames, True), forward(slabs, tasks, frames, False)
    assert (t["act"][:17] == 1.0).all(), "every fc1 input of an order-telling net on the all-zero frame is exactly 1.0"
    want = [tc.telling_hidden(0)] + [tc.telling_hidden(1)] * 16
    for r, w in enumerate(want):
        assert np.array_equal(words(t["hid"][r]), words(w)), (r, "tiled", np.flatnonzero(t["hid"][r] != w)[:8])
        assert np.array_equal(words(s["hid"][r]), words(w)), (r, "streamed")
    assert_same_outputs(t, s)
    assert t["status"] == 0


def test_edge_nets_subnormal_inf_nan_weight_and_conv_overflow_are_contained():
    C, n = 4, 6
    sub, zero, big, tie, over = edge_nets(C, n)
    nan = tie.copy()
    o = offsets(C, n)["fc1.weight"][0]
    nan[o + 77 * 3136 + 1234] = np.nan              # one NaN fc1 weight: output 77 of that task's rows
    g = np.random.Generator(np.random.PCG64(8))
    frames = g.integers(0, 256, size=(9, 84, 84, C), dtype=np.uint8)
    frames[8] = 255
    slabs = Slabs([sub, zero, big, tie, nan, over], C, n)
    # rows: sub 0 | zero 1 | big 2 | tie 3-4 | nan 5-6 | tie 7 | over 8 (255 frame: conv1 sums pass 65504)
    spec = [(0, 1), (1, 1), (2, 1), (3, 2), (4, 2), (3, 1), (5, 1)]
    tasks = task_table(slabs.stride, spec)
    t, s = forward(slabs, tasks, frames, True, status0=0x1000), forward(slabs, tasks, frames, False, status0=0x1000)
    assert_same_outputs(t, s)
    assert t["status"] == (0x1000 | ST_NO_ACTION), "the conv overflow's row selects no action; the foreign bit survives"
    assert not np.array_equal(t["hid"][0], t["hid"][1]) and (t["hid"][0] != 0).any(), "subnormal fc1 weights are not flushed"
    assert np.isposinf(t["hid"][2, 0]) and np.isfinite(t["hid"][2, 1:]).all(), "an fc1 sum past 65504 is inf"
    assert np.isnan(t["hid"][8]).all() and np.isfinite(t["hid"][:8][~np.isnan(t["hid"][:8])]).sum() > 0
    # the NaN weight: column 77 of rows 5-6 is NaN, every other word equals the run with the clean net in its place
    clean = Slabs([sub, zero, big, tie, tie, over], C, n)
    c = forward(clean, tasks, frames, True, status0=0x1000)
    assert np.isnan(t["hid"][5:7, 77]).all() and not np.isnan(c["hid"][5:7, 77]).any()
    keep = np.ones((9, 512), dtype=bool)
    keep[5:7, 77] = False
    assert np.array_equal(words(t["hid"])[keep], words(c["hid"])[keep]), "a word outside the NaN column changed"
    assert not np.isnan(t["hid"][:8][keep[:8]]).any()
    for r, net in ((0, sub), (2, big), (3, tie), (5, nan), (7, tie)):
        a, lg, st = ck.forward(net, C, n, frames[r])
        assert same_bits(t["logits"][r, :n], lg) and t["actions"][r] == a, r
    assert np.isnan(t["logits"][8, :n]).all() and t["actions"][8] == 0


def test_bad_tasks_are_reported_and_write_nothing():
    name = "shared_net_beside_lone_nets"
    C, n, _ = TASK_LISTS[name]
    nets, frames = random_case(name)
    want = checker_rows(name)
    slabs = Slabs(nets, C, n)
    st = slabs.stride
    g = np.random.Generator(np.random.PCG64(11))
    fr = np.concatenate([frames[:3], g.integers(0, 256, size=(19, 84, 84, C), dtype=np.uint8), frames[3:5]])
    # rows 0-2 net 0 | 3 (unaligned net_off) | 4-20 (17 rows) | 21 (0 rows, then served by nobody) | 22-23 net 0
    tasks = [(0, 0, 3), (st + 2, 3, 1), (st, 4, 17), (2 * st, 21, 0), (0, 22, 2)]
    for tiled in (True, False):
        out = forward(slabs, tasks, fr, tiled)
        assert out["rc"] == 0 and out["status"] == ST_BAD_TASK
        for r, (a, lg, _) in zip((0, 1, 2, 22, 23), want[:5]):
            assert same_bits(out["logits"][r, :n], lg) and out["actions"][r] == a, (tiled, r)
        skipped = slice(3, 21)   # (row 21 belongs to the 0-row task in front of it by task_of_row: skipped as well)
        assert np.isnan(out["hid"][skipped]).all() and np.isnan(out["act"][skipped]).all(), "a bad task's workspace rows"
        assert (words(out["logits"][skipped]) == POISON_I32).all() and (out["actions"][skipped] == POISON_I32).all()
        assert np.isnan(out["hid"][21]).all() and out["actions"][21] == POISON_I32


# ---------------------------------------------------------------------------------------------------------------- breeding
def breed_both(parents, C, n, sigma, flags, calls, *, stream_hi=bg.STREAM_HI, gen_dev=None, gen_bias=0, ref=None):
    """the launches of `calls` = ((child_first, n_children, stream_lo_first), ...) into poisoned 7-net child slabs, streamed and
    tiled -> (streamed children, tiled children, tiled partials per call, tiled ref)"""
    stride, nb = stride16(C, n), bg.blocks16(C, n)
    par_s = bg.pack16(parents, C, n)
    par_t = relayout(par_s, len(parents), C, n, 0, 1)
    ref_t = relayout(ref, 1, C, n, 0, 1) if ref is not None else None
    kids_s, kids_t = bg.poisoned(bg.NETS * stride), bg.poisoned(bg.NETS * stride)
    sig, parts = bg.dev_f32(sigma), []
    for first, count, slo in calls:
        idx = bg.dev_i32([c % len(parents) for c in range(count)])
        tail = (first, count, C, n, L._p(sig), bg.SEED, slo, stream_hi, flags, L._p(gen_dev) if gen_dev is not None else None,
                gen_bias)
        part = bg.nan_partials(count * nb) if ref is not None else None
        L.call("coevo_dqn16_perturb_dist", L._p(par_s), L._p(idx), L._p(kids_s), *tail, None, None)
        L.call("coevo_dqn16_perturb_dist_tiled", L._p(par_t), L._p(idx), L._p(kids_t), *tail,
               L._p(ref_t) if ref is not None else None, L._p(part) if part is not None else None)
        parts.append(part)
    torch.cuda.synchronize()
    return kids_s, kids_t, parts, ref_t


def assert_children_are_the_relayout(kids_s, kids_t, C, n, calls):
    stride = stride16(C, n)
    written = sorted(first + c for first, count, _ in calls for c in range(count))
    t = kids_t.cpu().numpy().view(np.uint32).reshape(bg.NETS, stride)
    for net in range(bg.NETS):
        if net not in written:
            assert (t[net] == POISON).all(), (net, "a net outside the written range changed")
            continue
        want = relayout(kids_s[net * stride:(net + 1) * stride], 1, C, n, 0, 1).cpu().numpy().view(np.uint32)
        assert np.array_equal(t[net], want), (net, "differs from the relayout of the streamed child",
                                              np.flatnonzero(t[net] != want)[:8])


@pytest.mark.parametrize("flags", [0, bg.SKIP_BN])
@pytest.mark.parametrize("sigma", [0.0, 0.05, 0.5])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"C{s[0]}n{s[1]}")
def test_tiled_children_are_the_relayout_of_the_streamed_children(shape, sigma, flags):
    """1 and 3 children at child_first > 0 in a poisoned slab, stream_lo_first 5 and 100"""
    C, n = shape
    kids_s, kids_t, _, _ = breed_both(bg.parents_of(C, n), C, n, sigma, flags, bg.CALLS)
    assert_children_are_the_relayout(kids_s, kids_t, C, n, bg.CALLS)
    if sigma:
        stride = stride16(C, n)
        assert not torch.equal(kids_t[3 * stride:4 * stride], kids_t[5 * stride:6 * stride]), "distinct streams, one parent"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"C{s[0]}n{s[1]}")
def test_copy_flag_and_a_generation_bias_that_wraps_stream_hi(shape):
    C, n = shape
    parents = bg.parents_of(C, n)
    kids_s, kids_t, _, _ = breed_both(parents, C, n, 0.5, bg.COPY, bg.CALLS)
    assert_children_are_the_relayout(kids_s, kids_t, C, n, bg.CALLS)
    stride = stride16(C, n)
    par_t = relayout(bg.pack16(parents, C, n), 2, C, n, 0, 1)
    assert torch.equal(kids_t[stride:2 * stride], par_t[:stride]) and torch.equal(kids_t[4 * stride:5 * stride], par_t[stride:])
    g = bg.dev_i32([3])
    ws, wt, _, _ = breed_both(parents, C, n, 0.05, 0, bg.CALLS, stream_hi=0xFFFFFFFE, gen_dev=g, gen_bias=-1)   # + 8 -> 6
    ps, pt, _, _ = breed_both(parents, C, n, 0.05, 0, bg.CALLS, stream_hi=6)
    assert_children_are_the_relayout(ws, wt, C, n, bg.CALLS)
    assert torch.equal(wt, pt) and torch.equal(ws, ps) and int(g.item()) == 3
    _, other, _, _ = breed_both(parents, C, n, 0.05, 0, bg.CALLS, stream_hi=2)
    assert not torch.equal(other, pt)


@pytest.mark.parametrize("sigma", [0.005, 0.05])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"C{s[0]}n{s[1]}")
def test_fused_partials_equal_the_distance_kernel_on_tiled_nets_and_distances_equal_the_checkers(shape, sigma):
    C, n = shape
    stride, nb = stride16(C, n), bg.blocks16(C, n)
    torch.manual_seed(7 + C)
    stale = dk.to_half(rp.dqn_init(C, n)[0])
    stream_hi, want = bg.order_proof_children(C, n, sigma, stale)
    ref_s = bg.pack16([stale], C, n)
    kids_s, kids_t, parts, ref_t = breed_both(bg.parents_of(C, n), C, n, sigma, 0, bg.CALLS, stream_hi=stream_hi, ref=ref_s)
    assert_children_are_the_relayout(kids_s, kids_t, C, n, bg.CALLS)
    for (first, count, slo), part in zip(bg.CALLS, parts):
        alone = bg.nan_partials(count * nb)
        L.call("coevo_dqn16_distance", L._p(ref_t), kids_t.data_ptr() + 4 * first * stride, count, C, n, L._p(alone))
        dist = torch.full((8,), -1.0, dtype=torch.float32, device=DEV)
        head = bg.dev_f32(123.5)
        L.call("coevo_fc16_distance_finalize", L._p(part), nb, count, L._p(dist), 2, L._p(head))
        torch.cuda.synchronize()
        assert np.isfinite(part.cpu().numpy()).all()
        assert np.array_equal(part.cpu().numpy().view(np.uint64), alone.cpu().numpy().view(np.uint64)), "fused != standalone"
        d = dist.cpu().numpy()
        assert d[0] == -1.0 and d[1] == 123.5 and (d[2 + count:] == -1.0).all(), "head / neighbours"
        for c in range(count):
            w = dk.distance(want[first + c], stale)
            assert bg.bits(d[2 + c])[0] == bg.bits(w)[0] and w > 0, (first + c, d[2 + c], w)


def test_a_tiled_net_against_itself_is_zero_and_bad_arguments_write_nothing():
    C, n = 3, 18
    stride, nb = stride16(C, n), bg.blocks16(C, n)
    a, b = bg.parents_of(C, n)
    slab = relayout(bg.pack16([a, b, a], C, n), 3, C, n, 0, 1)
    part = bg.nan_partials(3 * nb)
    L.call("coevo_dqn16_distance", L._p(slab), L._p(slab), 3, C, n, L._p(part))
    dist = torch.full((3,), -1.0, dtype=torch.float32, device=DEV)
    L.call("coevo_fc16_distance_finalize", L._p(part), nb, 3, L._p(dist), 0, None)
    torch.cuda.synchronize()
    d = dist.cpu().numpy()
    assert d[0] == 0 and d[2] == 0 and d[1] > 0
    if dk.distance_order_proof(b, a):
        assert bg.bits(d[1])[0] == bg.bits(dk.distance(b, a))[0]
    # the refusals of the tiled breeding launch: guard words round the child and the partials
    lib = L.load()
    child, part = bg.poisoned(3 * stride), bg.nan_partials(nb + 2)
    idx, sig = bg.dev_i32([1]), bg.dev_f32(0.05)
    good = dict(parent=L._p(slab), idx=L._p(idx), child=L._p(child), first=1, n=1, C=C, n_actions=n, sigma=L._p(sig), seed=bg.SEED,
                slo=0, shi=0, flags=0, gen=None, bias=0, ref=L._p(slab), partial=part.data_ptr() + 8)
    order = ("parent", "idx", "child", "first", "n", "C", "n_actions", "sigma", "seed", "slo", "shi", "flags", "gen", "bias", "ref",
             "partial")
    for bad in (dict(parent=None), dict(idx=None), dict(child=None), dict(sigma=None), dict(C=0), dict(C=C | L.DQN_FC1_TILED),
                dict(n_actions=33), dict(parent=L._p(slab) + 4), dict(child=L._p(child) + 8), dict(ref=L._p(slab) + 4), dict(n=-1),
                dict(first=-1), dict(ref=None), dict(partial=None), dict(flags=2), dict(flags=4), dict(flags=bg.COPY | 2)):
        assert lib.coevo_dqn16_perturb_dist_tiled(*[dict(good, **bad)[k] for k in order], L._stream()) == ERR_ARG, bad
    assert lib.coevo_dqn16_perturb_dist_tiled(*[dict(good, n=0)[k] for k in order], L._stream()) == 0
    torch.cuda.synchronize()
    assert (child.cpu().numpy().view(np.uint32) == POISON).all() and np.isnan(part.cpu().numpy()).all()
    assert lib.coevo_dqn16_perturb_dist_tiled(*[good[k] for k in order], L._stream()) == 0
    torch.cuda.synchronize()
    w, p = child.cpu().numpy().view(np.uint32).reshape(3, stride), part.cpu().numpy()
    assert (w[0] == POISON).all() and (w[2] == POISON).all() and (w[1, :bg.used_words(C, n)] != POISON).all()
    assert np.isnan(p[0]) and np.isnan(p[-1]) and np.isfinite(p[1:-1]).all()


# ------------------------------------------------------------------------------------------------------------------ engine
CONFIGS = {
    "pop4_hof2_C4_n6": dict(pop=4, hof=2, E=2, C=4, n=6, T_train=6, T_eval=2, adaptive=True, generations=3, seed=31),
    "pop5_hof3_C3_n18": dict(pop=5, hof=3, E=1, C=3, n=18, T_train=5, T_eval=2, adaptive=True, generations=3, seed=32),
}


@functools.lru_cache(maxsize=None)
def checker_run(name):
    cfg = CONFIGS[name]
    st = dk.State(*bg.initial(cfg))
    args = Bag(mutation_power_agent_0=bg.SIGMAS[0], mutation_power_agent_1=bg.SIGMAS[1], mutation_power_adversary=0.0,
               adaptive=cfg["adaptive"], max_timesteps_per_episode=cfg["T_train"], max_evaluation_steps=cfg["T_eval"])
    out = []
    for gen in range(cfg["generations"]):
        rec = dk.generation(st, gen, args, cfg["E"], cfg["C"], cfg["n"], bg.ENV_SEED, philox_seed=bg.SEED)
        rec["shas"] = bg.net_shas(st.popu, st.hof, st.elites)
        rec["dist"] = {r: st.dist[r].copy() for r in dk.ROLES}
        out.append(rec)
    return out


def make_engine(cfg, layout):
    eng = HalfDQNGAEngine(cfg["pop"], cfg["hof"], cfg["E"], cfg["C"], cfg["n"], cfg["T_train"], cfg["T_eval"], device=DEV,
                          env_seed=bg.ENV_SEED, philox_seed=bg.SEED, first_ordinal=1, capacity=16, sigmas=bg.SIGMAS,
                          sig_min=0.001, sig_max=0.2, adaptive=cfg["adaptive"], fc1_layout=layout)
    eng.load_initial(*bg.initial(cfg))
    return eng


@pytest.mark.parametrize("name", list(CONFIGS))
def test_tiled_engine_generations_equal_the_checker_and_the_streamed_engine(name):
    cfg = CONFIGS[name]
    n_main = 2 * cfg["pop"] * cfg["hof"]
    tiled, eager, streamed = make_engine(cfg, "tiled"), make_engine(cfg, "tiled"), make_engine(cfg, "streamed")
    try:
        assert tiled.fc1_tiled is True and streamed.fc1_tiled is False and tiled.ro.fc1_tiled is True and tiled.Cw == cfg["C"]
        # the slab IS tiled: relayout of the streamed engine's slab, net for net
        assert torch.equal(tiled.slab, relayout(streamed.slab, len(streamed.slab) // tiled.stride, cfg["C"], cfg["n"], 0, 1))
        dist0 = [bg.bits(tiled.dist_all[ri].cpu().numpy()) for ri in range(2)]
        states = []
        for gen in range(cfg["generations"]):
            tiled.step(use_graph=True)
            eager.step(use_graph=False)
            streamed.step(use_graph=True)
            got, got_eager, got_streamed = bg.engine_state(tiled), bg.engine_state(eager), bg.engine_state(streamed)
            assert got == got_eager, (gen, "graph replay differs from the eager generation")
            assert got == got_streamed, (gen, "the tiled engine differs from the streamed engine")
            assert got["status"] == 0 and got["gen_dev"] == gen + 1
            states.append(got)
        evals = tiled.eval_only()
        assert evals == eager.eval_only() == streamed.eval_only() and int(tiled.ro.status.item()) == 0
        # ... and the sequential restatement (computed once per configuration)
        want = checker_run(name)
        st0 = dk.State(*bg.initial(cfg))
        for ri, r in enumerate(dk.ROLES):   # generation 0's distances: coevo_dqn16_distance on two tiled nets
            assert np.array_equal(dist0[ri], bg.bits(st0.dist[r])), r
        for gen, (got, rec) in enumerate(zip(states, want)):
            assert got["acc"][:n_main] == rec["games"], (gen, "reward pairs")
            if gen > 0:
                assert got["acc"][n_main:] == want[gen - 1]["eval_games"], (gen, "evaluation reward pairs")
            for ri, r in enumerate(dk.ROLES):
                assert got["fitness"][ri] == bg.bits(rec["fitness"][ri]).tolist(), (gen, r, "fitness")
                assert got["diversity"][ri] == int(bg.bits(rec["diversity"][ri])[0]), (gen, r, "diversity")
                assert got["elite_ids"][ri] == rec["elite_ids"][ri], (gen, r, "elite ids")
                assert got["dist"][ri] == bg.bits(rec["dist"][r]).tolist(), (gen, r, "distances")
            assert got["sigma"] == rec["sigma_before"], (gen, "sigma")
            assert got["shas"] == rec["shas"], (gen, "nets")
        assert any(any(g) for rec in want for g in rec["games"]), "no hit was credited in any game"
        assert evals == want[-1]["eval_rewards"]
    finally:
        for e in (tiled, eager, streamed):
            e.close()


def test_the_trainer_with_the_tiled_layout_equals_the_trainer_without_it():
    cfg = tg.GA_CONFIGS["boxing_2_generations_fixed"]
    runs = []
    for layout in (None, "tiled"):
        args = tg.ga_args(cfg)
        if layout:
            args.coevo_fc1_layout = layout
        env = tg.make_env(args)
        torch.manual_seed(cfg["seed"])
        tr = DQNGATrainer(env, args)
        try:
            assert tr.eng.fc1_tiled is (layout == "tiled")
            for _ in range(cfg["generations"]):
                tr.step()
            res = tr.finish()
            runs.append(dict(games=[g.tolist() for g in res.game_rewards], fitness=[[bg.bits(f).tolist() for f in gen] for gen in res.fitness],
                             diversity=[bg.bits(d).tolist() for d in res.diversity], elite_ids=res.elite_ids, rewards=res.rewards,
                             sigma=res.sigma_after, shas=tg.engine_shas(tr.eng), resets=env.n_resets))
        finally:
            tr.close()
    assert runs[0] == runs[1]
    assert any(any(g) for gen in runs[0]["games"] for g in gen)
