"""Rounding points, faults, ties, dead channels, subnormals and ragged tasks in the float16 DeepQN forward, against the C checker
(csrc/dqn16.hip, csrc/dqn16_tiled.hip, the H16 paths of csrc/dqn_conv.hip.h, dqn_out_row<true> of csrc/dqn_common.hip.h in
dqn16_out_kernel and in the env-step launches of dqn_engine.hip, duel_env.hip and duel_seats.hip).

The judge is always ck.stages through the cache of tests/dqn16_edge_nets.py.  Every comparison is an equality of bit patterns (a
NaN matches any NaN): all 3136 conv3 activations and all 512 hidden words of the workspace, the logits with the poison behind
n_actions, the action, the status word; the tiled entry point against the streamed one word for word.  No tolerance anywhere.
tests/test_dqn16_edges_cpu.py pins the nets' properties and the teeth of every (site, mode) rounding pair on the checker alone, so
nothing here can pass vacuously: a kernel that rounds one of the nine conversions of a row toward zero, half away from zero,
flushes a subnormal result or saturates instead of returning inf differs from the checker on a row this file runs.

One kernel form serves every launch shape (dqn16_conv_kernel<CMAX, CT> by channel count; dqn16_fc1_kernel ->
dqn16_fc1_body<NG = ceil(rows / 4)>; dqn16_fc1_tiled_kernel -> dqn16_fc1_tiled_body<SHARED_NET = a neighbour task has the same
net_off>), so the launches are small: at most about 40 rows and 40 nets each.  Only numerical conditions are provoked: every
pointer is valid and every task table has the shape of one the suite already runs."""
import numpy as np
import pytest
import torch

from coevonet_amd import lib as L
from tests import dqn16_edge_nets as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
FOREIGN = 0x1000          # a bit no COEVO_ST_* uses: the status word is OR-ed into, so it must survive every launch
SENT = 0x5EAD             # an action word no forward has written
LAYOUTS = [False, True]   # streamed, tiled
FULL = [(4, 6), (6, 18)]
RUN_TIME_C = [(3, 6), (5, 18)]   # dqn16_conv_kernel<4, 0> / <6, 0>: the run-time channel count


@pytest.fixture(scope="module", autouse=True)
def release_nets():
    yield
    E.release()


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_outputs(t, s, what):
    """every word the tiled launch left behind equals the streamed one's"""
    for k in ("act", "hid", "logits"):
        assert np.array_equal(words(t[k]), words(s[k])), (what, k)
    assert np.array_equal(t["actions"], s["actions"]) and t["status"] == s["status"] and t["rc"] == s["rc"], what


def run_both(spec, nets, frames, C, n, what, preset=FOREIGN):
    """the launch in both fc1 forms: each against the checker, the tiled one against the streamed one -> (streamed, want, status)"""
    tasks, rows = E.tile_rows(spec)
    frames = np.stack(frames)
    assert rows == len(frames) <= 48 and len(nets) <= 40
    want, want_status = E.expected(tasks, nets, frames, C, n)
    outs = []
    for tiled in LAYOUTS:
        out = E.launch(tasks, nets, frames, C, n, tiled, preset)
        tag = f"{what} C={C} n={n} {'tiled' if tiled else 'streamed'}"
        assert out["rc"] == 0, tag
        E.assert_rows(out, want, n, tag)
        assert out["status"] == preset | want_status, f"{tag}: status {out['status']:#x}, want {preset | want_status:#x}"
        outs.append(out)
    assert_same_outputs(outs[1], outs[0], what)
    return outs[0], want, want_status


def healthy_task(C, n, k, rows, first_frame=0):
    return E.healthy(C, n, k), [E.ragged_frames(C)[(first_frame + i) % 16] for i in range(rows)]


def run_class_rows(C, n, rows, what):
    """the (class, frame) rows as one-row tasks of their own nets, between a healthy 3-row task and a healthy 2-row task"""
    nets, spec, frames = [], [], []

    def add(net, fr):
        for i, w in enumerate(nets):
            if w is net:
                break
        else:
            nets.append(net)
            i = len(nets) - 1
        spec.append((i, len(fr)))
        frames.extend(fr)

    add(*healthy_task(C, n, 0, 3))
    for name, fname in rows:
        add(E.make(name, C, n), [E.frame(C, fname)])
    add(*healthy_task(C, n, 1, 2, first_frame=5))
    return run_both(spec, nets, frames, C, n, what)


# =============================================================================== a. every class through both entry points
GROUP = 30


def groups_of(rows):
    return [rows[i:i + GROUP] for i in range(0, len(rows), GROUP)]


N_GROUPS = len(groups_of(E.class_rows(*FULL[0])))     # (the names alone: no checker call at import)


@pytest.mark.parametrize("C,n", FULL)
@pytest.mark.parametrize("group", range(N_GROUPS))
def test_every_class_row_in_both_layouts(group, C, n):
    """C = 4 (<4, 4>) and 6 (<6, 6>) in full: every class of the catalogue on the random frame, the conv1 one-tap classes on the lit
    frame (positions 0, 15 | 16, 383 | 384, 399 of channels 3 and 19), the plain net on the named frames, and every row of the 33
    rounding pairs - thirty rows per launch, each a one-row task of its own net between two healthy tasks.  Workspace NaN, logits
    and actions 0x7f bytes, status preset to a foreign bit: act, hid, logits, action and status are the checker's, the poison
    past n_actions is still there, the tiled launch left the streamed launch's words.
    Covers: ties (first maximum), rounding ties, signed zeros, -inf / +inf / NaN logits, NaN in each of the 16 tensors (gamma and
    beta are half here), inf in each weight tensor, gamma = 0 / < 0, dead channels, beta = -10, subnormal weights and results in
    every layer, sums at and just below 65520 in every conv layer, BatchNorm outputs past 65504, and the exact midpoint /
    subnormal / overflow words of fc1 (first and last k, first and last output of a 64-block, block 7) and of the output layer
    (first and last fma step; out_last_step: a term below half an fp32 ulp in the last step)"""
    rows = E.class_rows(C, n)
    groups = groups_of(rows)
    assert len(groups) == N_GROUPS and len(rows) > 75
    _, want, _ = run_class_rows(C, n, groups[group], f"class rows {group}")
    assert all(w is not None for w in want)


def run_time_rows(C, n):
    """ties, the NaN / inf classes and one rounding row per site"""
    names = [k for k in E.TIES] + ["signed_zeros", "all_neg_inf", "one_pos_inf", "one_nan_logit", "all_nan_logits"]
    names += [f"nan_{t}" for t in E.TENSORS] + [k for k in E.CLASSES if k.startswith("inf_")]
    rows = [(name, "random") for name in names]
    rr = E.rounding_rows(C, n)
    for site, mode in (("quotient", "toward_zero"), ("conv1", "ties_away"), ("bn1", "ties_away"), ("conv2", "ties_away"),
                       ("bn2", "ties_away"), ("conv3", "ties_away"), ("bn3", "ties_away"), ("fc1", "ties_away"), ("out", "ties_away")):
        rows += [r for r in rr[(site, mode)] if r not in rows]
    return rows


@pytest.mark.parametrize("C,n", RUN_TIME_C)
@pytest.mark.parametrize("group", range(2))
def test_run_time_channel_counts(group, C, n):
    """C = 3 (<4, 0>) and 5 (<6, 0>): conv1's weight block and everything behind it sit at channel-dependent slab offsets.  Ties,
    NaN in each of the 16 tensors, inf in each weight tensor, -inf / NaN logits, and one rounding row per conversion site (the
    ties-away rows: the one-tap channels on the lit frame, the recorded frames of the seeded sequence, the exact fc1 / output words)"""
    rows = run_time_rows(C, n)
    groups = groups_of(rows)
    assert len(groups) == 2
    run_class_rows(C, n, groups[group], f"run-time C rows {group}")


# =============================================================================== b. the fused output rows
def fused_cast(C, n):
    """one game per row: the output-sensitive classes, each a one-row task, and a second all_nan_logits row at the end"""
    names = list(E.OUTPUT_SENSITIVE) + ["plain", "all_nan_logits"]
    nets = []
    for name in names:
        w = E.make(name, C, n)
        if not any(w is x for x in nets):
            nets.append(w)
    spec = [(next(i for i, x in enumerate(nets) if x is E.make(name, C, n)), 1) for name in names]
    return names, nets, spec, [E.frame(C, "random")] * len(names)


def fused_step(kind, dev, C, n, G, limits, seed=0x5EED):
    """the env-step launch `kind` at t = 1 on the workspace a hidden launch filled -> (action words, status)"""
    rows = torch.arange(G, dtype=torch.int32, device=DEV)
    lim = torch.tensor(list(limits), dtype=torch.int32, device=DEV)
    ord0 = torch.arange(3, 3 + G, dtype=torch.int64, device=DEV)
    acc = torch.full((G, 3), 5.5, dtype=torch.float64, device=DEV)
    frames = torch.full((G * 84 * 84 * C,), 0xAB, dtype=torch.uint8, device=DEV)
    actions = torch.full((G,), SENT, dtype=torch.int32, device=DEV)
    status = torch.full((1,), FOREIGN, dtype=torch.int32, device=DEV)
    net = (L._p(dev["slab"]), L._p(dev["tasks"]), G, G, L._p(dev["ws"]), L._p(status))   # one task per row
    if kind == "synth":
        state = torch.full((G, 4), 77, dtype=torch.int32, device=DEV)
        L.call("coevo_synth_step", L._p(state), L._p(acc), G, L._p(ord0), None, 0, 0, L._p(lim), None, None, L._p(rows), L._p(frames),
               C, n, seed)
        L.call("coevo_dqn16_out_synth_step", L._p(state), L._p(acc), G, L._p(ord0), None, 0, 1, L._p(lim), L._p(rows), L._p(actions),
               L._p(rows), L._p(frames), C, n, seed, *net)
        booked = state[:, 0]
    else:
        state = torch.full((G, L.K_DUEL["COEVO_DUEL_STATE_WORDS"]), 77, dtype=torch.int32, device=DEV)
        L.call("coevo_duel_step", L._p(state), L._p(acc), G, L._p(ord0), None, 0, 0, L._p(lim), None, None, L._p(rows), L._p(frames),
               C, n, seed, 3, 0)
        if kind == "duel":
            L.call("coevo_dqn16_out_duel_step", L._p(state), L._p(acc), G, L._p(ord0), None, 0, 1, L._p(lim), L._p(rows),
                   L._p(actions), L._p(rows), L._p(frames), C, n, seed, 3, 0, *net)
        else:   # second_0 is a scripted seat that always plays action 0; first_0's net is booked by the same launch
            seats = torch.tensor([[L.K_BL["COEVO_BL_CONSTANT"], 0, 0, 0]] * G, dtype=torch.int32, device=DEV)
            script = torch.full((G,), SENT, dtype=torch.int32, device=DEV)
            L.call("coevo_dqn16_out_duel_seat_step", L._p(state), L._p(acc), G, L._p(ord0), None, 0, 1, L._p(lim), L._p(seats), 1,
                   L._p(rows), L._p(actions), L._p(script), L._p(rows), L._p(frames), C, n, seed, 3, 0, *net)
        booked = None
    torch.cuda.synchronize()
    return actions.cpu().numpy(), int(status.item()), None if booked is None else booked.cpu().numpy()


@pytest.mark.parametrize("tiled", LAYOUTS, ids=["streamed", "tiled"])
@pytest.mark.parametrize("C,n", FULL)
def test_fused_output_rows_on_the_hidden_workspace(C, n, tiled):
    """dqn_out_row<true> in its env-step callers, fed the hidden rows of the output-sensitive classes: coevo_dqn16_out_synth_step,
    coevo_dqn16_out_duel_step and coevo_dqn16_out_duel_seat_step directly on the workspace coevo_dqn16_forward_hidden[_tiled] left
    (ties, rounding ties, out_last_step, NaN / -inf logits, the exact output words, signed zeros; one game per row, C = 4 and 6).
    Every live game's action word is the one coevo_dqn16_forward_argmax[_tiled] stores (the checker's), the status word is the
    foreign bit | NO_ACTION.  With the faulty rows in FINISHED games (limit 0) the launch raises nothing and leaves their action
    words alone"""
    names, nets, spec, frames = fused_cast(C, n)
    tasks, G = E.tile_rows(spec)
    frames = np.stack(frames)
    want, want_status = E.expected(tasks, nets, frames, C, n)
    assert want_status == E.NO_ACTION
    full = E.launch(tasks, nets, frames, C, n, tiled, FOREIGN)
    E.assert_rows(full, want, n, "argmax")
    hidden = E.launch(tasks, nets, frames, C, n, tiled, FOREIGN, hidden_only=True)
    assert hidden["rc"] == 0 and hidden["status"] == FOREIGN
    E.assert_rows(hidden, want, n, "hidden", hidden_only=True)
    faulty = np.array([w["status"] != 0 for w in want])
    assert faulty.sum() == 3 and names[-1] == "all_nan_logits"
    for kind in ("synth", "duel", "duel_seat"):
        actions, status, booked = fused_step(kind, hidden["dev"], C, n, G, [5] * G)
        assert np.array_equal(actions, full["actions"]), (kind, actions, full["actions"])
        assert status == FOREIGN | E.NO_ACTION, (kind, hex(status))
        if booked is not None:
            assert np.array_equal(booked, full["actions"]), kind
        limits = np.where(faulty, 0, 5)                       # the rows without an action belong to finished games
        actions, status, _ = fused_step(kind, hidden["dev"], C, n, G, limits)
        assert status == FOREIGN, (kind, "a finished game's NaN row raised", hex(status))
        assert (actions[faulty] == SENT).all() and np.array_equal(actions[~faulty], full["actions"][~faulty]), kind


# =============================================================================== c. containment
@pytest.mark.parametrize("C,n", FULL)
def test_faulty_net_beside_healthy_nets(C, n):
    """healthy net (16 rows), faulty net (5 rows), healthy net (1 row), healthy net (7 rows), both layouts, status preset to a
    foreign bit.  First nan_conv2.weight in the five rows, then nan_vbn3.bias in three of them and bn1_saturate in two (two
    tasks), then one_nan_logit / one_pos_inf (no status bit).  Every healthy row keeps the checker's bits - the ones that share
    a conv grid, a row group's pad rows or an XCD's task range with the faulty net included"""
    F = [E.ragged_frames(C)[i] for i in (0, 1, 2)] + [E.frame(C, "random"), E.frame(C, "hot_last")]
    for special, st in (([("nan_conv2.weight", F)], E.NO_ACTION), ([("nan_vbn3.bias", F[:3]), ("bn1_saturate", F[3:])], E.NO_ACTION),
                        ([("one_nan_logit", F[:3]), ("one_pos_inf", F[3:])], 0)):
        nets, spec, frames = [E.healthy(C, n, 0)], [(0, 16)], list(healthy_task(C, n, 0, 16)[1])
        for name, fr in special:
            nets.append(E.make(name, C, n))
            spec.append((len(nets) - 1, len(fr)))
            frames += fr
        for k, r, f0 in ((1, 1, 5), (2, 7, 3)):
            nets.append(E.healthy(C, n, k))
            spec.append((len(nets) - 1, r))
            frames += healthy_task(C, n, k, r, f0)[1]
        out, want, want_status = run_both(spec, nets, frames, C, n, [s for s, _ in special])
        assert want_status == st
        if st:
            assert np.isnan(out["logits"][16:21, :n]).all() and (out["actions"][16:21] == 0).all()
            assert np.isfinite(out["logits"][:16, :n]).all() and np.isfinite(out["logits"][21:, :n]).all()


@pytest.mark.parametrize("C,n", FULL + RUN_TIME_C[:1])
def test_one_faulting_row_inside_a_tile_of_healthy_rows(C, n):
    """overflow_on_full is healthy on every frame but the all-255 one.  A 16-row task with that frame at row 7, and a 5-row task
    of the same net with it as the LAST row (the row group's pad rows follow): fifteen (four) rows keep the checker's healthy
    bits, the one row is all NaN with action 0, status NO_ACTION - a NaN in one row of a matrix tile stays in its row"""
    w = E.make("overflow_on_full", C, n)
    rf = E.ragged_frames(C)
    sixteen = [rf[i] for i in range(16)]
    sixteen[7] = E.frame(C, "full")
    five = [rf[i] for i in (9, 10, 11, 12)] + [E.frame(C, "full")]
    out, want, st = run_both([(0, 16), (1, 2), (0, 5)], [w, E.healthy(C, n, 2)], sixteen + [rf[0], rf[1]] + five, C, n, "one row")
    assert st == E.NO_ACTION
    bad = [7, 22]
    assert all((w_["status"] == E.NO_ACTION) == (r in bad) for r, w_ in enumerate(want))
    assert np.isnan(out["hid"][bad]).all() and np.isnan(out["logits"][bad][:, :n]).all() and (out["actions"][bad] == 0).all()
    rest = np.delete(np.arange(23), bad)
    assert np.isfinite(out["hid"][rest]).all() and np.isfinite(out["act"][rest]).all() and np.isfinite(out["logits"][rest][:, :n]).all()


# =============================================================================== d. ragged tasks
def run_spec(C, n, spec, what, nets=None):
    """spec [(net k, rows)]: row i of a task shows frame i of the 16 ragged frames (an unserved row too)"""
    nets = [E.healthy(C, n, k) for k in range(4)] if nets is None else nets
    frames = [E.ragged_frames(C)[i % 16] for _, r in spec for i in range(max(r, 1))]
    return run_both(spec, nets, frames, C, n, what)


RAGGED = {
    "rows_4_5_8_9_12": [(0, 4), (1, 5), (2, 8), (3, 9), (0, 12)],              # NG = 1 | 2, 2 | 3, 3: both sides of a row-group edge
    "rows_13_16_0_1": [(1, 13), (2, 16), (3, 0), (0, 1)],                       # NG = 4, 4; a task without rows
    "rows_17_3": [(2, 17), (3, 3)],                                             # a task past COEVO_DQN_MAX_ROWS writes nothing
    "nine_tasks": [(k % 4, 1 + k % 3) for k in range(9)],                       # a grid rounded up to 16 tasks
    "seventeen_tasks": [(k % 4, 1 + (k * 5) % 4) for k in range(17)],           # a grid rounded up to 24 tasks
    # one net in adjacent tasks (tiled: SHARED_NET, plain loads), in non-adjacent tasks (non-temporal loads), and on either side of
    # a bad task of its own net (the neighbour's net_off is read, not its row count) and of another net
    "shared_net": [(0, 3), (0, 2), (1, 2), (2, 1), (1, 4), (3, 2), (3, 0), (3, 5), (2, 1), (0, 0), (2, 2), (3, 16)],
}


@pytest.mark.parametrize("C,n", FULL)
@pytest.mark.parametrize("name", list(RAGGED))
def test_ragged_tasks(name, C, n):
    """row counts on both sides of every row-group edge of dqn16_fc1_body<NG> (4 | 5, 8 | 9, 12 | 13, 16), 17 and 0 rows
    (COEVO_ST_BAD_TASK: the rows nobody writes keep NaN in the workspace and poison in logits and actions), 9 and 17 tasks, one net
    in adjacent / non-adjacent tasks and round a bad task (the tiled kernel's plain / non-temporal choice reads the neighbours'
    net_off), the net in the slab's last slot under a 16-row task, and in every task row i shows frame i - a row or task mix-up
    cannot return a matching vector (the 64 filler pairs differ pairwise: tests/test_dqn16_edges_cpu.py)"""
    spec = RAGGED[name]
    out, want, st = run_spec(C, n, spec, name)
    bad = any(not 1 <= r <= 16 for _, r in spec)
    assert st == (E.BAD_TASK if bad else 0) and sum(w is None for w in want) == sum(max(r, 1) for _, r in spec if not 1 <= r <= 16)
    if name == "shared_net":
        nets = [k for k, _ in spec]
        assert nets[0] == nets[1] and nets[2] == nets[4] != nets[3] and nets[5] == nets[6] == nets[7] and nets[8] == nets[10] != nets[9]
        assert spec[-1] == (3, 16)     # the slab's last net, sixteen rows


@pytest.mark.parametrize("C,n", RUN_TIME_C)
def test_ragged_tasks_run_time_channel_counts(C, n):
    run_spec(C, n, RAGGED["rows_4_5_8_9_12"], "ragged")
    run_spec(C, n, RAGGED["shared_net"], "shared")


# =============================================================================== e. pack / unpack
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 2.0 ** -24, -(2.0 ** -24), 65504.0], dtype=np.float32)


@pytest.mark.parametrize("C,n", [(4, 6), (5, 18)])
def test_pack_and_unpack_carry_special_values_in_every_section(C, n):
    """NaN, +-inf, -0 and the smallest subnormal at the first, a middle and the last places of each of the 16 tensors: through
    coevo_dqn16_pack / _unpack and coevo_dqn16_pack_tiled / _unpack_tiled every entry comes back with its bits (a NaN as a NaN)"""
    lib = L.load()
    flat = E.base_net(C, n, 1699)
    for name, (off, shp) in E.offsets(C, n).items():
        m = int(np.prod(shp))
        k = min(m, len(SPECIALS))
        assert m >= 3 * k or m == n
        for at in (off, off + (m - k) // 2, off + m - k):
            flat[at:at + k] = SPECIALS[:k]
    stride = int(lib.coevo_dqn16_slab_stride(C, n))
    d_flat = torch.from_numpy(flat[None]).to(DEV)
    for sfx in ("", "_tiled"):
        slab = torch.full((stride,), E.POISON_I32, dtype=torch.int32, device=DEV)
        back = torch.full((1, flat.size), 7.0, dtype=torch.float32, device=DEV)
        L.call("coevo_dqn16_pack" + sfx, L._p(d_flat), L._p(slab), 1, C, n)
        L.call("coevo_dqn16_unpack" + sfx, L._p(slab), L._p(back), 1, C, n)
        torch.cuda.synchronize()
        got = back.cpu().numpy()[0]
        assert E.same_bits_up_to_nan(got, flat), (sfx, np.flatnonzero(words(got) != words(flat))[:8])
        assert int(np.isnan(got).sum()) == int(np.isnan(flat).sum()) >= 3 * 16 - 2
