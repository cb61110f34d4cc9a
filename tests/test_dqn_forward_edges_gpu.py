"""Status word, fault containment, ties, dead channels, subnormals and ragged tasks in EVERY fp32 DeepQN forward kernel, against
the oracle (csrc/deepqn.hip, csrc/dqn_conv.hip.h, dqn_out_row in csrc/dqn_common.hip.h, synth_step_kernel<true> in
csrc/dqn_engine.hip).

The judge is always rp.dqn_forward through the cache of tests/dqn_edge_nets.py; logits are compared as uint32 patterns (a NaN
matches any NaN: the default NaNs of the two machines differ), actions with the oracle's, the oracle's -1 (no logit compares
greater than -inf) being action 0 with COEVO_ST_NO_ACTION on the device.  No tolerance anywhere.  tests/test_dqn_edges_cpu.py
pins the nets' properties on the oracle alone, so nothing here can pass vacuously.

Launch shapes (dqn_forward_launch: <= 32 rows take the three small conv launches, more the one-workgroup-per-frame kernel;
<= 16 tasks take the narrow fc1 kernels, more the wide ones; the streamed wide kernel keeps a ring of 8 chunks up to 128 tasks
and of 2 above; the tiled wide kernel has one ring depth):

  shape  rows   tasks   conv kernels                         fc1, streamed layout              fc1, tiled layout
  S1     <= 32  <= 16   dqn_small_conv1/2/3_kernel           dqn_fc1_narrow_kernel<4>          dqn_fc1_narrow_tiled_kernel<4>
  S2     <= 32  17-32   dqn_small_conv1/2/3_kernel           dqn_fc1_kernel<8>                 dqn_fc1_tiled_kernel<7>
  S3     33-48  <= 16   dqn_conv_kernel                      dqn_fc1_narrow_kernel<4>          dqn_fc1_narrow_tiled_kernel<4>
  S4     > 32   17-128  dqn_conv_kernel                      dqn_fc1_kernel<8>                 dqn_fc1_tiled_kernel<7>
  S5     > 128  >= 129  dqn_conv_kernel                      dqn_fc1_kernel<2>                 dqn_fc1_tiled_kernel<7>

The conv template follows the channel count: <4, 4> for C = 4, <4, 0> for C = 3, <6, 6> for C = 6, <6, 0> for C = 5 (both
dqn_small_conv1_kernel and dqn_conv_kernel).  dqn_out_kernel (dqn_out_row's first caller) ends every one of these launches; its
second caller, synth_step_kernel<true>, is section d.

Only numerical conditions are provoked: every launch has the shape of one the suite already runs, all pointers valid."""
import numpy as np
import pytest
import torch

from coevonet_amd import lib as L
from oracle import ref_port as rp
from tests import dqn_edge_nets as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
FOREIGN = 0x1000          # a bit no COEVO_ST_* uses: the status word is OR-ed into, so it must survive every launch
SHAPES = ["S1", "S2", "S3", "S4", "S5"]
LAYOUTS = [0, L.DQN_FC1_TILED]
TASKS_OF = {"S1": (1, 16), "S2": (17, 32), "S3": (1, 16), "S4": (17, 128), "S5": (129, 100000)}
ROWS_OF = {"S1": (1, 32), "S2": (1, 32), "S3": (33, 48), "S4": (33, 100000), "S5": (129, 100000)}


@pytest.fixture(scope="module", autouse=True)
def release_nets():
    yield
    E.release()


class Launch:
    """one launch under construction: nets by identity, tasks in row order, a frame per row.  Healthy rows come from the 64
    cached (healthy net k, random frame i) pairs: row i of a healthy task shows frame i"""

    def __init__(self, C, n):
        self.C, self.n, self.nets, self.layout, self.frames, self.tags = C, n, [], [], [], []
        self._filler = 0

    def net_index(self, net):
        for i, w in enumerate(self.nets):
            if w is net:
                return i
        self.nets.append(net)
        return len(self.nets) - 1

    def task(self, net, frames, tag="healthy"):
        self.layout.append((self.net_index(net), len(frames)))
        self.frames += list(frames)
        self.tags += [tag] * len(frames)
        return self

    def healthy(self, k, rows, first_frame=0):
        return self.task(E.healthy(self.C, self.n, k % 4), [E.ragged_frames(self.C)[(first_frame + i) % 16] for i in range(rows)])

    def fill(self, n_tasks, k0=3):
        """one-row healthy tasks until the launch has n_tasks tasks: nets cycle (adjacent tasks never share one), frames move
        on with every cycle"""
        while len(self.layout) < n_tasks:
            j = self._filler
            self._filler += 1
            self.healthy(k0 + j, 1, first_frame=1 + j // 4)
        return self

    def run(self, tiled, shape=None, preset=FOREIGN):
        rows = len(self.frames)
        if shape is not None:   # the launch takes the path its name says
            assert TASKS_OF[shape][0] <= len(self.layout) <= TASKS_OF[shape][1], (shape, len(self.layout))
            assert ROWS_OF[shape][0] <= rows <= ROWS_OF[shape][1], (shape, rows)
        frames = np.stack(self.frames)
        self.want, self.want_status = E.expected(self.layout, self.nets, frames, self.C, self.n)
        self.logits, self.actions, self.status, self.rc = E.launch(self.layout, self.nets, frames, self.C, self.n, tiled, preset)
        return self

    def check(self, what):
        """return code 0, every row the oracle's, the status word exactly the preset bit | what the oracle's actions imply"""
        assert self.rc == 0, what
        E.assert_rows(self.logits, self.actions, self.want, what)
        assert self.status == FOREIGN | self.want_status, f"{what}: status word {self.status:#x}, want {FOREIGN | self.want_status:#x}"
        return self


def shaped(C, n, shape, special, head_rows=16):
    """a launch of the given shape around the `special` tasks [(net, frames, tag)]: healthy net 0 in front (head_rows rows; 3
    in S1 / S2, which hold 32 rows at most), healthy nets 1 and 2 behind (1 and 7 rows; 1 and 2 in S1 / S2), then what the
    shape needs: an 8-row task for S3's row count, one-row tasks for the task counts of S2 (17), S4 (18) and S5 (130).
    No two adjacent tasks share a net: every wide fc1 workgroup takes its SHARED_NET = false instantiation"""
    small = shape in ("S1", "S2")
    ln = Launch(C, n).healthy(0, min(head_rows, 3) if small else head_rows)
    for net, frames, tag in special:
        ln.task(net, frames, tag)
    ln.healthy(1, 1, first_frame=5).healthy(2, 2 if small else 7, first_frame=3)
    if shape == "S3" and len(ln.frames) <= 32:
        ln.healthy(3, 8, first_frame=7)
    return ln.fill({"S1": 0, "S2": 17, "S3": 0, "S4": 18, "S5": 130}[shape])


# =============================================================================== a. every class on every launch path
def class_rows(C, n, names):
    """[(net, [frame], tag)]: one row per class on the random named frame; "plain@<frame>" = the plain net on that frame"""
    F, out = E.FRAMES(C), []
    for name in names:
        cls, _, fname = name.partition("@")
        out.append((E.make(cls, C, n), [F[fname or "random"]], name))
    return out


def run_all_paths(C, n, names):
    """the class rows inside a launch of each of the five shapes, for both fc1 layouts; filler rows are checked as well"""
    want_status = None
    for shape in SHAPES:
        for tiled in LAYOUTS:
            ln = shaped(C, n, shape, class_rows(C, n, names)).run(tiled, shape)
            ln.check(f"C={C} n={n} {shape} tiled={tiled} {names}")
            want_status = ln.want_status
    return want_status


PLAIN_FRAMES = ["plain@" + f for f in ("random", "zeros", "full", "planes", "hot_first", "hot_last")]
QUIET = PLAIN_FRAMES + [c for c in E.NO_FAULT if c != "plain" and c not in E.SUB_SCALE]
QUIET_GROUPS = [QUIET[i:i + 8] for i in range(0, len(QUIET), 8)]


@pytest.mark.parametrize("group", range(len(QUIET_GROUPS)))
def test_quiet_classes_on_every_path(group):
    """C = 4, n = 6; eight classes that raise no status per launch, one row each, among healthy tasks: the plain net on the six
    named frames (the hot first / last byte of a frame: the staging loops of dqn_conv_kernel<4, 4> and
    dqn_small_conv1_kernel<4, 4>), ties (first maximum), signed zeros, one +inf, one NaN logit, NaN in output.weight /
    output.bias, finite 1e37-sized logits, dead conv channels (the summation order of the BatchNorm statistics in
    bn_relu_rows), gamma = 0 / < 0, beta = -10.  Status stays the preset bit.
    Reaches: both conv paths x <4, 4>; all five fc1 kernels (narrow, narrow tiled, dqn_fc1_kernel<8> and <2>, tiled); in the
    wide kernels NG = 1 (the class rows and fillers), 2 (the 7-row task) and 4 (16 rows), SHARED_NET false; dqn_out_kernel"""
    assert run_all_paths(4, 6, QUIET_GROUPS[group]) == 0


@pytest.mark.parametrize("name", sorted(E.SUB_SCALE))
def test_subnormal_classes_on_every_path(name):
    """C = 4, n = 6: subnormal weights through v_mfma_f32_16x16x4 (the conv stack, the narrow and tiled fc1 kernels),
    v_mfma_f32_4x4x1 (dqn_fc1_kernel) and the fmaf chain of dqn_out_row, on the random frame and on both hot-byte frames - the
    frames on which tests/test_dqn_edges_cpu.py shows that a flushing unit would give other logits.  No kernel flushes: the
    device has the unflushed oracle's bits on all ten paths"""
    assert run_all_paths(4, 6, [f"{name}@{f}" for f in ("random", "hot_first", "hot_last")]) == 0


@pytest.mark.parametrize("name", E.MAY_FAULT)
def test_fault_classes_on_every_path(name):
    """C = 4, n = 6; one class per launch: NaN in each of the 14 tensors in front of the output layer (the BatchNorm affine,
    which the slab stores beside the conv bias, included), inf in a conv / fc1 / output weight, conv weights x 1e38 (inf - inf in
    BatchNorm), all logits -inf, all logits NaN.  The status word is exactly preset | NO_ACTION where the oracle returns -1
    for the row (the two inf classes behind the conv stack: whatever the oracle says), the row's logits are the oracle's up to
    NaN, its action 0, and every filler row of the launch keeps the oracle's bits.  Kernels reached: as the quiet classes"""
    st = run_all_paths(4, 6, [name])
    if E.PROPERTY[name][0] == -1:
        assert st == E.NO_ACTION


OTHER_C = [(3, 6), (5, 18), (6, 18)]
SMALL_SET = ["tie_all", "tie2", "tie2_0_last", "tie2_last2", "signed_zeros", "one_pos_inf", "one_nan_logit",
             "plain@hot_first", "plain@hot_last", "plain@random"]


@pytest.mark.parametrize("C,n", OTHER_C)
def test_ties_and_hot_bytes_other_channel_counts(C, n):
    """C = 3 (<4, 0>: run-time channel count), 5 (<6, 0>) and 6 (<6, 6>) in both conv paths: ties, signed zeros, one +inf,
    one NaN logit, the hot first / last byte of a frame.  n = 18: lanes 0 .. 17 of dqn_out_row and a longer argmax scan"""
    assert run_all_paths(C, n, SMALL_SET[:5]) == 0
    assert run_all_paths(C, n, SMALL_SET[5:]) == 0


@pytest.mark.parametrize("C,n", OTHER_C)
@pytest.mark.parametrize("name", ["all_neg_inf", "all_nan_logits"] + [f"nan_{t}" for t in E.TENSORS if not t.startswith("output.")])
def test_nan_classes_other_channel_counts(name, C, n):
    """NaN in every tensor in front of the output layer, all -inf, all NaN for C = 3, 5, 6 on all ten paths: conv1's weight block
    and everything behind it sit at channel-dependent slab offsets (dqn_layout)"""
    assert run_all_paths(C, n, [name]) == E.NO_ACTION


@pytest.mark.parametrize("C,n", OTHER_C)
def test_nan_in_the_output_layer_other_channel_counts(C, n):
    """one NaN in output.weight / output.bias for C = 3, 5, 6 (n = 18: the NaN sits in lane 9 / 10 of dqn_out_row): exactly one
    NaN logit, no status bit, the first maximum of the others; all ten paths as above, dqn_out_kernel behind each"""
    assert run_all_paths(C, n, ["nan_output.weight", "nan_output.bias"]) == 0


# =============================================================================== b. containment and the status word
@pytest.mark.parametrize("tiled", LAYOUTS, ids=["streamed", "tiled"])
@pytest.mark.parametrize("shape", SHAPES)
def test_faulty_net_beside_healthy_nets(shape, tiled):
    """healthy net (16 rows; 3 in S2, whose <= 32 rows cannot hold 16 + 5 + 1 + 7 rows AND 17 tasks), faulty net (5 rows),
    healthy net (1 row), healthy net (7 rows), an 8-row task for S3's row count and one-row healthy tasks up to the task
    counts of S2, S4 and S5; the status word preset to 0x1000.  First launch: nan_conv2.weight in the five rows;
    second: nan_vbn3.bias in three of them and overflow_conv1 in the other two (two tasks).  Return code 0, status exactly
    0x1000 | 16, the faulty rows all NaN with stored action 0, every healthy row the oracle's bits and action - the ones that
    share a conv grid, a 16-row matrix tile's pad rows (narrow kernels: rows past the task's last repeat it; wide kernels:
    zeros) or an XCD's task range with the faulty net included.  Third launch: only one_nan_logit and one_pos_inf nets beside
    the healthy ones: status stays 0x1000, actions are the oracle's.
    Reaches: every row of the table in the module docstring at C = 4; NG = 2 with NaN weights (five rows = two row groups
    of dqn_fc1_body, pad rows of the second fed with NaN weights and zero activations)"""
    C, n = 4, 6
    F = E.FRAMES(C)
    five = [E.ragged_frames(C)[i] for i in (0, 1, 2)] + [F["random"], F["hot_last"]]

    def build(special):
        ln = Launch(C, n).healthy(0, 3 if shape == "S2" else 16)
        for net, frames, tag in special:
            ln.task(net, frames, tag)
        ln.healthy(1, 1, first_frame=5).healthy(2, 7, first_frame=3)
        if shape == "S3":
            ln.healthy(3, 8, first_frame=7)
        return ln.fill({"S1": 0, "S2": 17, "S3": 0, "S4": 18, "S5": 130}[shape])

    for special in ([(E.make("nan_conv2.weight", C, n), five, "faulty")],
                    [(E.make("nan_vbn3.bias", C, n), five[:3], "faulty"), (E.make("overflow_conv1", C, n), five[3:], "faulty")]):
        ln = build(special).run(tiled, shape, preset=FOREIGN)
        what = f"{shape} tiled={tiled} {[t for _, _, t in special]}"
        assert ln.rc == 0 and ln.status == FOREIGN | E.NO_ACTION, f"{what}: rc {ln.rc}, status {ln.status:#x}"
        faulty = np.array([t == "faulty" for t in ln.tags])
        assert faulty.sum() == 5 and np.isnan(ln.logits[faulty]).all() and (ln.actions[faulty] == 0).all(), what
        assert all(a == -1 for (a, _), f in zip(ln.want, faulty) if f) and all(a >= 0 for (a, _), f in zip(ln.want, faulty) if not f)
        E.assert_rows(ln.logits, ln.actions, ln.want, what)
    ln = build([(E.make("one_nan_logit", C, n), five[:3], "quiet"), (E.make("one_pos_inf", C, n), five[3:], "quiet")])
    ln.run(tiled, shape, preset=FOREIGN).check(f"{shape} tiled={tiled} one NaN / one +inf logit")
    assert ln.status == FOREIGN
    quiet = np.array([t == "quiet" for t in ln.tags])
    assert np.isnan(ln.logits[quiet][:3, 0]).all() and (ln.logits[quiet][3:, 2] == np.inf).all() and (ln.actions[quiet][3:] == 2).all()


# =============================================================================== c. ragged tasks in every fc1 kernel
def ragged(C, n, kind):
    """tasks of 1, 2, ..., 16 rows over the four healthy nets in turn (row i of a task: frame i, so all 64 cached pairs occur);
    "17": plus a one-row task; "runs": plus a run of two tasks (2 and 7 rows) and a run of three (12, 16, 3 rows) of ONE net
    each = SHARED_NET with 1, 2 and 3, 4, 1 row groups; "many": the sixteen sizes eight times over and the runs = 133 tasks"""
    ln = Launch(C, n)
    for rep in range(8 if kind == "many" else 1):
        for r in range(1, 17):
            ln.healthy(r + rep, r)          # (r + rep) % 4: adjacent tasks of different nets, also across the repeats
    if kind in ("17", "runs", "many"):
        ln.healthy(1 if kind != "many" else 0, 1)
    if kind in ("runs", "many"):
        k = len(ln.layout)
        for net, rows in ((k + 1, 2), (k + 1, 7), (k + 2, 12), (k + 2, 16), (k + 2, 3)):
            ln.healthy(net, rows)
        nets = [ln.layout[i][0] for i in range(k - 1, k + 5)]
        assert nets[0] != nets[1] == nets[2] != nets[3] == nets[4] == nets[5]
    # outside the runs no two adjacent tasks share a net (they would take the SHARED_NET instantiation unnoticed)
    n_shared = sum(a[0] == b[0] for a, b in zip(ln.layout, ln.layout[1:]))
    assert n_shared == (3 if kind in ("runs", "many") else 0)
    return ln


@pytest.mark.parametrize("C,n", [(4, 6), (6, 18)])
@pytest.mark.parametrize("kind", ["16", "17", "runs", "many"])
def test_ragged_tasks_in_every_fc1_kernel(kind, C, n):
    """every task row count 1 .. 16 in one launch, both fc1 layouts, each of the 64 (net, frame) pairs in many rows:
      16   (16 tasks, 136 rows)   dqn_fc1_narrow_kernel<4> / dqn_fc1_narrow_tiled_kernel<4>: the store guard 4 kk + i < nrows
                                  and the row clamp min(c, nrows - 1) at every nrows
      17   (17 tasks, 137 rows)   dqn_fc1_kernel<8> / dqn_fc1_tiled_kernel<7>: dqn_fc1_body<NG, 8, false> for NG = 1, 2, 3, 4
                                  (four task sizes each) and the guard r < nrows of its store
      runs (22 tasks, 177 rows)   ... plus dqn_fc1_body<NG, 8, true> for NG = 1, 2, 3, 4 and dqn_fc1_tiled_body<7, true>
      many (134 tasks, 1129 rows) dqn_fc1_kernel<2>: dqn_fc1_body<NG, 2, false> and <NG, 2, true> for NG = 1 .. 4; the row ->
                                  task search and the XCD task ranges over 134 tasks; dqn_fc1_tiled_kernel<7> at that size
    More than 32 rows each: dqn_conv_kernel<4, 4> / <6, 6>"""
    for tiled in LAYOUTS:
        ln = ragged(C, n, kind).run(tiled)
        assert len(ln.layout) == {"16": 16, "17": 17, "runs": 22, "many": 134}[kind]
        assert len(ln.frames) == {"16": 136, "17": 137, "runs": 177, "many": 1129}[kind]
        assert ln.check(f"ragged {kind} C={C} n={n} tiled={tiled}").status == FOREIGN


@pytest.mark.parametrize("C,n", [(3, 6), (5, 18)])
def test_ragged_tasks_run_time_channel_counts(C, n):
    """the 17-task shape for C = 3 and 5: dqn_conv_kernel<4, 0> / <6, 0> in front of dqn_fc1_kernel<8> / dqn_fc1_tiled_kernel<7>"""
    for tiled in LAYOUTS:
        ragged(C, n, "17").run(tiled).check(f"ragged 17 C={C} n={n} tiled={tiled}")


# =============================================================================== d. the fused output layer
SEED = 0x5EED1234


def play_twins(C, n, cast, limits, ordinals):
    """games = rows; cast = [(class, rows)] in row order.  coevo_synth_step(t = 0) writes the frames, then
    twin A: coevo_dqn_forward_argmax + coevo_synth_step(t = 1);  twin B, on copies of the state: coevo_dqn_forward_hidden_timed
    (no timing context) + coevo_dqn_out_synth_step(t = 1).  -> per twin dict(actions, gstate, acc, frames, status), the frames
    of t = 0, the nets of the rows"""
    lib = L.load()
    nets = [E.make(name, C, n) for name, _ in cast]
    layout = [(i, r) for i, (_, r) in enumerate(cast)]
    G = sum(r for _, r in layout)
    stride = int(lib.coevo_dqn_slab_stride(C, n))
    tasks, net_of_row = E.task_table(layout, stride)
    slab = torch.zeros(len(nets), stride, dtype=torch.float32, device=DEV)
    L.call("coevo_dqn_pack", L._p(torch.from_numpy(np.stack(nets)).to(DEV)), L._p(slab), len(nets), C, n)
    d_tasks = L.tasks_to_device(tasks, DEV)
    rows = torch.arange(G, dtype=torch.int32, device=DEV)
    lim = torch.tensor(limits, dtype=torch.int32, device=DEV)
    ord0 = torch.tensor(ordinals, dtype=torch.int64, device=DEV)
    stale = np.random.Generator(np.random.PCG64(9)).integers(0, 256, size=(G, 84, 84, C), dtype=np.uint8)
    frames0 = torch.from_numpy(stale).to(DEV)      # a game that never starts keeps these bytes in its row
    gstate0 = torch.full((G, 4), 77, dtype=torch.int32, device=DEV)
    acc0 = torch.full((G, 3), 5.5, dtype=torch.float64, device=DEV)
    L.call("coevo_synth_step", L._p(gstate0), L._p(acc0), G, L._p(ord0), None, 0, 0, L._p(lim), None, None, L._p(rows),
           L._p(frames0), C, n, SEED)
    torch.cuda.synchronize()
    out = {}
    for twin in "AB":
        gs, ac, fr = gstate0.clone(), acc0.clone(), frames0.clone()
        actions = torch.full((G,), E.SENT_A, dtype=torch.int32, device=DEV)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        ws = torch.zeros(int(lib.coevo_dqn_workspace_bytes(G)) // 4, dtype=torch.float32, device=DEV)
        if twin == "A":
            L.call("coevo_dqn_forward_argmax", L._p(slab), L._p(d_tasks), len(layout), 16, G, C, n, L._p(fr), L._p(actions),
                   None, L._p(status), L._p(ws))
            L.call("coevo_synth_step", L._p(gs), L._p(ac), G, L._p(ord0), None, 0, 1, L._p(lim), L._p(rows), L._p(actions),
                   L._p(rows), L._p(fr), C, n, SEED)
        else:
            L.call("coevo_dqn_forward_hidden_timed", L._p(slab), L._p(d_tasks), len(layout), 16, G, C, n, L._p(fr), L._p(ws),
                   None, 0)
            L.call("coevo_dqn_out_synth_step", L._p(gs), L._p(ac), G, L._p(ord0), None, 0, 1, L._p(lim), L._p(rows),
                   L._p(actions), L._p(rows), L._p(fr), C, n, SEED, L._p(slab), L._p(d_tasks), len(layout), G, L._p(ws),
                   L._p(status))
        torch.cuda.synchronize()
        out[twin] = dict(actions=actions.cpu().numpy(), gstate=gs.cpu().numpy(), acc=ac.cpu().numpy(), frames=fr.cpu().numpy(),
                         status=int(status.item()))
    return out, frames0.cpu().numpy(), stale, [nets[k] for k in net_of_row]


def assert_twins_agree(out, live):
    A, B = out["A"], out["B"]
    assert np.array_equal(A["actions"][live], B["actions"][live])
    assert np.array_equal(A["gstate"], B["gstate"]) and np.array_equal(A["acc"].view(np.uint64), B["acc"].view(np.uint64))
    assert np.array_equal(A["frames"], B["frames"])


GAMES = dict(cast=[("plain", 3), ("tie_all", 2), ("tie2", 3), ("signed_zeros", 2), ("one_nan_logit", 2)],
             #        plain      | tie_all | tie2       | zeros  | one NaN
             limits=[5, 0, 5,      5, 1,     5, 5, 5,     5, 5,    1, 5],
             ordinals=[3, 4, 5,    6, 7,     8, -9, 10,   11, 12,  13, 1 << 33])


@pytest.mark.parametrize("C,n", [(4, 6), (6, 18)])
def test_fused_output_layer_equals_the_separate_pair(C, n):
    """include/coevo.h: coevo_dqn_forward_hidden_timed + coevo_dqn_out_synth_step give the results of coevo_dqn_forward_argmax +
    coevo_synth_step.  Twelve games over five nets (ties, signed zeros, a NaN logit), one with its limit already reached
    (limit 0), one disabled (negative ordinal), two at their last step (limit 1: booked, no next frame), one with an ordinal
    past 2^32: equal booked actions of the live games, equal game state, fp64 returns bit for bit, equal next frames byte for
    byte, status 0 in both; the booked action of every live game is the oracle's on the frame of t = 0, which is
    oracle_synth_frame's.  Reaches dqn_out_row from synth_step_kernel<true> (256 threads: lanes 0 .. n - 1 of wave 0 work, the
    rest only meet the barriers) behind the small conv launches and dqn_fc1_narrow_kernel<4>"""
    cast, limits, ordinals = GAMES["cast"], np.array(GAMES["limits"]), np.array(GAMES["ordinals"])
    out, frames0, stale, net_of_game = play_twins(C, n, cast, limits, ordinals)
    live = (limits >= 1) & (ordinals >= 0)
    assert live.sum() == 10 and (limits[live] == 1).sum() == 2
    assert_twins_agree(out, live)
    assert out["A"]["status"] == out["B"]["status"] == 0
    B = out["B"]
    assert (B["actions"][~live] == E.SENT_A).all()       # the fused launch skips the output layer of a finished game
    for g in range(len(limits)):
        if not live[g]:
            assert np.array_equal(frames0[g], stale[g]) and np.array_equal(B["frames"][g], stale[g])
            assert list(B["gstate"][g][:2]) == [0xFF, 0] and not B["acc"][g].any()
            continue
        f0 = rp.synth_frame(SEED, int(ordinals[g]), 0, 0xFF, C)
        assert np.array_equal(frames0[g], f0), g
        a, _ = E.oracle(net_of_game[g], f0, C, n)
        assert a >= 0 and B["actions"][g] == a == B["gstate"][g][0], (g, a, B["actions"][g])
        hit = int(a == rp.lib().oracle_synth_target(SEED, int(ordinals[g]), 0, n))
        assert B["gstate"][g][1] == hit and list(B["acc"][g]) == [-float(hit), 0.0, 0.0]
        want_next = rp.synth_frame(SEED, int(ordinals[g]), 1, a, C) if limits[g] > 1 else f0
        assert np.array_equal(B["frames"][g], want_next), g
    assert len({int(B["actions"][g]) for g in np.flatnonzero(live)}) > 1


@pytest.mark.parametrize("C,n", [(4, 6), (6, 18)])
def test_fused_output_layer_no_action(C, n):
    """all_nan_logits in a live game and in a finished game: both twins raise COEVO_ST_NO_ACTION and book action 0 for the
    live game.  With the faulty net in the FINISHED game only, the twins' status words differ, as include/coevo.h says:
    dqn_out_kernel runs the output layer of every row, synth_step_kernel<true> only for games with t - 1 < limit, so the
    fused launch raises nothing for a row whose action is never booked (and leaves actions_prev[row] as it was)"""
    cast = [("plain", 3), ("all_nan_logits", 2), ("tie2", 2)]
    ordinals = np.array([3, 4, 5, 6, 7, 8, 9])
    for limits, want in ((np.array([5, 5, 5, 5, 0, 5, 1]), (E.NO_ACTION, E.NO_ACTION)),
                         (np.array([5, 5, 5, 0, 0, 5, 1]), (E.NO_ACTION, 0))):
        out, frames0, stale, net_of_game = play_twins(C, n, cast, limits, ordinals)
        live = limits >= 1
        assert_twins_agree(out, live)
        assert (out["A"]["status"], out["B"]["status"]) == want
        assert (out["A"]["actions"][3:5] == 0).all()                      # the separate pair stores action 0 for both rows
        assert (out["B"]["actions"][~live] == E.SENT_A).all()
        for g in np.flatnonzero(live):
            a, lg = E.oracle(net_of_game[g], rp.synth_frame(SEED, int(ordinals[g]), 0, 0xFF, C), C, n)
            assert out["B"]["actions"][g] == max(a, 0) == out["B"]["gstate"][g][0]
            assert (a == -1) == (g in (3, 4))
