"""Fault bits, ties, signed zeros and subnormals in EVERY fp32 policy-forward body of csrc/fc_forward.hip (fc_policy_body:
csrc/fc_body_unrolled.hip.h, fc_policy_body_c: fc_body_compact.hip.h, fc_policy_mfma_body: fc_body_mfma32.hip.h, fc_policy_mfma16_body:
fc_body_mfma16.hip.h, fc_rollout_small_kernel: fc_rollout_persistent.hip.h; the helpers: fc_forward_common.hip.h), against the oracle.

The bodies share the output chain, the first-maximum argmax with its BAD_OUT / NO_ACTION bits, the action store and (the two
lean forms) most of the packed LayerNorm passes as helpers; the observation entry, fc1, fc2 and the BAD_INPUT / BAD_FC1 /
BAD_FC2 detection of the tile bodies are still written out once per body, and a helper is inlined into every body's own
register budget, so the nets of
tests/fc_edge_nets.py (ties, -0, +-inf, NaN, variance 0, subnormal fc1 / fc2 weights) go through each of them.  Expected
logits, actions and status words are always rp.fc_forward's / rp.play_game_status's (oracle/coevo_oracle.c); finite values,
infinities and the sign of zero are compared as bits, NaN by NaN-ness (x86 and gfx950 have different default NaNs), and the
status word by equality with the OR of the oracle's words, so a missing bit fails like a surplus one.  No tolerance anywhere.

Cells (entry point, kernel form, row-count instantiation R) and where each is launched:

  observations given (sections "healthy", "fault", "per-row", "padding"; D = 8 and 10 each)
    coevo_fc_forward_argmax   fc_policy_body<R, MODE_OBS, 1>            R = 1, 2, 5, 8
    coevo_fc_forward_argmax   fc_policy_mfma_body<MODE_OBS>             32-row tiles (tasks of 32, 17, 9, 29, 1, 24 rows)
    coevo_fc_forward_merged   fc_policy_mfma16_body<MODE_OBS>           16-row tiles: tasks of 9..16 rows and of 5 / 1 rows
    coevo_fc_forward_merged   fc_policy_body_c<R, MODE_OBS, FC2_MFMA>   R = 1, 2, 5, 8
    merged_tiled              ... the 16-row table through the TILED branch of fc_policy_mfma16_body: every task of it carries
                              COEVO_TASK_TILED and reads its net's tile-major twin (coevo_fc_w2_tile_major, behind the nets in
                              the slab's allocation), the net's canonical fc2.weight is NaN in the slab - healthy, fault
                              (heavy16 and heavy_few, every class), per-row and padding sections
    merged_tiled_res          ... with COEVO_TASK_RESIDENT or-ed into those tasks: the same words (healthy section)
  state driven (whole games through RolloutPlan / DeviceRollout; the form is asserted, never assumed)
    persistent1 / persistent2 coevo_mpe_rollout_persistent, fc_rollout_small_kernel<8>, one / two cohorts
    small                     fc_cycle_small_kernel<8>: fc_policy_body_c<8, MODE_FUSED, FC2_DPP> for every task
    lean16                    fc_cycle16_kernel<5>: fc_policy_mfma16_body<MODE_FUSED> + fc_policy_body_c<5, MODE_FUSED>
    lean16_resident           ... with COEVO_TASK_RESIDENT on every other per-individual task (the RES = true twin)
    lean16_tiled              ... with COEVO_TASK_TILED on every shared-opponent task, as GAEngine._enable_hof_tiled sets it:
                              fc_policy_mfma16_body<MODE_FUSED>'s TILED branch; the shared opponents' canonical fc2.weight is
                              NaN in the slab, their twins are rebuilt after every packing (the oracle's games are lean16's)
    tile32                    fc_cycle_kernel<5, 1>: fc_policy_mfma_body<MODE_FUSED> + fc_policy_body<5, MODE_FUSED, 1>
    paired                    fc_cycle_kernel<1, 2>: 523 one-row nets, two per workgroup, the last workgroup with one
    two_launch                merged=False: coevo_mpe_policy_cycle_fused twice per cycle, fc_policy_mfma_kernel<MODE_FUSED>
                              beside fc_policy_kernel<5, MODE_FUSED> (fc_policy_body_c)
    plain                     coevo_mpe_policy_cycle + coevo_mpe_step: fc_policy_mfma_body<MODE_STATE> and
                              fc_policy_body<5, MODE_STATE, 1>
  COEVO_TASK_TILED where it must be ignored (include/coevo.h: "Every other launch and every per-individual task ignores it"):
  the bit names an in-allocation twin region that is NaN throughout, the nets are healthy and whole - status 0, the oracle's words
    coevo_fc_forward_merged   the light table, R = 1, 2, 5, 8, TILED and RESIDENT | TILED
    coevo_fc_forward_argmax   R = 1, 2, 5, 8, 32
    *_flagged                 persistent1, small, tile32, paired, two_launch, plain: every heavy and light task flagged;
                              lean16_light / lean16_light_resident: the per-individual tasks of the lean16 form

The non-finite STATE case runs on every form, the persistent one included: its launch reads the reset state from a buffer
the caller owns (DeviceRollout.state), so the test seeds it between reset() and run() without touching product code.

Only numerical status bits are provoked: every launch has the shape of one the suite already runs, all pointers valid."""
import numpy as np
import pytest
import torch

from coevonet_amd import lib as L
from coevonet_amd.rollout import DeviceRollout
from oracle import ref_port as rp
from tests import fc_edge_nets as E
from tests.test_kernels_gpu import to_slab
from tests.test_rollout_reuse_gpu import Setup

pytestmark = pytest.mark.gpu
DEV = "cuda"
FOREIGN = 0x4000        # a bit no COEVO_ST_* uses: the status word is OR-ed into, so it must survive every launch
SENT_A, SENT_L = -7, np.float32(777.0)
INF, NAN = np.float32(np.inf), np.float32(np.nan)
# rows of task i in a table whose instantiation is R: ROWS[R][i % len]; the first one fills the instantiation
ROWS = {1: [1], 2: [2, 1], 5: [5, 3, 1, 4], 8: [8, 6, 1, 7, 5], 16: [16, 9, 12, 5, 13, 1], 32: [32, 17, 9, 29, 1, 24]}
HEALTHY_CAST = ["plain", "tie2", "tie5", "subnormal_fc2", "signed_zeros", "tie2_04", "zero_variance", "subnormal_fc1",
                "tie2_23", "plain"]


def rng(*key):
    return np.random.Generator(np.random.PCG64([int(k) for k in key]))


def task(g, name, D, n, seed=0):
    """(class, net, observations [n][D]); subnormal classes get rows on which flushing would show (checked on the CPU first)"""
    w = E.make(name, D, seed)
    obs = E.observations(g, n, D, name, w)
    if name in E.SUBNORMAL:
        wf = E.flushed(w, D, name)
        assert all(E.has_teeth(w, wf, D, o) for o in obs), f"{name}: the rows cannot tell a flushing unit"
    return name, w, obs


def cast(g, names, D, R):
    return [task(g, name, D, ROWS[R][i % len(ROWS[R])], seed=i) for i, name in enumerate(names)]


# =============================================================================== observations given
def slab_with_twins(flat, D, recs, marked):
    """the nets packed at the slab's start; behind them, at a multiple of TASK_TWIN_UNIT and inside the same allocation, one
    twin slot per marked task (table, task index, net index, how, further bits), and the task's TILED word naming it:
      "twin"   the slot is the net's twin (coevo_fc_w2_tile_major), and the canonical fc2.weight of the net - which only this
               task reads - is overwritten with NaN afterwards: the oracle's words come out only if the twin is what was read
      "decoy"  the slot is NaN throughout and the net stays whole: the oracle's words come out only if the bit is ignored"""
    if not marked:
        return to_slab(flat, D)
    n, stride, o_w2 = len(flat), L.fc_slab_stride(D), D * 512 + 3 * 512
    assert len(marked) <= 16
    twin0 = -(-n * stride // L.TASK_TWIN_UNIT) * L.TASK_TWIN_UNIT
    slab = torch.zeros(twin0 + len(marked) * L.W2_FLOATS, dtype=torch.float32, device=DEV)
    L.call("coevo_fc_pack", L._p(torch.from_numpy(flat).to(DEV)), L._p(slab), n, D)
    for slot, (tname, t, net, how, bits) in enumerate(marked):
        off = twin0 + slot * L.W2_FLOATS
        if how == "twin":
            L.call("coevo_fc_w2_tile_major", slab.data_ptr() + 4 * net * stride, slab.data_ptr() + 4 * off, 1, D)
        else:
            assert how == "decoy"
            slab[off:off + L.W2_FLOATS] = float("nan")
        recs[tname]["reserved"][t] = L.task_tiled_flags(off) | bits
        assert ((int(recs[tname]["reserved"][t]) >> L.TASK_TWIN_SHIFT) * L.TASK_TWIN_UNIT + L.W2_FLOATS) <= slab.numel()
    for tname, t, net, how, bits in marked:   # (after every twin is built)
        if how == "twin":
            slab[net * stride + o_w2:net * stride + o_w2 + L.W2_FLOATS] = float("nan")
    return slab


# entry -> marks of launch(): the merged launch with its 16-row table through twins, and with COEVO_TASK_RESIDENT on top
MARKS = {"merged_tiled": {"heavy": ("twin", 0)}, "merged_tiled_res": {"heavy": ("twin", L.TASK_RESIDENT)}}


def launch(entry, D, tables, poison_padding=False, marks=None):
    """one launch of `entry`; tables = {"tasks": (R, [task ...])} for coevo_fc_forward_argmax, {"heavy": (16, ...), "light":
    (R, ...)} for coevo_fc_forward_merged.  Every task is followed by R - n_rows + 1 rows that belong to no task (what an
    instantiation that ignored n_rows would read and write); actions / logits start as sentinels; the status word starts
    at FOREIGN.  poison_padding: NaN / inf in the observation columns >= D of every row and in the rows of no task.
    marks = {table: ("twin" | "decoy", further COEVO_TASK_* bits)}: every task of that table carries COEVO_TASK_TILED
    (slab_with_twins); MARKS[entry] when None.
    -> (actions, logits, status word, [(table, task index, first row)])"""
    marks = MARKS.get(entry, {}) if marks is None else marks
    nets, recs, where, r0, marked = [], {}, [], 0, []
    for tname, (R, tasks) in tables.items():
        rec = np.zeros(len(tasks), dtype=L.TASK_DTYPE)
        for t, (name, w, obs) in enumerate(tasks):
            assert 1 <= len(obs) <= R and obs.shape[1] == D
            rec[t] = (len(nets) * L.fc_slab_stride(D), r0, len(obs), D, 0)
            if tname in marks:
                marked.append((tname, t, len(nets)) + tuple(marks[tname]))
            nets.append(w)
            where.append((tname, t, r0))
            r0 += R + 1
        recs[tname] = rec
    n_rows = r0 + 32
    obs_all = np.zeros((n_rows, L.OBS_STRIDE), dtype=np.float32)
    if poison_padding:
        obs_all[:] = np.where((np.arange(n_rows)[:, None] + np.arange(L.OBS_STRIDE)[None, :]) % 2 == 0, NAN, INF)
    is_task_row = np.zeros(n_rows, dtype=bool)
    for (tname, t, first), (_, _, obs) in zip(where, [x for _, ts in tables.values() for x in ts]):
        obs_all[first:first + len(obs), :D] = obs
        if not poison_padding:
            obs_all[first:first + len(obs), D:] = 0.0
        is_task_row[first:first + len(obs)] = True
    slab = slab_with_twins(np.stack(nets), D, recs, marked)
    d_obs = torch.from_numpy(obs_all).to(DEV)
    actions = torch.full((n_rows,), SENT_A, dtype=torch.int32, device=DEV)
    logits = torch.full((n_rows, L.LOGIT_STRIDE), float(SENT_L), dtype=torch.float32, device=DEV)
    status = torch.full((1,), FOREIGN, dtype=torch.int32, device=DEV)
    dev = {k: L.tasks_to_device(v) for k, v in recs.items()}   # (kept alive across the launch)
    if entry == "argmax":
        R = tables["tasks"][0]
        L.call("coevo_fc_forward_argmax", L._p(slab), L._p(dev["tasks"]), len(recs["tasks"]), R, L._p(d_obs), L._p(actions),
               L._p(logits), L._p(status))
    else:
        L.call("coevo_fc_forward_merged", L._p(slab), L._p(dev["heavy"]), len(recs["heavy"]), tables["heavy"][0],
               L._p(dev["light"]), len(recs["light"]), tables["light"][0], L._p(d_obs), L._p(actions), L._p(logits),
               L._p(status))
    torch.cuda.synchronize()
    got_a, got_l = actions.cpu().numpy(), logits.cpu().numpy()
    # rows of no task: nothing may be written there, whatever else the launch is about
    assert (got_a[~is_task_row] == SENT_A).all(), f"{entry}: action rows of no task were written"
    assert (got_l[~is_task_row] == SENT_L).all(), f"{entry}: logits rows of no task were written"
    return got_a, got_l, int(status.item()), where


def check(entry, D, tables, poison_padding=False, marks=None):
    """launch, then every row of every task against the oracle ON THE NET AS GIVEN (launch() poisons only the slab): logits
    bits (NaN by class), action (-1 -> 0, as the kernels and oracle_play_game have it), and the exact status word.
    -> the oracle's status OR (without FOREIGN)"""
    got_a, got_l, status, where = launch(entry, D, tables, poison_padding, marks)
    want_status, flat_tasks = 0, [x for _, ts in tables.values() for x in ts]
    for (tname, t, first), (name, w, obs) in zip(where, flat_tasks):
        for r, o in enumerate(obs):
            a, lg, st = rp.fc_forward(w, D, o)
            want_status |= st
            what = f"{entry} D={D} {tname}[{t}] ({name}, {len(obs)} rows) row {r}"
            assert E.same_bits_up_to_nan(got_l[first + r, :5], lg), f"{what}: logits {got_l[first + r, :5]} vs oracle {lg}"
            assert got_a[first + r] == max(a, 0), f"{what}: action {got_a[first + r]} vs oracle {a} (logits {lg})"
    assert status == FOREIGN | want_status, \
        f"{entry} D={D}: status word {status:#x}, the oracle's rows OR to {want_status:#x} on top of {FOREIGN:#x}"
    return want_status


OBS_CELLS = [("argmax", 1), ("argmax", 2), ("argmax", 5), ("argmax", 8), ("argmax", 32),
             ("merged", 1), ("merged", 2), ("merged", 5), ("merged", 8), ("merged_tiled", 5), ("merged_tiled", 8),
             ("merged_tiled_res", 5)]


@pytest.mark.parametrize("D", [10, 8])
@pytest.mark.parametrize("entry,R", OBS_CELLS)
def test_healthy_classes_bit_exact(entry, R, D):
    """ties (two- and five-way), signed zeros, variance 0 and both subnormal nets beside ordinary nets in one launch: status
    exactly 0, logits bit-equal, the FIRST maximum taken.  merged: the whole cast in the 16-row table and in the R table;
    merged_tiled: the 16-row table through its nets' twins (MARKS), the subnormal fc2 net with its teeth among them"""
    g = rng(1, R, D)
    if entry == "argmax":
        tables = {"tasks": (R, cast(g, HEALTHY_CAST, D, R))}
    else:
        tables = {"heavy": (16, cast(g, HEALTHY_CAST, D, 16)), "light": (R, cast(g, HEALTHY_CAST, D, R))}
    assert check(entry, D, tables) == 0


FAULT_CELLS = [("argmax", 1, "tasks"), ("argmax", 2, "tasks"), ("argmax", 5, "tasks"), ("argmax", 8, "tasks"),
               ("argmax", 32, "tasks"), ("merged", 5, "heavy16"), ("merged", 5, "heavy_few"), ("merged", 1, "light"),
               ("merged", 2, "light"), ("merged", 5, "light"), ("merged", 8, "light"),
               ("merged_tiled", 5, "heavy16"), ("merged_tiled", 5, "heavy_few")]
FAULTS = sorted(E.FAULTY) + ["obs_inf", "obs_nan"]


def faulted_task(g, fault, D, n, seed):
    if fault in E.FAULTY:
        return task(g, fault, D, n, seed)
    name, w, obs = task(g, "plain", D, n, seed)
    for r in range(n):   # every row of the task, another input column each
        obs[r, (r + 3) % D] = INF if fault == "obs_inf" else NAN
    return fault, w, obs


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("entry,R,where", FAULT_CELLS)
def test_one_faulted_task_among_healthy_ones(entry, R, where, fault):
    """one launch per fault class and body: the status word is exactly the OR of the oracle's words, every healthy task keeps
    the oracle's bits (nothing leaks between workgroups), the faulted rows have the oracle's action and logits up to NaN"""
    for D in (10, 8):
        g = rng(2, R, D, FAULTS.index(fault))
        around = ["plain", "tie2", None, "subnormal_fc2", "plain"]

        def table(RR, n_fault):
            return [faulted_task(g, fault, D, n_fault, i) if name is None else
                    task(g, name, D, ROWS[RR][i % len(ROWS[RR])], i) for i, name in enumerate(around)]

        if entry == "argmax":
            tables = {"tasks": (R, table(R, R))}
        elif where == "light":
            tables = {"heavy": (16, cast(g, ["plain", "tie2_04", "subnormal_fc1"], D, 16)), "light": (R, table(R, R))}
        else:
            tables = {"heavy": (16, table(16, 12 if where == "heavy16" else 5)), "light": (R, cast(g, ["tie5", "plain"], D, R))}
        want = E.BAD_OBS_STATUS if fault.startswith("obs_") else E.PROPERTY[fault][0]
        assert check(entry, D, tables) == want != 0


PER_ROW = {2: [0, 1], 5: [0, 2, 4], 8: [0, 3, 7], 16: [0, 5, 7, 8, 10, 15], 32: [0, 3, 5, 10, 15, 16, 21, 26, 28, 31]}


@pytest.mark.parametrize("bad", [INF, NAN], ids=["inf", "nan"])
@pytest.mark.parametrize("entry,R,where", [c for c in FAULT_CELLS if not (c[1] == 1 and c[2] != "heavy16") and c[2] != "heavy_few"])
def test_non_finite_observation_in_one_row(entry, R, where, bad):
    """full tasks that share one net, each with ONE poisoned row (first, middle, last; a row of every 4- and 8-row group of
    the tiles): the other rows of the task keep the oracle's bits, the poisoned one raises all five bits"""
    for D in (10, 8):
        RR = 16 if where == "heavy16" else R
        g = rng(3, RR, D)
        tasks = []
        for p in PER_ROW[RR]:
            name, w, obs = task(g, "plain", D, RR, seed=7)
            obs[p, p % D] = bad
            tasks.append((f"row {p} poisoned", w, obs))
        tasks.insert(1, task(g, "tie2", D, RR, seed=8))
        if entry == "argmax":
            tables = {"tasks": (R, tasks)}
        elif where == "light":
            tables = {"heavy": (16, cast(g, ["plain"], D, 16)), "light": (R, tasks)}
        else:
            tables = {"heavy": (16, tasks), "light": (R, cast(g, ["plain"], D, R))}
        assert check(entry, D, tables) == E.BAD_OBS_STATUS


@pytest.mark.parametrize("D", [8, 10])
@pytest.mark.parametrize("entry,R,n,where", [("argmax", 2, 1, "tasks"), ("argmax", 5, 3, "tasks"), ("argmax", 8, 6, "tasks"),
                                             ("argmax", 32, 17, "tasks"), ("merged", 5, 9, "heavy"), ("merged", 2, 1, "light"),
                                             ("merged", 5, 3, "light"), ("merged", 8, 6, "light"),
                                             ("merged_tiled", 5, 9, "heavy")])
def test_padding_stays_silent(entry, R, n, where, D):
    """tasks with fewer rows than the instantiation (1 of 2, 3 of 5, 6 of 8, 9 of 16, 17 of 32), NaN / inf in the observation
    columns >= D of every row (an 8-wide net: columns 8 .. 11) and in the rows of no task right after each task's last row;
    the output rows of no task keep their sentinels (launch() asserts it): status exactly 0, outputs as the oracle's"""
    g = rng(4, R, n, D)
    names = ["plain", "tie2", "subnormal_fc2", "plain", "zero_variance"]
    few = [task(g, name, D, n, i) for i, name in enumerate(names)]
    if entry == "argmax":
        tables = {"tasks": (R, few)}
    elif where == "light":
        tables = {"heavy": (16, [task(g, name, D, 9 + i, i) for i, name in enumerate(names[:3])]), "light": (R, few)}
    else:
        tables = {"heavy": (16, few), "light": (R, [task(g, name, D, 3, i) for i, name in enumerate(names[:3])])}
    assert check(entry, D, tables, poison_padding=True) == 0


# ---- include/coevo.h on COEVO_TASK_TILED: "Every other launch and every per-individual task ignores it."  The bit names an
#      in-allocation twin region that is NaN throughout ("decoy"): a body that followed it would raise BAD_FC2 on healthy nets
@pytest.mark.parametrize("bits", [0, L.TASK_RESIDENT], ids=["tiled", "resident_tiled"])
@pytest.mark.parametrize("R", [1, 2, 5, 8])
def test_tiled_bit_is_ignored_by_per_individual_tasks(R, bits):
    """the light table of coevo_fc_forward_merged (fc_policy_body_c<R, MODE_OBS, FC2_MFMA>), every task flagged, the healthy
    cast: status 0 and the oracle's bits; the 16-row table beside it unflagged"""
    for D in (10, 8):
        g = rng(5, R, D)
        tables = {"heavy": (16, cast(g, ["plain", "tie2_04"], D, 16)), "light": (R, cast(g, HEALTHY_CAST, D, R))}
        assert check("merged", D, tables, marks={"light": ("decoy", bits)}) == 0


@pytest.mark.parametrize("R", [1, 2, 5, 8, 32])
def test_tiled_bit_is_ignored_by_the_argmax_launch(R):
    """coevo_fc_forward_argmax, every task flagged: fc_policy_body<R> and, at R = 32, fc_policy_mfma_body (shared-opponent
    tasks of more than 16 rows have no twin path)"""
    for D in (10, 8):
        assert check("argmax", D, {"tasks": (R, cast(rng(6, R, D), HEALTHY_CAST, D, R))}, marks={"tasks": ("decoy", 0)}) == 0


# =============================================================================== state driven: whole games
FORMS = ["persistent1", "persistent2", "small", "lean16", "lean16_resident", "lean16_tiled", "tile32", "paired", "two_launch",
         "plain"]
# forms whose tasks carry COEVO_TASK_TILED although no body of theirs may follow it -> the form they are otherwise
# (every heavy and every light task flagged; lean16: the per-individual tasks only, without and with COEVO_TASK_RESIDENT)
FLAGGED = {"persistent1_flagged": "persistent1", "small_flagged": "small", "tile32_flagged": "tile32",
           "paired_flagged": "paired", "two_launch_flagged": "two_launch", "plain_flagged": "plain",
           "lean16_light_flagged": "lean16", "lean16_light_resident_flagged": "lean16"}
SHAPES = {"persistent1": (20, 4, 8, 1, True), "persistent2": (20, 4, 8, 2, True), "small": (20, 4, 8, 1, False),
          "lean16": (20, 4, 16, 2, False), "lean16_resident": (20, 4, 16, 2, False), "lean16_tiled": (20, 4, 16, 2, False),
          "tile32": (40, 4, 32, 2, False), "paired": (523, 1, 32, 1, False), "two_launch": (40, 4, 32, 1, False),
          "plain": (20, 4, 16, 1, False)}
O_W2 = {D: D * 512 + 3 * 512 for D in (8, 10)}   # fc2.weight's first slab position
_SETUPS = {}


def twin_room(s, n_twins, merged, persistent):
    """the Setup's slab reallocated with room for n_twins twins behind the nets, at a multiple of TASK_TWIN_UNIT and inside
    the same allocation, and its DeviceRollout rebuilt on it (as two_launch rebuilds it) -> float offset of the first twin"""
    twin0 = -(-s.slab.numel() // L.TASK_TWIN_UNIT) * L.TASK_TWIN_UNIT
    s.slab = torch.zeros(twin0 + n_twins * L.W2_FLOATS, dtype=torch.float32, device=DEV)
    s.ro = DeviceRollout(s.plan, s.slab, merged=merged)
    if not persistent:
        s.ro.sync_words, s.ro.desc.sync_words = None, None
    return twin0


def set_task_words(plan, table, words):
    """`reserved` of every task of plan.heavy / plan.light, in the host table and - in place, the rollout points to it - in
    the device table: exactly what GAEngine._enable_hof_tiled does"""
    tasks = getattr(plan, table + "_np").copy()
    tasks["reserved"] = words
    setattr(plan, table + "_np", tasks)
    getattr(plan, table).copy_(L.tasks_to_device(tasks))


def assert_task_words(s, table, bits):
    """the device table is the host table, every task of it carries `bits`, every twin it names lies inside the slab"""
    p = s.plan
    tnp = getattr(p, table + "_np")
    assert torch.equal(getattr(p, table).cpu(), L.tasks_to_device(tnp).cpu())
    words = tnp["reserved"].astype(np.int64)
    assert len(words) and ((words & (L.TASK_TILED | L.TASK_RESIDENT)) == bits).all()
    assert ((words >> L.TASK_TWIN_SHIFT) * L.TASK_TWIN_UNIT + L.W2_FLOATS <= s.slab.numel()).all()


def setup(form):
    """one Setup (tests/test_rollout_reuse_gpu.py) per form, kept for the module; the kernel form is asserted on every use"""
    s = _SETUPS.get(form)
    base = FLAGGED.get(form, form)
    if s is None:
        npop, nh, heavy_rows, K, persistent = SHAPES[base]
        s = Setup(npop, nh, heavy_rows, K, persistent=persistent)
        if base == "two_launch" and form == base:
            s.ro = DeviceRollout(s.plan, s.slab, merged=False)
        if form == "lean16_resident":   # the flag in the task table the rollout already points to (same device buffer)
            s.plan.light_np["reserved"][::2] = L.TASK_RESIDENT
            s.plan.light.copy_(L.tasks_to_device(s.plan.light_np))
        if form == "lean16_tiled":
            # a twin slot per shared opponent - in Setup these nets (agent_1: D = 10, adversary: D = 8) play heavy tasks only
            # and the heavy tasks play only them - and every heavy task pointed at its net's slot
            n10 = npop + nh
            twin0 = twin_room(s, 2 * nh, merged=True, persistent=False)
            s.twin_nets = [(npop * s.s10, 10, nh, twin0), (n10 * s.s10, 8, nh, twin0 + nh * L.W2_FLOATS)]
            slot = {first + k * L.fc_slab_stride(D): t0 + k * L.W2_FLOATS for first, D, n, t0 in s.twin_nets for k in range(n)}
            assert sorted(set(s.plan.heavy_np["net_off"].tolist())) == sorted(slot)
            assert not set(s.plan.light_np["net_off"].tolist()) & set(slot)
            set_task_words(s.plan, "heavy", [L.task_tiled_flags(slot[off]) for off in s.plan.heavy_np["net_off"].tolist()])
        if form in FLAGGED:   # one twin slot, NaN throughout and never written again, named by every flagged task
            twin0 = twin_room(s, 1, merged=base != "two_launch", persistent=persistent)
            s.slab[twin0:] = float("nan")
            word = L.task_tiled_flags(twin0) | (L.TASK_RESIDENT if "resident" in form else 0)
            for table in (("light",) if base == "lean16" else ("heavy", "light")):
                set_task_words(s.plan, table, word)
        s.load_nets(seed=77)
        s.base10, s.base8 = s.nets10, s.nets8
        s.n_cycles = 3 if base == "paired" else 5
        _SETUPS[form] = s
    lib, p, ro = L.load(), s.plan, s.ro
    if form == "lean16_tiled":
        assert_task_words(s, "heavy", L.TASK_TILED)
        assert not p.light_np["reserved"].any()
    elif form in FLAGGED:
        assert torch.isnan(s.slab[-L.W2_FLOATS:]).all()
        assert_task_words(s, "light", L.TASK_TILED | (L.TASK_RESIDENT if "resident" in form else 0))
        if base == "lean16":
            assert not p.heavy_np["reserved"].any()
        else:
            assert_task_words(s, "heavy", L.TASK_TILED)
    form = "lean16" if form == "lean16_tiled" else base
    if form.startswith("persistent"):
        s.assert_form("persistent")
        assert p.n_cohorts == int(form[-1]) and ro.desc.merged == 1
    elif form in ("small", "lean16", "tile32"):
        s.assert_form(form)
        assert ro.desc.merged == 1 and p.n_cohorts == (1 if form == "small" else 2)
    elif form == "lean16_resident":
        s.assert_form("lean16")
        flags = L.tasks_to_device(p.light_np).cpu()   # what the device table holds
        assert torch.equal(p.light.cpu(), flags) and (p.light_np["reserved"][::2] == L.TASK_RESIDENT).all() \
            and not p.light_np["reserved"][1::2].any()
    elif form == "paired":
        assert ro.sync_words is None and ro.desc.merged == 1 and len(p.light_np) % 2 == 1 and p.light_max == 1
        assert lib.coevo_mpe_cycle_kernel_form(*s.shape(0)) == 1   # COEVO_CYCLE_FORM_TILE32_PAIRED
    elif form == "two_launch":
        assert ro.sync_words is None and ro.desc.merged == 0 and ro.desc.state_alt and p.heavy_max > 8 and p.light_max == 4
    else:
        assert form == "plain" and p.heavy_max > 8 and p.light_max == 4
    return s


def install(s, edits10=None, edits8=None, flush=False):
    """the Setup's plain nets with `edits` = {net index: class} applied (flush: every subnormal class as a flushing unit would
    see it), packed into its slab as Setup.load_nets packs fresh ones; a tag per net names its content for the game cache"""
    nets = {10: s.base10.copy(), 8: s.base8.copy()}
    tags = {10: [("plain", s.npop, s.nh, i) for i in range(len(s.base10))], 8: [("plain", s.npop, s.nh, i) for i in range(len(s.base8))]}
    for D, edits in ((10, edits10 or {}), (8, edits8 or {})):
        for i, name in edits.items():
            w = E.make(name, D, i)
            flushed = flush and name in E.SUBNORMAL
            nets[D][i] = E.flushed(w, D, name) if flushed else w
            tags[D][i] = (name, D, i, flushed)
    s.nets10, s.nets8, s.tags10, s.tags8 = nets[10], nets[8], tags[10], tags[8]
    if s.slab is not None:
        for flat, D, first in ((s.nets10, 10, 0), (s.nets8, 8, len(s.nets10) * s.s10)):
            src = torch.from_numpy(np.ascontiguousarray(flat)).to(DEV)
            L.call("coevo_fc_pack", L._p(src), s.slab.data_ptr() + 4 * first, len(flat), D)
        # lean16_tiled: the shared opponents' twins rebuilt from the nets just packed, then the canonical fc2.weight of those
        # nets - which only twin-reading tasks play - NaN: the oracle's games come out only if the twins are what is read
        for first, D, n, twin0 in getattr(s, "twin_nets", ()):
            L.call("coevo_fc_w2_tile_major", s.slab.data_ptr() + 4 * first, s.slab.data_ptr() + 4 * twin0, n, D)
            nets_view = s.slab[first:first + n * L.fc_slab_stride(D)].view(n, L.fc_slab_stride(D))
            nets_view[:, O_W2[D]:O_W2[D] + L.W2_FLOATS] = float("nan")


def seats(s, form):
    """net indices the scenarios edit: per-individual seats (for the paired form the first and the second net of one
    workgroup, and the lone net of the last one), the shared agent_1 opponents, the shared adversaries"""
    ind = [4, 5, s.npop - 1, 1, 8] if form == "paired" else [1, 6, s.npop - 1, 3, 12]
    return ind, [s.npop + k for k in range(s.nh)], list(range(s.nh))


def limits_of(s, ragged):
    """agent-step limits that end inside the last cycle: 3 n - 2 everywhere, or 3 n, 3 n - 1, 3 n - 2 game by game"""
    n = s.n_cycles
    return np.array([3 * n - (g % 3 if ragged else 2) for g in range(s.plan.n_games)])


_GAMES = {}   # (the three nets' tags, reset ordinal, limit, cycles) -> play_game_status: forms with the same games share them


def oracle_games(s, first, limits, n_cycles, poke=None, choose=None, affected=None):
    """every game from the oracle -> (rewards [n_games][3], OR of the status words, [last cycle's actions by slot]).
    poke {game: f(MpeState)}: the state edited after the reset; choose(game, slot, logits, first maximum) -> action for the
    games `affected` names: those are replayed step by step (rp.play_game_steps), the others are oracle_play_game's"""
    stream, rewards, status, acts = rp.Stream(), np.zeros((len(s.games), 3)), 0, []
    for g, (adv, a0, a1) in enumerate(s.games):
        nets = (s.nets10[a0], s.nets10[a1], s.nets8[adv - s.npop - s.nh])
        if (poke and g in poke) or (choose and affected(g)):
            r = rp.play_game_steps(stream, *nets, int(limits[g]), n_cycles, ordinal=first + g, poke=(poke or {}).get(g),
                                   choose=choose and (lambda slot, lg, a, g=g: choose(g, slot, lg, a)))
        else:
            key = (s.tags10[a0], s.tags10[a1], s.tags8[adv - s.npop - s.nh], first + g, int(limits[g]), n_cycles)
            r = _GAMES.get(key)
            if r is None:
                r = _GAMES[key] = rp.play_game_status(stream, *nets, int(limits[g]), n_cycles, ordinal=first + g)
        rewards[g], status = r["rewards"], status | r["status"]
        acts.append(r["actions"][3 * (n_cycles - 1):])
    return rewards, status, acts


def run(s, form, first, limits, poke_game=None):
    """one rollout of every game on the Setup's DeviceRollout -> (rewards, status word, last action words [n_games][3]).
    poke_game: a game whose adversary's x becomes inf after the reset, or {game: [COEVO_MPE_STATE_DOUBLES] state column}"""
    ro, p, n = s.ro, s.plan, s.n_cycles
    ro.status.zero_()
    ro.set_limits(limits)
    ro.reset(0, p.n_games, first)
    if isinstance(poke_game, dict):
        games = sorted(poke_game)
        cols = np.stack([np.asarray(poke_game[g], dtype=np.float64) for g in games], axis=1)
        assert cols.shape == (L.MPE_STATE_DOUBLES, len(games))
        ro.state.index_copy_(1, torch.tensor(games, dtype=torch.int64, device=DEV), torch.from_numpy(cols).to(DEV))
    elif poke_game is not None:
        ro.state[0, poke_game] = float("inf")   # x of the adversary of that game: a buffer the test owns
    if form == "plain":
        for c in range(n):
            for tasks, tnp, mx in ((p.heavy, p.heavy_np, p.heavy_max), (p.light, p.light_np, p.light_max)):
                L.call("coevo_mpe_policy_cycle", L._p(s.slab), L._p(tasks), len(tnp), mx, L._p(ro.state), p.n_games,
                       L._p(p.row_game), L._p(p.row_slot), L._p(ro.actions), L._p(ro.status))
            L.call("coevo_mpe_step", L._p(ro.state), p.n_games, L._p(p.game_rows), L._p(ro.actions), c, L._p(ro.limits),
                   ro.pos_first)
        L.call("coevo_mpe_rewards", L._p(ro.state), p.n_games, L._p(ro.rewards))
        torch.cuda.synchronize()
        last = ro.actions.cpu().numpy()[p.game_rows_np]
    else:
        ro.run(n)
        torch.cuda.synchronize()
        last = ro.actions_by_game[(n - 1) & 1].cpu().numpy()
    return ro.rewards.cpu().numpy(), int(ro.status.item()), last


def assert_games(got, want, what, poisoned=()):
    for g in range(len(want)):
        if g in poisoned:
            ok = E.same_bits_up_to_nan(got[g], want[g])
        else:
            ok = np.array_equal(got[g].view(np.uint64), want[g].view(np.uint64))
        assert ok, f"{what}: game {g} rewards {got[g]} vs oracle {want[g]}"


def assert_last_actions(last, acts, what):
    """the action words of the last cycle, for the seats that acted inside their game's step limit"""
    for g, a in enumerate(acts):
        assert len(a) >= 1 and list(last[g][:len(a)]) == a, f"{what}: game {g} last actions {last[g]} vs oracle {a}"


@pytest.mark.parametrize("form", FORMS)
def test_games_of_tie_nets(form):
    """tie nets as individuals, as a shared agent_1 opponent and as the shared adversary (D = 8), the tied pair at other
    indices per net: every agent-step of those seats is a tie.  Shown on the CPU first: a seat kind that took the LAST
    maximum would change rewards.  Then: status 0, rewards bit-equal"""
    s = setup(form)
    ind, a1s, advs = seats(s, form)
    install(s, dict(zip(ind + a1s[:2], ["tie2", "tie5", "tie2_04", "tie2_23", "tie2", "tie2_23", "tie5"])),
            dict(zip(advs[:2], ["tie2", "tie5"])))
    first, limits = 11, limits_of(s, ragged=False)
    want, st, _ = oracle_games(s, first, limits, s.n_cycles)
    assert st == 0
    kinds = {"individual": lambda g, slot: slot == 1 and s.games[g][1] in ind,
             "agent_1": lambda g, slot: slot == 2 and s.games[g][2] in a1s[:2],
             "adversary": lambda g, slot: slot == 0 and s.games[g][0] - s.npop - s.nh in advs[:2]}
    for kind, is_tie in kinds.items():
        other, _, _ = oracle_games(s, first, limits, s.n_cycles, affected=lambda g: any(is_tie(g, slot) for slot in range(3)),
                                   choose=lambda g, slot, lg, a: E.last_maximum(lg) if is_tie(g, slot) else a)
        assert (other != want).any(), f"{form}: these games cannot tell the first maximum from the last for the {kind} seats"
    got, status, _ = run(s, form, first, limits)
    assert status == 0, f"{form}: status {status:#x}"
    s.ro.check_status()
    assert_games(got, want, f"{form} tie nets")


@pytest.mark.parametrize("form", FORMS)
def test_games_of_subnormal_nets(form):
    """subnormal fc2 / fc1 nets in per-individual seats and in the shared seats (agent_1: fc2, adversary: fc1, D = 8); on the
    CPU first: with the subnormal weights flushed the rewards differ.  Then: status 0, rewards bit-equal"""
    s = setup(form)
    ind, a1s, advs = seats(s, form)
    edits10 = {ind[0]: "subnormal_fc2", ind[1]: "subnormal_fc1", ind[2]: "subnormal_fc1"}
    sub_a1, sub_adv = a1s[0], advs[-1]   # (opponents of different games, unless there is only one of each)
    edits10[sub_a1], edits8 = "subnormal_fc2", {sub_adv: "subnormal_fc1"}
    first, limits = 23, limits_of(s, ragged=False)
    install(s, edits10, edits8, flush=True)
    other, st, _ = oracle_games(s, first, limits, s.n_cycles)
    install(s, edits10, edits8)
    want, st2, _ = oracle_games(s, first, limits, s.n_cycles)
    assert st == st2 == 0
    kinds = {"individual": lambda a0, a1, adv: a0 in ind[:3] and a1 != sub_a1 and adv != sub_adv,
             "agent_1": lambda a0, a1, adv: a0 not in ind[:3] and a1 == sub_a1 and adv != sub_adv,
             "adversary": lambda a0, a1, adv: a0 not in ind[:3] and a1 != sub_a1 and adv == sub_adv}
    for kind, only in kinds.items():   # games with a subnormal net in that kind of seat and nowhere else (one opponent: any)
        mine = [g for g, (adv, a0, a1) in enumerate(s.games) if s.nh == 1 or only(a0, a1, adv - s.npop - s.nh)]
        assert mine and (other[mine] != want[mine]).any(), f"{form}: flushing the {kind} seats' subnormal weights would not show"
    got, status, _ = run(s, form, first, limits)
    assert status == 0, f"{form}: status {status:#x}"
    assert_games(got, want, f"{form} subnormal nets")


def fault_cases():
    out = []
    for form in FORMS:
        for c, cls in enumerate(["all_nan_logits", "nan_in_fc2", "nan_in_fc1", "one_pos_inf"]):
            for seat in (["first_of_pair", "second_of_pair", "lone_last"] if form == "paired" else ["individual"]):
                out.append((form, cls, seat))
            out.append((form, cls, "agent_1" if c % 2 == 0 else "adversary"))   # a shared opponent: the heavy body
    return out


@pytest.mark.parametrize("form,cls,seat", fault_cases())
def test_games_with_one_faulted_net(form, cls, seat):
    """one faulted net per run: check_status() raises naming exactly the oracle's conditions, the status word is the OR of the
    oracle's per-step words (no COEVO_ST_SYNC_TIMEOUT: a faulted row still posts its action word), the rewards of ALL games
    and the last action words are the oracle's - the faulted seat plays 0 or its surviving maximum, physics stays finite"""
    s = setup(form)
    ind, a1s, advs = seats(s, form)
    if seat == "adversary":
        install(s, None, {advs[-1]: cls})
    else:
        i = {"individual": ind[1], "first_of_pair": ind[0], "second_of_pair": ind[1], "lone_last": ind[2], "agent_1": a1s[-1]}[seat]
        assert seat not in ("first_of_pair", "second_of_pair", "lone_last") or \
            (i % 2, i == s.npop - 1) == {"first_of_pair": (0, False), "second_of_pair": (1, False), "lone_last": (0, True)}[seat]
        install(s, {i: cls})
    first, limits = 31, limits_of(s, ragged=True)
    want, want_status, acts = oracle_games(s, first, limits, s.n_cycles)
    assert want_status == E.PROPERTY[cls][0] != 0 and np.isfinite(want).all()
    got, status, last = run(s, form, first, limits)
    what = f"{form} {cls} in the {seat} seat"
    assert status == want_status, f"{what}: status word {status:#x}, the oracle's steps OR to {want_status:#x}"
    assert not status & E.SYNC_TIMEOUT
    with pytest.raises(ValueError) as err:
        s.ro.check_status()
    for bit, text in L.ST_NAMES.items():
        assert (text in str(err.value)) == bool(want_status & bit), f"{what}: {err.value}"
    assert_games(got, want, what)
    assert_last_actions(last, acts, what)


@pytest.mark.parametrize("form", FORMS)
def test_games_with_a_non_finite_state(form):
    """x of one game's adversary set to inf after the reset: every seat of that game observes it (all five bits, as the
    oracle's forward has them for those rows); every OTHER game - the ones sharing its tiles and workgroups included - keeps
    the oracle's reward bits; the poisoned game's rewards agree by NaN-ness and otherwise (+-inf, finite) by bits"""
    s = setup(form)
    install(s)
    gp = 7

    def poke(state):
        state.ppos[0][0] = float("inf")

    first, limits = 41, limits_of(s, ragged=True)
    want, want_status, acts = oracle_games(s, first, limits, s.n_cycles, poke={gp: poke})
    assert want_status == E.BAD_OBS_STATUS and not np.isfinite(want[gp]).all() and np.isfinite(np.delete(want, gp, 0)).all()
    got, status, last = run(s, form, first, limits, poke_game=gp)
    assert status == want_status, f"{form}: status word {status:#x}, the oracle's steps OR to {want_status:#x}"
    assert_games(got, want, f"{form} non-finite state", poisoned=(gp,))
    assert_last_actions(last, acts, f"{form} non-finite state")


@pytest.mark.parametrize("form", sorted(FLAGGED))
def test_tiled_bit_is_ignored_outside_the_lean_shared_opponent_body(form):
    """include/coevo.h on COEVO_TASK_TILED: "Every other launch and every per-individual task ignores it."  The games of
    test_games_of_tie_nets (healthy nets; the oracle's games are the unflagged form's) with the bit on every task that must
    not follow it, naming an in-allocation twin region that is NaN throughout: status 0, rewards and last actions the oracle's
    - a body that honoured the bit would read NaN weights and raise BAD_FC2"""
    s, base = setup(form), FLAGGED[form]
    ind, a1s, advs = seats(s, base)
    install(s, dict(zip(ind + a1s[:2], ["tie2", "tie5", "tie2_04", "tie2_23", "tie2", "tie2_23", "tie5"])),
            dict(zip(advs[:2], ["tie2", "tie5"])))
    first, limits = 11, limits_of(s, ragged=False)
    want, st, acts = oracle_games(s, first, limits, s.n_cycles)
    assert st == 0
    got, status, last = run(s, base, first, limits)
    assert status == 0, f"{form}: status {status:#x}"
    s.ro.check_status()
    assert_games(got, want, f"{form} tie nets")
    assert_last_actions(last, acts, f"{form} tie nets")
