"""Fault bits, ties, signed zeros, subnormals, fp16 rounding points and padding rows in BOTH float16 policy-forward bodies -
fc16_policy_kernel (csrc/fc16.hip, coevo_fc16_forward_argmax) and fc16_cycle_kernel (csrc/fc16_rollout.hip, the body every
fp16 engine and trainer plays through) - against the C checker (tests/checker16/fc16_checker.c through tests/fp16_checker.py).

The two bodies are written separately: the cycle kernel's fc2 runs on mfma_f32_4x4x1f32 out of a k-quad LDS image fed by
ping-pong buffers, in two cache-policy instantiations, its LayerNorms go through per-(row, block) partials in LDS, h1q and h2
share storage across passes, and only an `r < nr` term keeps the rows past a task's last row out of the status.  So the nets of
tests/fc16_edge_nets.py go through each of them.  Expected logits, actions and status words are always the checker's; finite
values, infinities and the sign of zero are compared as bits, NaN by NaN-ness, and the status word - started at a foreign bit -
must end as exactly that bit OR the OR of the checker's words, so a missing bit fails like a surplus one.  No tolerance anywhere.

Cells (body, instantiation, row counts) and where each is launched:

  observations given: coevo_fc16_forward_argmax, fc16_policy_kernel, passes of 8 rows; D = 8 and 10 each
    healthy cast          tasks of 1, 5, 8, 9, 17, 32 rows, every healthy class at two row counts
    one faulted task      every faulty class + obs_inf / obs_nan, the faulted task at each of 1, 5, 8, 9, 17, 32 rows
    one poisoned row      8-row tasks (rows 0, 3, 7) and 32-row tasks (rows 0, 7, 8, 15, 16, 23, 24, 31)
    padding               tasks of 3, 6, 9, 17 rows x (plain, tie2, zero_variance, pad_fault, pad_fault_fc1), NaN / inf around
                          every task
  state driven: coevo_mpe16_policy_cycle, fc16_cycle_kernel, through Stepper (tests/test_fp16_rollout_gpu.py); the shape is
  asserted from the task table
    nt                    fc16_fc2_stream<true>  (non-temporal loads): tasks of 8, 8, 5, 5, 3, 3, 2, 2, 1, 1, 1, 1 (D = 10) and
                          8, 5, 3, 2, 1, 1 (D = 8) rows, no flag
    resident              fc16_fc2_stream<false> (plain loads), one pass: the same tasks with COEVO_TASK_RESIDENT
    multipass             fc16_fc2_stream<false>, two to four passes: tasks of 32, 17, 9 (D = 10) and 9, 20 (D = 8) rows
    each with: healthy classes in games, one faulted net per launch, one game with a non-finite state (multipass: the game's
    rows at rows 7 / 8 and 15 / 16 of their tasks)
    pad_fault             tasks of 3, 6 and 9 rows of pad_fault and of pad_fault_fc1 nets beside healthy ones, without and with
                          COEVO_TASK_RESIDENT
  heavy table: coevo_mpe16_rollout through DeviceRollout(precision="float16"), a 12-row task per shared opponent in the heavy
  table (blockIdx.x < n_heavy), the opponents one tie net and one fc2_overflow net

Only numerical status bits are provoked: every launch has the shape of one the suite already runs, all pointers valid."""
import numpy as np
import pytest
import torch

from coevonet_amd import lib as L
from oracle import ref_port as rp
from tests import fc16_edge_nets as E
from tests import fp16_checker as ck
from tests.test_fp16_gpu import pack
from tests.test_fp16_rollout_gpu import POISON_ACT, GaSetup, Stepper, eq_bits, pack16

pytestmark = pytest.mark.gpu
DEV = "cuda"
FOREIGN = 0x4000        # a bit no COEVO_ST_* uses: the status word is OR-ed into, so it must survive every launch
SENT_A, SENT_L = -7, np.float32(777.0)
INF, NAN = E.INF, E.NAN
ROW_COUNTS = (1, 5, 8, 9, 17, 32)   # one partial pass, one full pass, partial passes after one, two and (32) three full ones
PASS = 8                             # F16_R of csrc/fc16_layout.hip.h
HEALTHY_CAST = ["plain", "tie2", "tie2_04", "tie2_23", "tie3", "tie5", "signed_zeros", "zero_variance", "fc2_subnormal",
                "fc1_subnormal", "ln_rounding", "out_rounding", "out_rounding_up", "out_rounding_near"]
FAULTS = sorted(E.FAULTY) + ["obs_inf", "obs_nan"]


def rng(*key):
    return np.random.Generator(np.random.PCG64([int(k) for k in key]))


# =============================================================================== observations given: fc16_policy_kernel
def task(g, name, D, n, seed=0):
    """(class, net, observations [n][D]); subnormal classes get rows on which flushing would show (E.observations rejects the
    others through the checker)"""
    w = E.make(name, D, seed)
    return name, w, E.observations(g, n, D, name, w)


def launch(D, tasks, poison_padding=False):
    """one coevo_fc16_forward_argmax launch.  Every task's rows are followed by the rows that fill its last pass and one more,
    all rows of no task (what a pass that ignored n_rows would read and write); actions / logits start as sentinels, the
    status word at FOREIGN.  poison_padding: NaN / inf in the observation columns >= D of every row and in the rows of no task.
    -> (actions, logits, status word, first row per task)"""
    slab, stride = pack(np.stack([w for _, w, _ in tasks]), D)
    rec, first, r0 = np.zeros(len(tasks), dtype=L.TASK_DTYPE), [], 0
    for t, (_, _, obs) in enumerate(tasks):
        assert 1 <= len(obs) <= L.FC_MAX_ROWS and obs.shape[1] == D
        rec[t] = (t * stride, r0, len(obs), D, 0)
        first.append(r0)
        r0 += -(-len(obs) // PASS) * PASS + 1
    n_rows = r0 + PASS
    obs_all = np.zeros((n_rows, L.OBS_STRIDE), dtype=np.float32)
    if poison_padding:
        obs_all[:] = np.where((np.arange(n_rows)[:, None] + np.arange(L.OBS_STRIDE)[None, :]) % 2 == 0, NAN, INF)
    is_task_row = np.zeros(n_rows, dtype=bool)
    for r, (_, _, obs) in zip(first, tasks):
        obs_all[r:r + len(obs), :D] = obs
        is_task_row[r:r + len(obs)] = True
    d_obs = torch.from_numpy(obs_all).to(DEV)
    actions = torch.full((n_rows,), SENT_A, dtype=torch.int32, device=DEV)
    logits = torch.full((n_rows, L.LOGIT_STRIDE), float(SENT_L), dtype=torch.float32, device=DEV)
    status = torch.full((1,), FOREIGN, dtype=torch.int32, device=DEV)
    d_tasks = L.tasks_to_device(rec, DEV)
    L.call("coevo_fc16_forward_argmax", L._p(slab), L._p(d_tasks), len(rec), int(rec["n_rows"].max()), L._p(d_obs), L._p(actions),
           L._p(logits), L._p(status))
    torch.cuda.synchronize()
    got_a, got_l = actions.cpu().numpy(), logits.cpu().numpy()
    assert (got_a[~is_task_row] == SENT_A).all(), "action rows of no task were written"
    assert (got_l[~is_task_row] == SENT_L).all() and (got_l[:, 5:] == SENT_L).all(), "logit words of no task row were written"
    return got_a, got_l, int(status.item()), first


def check(D, tasks, poison_padding=False):
    """launch, then every row of every task against the checker: logits bits (NaN by class), action (-1 -> 0, as the kernels
    and fc16_play_game have it), and the exact status word -> (the checker's status OR without FOREIGN, per-task OR)"""
    got_a, got_l, status, first = launch(D, tasks, poison_padding)
    want_status, per_task = 0, []
    for t, (r0, (name, w, obs)) in enumerate(zip(first, tasks)):
        mine = 0
        for r, o in enumerate(obs):
            a, lg, st = ck.forward(w, D, o)
            mine |= st
            what = f"D={D} task {t} ({name}, {len(obs)} rows) row {r}"
            assert E.same_bits_up_to_nan(got_l[r0 + r, :5], lg), f"{what}: logits {got_l[r0 + r, :5]} vs checker {lg}"
            assert got_a[r0 + r] == max(a, 0), f"{what}: action {got_a[r0 + r]} vs checker {a} (logits {lg})"
        per_task.append(mine)
        want_status |= mine
    assert status == FOREIGN | want_status, \
        f"D={D}: status word {status:#x}, the checker's rows OR to {want_status:#x} on top of {FOREIGN:#x}"
    return want_status, per_task


@pytest.mark.parametrize("D", [10, 8])
def test_obs_healthy_classes_bit_exact(D):
    """28 tasks: every healthy class twice, at two of the row counts 1, 5, 8, 9, 17, 32 - ties (two-, three- and five-way),
    signed zeros, variance 0, both subnormal nets on rows with teeth, LayerNorm's and the output chain's rounding points -
    status exactly 0, logits bit-equal, the FIRST maximum taken"""
    g = rng(1, D)
    n = len(HEALTHY_CAST)
    tasks = [task(g, HEALTHY_CAST[i % n], D, ROW_COUNTS[(i + 3 * (i // n)) % len(ROW_COUNTS)], seed=i) for i in range(2 * n)]
    assert {len(o) for _, _, o in tasks} == set(ROW_COUNTS)
    assert check(D, tasks)[0] == 0


def faulted_task(g, fault, D, n, seed):
    if fault in E.FAULTY:
        return task(g, fault, D, n, seed)
    name, w, obs = task(g, "plain", D, n, seed)
    for r in range(n):   # every row of the task, another input column each
        obs[r, (r + 3) % D] = INF if fault == "obs_inf" else NAN
    return fault, w, obs


@pytest.mark.parametrize("D", [10, 8])
@pytest.mark.parametrize("fault", FAULTS)
def test_obs_one_faulted_task_among_healthy_ones(fault, D):
    """one launch per fault class and row count of the faulted task: the status word is exactly the OR of the checker's words,
    every healthy task keeps the checker's bits (nothing leaks between workgroups), the faulted rows have the checker's action
    and logits up to NaN"""
    want = E.BAD_OBS_STATUS if fault.startswith("obs_") else E.PROPERTY[fault][0]
    for n_fault in ROW_COUNTS:
        g = rng(2, D, FAULTS.index(fault), n_fault)
        around = ["plain", "tie2", None, "fc2_subnormal", "out_rounding", "plain"]
        tasks = [faulted_task(g, fault, D, n_fault, i) if name is None else
                 task(g, name, D, ROW_COUNTS[(i + n_fault) % len(ROW_COUNTS)], i) for i, name in enumerate(around)]
        status, per_task = check(D, tasks)
        assert status == want != 0 and [bool(s) for s in per_task] == [name is None for name in around]


PER_ROW = {8: [0, 3, 7], 32: [0, 7, 8, 15, 16, 23, 24, 31]}   # the first and the last row of every pass


@pytest.mark.parametrize("bad", [INF, NAN], ids=["inf", "nan"])
@pytest.mark.parametrize("D", [10, 8])
def test_obs_non_finite_observation_in_one_row(D, bad):
    """full tasks of 8 and 32 rows that share one net, each with ONE poisoned row: the other rows of the task - the ones of the
    same pass and of the passes before and after it - keep the checker's bits, the poisoned one raises all five bits"""
    g = rng(3, D)
    tasks = []
    for n, rows in PER_ROW.items():
        for p in rows:
            name, w, obs = task(g, "plain", D, n, seed=7)
            obs[p, p % D] = bad
            tasks.append((f"row {p} of {n} poisoned", w, obs))
    tasks.insert(1, task(g, "tie2", D, 32, seed=8))
    status, per_task = check(D, tasks)
    assert status == E.BAD_OBS_STATUS and per_task.count(0) == 1 and per_task[1] == 0


@pytest.mark.parametrize("D", [8, 10])
def test_obs_padding_stays_silent(D):
    """tasks of 3, 6, 9 and 17 rows (every one ends in a partial pass), cast with plain, a tie, zero_variance and the two
    pad_fault classes; NaN / inf in the observation columns >= D of every row and in the rows of no task right after each
    task's last row.  The preconditions, through the checker, before anything is launched: the pad_fault nets raise bits on
    the zero row (out of LayerNorm(256), out of LayerNorm(512)), and every real row of the launch is clean.
    Then: the output rows of no task keep their sentinels, the status is exactly 0"""
    g = rng(4, D)
    tasks = [task(g, name, D, n, seed=i + 5 * j) for j, n in enumerate((3, 6, 9, 17))
             for i, name in enumerate(("plain", "tie2", "zero_variance", "pad_fault", "pad_fault_fc1"))]
    for name, w, obs in tasks:
        if name in E.PAD_FAULT_ZERO_ROW:
            assert ck.forward(w, D, np.zeros(D, dtype=np.float32))[2] == E.PAD_FAULT_ZERO_ROW[name] != 0
        assert all(ck.forward(w, D, o)[2] == 0 for o in obs)
    assert check(D, tasks, poison_padding=True)[0] == 0


# =============================================================================== state driven: fc16_cycle_kernel
N_CYCLES = 4   # every seat acts four times; limits 3 N_CYCLES: every forward the launches run is one the checker runs
# layout -> (games, rows per D = 10 task, rows per D = 8 task).  Rows are dealt in order: the agent_0 rows of games 0, 1, ...,
# then the agent_1 rows, to the D = 10 tasks; the adversary rows to the D = 8 tasks - so a game's place in its tasks is known
LAYOUTS = {"light": (20, (8, 8, 5, 5, 3, 3, 2, 2, 1, 1, 1, 1), (8, 5, 3, 2, 1, 1)),
           "multi": (29, (32, 17, 9), (9, 20)),
           "pad": (24, (3, 6, 9, 3, 6, 9, 8, 4), (3, 6, 9, 6))}
SHAPES = {"nt": ("light", 0), "resident": ("light", L.TASK_RESIDENT), "multipass": ("multi", 0),
          "pad": ("pad", 0), "pad_resident": ("pad", L.TASK_RESIDENT)}
GAME_CAST = ["tie2", "tie2_04", "tie2_23", "tie5", "tie3", "signed_zeros", "zero_variance", "fc2_subnormal", "fc1_subnormal",
             "out_rounding", "out_rounding_up", "out_rounding_near"]
FIXED_ACTION = {name: E.PROPERTY[name][1] for name in list(E.TIES) + ["out_rounding_up", "out_rounding_near"]}
_GAMES = {}   # (the three nets' tags, ordinal, limit) -> the checker's game: launches with the same games share them


def deal(G, sizes10, sizes8):
    rows10 = [(g, 1) for g in range(G)] + [(g, 2) for g in range(G)]
    rows8 = [(g, 0) for g in range(G)]
    assert sum(sizes10) == len(rows10) and sum(sizes8) == len(rows8)
    out = []
    for rows, sizes in ((rows10, sizes10), (rows8, sizes8)):
        at = 0
        for n in sizes:
            out.append(rows[at:at + n])
            at += n
    return out   # task i is played by net i: the D = 10 nets, then the D = 8 nets


class Games:
    """one Stepper over a layout: names10 / names8 give the class of every net (net i plays task i)"""

    def __init__(self, shape, names10, names8, first, poke=None):
        lay, flag = SHAPES[shape]
        G, sizes10, sizes8 = LAYOUTS[lay]
        assert len(names10) == len(sizes10) and len(names8) == len(sizes8)
        self.G, self.names, self.first = G, list(names10) + list(names8), first
        self.Ds = [10] * len(names10) + [8] * len(names8)
        self.nets = [E.make(name, D, i) for i, (name, D) in enumerate(zip(self.names, self.Ds))]
        self.rows = deal(G, sizes10, sizes8)
        order = rng(9, len(self.rows)).permutation(len(self.rows))   # D = 8 and D = 10 workgroups side by side
        tasks = [(int(i), self.rows[i]) for i in order]
        seat = {gs: i for i, rows in enumerate(self.rows) for gs in rows}
        self.games = [(seat[g, 0], seat[g, 1], seat[g, 2]) for g in range(G)]
        self.limits = [3 * N_CYCLES] * G
        slab, off, Ds = pack16(self.nets[:len(names10)], self.nets[len(names10):])
        assert Ds == self.Ds
        reserved = {t: flag for t, (_, rows) in enumerate(tasks) if len(rows) <= PASS} if flag else None
        self.s = Stepper(slab, off, Ds, tasks, G, self.limits, first, status0=FOREIGN, reserved=reserved)
        # the cell, from the task table the launch reads
        t = self.s.tasks_np
        light = t["n_rows"] <= PASS
        assert (t["reserved"][light] == flag).all() and not t["reserved"][~light].any()
        if lay == "light":
            assert light.all() and set(t["n_rows"].tolist()) == {1, 2, 3, 5, 8}
        elif lay == "multi":
            assert not light.any() and set(t["n_rows"].tolist()) == {9, 17, 20, 32}
        self.poke = poke
        if poke is not None:   # one entry of one game's column of the reset state: x of that game's adversary
            gp, bad = poke
            self.s.state2[0][0, gp] = float(bad)

    def want(self):
        stream, out = rp.Stream(), []
        for g, (adv, a0, a1) in enumerate(self.games):
            if self.poke is not None and g == self.poke[0]:
                bad = self.poke[1]

                def poke(state):
                    state.ppos[0][0] = float(bad)
                out.append(ck.play_game_steps(stream, self.nets[a0], self.nets[a1], self.nets[adv], self.limits[g], 25,
                                              ordinal=self.first + g, poke=poke))
                continue
            key = tuple((self.names[i], self.Ds[i], i) for i in (adv, a0, a1)) + (self.first + g, self.limits[g])
            if key not in _GAMES:
                _GAMES[key] = ck.play_game(stream, self.nets[a0], self.nets[a1], self.nets[adv], self.limits[g], 25,
                                           ordinal=self.first + g)
            out.append(_GAMES[key])
        return out

    def play_and_compare(self, want, what):
        """every action of every game against the checker's list, cycle by cycle; the rewards (a poked game's by NaN-ness and
        otherwise by bits); the canary game and the padding rows untouched; the exact status word"""
        s = self.s
        for c in range(N_CYCLES):
            act = s.cycle(c)
            for g in range(self.G):
                assert list(act[g]) == want[g]["actions"][3 * c:3 * c + 3], (what, "cycle", c, "game", g, self.games[g])
            assert (act[s.n_real] == POISON_ACT).all(), "a padding row was played"
        rew = s.close(N_CYCLES)
        for g in range(self.G):
            assert want[g]["steps"] == s.T[g] == 3 * N_CYCLES
            if self.poke is not None and g == self.poke[0]:
                assert E.same_bits_up_to_nan(rew[g], np.array(want[g]["rewards"])), (what, g, rew[g], want[g]["rewards"])
            else:
                assert eq_bits(rew[g], want[g]["rewards"]), (what, g, rew[g], want[g]["rewards"])
        assert torch.isnan(s.state2[:, :18, s.n_real]).all(), "the canary game's state was written"
        want_st = 0
        for w in want:
            want_st |= w["status"]
        got = int(s.status.item())
        assert got == FOREIGN | want_st, \
            f"{what}: status word {got:#x}, the checker's games OR to {want_st:#x} on top of {FOREIGN:#x}"
        return want_st


@pytest.mark.parametrize("shape,part", [("nt", 0), ("resident", 0)] + [("multipass", part) for part in range(4)])
def test_games_of_healthy_classes(shape, part):
    """ties (two-, three-, five-way), signed zeros, variance 0, subnormal fc1 / fc2 and the three out_rounding nets in the seats
    of whole games: status exactly the foreign bit, every action and reward the checker's.  The tie and out_rounding seats
    show their class' action - the first maximum, the rounding to even - at every step of the checker's own list.
    multipass: three D = 10 and two D = 8 nets per launch, four launches for the cast"""
    n = len(GAME_CAST)
    if shape == "multipass":
        names10 = GAME_CAST[3 * part:3 * part + 3]
        names8 = [GAME_CAST[(3 * part + 5) % n], GAME_CAST[(3 * part + 8) % n]]
    else:
        k = 0 if shape == "nt" else 5   # (the other shape deals the classes to other row counts)
        names10 = [GAME_CAST[(i + k) % n] for i in range(n)]
        names8 = [GAME_CAST[(2 * i + 1 + k) % n] for i in range(6)]
    gm = Games(shape, names10, names8, first=21 + part)
    want = gm.want()
    shown = 0
    for g, seats in enumerate(gm.games):
        assert want[g]["status"] == 0
        for slot, net in enumerate(seats):
            if gm.names[net] in FIXED_ACTION:
                assert set(want[g]["actions"][slot::3]) == {FIXED_ACTION[gm.names[net]]}
                shown += 1
    assert shown >= gm.G
    assert gm.play_and_compare(want, f"{shape} healthy {part}") == 0


@pytest.mark.parametrize("cls", sorted(E.FAULTY))
@pytest.mark.parametrize("shape", ["nt", "resident", "multipass"])
def test_games_with_one_faulted_net(shape, cls):
    """one faulted net per launch (multipass: a net whose task makes two to four passes, so its rows lie in every pass): the
    games without it match the checker exactly and are clean, the games with it play the checker's actions (no action -> 0,
    or the surviving maximum), and the status word is the exact OR"""
    G, sizes10, sizes8 = LAYOUTS[SHAPES[shape][0]]
    n10, n = len(sizes10), len(sizes10) + len(sizes8)
    idx = sorted(E.FAULTY).index(cls)
    bad_net = (idx * (5 if n % 5 else 1) + 1) % n
    names = ["plain"] * n
    names[0 if bad_net else 1] = "tie2"
    names[bad_net] = cls
    gm = Games(shape, names[:n10], names[n10:], first=31 + idx)
    want = gm.want()
    with_it = [bad_net in seats for seats in gm.games]
    assert any(with_it) and (bad_net == 0 or not all(with_it))   # (net 0 of the multipass layout sits in every game)
    for g in range(gm.G):
        assert want[g]["status"] == (E.PROPERTY[cls][0] if with_it[g] else 0), (g, want[g]["status"])
        assert np.isfinite(want[g]["rewards"]).all()
    assert gm.play_and_compare(want, f"{shape} {cls} in net {bad_net}") == E.PROPERTY[cls][0] != 0


STATE_CELLS = [("nt", "inf", 7), ("nt", "nan", 12), ("resident", "inf", 12), ("resident", "nan", 7),
               ("multipass", "inf", 7), ("multipass", "nan", 8), ("multipass", "inf", 15), ("multipass", "nan", 16)]


@pytest.mark.parametrize("shape,bad,gp", STATE_CELLS)
def test_games_with_a_non_finite_state(shape, bad, gp):
    """x of one game's adversary set to inf / NaN after the reset: every seat of that game observes it (all five bits, as the
    checker's game has them); every OTHER game - the ones whose rows share its tasks and passes included - plays the checker's
    actions and keeps its reward bits.  multipass: the game's rows are the last row of a pass (7, 15) or the first of the next
    (8, 16) in the 32-row and the 9- / 20-row task"""
    G, sizes10, sizes8 = LAYOUTS[SHAPES[shape][0]]
    names10 = ["plain"] * len(sizes10)
    names10[1] = "tie2"
    gm = Games(shape, names10, ["plain"] * len(sizes8), first=41, poke=(gp, float(bad)))
    if shape == "multipass":
        at = sorted(rows.index((gp, slot)) for rows in gm.rows for slot in range(3) if (gp, slot) in rows)
        assert len(at) == 3 and sum(i in (7, 8, 15, 16) for i in at) >= 1, at
        assert max(len(rows) for rows in gm.rows if any((gp, slot) in rows for slot in range(3))) == 32
    want = gm.want()
    assert [w["status"] for w in want] == [E.BAD_OBS_STATUS if g == gp else 0 for g in range(gm.G)]
    assert not np.isfinite(want[gp]["rewards"]).all()
    assert gm.play_and_compare(want, f"{shape} state {bad} in game {gp}") == E.BAD_OBS_STATUS


@pytest.mark.parametrize("shape", ["pad", "pad_resident"])
def test_games_of_pad_fault_nets(shape):
    """pad_fault and pad_fault_fc1 nets in tasks of 3, 6 and 9 rows (D = 10 and D = 8) beside healthy tasks: every pass of
    theirs is partial, and the rows that fill it are the all-zero observation on which the net raises BAD_FC2 | BAD_OUT |
    NO_ACTION out of LayerNorm(256), or with BAD_FC1 out of LayerNorm(512) (asserted through the checker, as is that every
    real forward of these games is clean).  The status must then be exactly the foreign bit:
    this is the test that fails if the `r < nr` term goes missing in either LayerNorm.  3- and 6-row tasks: the non-temporal
    instantiation, or with COEVO_TASK_RESIDENT the plain one; the 9-row tasks: plain loads, a full pass and a pass of one row"""
    gm = Games(shape, ["pad_fault"] * 3 + ["pad_fault_fc1"] * 3 + ["plain", "tie2"],
               ["pad_fault_fc1", "pad_fault", "pad_fault_fc1", "plain"], first=51)
    rows_of = {name: sorted(len(rows) for rows, nm in zip(gm.rows, gm.names) if nm == name) for name in set(gm.names)}
    assert rows_of["pad_fault"] == [3, 6, 6, 9] and rows_of["pad_fault_fc1"] == [3, 3, 6, 9, 9]
    assert sorted(gm.s.tasks_np["n_rows"].tolist()) == [3, 3, 3, 4, 6, 6, 6, 6, 8, 9, 9, 9]
    for net, (name, D) in enumerate(zip(gm.names, gm.Ds)):
        if name in E.PAD_FAULT_ZERO_ROW:
            assert ck.forward(gm.nets[net], D, np.zeros(D, dtype=np.float32))[2] == E.PAD_FAULT_ZERO_ROW[name] != 0
    want = gm.want()
    assert all(w["status"] == 0 for w in want), "a real forward of a pad_fault net is faulty: the games cannot tell"
    assert gm.play_and_compare(want, shape) == 0


# =============================================================================== the heavy table of the same kernel
def test_heavy_table_with_a_tie_and_an_overflow_opponent():
    """DeviceRollout(precision="float16") on a GA-shaped plan whose shared opponents have 12 rows each: they are the HEAVY table
    of coevo_mpe16_rollout's launches (blockIdx.x < n_heavy), the individuals the light one.  One agent_1 opponent is a tie
    net, one adversary opponent overflows fc2: rewards of all 36 games bit-equal to the checker's, the status word the exact OR"""
    npop, nh, n_cycles, first = 6, 2, 4, 7
    s = GaSetup(npop, nh, 1, seed=61, heavy_rows=16)
    p = s.plan
    assert len(p.heavy_np) == 3 * nh and (p.heavy_np["n_rows"] == 2 * npop).all() and s.ro.desc.n_heavy == len(p.heavy_np)
    assert len(p.light_np) == 3 * npop and (p.light_np["n_rows"] == nh).all()
    stride = {10: L.fc16_slab_stride(10), 8: L.fc16_slab_stride(8)}
    # HoF slot 0 of agent_1, slot 1 of the adversary
    edits = {s.base[1] + npop: ("tie2", 10), s.base[2] + npop + 1: ("fc2_overflow", 8)}
    for net, (name, D) in edits.items():
        w = E.make(name, D, net)
        s.flats[net] = w
        off = net * stride[10] if D == 10 else len(s.flats10) * stride[10] + (net - len(s.flats10)) * stride[8]
        assert off in p.heavy_np["net_off"].tolist() and off not in p.light_np["net_off"].tolist()
        L.call("coevo_fc16_pack", L._p(torch.from_numpy(w[None].copy()).to(DEV)), s.slab.data_ptr() + 4 * off, 1, D)
    limits = [3 * n_cycles] * len(s.games)
    s.ro.set_limits(limits)
    s.ro.status.fill_(FOREIGN)
    s.ro.use_graph = False
    s.ro.reset(0, len(s.games), first)
    s.ro.run(n_cycles)
    torch.cuda.synchronize()
    got = s.ro.rewards.cpu().numpy()
    want = s.want(first, limits, n_cycles)
    want_st = 0
    tie_net, over_net = sorted(edits)
    for g, (adv, a0, a1) in enumerate(s.games):
        assert want[g]["status"] == (E.PROPERTY["fc2_overflow"][0] if adv == over_net else 0)
        if a1 == tie_net:
            assert set(want[g]["actions"][2::3]) == {1}   # the first of the tied pair
        if adv == over_net:
            assert set(want[g]["actions"][0::3]) == {0}   # no action -> 0, the game goes on
        want_st |= want[g]["status"]
        assert eq_bits(got[g], want[g]["rewards"]), (g, got[g], want[g]["rewards"])
    assert want_st == E.PROPERTY["fc2_overflow"][0] and int(s.ro.status.item()) == FOREIGN | want_st
