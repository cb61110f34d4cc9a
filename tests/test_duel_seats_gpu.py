"""The duel's scripted seats on the device (csrc/duel_seats.hip, include/coevo_duel_seats.h, coevonet_amd/duel_crossplay.py):
1. coevo_duel_seat_step alone against tests/duel_seat_cases.DuelSeatRef - state words, fp64 returns as bits, the seats' action
   words, the status word and every frame byte after every launch, between guards; crafted tracker states; the deciding point in
   either half of a launch.
2. the fused launches against the separate pair, float32 and float16, with the one stated exception pinned both ways.
3. DuelSeatRollout / HalfDuelSeatRollout against the host loop (_play_atari_aec with the net and DuelTracker or a baseline player).
4. DuelCrossPlay, duel_test_agents and duel_cross_play_checkpoints against the loop over play_game.
Every comparison is exact equality; every whole-game reference is shown to hold a scored point."""
import numpy as np
import pytest
import torch

from coevonet_amd import atari_duel as ad
from coevonet_amd import duel_crossplay as dx
from coevonet_amd import game_logic as gl
from coevonet_amd import io_utils
from coevonet_amd import lib as L
from coevonet_amd.baselines import ConstantBaseline, PeriodicBaseline, RandomBaseline
from coevonet_amd.deepqn import DeepQN, DeepQNHalf
from coevonet_amd.dqn_population import half_values
from coevonet_amd.population import ROLES2
from tests import crossplay_cases as cc
from tests import dqn_edge_nets as E
from tests import duel_cases as dc
from tests import duel_seat_cases as sc
from tests.util import Bag

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 32
OWN = L.K_DUEL["COEVO_DUEL_CREDIT_OWN"]
SW = ad.STATE_WORDS


@pytest.fixture(scope="module", autouse=True)
def release_nets():
    yield
    E.release()


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


class SeatDevice:
    """game state (77 everywhere), returns (5.5), the seats' action words (-77) and frame rows (0xA5), each between guards of
    the same fill; the status word"""

    def __init__(self, G, n_rows, C):
        self.G, self.R, self.nbytes = G, n_rows, 84 * 84 * C
        self.state = torch.full((SW * G + 2 * PAD,), dc.FILL_STATE, dtype=torch.int32, device=DEV)
        self.acc = torch.full((3 * G + 2 * PAD,), dc.FILL_ACC, dtype=torch.float64, device=DEV)
        self.script = torch.full((G + 2 * PAD,), sc.FILL_SCRIPT, dtype=torch.int32, device=DEV)
        self.frames = torch.full((n_rows + 2, self.nbytes), dc.POISON, dtype=torch.uint8, device=DEV)
        self.status = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.state_p, self.acc_p, self.script_p = (x[PAD:].data_ptr() for x in (self.state, self.acc, self.script))
        self.frames_p = self.frames[1:].data_ptr()
        assert self.frames_p % 16 == 0

    def poke(self, words):
        self.state[PAD:PAD + SW * self.G].copy_(dev(np.ascontiguousarray(words, dtype=np.int32).reshape(-1)))

    def read(self):
        torch.cuda.synchronize()
        s, a, k, f = (x.cpu().numpy() for x in (self.state, self.acc, self.script, self.frames))
        assert (s[:PAD] == dc.FILL_STATE).all() and (s[-PAD:] == dc.FILL_STATE).all(), "a state guard word was written"
        assert (a[:PAD] == dc.FILL_ACC).all() and (a[-PAD:] == dc.FILL_ACC).all(), "a guard word of the returns was written"
        assert (k[:PAD] == sc.FILL_SCRIPT).all() and (k[-PAD:] == sc.FILL_SCRIPT).all(), "a guard word of the seats' actions"
        assert (f[0] == dc.POISON).all() and (f[-1] == dc.POISON).all(), "a guard frame row was written"
        return s[PAD:-PAD].reshape(self.G, SW), a[PAD:-PAD].reshape(self.G, 3), k[PAD:-PAD], f[1:-1], int(self.status.item())


class Chain:
    """one device and one DuelSeatRef driven launch by launch; after EVERY launch every buffer is compared"""

    def __init__(self, ord0, lim, gen, per_gen, C, n_act, seed, seats, parity, points, own, R=None):
        G = len(ord0)
        self.d = SeatDevice(G, R or G, C)
        self.ref = sc.DuelSeatRef(ord0, lim, gen, per_gen, C, n_act, seed, seats, parity, points=points, own=bool(own))
        self.d_ord0, self.d_lim = dev(np.asarray(ord0, dtype=np.int64)), dev(np.asarray(lim, dtype=np.int32))
        self.d_gen = None if gen is None else dev(np.array([gen], dtype=np.int32))
        self.d_seats = dev(sc.seat_table(seats))
        self.per_gen, self.C, self.n_act, self.seed, self.points, self.flags = per_gen, C, n_act, seed, points, OWN if own else 0
        self.parity = parity

    def launch(self, kind, t, row_prev=None, actions=None, row_next=None, frames=True):
        d, ref, C = self.d, self.ref, self.C
        G = d.G
        row_next = np.arange(G, dtype=np.int32) if row_next is None else row_next
        want_frames = np.full((d.R, 84, 84, C), dc.POISON, dtype=np.uint8)
        d.frames.fill_(dc.POISON)
        d_prev, d_act = (dev(np.asarray(row_prev, dtype=np.int32)), dev(np.asarray(actions, dtype=np.int32))) if t else (None, None)
        d_next = dev(np.asarray(row_next, dtype=np.int32))
        head = (d.state_p, d.acc_p, G, L._p(self.d_ord0), L._p(self.d_gen), self.per_gen, t, L._p(self.d_lim))
        tail = (C, self.n_act, self.seed, self.points, self.flags)
        if kind == "reset":
            rendered = ref.step(0, None, None, row_next, want_frames if frames else None)
            L.call("coevo_duel_step", *head, None, None, L._p(d_next), d.frames_p if frames else None, *tail)
        else:
            rendered = ref.seat_step(t, row_prev, actions, row_next, want_frames if frames else None)
            L.call("coevo_duel_seat_step", *head, L._p(self.d_seats), self.parity, L._p(d_prev), L._p(d_act), d.script_p,
                   L._p(d_next), d.frames_p if frames else None, *tail, L._p(d.status))
        state, acc, script, got, status = d.read()
        assert np.array_equal(state, ref.state), (t, state.tolist(), ref.state.tolist())
        assert np.array_equal(acc.view(np.uint64), ref.acc.view(np.uint64)), (t, acc.tolist(), ref.acc.tolist())
        assert np.array_equal(script, ref.script_actions), (t, script.tolist(), ref.script_actions.tolist())
        assert status == ref.status, (t, status, ref.status)
        for r in range(d.R):
            assert np.array_equal(got[r], want_frames[r].reshape(-1)), (t, r, r in rendered)
            assert (r in rendered) or (got[r] == dc.POISON).all()
        return rendered

    def poke(self, g, word15=None, **words):
        if word15 is not None:
            self.ref.state[g, 15] = np.uint32(word15).astype(np.int32)
        self.ref.poke(g, **words)

    def push(self):
        self.d.poke(self.ref.state)


# ------------------------------------------------------------------------------------------- 1. the seat kernel alone
@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("n_act", [6, 18])
@pytest.mark.parametrize("C", [4, 6])
@pytest.mark.parametrize("G", [1, 2, 7])
def test_seat_steps_vs_numpy(G, C, n_act, parity):
    """a T = 9 rollout's launches and one more, random net action words (-1, n_actions and 255 among them) over G games: seat
    kinds mixed in one launch (an invalid constant seat plays 0 and raises COEVO_ST_BAD_TASK), limits 0, 1, 2, T - 1, T side by
    side, a disabled game, ordinals 0 and 2^63 - 1 (one moved by the generation word), seeds 0 / 2^64 - 1 / the reference's, rows
    permuted anew at every launch, credit flag by case; game 0 is poked near a plane so that points and serves are booked"""
    T = 9
    seed = (0, 2 ** 64 - 1, dc.SEED)[(G + C + n_act + parity) % 3]
    own = (G + n_act // 6 + parity) % 2
    per_gen, gen = 5, 2
    ord0 = np.array([2 ** 63 - 1 - gen * per_gen, -gen * per_gen, 7, -1 - gen * per_gen, 1, 2 ** 40, 3][:G], dtype=np.int64)
    lim = np.array([T, T - 1, 2, T, 0, 1, T][:G], dtype=np.int32)      # (game 3 is disabled: ordinal -1)
    seats = [sc.raw_seat(sc.TRACKER), sc.raw_seat(sc.CONSTANT, n_act), sc.raw_seat(sc.RANDOM, 0, 2 ** 64 - 1),
             sc.raw_seat(sc.PERIODIC, 5), sc.raw_seat(sc.CONSTANT, 2), sc.raw_seat(sc.TRACKER), sc.raw_seat(sc.RANDOM, 0, 0)][:G]
    R = G + 2
    ch = Chain(ord0, lim, gen, per_gen, C, n_act, seed, seats, parity, 2, own, R=R)
    ref = ch.ref
    assert ref.ordinal[0] == 2 ** 63 - 1 and (G < 2 or ref.ordinal[1] == 0) and (G < 4 or ref.ordinal[3] == -1)
    rng = np.random.default_rng([G, C, n_act, parity])
    pool = np.array(list(range(n_act)) + [-1, n_act, 255], dtype=np.int32)
    rendered = 0
    launches = sc.schedule(T + 2, parity)
    for i, (kind, t) in enumerate(launches):
        rows = lambda s: np.array([(2 * g + s) % R for g in range(G)], dtype=np.int32)      # (2 and R = 3, 4, 9: distinct rows)
        row_next, row_prev = rows(i), rows(i + 1)
        actions = np.full(R, -9, dtype=np.int32)
        actions[row_prev] = rng.choice(pool, size=G)
        rendered += len(ch.launch(kind, t, row_prev if t else None, actions, row_next, frames=i + 1 < len(launches)))      # (the last: bookkeeping only)
        if t == 0:      # game 0: the ball two world steps from the left plane, the paddle far away -> a point, then serve 1
            ch.poke(0, bx=11, by=70, vx=-3, vy=0, p0=0)
            ch.push()
    assert rendered >= T // 2 and sum(ref.games[0].score) >= 1
    assert ref.status == (sc.BAD_TASK if G >= 2 else 0)
    if G >= 2:
        assert ref.script_actions[1] == 0
    if G == 7:
        assert [g.t for g in ref.games][1:6] == [T - 1, 2, 0, 0, 1]
        assert ref.script_actions[3] == sc.FILL_SCRIPT == ref.script_actions[4]      # never played: the word is left alone


def _tracker_targets():
    """(s, bx, by, p): the ball in the tracker's column around its paddle, |d| = 4 and 6 on both sides, paddles at 0 and 72"""
    out = []
    for s, cols in ((0, (3, 4)), (1, (77, 78))):
        for bx in cols:
            out += [(s, bx, 30 + off, 30) for off in (-2, -1, 0, 5, 11, 12)]
        out += [(s, 41, by, 30) for by in (37, 33, 38, 32)]      # d = 2 by + 2 - 72 = 4, -4, 6, -6
        out += [(s, 41, 0, 0), (s, 41, 82, 72), (s, cols[0], 0, 0), (s, cols[1], 82, 72)]
    return out


@pytest.mark.parametrize("n_act", [6, 3])
@pytest.mark.parametrize("parity", [0, 1])
def test_crafted_tracker_states(parity, n_act):
    """one game per crafted snapshot, poked so that the tracker of player `parity` reads it: parity 1 reads the poked word 15
    itself (the net's step before it is first_0's and moves nothing); parity 0 reads the snapshot of the net's world step, which
    is poked one ball step short of the target.  n_actions = 3: action 2 moves the paddle, action 3 is outside the space"""
    cases = [c for c in _tracker_targets() if c[0] == parity]
    G, C = len(cases), 4
    ch = Chain(np.full(G, 3, dtype=np.int64), np.full(G, 100, dtype=np.int32), None, 0, C, n_act, dc.SEED,
               [sc.raw_seat(sc.TRACKER)] * G, parity, 21, 0)
    rows = np.arange(G, dtype=np.int32)[::-1].copy()
    ch.launch("reset" if parity else "seat", 0, row_next=rows)
    other = 36
    for g, (s, bx, by, p) in enumerate(cases):
        p0, p1 = (p, other) if s == 0 else (other, p)
        if parity:      # second_0 acts in the same launch on the word as poked
            ch.poke(g, word15=ad.snapshot_word(bx, by, p0, p1), bx=bx, by=by, vx=-3, vy=0, p0=p0, p1=p1, pending=ad.NO_ACTION)
        else:           # first_0 acts behind the net's world step: the ball moves 3 columns toward the target, away from a plane
            ch.poke(g, bx=bx - 3, by=by, vx=3, vy=0, p0=p0, p1=p1, pending=0)
    ch.push()
    t = 1 if parity else 2
    before = ch.ref.state.copy()
    ch.launch("seat", t, rows, np.zeros(G, dtype=np.int32), rows)
    want = [dx.duel_tracker_word(ad.snapshot_word(bx, by, *((p, other) if s == 0 else (other, p))), s) for s, bx, by, p in cases]
    assert ch.ref.script_actions.tolist() == want and set(want) == {0, 2, 3}
    hidden = [g for g, (s, bx, by, p) in enumerate(cases) if bx in (3, 4, 77, 78) and by < p <= by + 1]
    assert hidden      # the ball covers paddle row p itself: min(p, by) decided
    # what the action did to the seat's paddle: action 2 moves up while 2 < n_actions, action 3 moves down only when 3 < n_actions
    if parity:
        for g, (s, bx, by, p) in enumerate(cases):
            move = {0: 0, 2: -4, 3: 4 if n_act > 3 else 0}[want[g]]
            assert ch.ref.state[g, 6] == min(max(before[g, 6] + move, 0), 72), (g, cases[g])
    else:
        assert ch.ref.state[:, 0].tolist() == want      # first_0's action waits in word 0


@pytest.mark.parametrize("C,own", [(4, 0), (6, 1)])
@pytest.mark.parametrize("half_of_launch", ["first", "second"])
def test_the_deciding_point_inside_a_seat_launch(half_of_launch, C, own):
    """points_to_win = 1.  first: the net is second_0 and its step ends the game - the seat's step of the same launch is not
    booked, its script_actions word keeps its fill and no frame byte is written.  second: the seat is second_0 and its step ends
    the game - no frame is written.  Later launches write nothing; the game beside it plays on"""
    n_act, G = 6, 2
    parity = 0 if half_of_launch == "first" else 1
    ch = Chain(np.array([4, 5], dtype=np.int64), np.array([20, 20], dtype=np.int32), None, 0, C, n_act, dc.SEED,
               [sc.raw_seat(sc.CONSTANT, 0), sc.raw_seat(sc.TRACKER)], parity, 1, own, R=3)
    ref, rows = ch.ref, np.array([2, 0], dtype=np.int32)
    for kind, t in sc.schedule(9, parity):
        actions = np.array([1, -9, 0], dtype=np.int32)
        before = (ref.state[0].copy(), ref.acc[0].copy(), ref.script_actions[0])
        rendered = ch.launch(kind, t, rows if t else None, actions, rows)
        if t == 0:      # game 0 reaches the right plane in the next world step, far from second_0's paddle
            ch.poke(0, bx=74, by=10, vx=3, vy=0, p1=60)
            ch.push()
        if kind == "seat" and t in (1, 2):
            assert ref.games[0].ended == 2 and ref.games[0].score == [1, 0] and ref.state[0, 11] == 2
            assert ref.acc[0].tolist() == ([0.0, -1.0, 0.0] if own else [0.0, 1.0, 0.0])
            assert rendered == [0]                      # game 1's row alone
            # first: the seat (first_0) played step 0 only - its word holds that action, step 2 left it alone
            assert ref.script_actions[0] == 0 and (parity == 1 or before[2] == 0)
        if t >= 3:
            assert rendered in ([0], []) and np.array_equal(ref.state[0], before[0]) and np.array_equal(ref.acc[0], before[1])
            assert ref.script_actions[0] == before[2]
    assert ref.games[0].ended == 2 < 20 and not ref.games[1].ended and ref.state[1, 11] == 0


def test_a_seat_word_is_left_alone_when_the_nets_step_ends_the_game():
    """(the case above with a seat whose action is never 0, so that an untouched word cannot be mistaken for a played one)"""
    ch = Chain(np.array([4], dtype=np.int64), np.array([20], dtype=np.int32), None, 0, 4, 6, dc.SEED,
               [sc.raw_seat(sc.CONSTANT, 5)], 0, 1, 0)
    rows = np.zeros(1, dtype=np.int32)
    ch.launch("seat", 0)
    assert ch.ref.script_actions[0] == 5
    ch.d.script.fill_(sc.FILL_SCRIPT)
    ch.ref.script_actions[:] = sc.FILL_SCRIPT
    ch.poke(0, bx=74, by=10, vx=3, vy=0, p1=60)
    ch.push()
    assert ch.launch("seat", 2, rows, np.array([1], dtype=np.int32), rows) == []
    assert ch.ref.games[0].ended == 2 and ch.ref.script_actions[0] == sc.FILL_SCRIPT
    assert ch.launch("seat", 4, rows, np.array([1], dtype=np.int32), rows) == []


def test_refusals_write_nothing():
    ch = Chain(np.array([7, 8], dtype=np.int64), np.array([9, 9], dtype=np.int32), None, 0, 4, 6, dc.SEED,
               [sc.raw_seat(sc.TRACKER)] * 2, 1, 21, 0)
    ch.launch("reset", 0)
    d = ch.d
    rows, acts = dev(np.arange(2, dtype=np.int32)), dev(np.zeros(2, dtype=np.int32))
    args = [d.state_p, d.acc_p, 2, L._p(ch.d_ord0), None, 0, 1, L._p(ch.d_lim), L._p(ch.d_seats), 1, L._p(rows), L._p(acts),
            d.script_p, L._p(rows), d.frames_p, 4, 6, dc.SEED, 21, 0, L._p(d.status)]
    at = dict(t=6, seats=8, parity=9, script=12, row_next=13, frames=14, status=20)
    d.frames.fill_(dc.POISON)
    for bad in (dict(t=2), dict(t=0), dict(parity=0), dict(parity=2), dict(seats=None), dict(script=None), dict(status=None),
                dict(row_next=None), dict(frames=d.frames_p + 4), dict(t=65537)):
        a = list(args)
        for k, v in bad.items():
            a[at[k]] = v
        assert getattr(L.load(), "coevo_duel_seat_step")(*a, L._stream()) == L.K["COEVO_ERR_ARG"], bad
    state, acc, script, frames, status = d.read()
    assert np.array_equal(state, ch.ref.state) and not acc.any() and (script == sc.FILL_SCRIPT).all()
    assert (frames == dc.POISON).all() and status == 0


# ------------------------------------------------------------------------------------------- 2. fused = unfused
SENT_A = -7


def pack_slab(nets, half, C, n, tiled=False):
    sym = "coevo_dqn16" if half else "coevo_dqn"
    stride = int(getattr(L.load(), sym + "_slab_stride")(C, n))
    slab = torch.zeros(len(nets) * stride, dtype=torch.int32 if half else torch.float32, device=DEV)
    L.call(sym + "_pack", L._p(dev(np.stack(nets))), L._p(slab), len(nets), C, n)
    return slab, stride


def play_seat_twin(half, fused, nan_live, parity):
    """3 games over 2 nets (plain, all-NaN logits) against tracker seats, T = 8, points_to_win = 1: game 0 (plain) plays on,
    game 1 (plain) is poked so that it ends at the next world step, game 2 (NaN) is live or - not nan_live - poked as ended from
    the start.  fused: the hidden forward + the out_duel_seat_step launch; else the argmax forward + coevo_duel_seat_step"""
    C, n, T = 4, 6, 8
    nets = [E.make("plain", C, n), E.make("all_nan_logits", C, n)]
    if half:
        nets = [half_values(w) for w in nets]
    slab, stride = pack_slab(nets, half, C, n)
    ro = (dx.HalfDuelSeatRollout if half else dx.DuelSeatRollout)([0, 0, 1], [0, stride], parity, sc.seat_table([dx.TrackerSeat()] * 3),
                                                                 [3, 4, 5], C, n, slab, dc.SEED, DEV, points_to_win=1)
    ro.fused_out = fused
    ro.set_limits([T, T, T])
    ro.actions.fill_(SENT_A)
    for kind, t in ro.steps(T):
        ro.enqueue_step(kind, t, T)
        if t == 0:
            torch.cuda.synchronize()
            state = ro.dstate.cpu().numpy()
            state[1, 1:7] = [11, 70, -3, 0, 0, 36]      # two world steps from the left plane, first_0's paddle out of reach
            if parity == 0:
                state[1, 0] = 0                          # (first_0 is the tracker: whatever it played at step 0, it stays put)
                state[1, 1:7] = [8, 70, -3, 0, 0, 36]    # ... and one world step from the plane, before it can get there
            if not nan_live:
                state[2, 11] = 1
            ro.dstate.copy_(dev(state))
    torch.cuda.synchronize()
    return dict(state=ro.dstate.cpu().numpy(), acc=ro.acc.cpu().numpy(), frames=ro.frames.cpu().numpy(),
                status=int(ro.status.item()), actions=ro.actions.cpu().numpy(), script=ro.script_actions.cpu().numpy(),
                rows=ro.rows.cpu().numpy())


@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("half", [False, True], ids=["float32", "float16"])
def test_fused_seat_launch_equals_the_separate_pair(half, parity):
    """every buffer equal; the status word differs only where the header says: a net without an action in a game that has ENDED
    raises COEVO_ST_NO_ACTION in the separate pair (its forward computes every row) and nothing in the fused launch (the row of
    a finished game is not evaluated, its action word keeps what it held); the same net in a live game raises the bit in both"""
    for nan_live, want_status in ((False, (E.NO_ACTION, 0)), (True, (E.NO_ACTION, E.NO_ACTION))):
        A, B = play_seat_twin(half, False, nan_live, parity), play_seat_twin(half, True, nan_live, parity)
        assert np.array_equal(A["state"], B["state"]) and np.array_equal(A["acc"].view(np.uint64), B["acc"].view(np.uint64))
        assert np.array_equal(A["frames"], B["frames"]) and np.array_equal(A["script"], B["script"])
        assert (A["status"], B["status"]) == want_status
        s, rows = B["state"], B["rows"]
        assert s[0, 11] == 0 and s[1, 11] in (2, 4) and s[1, 8] == 1 and s[2, 11] == (0 if nan_live else 1)
        assert A["actions"][rows[0]] == B["actions"][rows[0]]
        if not nan_live:    # never evaluated in the fused launch; the separate pair stores action 0 for the faulted row
            assert B["actions"][rows[2]] == SENT_A and A["actions"][rows[2]] == 0
        else:               # the faulted row plays action 0 in both
            assert B["actions"][rows[2]] == 0 == A["actions"][rows[2]]


# ------------------------------------------------------------------------------------------- 3. whole games
def make_net(half, C, n, seed):
    torch.manual_seed(seed)
    return (DeepQNHalf if half else DeepQN)(C, n, "float16" if half else "float32")


def serve_toward(side, start=1):
    """the first reset ordinal >= start at which a ConstantBaseline(3) seat on `side` (0 first_0, 1 second_0) concedes the first
    serve whatever the other side plays: the serve flies toward it and passes its paddle, parked at the bottom, before the ball
    has been anywhere near the other paddle"""
    for o in range(start, start + 64):
        g = ad.DuelGame(dc.SEED, o, 6)
        if (g.vx > 0) != bool(side):
            continue
        for _ in range(13):
            g.step(0 if side else 3)
            g.step(3 if side else 0)
        if g.score[1 - side] >= 1:
            return o
    raise AssertionError("no such ordinal")


def host_seat(seat, env, parity, n):
    return ad.DuelTracker(parity) if isinstance(seat, dx.TrackerSeat) else sc.SeatPlayer(seat, env, parity, n)


def host_game(net, seat, parity, ordinal, T, C, n, points, credit, game="pong_v3"):
    """_play_atari_aec with the net's façade forward on one side and the seat's host twin on the other -> (returns, env)"""
    env = dc.env_at(ordinal, game=game, channels=C, points_to_win=points, credit=credit)
    env.reset()
    players = [net, host_seat(seat, env, parity, n)] if parity else [host_seat(seat, env, parity, n), net]
    r = gl._play_atari_aec(env, players[0], players[1], Bag(game=game, max_timesteps_per_episode=T), False)
    return (float(r[0]), float(r[1])), env


@pytest.mark.parametrize("credit", ["next", "own"])
@pytest.mark.parametrize("C", [4, 6])
@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("half", [False, True], ids=["float32", "float16"])
def test_seat_rollout_equals_the_host_loop(half, parity, C, credit):
    """one rollout of ten games with limits 1, 2, 3, 30 and 61 against tracker, random, periodic and constant seats = the host
    loop game by game: returns, final state words (the env object's books among them).  The constant seat parks its paddle at
    the bottom and its games are served toward it, so the reference holds a point whatever the net plays"""
    n = 6 if C == 4 else 18
    game = "pong_v3" if C == 4 else "boxing_v2"
    net = make_net(half, C, n, 50 + C)
    o = serve_toward(parity)
    games = [(1, 1, dx.TrackerSeat()), (2, 2, dx.TrackerSeat()), (3, 3, RandomBaseline(9)), (30, 4, dx.TrackerSeat()),
             (61, 5, dx.TrackerSeat()), (61, o, ConstantBaseline(3)), (30, o, ConstantBaseline(3)),
             (61, serve_toward(parity, o + 1), ConstantBaseline(3)), (61, 6, PeriodicBaseline(2)), (61, 7, RandomBaseline(1))]
    points = 2
    want = [host_game(net, seat, parity, ordinal, T, C, n, points, credit, game) for T, ordinal, seat in games]
    assert sum(sum(env.state.score) for _, env in want) >= 1      # the reference alone: a point was scored
    flat = net.flat()
    slab, stride = pack_slab([flat], half, C, n)
    ro = (dx.HalfDuelSeatRollout if half else dx.DuelSeatRollout)([0] * len(games), [0], parity,
                                                                 sc.seat_table([g[2] for g in games]), [g[1] for g in games], C, n,
                                                                 slab, dc.SEED, DEV, points_to_win=points, credit=credit)
    ro.set_limits([g[0] for g in games])
    ro.enqueue(61)
    torch.cuda.synchronize()
    L.raise_on_status(ro.status)
    acc, words = ro.acc.cpu().numpy(), ro.dstate.cpu().numpy()
    for g, ((r, env), (T, ordinal, seat)) in enumerate(zip(want, games)):
        assert tuple(acc[g, :2]) == r and acc[g, 2] == 0, (g, T, seat, acc[g].tolist(), r)
        assert np.array_equal(words[g], env.state.words()), (g, T, seat, words[g].tolist(), env.state.words().tolist())
        assert (words[g, 11] or T) == env.state.t


# ------------------------------------------------------------------------------------------- 4. cross-play
def loop_over_play_game(first, second, flat_first, flat_second, E_, first_ordinal, T, C, n, points, credit):
    """the table by main.py's loop: play_game (through the host loop) per game -> rewards [A B E][3], points [A, B, E, 2],
    ended [A, B, E]"""
    A, B = len(first), len(second)
    rewards, pts, ended = np.zeros((A * B * E_, 3)), np.zeros((A, B, E_, 2), dtype=np.int64), np.zeros((A, B, E_), dtype=np.int64)
    args = Bag(game="pong_v3", max_evaluation_steps=T, max_timesteps_per_episode=1, coevo_host_aec=True)
    for a in range(A):
        for b in range(B):
            for e in range(E_):
                env = dc.env_at(first_ordinal + e, channels=C, points_to_win=points, credit=credit)
                p1 = first[a] if flat_first else host_seat(first[a], env, 0, n)
                p2 = second[b] if flat_second else host_seat(second[b], env, 1, n)
                r = gl.play_game(env=env, player1=p1, player2=p2, args=args, eval=True)
                rewards[(a * B + b) * E_ + e, :2] = r
                pts[a, b, e], ended[a, b, e] = env.state.score, env.state.ended
    return rewards, pts, ended


def assert_duel_result(res, rewards, pts, ended, A, B, E_):
    payoff, *marg = cc.reduce_ref(rewards, A, B, 1, E_)
    assert res.n_games == A * B * E_
    assert same_bits(res.rewards, rewards.reshape(A, B, E_, 3)[..., :2])
    assert same_bits(res.payoff, payoff.reshape(A, B, 3)[..., :2])
    assert sorted(res.marginals) == sorted(ROLES2)
    for r, m in zip(ROLES2, marg):
        assert same_bits(res.marginals[r], m[:, :2]), r
    assert np.array_equal(res.points, pts) and np.array_equal(res.ended, ended)
    assert same_bits(res.point_margin, (pts[..., 0] - pts[..., 1]).mean(axis=-1))


@pytest.mark.parametrize("seat_side,points", [(1, 1), (0, 2)])
def test_duel_cross_play_nets_against_seats(seat_side, points):
    """2 nets x {TrackerSeat, RandomBaseline(1), ConstantBaseline(3)} x 2 episodes, the seats on each side in turn; then one net
    replaced by ``upload``.  points_to_win = 1: a game ends before its limit"""
    C, n, E_, T = 4, 6, 2, 61
    nets = [make_net(False, C, n, 60 + i) for i in range(3)]
    seats = [dx.TrackerSeat(), RandomBaseline(1), ConstantBaseline(3)]
    first = serve_toward(seat_side)
    lists = (nets[:2], seats) if seat_side else (seats, nets[:2])
    cp = dx.DuelCrossPlay(lists[0], lists[1], C, n, episodes=E_, limit=T, points_to_win=points, env_seed=dc.SEED)
    assert type(cp.ro).__name__ == "DuelSeatRollout" and cp.ro.script_parity == seat_side
    res = cp.run(first)
    rewards, pts, ended = loop_over_play_game(lists[0], lists[1], seat_side == 1, seat_side == 0, E_, first, T, C, n, points, "next")
    assert pts.sum() >= 1 and (points > 1 or ((ended > 0) & (ended < T)).any())      # the reference alone
    A, B = len(lists[0]), len(lists[1])
    assert_duel_result(res, rewards, pts, ended, A, B, E_)
    net_role = ROLES2[1 - seat_side]
    cp.upload(net_role, 1, nets[2])
    with pytest.raises(ValueError, match="scripted"):
        cp.upload(ROLES2[seat_side], 0, nets[2])
    swapped = ([nets[0], nets[2]], seats) if seat_side else (seats, [nets[0], nets[2]])
    rewards2, pts2, ended2 = loop_over_play_game(swapped[0], swapped[1], seat_side == 1, seat_side == 0, E_, first, T, C, n, points,
                                                 "next")
    assert_duel_result(cp.run(first), rewards2, pts2, ended2, A, B, E_)
    tiled = dx.DuelCrossPlay(lists[0], lists[1], C, n, episodes=E_, limit=T, points_to_win=points, env_seed=dc.SEED,
                             fc1_layout="tiled")
    assert_duel_result(tiled.run(first), rewards, pts, ended, A, B, E_)


@pytest.mark.parametrize("precision", ["float32", "float16"])
def test_duel_cross_play_nets_against_nets(precision):
    """2 x 2 nets x 2 episodes through DuelRollout / HalfDuelRollout = the loop over play_game through the host loop"""
    half = precision == "float16"
    C, n, E_, T, points, first = 4, 6, 2, 61, 1, 3
    nets = [make_net(half, C, n, 70 + i) for i in range(4)]
    cp = dx.DuelCrossPlay(nets[:2], nets[2:], C, n, episodes=E_, limit=T, points_to_win=points, credit="own", precision=precision,
                          env_seed=dc.SEED)
    assert type(cp.ro).__name__ == ("HalfDuelRollout" if half else "DuelRollout")
    rewards, pts, ended = loop_over_play_game(nets[:2], nets[2:], True, True, E_, first, T, C, n, points, "own")
    assert pts.sum() >= 1 and ((ended > 0) & (ended < T)).any()      # the reference alone
    assert_duel_result(cp.run(first), rewards, pts, ended, 2, 2, E_)
    tiled = dx.DuelCrossPlay(nets[:2], nets[2:], C, n, episodes=E_, limit=T, points_to_win=points, credit="own",
                             precision=precision, env_seed=dc.SEED, fc1_layout="tiled")
    assert_duel_result(tiled.run(first), rewards, pts, ended, 2, 2, E_)
    cp.ro.close()
    tiled.ro.close()


def test_half_nets_against_seats_in_a_table(monkeypatch):
    """a float16 net against {constant, tracker} through HalfDuelSeatRollout = the host loop; the tiled fc1 layout and the
    COEVO_DQN16_FUSED_OUT=0 route (coevo_dqn16_forward_argmax + coevo_duel_seat_step) give the same words"""
    C, n, E_, T, points = 6, 18, 2, 61, 2
    nets, seats = [make_net(True, C, n, 80)], [ConstantBaseline(3), dx.TrackerSeat()]
    first = serve_toward(1)
    cp = dx.DuelCrossPlay(nets, seats, C, n, episodes=E_, limit=T, points_to_win=points, credit="own", precision="float16",
                          env_seed=dc.SEED)
    assert type(cp.ro).__name__ == "HalfDuelSeatRollout"
    A, B = 1, 2
    rewards, pts, ended = np.zeros((A * B * E_, 3)), np.zeros((A, B, E_, 2), dtype=np.int64), np.zeros((A, B, E_), dtype=np.int64)
    for b in range(B):
        for e in range(E_):
            r, env = host_game(nets[0], seats[b], 1, first + e, T, C, n, points, "own", game="boxing_v2")
            rewards[b * E_ + e, :2], pts[0, b, e], ended[0, b, e] = r, env.state.score, env.state.ended
    assert pts.sum() >= 1      # the reference alone
    assert cp.ro.fused_out
    assert_duel_result(cp.run(first), rewards, pts, ended, A, B, E_)
    kw = dict(episodes=E_, limit=T, points_to_win=points, credit="own", precision="float16", env_seed=dc.SEED)
    assert_duel_result(dx.DuelCrossPlay(nets, seats, C, n, fc1_layout="tiled", **kw).run(first), rewards, pts, ended, A, B, E_)
    monkeypatch.setenv("COEVO_DQN16_FUSED_OUT", "0")
    unfused = dx.DuelCrossPlay(nets, seats, C, n, **kw)
    assert not unfused.ro.fused_out
    assert_duel_result(unfused.run(first), rewards, pts, ended, A, B, E_)


def duel_args(tmp_path, agents, **kw):
    path = str(tmp_path / "hof.pth")
    io_utils.save_model(agents, path)
    args = Bag(algorithm="GA", game="pong_v3", max_evaluation_steps=61, max_timesteps_per_episode=1, test=True,
               coevo_atari_env="duel", coevo_duel_points=1, **kw)
    for attr in ("GA_hof_to_test_agent_0", "GA_hof_to_test_agent_1", "GA_hof_to_test_adversary"):
        setattr(args, attr, path)
    return args


def test_duel_test_agents_equals_the_loop_over_play_game(tmp_path):
    """self-play and a TrackerSeat opponent: main.py's sums and division over play_game on a twin env, the mean points beside
    them; the env's n_resets moves on by `episodes`"""
    episodes = 4
    plain = Bag(algorithm="GA", game="pong_v3", coevo_atari_env="duel", coevo_duel_points=1)
    env, twin = gl.initialize_env(plain), gl.initialize_env(plain)
    assert type(env) is ad.DuelAEC and env.points_to_win == 1
    torch.manual_seed(90)
    agent = gl.create_agent(env, plain)
    agent.mutate(0.02)
    args = duel_args(tmp_path, [agent], play_against_yourself=True)
    host = Bag(**dict(vars(args), coevo_host_aec=True))
    for opponent in (None, dx.TrackerSeat()):
        start = env.n_resets
        twin.n_resets = start
        got = dx.duel_test_agents(env, args, episodes=episodes, opponent=opponent)
        total, pts, ended = [0, 0], [], []
        for _ in range(episodes):         # main.py:234-245
            other = agent.model if opponent is None else ad.DuelTracker(1)
            r = gl.play_game(env=twin, player1=agent.model, player2=other, args=host, eval=True)
            total = [t + x for t, x in zip(total, r)]
            pts.append(list(twin.state.score))
            ended.append(twin.state.ended)
        want = tuple(t / episodes for t in total)
        assert sum(map(sum, pts)) >= 1 and any(0 < e < 61 for e in ended)      # the reference alone
        assert same_bits(got[0], want), (got, want)
        assert got[1] == tuple(float(v) for v in np.array(pts, dtype=np.int64).mean(axis=0))
        assert env.n_resets == twin.n_resets == start + episodes


def test_duel_cross_play_checkpoints_plays_every_member(tmp_path):
    args = Bag(algorithm="GA", game="pong_v3", max_evaluation_steps=61, max_timesteps_per_episode=1, coevo_atari_env="duel",
               coevo_duel_points=1)
    env = gl.initialize_env(args)
    torch.manual_seed(91)
    agents = {r: [gl.create_agent(env, args) for _ in range(k)] for r, k in (("first_0", 2), ("second_0", 1))}
    paths = {}
    for r in ROLES2:
        for a in agents[r]:
            a.mutate(0.02)
        paths[r] = str(tmp_path / f"{r}.pth")
        io_utils.save_model(agents[r], paths[r])
    res = dx.duel_cross_play_checkpoints(env, args, paths, episodes=2)
    assert env.n_resets == 3 and res.payoff.shape == (2, 1, 2) and res.points.shape == (2, 1, 2, 2) and res.ended.shape == (2, 1, 2)
    rewards, pts, ended = loop_over_play_game([a.model for a in agents["first_0"]], [a.model for a in agents["second_0"]], True,
                                              True, 2, 1, 61, env.C, env.n_actions, 1, "next")
    assert pts.sum() >= 1 and ((ended > 0) & (ended < 61)).any()      # the reference alone
    assert_duel_result(res, rewards, pts, ended, 2, 1, 2)
    again = dx.duel_cross_play_checkpoints(env, args, paths, episodes=2, first_ordinal=1)      # a stated ordinal: the env is left alone
    assert env.n_resets == 3 and same_bits(again.rewards, res.rewards) and np.array_equal(again.points, res.points)
