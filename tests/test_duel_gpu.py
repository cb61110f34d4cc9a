"""The paddle duel on the device (csrc/duel_env.hip, include/coevo_duel.h) against plain numpy and code that exists without it:
1. coevo_duel_step alone against tests/duel_cases.DuelRef - state words, fp64 returns as bits and every frame byte after every
   launch, between guard words and rows; crafted states; the game that ends; limits, a disabled game, deep ordinals, extreme
   seeds, permuted rows, action words outside the space, both credit flags; refusals that write nothing.
2. the fused launches against the separate pair (coevo_dqn_forward_argmax + coevo_duel_step), float32 and float16, with the one
   stated exception pinned both ways.
3. play_game on the device against play_game through the host loop (_play_atari_aec), and against the oracle's forward.
4. the four engines against a host replay of every game of their table, and the trainers with the graph on and off.
Every comparison is exact equality."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from coevonet_amd import atari_duel as ad
from coevonet_amd import lib as L
from coevonet_amd.deepqn import DeepQN, DeepQNHalf
from coevonet_amd.dqn_population import half_values
from coevonet_amd.game_logic import _play_atari_aec, initialize_env, play_game
from coevonet_amd.population import N_EVAL, ROLES2, mean_eval
from tests import dqn_edge_nets as E
from tests import duel_cases as dc
from tests.util import Bag

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 32
ERR_ARG = -1
OWN = L.K_DUEL["COEVO_DUEL_CREDIT_OWN"]
SW = ad.STATE_WORDS


@pytest.fixture(scope="module", autouse=True)
def release_nets():
    yield
    E.release()


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def rc(name, *args):
    """the entry point's return code (no exception)"""
    return getattr(L.load(), name)(*args, L._stream())


class DuelDevice:
    """game state (77 everywhere), returns (5.5) and frame rows (0xA5), each between guards of the same fill"""

    def __init__(self, G, n_rows, C):
        self.G, self.R, self.nbytes = G, n_rows, 84 * 84 * C
        self.state = torch.full((SW * G + 2 * PAD,), dc.FILL_STATE, dtype=torch.int32, device=DEV)
        self.acc = torch.full((3 * G + 2 * PAD,), dc.FILL_ACC, dtype=torch.float64, device=DEV)
        self.frames = torch.full((n_rows + 2, self.nbytes), dc.POISON, dtype=torch.uint8, device=DEV)
        self.state_p, self.acc_p = self.state[PAD:].data_ptr(), self.acc[PAD:].data_ptr()
        self.frames_p = self.frames[1:].data_ptr()
        assert self.frames_p % 16 == 0

    def poke(self, words):
        self.state[PAD:PAD + SW * self.G].copy_(dev(np.ascontiguousarray(words, dtype=np.int32).reshape(-1)))

    def read(self):
        torch.cuda.synchronize()
        s, a, f = self.state.cpu().numpy(), self.acc.cpu().numpy(), self.frames.cpu().numpy()
        assert (s[:PAD] == dc.FILL_STATE).all() and (s[-PAD:] == dc.FILL_STATE).all(), "a state guard word was written"
        assert (a[:PAD] == dc.FILL_ACC).all() and (a[-PAD:] == dc.FILL_ACC).all(), "a guard word of the returns was written"
        assert (f[0] == dc.POISON).all() and (f[-1] == dc.POISON).all(), "a guard frame row was written"
        return s[PAD:-PAD].reshape(self.G, SW), a[PAD:-PAD].reshape(self.G, 3), f[1:-1]


def launch_and_compare(d, ref, t, row_prev, actions, row_cur, d_ord0, d_gen, per_gen, d_lim, C, n_act, seed, points, flags,
                       frames=True):
    """one coevo_duel_step on the device and in DuelRef; every state word, return bit and frame byte compared"""
    want_frames = np.full((d.R, 84, 84, C), dc.POISON, dtype=np.uint8)
    rendered = ref.step(t, row_prev, actions, row_cur, want_frames if frames else None)
    d.frames.fill_(dc.POISON)
    d_prev, d_act = (dev(np.asarray(row_prev, dtype=np.int32)), dev(np.asarray(actions, dtype=np.int32))) if t else (None, None)
    d_cur = dev(np.asarray(row_cur, dtype=np.int32))
    L.call("coevo_duel_step", d.state_p, d.acc_p, d.G, L._p(d_ord0), L._p(d_gen), per_gen, t, L._p(d_lim), L._p(d_prev),
           L._p(d_act), L._p(d_cur), d.frames_p if frames else None, C, n_act, seed, points, flags)
    state, acc, got = d.read()
    assert np.array_equal(state, ref.state), (t, state.tolist(), ref.state.tolist())
    assert np.array_equal(acc.view(np.uint64), ref.acc.view(np.uint64)), (t, acc.tolist(), ref.acc.tolist())
    for r in range(d.R):
        assert np.array_equal(got[r], want_frames[r].reshape(-1)), (t, r, r in rendered)
        assert (r in rendered) or (got[r] == dc.POISON).all()
    return rendered


# ------------------------------------------------------------------------------------------- 1. the step kernel alone
@pytest.mark.parametrize("n_act", [6, 18])
@pytest.mark.parametrize("C", [4, 6])
@pytest.mark.parametrize("G", [1, 2, 7])
def test_duel_steps_vs_numpy(G, C, n_act):
    """T = 9 launches with random action words (-1, n_actions and 255 among them) over G games: limits 0, 1, 2, T - 1, T side by
    side, a disabled game, ordinals 0 and 2^63 - 1 (and one moved by the generation word), seeds 0 / 2^64 - 1 / the reference's,
    frame rows permuted anew at every step, credit flag by case; one game is poked one world step from a plane so that hits,
    points and serves are booked"""
    T = 9
    seed = (0, 2 ** 64 - 1, dc.SEED)[(G + C + n_act) % 3]
    own = (G + n_act // 6) % 2
    per_gen, gen = 5, 2
    ord0 = np.array([2 ** 63 - 1 - gen * per_gen, -gen * per_gen, 7, -1 - gen * per_gen, 1, 2 ** 40, 3][:G], dtype=np.int64)
    lim = np.array([T, T - 1, 2, T, 0, 1, T][:G], dtype=np.int32)      # (game 3 is disabled: ordinal -1)
    R = G + 2
    d = DuelDevice(G, R, C)
    ref = dc.DuelRef(ord0, lim, gen, per_gen, C, n_act, seed, points=2, own=bool(own))
    assert ref.ordinal[0] == 2 ** 63 - 1 and (G < 2 or ref.ordinal[1] == 0) and (G < 4 or ref.ordinal[3] == -1)
    d_ord0, d_lim, d_gen = dev(ord0), dev(lim), dev(np.array([gen], dtype=np.int32))
    rng = np.random.default_rng([G, C, n_act])
    pool = np.array(list(range(n_act)) + [-1, n_act, 255], dtype=np.int32)
    booked = rendered = 0
    for t in range(T + 1):
        rows = lambda s: np.array([(2 * g + s) % R for g in range(G)], dtype=np.int32)      # (2 and R = 3, 4, 9: distinct rows)
        row_cur, row_prev = rows(t), rows(t - 1)
        assert len(set(row_cur.tolist())) == G
        actions = np.full(R, -9, dtype=np.int32)
        if t:
            actions[row_prev] = rng.choice(pool, size=G)
        before = ref.acc.copy()
        rendered += len(launch_and_compare(d, ref, t, row_prev if t else None, actions, row_cur, d_ord0, d_gen, per_gen, d_lim, C,
                                           n_act, seed, 2, OWN if own else 0, frames=t < T))
        booked += int((ref.acc != before).any()) if t else 0
        if t == 0:      # game 0: the ball two world steps from the left plane, the paddle far away -> a point, then serve 1
            ref.poke(0, bx=11, by=70, vx=-3, vy=0, p0=0)
            d.poke(ref.state)
    assert rendered >= T and ref.games[0].score[1] >= 1 and booked >= 1
    if G == 7:
        assert [g.t for g in ref.games] == [T, T - 1, 2, 0, 0, 1, T] or ref.games[0].ended or ref.games[6].ended


def test_crafted_states_on_the_device():
    """every crafted state of tests/duel_cases.crafted() as one game of one launch chain: reset, poke, first_0's step, second_0's
    step and the world step - walls for every |vy|, all 13 hit offsets and the nearest misses on both sides, wall and plane in
    one step, paddles pushed outward"""
    cases = dc.crafted()
    G, C, n_act = len(cases), 4, 6
    d = DuelDevice(G, G, C)
    ord0, lim = np.full(G, 3, dtype=np.int64), np.full(G, 100, dtype=np.int32)
    ref = dc.DuelRef(ord0, lim, None, 0, C, n_act, dc.SEED)
    d_ord0, d_lim = dev(ord0), dev(lim)
    rows = np.arange(G, dtype=np.int32)[::-1].copy()
    common = (d_ord0, None, 0, d_lim, C, n_act, dc.SEED, 21, 0)
    launch_and_compare(d, ref, 0, None, None, rows, *common)
    for g, (_, words, _, _) in enumerate(cases):
        ref.poke(g, **words)
    d.poke(ref.state)
    for t in (1, 2):
        actions = np.zeros(G, dtype=np.int32)
        actions[rows] = [c[2][t - 1] for c in cases]
        launch_and_compare(d, ref, t, rows, actions, rows, *common)
    for g, (name, _, _, want) in enumerate(cases):      # (the numpy side of these is proven in tests/test_duel_cpu.py)
        gm = ref.games[g]
        got = dict(bx=gm.bx, by=gm.by, vx=gm.vx, vy=gm.vy, p0=gm.p[0], p1=gm.p[1], score0=gm.score[0], score1=gm.score[1])
        assert all(got[k] == v for k, v in want.items()) or "score0" in want or "score1" in want, (name, got)


@pytest.mark.parametrize("C,own", [(4, 0), (6, 1)])
def test_the_point_that_ends_a_game(C, own):
    """points_to_win = 1: the launch that books the deciding point writes the state and the returns and renders nothing; two
    more launches book nothing and write no frame byte; the game beside it plays on"""
    n_act, G = 6, 2
    d = DuelDevice(G, 3, C)
    ord0, lim = np.array([4, 5], dtype=np.int64), np.array([20, 20], dtype=np.int32)
    ref = dc.DuelRef(ord0, lim, None, 0, C, n_act, dc.SEED, points=1, own=bool(own))
    common = (dev(ord0), None, 0, dev(lim), C, n_act, dc.SEED, 1, OWN if own else 0)
    rows = np.array([2, 0], dtype=np.int32)
    launch_and_compare(d, ref, 0, None, None, rows, *common)
    ref.poke(0, bx=74, by=10, vx=3, vy=0, p1=60)      # reaches the right plane in the next world step, far from the paddle
    d.poke(ref.state)
    for t in range(1, 7):
        actions = np.array([1, -9, 0], dtype=np.int32)
        before = (ref.state[0].copy(), ref.acc[0].copy())
        rendered = launch_and_compare(d, ref, t, rows, actions, rows, *common)
        if t == 2:
            assert ref.games[0].ended == 2 and ref.games[0].score == [1, 0] and ref.state[0, 11] == 2
            assert ref.acc[0].tolist() == ([0.0, -1.0, 0.0] if own else [0.0, 1.0, 0.0])
        if t >= 2:
            assert rendered == [0]                      # game 1's row alone
        if t >= 3:
            assert np.array_equal(ref.state[0], before[0]) and np.array_equal(ref.acc[0], before[1])
    assert not ref.games[1].ended and ref.games[1].t == 6


def test_largest_step_and_refusals_write_nothing():
    """t = 65535 is served; t = 65536, a flag bit other than COEVO_DUEL_CREDIT_OWN, C = 5 and NULL pointers are COEVO_ERR_ARG with
    no word, return or frame byte written"""
    C, n_act, t = 4, 18, 65535
    d = DuelDevice(2, 3, C)
    ord0, lim = np.array([7, 2 ** 33 + 1], dtype=np.int64), np.array([65536, 65535], dtype=np.int32)
    ref = dc.DuelRef(ord0, lim, None, 0, C, n_act, dc.SEED)
    d_ord0, d_lim = dev(ord0), dev(lim)
    rows_prev, rows_cur = np.array([2, 0], dtype=np.int32), np.array([1, 2], dtype=np.int32)
    actions = np.array([3, -9, 2], dtype=np.int32)
    launch_and_compare(d, ref, 0, None, None, rows_cur, d_ord0, None, 0, d_lim, C, n_act, dc.SEED, 21, 0)
    state0 = ref.state.copy()
    d.frames.fill_(dc.POISON)
    d_prev, d_act, d_cur = dev(rows_prev), dev(actions), dev(rows_cur)
    args = [d.state_p, d.acc_p, 2, L._p(d_ord0), None, 0, t, L._p(d_lim), L._p(d_prev), L._p(d_act), L._p(d_cur), d.frames_p, C,
            n_act, dc.SEED, 21, 0]
    at = dict(state=0, acc=1, n_games=2, ord0=3, t=6, limit=7, row_prev=8, actions=9, row_cur=10, frames=11, C=12, n_act=13,
              points=15, flags=16)

    def refused(**kw):
        a = list(args)
        for k, v in kw.items():
            a[at[k]] = v
        return rc("coevo_duel_step", *a)
    for bad in (dict(t=65536), dict(t=-1), dict(flags=2), dict(flags=3), dict(flags=4), dict(C=5), dict(C=3), dict(C=7),
                dict(n_act=0), dict(n_act=33), dict(points=0), dict(state=None), dict(acc=None), dict(ord0=None), dict(limit=None),
                dict(row_prev=None), dict(actions=None), dict(row_cur=None), dict(n_games=0), dict(frames=d.frames_p + 4)):
        assert refused(**bad) == ERR_ARG, bad
    state, acc, frames = d.read()
    assert np.array_equal(state, state0) and not acc.any() and (frames == dc.POISON).all(), "a refused call wrote"
    want_frames = np.full((3, 84, 84, C), dc.POISON, dtype=np.uint8)
    assert ref.step(t, rows_prev, actions, rows_cur, want_frames) == [1]      # game 1 has reached its limit: booked, no frame
    L.call("coevo_duel_step", *args)
    state, acc, frames = d.read()
    assert np.array_equal(state, ref.state) and np.array_equal(acc.view(np.uint64), ref.acc.view(np.uint64))
    assert np.array_equal(frames, want_frames.reshape(3, -1))
    assert ref.state[0, 0] == 2 and ref.state[1, 0] == 3 and (ref.state[:, 5:7] == 36).all()      # step 65534 is first_0's: held


# ------------------------------------------------------------------------------------------- 2. fused = unfused
SENT_A = -7


def play_twin(half, fused, nan_live):
    """3 games over 2 nets (plain, all-NaN logits), T = 6, points_to_win = 1: game 0 (plain, plain) plays on, game 1 (plain,
    plain) is poked so that it ends at agent-step 3, game 2 (NaN, NaN) is live or - not nan_live - poked as ended from the start.
    fused: the hidden forward + the out_duel_step launch; else the argmax forward + coevo_duel_step.  -> dict of every buffer"""
    from coevonet_amd.duel_rollout import DuelRollout, HalfDuelRollout
    C, n, T, lib = 4, 6, 6, L.load()
    nets = [E.make("plain", C, n), E.make("all_nan_logits", C, n)]
    if half:
        nets = [half_values(w) for w in nets]
    sym = "coevo_dqn16" if half else "coevo_dqn"
    stride = int(getattr(lib, sym + "_slab_stride")(C, n))
    slab = torch.zeros(2 * stride, dtype=torch.int32 if half else torch.float32, device=DEV)
    L.call(sym + "_pack", L._p(dev(np.stack(nets))), L._p(slab), 2, C, n)
    ro = (HalfDuelRollout if half else DuelRollout)([(0, 0), (0, 0), (1, 1)], [0, stride], [3, 4, 5], C, n, slab, dc.SEED, 0, DEV,
                                                    points_to_win=1, credit="next")
    ro.set_limits([T, T, T])
    ln = ro.lanes[0]
    ln["actions"].fill_(SENT_A)
    stream = torch.cuda.current_stream().cuda_stream
    env = lambda t: (L._p(ro.dstate), L._p(ro.acc), 3, L._p(ro.ordinal0), None, 0, t, L._p(ro.limit),
                     L._p(ln["rows"][(t - 1) & 1]) if t else None, ln["actions"][(t - 1) & 1].data_ptr() if t else None,
                     L._p(ln["rows"][t & 1]) if t < T else None, L._p(ln["frames"]) if t < T else None, C, n, dc.SEED, 1, 0)
    live_actions = []
    for t in range(T + 1):
        p, q = t & 1, (t - 1) & 1
        if half:
            ro.fused_out = fused
            ro.enqueue_step(ln, t, T, None, stream)
        else:
            fwd = (L._p(slab), L._p(ln["tasks"][p]), ln["n_tasks"][p], ln["max_rows"][p], 3, ro.Cw, n, L._p(ln["frames"]))
            if t and fused:
                L._check(lib.coevo_dqn_out_duel_step(*env(t), L._p(slab), L._p(ln["tasks"][q]), ln["n_tasks"][q], 3, L._p(ln["ws"]),
                                                     L._p(ro.status), stream), "coevo_dqn_out_duel_step")
            else:
                L._check(lib.coevo_duel_step(*env(t), stream), "coevo_duel_step")
            if t < T and fused:
                L._check(lib.coevo_dqn_forward_hidden_timed(*fwd, L._p(ln["ws"]), None, 0, stream), "hidden")
            elif t < T:
                L._check(lib.coevo_dqn_forward_argmax(*fwd, ln["actions"][p].data_ptr(), None, L._p(ro.status), L._p(ln["ws"]),
                                                      stream), "argmax")
        torch.cuda.synchronize()
        state = ro.dstate.cpu().numpy()
        if t == 0:
            state[1, 1:7] = [11, 70, -3, 0, 0, 36]      # two world steps from the left plane, the paddle out of reach
            if not nan_live:
                state[2, 11] = 1
            ro.dstate.copy_(dev(state))
        else:   # the action words of the games that were live at step t - 1, as booked
            rows = ln["rows"][q].cpu().numpy()
            acts = ln["actions"][q].cpu().numpy()
            live_actions.append([int(acts[rows[g]]) if live[g] else None for g in range(3)])
        live = [not state[g, 11] for g in range(3)]
    out = dict(state=ro.dstate.cpu().numpy(), acc=ro.acc.cpu().numpy(), frames=ln["frames"].cpu().numpy(),
               status=int(ro.status.item()), live_actions=live_actions, actions=ln["actions"].cpu().numpy(),
               rows=[r.cpu().numpy() for r in ln["rows"]])
    ro.close()
    return out


@pytest.mark.parametrize("half", [False, True], ids=["float32", "float16"])
def test_fused_launch_equals_the_separate_pair(half):
    """every buffer equal; the status word differs only where the header says: a net without an action in a game that has ENDED
    raises COEVO_ST_NO_ACTION in the separate pair (its forward computes every row) and nothing in the fused launch (the row of
    a finished game is not evaluated, its action word keeps what it held); the same net in a live game raises the bit in both"""
    for nan_live, want_status in ((False, (E.NO_ACTION, 0)), (True, (E.NO_ACTION, E.NO_ACTION))):
        A, B = play_twin(half, False, nan_live), play_twin(half, True, nan_live)
        assert np.array_equal(A["state"], B["state"]) and np.array_equal(A["acc"].view(np.uint64), B["acc"].view(np.uint64))
        assert np.array_equal(A["frames"], B["frames"]) and A["live_actions"] == B["live_actions"]
        assert (A["status"], B["status"]) == want_status
        s = B["state"]
        assert s[0, 11] == 0 and s[1, 11] == 4 and s[1, 8] == 1 and s[2, 11] == (0 if nan_live else 1)
        assert B["acc"][1].tolist() == [0.0, -1.0, 0.0]      # "next": second_0 books cum0 = -1 at step 3; first_0 never collects
        rows = B["rows"]
        if not nan_live:    # never evaluated in the fused launch; the separate pair stores action 0 for the faulted rows
            assert B["actions"][0][rows[0][2]] == SENT_A == B["actions"][1][rows[1][2]]
            assert A["actions"][0][rows[0][2]] == 0 == A["actions"][1][rows[1][2]]
        else:
            assert all(la[2] == 0 for la in B["live_actions"])      # the faulted rows play action 0 in both


# ------------------------------------------------------------------------------------------- 3. whole games
def _players(half, C, n, seed):
    torch.manual_seed(seed)
    cls = DeepQNHalf if half else DeepQN
    return cls(C, n, "float16" if half else "float32"), cls(C, n, "float16" if half else "float32")


@pytest.mark.parametrize("credit", ["next", "own"])
@pytest.mark.parametrize("game,C", [("pong_v3", 4), ("boxing_v2", 6)])
@pytest.mark.parametrize("half", [False, True], ids=["float32", "float16"])
def test_play_game_device_equals_host_loop(half, game, C, credit):
    """play_game on the device = play_game through _play_atari_aec (args.coevo_host_aec) on two DuelAECs: equal returns and
    equal env objects afterwards, for T = 1, 2, 3, 30, 61 and 200, training and evaluation limits"""
    n = ad.ATARI_GAMES[game]
    a, b = _players(half, C, n, 21)
    seen = 0.0
    for ordinal, T in [(1, 1), (2, 2), (3, 3), (4, 30), (5, 61), (6, 200)]:      # (200: long enough for points with any nets)
        envs = [dc.env_at(ordinal, game=game, channels=C, points_to_win=2, credit=credit) for _ in range(2)]
        ev = T == 3
        kw = dict(game=game, max_timesteps_per_episode=None if ev else T, max_evaluation_steps=T if ev else 1)
        got = play_game(env=envs[0], player1=a, player2=b, args=Bag(**kw), eval=ev)
        host = play_game(env=envs[1], player1=a, player2=b, args=Bag(coevo_host_aec=True, **kw), eval=ev)
        assert tuple(got) == tuple(host), (T, got, host)
        assert envs[0].snapshot() == envs[1].snapshot() and envs[0].last() == envs[1].last(), T
        assert envs[0].ordinal == ordinal and envs[0].n_resets == ordinal + 1
        assert np.array_equal(envs[0].observe("first_0"), envs[1].observe("first_0"))
        seen += abs(host[0]) + abs(host[1])
    assert seen > 0      # some point was booked


def test_play_game_device_equals_the_oracle_forward_and_a_tracker_plays_the_host_loop():
    C, n, T = 4, 6, 30
    a, b = _players(False, C, n, 22)
    env_d, env_o = dc.env_at(9, channels=C), dc.env_at(9, channels=C)
    args = Bag(game="pong_v3", max_timesteps_per_episode=T)
    got = play_game(env=env_d, player1=a, player2=b, args=args)
    env_o.reset()
    want = _play_atari_aec(env_o, dc.OraclePlayer(a.flat(), C, n), dc.OraclePlayer(b.flat(), C, n), args, False)
    assert tuple(got) == tuple(want) and env_d.snapshot() == env_o.snapshot()
    # a scripted seat: the pair is not two nets of one kind, so play_game walks the host loop
    env_t = dc.env_at(9, channels=C, credit="own")
    r = play_game(env=env_t, player1=ad.DuelTracker(0), player2=b, args=Bag(game="pong_v3", max_timesteps_per_episode=120))
    assert env_t.t == 120 and env_t.state.score[1] == 0 and r[0] >= 0 and r[1] <= 0      # the tracker never concedes


# ------------------------------------------------------------------------------------------- 4. engines and trainers
def _replay(jobs, half, C, n, T, points, credit):
    """jobs: [(flat of first_0, flat of second_0, ordinal)] -> [(first_0, second_0) returns] through the host loop"""
    def one(job):
        f0, f1, ordinal = job
        env = dc.env_at(ordinal, channels=C, points_to_win=points, credit=credit)
        env.reset()
        if half:
            p0, p1 = DeepQNHalf(C, n), DeepQNHalf(C, n)
            p0.set_flat(f0)
            p1.set_flat(f1)
        else:
            p0, p1 = dc.OraclePlayer(f0, C, n), dc.OraclePlayer(f1, C, n)
        return _play_atari_aec(env, p0, p1, Bag(game="pong_v3", max_timesteps_per_episode=T), False)
    if half:      # (device forwards: one at a time)
        return [one(j) for j in jobs]
    with ThreadPoolExecutor(8) as ex:     # the oracle's C forward releases the interpreter lock
        return list(ex.map(one, jobs))


def _initial(pop, hof, C, n, half, seed):
    from coevonet_amd.dqn_population import dqn_initial_population
    torch.manual_seed(seed)
    pop_flat, hof_flat = dqn_initial_population(pop, hof, C, n)
    if half:
        pop_flat, hof_flat = ({r: half_values(f[r]) for r in ROLES2} for f in (pop_flat, hof_flat))
    return pop_flat, hof_flat


@pytest.mark.parametrize("credit", ["next", "own"])
@pytest.mark.parametrize("half", [False, True], ids=["float32", "float16"])
def test_ga_engine_over_the_duel_against_a_host_replay(half, credit):
    """two generations at pop 3 / HoF 1 / elites 1 / T 30 / C 4: before each step the nets that will play are downloaded, after
    it every game of the engine's table (the evaluation games of the previous generation included) is replayed on the host"""
    from coevonet_amd.dqn_ga_half import HalfDQNGAEngine
    from coevonet_amd.dqn_population import DQNGAEngine
    pop, hof, C, n, T, points, first = 3, 1, 4, 6, 30, 3, 1
    eng = (HalfDQNGAEngine if half else DQNGAEngine)(pop, hof, 1, C, n, T, T, first_ordinal=first, env="duel", duel_points=points,
                                                      duel_credit=credit)
    eng.load_initial(*_initial(pop, hof, C, n, half, 31))
    M, per_gen = 2 * pop * hof, 2 * pop * hof + N_EVAL
    assert eng.per_gen == per_gen and eng.n_main == M and type(eng.ro).__name__ == ("HalfDuelRollout" if half else "DuelRollout")
    for gen in range(2):
        nets = {r: {reg: eng.download(r, reg, 0, k) for reg, k in (("pop", pop), ("hof", hof))} for r in ROLES2}
        eng.step(use_graph=bool(gen))
        torch.cuda.synchronize()
        L.raise_on_status(eng.ro.status)
        got = eng.ro.acc.cpu().numpy()
        jobs = []
        for ph in range(2):
            for i in range(pop):
                for k in range(hof):
                    me, opp = nets[ROLES2[ph]]["pop"][i], nets[ROLES2[1 - ph]]["hof"][hof - 1 - k]
                    jobs.append((me, opp, first + gen * per_gen + ph * pop * hof + i * hof + k) if ph == 0 else
                                (opp, me, first + gen * per_gen + ph * pop * hof + i * hof + k))
        if gen:     # the evaluation games of generation gen - 1: its newest Hall-of-Fame pair, behind that generation's main games
            jobs += [(nets["first_0"]["hof"][hof - 1], nets["second_0"]["hof"][hof - 1], first + (gen - 1) * per_gen + M + j)
                     for j in range(N_EVAL)]
        want = _replay(jobs, half, C, n, T, points, credit)
        assert sum(1 for w in want[:M] if w[0] or w[1]) * 4 >= M, want      # (not vacuous: a quarter of the games score)
        for g, w in enumerate(want):
            assert tuple(got[g, :2]) == tuple(w), (gen, g, got[g].tolist(), w)
        if not gen:
            assert not got[M:].any()
    eng.close()


@pytest.mark.parametrize("half", [False, True], ids=["float32", "float16"])
def test_es_engine_over_the_duel_against_a_host_replay(half):
    from coevonet_amd.dqn_es_half import HalfDQNESEngine
    from coevonet_amd.dqn_population import DQNESEngine, dqn_init_flat
    pop, C, n, T, points, first, credit = 4, 4, 6, 30, 3, 1, "own"
    eng = (HalfDQNESEngine if half else DQNESEngine)(pop, C, n, T, T, first_ordinal=first, env="duel", duel_points=points,
                                                      duel_credit=credit)
    torch.manual_seed(32)
    for r in ROLES2:
        w = dqn_init_flat(C, n)
        eng.upload(r, "base", 0, (half_values(w) if half else w)[None])
    per_gen = 2 * pop + N_EVAL
    assert eng.per_gen == per_gen and type(eng.ro).__name__ == type(eng.eval_ro).__name__ == ("HalfDuelRollout" if half else "DuelRollout")
    for gen in range(2):
        base = {r: eng.download(r, "base", 0, 1)[0] for r in ROLES2}
        means = eng.generation(gen, (0.05, 0.08), 0.1, False)
        pert = {r: eng.download(r, "pert", 0, pop) for r in ROLES2}     # this generation's perturbed nets are still in the slab
        new_base = {r: eng.download(r, "base", 0, 1)[0] for r in ROLES2}
        got, got_eval = eng.ro.acc.cpu().numpy(), eng.eval_ro.acc.cpu().numpy()
        jobs = []
        for j in range(pop):
            jobs.append((pert["first_0"][j], base["second_0"], first + gen * per_gen + 2 * j))
            jobs.append((base["first_0"], pert["second_0"][j], first + gen * per_gen + 2 * j + 1))
        jobs += [(new_base["first_0"], new_base["second_0"], first + gen * per_gen + 2 * pop + j) for j in range(N_EVAL)]
        want = _replay(jobs, half, C, n, T, points, credit)
        assert sum(1 for w in want[:2 * pop] if w[0] or w[1]) * 4 >= 2 * pop, want
        for g, w in enumerate(want[:2 * pop]):
            assert tuple(got[g, :2]) == tuple(w), (gen, g, got[g].tolist(), w)
        for j, w in enumerate(want[2 * pop:]):
            assert tuple(got_eval[j, :2]) == tuple(w), (gen, j, got_eval[j].tolist(), w)
        assert list(means) == mean_eval(np.array(want[2 * pop:]), 2)
    eng.ro.close()
    eng.eval_ro.close()


@pytest.mark.parametrize("precision", ["float32", "float16"])
def test_ga_trainer_over_the_duel_graph_on_and_off(precision):
    from coevonet_amd import genetic_algorithm as ga
    runs = []
    for graph in (True, False):
        torch.manual_seed(33)
        args = Bag(algorithm="GA", game="pong_v3", generations=2, population=3, hof_size=1, elites_number=1, precision=precision,
                   max_timesteps_per_episode=30, max_evaluation_steps=30, coevo_atari_env="duel", coevo_duel_points=3,
                   coevo_graph=graph)
        env = initialize_env(args)
        assert type(env) is ad.DuelAEC
        res = ga.genetic_algorithm_train(env, env.agents[0], args, None)
        assert type(res.engine.ro).__name__ == ("HalfDuelRollout" if precision == "float16" else "DuelRollout")
        assert env.n_resets == 1 + 2 * (2 * 3 + N_EVAL)
        runs.append((np.stack(res.game_rewards), res.rewards, res.elite_ids))
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] and runs[0][2] == runs[1][2]
    assert np.count_nonzero(runs[0][0].any(axis=2)) * 4 >= runs[0][0].shape[0] * runs[0][0].shape[1]


@pytest.mark.parametrize("precision", ["float32", "float16"])
def test_es_trainer_over_the_duel_graph_on_and_off(precision, monkeypatch):
    from coevonet_amd import evolutionary_strategy as es
    runs = []
    for graph in ("1", "0"):
        monkeypatch.setenv("COEVO_DQN_EVAL_GRAPH", graph)
        torch.manual_seed(34)
        args = Bag(algorithm="ES", game="boxing_v2", generations=2, population=4, learning_rate=0.1, precision=precision,
                   max_timesteps_per_episode=30, max_evaluation_steps=30, coevo_atari_env="duel", coevo_duel_points=3,
                   coevo_channels=6, coevo_duel_credit="own")
        env = initialize_env(args)
        base, res = es.evolution_strategy_train(env, args, None)
        assert type(res.engine.ro).__name__ == ("HalfDuelRollout" if precision == "float16" else "DuelRollout")
        runs.append((np.stack(res.game_rewards), res.rewards, [np.asarray(b).copy() for b in base]))
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(runs[0][2], runs[1][2]))
    assert np.count_nonzero(runs[0][0].any(axis=2)) * 4 >= runs[0][0].shape[0] * runs[0][0].shape[1]
