"""The fused float16 env step on the GPU, equalities only: coevo_dqn16_forward_hidden + coevo_dqn16_out_synth_step against the
unfused pair coevo_dqn16_forward_argmax + coevo_synth_step (words of acc, game state, status, frames, the actions of live
rows) and against the CPU restatement (tests/dqn16_checker.py, tests/dqn_ga16_checker.play_game): two HalfSynthRollouts on one
slab - the three-launch route and COEVO_DQN16_FUSED_OUT=0 -, ragged tasks, the widest shape, the edges of the output row on a
hand-made output layer (a tie made by the fp16 rounding, NaN, -inf, a task the forward cannot serve) and every bad argument."""
import functools

import numpy as np
import pytest
import torch

from coevonet_amd import lib as L
from coevonet_amd.dqn_ga_half import HalfSynthRollout
from oracle import ref_port as rp
from tests import dqn16_checker as ck
from tests import dqn_ga16_checker as dk

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 0x5EAD                      # the poison of an actions word: no action
ERR_ARG = -1
ST_NO_ACTION, ST_BAD_TASK = 16, 64
SHAPES = ((4, 6), (3, 18))
ENV_SEED = {(4, 6): 124, (3, 18): 123}   # chosen on the CPU: a hit is credited in the five-game table (test below asserts it)


def stride16(C, n):
    return int(L.load().coevo_dqn16_slab_stride(C, n))


def pack16(flats, C, n):
    flats = np.ascontiguousarray(np.stack(flats), dtype=np.float32)
    slab = torch.zeros(len(flats) * stride16(C, n), dtype=torch.int32, device=DEV)
    L.call("coevo_dqn16_pack", L._p(torch.from_numpy(flats).to(DEV)), L._p(slab), len(flats), C, n)
    return slab


@functools.lru_cache(maxsize=None)
def nets_of(C, n, count=4):
    """generic fp16-valued nets: one initial net per index after a mutation of every parameter"""
    torch.manual_seed(300 + C + n)
    return tuple(dk.mutate(dk.to_half(rp.dqn_init(C, n)[0]), C, n, 0.02, 91, i, 0) for i in range(count))


def snapshot(ro):
    torch.cuda.synchronize()
    ln = ro.lanes[0]
    return dict(acc=ro.acc.cpu().numpy().view(np.uint64).copy(), gstate=ro.gstate.cpu().numpy().copy(), status=int(ro.status.item()),
                frames=ln["frames"].cpu().numpy().copy(), actions=ln["actions"].cpu().numpy().copy())


def rollout_pair(monkeypatch, game_nets, nets, ordinals, limits, C, n, env_seed):
    """the fused and the four-launch rollout over ONE slab -> {True: fused, False: unfused}"""
    slab = pack16(nets, C, n)
    net_off = [i * stride16(C, n) for i in range(len(nets))]
    ros = {}
    for fused, value in ((True, None), (False, "0")):
        if value is None:
            monkeypatch.delenv("COEVO_DQN16_FUSED_OUT", raising=False)   # the default is the fused route
        else:
            monkeypatch.setenv("COEVO_DQN16_FUSED_OUT", value)
        ro = ros[fused] = HalfSynthRollout(game_nets, net_off, ordinals, C, n, slab, env_seed, 0, DEV)
        assert ro.fused_out is fused
        ro.set_limits(np.asarray(limits, dtype=np.int32))
    return ros


def play(ro, T):
    """T agent-steps from poisoned scratch -> snapshot"""
    ln = ro.lanes[0]
    ln["actions"].fill_(SENT)
    ln["frames"].fill_(0xAB)
    ln["ws"].fill_(float("nan"))
    ro.gstate.fill_(77)
    ro.acc.fill_(5.5)
    ro.enqueue(T, None)
    return snapshot(ro)


def last_step(parity, T):
    """the last agent-step below T in which the player of `parity` acts (-1: none)"""
    return T - 1 if (T - 1) % 2 == parity else T - 2


def assert_equal_effects(F, U, live, what, same_status=True):
    assert np.array_equal(F["acc"], U["acc"]), (what, "acc")
    assert np.array_equal(F["gstate"], U["gstate"]), (what, "game state")
    assert F["status"] == U["status"] or not same_status, (what, "status")
    assert np.array_equal(F["frames"], U["frames"]), (what, "frames")
    assert np.array_equal(F["actions"][live], U["actions"][live]), (what, "actions of live rows")


# ------------------------------------------------------------------------------------------------ five games, ragged tasks
FIVE_NETS = [(0, 3), (1, 3), (0, 3), (2, 3), (2, 3)]     # first_0: nets 0, 1, 0, 2, 2 -> tasks of 2, 1, 2 rows; second_0: net 3
T_FULL = 4
FIVE_LIMITS = (0, 1, 2, T_FULL, T_FULL)
FIVE_ORDINALS = (3, 4, 5, 1 << 33, -7)                   # the last game is disabled: a negative ordinal


@functools.lru_cache(maxsize=None)
def five_games_want(C, n, T):
    """checker: the reward pair of every game after T agent-steps (a finished or disabled game: what it had)"""
    nets = nets_of(C, n)
    out = []
    for (a, b), lim, o in zip(FIVE_NETS, FIVE_LIMITS, FIVE_ORDINALS):
        steps = min(lim, T) if o >= 0 else 0
        out.append(dk.play_game(nets[a], nets[b], C, n, ENV_SEED[(C, n)], o, steps) if steps else [0.0, 0.0])
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"C{s[0]}n{s[1]}")
def test_five_games_fused_equals_unfused_equals_the_checker(shape, monkeypatch):
    """Five games with limits (0, 1, 2, T, T), the second T-game disabled by a negative ordinal.  first_0 acts for three nets in
    tasks of 2, 1, 2 rows whose row_of_game is not the identity, second_0 in one 5-row task; T = 1, 2, 4 agent-steps."""
    C, n = shape
    ros = rollout_pair(monkeypatch, FIVE_NETS, nets_of(C, n), FIVE_ORDINALS, FIVE_LIMITS, C, n, ENV_SEED[shape])
    ln = ros[True].lanes[0]
    assert [int(t["n_rows"]) for t in ln["tasks_np"][0]] == [2, 1, 2] and [int(t["n_rows"]) for t in ln["tasks_np"][1]] == [5]
    rows = [ln["rows"][p].cpu().numpy() for p in range(2)]
    assert rows[0].tolist() == [0, 2, 1, 3, 4] and rows[1].tolist() == [0, 1, 2, 3, 4]
    lim, ordn = np.array(FIVE_LIMITS), np.array(FIVE_ORDINALS)
    for T in (1, 2, 4):
        F, U = play(ros[True], T), play(ros[False], T)
        live = np.zeros((2, 5), dtype=bool)      # [parity][row]: the row's last forward below T was booked
        never = np.zeros((2, 5), dtype=bool)     # [parity][row]: no forward of the row was ever booked
        for p in range(2):
            for g in range(5):
                live[p, rows[p][g]] = ordn[g] >= 0 and 0 <= last_step(p, T) < lim[g]
                never[p, rows[p][g]] = ordn[g] < 0 or min(lim[g], T) <= p
        assert_equal_effects(F, U, live, (shape, T))
        assert F["status"] == 0
        assert (F["actions"][never] == SENT).all(), "the fused route evaluated a finished or disabled game's row"
        assert (U["actions"][:min(T, 2)] != SENT).all(), "the unfused pair computes every row of a parity that acted"
        assert never[:, rows[0][0]].all() and never[:, 4].all() and never[1, rows[1][1]] and live.any()
        want = five_games_want(C, n, T)
        got = F["acc"].view(np.float64)[:, :2].tolist()
        assert got == want, (shape, T, "rewards differ from the checker")
        for g in (0, 4):    # never started: reset, or left alone
            assert F["gstate"][g][:2].tolist() == [0xFF, 0] and (F["frames"].reshape(5, -1)[rows[0][g]] == 0xAB).all()
    assert any(any(r) for r in five_games_want(C, n, T_FULL)), "no hit was credited: choose another env seed"


def test_seventeen_games_of_one_net_fused_equals_unfused(monkeypatch):
    """one net acts in every game of a parity: tasks of 16 + 1 rows (dqn16_fc1_body<4> and <1>, the row -> task search of the
    fused launch past the first task); one game finished after its first step, one disabled"""
    C, n, T = 4, 6, 2
    nets = nets_of(C, n)
    ordinals = [10 + g for g in range(17)]
    ordinals[5] = -1
    limits = [T] * 17
    limits[9] = 1
    ros = rollout_pair(monkeypatch, [(0, 1)] * 17, nets[:2], ordinals, limits, C, n, 321)
    assert [int(t["n_rows"]) for t in ros[True].lanes[0]["tasks_np"][0]] == [16, 1]
    F, U = play(ros[True], T), play(ros[False], T)
    live = np.ones((2, 17), dtype=bool)
    live[:, 5] = False
    live[1, 9] = False
    assert_equal_effects(F, U, live, "seventeen games")
    assert F["status"] == 0 and (F["actions"][~live] == SENT).all() and (F["actions"][live] != SENT).all()
    for g in (9, 16):   # the game in the one-row task, and the one that ends early, against the checker
        want = dk.play_game(nets[0], nets[1], C, n, 321, ordinals[g], limits[g])
        assert F["acc"].view(np.float64)[g, :2].tolist() == want


# ------------------------------------------------------------------------------------------------------------ direct calls
class Twins:
    """games = rows, one task per entry of `layout` [(net index, rows)].  coevo_synth_step(t = 0) writes the frames, then
    twin U: coevo_dqn16_forward_argmax + coevo_synth_step(t = 1); twin F, on copies: coevo_dqn16_forward_hidden +
    coevo_dqn16_out_synth_step(t = 1).  `preset`: the actions words before the forward"""

    def __init__(self, C, n, nets, layout, limits, ordinals, seed=0x5EED, preset=SENT, net_off_shift=None):
        lib = L.load()
        G = sum(r for _, r in layout)
        stride = stride16(C, n)
        tasks = np.zeros(len(layout), dtype=L.DQN_TASK_DTYPE)
        row = 0
        self.net_of_row = []
        for i, (k, r) in enumerate(layout):
            tasks[i] = (k * stride + (net_off_shift or {}).get(i, 0), row, r)
            self.net_of_row += [k] * r
            row += r
        slab = pack16(nets, C, n)
        d_tasks = L.tasks_to_device(tasks, DEV)
        rows = torch.arange(G, dtype=torch.int32, device=DEV)
        lim = torch.tensor(list(limits), dtype=torch.int32, device=DEV)
        ord0 = torch.tensor(list(ordinals), dtype=torch.int64, device=DEV)
        frames0 = torch.full((G * 84 * 84 * C,), 0xAB, dtype=torch.uint8, device=DEV)
        gstate0 = torch.full((G, 4), 77, dtype=torch.int32, device=DEV)
        acc0 = torch.full((G, 3), 5.5, dtype=torch.float64, device=DEV)
        L.call("coevo_synth_step", L._p(gstate0), L._p(acc0), G, L._p(ord0), None, 0, 0, L._p(lim), None, None, L._p(rows),
               L._p(frames0), C, n, seed)
        torch.cuda.synchronize()
        self.frames0 = frames0.cpu().numpy().reshape(G, 84, 84, C)
        self.out = {}
        for twin in "UF":
            gs, ac, fr = gstate0.clone(), acc0.clone(), frames0.clone()
            actions = torch.full((G,), preset, dtype=torch.int32, device=DEV)
            status = torch.zeros(1, dtype=torch.int32, device=DEV)
            ws = torch.full((int(lib.coevo_dqn16_workspace_bytes(G)) // 4,), float("nan"), dtype=torch.float32, device=DEV)
            if twin == "U":
                L.call("coevo_dqn16_forward_argmax", L._p(slab), L._p(d_tasks), len(layout), 16, G, C, n, L._p(fr),
                       L._p(actions), None, L._p(status), L._p(ws))
                L.call("coevo_synth_step", L._p(gs), L._p(ac), G, L._p(ord0), None, 0, 1, L._p(lim), L._p(rows), L._p(actions),
                       L._p(rows), L._p(fr), C, n, seed)
            else:
                L.call("coevo_dqn16_forward_hidden", L._p(slab), L._p(d_tasks), len(layout), 16, G, C, n, L._p(fr),
                       L._p(status), L._p(ws))
                L.call("coevo_dqn16_out_synth_step", L._p(gs), L._p(ac), G, L._p(ord0), None, 0, 1, L._p(lim), L._p(rows),
                       L._p(actions), L._p(rows), L._p(fr), C, n, seed, L._p(slab), L._p(d_tasks), len(layout), G, L._p(ws),
                       L._p(status))
            torch.cuda.synchronize()
            self.out[twin] = dict(actions=actions.cpu().numpy(), gstate=gs.cpu().numpy(), acc=ac.cpu().numpy().view(np.uint64),
                                  frames=fr.cpu().numpy(), status=int(status.item()))

    def agree(self, live, what, same_status=True):
        assert_equal_effects(self.out["F"], self.out["U"], live, what, same_status)
        return self.out["F"]


def test_widest_shape_fused_equals_unfused_and_the_checker():
    """n_actions = 32 (every lane of the output row's half wave that the ABI can ask for), C = 6: three games over two nets in
    tasks of 2 and 1 rows, the last game at its last step"""
    C, n, seed = 6, 32, 0x5EED
    nets = nets_of(C, n, 2)
    limits, ordinals = [3, 3, 1], [2, 3, 4]
    tw = Twins(C, n, nets, [(0, 2), (1, 1)], limits, ordinals, seed)
    F = tw.agree(np.ones(3, dtype=bool), "n = 32")
    assert F["status"] == 0
    for g in range(3):
        f0 = rp.synth_frame(seed, ordinals[g], 0, 0xFF, C)
        assert np.array_equal(tw.frames0[g], f0)
        a, _, st = ck.forward(nets[tw.net_of_row[g]], C, n, f0)
        assert st == 0 and F["actions"][g] == a == F["gstate"][g][0]
        want_next = rp.synth_frame(seed, ordinals[g], 1, a, C) if limits[g] > 1 else f0
        assert np.array_equal(F["frames"].reshape(3, 84, 84, C)[g], want_next)


# ---- a hand-made output layer on a real trunk
def out_slices(C, n):
    P = int(L.load().coevo_dqn_param_count(C, n))
    w0 = P - 320 - n - 512 * n
    return slice(w0, w0 + 512 * n), slice(w0 + 512 * n, w0 + 512 * n + n)


def with_output_layer(net, C, n, weight, bias):
    w_sl, b_sl = out_slices(C, n)
    out = net.copy()
    out[w_sl] = np.asarray(weight, dtype=np.float32).ravel()
    out[b_sl] = np.asarray(bias, dtype=np.float32)
    return out


@functools.lru_cache(maxsize=None)
def hidden_unit(C, n, seed, ordinal):
    """a hidden unit k of the trunk of nets_of(C, n)[0] on the frame of t = 0 with 0.25 <= hid[k] < 1024 and its value, read on
    the CPU through one-hot output rows (logit a = f16(0 + 1 * hid[k_a]) = hid[k_a], exact)"""
    net, f0 = nets_of(C, n)[0], rp.synth_frame(seed, ordinal, 0, 0xFF, C)
    for k0 in range(0, 512, n):
        w = np.zeros((n, 512), dtype=np.float32)
        for a in range(n):
            w[a, (k0 + a) % 512] = 1.0
        _, logits, st = ck.forward(with_output_layer(net, C, n, w, np.zeros(n)), C, n, f0)
        for a in np.flatnonzero((logits >= 0.25) & (logits < 1024.0)):
            return (k0 + int(a)) % 512, float(logits[a])
    raise AssertionError("no hidden unit in range")


EDGE_SEED, EDGE_ORD = 0x5EED, 3


def edge_nets(C, n):
    """-> {name: net}: the trunk of nets_of(C, n)[0] under four hand-made output layers over ONE hidden unit h = hid[k]:
    rounding_tie   logit 1 = f16(h), logit 2 = f16(fl32(h + 2^-14)) - the chain values differ, the higher index is larger, both
                   round to the fp16 word of h; every other logit is -1
    nan_beside     that tie at actions 3 and 4 (when n allows; else 1 and 2) with logit 0 NaN
    all_nan / all_neg_inf"""
    k, h = hidden_unit(C, n, EDGE_SEED, EDGE_ORD)
    eps = np.float32(2.0 ** -14)
    assert np.float32(h) + eps > np.float32(h) and np.float16(np.float32(h) + eps) == np.float16(h)   # differ, then one word
    base = nets_of(C, n)[0]

    def layer(lo, nan_at=None, bias_all=None):
        w, b = np.zeros((n, 512), dtype=np.float32), np.full(n, -1.0, dtype=np.float32)
        w[lo, k] = w[lo + 1, k] = 1.0
        b[lo], b[lo + 1] = 0.0, eps
        if nan_at is not None:
            w[nan_at, k] = np.nan
        if bias_all is not None:
            b[:] = bias_all
        return with_output_layer(base, C, n, w, b)
    return {"rounding_tie": layer(1), "nan_beside": layer(3, nan_at=0), "all_nan": layer(1, bias_all=np.nan),
            "all_neg_inf": layer(1, bias_all=-np.inf)}, (k, h)


def test_edges_of_the_output_row_on_a_hand_made_output_layer():
    C, n = 4, 6
    nets, (k, h) = edge_nets(C, n)
    names = list(nets)
    f0 = rp.synth_frame(EDGE_SEED, EDGE_ORD, 0, 0xFF, C)
    # the checker's view of the four rows: what makes them edges
    want = {}
    for name in names:
        a, logits, st = ck.forward(nets[name], C, n, f0)
        want[name] = (a, st)
        bits = logits.view(np.uint32)
        if name == "rounding_tie":
            assert bits[1] == bits[2] == np.float32(h).view(np.uint32) and (logits[[0, 3, 4, 5]] == -1).all() and (a, st) == (1, 0)
        if name == "nan_beside":
            assert np.isnan(logits[0]) and bits[3] == bits[4] and (a, st) == (3, 0)
        if name == "all_nan":
            assert np.isnan(logits).all() and (a, st) == (0, ST_NO_ACTION)
        if name == "all_neg_inf":
            assert (logits == -np.inf).all() and (a, st) == (0, ST_NO_ACTION)
    # every game sees the same frame: one ordinal, four nets, one row each; then the quiet rows alone (status stays 0)
    for cast in (names, names[:2]):
        tw = Twins(C, n, [nets[c] for c in cast], [(i, 1) for i in range(len(cast))], [3] * len(cast), [EDGE_ORD] * len(cast),
                   EDGE_SEED)
        F = tw.agree(np.ones(len(cast), dtype=bool), cast)
        assert F["actions"].tolist() == [want[c][0] for c in cast] == F["gstate"][:, 0].tolist()
        assert F["status"] == tw.out["U"]["status"] == (ST_NO_ACTION if len(cast) == 4 else 0)
    # a finished game's stale row is not evaluated: the NaN rows behind a reached limit raise nothing on the fused route
    tw = Twins(C, n, [nets[c] for c in names], [(i, 1) for i in range(4)], [3, 3, 0, 3], [EDGE_ORD] * 3 + [-2], EDGE_SEED)
    F = tw.agree(np.array([True, True, False, False]), "NaN rows in finished games", same_status=False)
    assert F["status"] == 0 and tw.out["U"]["status"] == ST_NO_ACTION and F["actions"].tolist()[2:] == [SENT, SENT]


def test_a_task_the_forward_cannot_serve_books_the_stale_action():
    """net_off & 3: fc1 raises COEVO_ST_BAD_TASK, nothing is loaded through the offset, no output row runs - the word the actions
    row already holds is booked, as the unfused pair books it"""
    C, n = 4, 6
    nets = nets_of(C, n)
    stale = int(rp.synth_target(0x5EED, 8, 0, n))    # the stale word scores in game 1: the booking is visible in acc
    tw = Twins(C, n, nets[:2], [(0, 1), (1, 2), (0, 1)], [3, 3, 3, 3], [7, 8, 9, 10], 0x5EED, preset=stale, net_off_shift={1: 2})
    F = tw.agree(np.ones(4, dtype=bool), "bad task")
    assert F["status"] == tw.out["U"]["status"] == ST_BAD_TASK
    assert F["actions"][1:3].tolist() == [stale, stale] == F["gstate"][1:3, 0].tolist()
    assert F["gstate"][1, 1] == 1 and F["acc"].view(np.float64)[1].tolist() == [-1.0, 0.0, 0.0]
    for g in (0, 3):
        a, _, st = ck.forward(nets[0], C, n, tw.frames0[g])
        assert st == 0 and F["actions"][g] == a


# ---------------------------------------------------------------------------------------------------------- bad arguments
def test_every_bad_argument_returns_err_arg_and_writes_nothing():
    C, n, G = 4, 6, 2
    lib, stride = L.load(), stride16(C, n)
    slab = pack16(nets_of(C, n)[:2], C, n)
    tasks = np.zeros(2, dtype=L.DQN_TASK_DTYPE)
    tasks[0], tasks[1] = (0, 0, 1), (stride, 1, 1)
    d_tasks = L.tasks_to_device(tasks, DEV)
    rows = torch.arange(G, dtype=torch.int32, device=DEV)
    lim = torch.full((G,), 3, dtype=torch.int32, device=DEV)
    ord0 = torch.tensor([1, 2], dtype=torch.int64, device=DEV)
    gen = torch.zeros(1, dtype=torch.int32, device=DEV)
    poison = dict(gs=torch.full((G, 4), 77, dtype=torch.int32, device=DEV), acc=torch.full((G, 3), 5.5, dtype=torch.float64, device=DEV),
                  actions=torch.full((G,), SENT, dtype=torch.int32, device=DEV),
                  frames=torch.full((G * 84 * 84 * C,), 0xAB, dtype=torch.uint8, device=DEV),
                  status=torch.full((1,), 0x1000, dtype=torch.int32, device=DEV),
                  ws=torch.full((int(lib.coevo_dqn16_workspace_bytes(G)) // 4,), 3.25, dtype=torch.float32, device=DEV))
    before = {k: v.clone() for k, v in poison.items()}
    p = {k: L._p(v) for k, v in poison.items()}
    step_order = ("gs", "acc", "n_games", "ord0", "gen", "per_gen", "t", "lim", "row_prev", "actions", "row_cur", "frames", "C", "n",
                  "seed", "slab", "tasks", "n_tasks", "n_rows", "ws", "status")
    good = dict(gs=p["gs"], acc=p["acc"], n_games=G, ord0=L._p(ord0), gen=L._p(gen), per_gen=0, t=1, lim=L._p(lim),
                row_prev=L._p(rows), actions=p["actions"], row_cur=L._p(rows), frames=p["frames"], C=C, n=n, seed=5,
                slab=L._p(slab), tasks=L._p(d_tasks), n_tasks=2, n_rows=G, ws=p["ws"], status=p["status"])
    bad = [{k: None} for k in ("gs", "acc", "ord0", "lim", "row_prev", "actions", "row_cur", "slab", "tasks", "ws", "status")]
    bad += [dict(t=0), dict(t=-1), dict(t=65536), dict(n_games=0), dict(n_games=-1), dict(n_tasks=0), dict(n_rows=0), dict(C=0),
            dict(C=7), dict(n=0), dict(n=33), dict(C=C | L.DQN_FC1_TILED), dict(slab=L._p(slab) + 4), dict(slab=L._p(slab) + 8)]
    for b in bad:
        a = dict(good, **b)
        assert lib.coevo_dqn16_out_synth_step(*[a[k] for k in step_order], L._stream()) == ERR_ARG, b
    hid_order = ("slab", "tasks", "n_tasks", "max_rows", "n_rows", "C", "n", "frames", "status", "ws")
    hgood = dict(slab=L._p(slab), tasks=L._p(d_tasks), n_tasks=2, max_rows=1, n_rows=G, C=C, n=n, frames=p["frames"],
                 status=p["status"], ws=p["ws"])
    hbad = [{k: None} for k in ("slab", "tasks", "frames", "status", "ws")]
    hbad += [dict(n_tasks=0), dict(n_rows=0), dict(max_rows=0), dict(max_rows=17), dict(C=0), dict(C=7), dict(n=0), dict(n=33),
             dict(C=C | L.DQN_FC1_TILED), dict(slab=L._p(slab) + 4), dict(slab=L._p(slab) + 8)]
    for b in hbad:
        a = dict(hgood, **b)
        assert lib.coevo_dqn16_forward_hidden(*[a[k] for k in hid_order], L._stream()) == ERR_ARG, b
    torch.cuda.synchronize()
    for k, v in poison.items():
        assert torch.equal(v, before[k]), f"a refused call wrote {k}"
    # frames == NULL with row_cur == NULL is the closing call, not an error; the good calls do write
    assert lib.coevo_dqn16_forward_hidden(*[hgood[k] for k in hid_order], L._stream()) == 0
    assert lib.coevo_dqn16_out_synth_step(*[dict(good, frames=None, row_cur=None)[k] for k in step_order], L._stream()) == 0
    torch.cuda.synchronize()
    assert not torch.equal(poison["ws"], before["ws"]) and not torch.equal(poison["actions"], before["actions"])
    assert torch.equal(poison["frames"], before["frames"]) and int(poison["status"].item()) == 0x1000
