"""Rollouts played back to back on ONE DeviceRollout, against the oracle's play_game bit for bit.

Training plays generation after generation on the same buffers: the persistent launch's sync words, the clock stamps, the
second state buffer, the action words and the rewards hold the previous rollout's leftovers, and the persistent launch skips
its own clearing of the sync words (and the rollout its re-arming of the stamps) when the reset launch in front of it claims to
have done both (reset_segments(arm=...) + armed=True).  Here every entry point the trainers use plays three rollouts on one
object - A, then B with other nets (packed into the same slab), other reset ordinals and the same n_cycles, then C with another
n_cycles - optionally with the scratch poisoned in between, and games that stop at different step limits in one launch."""
import numpy as np
import pytest
import torch

from coevonet_amd import genetic_algorithm as ga
from coevonet_amd import lib as L
from coevonet_amd.rollout import DeviceRollout, RolloutPlan
from oracle import ref_port as rp
from tests.test_kernels_gpu import make_nets
from tests.util import Bag

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORM = {n: L.K["COEVO_CYCLE_FORM_" + n.upper()] for n in ("tile32", "lean16", "small")}


class Setup:
    """GA-shaped games (individual i's agent_0 against shared opponents k), individuals dealt to K contiguous cohorts (as the
    trainers deal them), one slab that later rollouts repack with other nets"""

    def __init__(self, npop, nh, heavy_rows, K, persistent=True):
        self.npop, self.nh = npop, nh
        self.s10, self.s8 = L.fc_slab_stride(10), L.fc_slab_stride(8)
        n10 = npop + nh
        off = [i * self.s10 for i in range(n10)] + [n10 * self.s10 + k * self.s8 for k in range(nh)]
        D = [10] * n10 + [8] * nh
        self.games = [(n10 + k, i, npop + k) for i in range(npop) for k in range(nh)]   # (adversary, agent_0, agent_1)
        cohort = np.array([i * K // npop for i in range(npop) for _ in range(nh)], dtype=np.int32)
        self.plan = RolloutPlan(np.array(self.games), off, D, device=DEV, heavy_rows=heavy_rows, game_cohort=cohort)
        assert self.plan.n_cohorts == K
        self.cohort_games = [(int(np.argmax(cohort == k)), int((cohort == k).sum())) for k in range(K)]   # contiguous
        self.slab = torch.zeros(n10 * self.s10 + nh * self.s8, dtype=torch.float32, device=DEV)
        self.ro = DeviceRollout(self.plan, self.slab, merged=True)
        if not persistent:
            self.ro.sync_words, self.ro.desc.sync_words = None, None

    def shape(self, k):
        p = self.plan
        _, n_h, _, _, n_l, _ = p.cohort_tasks(k)
        return (n_h, n_l, p.heavy_max, p.light_max, p.n_cohorts)

    def assert_form(self, form):
        """every cohort takes the form the test is about: ONE persistent launch (conc = K), or that per-cycle kernel"""
        lib = L.load()
        for k in range(self.plan.n_cohorts):
            if form == "persistent":
                assert self.ro.sync_words is not None and lib.coevo_mpe_persistent_fits(*self.shape(k)) == 1
            else:
                assert self.ro.sync_words is None and lib.coevo_mpe_cycle_kernel_form(*self.shape(k)) == FORM[form]

    def load_nets(self, seed):
        """new nets for every seat, packed into the SAME slab (what breeding does between generations)"""
        self.seed = seed
        self.nets10 = make_nets(self.npop + self.nh, 10, seed=seed, mutate=False)
        self.nets8 = make_nets(self.nh, 8, seed=seed + 1, mutate=False)
        for flat, D, first in ((self.nets10, 10, 0), (self.nets8, 8, len(self.nets10) * self.s10)):
            src = torch.from_numpy(flat).to(DEV)
            L.call("coevo_fc_pack", L._p(src), self.slab.data_ptr() + 4 * first, len(flat), D)

    def want(self, first, limits, n_cycles):
        """the oracle's play_game of every game: reset ordinal first + g, its own step limit, n_cycles world cycles (the games
        do not depend on the cohorts or the kernel form: kept for the other cases of the module)"""
        key = (self.npop, self.nh, self.seed, first, np.asarray(limits).tobytes(), n_cycles)
        if key not in _WANT:
            stream = rp.Stream()
            out = np.zeros((len(self.games), 3))
            for g, (adv, a0, a1) in enumerate(self.games):
                out[g] = rp.play_game(stream, self.nets10[a0], self.nets10[a1], self.nets8[adv - self.npop - self.nh],
                                      int(limits[g]), n_cycles, ordinal=first + g)["rewards"]
            _WANT[key] = out
        return _WANT[key]


_WANT = {}


def poison(ro, n_cycles):
    """junk in every cohort's scratch: the abort word raised, every tag word carrying the tag the closing wait of an
    n_cycles rollout looks for, clock stamps that no real start time undercuts, NaN / 0x7f bytes in the second state buffer,
    the action words and the rewards"""
    if ro.sync_words is not None:
        w = ro.sync_words.view(ro.n_cohorts, ro.sync_words_per_cohort)
        w.fill_((n_cycles << 8) | 4)
        w[:, 0] = 1
    ro.stamps.fill_(5)
    ro.state2[1].fill_(float("nan"))
    ro.actions_by_game.fill_(0x7f7f7f7f)
    ro.rewards.fill_(float("nan"))


def assert_armed(ro, cohorts, n_cycles):
    """read back what the arming reset launch left for the cohorts the next call runs: zero sync words, stamps {UINT64_MAX, 0}"""
    torch.cuda.synchronize()
    K = ro.n_cohorts
    if ro.sync_words is not None:
        w = ro.sync_words.view(K, ro.sync_words_per_cohort)[list(cohorts)].cpu().numpy()
        assert not w.any(), f"sync words left for cohorts {list(cohorts)}: {np.unique(w)[:8]}"
    if ro.time_light:
        st = ro.stamps[:K * n_cycles].view(K, n_cycles, L.STAMP_SLOTS, 2)[list(cohorts)].cpu().numpy()
        assert (st[..., 0] == -1).all() and (st[..., 1] == 0).all(), f"stamps of cohorts {list(cohorts)} not re-armed"


def play(s, mode, n_cycles, first):
    """one rollout of every game (game g: reset ordinal first + g) through one entry point of DeviceRollout"""
    ro, n_games, K = s.ro, s.plan.n_games, s.plan.n_cohorts
    if mode in ("run_eager", "run_graph"):
        ro.use_graph = mode == "run_graph"   # (graph: B replays the graph captured for A, its in-graph clearing launches)
        ro.reset(0, n_games, first)
        ro.run(n_cycles)
    elif mode == "armed":   # GAEngine.step_sharded
        ro.reset_segments([(0, n_games // 2, first), (n_games // 2, n_games - n_games // 2, first + n_games // 2)],
                          arm=(0 if K == 1 else None, n_cycles))
        assert_armed(ro, range(K), n_cycles)
        ro.enqueue(n_cycles, armed=True)
    elif mode == "cohorts":   # GAEngine._enqueue_cohort_chains
        for k, (g0, cnt) in enumerate(s.cohort_games):
            ro.reset_segments([(g0, cnt, first + g0)], arm=(k, n_cycles))
            assert_armed(ro, [k], n_cycles)
            ro.enqueue_cohort(k, n_cycles, torch.cuda.current_stream(), armed=True)
        ro.enqueue_final_step(n_cycles)
    elif mode == "open_books":
        ro.reset(0, n_games, first)
        ro.enqueue(n_cycles, final=False)
        ro.enqueue_final_step(n_cycles)
    else:
        raise AssertionError(mode)
    torch.cuda.synchronize()
    ro.check_status()
    return ro.rewards.cpu().numpy()


def assert_equal_bits(got, want, what):
    bad = np.nonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} games differ from the oracle, first {bad[:4]}: {got[bad[:2]]} vs {want[bad[:2]]}"


def back_to_back(s, mode, poisoned, timed, cycles=(14, 14, 9)):
    """A, B (other nets, other ordinals, same n_cycles), C (other n_cycles) on one object, each against the oracle"""
    ro = s.ro
    ro.time_light = timed
    for i, n_cycles in enumerate(cycles):
        s.load_nets(seed=301 + 10 * i)
        T = 3 * n_cycles - 2 + i   # (the last cycle's three seats all acting, or only the first one / two)
        limits = np.full(s.plan.n_games, T)
        ro.set_limits(limits)
        first = 3 + 1000 * i
        if poisoned and i > 0:
            poison(ro, n_cycles)
        got = play(s, mode, n_cycles, first)
        assert_equal_bits(got, s.want(first, limits, n_cycles), f"{mode} rollout {'ABC'[i]}")
        if timed and mode != "run_eager":   # (eager run() times with events, not stamps)
            st = ro.stamps[:s.plan.n_cohorts * n_cycles].cpu().numpy()
            assert (st[..., 0] != 5).all(), f"{mode} rollout {'ABC'[i]}: a clock stamp still holds the poison"


PERSISTENT_CASES = [(mode, K, poisoned, timed) for mode, K in (("run_eager", 1), ("run_graph", 1), ("run_graph", 2), ("armed", 1),
                                                                 ("armed", 2), ("cohorts", 2), ("open_books", 1), ("open_books", 2))
                    for poisoned in (False, True) for timed in (False, True)
                    if not (mode == "run_eager" and timed)]   # (eager run() times its launches with events, not stamps)


@pytest.mark.parametrize("mode,K,poisoned,timed", PERSISTENT_CASES)
def test_persistent_rollouts_back_to_back(mode, K, poisoned, timed):
    """the persistent launch (ONE launch per cohort for all its cycles) on reused, and on poisoned, scratch: every rollout
    equals the oracle, the status word stays clean, no stamp keeps the poison"""
    s = Setup(20, 4, 8, K)
    s.assert_form("persistent")
    back_to_back(s, mode, poisoned, timed)


@pytest.mark.parametrize("mode", ["run_graph", "armed", "cohorts"])
@pytest.mark.parametrize("form,npop,heavy_rows", [("small", 20, 8), ("lean16", 20, 16), ("tile32", 40, 32)])
def test_per_cycle_rollouts_back_to_back(form, npop, heavy_rows, mode):
    """the launches per env-cycle (sync words None) of every kernel form, two cohorts, poisoned and timed"""
    s = Setup(npop, 4, heavy_rows, 2, persistent=False)
    s.assert_form(form)
    back_to_back(s, mode, poisoned=True, timed=True)


def test_armed_cannot_be_over_claimed():
    """armed=True holds only for cohorts the last arming reset covered, for that n_cycles, and only once"""
    s = Setup(20, 4, 8, 2)
    ro, n, segs, main = s.ro, 14, [(0, s.plan.n_games, 3)], torch.cuda.current_stream()
    ro.set_limits(np.full(s.plan.n_games, 3 * n))
    s.load_nets(seed=5)
    ro.reset_segments(segs, arm=(0, n))
    with pytest.raises(ValueError, match="cohort 1"):     # the call runs both cohorts; only cohort 0 was armed
        ro.enqueue(n, armed=True)
    ro.reset_segments(segs, arm=(None, n))
    with pytest.raises(ValueError, match="cycles"):       # armed for another cycle count (another stamp layout)
        ro.enqueue(n - 1, armed=True)
    ro.enqueue(n, armed=True)
    with pytest.raises(ValueError, match="cohort 0"):     # that rollout used the arm up
        ro.enqueue(n, armed=True)
    ro.reset_segments(segs, arm=(0, n))
    with pytest.raises(ValueError, match="cohort 1"):
        ro.enqueue_cohort(1, n, main, armed=True)
    ro.enqueue_cohort(0, n, main, armed=True)
    ro.reset_segments(segs, arm=(1, n))
    ro.time_light = True
    with pytest.raises(ValueError, match="cohort 1"):     # armed before the stamps were switched on
        ro.enqueue_cohort(1, n, main, armed=True)
    with pytest.raises(ValueError, match="cohort 2"):
        ro.reset_segments(segs, arm=(2, n))
    torch.cuda.synchronize()
    ro.check_status()


RAGGED = (0, 1, 2, 3, 4)


@pytest.mark.parametrize("form,K,npop,heavy_rows", [("persistent", 1, 20, 8), ("persistent", 2, 20, 8), ("small", 1, 20, 8),
                                                    ("lean16", 2, 20, 16), ("tile32", 2, 40, 32)])
def test_ragged_limits_in_one_launch(form, K, npop, heavy_rows):
    """limits 0, 1, 2, 3, 4, T-1 and T side by side in one rollout of (T+2)//3 cycles (generation 0 of every GA run has
    limit-0 evaluation games next to full ones): each game against play_game with its own limit"""
    s = Setup(npop, 4, heavy_rows, K, persistent=form == "persistent")
    s.assert_form(form)
    T = 40
    n_cycles = (T + 2) // 3
    choices = RAGGED + (T - 1, T)
    limits = np.array([choices[(7 * g + g // 5) % len(choices)] for g in range(s.plan.n_games)])
    assert set(limits) == set(choices)
    s.ro.set_limits(limits)
    for i, mode in enumerate(("run_graph", "armed")):   # (the second on the first's leftovers)
        s.load_nets(seed=401 + i)
        got = play(s, mode, n_cycles, 7 + 500 * i)
        assert_equal_bits(got, s.want(7 + 500 * i, limits, n_cycles), f"{form} {mode}")
        assert not got[limits == 0].any()


def test_sharded_loop_two_persistent_cohorts_match_oracle_port(monkeypatch):
    """the population-sharded generation loop on one GPU with two cohorts and without the cohort-wise path (COEVO_PIPELINED=0):
    ONE reset launch arms both cohorts, ONE enqueue(armed=True) runs both persistent launches, generation after generation on
    the same scratch - every number equals the sequential CPU port with the same counter-based noise"""
    from coevonet_amd.game_logic import initialize_env
    monkeypatch.setenv("COEVO_PIPELINED", "0")   # (both read when the engine is built)
    # shared-opponent chunks of <= 8 rows: the newest HoF trio also plays the 10 evaluation games in the last cohort, so with
    # the 16-row chunks of a cohort split that cohort would always hold a chunk of more than 8 rows (no persistent launch)
    monkeypatch.setenv("COEVO_HEAVY_ROWS", "8")
    cfg = dict(generations=4, population=10, hof_size=3, elites_number=2, fitness_sharing=True, max_timesteps_per_episode=40,
               max_evaluation_steps=40)
    torch.manual_seed(5)
    np.random.seed(5)
    args = Bag(algorithm="GA", coevo_force_sharded_loop=True, coevo_cohorts=2, **cfg)
    env = initialize_env(args)
    env.max_cycles = 25
    res = ga.genetic_algorithm_train(env, env.agents[0], args, None, rng="device_philox", env_mode="device")
    eng = res.engine
    assert eng.K == 2 and eng.ro.n_cohorts == 2 and not eng.pipelined and eng.ro.desc.merged and eng.sharded_run
    p = eng.ro.plan
    for k in range(2):
        _, n_h, _, _, n_l, _ = p.cohort_tasks(k)
        assert L.load().coevo_mpe_persistent_fits(n_h, n_l, p.heavy_max, p.light_max, 2) == 1
    torch.manual_seed(5)
    np.random.seed(5)
    want = rp.ga_train(Bag(algorithm="GA", **cfg), noise="philox", philox_seed=0)
    pop, hof = cfg["population"], cfg["hof_size"]
    assert len(res.elite_ids) == len(want) == args.generations
    for g, w in enumerate(want):
        assert res.elite_ids[g] == w["elite_ids"], g
        got = res.game_rewards[g]
        for i in range(3 * pop * hof):
            assert list(got[i]) == w["games"][i]["rewards"], (g, i)
        for ph in range(3):
            np.testing.assert_allclose(res.fitness[g][ph], w["fitness"][ph], rtol=2e-6)
        assert [res.rewards[r][g] for r in ga.ROLES] == w["eval_rewards"]
        assert res.sigma_after[g] == w["sigma_after"]
