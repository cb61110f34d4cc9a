"""MI355X-native accelerator for CoEvoNet's population-evaluation hot path."""
import os as _os
import sys as _sys

# GPU_MAX_HW_QUEUES: HIP maps streams onto this many hardware queues round robin (default 4).  With several engines in
# one process a later engine's cohort stream then shares the caller's queue and its launches serialise (cfg 5 after the
# headline engine: 8.3 instead of 10.1 generations/s), so the package asks for 8 - which only counts when the variable is
# set BEFORE the HIP runtime starts.  Under rocprofv3 the profiler's library starts the runtime first: export it in the
# shell (tools/profile_round.sh, tools/pmc_kernel.sh do).  bench.py records the value it ran with.
if "GPU_MAX_HW_QUEUES" not in _os.environ:
    _t = _sys.modules.get("torch")
    if _t is not None and _t.cuda.is_initialized():
        import warnings as _w
        _w.warn("coevonet_amd: the HIP runtime started before this import, so GPU_MAX_HW_QUEUES=8 cannot take effect; "
                "export it before the process starts (cohort streams otherwise share hardware queues)")
    _os.environ["GPU_MAX_HW_QUEUES"] = "8"
# DEBUG_HIP_DYNAMIC_QUEUES (NOT set here).  With the runtime's default (static) mapping a stream keeps the hardware queue it was
# dealt when it was created; the first hipGraph launch of a process creates the graph executor's own parallel streams, and
# streams created after that share hardware queues - every operation on them queues behind its neighbours' (~9 us per
# operation: the host-cores env mode after the device-resident loop ran 233-303 instead of 440-455 generations/s; bisected to
# ONE replayed graph in round 4, mechanism found in round 5: profiles/r05_experiments.md section 1).  DEBUG_HIP_DYNAMIC_QUEUES=1
# (a stream takes a free hardware queue when it has work) removes the cliff - both orders then run at a fresh process's rate -
# but it is a debug switch of the runtime: a long process that builds and tears down many engines (the DeepQN GPU tests, 34
# in one process) died with a segmentation fault inside hipDeviceSynchronize under it, twice out of two, and never without.
# So: export it yourself for a process that runs the host-cores mode after a graph-replaying mode and is short-lived, or do
# what bench.py does - run the host-cores mode in a process of its own.

__all__ = ["HalfGAEngine", "HalfESEngine", "DeepQNHalf", "HalfDQNGAEngine", "HalfSynthRollout", "HalfDQNESEngine",
           "CrossPlay", "DQNCrossPlay", "test_agents", "cross_play_checkpoints", "BaselineCrossPlay", "DQNBaselineCrossPlay",
           "RandomBaseline", "PeriodicBaseline", "ConstantBaseline", "AlwaysFire", "MLPBaseline", "load_ppo_baseline"]
_BASELINE_NAMES = frozenset(__all__[__all__.index("BaselineCrossPlay"):])
_GAUNTLET_NAMES = ("Gauntlet", "Champion", "GauntletResult", "GauntletSpec")
__all__ += list(_GAUNTLET_NAMES)
_DUEL_CROSSPLAY_NAMES = ("DuelCrossPlay", "DuelCrossPlayResult", "DuelSeatRollout", "HalfDuelSeatRollout", "TrackerSeat",
                         "duel_seat_action", "duel_tracker_word", "duel_test_agents", "duel_cross_play_checkpoints")
__all__ += list(_DUEL_CROSSPLAY_NAMES)


def __getattr__(name):
    # resolved on first use: importing the package alone loads neither torch nor the trainers
    if name == "HalfGAEngine":
        from .ga_half import HalfGAEngine
        return HalfGAEngine
    if name == "HalfESEngine":
        from .es_half import HalfESEngine
        return HalfESEngine
    if name == "DeepQNHalf":
        from .deepqn import DeepQNHalf
        return DeepQNHalf
    if name in ("HalfDQNGAEngine", "HalfSynthRollout"):
        from . import dqn_ga_half
        return getattr(dqn_ga_half, name)
    if name == "HalfDQNESEngine":
        from .dqn_es_half import HalfDQNESEngine
        return HalfDQNESEngine
    if name in ("CrossPlay", "DQNCrossPlay", "test_agents", "cross_play_checkpoints"):
        from . import crossplay
        return getattr(crossplay, name)
    if name in _BASELINE_NAMES:
        from . import baselines
        return getattr(baselines, name)
    if name in _GAUNTLET_NAMES:
        from . import gauntlet
        return getattr(gauntlet, name)
    if name in _DUEL_CROSSPLAY_NAMES:
        from . import duel_crossplay
        return getattr(duel_crossplay, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
