"""Python driver of tests/checker16/fc16_checker.c: the float16 FCNetwork forward and play_game restated in plain C
(the contract of DESIGN.md "float16 nets"), compiled with the oracle's flags into a temporary directory on first use and
linked against the oracle's liboracle.so, whose env functions (oracle_mpe_reset / _observe / _world_step) it calls."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from oracle import ref_port as rp

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "checker16", "fc16_checker.c")
NACT = 5

_lib = None


def lib():
    global _lib
    if _lib is None:
        oracle_so = rp.build()
        rp.lib()   # the oracle's own symbols, loaded first
        out = os.path.join(tempfile.mkdtemp(prefix="fc16_checker_"), "libfc16_checker.so")
        odir = os.path.dirname(oracle_so)
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-Wall",
                               "-o", out, SRC, "-L", odir, "-loracle", "-Wl,-rpath," + odir, "-lm"])
        L = C.CDLL(out)
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
        L.fc16_forward.restype = C.c_int
        L.fc16_forward.argtypes = [fp, C.c_int, fp, fp, ip]
        L.fc16_play_game.restype = C.c_int
        L.fc16_play_game.argtypes = [fp, fp, fp] + [C.c_uint64] * 5 + [C.c_int, C.c_int, C.POINTER(C.c_double), ip, fp, ip]
        L.fc16_f32_to_f16.restype = C.c_uint16
        L.fc16_f32_to_f16.argtypes = [C.c_float]
        _lib = L
    return _lib


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def f16_bits(x):
    """the checker's own fp32 -> fp16 rounding, element by element (for pinning it against numpy)"""
    L = lib()
    return np.array([L.fc16_f32_to_f16(float(v)) for v in np.asarray(x, dtype=np.float32).ravel()], dtype=np.uint16)


def forward(flat, D, obs):
    """-> (action, logits [5] fp32 holding fp16 values, status bits)"""
    flat = np.ascontiguousarray(flat, dtype=np.float32)
    obs = np.ascontiguousarray(obs, dtype=np.float32)
    logits = np.zeros(NACT, dtype=np.float32)
    st = C.c_int(0)
    a = lib().fc16_forward(_fp(flat), D, _fp(obs), _fp(logits), C.byref(st))
    return a, logits, st.value


def play_game(stream, net_a0, net_a1, net_adv, limit=None, max_cycles=25, ordinal=None):
    """rp.play_game with the fp16 forward -> dict(rewards, steps, actions, margins, status, ordinal)"""
    o = stream.next_ordinal() if ordinal is None else ordinal
    rewards = (C.c_double * 3)()
    actions = np.zeros(3 * max_cycles + 3, dtype=np.int32)
    margins = np.zeros(3 * max_cycles + 3, dtype=np.float32)
    st = C.c_int(0)
    nets = [np.ascontiguousarray(n, dtype=np.float32) for n in (net_adv, net_a0, net_a1)]
    steps = lib().fc16_play_game(_fp(nets[0]), _fp(nets[1]), _fp(nets[2]), *stream.st, o,
                                 -1 if limit is None else int(limit), max_cycles, rewards,
                                 actions.ctypes.data_as(C.POINTER(C.c_int)), _fp(margins), C.byref(st))
    return {"rewards": [rewards[0], rewards[1], rewards[2]], "steps": steps, "actions": actions[:steps].tolist(),
            "margins": margins[:steps].tolist(), "status": st.value, "ordinal": o}


def play_game_steps(stream, net_a0, net_a1, net_adv, limit=None, max_cycles=25, ordinal=None, poke=None):
    """fc16_play_game's loop in Python on the same pieces (oracle_mpe_reset / _observe / _world_step, fc16_forward): the twin
    of rp.play_game_steps, for tests that edit a game's state after the reset with poke(MpeState).  With no poke it returns
    play_game's rewards, steps, actions and status bit for bit."""
    o = stream.next_ordinal() if ordinal is None else ordinal
    O, L = rp.lib(), lib()
    nets = [np.ascontiguousarray(n, dtype=np.float32) for n in (net_adv, net_a0, net_a1)]
    s = rp.MpeState()
    O.oracle_mpe_reset(*stream.st, o, C.byref(s))
    if poke is not None:
        poke(s)
    cum, rew, acc, act = [0.0] * 3, [0.0] * 3, [0.0] * 3, (C.c_int * 3)(0, 0, 0)
    sel = world_steps = timesteps = 0
    trunc, actions = False, []
    obs, logits, st = np.zeros(10, dtype=np.float32), np.zeros(NACT, dtype=np.float32), C.c_int(0)
    rg, ra = C.c_double(0), C.c_double(0)
    while True:
        agent = sel
        O.oracle_mpe_observe(C.byref(s), agent, _fp(obs))
        a = L.fc16_forward(_fp(nets[agent]), 8 if agent == 0 else 10, _fp(obs), _fp(logits), C.byref(st))
        a = max(a, 0)
        actions.append(int(a))
        sel = (agent + 1) % 3
        act[agent] = int(a)
        if sel == 0:
            O.oracle_mpe_world_step(C.byref(s), act, C.byref(rg), C.byref(ra))
            rew = [ra.value, rg.value, rg.value]
            world_steps += 1
            trunc = world_steps >= max_cycles
        else:
            rew = [0.0, 0.0, 0.0]
        cum[agent] = 0.0
        cum = [c + r for c, r in zip(cum, rew)]
        acc[agent] += cum[sel]
        timesteps += 1
        if (limit is not None and timesteps >= limit) or trunc:
            break
    return {"rewards": [acc[1], acc[2], acc[0]], "steps": timesteps, "actions": actions, "status": st.value, "ordinal": o}


def ulp16(v):
    """the fp16 spacing at |v|"""
    return float(np.spacing(np.abs(np.float16(v))))


def safe_steps(actions_margins_logits):
    """number of leading forwards whose top-2 margin exceeds 2 fp16 ulps of the top logit"""
    n = 0
    for margin, top in actions_margins_logits:
        if not margin > 2 * ulp16(top):
            break
        n += 1
    return n
