"""Python driver of tests/checker16/dqn16_checker.c: the float16 DeepQN forward restated in plain sequential C (the contract
of DESIGN.md 6a "Float16 DeepQN"), compiled on first use into a temporary directory with the flags tests/fp16_checker.py
uses, together with fc16_checker.c, whose fp32 -> fp16 rounding it reuses (that file's env calls bind to liboracle.so)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from oracle import ref_port as rp

HERE = os.path.dirname(os.path.abspath(__file__))
SRCS = [os.path.join(HERE, "checker16", "dqn16_checker.c"), os.path.join(HERE, "checker16", "fc16_checker.c")]
ST_NO_ACTION = 16

_lib = None


def lib():
    global _lib
    if _lib is None:
        oracle_so = rp.build()
        rp.lib()   # the oracle's own symbols, loaded first
        out = os.path.join(tempfile.mkdtemp(prefix="dqn16_checker_"), "libdqn16_checker.so")
        odir = os.path.dirname(oracle_so)
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-Wall",
                               "-o", out] + SRCS + ["-L", odir, "-loracle", "-Wl,-rpath," + odir, "-lm"])
        L = C.CDLL(out)
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
        L.dqn16_forward.restype = C.c_int
        L.dqn16_forward.argtypes = [fp, C.c_int, C.c_int, C.c_void_p, fp, ip]
        L.fc16_f32_to_f16.restype = C.c_uint16
        L.fc16_f32_to_f16.argtypes = [C.c_float]
        _lib = L
    return _lib


def f16_bits(x):
    """the checker's fp32 -> fp16 rounding, element by element (for pinning it against numpy)"""
    L = lib()
    return np.array([L.fc16_f32_to_f16(float(v)) for v in np.asarray(x, dtype=np.float32).ravel()], dtype=np.uint16)


def forward(flat, C_, n_actions, frame_u8):
    """-> (action (0 with ST_NO_ACTION when no logit compares), logits [n] fp32 holding fp16 values, status bits)"""
    flat = np.ascontiguousarray(flat, dtype=np.float32)
    assert flat.size == rp.lib().oracle_dqn_param_count(C_, n_actions)
    f = np.ascontiguousarray(frame_u8, dtype=np.uint8)
    assert f.shape == (84, 84, C_)
    logits = np.zeros(n_actions, dtype=np.float32)
    st = C.c_int(0)
    a = lib().dqn16_forward(flat.ctypes.data_as(C.POINTER(C.c_float)), C_, n_actions, f.ctypes.data,
                            logits.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st))
    return a, logits, st.value


def ulp16(v):
    """the fp16 spacing at |v|"""
    return float(np.spacing(np.abs(np.float16(v))))


def half_net(C_, n_actions, sigma=0.02):
    """rp.dqn_init + a torch mutation of every parameter, rounded to half (draws from the global torch generator)"""
    flat, shapes = rp.dqn_init(C_, n_actions)
    return rp.dqn_mutate_torch(flat, shapes, sigma).astype(np.float16).astype(np.float32)
