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
        L.dqn16_forward_stages.restype = C.c_int
        L.dqn16_forward_stages.argtypes = [fp, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int] + [fp] * 9 + [ip]
        L.dqn16_round_mode.restype = C.c_float
        L.dqn16_round_mode.argtypes = [C.c_float, C.c_int]
        _lib = L
    return _lib


def round_mode(x, mode):
    """fp32 -> fp16 (kept as fp32) under one of MODES, element by element: the conversion dqn16_forward_stages applies at a site"""
    L, m = lib(), MODES.index(mode)
    x = np.asarray(x, dtype=np.float32)
    return np.array([L.dqn16_round_mode(float(v), m) for v in x.ravel()], dtype=np.float32).reshape(x.shape)


# the conversion sites of one row in forward order, the rounding modes (nearest_even is the contract) and the action scans
# (first_maximum is the contract) of dqn16_forward_stages; the order is the enum order of dqn16_checker.c
SITES = ("quotient", "conv1", "bn1", "conv2", "bn2", "conv3", "bn3", "fc1", "out")
MODES = ("nearest_even", "toward_zero", "ties_away", "flush_results", "saturate")
ACTION_SCANS = ("first_maximum", "scan_before_rounding", "last_maximum")
STAGES = ("x", "s1", "a1", "s2", "a2", "s3", "a3", "hid", "logits")


def stages(flat, C_, n_actions, frame_u8, site=None, mode="nearest_even", scan="first_maximum"):
    """the forward with its stages -> dict: x [C, 84, 84] the quotient image, s1 / a1 [32, 400], s2 / a2 [64, 81], s3 / a3
    [64, 49] the rounded conv sums / BatchNorm + ReLU outputs, hid [512] after ReLU, logits [n] (all fp32 holding fp16 values),
    action, status.  site (one of SITES, None: none) converts under `mode` (one of MODES), the action comes from `scan` (one of
    ACTION_SCANS): with the defaults this is forward(), anything else is a wrong kernel on paper."""
    flat = np.ascontiguousarray(flat, dtype=np.float32)
    assert flat.size == rp.lib().oracle_dqn_param_count(C_, n_actions) and 1 <= n_actions <= 32
    f = np.ascontiguousarray(frame_u8, dtype=np.uint8)
    assert f.shape == (84, 84, C_)
    out = {"x": np.zeros((C_, 84, 84), np.float32), "s1": np.zeros((32, 400), np.float32), "a1": np.zeros((32, 400), np.float32),
           "s2": np.zeros((64, 81), np.float32), "a2": np.zeros((64, 81), np.float32), "s3": np.zeros((64, 49), np.float32),
           "a3": np.zeros((64, 49), np.float32), "hid": np.zeros(512, np.float32), "logits": np.zeros(n_actions, np.float32)}
    st = C.c_int(0)
    fp = C.POINTER(C.c_float)
    a = lib().dqn16_forward_stages(flat.ctypes.data_as(fp), C_, n_actions, f.ctypes.data, -1 if site is None else SITES.index(site),
                                   MODES.index(mode), ACTION_SCANS.index(scan), *[out[k].ctypes.data_as(fp) for k in STAGES],
                                   C.byref(st))
    out["action"], out["status"] = a, st.value
    return out


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
