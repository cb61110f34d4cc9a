"""ctypes binding of libcoevo.so (the C ABI in include/coevo.h).

PyTorch-ROCm is only plumbing here: tensors give device memory (``data_ptr()``) and streams.  There is NO CPU or
eager fallback: if the HIP library is missing or a call fails, this raises.

The header is the one statement of the ABI: ``parse_header`` turns its text into the constants, the ``ctypes.Structure``
mirrors and the signature table ``_SIGS`` at import.  An entry point, struct or ``COEVO_*`` value declared there is bound here.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import re

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("COEVO_LIB") or os.path.join(HERE, "libcoevo.so")  # COEVO_LIB: A/B builds
HEADER_PATH = os.path.join(HERE, "..", "include", "coevo.h")
EXT_HEADER_PATH = os.path.join(HERE, "..", "include", "coevo_ext.h")   # additions that are not yet part of the pinned ABI
CROSSPLAY_HEADER_PATH = os.path.join(HERE, "..", "include", "coevo_crossplay.h")   # the cross-play entry points, likewise
SHARING_HEADER_PATH = os.path.join(HERE, "..", "include", "coevo_sharing.h")   # the Co-GA population-sharing entry points, likewise
SHARING16_HEADER_PATH = os.path.join(HERE, "..", "include", "coevo_sharing16.h")   # ... and their float16 pairwise distance
BASELINE_HEADER_PATH = os.path.join(HERE, "..", "include", "coevo_baseline.h")   # the baseline-opponent entry points, likewise
GAUNTLET_HEADER_PATH = os.path.join(HERE, "..", "include", "coevo_gauntlet.h")   # the baseline-gauntlet entry points, likewise
DUEL_HEADER_PATH = os.path.join(HERE, "..", "include", "coevo_duel.h")   # the paddle-duel env-step entry points, likewise
DUEL_SEATS_HEADER_PATH = os.path.join(HERE, "..", "include", "coevo_duel_seats.h")   # ... with a scripted seat in the launch


class CoevoError(RuntimeError):
    pass


# ---------------------------------------------------------------------------------------------------- the header reader
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
            "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
_POINTED_TO = ("void", "char", "uint8_t")   # what the header names behind a '*' only


def _declare(text, structs, decl, spec=None):
    """one C declarator, 'const float *obs' or 'tasks[2]' -> (name, ctypes type or None for void, type word); `spec` is the
    type word of the list's first declarator for the later ones ('int32_t game_first, count').  `decl` is quoted in errors."""
    m = re.fullmatch(r"([\w\s]*?)\s*(\**)\s*(\w+)\s*(?:\[(\d+)\])?", text.strip())
    words = [w for w in (m.group(1).split() if m else []) if w not in ("const", "struct")]
    if not m or len(words) > 1 or not (words or spec):
        raise CoevoError(f"include/coevo.h: cannot read the declarator {text.strip()!r} in {decl!r}")
    base = words[0] if words else spec
    known = structs.get(base) or _SCALARS.get(base)
    if m.group(2):   # every pointer is an address; const char * is a string
        if known is None and base not in _POINTED_TO:
            raise CoevoError(f"include/coevo.h: pointer to the unknown type {base!r} in {decl!r}")
        t = C.c_char_p if base == "char" else C.c_void_p
    elif base == "void":
        t = None
    elif known is not None:
        t = known
    else:
        raise CoevoError(f"include/coevo.h: unknown type {base!r} in {decl!r}")
    if m.group(4):
        t = t * int(m.group(4))
    return m.group(3), t, base


def parse_header(text, mirror=lambda name, fields: type(name, (C.Structure,), {"_fields_": fields}), known=None):
    """the text of include/coevo.h -> ({COEVO_X: int}, {struct name: ctypes.Structure class}, {entry point: (restype,
    [argtypes])}).  The grammar is the header's, not C's: comments, ``#define NAME`` + a decimal or hex literal, a
    parenthesised negative or a product of earlier names, ``typedef struct [tag] { fields } name;`` and prototypes.  Whatever
    does not fit raises CoevoError with the declaration quoted; nothing is guessed.  mirror(name, fields) makes a struct's class.
    `known`: the structs of a header this one includes (its ``#include "coevo.h"`` line is skipped), usable in its prototypes."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r'^[ \t]*#[ \t]*include[ \t]+"coevo\.h"[ \t]*$', "", text, flags=re.M)   # the extension header builds on coevo.h
    consts, structs, sigs = {}, dict(known or {}), {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)(.*)$", text, flags=re.M):
        v = value.strip()
        v = v[1:-1].strip() if v.startswith("(") and v.endswith(")") else v
        factors = [f.strip() for f in v.split("*")]
        if re.fullmatch(r"-?(0|[1-9]\d*)|0[xX][0-9a-fA-F]+", v):
            consts[name] = int(v, 0)
        elif all(f in consts for f in factors):
            consts[name] = math.prod(consts[f] for f in factors)
        elif v:   # a bare '#define COEVO_H' is the include guard
            raise CoevoError(f"include/coevo.h: not a literal or a product of earlier names: '#define {name}{value.rstrip()}'")
    text = re.sub(r"^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus.*?^[ \t]*#[ \t]*endif.*?$", "", text, flags=re.S | re.M)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)

    def struct(m):
        decl, fields = f"struct {m.group(2)}", []
        for line in filter(None, (d.strip() for d in m.group(1).split(";"))):
            spec = None
            for part in line.split(","):
                field, t, spec = _declare(part, structs, f"{decl}: {' '.join(line.split())}", spec)
                if t is None:
                    raise CoevoError(f"include/coevo.h: a void field in {decl}: {line!r}")
                fields.append((field, t))
        structs[m.group(2)] = mirror(m.group(2), fields)
        return ""
    text = re.sub(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    for decl in filter(None, (" ".join(d.split()) for d in text.split(";"))):
        m = re.fullmatch(r"(.*?\w)\s*\((.*)\)", decl)
        if not m:
            raise CoevoError(f"include/coevo.h: neither a typedef struct nor a prototype: {decl!r}")
        name, res, _ = _declare(m.group(1), structs, decl)
        args = [] if m.group(2).strip() == "void" else [_declare(p, structs, decl)[1] for p in m.group(2).split(",")]
        if None in args:
            raise CoevoError(f"include/coevo.h: a void argument in {decl!r}")
        sigs[name] = (res, args)
    return consts, structs, sigs


class PCG64State(C.Structure):
    """coevo_pcg64, derived like the others but under Python field names without the header's pcg_ prefix (state_hi, state_lo,
    inc_hi, inc_lo): the recorded launch scripts under tests/golden name them so"""

    @classmethod
    def from_seed(cls, seed):
        st = np.random.PCG64(seed).state["state"]
        m = (1 << 64) - 1
        return cls(st["state"] >> 64, st["state"] & m, st["inc"] >> 64, st["inc"] & m)


def _mirror(name, fields):
    if name != "coevo_pcg64":
        return type(name, (C.Structure,), {"_fields_": fields})
    PCG64State._fields_ = [(f[len("pcg_"):], t) for f, t in fields]
    return PCG64State


def _header_text(path=None):
    path = HEADER_PATH if path is None else path
    try:
        with open(path) as f:
            return f.read()
    except OSError as e:
        raise CoevoError(f"{path} is missing: the binding is derived from the header ({e})") from e


K, STRUCTS, _SIGS = parse_header(_header_text(), _mirror)


def _parse_ext_header(text):
    """include/coevo_ext.h -> (its constants, its entry points): the reader of coevo.h, which has seen coevo.h's structs; the
    extension header declares prototypes and constants only, and no name coevo.h declares"""
    consts, structs, sigs = parse_header(text, known=STRUCTS)
    if set(structs) != set(STRUCTS) or set(sigs) & set(_SIGS) or set(consts) & set(K):
        raise CoevoError("include/coevo_ext.h: declares a struct or repeats a name of include/coevo.h")
    return consts, sigs


K_EXT, _EXT_SIGS = _parse_ext_header(_header_text(EXT_HEADER_PATH))


def _parse_crossplay_header(text):
    """include/coevo_crossplay.h -> (its constants, its entry points), read like coevo_ext.h: prototypes and constants only, and
    no name that coevo.h or coevo_ext.h declares"""
    consts, structs, sigs = parse_header(text, known=STRUCTS)
    if set(structs) != set(STRUCTS) or set(sigs) & (set(_SIGS) | set(_EXT_SIGS)) or set(consts) & (set(K) | set(K_EXT)):
        raise CoevoError("include/coevo_crossplay.h: declares a struct or repeats a name of include/coevo.h or include/coevo_ext.h")
    return consts, sigs


K_XP, _XP_SIGS = _parse_crossplay_header(_header_text(CROSSPLAY_HEADER_PATH))


def _parse_sharing_header(text):
    """include/coevo_sharing.h -> (its constants, its entry points), read like coevo_crossplay.h: prototypes and constants only,
    and no name that one of the three other headers declares"""
    consts, structs, sigs = parse_header(text, known=STRUCTS)
    if (set(structs) != set(STRUCTS) or set(sigs) & (set(_SIGS) | set(_EXT_SIGS) | set(_XP_SIGS))
            or set(consts) & (set(K) | set(K_EXT) | set(K_XP))):
        raise CoevoError("include/coevo_sharing.h: declares a struct or repeats a name of include/coevo.h, include/coevo_ext.h "
                         "or include/coevo_crossplay.h")
    return consts, sigs


K_SH, _SH_SIGS = _parse_sharing_header(_header_text(SHARING_HEADER_PATH))


def _parse_sharing16_header(text):
    """include/coevo_sharing16.h -> its entry points, read like coevo_sharing.h: prototypes and constants only, and no name
    that one of the four other headers declares"""
    consts, structs, sigs = parse_header(text, known=STRUCTS)
    if (set(structs) != set(STRUCTS) or set(sigs) & (set(_SIGS) | set(_EXT_SIGS) | set(_XP_SIGS) | set(_SH_SIGS))
            or set(consts) & (set(K) | set(K_EXT) | set(K_XP) | set(K_SH))):
        raise CoevoError("include/coevo_sharing16.h: declares a struct or repeats a name of include/coevo.h, "
                         "include/coevo_ext.h, include/coevo_crossplay.h or include/coevo_sharing.h")
    return sigs


_SH16_SIGS = _parse_sharing16_header(_header_text(SHARING16_HEADER_PATH))


def _parse_baseline_header(text):
    """include/coevo_baseline.h -> (its constants, its entry points), read like coevo_crossplay.h: prototypes and constants
    only, and no name that one of the five other headers declares"""
    consts, structs, sigs = parse_header(text, known=STRUCTS)
    if (set(structs) != set(STRUCTS) or set(sigs) & (set(_SIGS) | set(_EXT_SIGS) | set(_XP_SIGS) | set(_SH_SIGS) | set(_SH16_SIGS))
            or set(consts) & (set(K) | set(K_EXT) | set(K_XP) | set(K_SH))):
        raise CoevoError("include/coevo_baseline.h: declares a struct or repeats a name of another header")
    return consts, sigs


K_BL, _BL_SIGS = _parse_baseline_header(_header_text(BASELINE_HEADER_PATH))


def _parse_gauntlet_header(text):
    """include/coevo_gauntlet.h -> (its constants, its entry points), read like coevo_baseline.h: prototypes and constants
    only, and no name that one of the six other headers declares"""
    consts, structs, sigs = parse_header(text, known=STRUCTS)
    if (set(structs) != set(STRUCTS)
            or set(sigs) & (set(_SIGS) | set(_EXT_SIGS) | set(_XP_SIGS) | set(_SH_SIGS) | set(_SH16_SIGS) | set(_BL_SIGS))
            or set(consts) & (set(K) | set(K_EXT) | set(K_XP) | set(K_SH) | set(K_BL))):
        raise CoevoError("include/coevo_gauntlet.h: declares a struct or repeats a name of another header")
    return consts, sigs


K_GT, _GT_SIGS = _parse_gauntlet_header(_header_text(GAUNTLET_HEADER_PATH))


def _parse_duel_header(text):
    """include/coevo_duel.h -> (its constants, its entry points), read like coevo_gauntlet.h: prototypes and constants only,
    and no name that one of the seven other headers declares"""
    consts, structs, sigs = parse_header(text, known=STRUCTS)
    if (set(structs) != set(STRUCTS)
            or set(sigs) & (set(_SIGS) | set(_EXT_SIGS) | set(_XP_SIGS) | set(_SH_SIGS) | set(_SH16_SIGS) | set(_BL_SIGS)
                            | set(_GT_SIGS))
            or set(consts) & (set(K) | set(K_EXT) | set(K_XP) | set(K_SH) | set(K_BL) | set(K_GT))):
        raise CoevoError("include/coevo_duel.h: declares a struct or repeats a name of another header")
    return consts, sigs


K_DUEL, _DUEL_SIGS = _parse_duel_header(_header_text(DUEL_HEADER_PATH))


def _parse_duel_seats_header(text):
    """include/coevo_duel_seats.h -> (its constants, its entry points), read like coevo_duel.h: prototypes and constants only,
    and no name that one of the eight other headers declares"""
    consts, structs, sigs = parse_header(text, known=STRUCTS)
    if (set(structs) != set(STRUCTS)
            or set(sigs) & (set(_SIGS) | set(_EXT_SIGS) | set(_XP_SIGS) | set(_SH_SIGS) | set(_SH16_SIGS) | set(_BL_SIGS)
                            | set(_GT_SIGS) | set(_DUEL_SIGS))
            or set(consts) & (set(K) | set(K_EXT) | set(K_XP) | set(K_SH) | set(K_BL) | set(K_GT) | set(K_DUEL))):
        raise CoevoError("include/coevo_duel_seats.h: declares a struct or repeats a name of another header")
    return consts, sigs


K_DUEL_SEATS, _DUEL_SEATS_SIGS = _parse_duel_seats_header(_header_text(DUEL_SEATS_HEADER_PATH))

OBS_STRIDE, LOGIT_STRIDE, FC_MAX_ROWS = K["COEVO_OBS_STRIDE"], K["COEVO_LOGIT_STRIDE"], K["COEVO_FC_MAX_ROWS"]
MPE_STATE_DOUBLES, STAMP_SLOTS = K["COEVO_MPE_STATE_DOUBLES"], K["COEVO_STAMP_SLOTS"]
ST_NAMES = {K["COEVO_ST_BAD_INPUT"]: "input contains inf or NaN",
            K["COEVO_ST_BAD_FC1"]: "output contains inf or NaN after fc1",
            K["COEVO_ST_BAD_FC2"]: "output contains inf or NaN after fc2",
            K["COEVO_ST_BAD_OUT"]: "output contains inf or NaN",
            K["COEVO_ST_NO_ACTION"]: "no action selected (current_best_position = -1)",
            K["COEVO_ST_SYNC_TIMEOUT"]: "persistent rollout: a workgroup timed out waiting for the other rows of its games "
                                        "(COEVO_ST_SYNC_TIMEOUT)",
            K["COEVO_ST_BAD_TASK"]: "fp16 forward: a task with a bad width, row count or unaligned net offset was skipped "
                                    "(COEVO_ST_BAD_TASK)"}

DQN_LOGIT_STRIDE, DQN_MAX_ROWS = K["COEVO_DQN_LOGIT_STRIDE"], K["COEVO_DQN_MAX_ROWS"]
DQN_FC1_TILED = K["COEVO_DQN_FC1_TILED"]   # or-ed into the channel argument of the layout-dependent DeepQN entry points
DQP_SKIP_BN = K["COEVO_DQP_SKIP_BN"]       # the BatchNorm affine keeps its words (Co-ES)


def _dtype(struct):
    """numpy view of a header struct (one without padding)"""
    dt = np.dtype([(f, np.dtype(t)) for f, t in struct._fields_])
    assert dt.itemsize == C.sizeof(struct), struct
    return dt


TASK_DTYPE, DQN_TASK_DTYPE = _dtype(STRUCTS["coevo_fc_task"]), _dtype(STRUCTS["coevo_dqn_task"])
TASK_RESIDENT = K["COEVO_TASK_RESIDENT"]   # coevo_fc_task.reserved bit
# COEVO_TASK_TILED: a shared-opponent task reads W2 from the net's tile-major twin, W2_FLOATS floats that start
# (reserved >> TASK_TWIN_SHIFT) * TASK_TWIN_UNIT floats into the slab
TASK_TILED, TASK_TWIN_SHIFT, TASK_TWIN_UNIT = K["COEVO_TASK_TILED"], K["COEVO_TASK_TWIN_SHIFT"], K["COEVO_TASK_TWIN_UNIT"]
W2_FLOATS = K["COEVO_FC_W2_FLOATS"]


def task_tiled_flags(twin_off):
    """coevo_fc_task.reserved of a task whose net's W2 twin starts twin_off floats into the slab"""
    assert twin_off % TASK_TWIN_UNIT == 0 and 0 <= twin_off // TASK_TWIN_UNIT < 1 << (31 - TASK_TWIN_SHIFT)
    return TASK_TILED | (twin_off // TASK_TWIN_UNIT) << TASK_TWIN_SHIFT


PerturbJob, Perturb16Job = STRUCTS["coevo_fc_perturb_job"], STRUCTS["coevo_fc16_perturb_job"]
FinalizeJob, ResetSeg, FinalPack = STRUCTS["coevo_fc_finalize_job"], STRUCTS["coevo_reset_seg"], STRUCTS["coevo_final_pack"]
RolloutDesc = STRUCTS["coevo_rollout_desc"]
HostCohort, HostRolloutDesc = STRUCTS["coevo_host_cohort"], STRUCTS["coevo_host_rollout_desc"]
FrameCohort, FramesRolloutDesc = STRUCTS["coevo_frame_cohort"], STRUCTS["coevo_frames_rollout_desc"]
GaSelectRole, GaAdaptArgs = STRUCTS["coevo_ga_select_role"], STRUCTS["coevo_ga_adapt_args"]
GaPromoteRole = STRUCTS["coevo_ga_promote_role"]   # also serves coevo_ga16_promote_role: the same fields, untyped regions

_lib = None


def exported_symbols():
    return sorted(_SIGS)


def extension_symbols():
    """the entry points of include/coevo_ext.h, bound by load() beside the pinned ABI's"""
    return sorted(_EXT_SIGS)


def crossplay_symbols():
    """the entry points of include/coevo_crossplay.h, bound by load() beside the two other tables"""
    return sorted(_XP_SIGS)


def sharing_symbols():
    """the entry points of include/coevo_sharing.h, bound by load() beside the three other tables"""
    return sorted(_SH_SIGS)


def sharing16_symbols():
    """the entry points of include/coevo_sharing16.h, bound by load() beside the four other tables"""
    return sorted(_SH16_SIGS)


def baseline_symbols():
    """the entry points of include/coevo_baseline.h, bound by load() beside the five other tables"""
    return sorted(_BL_SIGS)


def gauntlet_symbols():
    """the entry points of include/coevo_gauntlet.h, bound by load() beside the six other tables"""
    return sorted(_GT_SIGS)


def duel_symbols():
    """the entry points of include/coevo_duel.h, bound by load() beside the seven other tables"""
    return sorted(_DUEL_SIGS)


def duel_seats_symbols():
    """the entry points of include/coevo_duel_seats.h, bound by load() beside the eight other tables"""
    return sorted(_DUEL_SEATS_SIGS)


def load():
    """dlopen libcoevo.so; raises CoevoError when it has not been built (python -m coevonet_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CoevoError(f"{LIB_PATH} is missing: build the HIP extension first "
                             "(python -m coevonet_amd.build); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in {**_SIGS, **_EXT_SIGS, **_XP_SIGS, **_SH_SIGS, **_SH16_SIGS, **_BL_SIGS,
                                  **_GT_SIGS, **_DUEL_SIGS, **_DUEL_SEATS_SIGS}.items():
            fn = getattr(L, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        flags = (L.coevo_build_flags() or b"").decode()
        if flags and os.environ.get("COEVO_ALLOW_VARIANT") != "1":
            raise CoevoError(f"{LIB_PATH} was built with non-default switches ({flags}): a measurement variant, not the "
                             "product (rebuild with python -m coevonet_amd.build, or set COEVO_ALLOW_VARIANT=1 in tools/)")
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        raise CoevoError(f"{what} failed with code {rc} "
                         f"({'bad argument' if rc == -1 else 'HIP runtime error' if rc == -2 else 'unsupported here' if rc == -3 else 'unknown'})")


def _p(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device-resident contiguous tensor required"
    return t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def call(name, *args):
    _check(getattr(load(), name)(*args, _stream()), name)


def raise_on_status(status_tensor):
    """Turn COEVO_ST_* bits into the ValueError the reference raises (MPE/fcnetwork.py:39-65,87)."""
    st = int(status_tensor.item())
    if st:
        msgs = [m for b, m in ST_NAMES.items() if st & b]
        raise ValueError("\n\t Warning: " + "; ".join(msgs))


def fc_param_count(D):
    return int(load().coevo_fc_param_count(D))


def fc_slab_stride(D):
    return int(load().coevo_fc_slab_stride(D))


def fc16_slab_stride(D):
    return int(load().coevo_fc16_slab_stride(D))


def fc16_perturb_blocks(D):
    return int(load().coevo_fc16_perturb_blocks(D))


def es16_partial_floats(D):
    return int(load().coevo_es16_partial_floats(D))


def host_tensor(ctx, shape, dtype):
    """zero-filled page-locked, device-mapped host tensor owned by the host-rollout context `ctx` (coevo_host_rollout_alloc:
    first touched on the NUMA node the context's cores run on); valid until the context is destroyed"""
    shape = tuple(int(x) for x in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    np_dtype = np.dtype(dtype)
    nbytes = max(int(np.prod(shape)) * np_dtype.itemsize, 1)
    ptr = load().coevo_host_rollout_alloc(ctx, nbytes)
    if not ptr:
        raise CoevoError("coevo_host_rollout_alloc failed")
    buf = (C.c_char * nbytes).from_address(ptr)
    return torch.from_numpy(np.frombuffer(buf, dtype=np_dtype, count=int(np.prod(shape))).reshape(shape))


def host_placement(ctx, max_cpus=256):
    """-> {"cpus": [...], "gpu_numa_node": n, "cpu_numa_node": n, "pinned": bool, "on_gpu_node": bool, "one_l3": bool}"""
    cpus = np.zeros(max_cpus, dtype=np.int32)
    info = np.zeros(4, dtype=np.int32)
    n = load().coevo_host_rollout_placement(ctx, cpus.ctypes.data, max_cpus, info.ctypes.data)
    if n < 0:
        raise CoevoError(f"coevo_host_rollout_placement failed with code {n}")
    return {"cpus": [int(c) for c in cpus[:n]], "gpu_numa_node": int(info[0]), "cpu_numa_node": int(info[1]),
            "pinned": bool(info[3]), "on_gpu_node": bool(info[2] & 1), "one_l3": bool(info[2] & 2),
            "mode": os.environ.get("COEVO_HOST_PIN", "1")}


def tasks_to_device(tasks_np, device="cuda"):
    """numpy structured array (TASK_DTYPE) -> device byte tensor usable as coevo_fc_task*"""
    assert tasks_np.dtype in (TASK_DTYPE, DQN_TASK_DTYPE)
    return torch.from_numpy(tasks_np.view(np.uint8).copy()).to(device)
