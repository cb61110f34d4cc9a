"""Adversarial float16 DeepQN parameter vectors and frames for the fp16 DeepQN forward (csrc/dqn16.hip, csrc/dqn16_tiled.hip, the
H16 paths of csrc/dqn_conv.hip.h, dqn_out_row<true>), with the C checker (tests/checker16/dqn16_checker.c through
tests/dqn16_checker.py) as the only judge.

Every net is a healthy half net (ck.half_net: every entry an fp16 value, the BatchNorm affine included) with entries overwritten
and rounded to fp16 again (inf and NaN kept).  Nothing here knows what a kernel returns: the expected conv3 activations, hidden
row, logits, action and status of a (net, frame) pair always come from ck.stages through the cache below; PROPERTY and ROUNDING
only say what tests/test_dqn16_edges_cpu.py pins of the checker itself.  The conventions are tests/dqn_edge_nets.py's, whose
offsets / view / FRAMES / class functions are reused.  No GPU needed: launch() imports torch's device side when it is called
(tests/test_dqn16_forward_edges_gpu.py); tests/test_fp16_dqn_gpu.py imports the nets it used to build itself (edge_nets)."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from tests import dqn16_checker as ck
from tests import dqn_edge_nets as E32
from tests.dqn_edge_nets import TENSORS, digest, offsets, ragged_frames, view   # noqa: F401  (re-exported)
from tests.fc16_edge_nets import f16, last_maximum, same_bits_up_to_nan   # noqa: F401  (re-exported)

NO_ACTION, BAD_TASK = E32.NO_ACTION, E32.L.K["COEVO_ST_BAD_TASK"]
MIN_NORMAL16 = np.float32(2.0 ** -14)
POISON_I32 = 0x7f7f7f7f      # logits and action words before a launch; the workspace starts as NaN
SITES, MODES = ck.SITES, ck.MODES
WRONG_MODES = MODES[1:]
CLASS_SEED = 1600


@functools.lru_cache(maxsize=None)
def _base(C, n, seed):
    torch.manual_seed(seed)
    w = ck.half_net(C, n, 0.02)
    w.flags.writeable = False
    return w


def base_net(C, n, seed):
    """a healthy half net: fresh initialisation plus N(0, 0.02) on every entry, rounded to fp16"""
    return _base(C, n, seed).copy()


def healthy(C, n, k):
    """healthy net k = 0 .. 3 of the ragged and filler rows"""
    return _base(C, n, 1610 + k % 4)


# ------------------------------------------------------------------------------------------- the carried-over classes
CLASSES = {name: E32.CLASSES[name] for name in (
    "plain", "tie_all", "tie2", "tie2_0_last", "tie2_last2", "signed_zeros", "all_neg_inf", "one_pos_inf", "one_nan_logit",
    "all_nan_logits", "beta_off_conv3")}
for _t in TENSORS:
    CLASSES[f"nan_{_t}"] = E32.CLASSES[f"nan_{_t}"]
for _t in ("conv1.weight", "conv2.weight", "conv3.weight", "fc1.weight", "output.weight"):
    CLASSES[f"inf_{_t}"] = E32.CLASSES[f"inf_{_t}"]
# the constant of a dead channel.  In this format the constant CANNOT show the summation order: 400 (81, 49) copies of one fp16
# value add up exactly in fp32 in any order, the mean is the value itself, d = 0 and the channel is relu(beta) whatever the bias
DEAD_BIAS = np.float32(0.0130004883)
for _k in (1, 2, 3):
    CLASSES[f"dead_conv{_k}"] = E32._dead(_k, DEAD_BIAS)
    CLASSES[f"gamma0_conv{_k}"] = E32.CLASSES[f"gamma0_conv{_k}"]
    CLASSES[f"gamma_neg_conv{_k}"] = E32.CLASSES[f"gamma_neg_conv{_k}"]
dead_channel = E32.dead_channel


# ------------------------------------------------------------------------------------------- subnormal weights
SUB_SCALE = {"sub_conv1": ("conv1.weight", 2.0 ** -12), "sub_conv2": ("conv2.weight", 2.0 ** -12),
             "sub_conv3": ("conv3.weight", 2.0 ** -12)}
SUBNORMAL = dict({k: v[0] for k, v in SUB_SCALE.items()}, sub_fc1="fc1.weight", sub_out="output.weight")


def _sub_conv(k):
    """conv k's weights x 2^-12 (fp16 subnormals, a few bits each), bias 0: sums of order 1e-5, many of them below 2^-14; the
    variance is far below eps, rstd = 1/sqrt(eps), and gamma x 32 brings the activations back to order 0.1"""
    def f(w, C, n):
        view(w, C, n, f"conv{k}.weight")[:] *= np.float32(SUB_SCALE[f"sub_conv{k}"][1])
        view(w, C, n, f"conv{k}.bias")[:] = 0.0
        view(w, C, n, f"vbn{k}.weight")[:] *= 32.0
    return f


def _subnormal_values(g, m):
    return (g.integers(1, 1024, m) * g.choice([-1.0, 1.0], m) * 2.0 ** -24).astype(np.float32)


def sub_fc1(w, C, n):
    """every fc1 weight an fp16 subnormal k 2^-24, |k| = 1 .. 1023"""
    t = view(w, C, n, "fc1.weight")
    t[:] = _subnormal_values(np.random.default_rng(4), t.size).reshape(t.shape)


def sub_out(w, C, n):
    """every output weight an fp16 subnormal, bias 0: the logits themselves are subnormal or tiny"""
    t = view(w, C, n, "output.weight")
    t[:] = _subnormal_values(np.random.default_rng(5), t.size).reshape(t.shape)
    view(w, C, n, "output.bias")[:] = 0.0


for _k in (1, 2, 3):
    CLASSES[f"sub_conv{_k}"] = _sub_conv(_k)
CLASSES.update(sub_fc1=sub_fc1, sub_out=sub_out)


# ------------------------------------------------------------------------------------------- rounding classes: conv1
# frames of bytes 0 and 255: x = 0 or 1.  Channels 3 (< 16) and 19 (>= 16: the split half unit's own store) keep ONE tap w at
# (ci = C - 1, ky, kx) = LIT_TAP and bias b: the conv sum is f16(b) off the lit positions and f16(b + w) on them
LIT_POSITIONS = (0, 15, 16, 383, 384, 399)     # of the 400: first, the tile seams, the last (the half unit's tile 24)
LIT_TAP = (5, 2)
LIT_CHANNELS = (3, 19)
CONV1_BW = {"conv1_ties_away": (1.0, 2.0 ** -11),     # 1 + 2^-11: a midpoint, to even 1.0 (the channel is constant), away 1 + 2^-10
            "conv1_flush": (0.0, 2.0 ** -15),         # 2^-15: kept as a subnormal
            "conv1_saturate": (65504.0, 16.0),        # 65520: the first fp32 that rounds to inf
            "conv1_below": (65504.0, 15.0)}           # 65519: 65504, the channel is constant and the net healthy


def lit_frame(C):
    f = np.zeros((84, 84, C), dtype=np.uint8)
    for p in LIT_POSITIONS:
        oy, ox = divmod(p, 20)
        f[4 * oy + LIT_TAP[0], 4 * ox + LIT_TAP[1], C - 1] = 255
    return f


def _conv1_one_tap(b, wt):
    def f(w, C, n):
        W, B = view(w, C, n, "conv1.weight"), view(w, C, n, "conv1.bias")
        for ch in LIT_CHANNELS:
            W[ch] = 0.0
            W[ch, C - 1, LIT_TAP[0], LIT_TAP[1]] = wt
            B[ch] = b
    return f


for _name, (_b, _w) in CONV1_BW.items():
    CLASSES[_name] = _conv1_one_tap(_b, _w)

FULL_CHANNEL = 7


def overflow_on_full(w, C, n):
    """conv1 channel 7 sums the whole patch with weight 1200 / C on bias 0: 76 800 (inf, then NaN everywhere) on the all-255
    frame, 38 400 +- a few thousand on a random frame - a net that is healthy but for ONE frame"""
    view(w, C, n, "conv1.weight")[FULL_CHANNEL] = 1200.0 / C
    view(w, C, n, "conv1.bias")[FULL_CHANNEL] = 0.0


CLASSES["overflow_on_full"] = overflow_on_full


# ------------------------------------------------------------------------------------------- rounding classes: conv2, conv3, BatchNorm
NEXT_LAYER = {1: "conv2.weight", 2: "conv3.weight", 3: "fc1.weight"}
SAT_CHANNEL = 5
SAT_SCALE = {2: 64.0, 3: 64.0}


def _bn_flush(k):
    """gamma_k x 2^-16, beta_k = 0: BatchNorm outputs of order 1e-5, most of them below 2^-14; the next layer x 2^12"""
    def f(w, C, n):
        view(w, C, n, f"vbn{k}.weight")[:] *= np.float32(2.0 ** -16)
        view(w, C, n, f"vbn{k}.bias")[:] = 0.0
        view(w, C, n, NEXT_LAYER[k])[:] *= np.float32(2.0 ** 12)
    return f


def _bn_saturate(k):
    """gamma_k x 30000: BatchNorm outputs past 65504 are inf"""
    def f(w, C, n):
        view(w, C, n, f"vbn{k}.weight")[:] *= np.float32(30000.0)
    return f


def _conv_saturate(k, bias):
    """channel SAT_CHANNEL of conv k: weights x 64 on a bias just under the largest half.  bias 65504: the sums pass 65520 (inf)
    at some positions and not at others; bias 63456 (the companion `_below`): every sum stays finite and the net healthy"""
    def f(w, C, n):
        view(w, C, n, f"conv{k}.weight")[SAT_CHANNEL] *= np.float32(SAT_SCALE[k])
        view(w, C, n, f"conv{k}.bias")[SAT_CHANNEL] = bias
    return f


for _k in (1, 2, 3):
    CLASSES[f"bn{_k}_flush"] = _bn_flush(_k)
    CLASSES[f"bn{_k}_saturate"] = _bn_saturate(_k)
for _k in (2, 3):
    CLASSES[f"conv{_k}_saturate"] = _conv_saturate(_k, 65504.0)
    CLASSES[f"conv{_k}_below"] = _conv_saturate(_k, 63456.0)


# ------------------------------------------------------------------------------------------- rounding classes: fc1 and the output layer
# exact by construction.  Six sums per group, from biases (1, 1, 0, 0, 65504, 65504) and ONE product each (two for the second):
#   1 + 2^-11            a midpoint: to even 1.0, away 1 + 2^-10
#   1 + 2^-11 + 2^-10    a midpoint: to even 1 + 2^-9, toward zero 1 + 2^-10
#   2^-15                a subnormal result, kept; flushed 0
#   2^-25                half the smallest subnormal: to even 0, away 2^-24
#   65504 + 16           inf; toward zero and saturated 65504
#   65504 + 15           65504 under every mode
# The inputs are all 0.5 (2^-25 = 2^-24 x 0.5 is no fp16 value), so the weights are twice the products.
HALF_IN = np.float32(0.5)
GROUP_BIAS = np.array([1, 1, 0, 0, 65504, 65504], dtype=np.float32)
GROUP_WORDS = np.array([1.0, 1 + 2.0 ** -9, 2.0 ** -15, 0.0, np.inf, 65504.0], dtype=np.float32)   # what the contract gives
CHANGED_BY = {"toward_zero": (1, 4), "ties_away": (0, 3), "flush_results": (2,), "saturate": (4,)}
# fc1 groups (first output, k of the critical weight): first / last k, first / last outputs of a 64-block, block 7
FC1_GROUPS = ((0, 0), (58, 3135), (448, 1567), (506, 3135), (250, 0))


def _group_weights(W, j0, k, k_max):
    k2 = k + 1 if k < k_max else k - 1
    W[j0, k] = 2.0 ** -10
    W[j0 + 1, k], W[j0 + 1, k2] = 2.0 ** -10, 2.0 ** -9
    W[j0 + 2, k] = 2.0 ** -14
    W[j0 + 3, k] = 2.0 ** -24
    W[j0 + 4, k] = 32.0
    W[j0 + 5, k] = 30.0
    return k2


def fc1_rounding(w, C, n):
    """a3 = 0.5 everywhere (vbn3.weight = 0, vbn3.bias = 0.5), fc1.weight = 0 but the critical weights: hid[j0 .. j0 + 5] =
    GROUP_WORDS for every group of FC1_GROUPS, hid = relu(fc1.bias) elsewhere.  The inf columns enter the output layer with
    weight -0.5, in row 2 with +0.5: logit 2 is +inf, the others -inf, the action 2"""
    view(w, C, n, "vbn3.weight")[:] = 0.0
    view(w, C, n, "vbn3.bias")[:] = HALF_IN
    W, b, Wo = view(w, C, n, "fc1.weight"), view(w, C, n, "fc1.bias"), view(w, C, n, "output.weight")
    W[:] = 0.0
    for j0, k in FC1_GROUPS:
        _group_weights(W, j0, k, 3135)
        b[j0:j0 + 6] = GROUP_BIAS
        Wo[:, j0 + 4] = -0.5
        Wo[2, j0 + 4] = 0.5


OUT_GROUP_K = (511, 0, 255)      # group g = logits 6 g .. 6 g + 5: the LAST fma step of the chain, the first, the middle


def out_groups(n):
    return [(6 * g, OUT_GROUP_K[g]) for g in range(min(n // 6, 3))]


def _out_rounding(first_k):
    def f(w, C, n):
        view(w, C, n, "fc1.weight")[:] = 0.0
        b = view(w, C, n, "fc1.bias")
        b[:] = 0.0
        Wo, bo = view(w, C, n, "output.weight"), view(w, C, n, "output.bias")
        Wo[:], bo[:] = 0.0, -1.0
        for g, (i0, k) in enumerate(out_groups(n)):
            k = first_k if g == 0 else k
            k2 = _group_weights(Wo, i0, k, 511)
            b[k] = b[k2] = HALF_IN
            bo[i0:i0 + 6] = GROUP_BIAS
    return f


# out_last_step: the conversion a compiler once fused into the chain's last fma.  hid[511] = 145 / 128, output.weight[1][511] =
# 113 2^-18: the last step adds 16385 2^-25 = 2^-11 + 2^-25 to 1.  Rounded to fp32 first (the contract) that is 1 + 2^-11, a
# midpoint, to even 1.0 = logit 0: a tie, action 0.  Rounded once from the exact sum it is above the midpoint: 1 + 2^-10, action 1
LAST_STEP_HID, LAST_STEP_W = np.float32(145.0 / 128.0), np.float32(113.0 * 2.0 ** -18)


def out_last_step(w, C, n):
    view(w, C, n, "fc1.weight")[:] = 0.0
    b = view(w, C, n, "fc1.bias")
    b[:] = 0.0
    b[511] = LAST_STEP_HID
    Wo, bo = view(w, C, n, "output.weight"), view(w, C, n, "output.bias")
    Wo[:], bo[:] = 0.0, -1.0
    Wo[1, 511] = LAST_STEP_W
    bo[0] = bo[1] = 1.0


def _rounding_tie(larger_second):
    """logits 1 and 3 equal only after rounding: fp32 sums 1 and 1 + 2^-12 (below the midpoint: 1.0), the larger one second - a
    scan in front of the conversion takes 3 - or, reversed, first: a last-maximum scan takes 3"""
    def f(w, C, n):
        view(w, C, n, "fc1.weight")[:] = 0.0
        b = view(w, C, n, "fc1.bias")
        b[:] = 0.0
        b[0] = HALF_IN
        Wo, bo = view(w, C, n, "output.weight"), view(w, C, n, "output.bias")
        Wo[:], bo[:] = 0.0, -1.0
        bo[1] = bo[3] = 1.0
        Wo[3 if larger_second else 1, 0] = 2.0 ** -11
    return f


CLASSES.update(fc1_rounding=fc1_rounding, out_rounding=_out_rounding(511), out_rounding_first=_out_rounding(0),
               out_last_step=out_last_step, rounding_tie=_rounding_tie(True), rounding_tie_rev=_rounding_tie(False))

TIES = {"tie_all": 0, "tie2": 1, "tie2_0_last": 0, "tie2_last2": -2, "rounding_tie": 1, "rounding_tie_rev": 1, "out_last_step": 0}
# what the checker says of each class on ANY frame: (action | None where it depends on net and frame; negative below -1: counted
# from n, NaN pattern of the logits "all" / "one" / "none" / None where it depends on the frame, status)
PROPERTY = {name: (None, "none", 0) for name in CLASSES}
PROPERTY.update({name: (a, "none", 0) for name, a in TIES.items()})
PROPERTY.update({"signed_zeros": (0, "none", 0), "all_neg_inf": (-1, "none", NO_ACTION), "one_pos_inf": (2, "none", 0),
                 "one_nan_logit": (None, "one", 0), "all_nan_logits": (-1, "all", NO_ACTION),
                 "nan_output.weight": (None, "one", 0), "nan_output.bias": (None, "one", 0), "inf_fc1.weight": (None, None, None),
                 "inf_output.weight": (None, None, None), "fc1_rounding": (2, "none", 0), "out_rounding": (4, "none", 0),
                 "out_rounding_first": (4, "none", 0)})
for _t in TENSORS:
    if not _t.startswith("output."):
        PROPERTY[f"nan_{_t}"] = (-1, "all", NO_ACTION)
for _k in (1, 2, 3):
    PROPERTY[f"inf_conv{_k}.weight"] = (-1, "all", NO_ACTION)
    PROPERTY[f"bn{_k}_saturate"] = (-1, "all", NO_ACTION)
for _k in (2, 3):
    PROPERTY[f"conv{_k}_saturate"] = (-1, "all", NO_ACTION)
# conv1_saturate is all NaN wherever its tap meets a pixel of 255 (the lit frame) or near it; on the all-zero frame it is healthy
PROPERTY["conv1_saturate"] = (None, None, None)
FAULTY = sorted(name for name, (a, nan, st) in PROPERTY.items() if st != 0)
QUIET = sorted(set(CLASSES) - set(FAULTY))
OUTPUT_SENSITIVE = ("tie_all", "tie2", "tie2_0_last", "tie2_last2", "rounding_tie", "rounding_tie_rev", "out_last_step",
                    "one_nan_logit", "all_nan_logits", "all_neg_inf", "nan_output.weight", "nan_output.bias", "out_rounding",
                    "out_rounding_first", "signed_zeros")


@functools.lru_cache(maxsize=None)
def _make(name, C, n):
    w = base_net(C, n, CLASS_SEED)
    CLASSES[name](w, C, n)
    w[:] = f16(w)
    w.flags.writeable = False
    return w


def make(name, C, n):
    """the net of class `name` (read-only and shared: the checker cache keys on it; .copy() to edit); every entry an fp16 value"""
    return _make(name, C, n)


@functools.lru_cache(maxsize=None)
def flushed(name, C, n):
    """a sub_* net as a unit that flushes subnormal operands would see it: every |entry| < 2^-14 of the class' tensor is zero"""
    w = make(name, C, n).copy()
    t = view(w, C, n, SUBNORMAL[name])
    assert (np.abs(t) < MIN_NORMAL16).all() and np.count_nonzero(t) > 0.5 * t.size, "the class' tensor is not subnormal throughout"
    t[:] = 0.0
    w.flags.writeable = False
    return w


@functools.lru_cache(maxsize=None)
def dead_with_bias(k, C, n, bias):
    w = base_net(C, n, CLASS_SEED)
    E32._dead(k, np.float32(bias))(w, C, n)
    w[:] = f16(w)
    w.flags.writeable = False
    return w


def edge_nets(C, n):
    """the five nets of tests/test_fp16_dqn_gpu.py and tests/test_fp16_dqn_tiled_gpu.py: fc1 weights all fp16-subnormal, the same
    net with fc1.weight = 0, fc1 output 0 past 65504, a hand-made tie, conv1 sums past 65504"""
    torch.manual_seed(9)
    base = ck.half_net(C, n, 0.02)
    g = np.random.default_rng(4)
    sub = base.copy()
    t = view(sub, C, n, "fc1.weight").reshape(-1)
    t[:] = (g.integers(1, 1024, t.size) * g.choice([-1.0, 1.0], t.size) * 2.0 ** -24).astype(np.float32)
    zero = sub.copy()
    view(zero, C, n, "fc1.weight")[:] = 0.0
    big = base.copy()
    view(big, C, n, "fc1.weight")[0] = 60000.0
    tie = base.copy()
    view(tie, C, n, "output.weight")[:] = 0.0
    view(tie, C, n, "output.bias")[:] = np.array([0.125, 0.25, 0.5, 0.375, 0.5, 0.125], dtype=np.float32)
    over = base.copy()
    view(over, C, n, "conv1.weight")[:] = 60000.0
    return sub, zero, big, tie, over


# ------------------------------------------------------------------------------------------- frames
@functools.lru_cache(maxsize=None)
def seq_frames(C):
    """the seeded sequence of 64 random frames the ties_away search walks"""
    f = np.random.Generator(np.random.PCG64([C, 16])).integers(0, 256, size=(64, 84, 84, C), dtype=np.uint8)
    f.flags.writeable = False
    return f


@functools.lru_cache(maxsize=None)
def _frames(C):
    out = dict(E32.FRAMES(C), lit=lit_frame(C))
    out["lit"].flags.writeable = False
    return out


def frame(C, name):
    """a named frame: those of dqn_edge_nets.FRAMES, "lit", "seq<i>" = frame i of seq_frames"""
    return seq_frames(C)[int(name[3:])] if name.startswith("seq") else _frames(C)[name]


# ------------------------------------------------------------------------------------------- the (site, mode) pairs
SHAPES = ((4, 6), (6, 18), (3, 6), (5, 18))
# first frame of seq_frames(C) on which ties-away at the site shows in act / hid / logits of the plain net (found with
# first_tie_frame below, at most 64 frames looked at; tests/test_dqn16_edges_cpu.py asserts that each one shows)
TIES_AWAY_FRAME = {(4, 6): {"conv1": 1, "bn1": 1, "conv2": 4, "bn2": 4, "conv3": 16, "bn3": 24},
                   (6, 18): {"conv1": 4, "bn1": 4, "conv2": 4, "bn2": 6, "conv3": 2, "bn3": 9},
                   (3, 6): {"conv1": 1, "bn1": 2, "conv2": 0, "bn2": 12, "conv3": 1, "bn3": 7},
                   (5, 18): {"conv1": 2, "bn1": 0, "conv2": 7, "bn2": 2, "conv3": 17, "bn3": 25}}
VACUOUS = (("quotient", "ties_away"), ("quotient", "flush_results"), ("quotient", "saturate"))
VISIBLE = ("a3", "hid", "logits")     # the stages a launch leaves behind (workspace act and hid, logits), and the action


def rounding_rows(C, n):
    """(site, mode) -> [(class, frame name)]: rows on which the checker under that variant differs from the contract in the
    GPU-visible words.  33 pairs: nine sites x four wrong modes without the three VACUOUS ones"""
    tf = TIES_AWAY_FRAME[(C, n)]
    rows = {(s, "toward_zero"): [("plain", "random")] for s in SITES[:7]}
    rows[("conv1", "ties_away")] = [("conv1_ties_away", "lit"), ("plain", f"seq{tf['conv1']}")]
    rows[("conv1", "flush_results")] = [("conv1_flush", "lit"), ("sub_conv1", "random")]
    rows[("conv1", "saturate")] = [("conv1_saturate", "lit")]
    for k in (1, 2, 3):
        rows[(f"bn{k}", "ties_away")] = [("plain", f"seq{tf[f'bn{k}']}")]
        rows[(f"bn{k}", "flush_results")] = [(f"bn{k}_flush", "random")]
        rows[(f"bn{k}", "saturate")] = [(f"bn{k}_saturate", "random")]
    for k in (2, 3):
        rows[(f"conv{k}", "ties_away")] = [("plain", f"seq{tf[f'conv{k}']}")]
        rows[(f"conv{k}", "flush_results")] = [(f"sub_conv{k}", "random")]
        rows[(f"conv{k}", "saturate")] = [(f"conv{k}_saturate", "random")]
    for m in WRONG_MODES:
        rows[("fc1", m)] = [("fc1_rounding", "random")]
        rows[("out", m)] = [("out_rounding", "random"), ("out_rounding_first", "random")]
    rows[("out", "ties_away")].append(("out_last_step", "random"))
    assert len(rows) == 33 and not set(rows) & set(VACUOUS)
    return rows


def shows(want, got):
    """the variant's stages differ from the contract's in a GPU-visible word"""
    return want["action"] != got["action"] or any(not same_bits_up_to_nan(want[k], got[k]) for k in VISIBLE)


def first_tie_frame(C, n, site, limit=64):
    """index of the first frame of seq_frames(C) on which ties-away at `site` shows for the plain net (None: none of `limit`)"""
    w = make("plain", C, n)
    for i in range(limit):
        f = seq_frames(C)[i]
        if shows(ck.stages(w, C, n, f), ck.stages(w, C, n, f, site, "ties_away")):
            return i
    return None


def class_rows(C, n):
    """every (class, frame name) row of the catalogue: each class on the random frame, the conv1 one-tap classes on the lit
    frame, the plain net on every named frame, and every row of rounding_rows"""
    rows = [(name, "random") for name in sorted(CLASSES)]
    rows += [(name, "lit") for name in CONV1_BW] + [("plain", f) for f in ("zeros", "full", "planes", "hot_first", "hot_last", "lit")]
    for rr in rounding_rows(C, n).values():
        rows += [r for r in rr if r not in rows]
    return rows


# ------------------------------------------------------------------------------------------- the checker, cached
_CHECKER = {}
N_CHECKER_CALLS = 0


def _forward(net, C, n, frame_u8):
    s = ck.stages(net, C, n, frame_u8)
    out = {"act": s["a3"].reshape(-1), "hid": s["hid"], "logits": s["logits"], "action": s["action"], "status": s["status"]}
    for k in ("act", "hid", "logits"):
        out[k].flags.writeable = False
    return out


def checker_many(pairs, C, n):
    """[(net, frame)] -> [dict(act [3136], hid [512], logits [n], action, status)]: the contract's stages once per distinct
    pair, the missing ones on a few threads (the C call releases the interpreter lock)"""
    global N_CHECKER_CALLS
    ck.lib()
    keys = [(digest(net), digest(f), n) for net, f in pairs]
    todo = {}
    for k, p in zip(keys, pairs):
        if k not in _CHECKER:
            todo.setdefault(k, p)
    if todo:
        N_CHECKER_CALLS += len(todo)
        with ThreadPoolExecutor(max(1, min(8, len(todo), len(os.sched_getaffinity(0))))) as ex:
            for k, r in zip(todo, ex.map(lambda p: _forward(p[0], C, n, p[1]), todo.values())):
                _CHECKER[k] = r
    return [_CHECKER[k] for k in keys]


def checker(net, frame_u8, C, n):
    return checker_many([(net, frame_u8)], C, n)[0]


def release():
    """drop the cached nets (7 MB each); checker results stay"""
    for f in (_base, _make, flushed, dead_with_bias):
        f.cache_clear()
    E32._DIGEST.clear()


# ------------------------------------------------------------------------------------------- one launch
def tile_rows(spec):
    """[(net index, rows)] -> tasks [(net index, row_begin, n_rows)] that tile the rows.  rows outside 1 .. 16 make a task the
    forward refuses (COEVO_ST_BAD_TASK): it still owns max(rows, 1) rows, which nobody writes"""
    out, row = [], 0
    for net, r in spec:
        out.append((net, row, r))
        row += max(r, 1)
    return out, row


def served_rows(tasks, n_rows):
    """net index of every row, None for a row no served task owns"""
    out = [None] * n_rows
    for net, begin, r in tasks:
        if 1 <= r <= 16:
            out[begin:begin + r] = [net] * r
    return out


def pack(nets, C, n, tiled):
    from coevonet_amd import lib as L
    stride = int(L.load().coevo_dqn16_slab_stride(C, n))
    flat = torch.from_numpy(np.ascontiguousarray(np.stack(nets), dtype=np.float32)).to("cuda")
    slab = torch.full((len(nets) * stride,), POISON_I32, dtype=torch.int32, device="cuda")
    L.call("coevo_dqn16_pack_tiled" if tiled else "coevo_dqn16_pack", L._p(flat), L._p(slab), len(nets), C, n)
    return slab, stride


def launch(tasks, nets, frames, C, n, tiled, preset_status=0, hidden_only=False):
    """one coevo_dqn16_forward_argmax[_tiled] (hidden_only: coevo_dqn16_forward_hidden[_tiled]) over `nets` packed into a slab of
    the fc1 form `tiled`, tasks = [(net index, row_begin, n_rows)], frames [rows][84][84][C] uint8, on a NaN workspace and
    0x7f7f7f7f logits and action words -> dict(rc, act [rows, 3136], hid [rows, 512], logits [rows, 32], actions, status) and the
    device buffers (slab, d_tasks, ws) for a launch that goes on from them"""
    from coevonet_amd import lib as L
    lib, dev = L.load(), "cuda"
    slab, stride = pack(nets, C, n, tiled)
    frames = np.ascontiguousarray(frames)
    rows = len(frames)
    assert frames.shape == (rows, 84, 84, C) and frames.dtype == np.uint8
    t = np.zeros(len(tasks), dtype=L.DQN_TASK_DTYPE)
    for i, (net, begin, r) in enumerate(tasks):
        assert 0 <= net < len(nets) and 0 <= begin and begin + max(r, 0) <= rows
        t[i] = (net * stride, begin, r)
    d_tasks, d_frames = L.tasks_to_device(t, dev), torch.from_numpy(frames).to(dev)
    ws = torch.full((int(lib.coevo_dqn16_workspace_bytes(rows)) // 4,), float("nan"), dtype=torch.float32, device=dev)
    lg = torch.full((rows, L.DQN_LOGIT_STRIDE), POISON_I32, dtype=torch.int32, device=dev).view(torch.float32)
    act = torch.full((rows,), POISON_I32, dtype=torch.int32, device=dev)
    status = torch.full((1,), int(preset_status), dtype=torch.int32, device=dev)
    head = (L._p(slab), L._p(d_tasks), len(tasks), min(max(1, max(r for _, _, r in tasks)), 16), rows, C, n, L._p(d_frames))
    sfx = "_tiled" if tiled else ""
    if hidden_only:
        rc = getattr(lib, "coevo_dqn16_forward_hidden" + sfx)(*head, L._p(status), L._p(ws), L._stream())
    else:
        rc = getattr(lib, "coevo_dqn16_forward_argmax" + sfx)(*head, L._p(act), L._p(lg), L._p(status), L._p(ws), L._stream())
    torch.cuda.synchronize()
    w = ws.cpu().numpy()
    return {"rc": int(rc), "act": w[:rows * 3136].reshape(rows, 3136), "hid": w[rows * 3136:].reshape(rows, 512),
            "logits": lg.cpu().numpy(), "actions": act.cpu().numpy(), "status": int(status.item()),
            "dev": dict(slab=slab, tasks=d_tasks, ws=ws, stride=stride)}


def expected(tasks, nets, frames, C, n):
    """the checker's dict of every served row (None for a row nobody writes) and the status word the launch must add"""
    owner = served_rows(tasks, len(frames))
    got = iter(checker_many([(nets[k], frames[i]) for i, k in enumerate(owner) if k is not None], C, n))
    want = [None if k is None else next(got) for k in owner]
    status = BAD_TASK if any(not 1 <= r <= 16 for _, _, r in tasks) else 0
    for w in want:
        status |= w["status"] if w is not None else 0
    return want, status


def assert_rows(out, want, n, what="", hidden_only=False):
    """every served row: all 3136 conv3 activations, all 512 hidden words and the n logits bit for bit (a NaN matches any NaN),
    the action, the logits past n still poison; every other row: workspace NaN, logits and action poison"""
    assert len(want) == len(out["act"]) == len(out["hid"]) == len(out["logits"]) == len(out["actions"])
    lg_words = out["logits"].view(np.uint32)
    for r, w in enumerate(want):
        if w is None:
            assert np.isnan(out["act"][r]).all() and np.isnan(out["hid"][r]).all(), f"{what} row {r}: an unserved row's workspace"
        else:
            assert same_bits_up_to_nan(out["act"][r], w["act"]), f"{what} row {r}: conv3 activations"
            assert same_bits_up_to_nan(out["hid"][r], w["hid"]), f"{what} row {r}: hidden row"
        if w is None or hidden_only:
            assert (lg_words[r] == POISON_I32).all() and out["actions"][r] == POISON_I32, f"{what} row {r}: logits / action written"
            continue
        assert same_bits_up_to_nan(out["logits"][r, :n], w["logits"]), f"{what} row {r}: logits {out['logits'][r, :n]} vs {w['logits']}"
        assert (lg_words[r, n:] == POISON_I32).all(), f"{what} row {r}: logits past n_actions were written"
        assert out["actions"][r] == w["action"], f"{what} row {r}: action {out['actions'][r]} vs {w['action']} ({w['logits']})"
