"""Adversarial DeepQN parameter vectors and frames for the fp32 DeepQN forward, with the oracle as the only judge.

Every net is base_net(C, n, seed) = rp.dqn_mutate_torch(*rp.dqn_init(C, n), 0.02) with entries of the canonical flat vector
overwritten (parameters() order, offsets as oracle_dqn_forward reads them).  Nothing here knows what a kernel returns: the
expected logits and action of a (net, frame) pair always come from rp.dqn_forward through the cache below; PROPERTY only says
what tests/test_dqn_edges_cpu.py pins of the oracle itself.  The module needs no GPU and no libcoevo: launch() imports torch's
device side and coevonet_amd.lib when it is called (tests/test_dqn_forward_edges_gpu.py)."""
import functools
import hashlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from coevonet_amd import lib as L
from oracle import ref_port as rp
from tests.fc_edge_nets import last_maximum, same_bits_up_to_nan   # noqa: F401  (re-exported for the two test files)

NO_ACTION = L.K["COEVO_ST_NO_ACTION"]   # the only bit the DeepQN forward raises
MIN_NORMAL = np.float32(2.0 ** -126)
SENT_A, SENT_L = -7, np.float32(777.0)
TENSORS = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias", "fc1.weight",
           "fc1.bias", "output.weight", "output.bias", "vbn1.weight", "vbn1.bias", "vbn2.weight", "vbn2.bias",
           "vbn3.weight", "vbn3.bias")


def shapes(C, n):
    return [(32, C, 8, 8), (32,), (64, 32, 4, 4), (64,), (64, 64, 3, 3), (64,), (512, 3136), (512,), (n, 512), (n,),
            (32,), (32,), (64,), (64,), (64,), (64,)]


@functools.lru_cache(maxsize=None)
def offsets(C, n):
    """name -> (offset, shape) in the canonical flat vector"""
    out, off = {}, 0
    for name, shp in zip(TENSORS, shapes(C, n)):
        out[name] = (off, shp)
        off += int(np.prod(shp))
    assert off == rp.lib().oracle_dqn_param_count(C, n)
    return out


def view(flat, C, n, name):
    """writable view of one parameter tensor inside `flat`"""
    off, shp = offsets(C, n)[name]
    return flat[off:off + int(np.prod(shp))].reshape(shp)


@functools.lru_cache(maxsize=None)
def _base(C, n, seed):
    torch.manual_seed(seed)
    w = rp.dqn_mutate_torch(*rp.dqn_init(C, n), 0.02)
    w.flags.writeable = False
    return w


def base_net(C, n, seed):
    """a healthy net: fresh initialisation plus N(0, 0.02) on every entry (the BatchNorm affine included)"""
    return _base(C, n, seed).copy()


# ------------------------------------------------------------------------------------------- the classes
def tie_all(w, C, n):
    """every logit 0.25: the first of them is the action"""
    view(w, C, n, "output.weight")[:] = 0.0
    view(w, C, n, "output.bias")[:] = 0.25


def tie2(w, C, n, i=1, j=3):
    """logits i < j bit-equal (row j of the output layer is a copy of row i) and far above the rest"""
    i, j = i % n, j % n
    assert i < j
    Wo, bo = view(w, C, n, "output.weight"), view(w, C, n, "output.bias")
    Wo[j], bo[j] = Wo[i], bo[i]
    for o in range(n):
        if o not in (i, j):
            bo[o] = -1e3


def signed_zeros(w, C, n):
    """logits -0, +0, -0, +0, ...: output.w = 0 carrying its row's sign, so that the fmaf chain keeps the bias' zero"""
    sign = np.where(np.arange(n) % 2 == 0, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    view(w, C, n, "output.weight")[:] = sign[:, None]
    view(w, C, n, "output.bias")[:] = sign


def all_neg_inf(w, C, n):
    view(w, C, n, "output.weight")[:] = 0.0
    view(w, C, n, "output.bias")[:] = -np.inf


def one_pos_inf(w, C, n):
    view(w, C, n, "output.bias")[2] = np.inf


def one_nan_logit(w, C, n):
    view(w, C, n, "output.bias")[0] = np.nan


def all_nan_logits(w, C, n):
    view(w, C, n, "output.bias")[:] = np.nan


def _poke(name, value):
    """one entry of the tensor (in its middle, never the first one) set to `value`"""
    def f(w, C, n):
        t = view(w, C, n, name).reshape(-1)
        t[t.size // 2 + 1 if t.size > 2 else t.size - 1] = value
    return f


def _overflow_conv(k):
    """conv k's weights and bias x 1e38 (finite each): the strided sums of BatchNorm reach inf, d = x - inf, d * rstd with
    rstd = 1/sqrt(inf) = 0 is NaN"""
    def f(w, C, n):
        view(w, C, n, f"conv{k}.weight")[:] *= np.float32(1e38)
        view(w, C, n, f"conv{k}.bias")[:] *= np.float32(1e38)
    return f


def overflow_fc1(w, C, n):
    """fc1.w x 1e37: hidden values and logits of order 1e36 .. 1e37, finite on every named frame (x 1e38 takes the hidden
    layer to inf on the hot-byte frames, whose BatchNorm images have one large entry)"""
    view(w, C, n, "fc1.weight")[:] *= np.float32(1e37)


# the constant of dead_conv<k>: the channel's conv output is this value at every position, so d = x - S / N is the rounding
# residue of the canonical strided-sum and tree order (400, 81, 49 positions), scaled by 1/sqrt(1e-5).  Chosen on the oracle
# (tests/test_dqn_edges_cpu.py asserts the residue shows in the logits, for conv1 as a MUST)
DEAD_BIAS = {1: np.float32(0.013), 2: np.float32(0.013), 3: np.float32(0.011)}


def dead_channel(w, C, n, k):
    """the channel dead_conv<k> switches off: the first one past 0 whose BatchNorm affine lets the residue through ReLU"""
    g, b = view(w, C, n, f"vbn{k}.weight"), view(w, C, n, f"vbn{k}.bias")
    for ch in range(1, len(g)):
        if g[ch] > 0.5 and b[ch] > 0.005:
            return ch
    raise AssertionError("no channel with a positive BatchNorm shift")


def _dead(k, bias=None):
    def f(w, C, n):
        ch = dead_channel(w, C, n, k)
        view(w, C, n, f"conv{k}.weight")[ch] = 0.0
        view(w, C, n, f"conv{k}.bias")[ch] = DEAD_BIAS[k] if bias is None else bias
    return f


def _gamma(k, how):
    def f(w, C, n):
        g = view(w, C, n, f"vbn{k}.weight")
        g[:] = 0.0 if how == "zero" else -g
    return f


def beta_off_conv3(w, C, n):
    """|d * rstd| <= sqrt(49) = 7 and gamma ~ 1: with beta = -10 every conv3 activation is 0, the logits come from fc1.b"""
    view(w, C, n, "vbn3.bias")[:] = -10.0


# subnormal classes: name -> (the tensor that is scaled, its scale).  The scales are the ones tried on the oracle
SUB_SCALE = {"sub_conv1": ("conv1.weight", 2.0 ** -125), "sub_conv2": ("conv2.weight", 2.0 ** -125),
             "sub_conv3": ("conv3.weight", 2.0 ** -125), "sub_fc1": ("fc1.weight", 2.0 ** -128),
             "sub_out": ("output.weight", 2.0 ** -130)}
SUB_GAMMA, SUB_OUT_SCALE = np.float32(2.0 ** 110), np.float32(2.0 ** 120)


def _sub_conv(k):
    """conv k's weights x 2^-125 (subnormal, as is every product and sum of the layer), bias 0; (x - mean)^2 underflows, the
    variance is 0, rstd = 1/sqrt(eps), and gamma = 2^110 brings the activations back into the normal range"""
    def f(w, C, n):
        view(w, C, n, f"conv{k}.weight")[:] *= np.float32(SUB_SCALE[f"sub_conv{k}"][1])
        view(w, C, n, f"conv{k}.bias")[:] = 0.0
        view(w, C, n, f"vbn{k}.weight")[:] = SUB_GAMMA
        view(w, C, n, f"vbn{k}.bias")[:] = 0.0
    return f


def sub_fc1(w, C, n):
    """fc1.w x 2^-128: every hidden value subnormal; output.w x 2^120 brings the logits back"""
    view(w, C, n, "fc1.weight")[:] *= np.float32(SUB_SCALE["sub_fc1"][1])
    view(w, C, n, "fc1.bias")[:] = 0.0
    view(w, C, n, "output.weight")[:] *= SUB_OUT_SCALE


def sub_out(w, C, n):
    """output.w x 2^-130, output.b = 0: the logits themselves are subnormal"""
    view(w, C, n, "output.weight")[:] *= np.float32(SUB_SCALE["sub_out"][1])
    view(w, C, n, "output.bias")[:] = 0.0


CLASSES = {"plain": lambda w, C, n: None, "tie_all": tie_all, "tie2": tie2,
           "tie2_0_last": lambda w, C, n: tie2(w, C, n, 0, n - 1), "tie2_last2": lambda w, C, n: tie2(w, C, n, n - 2, n - 1),
           "signed_zeros": signed_zeros, "all_neg_inf": all_neg_inf, "one_pos_inf": one_pos_inf, "one_nan_logit": one_nan_logit,
           "all_nan_logits": all_nan_logits, "overflow_fc1": overflow_fc1, "beta_off_conv3": beta_off_conv3,
           "sub_fc1": sub_fc1, "sub_out": sub_out}
for _t in TENSORS:
    CLASSES[f"nan_{_t}"] = _poke(_t, np.nan)
for _t in ("conv1.weight", "conv2.weight", "conv3.weight", "fc1.weight", "output.weight"):
    CLASSES[f"inf_{_t}"] = _poke(_t, np.inf)
for _k in (1, 2, 3):
    CLASSES[f"overflow_conv{_k}"] = _overflow_conv(_k)
    CLASSES[f"dead_conv{_k}"] = _dead(_k)
    CLASSES[f"gamma0_conv{_k}"] = _gamma(_k, "zero")
    CLASSES[f"gamma_neg_conv{_k}"] = _gamma(_k, "neg")
    CLASSES[f"sub_conv{_k}"] = _sub_conv(_k)

TIES = {"tie_all": 0, "tie2": 1, "tie2_0_last": 0, "tie2_last2": -2}     # class -> its action (negative: counted from n)
# what the oracle says of each class on ANY frame: (action | None where it depends on net and frame, NaN pattern of the logits:
# "all", "one", "none", or None where it depends on the frame - an inf weight meets a zero or a positive activation)
PROPERTY = {name: (None, "none") for name in CLASSES}
PROPERTY.update({name: (a, "none") for name, a in TIES.items()})
PROPERTY.update({"signed_zeros": (0, "none"), "all_neg_inf": (-1, "none"), "one_pos_inf": (2, "none"),
                 "one_nan_logit": (None, "one"), "all_nan_logits": (-1, "all"), "nan_output.weight": (None, "one"),
                 "nan_output.bias": (None, "one"), "inf_fc1.weight": (None, None), "inf_output.weight": (None, None)})
for _t in TENSORS:
    if not _t.startswith("output."):
        PROPERTY[f"nan_{_t}"] = (-1, "all")
for _k in (1, 2, 3):
    PROPERTY[f"inf_conv{_k}.weight"] = (-1, "all")
    PROPERTY[f"overflow_conv{_k}"] = (-1, "all")
NO_FAULT = sorted(name for name, (a, nan) in PROPERTY.items() if a != -1 and nan is not None)   # never raise NO_ACTION
MAY_FAULT = sorted(set(CLASSES) - set(NO_FAULT))
DEAD = ("dead_conv1", "dead_conv2", "dead_conv3")
CLASS_SEED = 1000


@functools.lru_cache(maxsize=None)
def _make(name, C, n, seed):
    w = base_net(C, n, CLASS_SEED + seed)
    CLASSES[name](w, C, n)
    w.flags.writeable = False
    return w


def make(name, C, n, seed=0):
    """the net of class `name` (read-only and shared: the oracle cache keys on it; .copy() to edit)"""
    return _make(name, C, n, seed)


@functools.lru_cache(maxsize=None)
def flushed(name, C, n, seed=0):
    """a sub_* net as a unit that flushes subnormal operands or results would see it: the scaled tensor is zero"""
    w = make(name, C, n, seed).copy()
    t = view(w, C, n, SUB_SCALE[name][0])
    assert (np.abs(t) < MIN_NORMAL).all() and np.count_nonzero(t) > 0.99 * t.size, "the class' tensor is not subnormal throughout"
    t[:] = 0.0
    w.flags.writeable = False
    return w


@functools.lru_cache(maxsize=None)
def dead_with_bias(k, C, n, bias, seed=0):
    """dead_conv<k> with another constant in the dead channel (0: d is exactly zero, nothing of the summation order shows)"""
    w = base_net(C, n, CLASS_SEED + seed)
    _dead(k, np.float32(bias))(w, C, n)
    w.flags.writeable = False
    return w


def healthy(C, n, k):
    """healthy net k = 0 .. 3 of the ragged and filler rows"""
    return _base(C, n, 10 + k)


# ------------------------------------------------------------------------------------------- frames
def FRAMES(C, seed=0):
    """named uint8 frames [84][84][C]"""
    g = np.random.Generator(np.random.PCG64([C, seed, 1]))
    out = {"random": g.integers(0, 256, size=(84, 84, C), dtype=np.uint8), "zeros": np.zeros((84, 84, C), dtype=np.uint8),
           "full": np.full((84, 84, C), 255, dtype=np.uint8),
           "planes": np.broadcast_to((17 + 40 * np.arange(C)).astype(np.uint8), (84, 84, C)).copy(),
           "hot_first": np.zeros((84, 84, C), dtype=np.uint8), "hot_last": np.zeros((84, 84, C), dtype=np.uint8)}
    out["hot_first"][0, 0, 0] = 255
    out["hot_last"][83, 83, C - 1] = 255      # the last byte of the frame: only conv1's last output position reads it
    for f in out.values():
        f.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def ragged_frames(C):
    """the 16 random frames of the ragged and filler rows: row i of a task shows frame i"""
    g = np.random.Generator(np.random.PCG64([C, 2]))
    f = g.integers(0, 256, size=(16, 84, 84, C), dtype=np.uint8)
    f.flags.writeable = False
    return f


# ------------------------------------------------------------------------------------------- the oracle, cached
_DIGEST, _ORACLE = {}, {}
N_ORACLE_CALLS = 0


def digest(a):
    """content key of an array; a net (megabytes) is hashed once and frozen, so that the key stays true"""
    assert a.flags.c_contiguous
    if a.nbytes < (1 << 20):
        return hashlib.blake2b(a.view(np.uint8).reshape(-1), digest_size=16).digest()
    e = _DIGEST.get(id(a))
    if e is None or e[0] is not a:
        a.flags.writeable = False
        e = _DIGEST[id(a)] = (a, hashlib.blake2b(a.view(np.uint8).reshape(-1), digest_size=16).digest())
    return e[1]


def _forward(net, C, n, frame):
    a, lg = rp.dqn_forward(net, C, n, frame)
    lg.flags.writeable = False
    return a, lg


def oracle_many(pairs, C, n):
    """[(net, frame)] -> [(action, logits)]: rp.dqn_forward once per distinct pair, the missing ones on a few threads
    (the C call releases the interpreter lock)"""
    global N_ORACLE_CALLS
    rp.lib()
    keys = [(digest(net), digest(frame), n) for net, frame in pairs]
    todo = {}
    for k, p in zip(keys, pairs):
        if k not in _ORACLE:
            todo.setdefault(k, p)
    if todo:
        N_ORACLE_CALLS += len(todo)
        with ThreadPoolExecutor(max(1, min(8, len(todo), len(os.sched_getaffinity(0))))) as ex:
            for k, r in zip(todo, ex.map(lambda p: _forward(p[0], C, n, p[1]), todo.values())):
                _ORACLE[k] = r
    return [_ORACLE[k] for k in keys]


def oracle(net, frame, C, n):
    return oracle_many([(net, frame)], C, n)[0]


def release():
    """drop the cached nets (7 MB each, about a hundred of them by the end of a test module); oracle results stay"""
    for f in (_base, _make, flushed, dead_with_bias):
        f.cache_clear()
    _DIGEST.clear()


# ------------------------------------------------------------------------------------------- one launch
def task_table(layout, stride):
    """layout = [(net index, rows), ...] in ascending row order -> (coevo_dqn_task records, net index of every row)"""
    from coevonet_amd import lib as L
    tasks = np.zeros(len(layout), dtype=L.DQN_TASK_DTYPE)
    net_of_row, row = [], 0
    for i, (net, r) in enumerate(layout):
        assert 1 <= r <= L.DQN_MAX_ROWS
        tasks[i] = (net * stride, row, r)
        net_of_row += [net] * r
        row += r
    return tasks, net_of_row


def launch(layout, nets, frames, C, n, tiled=0, preset_status=0):
    """one coevo_dqn_forward_argmax over `nets` packed into a slab of the fc1 layout `tiled` (0 or L.DQN_FC1_TILED), the task
    table built from layout = [(net index, rows), ...] in ascending row order, frames [rows][84][84][C] uint8.
    -> (logits [rows][n], actions [rows], status word, return code); never raises on a non-zero status word.  The logits
    columns past n must keep the sentinel they start with (asserted here)."""
    from coevonet_amd import lib as L
    lib, dev = L.load(), "cuda"
    stride = int(lib.coevo_dqn_slab_stride(C, n))
    tasks, net_of_row = task_table(layout, stride)
    rows = len(net_of_row)
    frames = np.ascontiguousarray(frames)
    assert frames.shape == (rows, 84, 84, C) and frames.dtype == np.uint8 and max(net_of_row) < len(nets)
    flat = torch.from_numpy(np.stack(nets)).to(dev)
    slab = torch.zeros(len(nets), stride, dtype=torch.float32, device=dev)
    L.call("coevo_dqn_pack", L._p(flat), L._p(slab), len(nets), C | tiled, n)
    d_tasks = L.tasks_to_device(tasks, dev)
    d_frames = torch.from_numpy(frames).to(dev)
    actions = torch.full((rows,), SENT_A, dtype=torch.int32, device=dev)
    logits = torch.full((rows, L.DQN_LOGIT_STRIDE), float(SENT_L), dtype=torch.float32, device=dev)
    status = torch.full((1,), int(preset_status), dtype=torch.int32, device=dev)
    ws = torch.zeros(int(lib.coevo_dqn_workspace_bytes(rows)) // 4, dtype=torch.float32, device=dev)
    rc = lib.coevo_dqn_forward_argmax(L._p(slab), L._p(d_tasks), len(layout), max(r for _, r in layout), rows, C | tiled, n,
                                      L._p(d_frames), L._p(actions), L._p(logits), L._p(status), L._p(ws), L._stream())
    torch.cuda.synchronize()
    got = logits.cpu().numpy()
    assert (got[:, n:] == SENT_L).all(), "logits columns past n_actions were written"
    return np.ascontiguousarray(got[:, :n]), actions.cpu().numpy(), int(status.item()), int(rc)


def expected(layout, nets, frames, C, n):
    """the oracle's (action, logits) of every row of a launch, and the status word its actions imply (no action: NO_ACTION)"""
    net_of_row = [net for net, r in layout for _ in range(r)]
    want = oracle_many([(nets[k], frames[i]) for i, k in enumerate(net_of_row)], C, n)
    return want, (NO_ACTION if any(a < 0 for a, _ in want) else 0)


def assert_rows(got_logits, got_actions, want, what=""):
    """every row: logits bit for bit (uint32 patterns; a NaN matches any NaN: the two machines' default NaNs differ), the
    oracle's action, with the oracle's -1 (nothing compares greater than -inf) stored as action 0"""
    assert len(want) == len(got_logits) == len(got_actions)
    for r, (a, lg) in enumerate(want):
        assert same_bits_up_to_nan(got_logits[r], lg), f"{what} row {r}: logits {got_logits[r]} vs oracle {lg}"
        assert got_actions[r] == max(a, 0), f"{what} row {r}: action {got_actions[r]} vs oracle {a} (logits {lg})"
