"""Adversarial FCNetwork parameter vectors and observations for the fp32 policy forward, with the oracle as the only judge.

Every net is rp.init_net(D) with entries of the flat vector overwritten (canonical order, offsets as oracle_fc_forward reads
them).  Nothing here knows what a kernel returns: the expected logits / action / status of a class always come from
rp.fc_forward at the place of use; PROPERTY only says what tests/test_fc_edges_cpu.py pins of the oracle itself.
No GPU and no libcoevo needed: tests/test_fc_forward_edges_gpu.py imports the library from here."""
import numpy as np
import torch

from coevonet_amd import lib as L
from oracle import ref_port as rp

H1, H2, NACT = rp.H1, rp.H2, rp.NACT
BAD_INPUT, BAD_FC1, BAD_FC2, BAD_OUT, NO_ACTION, SYNC_TIMEOUT = (
    L.K["COEVO_ST_" + n] for n in ("BAD_INPUT", "BAD_FC1", "BAD_FC2", "BAD_OUT", "NO_ACTION", "SYNC_TIMEOUT"))
MIN_NORMAL = np.float32(2.0 ** -126)


def offsets(D):
    """name -> (offset, shape) in the flat vector"""
    out, off = {}, 0
    for name, shp in rp.param_shapes(D):
        out[name] = (off, shp)
        off += int(np.prod(shp))
    return out


def view(flat, D, name):
    """writable view of one parameter tensor inside `flat`"""
    off, shp = offsets(D)[name]
    return flat[off:off + int(np.prod(shp))].reshape(shp)


def base_net(D, seed):
    torch.manual_seed(seed)
    return rp.init_net(D)


# ------------------------------------------------------------------------------------------- the classes
def tie2(w, D, i=1, j=3):
    """logits i and j bit-equal and far above the rest: the first of them is the action"""
    W3, b3 = view(w, D, "output.weight"), view(w, D, "output.bias")
    W3[j], b3[j] = W3[i], b3[i]
    for o in range(NACT):
        if o not in (i, j):
            b3[o] = -1e3


def tie5(w, D):
    view(w, D, "output.weight")[:] = 0.0
    view(w, D, "output.bias")[:] = 0.25


def signed_zeros(w, D):
    """logits (-0, +0, -0, +0, +0): W3 = 0 carrying its row's sign, so that the fmaf chain keeps the bias' zero"""
    sign = np.array([-0.0, 0.0, -0.0, 0.0, 0.0], dtype=np.float32)
    view(w, D, "output.weight")[:] = sign[:, None]
    view(w, D, "output.bias")[:] = sign


def all_neg_inf(w, D):
    view(w, D, "output.weight")[:] = 0.0
    view(w, D, "output.bias")[:] = -np.inf


def one_pos_inf(w, D):
    view(w, D, "output.bias")[2] = np.inf


def one_nan_logit(w, D):
    view(w, D, "output.bias")[0] = np.nan


def all_nan_logits(w, D):
    view(w, D, "output.bias")[:] = np.nan


def nan_in_fc2(w, D):
    view(w, D, "fc2.weight")[77, 301] = np.nan


def fc2_overflow(w, D):
    W2 = view(w, D, "fc2.weight")
    W2[:] = np.where(W2 < 0, np.float32(-3e38), np.float32(3e38))


def nan_in_fc1(w, D):
    view(w, D, "fc1.weight")[5, D - 1] = np.nan


def zero_variance(w, D):
    """every fc1 output equal: LayerNorm(512) sees variance 0, rstd = 1/sqrt(eps)"""
    view(w, D, "fc1.weight")[:] = 0.0
    view(w, D, "fc1.bias")[:] = 0.5


def subnormal_fc2(w, D):
    """every fc2 weight subnormal (|w| <= 1/sqrt(512) * 1e-38), brought back by ln2.w = 1e30: logits of order 1e-7"""
    view(w, D, "fc2.weight")[:] *= np.float32(1e-38)
    view(w, D, "fc2.bias")[:] = 0.0
    view(w, D, "ln2.weight")[:] = 1e30
    view(w, D, "output.bias")[:] = 0.0


def subnormal_fc1(w, D):
    """every fc1 weight subnormal, so every fc1 product of an order-1 observation is; (x - mean)^2 underflows, the variance
    is 0, rstd = 1/sqrt(eps), and ln1.w = 1e36 brings the activations back to order 1"""
    view(w, D, "fc1.weight")[:] *= np.float32(1e-38)
    view(w, D, "fc1.bias")[:] = 0.0
    view(w, D, "ln1.weight")[:] = 1e36


HEALTHY = {"tie2": tie2, "tie2_04": lambda w, D: tie2(w, D, 0, 4), "tie2_23": lambda w, D: tie2(w, D, 2, 3), "tie5": tie5,
           "signed_zeros": signed_zeros, "zero_variance": zero_variance, "subnormal_fc2": subnormal_fc2,
           "subnormal_fc1": subnormal_fc1}
FAULTY = {"all_neg_inf": all_neg_inf, "one_pos_inf": one_pos_inf, "one_nan_logit": one_nan_logit,
          "all_nan_logits": all_nan_logits, "nan_in_fc2": nan_in_fc2, "fc2_overflow": fc2_overflow, "nan_in_fc1": nan_in_fc1}
CLASSES = dict(HEALTHY, **FAULTY)
# what the oracle says of each class for any finite observation: (status word, action or None where it depends on the net)
PROPERTY = {"tie2": (0, 1), "tie2_04": (0, 0), "tie2_23": (0, 2), "tie5": (0, 0), "signed_zeros": (0, 0),
            "zero_variance": (0, None), "subnormal_fc2": (0, None), "subnormal_fc1": (0, None),
            "all_neg_inf": (BAD_OUT | NO_ACTION, -1), "one_pos_inf": (BAD_OUT, 2), "one_nan_logit": (BAD_OUT, None),
            "all_nan_logits": (BAD_OUT | NO_ACTION, -1), "nan_in_fc2": (BAD_FC2 | BAD_OUT | NO_ACTION, -1),
            "fc2_overflow": (BAD_FC2 | BAD_OUT | NO_ACTION, -1), "nan_in_fc1": (BAD_FC1 | BAD_FC2 | BAD_OUT | NO_ACTION, -1)}
BAD_OBS_STATUS = BAD_INPUT | BAD_FC1 | BAD_FC2 | BAD_OUT | NO_ACTION   # inf / NaN in an observation column < D
SUBNORMAL = {"subnormal_fc2": "fc2.weight", "subnormal_fc1": "fc1.weight"}
TIES = ("tie2", "tie2_04", "tie2_23", "tie5")


def make(name, D, seed=0):
    """the net of class `name` ("plain": the freshly initialised net itself)"""
    w = base_net(D, 1000 + seed)
    if name != "plain":
        CLASSES[name](w, D)
    return w


def flushed(w, D, name):
    """the same net as a unit that flushes subnormal inputs would see it: every |entry| < 2^-126 of the class' tensor is 0"""
    out = w.copy()
    t = view(out, D, SUBNORMAL[name])
    assert (np.abs(t) < MIN_NORMAL).all() and (t != 0).mean() > 0.99, "the class' tensor is not subnormal throughout"
    t[np.abs(t) < MIN_NORMAL] = 0.0
    return out


def has_teeth(w, w_flushed, D, obs):
    """flushing changes the logits' bits AND the action for this observation (oracle against oracle)"""
    a, lg, st = rp.fc_forward(w, D, obs)
    af, lf, sf = rp.fc_forward(w_flushed, D, obs)
    return st == 0 and sf == 0 and a != af and not np.array_equal(lg.view(np.uint32), lf.view(np.uint32))


def observations(g, n, D, name="plain", w=None):
    """n observation rows [n][D] of order 1; for a subnormal class only rows on which the class has teeth (rejection by
    the oracle: about one row in five has the flushed net's action anyway)"""
    if name not in SUBNORMAL:
        return g.uniform(-2, 2, size=(n, D)).astype(np.float32)
    wf, rows = flushed(w, D, name), []
    for _ in range(200 * n):
        o = g.uniform(-2, 2, size=D).astype(np.float32)
        if has_teeth(w, wf, D, o):
            rows.append(o)
            if len(rows) == n:
                return np.stack(rows)
    raise AssertionError(f"{name} (D = {D}): no observation on which flushing subnormals shows")


def same_bits_up_to_nan(got, want):
    """fp arrays equal bit for bit (sign of zero, infinities included) except that a NaN matches any NaN"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(u)[~gn], want.view(u)[~wn]))


def last_maximum(logits):
    """what a `>=` scan returns: the LAST index of the maximum (-1 when nothing compares)"""
    best, cur = -1, -np.inf
    for i, v in enumerate(logits):
        if v >= cur and not np.isnan(v):
            cur, best = v, i
    return best
