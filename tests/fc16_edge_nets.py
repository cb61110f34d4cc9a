"""Adversarial float16 FCNetwork parameter vectors and observations for the two fp16 policy-forward bodies (fc16_policy_kernel in
csrc/fc16.hip, fc16_cycle_kernel in csrc/fc16_rollout.hip), with the C checker (tests/checker16/fc16_checker.c through
tests/fp16_checker.py) as the only judge.

Every net is a healthy random_flat net (canonical parameters() order, Linear entries fp16 values, LayerNorm affine fp32) with
entries overwritten.  Nothing here knows what a kernel returns: the expected logits / action / status of a class always come
from ck.forward, ck.play_game or ck.play_game_steps at the place of use; PROPERTY only says what tests/test_fc16_edges_cpu.py
pins of the checker itself.  No GPU and no libcoevo needed: tests/test_fc16_forward_edges_gpu.py imports the library from here,
tests/test_fp16_gpu.py and tests/test_fp16_rollout_gpu.py import the nets they used to build themselves."""
import numpy as np

from coevonet_amd import lib as L
from oracle import ref_port as rp
from tests import fp16_checker as ck

H1, H2, NACT = rp.H1, rp.H2, rp.NACT
BAD_INPUT, BAD_FC1, BAD_FC2, BAD_OUT, NO_ACTION = (
    L.K["COEVO_ST_" + n] for n in ("BAD_INPUT", "BAD_FC1", "BAD_FC2", "BAD_OUT", "NO_ACTION"))
LINEAR_KEYS = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "output.weight", "output.bias")
MIN_NORMAL16 = np.float32(2.0 ** -14)
INF, NAN = np.float32(np.inf), np.float32(np.nan)


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


def linear_mask(D):
    return np.concatenate([np.full(int(np.prod(s)), k in LINEAR_KEYS) for k, s in rp.param_shapes(D)])


def f16(x):
    """round to nearest even fp16, kept as float32 (numpy's conversion: the CPU file pins the checker's against it)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def random_flat(rng, D, scale=0.05, ln_noise=0.05):
    """a GA-like fp16 net: torch-like init magnitudes, fp16 Linear entries, perturbed fp32 LayerNorm affine"""
    P = rp.param_count(D)
    flat = rng.uniform(-0.3, 0.3, P).astype(np.float32) * np.float32(scale / 0.05)
    off = 0
    for k, s in rp.param_shapes(D):
        n = int(np.prod(s))
        if k.startswith("ln"):
            base = 1.0 if k.endswith("weight") else 0.0
            flat[off:off + n] = np.float32(base) + rng.normal(0, ln_noise, n).astype(np.float32)
        off += n
    m = linear_mask(D)
    flat[m] = flat[m].astype(np.float16).astype(np.float32)
    return flat


def subnormal_values(rng, n):
    k = rng.integers(1, 1024, n) * rng.choice([-1, 1], n)
    return (k.astype(np.float64) * 2.0 ** -24).astype(np.float32)   # every one an fp16 subnormal, exactly


# ------------------------------------------------------------------------------------------- the classes: f(w, D, rng)
def tie2(w, D, g=None, i=1, j=3):
    """logits i and j bit-equal and far above the rest: the first of them is the action"""
    W3, b3 = view(w, D, "output.weight"), view(w, D, "output.bias")
    W3[j], b3[j] = W3[i], b3[i]
    for o in range(NACT):
        if o not in (i, j):
            b3[o] = -1e3


def tie3(w, D, g=None):
    """actions 1, 3 and 4 share their output row and bias and carry the maximum: exact three-way logit ties"""
    W3, b3 = view(w, D, "output.weight"), view(w, D, "output.bias")
    W3[3] = W3[4] = W3[1]
    b3[1] = np.float32(np.float16(b3[1] + np.float32(64.0)))
    b3[3] = b3[4] = b3[1]


def tie5(w, D, g=None):
    view(w, D, "output.weight")[:] = 0.0
    view(w, D, "output.bias")[:] = 0.25


def signed_zeros(w, D, g=None):
    """logits (-0, +0, -0, +0, +0): W3 = 0 carrying its row's sign, so that the fmaf chain (h2 >= 0) keeps the bias' zero"""
    sign = np.array([-0.0, 0.0, -0.0, 0.0, 0.0], dtype=np.float32)
    view(w, D, "output.weight")[:] = sign[:, None]
    view(w, D, "output.bias")[:] = sign


def all_neg_inf(w, D, g=None):
    view(w, D, "output.weight")[:] = 0.0
    view(w, D, "output.bias")[:] = -np.inf


def one_pos_inf(w, D, g=None):
    view(w, D, "output.bias")[2] = np.inf


def one_nan_logit(w, D, g=None):
    view(w, D, "output.bias")[2] = np.nan


def all_nan_logits(w, D, g=None):
    view(w, D, "output.bias")[:] = np.nan


def gamma_inf(w, D, g=None):
    """ln1.weight[7] = inf.  inf * (x - mean) * rstd is +inf only where feature 7 lies above the row's mean (below it the ReLU
    swallows -inf and the net is healthy), so feature 7 is pinned there: fc1 row 7 = 0, fc1.bias[7] = 8.  h1[7] = +inf, every
    fc2 output is +-inf or NaN, LayerNorm(256) makes NaN of the row"""
    view(w, D, "ln1.weight")[7] = np.inf
    view(w, D, "fc1.weight")[7] = 0.0
    view(w, D, "fc1.bias")[7] = 8.0


def zero_variance(w, D, g=None):
    """every fc1 output equal: LayerNorm(512) sees variance 0, rstd = 1/sqrt(eps), its output row is f16(ln1.bias)"""
    view(w, D, "fc1.weight")[:] = 0.0
    view(w, D, "fc1.bias")[:] = 0.5


def fc2_subnormal(w, D, g):
    view(w, D, "fc2.weight")[:] = subnormal_values(g, H2 * H1).reshape(H2, H1)


def fc1_subnormal(w, D, g):
    view(w, D, "fc1.weight")[:] = subnormal_values(g, H1 * D).reshape(H1, D)


def fc2_overflow(w, D, g=None):
    """fc2 outputs past 65504 become inf, the LayerNorm then makes NaN"""
    view(w, D, "fc2.weight")[:] = 60000.0


def fc1_overflow(w, D, g=None):
    """fc1 outputs of +-inf (huge weights on a huge bias)"""
    b1 = view(w, D, "fc1.bias")
    b1[:] = 65504.0
    b1[0] = -65504.0
    view(w, D, "fc1.weight")[:] = 8000.0


def _constant_h2(w, D, be2):
    """fc2.weight = 0, fc2.bias = 0.5, ln2.weight = 1: LayerNorm(256) sees variance 0 and returns f16(ln2.bias[j]), whatever
    the observation; ln2.bias is fp32 in the slab and is not rounded by the pack"""
    view(w, D, "fc2.weight")[:] = 0.0
    view(w, D, "fc2.bias")[:] = 0.5
    view(w, D, "ln2.weight")[:] = 1.0
    b = view(w, D, "ln2.bias")
    b[:] = 0.0
    b[:len(be2)] = be2


LN_VALS = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -25, 3 * 2.0 ** -25, 65519.996], dtype=np.float32)
LN_VALS_INF = np.concatenate([LN_VALS[:4], np.array([65520.0], dtype=np.float32)])


def ln_rounding(w, D, g=None, vals=LN_VALS):
    """LayerNorm's fp16 rounding point made visible in the logits: h2[:5] = f16(vals) - two midpoints of the normal range (to
    even: down, up), two of the subnormal range (to 0, to 2^-23), the last fp32 below 65520 (to 65504) - and a one-hot output
    layer hands them through unchanged"""
    _constant_h2(w, D, vals)
    W3 = view(w, D, "output.weight")
    W3[:] = 0.0
    W3[np.arange(NACT), np.arange(NACT)] = 1.0
    view(w, D, "output.bias")[:] = 0.0


def ln_rounding_inf(w, D, g=None):
    """entry 4 = 65520, the first fp32 that rounds to inf: logits (NaN, NaN, NaN, NaN, inf) (0 * inf in the other rows)"""
    ln_rounding(w, D, g, LN_VALS_INF)


def out_rounding(w, D, g=None, k=1):
    """the output chain's rounding decides the action: h2 = (1, 0, 0, ...), logit 0 = 1, logit 1 = f16(1 + k 2^-11).  k = 1: a
    midpoint, to even 1.0, ties logit 0 -> action 0; k = 3: the midpoint above, to even 1.001953 -> action 1 (half-up gets
    k = 1 wrong); k = 1.5: nearer to 1.000977 -> action 1 (truncation gets it wrong: it takes both midpoints the right way)"""
    _constant_h2(w, D, [1.0])
    W3 = view(w, D, "output.weight")
    W3[:] = 0.0
    W3[1][0] = k * 2.0 ** -11
    view(w, D, "output.bias")[:] = (1.0, 1.0, -1000.0, -1000.0, -1000.0)


def out_rounding_up(w, D, g=None):
    out_rounding(w, D, g, 3)


def out_rounding_near(w, D, g=None):
    out_rounding(w, D, g, 1.5)


def pad_fault(w, D, g):
    """healthy on every real observation, faulty on the all-zero row that pads a partial pass: fc1.bias = s (random +-1),
    fc1.weight random +-100, fc2.weight[j][k] = 300 s[k], LayerNorm affines the identity.  x = 0: h1 = relu(LN(s)) is about 1
    where s = 1, fc2 = 300 * (about 256) is past 65504.  x of order 1: the fc1 outputs are x's, their signs are independent
    of s, and 300 * sum s[k] h1[k] is a random walk of a few thousand"""
    s = g.choice(np.float32([-1.0, 1.0]), H1)
    view(w, D, "fc1.bias")[:] = s
    view(w, D, "fc1.weight")[:] = g.choice(np.float32([-100.0, 100.0]), (H1, D))
    view(w, D, "fc2.weight")[:] = 300.0 * s[None, :]
    for k in ("ln1", "ln2"):
        view(w, D, k + ".weight")[:] = 1.0
        view(w, D, k + ".bias")[:] = 0.0


def pad_fault_fc1(w, D, g):
    """the same for LayerNorm(512): fc1.weight random +-100, fc1.bias = 0, but feature 7 has fc1 row 0 and bias 1, gamma 4000
    and no way into fc2 (fc2.weight[:, 7] = 0).  x = 0: fc1 is one-hot, feature 7 normalises to sqrt(511) = 22.6, times 4000 is
    past 65504: +inf.  x of order 1: the other features spread by hundreds, feature 7 normalises to well below 1"""
    W1, b1 = view(w, D, "fc1.weight"), view(w, D, "fc1.bias")
    W1[:] = g.choice(np.float32([-100.0, 100.0]), (H1, D))
    W1[7], b1[:] = 0.0, 0.0
    b1[7] = 1.0
    view(w, D, "ln1.weight")[:] = 1.0
    view(w, D, "ln1.bias")[:] = 0.0
    view(w, D, "ln1.weight")[7] = 4000.0
    view(w, D, "fc2.weight")[:, 7] = 0.0


HEALTHY = {"tie2": tie2, "tie2_04": lambda w, D, g: tie2(w, D, g, 0, 4), "tie2_23": lambda w, D, g: tie2(w, D, g, 2, 3),
           "tie3": tie3, "tie5": tie5, "signed_zeros": signed_zeros, "zero_variance": zero_variance,
           "fc2_subnormal": fc2_subnormal, "fc1_subnormal": fc1_subnormal, "ln_rounding": ln_rounding,
           "out_rounding": out_rounding, "out_rounding_up": out_rounding_up, "out_rounding_near": out_rounding_near,
           "pad_fault": pad_fault, "pad_fault_fc1": pad_fault_fc1}
FAULTY = {"all_neg_inf": all_neg_inf, "one_pos_inf": one_pos_inf, "one_nan_logit": one_nan_logit,
          "all_nan_logits": all_nan_logits, "gamma_inf": gamma_inf, "ln_rounding_inf": ln_rounding_inf,
          "fc2_overflow": fc2_overflow, "fc1_overflow": fc1_overflow}
CLASSES = dict(HEALTHY, **FAULTY)
# what the checker says of each class for any observation of order 1: (status word, action or None where it depends on the net)
PROPERTY = {"tie2": (0, 1), "tie2_04": (0, 0), "tie2_23": (0, 2), "tie3": (0, 1), "tie5": (0, 0), "signed_zeros": (0, 0),
            "zero_variance": (0, None), "fc2_subnormal": (0, None), "fc1_subnormal": (0, None), "ln_rounding": (0, 4),
            "out_rounding": (0, 0), "out_rounding_up": (0, 1), "out_rounding_near": (0, 1), "pad_fault": (0, None),
            "pad_fault_fc1": (0, None),
            "all_neg_inf": (BAD_OUT | NO_ACTION, -1), "one_pos_inf": (BAD_OUT, 2), "one_nan_logit": (BAD_OUT, None),
            "all_nan_logits": (BAD_OUT | NO_ACTION, -1), "gamma_inf": (BAD_FC1 | BAD_FC2 | BAD_OUT | NO_ACTION, -1),
            "ln_rounding_inf": (BAD_FC2 | BAD_OUT, 4), "fc2_overflow": (BAD_FC2 | BAD_OUT | NO_ACTION, -1),
            "fc1_overflow": (BAD_FC1 | BAD_FC2 | BAD_OUT | NO_ACTION, -1)}
# the pad_fault classes on the all-zero observation
PAD_FAULT_ZERO_ROW = {"pad_fault": BAD_FC2 | BAD_OUT | NO_ACTION, "pad_fault_fc1": BAD_FC1 | BAD_FC2 | BAD_OUT | NO_ACTION}
BAD_OBS_STATUS = BAD_INPUT | BAD_FC1 | BAD_FC2 | BAD_OUT | NO_ACTION   # inf / NaN in an observation column < D
SUBNORMAL = {"fc2_subnormal": "fc2.weight", "fc1_subnormal": "fc1.weight"}
TIES = {"tie2": 2, "tie2_04": 2, "tie2_23": 2, "tie3": 3, "tie5": 5, "out_rounding": 2}   # class -> logits that share the maximum


def make(name, D, seed=0):
    """the net of class `name` ("plain": the healthy net itself); Linear entries are fp16 values (inf / NaN kept)"""
    g = np.random.default_rng([16, D, seed])
    w = random_flat(g, D)
    if name != "plain":
        CLASSES[name](w, D, g)
        m = linear_mask(D)
        w[m] = f16(w[m])
    return w


def edge_nets(rng):
    """the five nets of tests/test_fp16_rollout_gpu.py's EDGE_CASES -> {name: (flat, D)}"""
    out = {}
    for name, cls, D in (("ties", tie3, 10), ("fc2_subnormal", fc2_subnormal, 10), ("fc1_subnormal", fc1_subnormal, 8),
                         ("fc2_overflow", fc2_overflow, 10), ("fc1_overflow", fc1_overflow, 10)):
        f = random_flat(rng, D)
        cls(f, D, rng)
        out[name] = (f, D)
    return out


def flushed(w, D, name):
    """the same net as a unit that flushes fp16 subnormals would see it: every |entry| < 2^-14 of the class' tensor is 0"""
    out = w.copy()
    t = view(out, D, SUBNORMAL[name])
    assert (np.abs(t) < MIN_NORMAL16).all() and (t != 0).all(), "the class' tensor is not subnormal throughout"
    t[:] = 0.0
    return out


def has_teeth(w, w_flushed, D, obs):
    """flushing changes the logits' bits for this observation (checker against checker)"""
    a, lg, st = ck.forward(w, D, obs)
    af, lf, sf = ck.forward(w_flushed, D, obs)
    return st == 0 and sf == 0 and not np.array_equal(lg.view(np.uint32), lf.view(np.uint32))


def observations(g, n, D, name="plain", w=None):
    """n observation rows [n][D] of order 1 (the pad_fault classes need that: they fault on rows that are tiny in every
    column); for a subnormal class only rows on which the class has teeth (rejection by the checker)"""
    if name not in SUBNORMAL:
        return g.uniform(-2, 2, size=(n, D)).astype(np.float32)
    wf, rows = flushed(w, D, name), []
    for _ in range(50 * n):
        o = g.uniform(-2, 2, size=D).astype(np.float32)
        if has_teeth(w, wf, D, o):
            rows.append(o)
            if len(rows) == n:
                return np.stack(rows)
    raise AssertionError(f"{name} (D = {D}): no observation on which flushing subnormals shows")


def round_toward_zero16(x):
    """fp32 -> fp16 by truncation (a wrong kernel's rounding, for the teeth of the rounding classes)"""
    x = np.asarray(x, dtype=np.float32)
    r = f16(x)
    with np.errstate(over="ignore"):
        toward = np.nextafter(r.astype(np.float16), np.float16(0)).astype(np.float32)
    return np.where(np.abs(r) > np.abs(x), toward, r).astype(np.float32)


def round_half_up16(x):
    """fp32 -> fp16 to nearest, midpoints away from zero"""
    x = np.asarray(x, dtype=np.float32)
    r = f16(x)
    with np.errstate(over="ignore"):
        away = np.nextafter(r.astype(np.float16), (np.sign(x) * np.float16(np.inf)).astype(np.float16)).astype(np.float32)
    mid = (r.astype(np.float64) + away.astype(np.float64)) / 2   # (65504 + inf) / 2 = inf: never equal to a finite x
    return np.where((np.abs(r) < np.abs(x)) & (x.astype(np.float64) == mid), away, r).astype(np.float32)


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
