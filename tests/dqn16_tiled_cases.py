"""Numpy statements for the tiled fc1 block of the fp16 DeepQN slab (include/coevo_ext.h; csrc/dqn16_layout.hip.h wft16): the
permutation, one fc1 row of the float16 contract in fp32, and the ORDER-TELLING nets whose fc1 outputs say in which order a
kernel added its k terms.  No GPU, no library."""
import numpy as np

FC1_IN, FC1_OUT, SUPER = 3136, 512, 98
HALVES = FC1_IN * FC1_OUT
BIG, SMALL = 32768.0, 2.0 ** -10


def tiled_index(out, k):
    """half of the tiled fc1 block that holds fc1.w[out][k]: [ob 8][S 98][T 4][lane 64][j 8] with out = 64 ob + 16 T + lane % 16
    and k = 32 S + 4 j + lane / 16"""
    out, k = np.asarray(out, dtype=np.int64), np.asarray(k, dtype=np.int64)
    ob, T, c = out >> 6, (out >> 4) & 3, out & 15
    S, j, kk = k >> 5, (k >> 2) & 7, k & 3
    return ((((ob * SUPER + S) * 4 + T) * 64 + 16 * kk + c) << 3) + j


def streamed_index(out, k):
    """half of the streamed fc1 block that holds fc1.w[out][k]: [ob 8][k / 8][out % 64][k % 8]"""
    out, k = np.asarray(out, dtype=np.int64), np.asarray(k, dtype=np.int64)
    return ((((out >> 6) * (FC1_IN // 8) + (k >> 3)) * 64 + (out & 63)) << 3) + (k & 7)


def streamed_to_tiled():
    """perm with tiled_block[perm_target] = streamed_block: -> (src, dst) index arrays over all 512 x 3136 halves"""
    out, k = np.divmod(np.arange(HALVES, dtype=np.int64), FC1_IN)
    return streamed_index(out, k), tiled_index(out, k)


def f16(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def fc1_rows(W, bias, x, order=None):
    """the float16 contract's fc1 + ReLU of ONE input row, all 512 outputs at once: acc = bias; acc = f32(acc + w * x) over k in
    `order` (default: ascending) with the exact product and one rounding per step - the fmaf chain, as long as every sum's
    terms lie within 49 bits of each other (an fp64 add is then exact before the fp32 rounding) - y = relu(f16(acc)), NaN kept.
    W [512, 3136] and x [3136] hold fp16 values."""
    W64, x64 = np.asarray(W, dtype=np.float64), np.asarray(x, dtype=np.float64)
    acc = np.asarray(bias, dtype=np.float32).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for k in (range(FC1_IN) if order is None else order):
            acc = (acc.astype(np.float64) + W64[:, k] * x64[k]).astype(np.float32)
    y = f16(acc)
    return np.where(y < 0, np.float32(0), y)   # (a NaN compares false and stays)


# ------------------------------------------------------------------------------------------------ orders a defect would give
def order_descending():
    return list(range(FC1_IN - 1, -1, -1))


def order_kk_swapped():
    """k % 4 pairs (0, 1) and (2, 3) swapped inside every k-quad"""
    return [k ^ 1 for k in range(FC1_IN)]


def order_j_reversed():
    """the eight k-quads of every 32-k piece in reverse order"""
    return [32 * (k >> 5) + 4 * (7 - ((k >> 2) & 7)) + (k & 3) for k in range(FC1_IN)]


# ------------------------------------------------------------------------------------------------ the order-telling nets
KK_PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
RING = 7   # super-pieces in the kernel's register ring (DQ16_FC1_TNB): a ring round ends at every multiple of 32 * 7 k


def telling_pairs(variant=0):
    """(k_plus[512], k_minus[512]): where fc1 row o of an order-telling net holds +32768 and -32768.  Column c of tile t = o / 16
    (32 tiles = 8 output blocks x 4 column tiles) takes case c of the list below around a super-piece S0 that moves with the tile:
      0-5    both in one k-quad, at each of the six kk pairs          6   adjacent quads of one piece
      7      the piece seam 32 S + 31 | 32 S + 32                      8-9 a seam of the ring's rounds, both signs first
      10-11  k = 0 and k = 3135, both signs first                       12  far apart, 1 term before and 3 after
      13     far apart from kk 1 to kk 2                               14  far apart from j 1 to j 3
      15     the first and the last k of one piece
    variant 1 swaps the two signs of every row."""
    kp, km = np.zeros(FC1_OUT, dtype=np.int64), np.zeros(FC1_OUT, dtype=np.int64)
    for o in range(FC1_OUT):
        t, c = o >> 4, o & 15
        S0 = (3 * t + 1) % (SUPER - 1)
        base = 32 * S0
        if c < 6:
            q = base + 4 * ((t + c) % 8)
            a, b = q + KK_PAIRS[c][0], q + KK_PAIRS[c][1]
        elif c == 6:
            j = t % 7
            a, b = base + 4 * j + 3, base + 4 * (j + 1)
        elif c == 7:
            a, b = base + 31, base + 32
        elif c in (8, 9):
            r = 1 + t % (SUPER // RING - 1)
            a, b = 32 * RING * r - 1, 32 * RING * r
            if c == 9:
                a, b = b, a
        elif c == 10:
            a, b = 0, FC1_IN - 1
        elif c == 11:
            a, b = FC1_IN - 1, 0
        elif c == 12:
            a, b = 1, FC1_IN - 4
        elif c == 13:
            a = 32 * (S0 % 30) + 4 * (t % 8) + 1
            b = a + 2048 + 1
        elif c == 14:
            a = 32 * (S0 % 30) + 4
            b = a + 2048 + 8
        else:
            a, b = base, base + 31
        kp[o], km[o] = (a, b) if variant == 0 else (b, a)
    assert (kp != km).all() and kp.min() >= 0 and km.min() >= 0 and max(kp.max(), km.max()) < FC1_IN
    return kp, km


def telling_fc1(variant=0):
    """fc1.weight [512, 3136] of an order-telling net: +32768 at k_plus(o), -32768 at k_minus(o), 2^-10 everywhere else"""
    kp, km = telling_pairs(variant)
    W = np.full((FC1_OUT, FC1_IN), SMALL, dtype=np.float32)
    W[np.arange(FC1_OUT), kp] = BIG
    W[np.arange(FC1_OUT), km] = -BIG
    return W


def telling_net(base_flat, offsets, variant=0, gamma3=None):
    """`base_flat` (a flat fp16-valued net in parameters() order; offsets: name -> (offset, count)) turned into an order-telling
    net: vbn3.bias = 1 and an all-zero frame make every fc1 input exactly 1.0 - BatchNorm at variance 0 returns beta, and
    conv3.weight = conv3.bias = 0 keeps its input a plain zero whatever the layers in front compute - fc1.bias = 0, fc1.weight =
    telling_fc1(variant).  vbn3.weight is arbitrary (gamma3)."""
    net = np.array(base_flat, dtype=np.float32, copy=True)

    def put(name, value):
        o, m = offsets[name]
        net[o:o + m] = np.broadcast_to(np.asarray(value, dtype=np.float32).reshape(-1), (m,)) if np.size(value) == 1 else value

    put("conv3.weight", 0.0)
    put("conv3.bias", 0.0)
    put("vbn3.bias", 1.0)
    if gamma3 is not None:
        put("vbn3.weight", gamma3)
    put("fc1.bias", 0.0)
    put("fc1.weight", telling_fc1(variant).reshape(-1))
    return net


def telling_hidden(variant=0, order=None):
    """the hidden row (post-ReLU fc1 outputs) of an order-telling net on the all-zero frame, by fc1_rows"""
    return fc1_rows(telling_fc1(variant), np.zeros(FC1_OUT, dtype=np.float32), np.ones(FC1_IN, dtype=np.float32), order)
