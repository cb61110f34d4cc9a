"""The breeding kernels' canonical-quad <-> slab-position maps (csrc/offspring.hip: w1t_slab_of_flat, w2_piece_quad, the
small regions of slab_quad_normals), written out in numpy with the kernels' 32-bit integer steps and held against the
host-side slab <-> flat map the other breeding tests use (tests/breed_cases.slab_to_flat, which test_breed_edges_gpu pins
to the pack kernel).  One Philox block = one canonical quad q = the normals of canonical indices 4 q .. 4 q + 3."""
import numpy as np
import pytest

from tests import breed_cases as bc

H1, H2, NACT = 512, 256, 5
DS = (8, 10)


def offsets(D):
    o_b1 = D * H1
    o_w2 = o_b1 + 3 * H1
    o_b2 = o_w2 + H1 * H2
    return o_b1, o_w2, o_b2, o_b2 + 3 * H2 + NACT * H2 + NACT


def w1t_slab_of_flat(p, D):
    """the device helper: canonical index p = j D + k of fc1.weight -> W1t[k][j]"""
    p = np.asarray(p, dtype=np.uint32)
    j = p >> 3 if D == 8 else p // np.uint32(10)
    return ((p - j * np.uint32(D)) * np.uint32(H1) + j).astype(np.int64)


def w2_piece_quad(s0, o_w2):
    t = np.asarray(s0, dtype=np.int32) - np.int32(o_w2)
    lane, kq, jb = (t >> 2) & 63, (t >> 8) & 127, t >> 15
    return ((o_w2 + (jb * 64 + lane) * H1 + kq * 4) >> 2).astype(np.int64)


def breeding_map(D):
    """int64 [stride]: for every slab position the canonical index whose normal the breeding launch adds there, -1 where it
    adds none - assembled the way the launch walks a net: the W1t region by canonical quad (workgroup 0), W2 and the small
    regions by 16-byte piece"""
    o_b1, o_w2, o_b2, P = offsets(D)
    stride = bc.stride(D)
    out = np.full(stride, -2, dtype=np.int64)
    # workgroup 0: quads 0 .. D * 128 - 1, thread t takes q = t, t + 256, ...
    hits = np.zeros(stride, dtype=np.int64)
    for q in range(D * H1 // 4):
        for i in range(4):
            s = int(w1t_slab_of_flat(4 * q + i, D))
            assert 0 <= s < o_b1, (q, i, s)
            out[s] = 4 * q + i
            hits[s] += 1
    assert (hits[:o_b1] == 1).all() and not hits[o_b1:].any()
    # every other piece
    s0 = np.arange(o_b1, stride, 4, dtype=np.int64)
    in_w2 = (s0 >= o_w2) & (s0 < o_b2)
    quad = np.where(in_w2, w2_piece_quad(np.where(in_w2, s0, o_w2), o_w2), s0 >> 2)
    for i in range(4):
        p = 4 * quad + i
        out[s0 + i] = np.where((s0 + i < P) | in_w2, p, -1)
    return out


@pytest.mark.parametrize("D", DS)
def test_region_bounds(D):
    o_b1, o_w2, o_b2, P = offsets(D)
    assert P == bc.params(D) and [o for o, _ in bc.segments(D)][:6] == [0, o_b1, o_b1 + H1, o_b1 + 2 * H1, o_w2, o_b2]
    # the launch's assumptions: the W1t region is whole blocks, D * 128 quads split evenly over 256 threads, every region
    # edge except P is a multiple of 4 (a piece is LayerNorm / W2 / W1t as a whole), and 32-bit math holds
    assert o_b1 % bc.BLOCK == 0 and o_b1 // bc.BLOCK == D // 2 and (D * H1 // 4) % 256 == 0
    edges = [o for o, _ in bc.segments(D)]
    assert all(e % 4 == 0 for e in edges) and bc.stride(D) % 4 == 0 and bc.stride(D) < 2 ** 18
    assert D * H1 <= 10 * H1          # W1T_MAX_FLOATS


@pytest.mark.parametrize("D", DS)
def test_breeding_map_is_the_slab_map(D):
    got, want = breeding_map(D), bc.slab_to_flat(D)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


@pytest.mark.parametrize("D", DS)
def test_every_parameter_hit_exactly_once(D):
    m = breeding_map(D)
    P = bc.params(D)
    assert (m[P:] == -1).all() and (m[:P] >= 0).all()
    assert np.array_equal(np.sort(m[:P]), np.arange(P))


@pytest.mark.parametrize("D", DS)
def test_w1t_quads(D):
    """a canonical quad of fc1.weight: D = 8 - half a row j (k = 0..3 or 4..7); D = 10 - quads start at k = 0, 4, 8, 2, 6 in
    turn, and the one that starts at k = 8 holds rows j and j + 1"""
    p = np.arange(D * H1, dtype=np.int64)
    s = w1t_slab_of_flat(p, D)
    assert np.array_equal(s, (p % D) * H1 + p // D)
    rows = (p // D).reshape(-1, 4)
    straddle = rows[:, 0] != rows[:, 3]
    assert straddle.sum() == (0 if D == 8 else (D * H1 // 4) // 5)
    assert (p[0::4][straddle] % D == 8).all()
    # and back: the four positions of a W1t piece lie in four different quads (what a piece-wise generator pays)
    q = (bc.slab_to_flat(D)[:D * H1] >> 2).reshape(-1, 4)
    assert (np.diff(np.sort(q, axis=1), axis=1) > 0).all()


@pytest.mark.parametrize("D", DS)
def test_small_region_pieces_are_one_quad(D):
    o_b1, o_w2, o_b2, P = offsets(D)
    m = bc.slab_to_flat(D)
    for lo, hi in ((o_b1, o_w2), (o_b2, bc.stride(D))):
        pieces = m[lo:hi].reshape(-1, 4)
        s0 = np.arange(lo, hi, 4)
        live = s0 < P
        assert np.array_equal(pieces[live][:, 0], s0[live]) and (pieces[~live] == -1).all()
        full = s0 + 3 < P
        assert (pieces[full] == s0[full, None] + np.arange(4)).all()
    # the one piece that holds the last parameters and the first padding words
    assert P % 4 != 0 and (m[P - P % 4:P] >= 0).all() and (m[P:P - P % 4 + 4] == -1).all()
    # LayerNorm ranges begin and end on piece edges
    ln = np.flatnonzero(bc.ln_mask(D))
    cuts = np.flatnonzero(np.diff(ln) != 1)
    for e in (ln[0], ln[-1] + 1, *(ln[cuts] + 1), *ln[cuts + 1]):
        assert e % 4 == 0
