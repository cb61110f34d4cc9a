"""COEVO_TASK_TILED on the host side: the task word that names a twin, the constants lib.py mirrors from include/coevo.h, and
the numpy statements of tests/tile_major_cases.py (twin_of, promote_tiled) that the GPU tests take as their expectation."""
import os
import re

import numpy as np
import pytest

from coevonet_amd import lib as L
from tests import breed_cases as bc, tile_major_cases as tm

H1, H2 = tm.H1, tm.H2


def test_twin_of_is_the_headers_index_formula():
    """include/coevo.h: inside the group of 256 floats of (output block w, k-quad q), twin piece l = 16 lg + lc, element T =
    the net's piece 16 T + lc, element lg = fc2.weight[64 w + 16 T + lc][4 q + lg].  Every (w, q, l, T) of one group, every
    (l, T) of sampled groups - the corners among them - and both halves of the sentence: against fc2.weight and against the
    net's own pieces in the slab"""
    W2 = np.arange(H2 * H1, dtype=np.float32).reshape(H2, H1)   # (every entry exact and distinct in fp32)
    t = tm.twin_of(W2).reshape(4, 128, 64, 4)
    for D in (8, 10):
        row = bc.to_slab_rows(np.arange(bc.params(D), dtype=np.float32), D, -1.0)
        assert tm.w2_offset(D) == bc.segments(D)[4][0]
        canon = np.arange(bc.params(D), dtype=np.float32)[tm.w2_offset(D):tm.w2_offset(D) + tm.W2_FLOATS].reshape(H2, H1)
        assert np.array_equal(tm.w2_of_slab_row(row, D), canon)   # the slab's W2q pieces, read back
    pieces = W2.reshape(4, 64, 128, 4).transpose(0, 2, 1, 3)     # the net's W2q [jb][kq][piece][element]
    g = np.random.Generator(np.random.PCG64(5))
    groups = {(0, 0), (3, 127), (0, 127), (3, 0), (2, 17)} | {(int(g.integers(4)), int(g.integers(128))) for _ in range(12)}
    n = 0
    for w, q in sorted(groups):
        for l in range(64):
            lc, lg = l % 16, l // 16
            for T in range(4):
                assert t[w, q, l, T] == W2[64 * w + 16 * T + lc, 4 * q + lg] == pieces[w, q, 16 * T + lc, lg], (w, q, l, T)
                n += 1
    assert n == len(groups) * 256 and len(groups) >= 12


def test_twin_of_is_a_permutation():
    """every entry of fc2.weight exactly once, inside its own group of 256 floats; the words themselves untouched"""
    idx = tm.twin_of(np.arange(H2 * H1, dtype=np.int64).reshape(H2, H1))
    assert idx.shape == (tm.W2_FLOATS,) and np.array_equal(np.sort(idx), np.arange(H2 * H1))
    # the group of twin position p is the group of the net's slab position of the same entry
    j, k = idx // H1, idx % H1
    slab_pos = ((j // 64) * 128 + k // 4) * 256 + (j % 64) * 4 + k % 4
    assert np.array_equal(slab_pos // 256, np.arange(H2 * H1) // 256)
    raw = tm.raw_words(np.random.Generator(np.random.PCG64(6)), H2 * H1)
    assert np.isnan(raw).any() and (raw.view(np.uint32) == 0x80000000).any()
    assert np.array_equal(tm.twin_of(raw.reshape(H2, H1)).view(np.uint32), raw.view(np.uint32)[idx])


def test_promote_tiled_three_slots_by_hand():
    """rows are names, w2_of looks the name's fc2.weight up: every list written out"""
    W = {name: np.full((H2, H1), v, dtype=np.float32) for name, v in (("p0", 0.0), ("p1", 1.0), ("p2", 2.0), ("e0", 10.0))}
    pop, hof, elite, twins = ["p0", "p1", "p2"], ["h0", "h1", "h2"], ["e0", "e1"], ["t0", "t1", "t2"]
    # the best is pop[2]; elites gathered, pop[0] overwritten
    p, h, e, t = tm.promote_tiled(pop, hof, elite, twins, [2, 0], 2, True, True, W.__getitem__)
    assert (p, h, e, t[:2]) == (["p2", "p1", "p2"], ["h1", "h2", "p2"], ["p2", "p0"], ["t1", "t2"])
    assert np.array_equal(t[2], np.full(tm.W2_FLOATS, 2.0, dtype=np.float32))
    # the elites are in place: elite[0] is the best, pop[0] left alone
    p, h, e, t = tm.promote_tiled(pop, hof, elite, twins, None, 2, False, False, W.__getitem__)
    assert (p, h, e, t[:2]) == (pop, ["h1", "h2", "e0"], elite, ["t1", "t2"])
    assert np.array_equal(t[2], np.full(tm.W2_FLOATS, 10.0, dtype=np.float32))
    # the best already in pop[0], written onto itself; a second step pushes the first one's twin down
    W3 = np.arange(H2 * H1, dtype=np.float32).reshape(H2, H1)
    W["p0"] = W3
    p, h, e, t = tm.promote_tiled(pop, hof, elite, twins, [0, 1], 2, True, True, W.__getitem__)
    assert (p, h, e, t[:2]) == (pop, ["h1", "h2", "p0"], ["p0", "p1"], ["t1", "t2"]) and np.array_equal(t[2], tm.twin_of(W3))
    p, h, e, t2 = tm.promote_tiled(p, h, e, t, [1, 0], 2, True, False, W.__getitem__)
    assert (p, h, e, t2[0]) == (pop, ["h2", "p0", "p1"], ["p1", "p0"], "t2")
    assert t2[1] is t[2] and np.array_equal(t2[2], np.full(tm.W2_FLOATS, 1.0, dtype=np.float32))
    # one slot: nothing shifts
    assert tm.promote_tiled(pop, ["h0"], elite, ["t0"], None, 2, False, True, W.__getitem__)[1:3] == (["e0"], elite)
    (one,) = tm.promote_tiled(pop, ["h0"], elite, ["t0"], None, 2, False, True, W.__getitem__)[3]
    assert np.array_equal(one, np.full(tm.W2_FLOATS, 10.0, dtype=np.float32))


def test_constants_mirror_the_header():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(here, "include", "coevo.h")).read()
    for name, value in (("COEVO_TASK_RESIDENT", L.TASK_RESIDENT), ("COEVO_TASK_TILED", L.TASK_TILED),
                        ("COEVO_TASK_TWIN_SHIFT", L.TASK_TWIN_SHIFT), ("COEVO_TASK_TWIN_UNIT", L.TASK_TWIN_UNIT)):
        assert int(re.search(rf"#define {name} (\d+)", text).group(1)) == value, name
    assert L.W2_FLOATS == 512 * 256 and L.W2_FLOATS % L.TASK_TWIN_UNIT == 0
    assert L.TASK_TILED & L.TASK_RESIDENT == 0 and L.TASK_TILED < 1 << L.TASK_TWIN_SHIFT


def test_task_word_names_the_twin_offset():
    for off in (0, L.TASK_TWIN_UNIT, 87 * L.W2_FLOATS, ((1 << 23) - 1) * L.TASK_TWIN_UNIT):
        word = L.task_tiled_flags(off)
        assert word & L.TASK_TILED and 0 < word < 1 << 31   # (coevo_fc_task.reserved is an int32)
        assert (word >> L.TASK_TWIN_SHIFT) * L.TASK_TWIN_UNIT == off
    for bad in (-L.TASK_TWIN_UNIT, 513, (1 << 23) * L.TASK_TWIN_UNIT):
        with pytest.raises(AssertionError):
            L.task_tiled_flags(bad)
