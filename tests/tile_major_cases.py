"""The tile-major twin of fc2.weight (COEVO_TASK_TILED, include/coevo.h) and the promotion that keeps the Hall of Fame's twins,
as plain numpy / list operations.  Nothing here knows what a kernel returns; no GPU and no libcoevo needed: proven on the CPU by
tests/test_hof_tile_major_cpu.py, used as the expectation by tests/test_hof_tile_major_gpu.py, tests/test_breed_edges_gpu.py
and tests/test_fc_forward_edges_gpu.py."""
import numpy as np

from tests import breed_cases as bc

H1, H2 = 512, 256
W2_FLOATS = H1 * H2


def twin_of(W2):
    """fc2.weight [256][512] -> its tile-major twin: piece (w, q, l = 16 lg + lc), element T = W2[64 w + 16 T + lc][4 q + lg].
    A pure re-ordering: the dtype and every bit of every element are kept"""
    assert W2.shape == (H2, H1)
    return np.ascontiguousarray(W2.reshape(4, 4, 16, 128, 4).transpose(0, 3, 4, 2, 1)).reshape(-1)   # [w][q][lg][lc][T]


def w2_offset(D):
    """first slab position of the second layer's weights: behind W1t, fc1.bias and the LayerNorm(512) affine"""
    return D * H1 + 3 * H1


def w2_of_slab_row(row, D):
    """fc2.weight [256][512] out of one raw slab row (any words: nothing is interpreted): W2q[jb][kq][l][c] =
    fc2.weight[64 jb + l][4 kq + c]"""
    o = w2_offset(D)
    blk = np.asarray(row)[o:o + W2_FLOATS].reshape(4, 128, 64, 4)   # [jb][kq][l][c]
    return np.ascontiguousarray(blk.transpose(0, 2, 1, 3)).reshape(H2, H1)


def promote_tiled(pop, hof, elite, twins, order, E, from_pop, to_pop0, w2_of):
    """breed_cases.promote + the twin FIFO -> (pop, hof, elite, twins): the oldest twin leaves, the others move one slot down
    as they are (whatever they hold), and the last slot is the twin of the best's fc2.weight as it is BEFORE anything is
    written.  w2_of(row) -> fc2.weight [256][512] of a row"""
    assert len(twins) == len(hof)
    best = pop[order[0]] if from_pop else elite[0]
    new_twin = twin_of(w2_of(best))
    pop, hof, elite = bc.promote(pop, hof, elite, order, E, from_pop, to_pop0)
    return pop, hof, elite, list(twins)[1:] + [new_twin]


def raw_words(g, n):
    """n float32 words of random bits with NaN payloads (quiet and signalling, both signs), infinities, -0.0, +0.0 and
    subnormals planted at random places: what only a bit copy reproduces"""
    u = g.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    plants = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0xff923456, 0x7f800000, 0xff800000, 0x80000000, 0x00000000,
                       0x00000001, 0x807fffff, 0x00400000], dtype=np.uint32)
    where = g.choice(n, size=min(n, 64 * len(plants)), replace=False)
    u[where] = plants[np.arange(len(where)) % len(plants)]
    return u.view(np.float32)
