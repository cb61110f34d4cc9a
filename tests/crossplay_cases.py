"""Numpy / plain-Python statements for the cross-play feature (include/coevo_crossplay.h): the game numbering as a brute-force
loop, the reduction coevo_crossplay_reduce in its stated order, and the reward tables of its tests - among them the ORDER-TELLING
table whose payoffs say in which order a kernel added the episodes.  No GPU, no library."""
import numpy as np

SHAPES = [(1, 1, 1, 1), (1, 1, 1, 10), (2, 3, 2, 3), (3, 1, 2, 65), (1, 5, 1, 7)]   # (A, B, C, E) of the reduction tests


def brute_games(A, B, C, E):
    """-> {game number: ((role, index) of the adversary, of agent_0, of agent_1, episode)} by the formula of the issue"""
    out = {}
    for a in range(A):
        for b in range(B):
            for c in range(C):
                for e in range(E):
                    out[((a * B + b) * C + c) * E + e] = (("adversary_0", c), ("agent_0", a), ("agent_1", b), e)
    return out


def brute_games2(A, B, E):
    return {(a * B + b) * E + e: (("first_0", a), ("second_0", b), e) for a in range(A) for b in range(B) for e in range(E)}


def reduce_ref(rewards, A, B, C, E):
    """rewards [A B C E][3] -> (payoff [A B C][3], marg_a [A][3], marg_b [B][3], marg_c [C][3]): every word one left-to-right
    chain of IEEE double additions from +0.0 and one division - main.py's `total += reward; total / episodes`"""
    r = np.asarray(rewards, dtype=np.float64).reshape(A * B * C, E, 3)
    payoff = np.zeros((A * B * C, 3))
    with np.errstate(all="ignore"):
        for t in range(A * B * C):
            for s in range(3):
                tot = np.float64(0.0)
                for e in range(E):
                    tot = tot + r[t, e, s]
                payoff[t, s] = tot / np.float64(E)
        marg = [np.zeros((n, 3)) for n in (A, B, C)]
        for role, n in enumerate((A, B, C)):
            for i in range(n):
                for s in range(3):
                    tot, count = np.float64(0.0), 0
                    for t in range(A * B * C):   # ascending t
                        if ((t // (B * C)), (t // C) % B, t % C)[role] == i:
                            tot = tot + payoff[t, s]
                            count += 1
                    marg[role][i, s] = tot / np.float64(count)
    return (payoff, *marg)


def numpy_sum_payoff(rewards, A, B, C, E):
    """the payoff table as np.sum adds it (pairwise / eight-way unrolled from 8 terms on): another order"""
    r = np.ascontiguousarray(np.asarray(rewards, dtype=np.float64).reshape(A * B * C, E, 3).transpose(0, 2, 1))
    with np.errstate(all="ignore"):
        return np.sum(r, axis=2) / np.float64(E)


def reversed_payoff(rewards, A, B, C, E):
    """... and as a right-to-left chain adds it"""
    r = np.asarray(rewards, dtype=np.float64).reshape(A * B * C, E, 3)
    return reduce_ref(r[:, ::-1], A, B, C, E)[0]


# ---- reward tables
def normal_rewards(A, B, C, E, seed=0):
    """seeded normals x 1e8: full mantissas, so nearly every addition rounds"""
    g = np.random.Generator(np.random.PCG64(seed))
    return g.standard_normal((A * B * C * E, 3)) * 1e8


_PATTERN = (1.0, 1e16, -1e16, 0.5, 3.0, -1e16, 1e16, 2.0 ** -30)


def cancellation_rewards(A, B, C, E):
    """huge terms that cancel around small ones (1e16 + 1.0 is 1e16): the sum depends on the order of its terms"""
    g, s = np.meshgrid(np.arange(A * B * C * E), np.arange(3), indexing="ij")
    return np.asarray(_PATTERN)[(g + 3 * s + 5 * (g // E)) % len(_PATTERN)]


def negative_zero_rewards(A, B, C, E):
    """all -0.0: a chain that starts from +0.0 ends at +0.0, one that starts from its first term at -0.0"""
    return np.full((A * B * C * E, 3), -0.0)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
