"""Seeded inputs, an exact case with its hand values and an independent yardstick for the consensus-registration tests
(`tests/test_consensus_host.py`, `tests/test_gpu_consensus.py`).  Everything is read-only; what costs something on the host
is computed once (`functools.lru_cache`) and must not be written to."""
import functools

import numpy as np

import hotformerloc_amd as hfl
from tests import global_registration_cases as gc
from tests import spectral_cases as sc

DISTANCE = 0.1                         # d of the ragged batch and of the purpose cases: a tenth of the clouds' spacing
SEEDS, SIZE = 64, 10                   # S and k1 of the purpose cases, the defaults
# a word, a 128-bit group, a workgroup's rows and an LDS tile, each with both neighbours
C_SIZES = (0, 1, 2, 3, 31, 32, 33, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 2049)
RAGGED_SEED = 5
S_SIZES = (1, 63, 64, 65, 300)
K_SIZES = (3, 10, 64)
PURPOSE_FRACTIONS = (0.6, 0.9, 0.95, 0.97, 0.98)       # consensus finds the pose at every one of them
RANSAC_FAILS_AT = (0.95, 0.97)                         # where 4 096 drawn triples do not
EXACT_DISTANCE = 0.5
GUARD_ULPS = 4


def ragged_batch(sizes=C_SIZES, seed=RAGGED_SEED):
    """(sources, targets, rows): the two plane clouds with one pair per size, 30 % of the rows wrong"""
    src, dst = gc.clouds()
    return [src] * len(sizes), [dst] * len(sizes), [gc.rows(c, 0.3, seed + i) for i, c in enumerate(sizes)]


@functools.lru_cache(maxsize=None)
def host_ragged(seeds=SEEDS, size=SIZE):
    """`consensus_hypotheses_host(return_details=True)` on `ragged_batch()` with DISTANCE, shared"""
    return hfl.consensus_hypotheses_host(*ragged_batch(), distance_threshold=DISTANCE, seeds=seeds, consensus_size=size,
                                         return_details=True)


@functools.lru_cache(maxsize=None)
def host_sized(sizes, seeds, size):
    """the same on `ragged_batch(sizes)`, `sizes` a tuple"""
    return hfl.consensus_hypotheses_host(*ragged_batch(sizes), distance_threshold=DISTANCE, seeds=seeds,
                                         consensus_size=size, return_details=True)


@functools.lru_cache(maxsize=None)
def host_purpose(frac):
    src, dst, rows = gc.corrupted(frac)
    return hfl.consensus_registration_host([src], [dst], [rows], distance_threshold=DISTANCE, seeds=SEEDS,
                                           consensus_size=SIZE, max_correspondence_distance=gc.TAU)


# ---------------------------------------------------------------------------------------------------------------- yardstick
def dense_lengths(src, dst, rows):
    """(a, b): the (C, C) float64 lengths |p_i - p_j| and |q_i - q_j|, no code of the package"""
    p, q = src[rows[:, 0]].astype(np.float64), dst[rows[:, 1]].astype(np.float64)
    return np.sqrt(((p[:, None] - p[None]) ** 2).sum(2)), np.sqrt(((q[:, None] - q[None]) ** 2).sum(2))


def dense_graph(src, dst, rows, d):
    """(B (C, C) bool, deg (C,), n (C, C) with n[s, j] = B_sj sum_k B_sk B_jk) built densely in float64 and integers"""
    a, b = dense_lengths(src, dst, rows)
    graph = np.abs(a - b) <= np.float64(np.float32(d))
    np.fill_diagonal(graph, False)
    wide = graph.astype(np.float64)                                    # integers below 2^53: the product is exact
    return graph, graph.sum(1), ((wide @ wide) * wide).astype(np.int64)


def guard_lengths(src, dst, rows, d, ulps=GUARD_ULPS):
    """asserts that no | |e| - d | of the float64 construction is as small as `ulps` fp32 ulps of the largest of a, b and d.
    The fp32 e = a - b carries the rounding of its two roots and their d2 chains, which is of the size of an ulp of the
    LENGTHS (metres here), not of d: nearer to d than that, fp32 and float64 may decide differently and neither is wrong.
    The margin is never smaller than `ulps` ulps of d."""
    a, b = dense_lengths(src, dst, rows)
    d32 = np.float32(d)
    margin = ulps * np.spacing(np.maximum(np.maximum(a, b), np.float64(d32)).astype(np.float32)).astype(np.float64)
    near = np.abs(np.abs(a - b) - np.float64(d32)) <= margin
    np.fill_diagonal(near, False)
    assert not near.any(), '%d entries with |e| within %d ulps of d' % (int(near.sum()) // 2, ulps)


# --------------------------------------------------------------------------------------------------------------- exact case
def exact_expected(seeds=SEEDS, size=SIZE):
    """the hand values of `spectral_cases.exact_case()` (integer points, 16 true of 40) with d = 0.5: every B entry is
    exactly 1 inside the true block and 0 outside, so deg = 15 on true rows and 0 elsewhere, n_sj = 14 inside the block, the
    seeds are the true rows in index order and then the rest, a true seed's set is itself and the `size` - 1 lowest other
    true rows, a false seed's set has size 1 and is invalid -> dict(degree, seeds, valid, members, support)"""
    true = sc.exact_case()[3]
    n_corr, at = true.shape[0], np.nonzero(true)[0]
    order = np.concatenate([at, np.nonzero(~true)[0]])
    seed_rows = np.full(seeds, -1, np.int64)
    seed_rows[:min(seeds, n_corr)] = order[:seeds]
    valid = np.zeros(seeds, bool)
    valid[:min(seeds, at.shape[0])] = True
    members = np.full((seeds, size), -1, np.int64)
    for h in np.nonzero(valid)[0]:
        others = at[at != seed_rows[h]][:size - 1]
        members[h, :others.shape[0] + 1] = np.sort(np.append(others, seed_rows[h]))
    return dict(degree=np.where(true, at.shape[0] - 1, 0).astype(np.int32), seeds=seed_rows, valid=valid, members=members,
                support=np.where(valid, at.shape[0] - 2, 0).astype(np.int64))
