"""Seeded inputs, an exact case and an independent yardstick for the spectral-verification tests
(`tests/test_spectral_host.py`, `tests/test_gpu_spectral.py`).  Everything is float32 and read-only; what costs something on
the host is computed once (`functools.lru_cache`) and must not be written to."""
import functools

import numpy as np

import hotformerloc_amd as hfl
from hotformerloc_amd import ops
from tests import fpfh_cases as fc
from tests import global_registration_cases as gc

SIGMA, ITERATIONS = 0.2, 10            # the yardstick and purpose cases: a fifth of the clouds' spacing
FRACTIONS = (0.0, 0.6, 0.9, 1.0)
R, T = ops.SPECTRAL_ROWS, ops.SPECTRAL_TILE
C_SIZES = (0, 1, 2, 3, R - 1, R, R + 1, T - 1, T, T + 1, 2 * T + 1)    # every size round a workgroup's rows and an LDS tile
K_SIZES = (1, 2, 10)
RAGGED_SEED = 5
QUERY = 'planes_moved'
DATABASE = ('duplicated', 'plane37', 'collinear', 'planes700', 'planes')
EXPECTED_ORDER = ('planes', 'planes700', 'duplicated', 'plane37', 'collinear')


def dense_eigenvalues(src, dst, rows, sigma):
    """the eigenvalues, ascending, of the consistency matrix built densely in float64: `numpy.linalg.eigvalsh`, no code of
    the package"""
    p, q = src[rows[:, 0]].astype(np.float64), dst[rows[:, 1]].astype(np.float64)
    a = np.sqrt(((p[:, None] - p[None]) ** 2).sum(2))
    b = np.sqrt(((q[:, None] - q[None]) ** 2).sum(2))
    m = np.maximum(0.0, 1.0 - (a - b) ** 2 / sigma ** 2)
    np.fill_diagonal(m, 0.0)
    return np.linalg.eigvalsh(m)


@functools.lru_cache(maxsize=None)
def host_corrupted(frac):
    """the host result on `corrupted(frac)` with SIGMA and ITERATIONS, shared"""
    src, dst, rows = gc.corrupted(frac)
    return hfl.spectral_consistency_host([src], [dst], [rows], distance_threshold=SIGMA, iterations=ITERATIONS)


@functools.lru_cache(maxsize=None)
def exact_case(n_true=16, n_corr=40, seed=3):
    """(source, target, rows, true mask): `n_corr` integer points in +-8; `n_true` of them, at seeded places, are paired with
    their image under a 90 degree turn plus an integer shift, the target of every other correspondence c lies at (1000 (c +
    1), 0, 0).  Every squared length is an integer, so every entry of M is exactly 1 inside the true block and exactly 0
    outside.  With n_true a power of four the iterates are exact as well: v = 1 / sqrt(n_true) inside, w = (n_true - 1) v."""
    rng = np.random.default_rng(seed)
    src = rng.integers(-8, 9, (n_corr, 3))
    true = np.zeros(n_corr, bool)
    true[rng.permutation(n_corr)[:n_true]] = True
    turned = np.stack([-src[:, 1] + 1, src[:, 0] + 2, src[:, 2] + 3], 1)               # rz by 90 degrees, then (1, 2, 3)
    far = np.stack([1000 * (np.arange(n_corr) + 1), np.zeros(n_corr, np.int64), np.zeros(n_corr, np.int64)], 1)
    dst = np.where(true[:, None], turned, far)
    rows = np.stack([np.arange(n_corr), np.arange(n_corr)], 1).astype(np.int64)
    out = (src.astype(np.float32), dst.astype(np.float32), rows, true)
    for a in out:
        a.setflags(write=False)
    return out


def ragged_batch():
    """(sources, targets, rows): the two plane clouds with one pair per size of C_SIZES, 30 % of the rows wrong"""
    src, dst = gc.clouds()
    return [src] * len(C_SIZES), [dst] * len(C_SIZES), [gc.rows(c, 0.3, RAGGED_SEED + i) for i, c in enumerate(C_SIZES)]


@functools.lru_cache(maxsize=None)
def host_ragged(iterations):
    """the host result on `ragged_batch()` with the default threshold, shared"""
    return hfl.spectral_consistency_host(*ragged_batch(), iterations=iterations)


def rerank_inputs():
    """(queries, database, candidates (1, 6)): the moved corner against five clouds, retrieved in the order of DATABASE, and
    one unused slot"""
    return [fc.cloud_of(QUERY)], [fc.cloud_of(n) for n in DATABASE], np.array([[0, 1, 2, 3, 4, -1]], np.int64)


@functools.lru_cache(maxsize=None)
def host_rerank(register=False):
    return hfl.rerank_candidates_host(*rerank_inputs(), register=register)


def rerank_truth():
    """(3, 4): the pose query frame -> frame of 'planes', the inverse of `global_registration_cases.truth`"""
    return np.linalg.inv(np.vstack([gc.truth(), [0.0, 0.0, 0.0, 1.0]]))[:3]
