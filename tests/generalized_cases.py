"""Inputs and helpers of the generalized-ICP tests (`tests/test_generalized_icp_host.py`,
`tests/test_gpu_registration_generalized.py`).  Everything is seeded and float32; what costs something on the host is computed
once (`functools.lru_cache`) and must be left unchanged.

`rows_by_linear_algebra` is the row of the definition written with matrices -- `numpy.linalg.inv` of C, explicit J -- against
which the host route's fixed-order row (`registration._host_generalized_rows`) is checked; the device's sums are then checked
against that host row on the device's own correspondences."""
import functools
import os

import numpy as np

from hotformerloc_amd import estimate_normals_host, icp_refine_host
from tests import normals_cases as nc
from tests import registration_cases as rc

EPS = 1e-3                             # the default covariance_epsilon
MAX_DIST = 1.0                         # max_correspondence_distance of the corner cases
NB = 20                                # neighbours of the normals
CORNERS = (dict(), dict(n_source=1500, n_target=600), dict(seed=3))    # the three cases of the purpose
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'registration_plane_corner.npz')


def unit_normals(rows, seed, zero_every=0, phase=0):
    """seeded unit vectors rounded to fp32; every `zero_every`-th row from `phase` on the "no normal" marker"""
    v = np.random.default_rng(seed).normal(0.0, 1.0, (rows, 3))
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    if zero_every:
        v[phase::zero_every] = 0.0
    return v


def cross_matrix(p):
    return np.array([[0.0, -p[2], p[1]], [p[2], 0.0, -p[0]], [-p[1], p[0], 0.0]])


def covariance(a, b, eps=EPS):
    """C = (I - (1 - eps) a a^T) + (I - (1 - eps) b b^T) of one row, float64"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 2.0 * np.eye(3) - (1.0 - eps) * (np.outer(a, a) + np.outer(b, b))


def rows_by_linear_algebra(p, q, a, b, eps=EPS):
    """per row (M (3, 3), g = J^T M r (6,), A = J^T M J (6, 6)) with M = `numpy.linalg.inv`(C) and J = (-[p]x | I)"""
    out = []
    for pp, qq, aa, bb in zip(*(np.asarray(x, np.float64) for x in (p, q, a, b))):
        m = np.linalg.inv(covariance(aa, bb, eps))
        jac = np.concatenate([-cross_matrix(pp), np.eye(3)], 1)
        out.append((m, jac.T @ m @ (pp - qq), jac.T @ m @ jac))
    return out


def blocks_of(row):
    """(g (6,), A (6, 6) symmetric, M (3, 3)) of one (29,) row of the host route"""
    a = np.zeros((6, 6))
    a[np.triu_indices(6)] = row[8:]
    a = a + np.triu(a, 1).T
    return np.asarray(row[2:8], np.float64), a, a[3:, 3:]


@functools.lru_cache(maxsize=None)
def corner(**kw):
    """(source, target, G, source normals, target normals) of `normals_cases.corner_pair(**kw)`, the normals from the host"""
    src, dst, g = nc.corner_pair(**kw)
    ns, nt = estimate_normals_host([src, dst], NB)
    return src, dst, g, ns, nt


@functools.lru_cache(maxsize=None)
def corner_runs(**kw):
    """(G, point-to-plane result, generalized result) of one corner on the host route, from the identity"""
    src, dst, g, ns, nt = corner(**kw)
    plane = icp_refine_host([src], [dst], max_correspondence_distance=MAX_DIST, estimation='point_to_plane', target_normals=[nt])
    gen = icp_refine_host([src], [dst], max_correspondence_distance=MAX_DIST, estimation='generalized', target_normals=[nt],
                          source_normals=[ns])
    return g, plane, gen


def flat_pair():
    """(source, target, source normals, target normals): a flat target under exactly vertical normals, the source its first
    150 points -- three zero rows in the A of point-to-plane"""
    flat = rc.target(400) * np.float32([1.0, 1.0, 0.0])
    up = np.tile(np.float32([0.0, 0.0, 1.0]), (len(flat), 1))
    return flat[:150].copy(), flat, up[:150].copy(), up


@functools.lru_cache(maxsize=None)
def loop_batch():
    """P = 4, the `loop_batch` of tests/test_gpu_registration_plane.py with normals on both sides: two corners (different
    seeds and motions), a pair whose every point is beyond the distance (TOO_FEW), and the flat target under vertical
    normals; the host route's generalized and point-to-plane results"""
    c0, c1 = nc.corner_pair(seed=0), nc.corner_pair(600, 2100, seed=4, deg=-2.0, shift=0.1)
    f_src, f_dst, f_ns, f_nt = flat_pair()
    srcs = [c0[0], c1[0], rc.far_points(100, 9), f_src]
    dsts = [c0[1], c1[1], rc.target(300), f_dst]
    n_t = list(estimate_normals_host(dsts[:3], NB)) + [f_nt]
    n_s = list(estimate_normals_host(srcs[:3], NB)) + [f_ns]
    host = icp_refine_host(srcs, dsts, max_correspondence_distance=MAX_DIST, estimation='generalized', target_normals=n_t,
                           source_normals=n_s)
    plane = icp_refine_host(srcs, dsts, max_correspondence_distance=MAX_DIST, estimation='point_to_plane', target_normals=n_t)
    return dict(srcs=srcs, dsts=dsts, n_s=n_s, n_t=n_t, g=[c0[2], c1[2]], host=host, plane=plane)


def orthonormal(r, tol=1e-12):
    return np.abs(r.T @ r - np.eye(3)).max() <= tol and abs(np.linalg.det(r) - 1.0) <= tol
