"""Surface normals and the surface variation of every point, for a whole ragged batch of clouds on the device.

Nothing else in the package knows the local surface at a point, and three things want it: point-to-plane ICP
(`registration.icp_refine(estimation='point_to_plane')`, which needs the target's normals), descriptors and input features
built on normals, and planarity / curvature filters.  open3d offers `estimate_normals(KDTreeSearchParamKNN(knn))`; it is not
a dependency and works through a float64 k-d tree, so this module DEFINES the estimate, as `outliers.py` defines its filter.
**Parity with open3d is not claimed.**  The numpy route (`estimate_normals_host`) is this definition; the device route is
compared with it.

Definition, for one cloud of n finite fp32 points, `nb_neighbors` an integer in 3..32 and k = min(`nb_neighbors`, n):

 1. Squared distance: d2(i, j) exactly as in `outliers.py` step 1 -- fp32 on the differences, (dx dx + dy dy) + dz dz,
    every operation rounded once.  The point itself is included.
 2. Neighbourhood: r2_i is the k-th smallest d2(i, .), N(i) = { j : d2(i, j) <= r2_i }.  Ties at the k-th place are ALL
    included, so |N(i)| >= k, and N(i) is a pure function of the input: it depends neither on a scan order nor on the
    search grid.  counts[i] = |N(i)| (int32).
 3. Covariance, in float64 about the query point itself, so no mean is subtracted from large coordinates:
    e_j = float64(p_j) - float64(p_i), S1 = sum e_j, S2 = sum e_j e_j^T (6 unique entries), m = |N(i)|,
    C = S2 / m - (S1 / m)(S1 / m)^T.
 4. Eigen-decomposition: the one-sided cyclic Jacobi of `registration.py` on the symmetric 3 x 3 C in float64 -- G = C V,
    `JACOBI_SWEEPS` = 12 sweeps over the column pairs (0,1), (0,2), (1,2) until G's columns are orthogonal; their norms are
    the eigenvalues of the positive semi-definite C, V's columns the eigenvectors.  Ordered l0 <= l1 <= l2 (the largest
    first, then the larger of the other two, the lowest column on a tie): normal = the column of V at l0, a unit vector;
    curvature = l0 / ((l0 + l1) + l2), the "surface variation", 0 when the sum is 0.
 5. Degenerate points: m < 3, or l1 <= 1e-12 l2 (a coincident or collinear neighbourhood; a NaN too): normal = (0, 0, 0)
    and curvature = 0.  **A zero normal is the marker for "no normal"**; point-to-plane ICP relies on it.
 6. Sign.  With `viewpoint` (one (3,) point per cloud, or one for all, taken as float64): flip so that
    (nx (vx - px) + ny (vy - py)) + nz (vz - pz) >= 0 in float64.  Without: "upward" -- flip so that n_z > 0, or, if
    n_z == 0, n_y > 0, or, if that is 0 too, n_x > 0.
 7. Outputs, rounded once to fp32: normals (n, 3), curvature (n,); counts (n,) int32.

Radius and hybrid neighbourhoods (`radius=`; after open3d's `KDTreeSearchParamHybrid(radius,
max_nn)` and `KDTreeSearchParamRadius`, parity again not claimed).  A k-nearest neighbourhood has no physical size: it
shrinks where a cloud is dense and grows where it is sparse, so two clouds of different density describe different patches
of one surface.  `radius` is a float, positive and finite in fp32, and R2 = `global_registration.inlier_d2(radius)`, the
largest fp32 d2 with sqrtf(d2) <= float32(radius): "within the radius" means exactly what "within
`max_correspondence_distance`" means to ICP and RANSAC.  Only step 2 changes:

 * **Hybrid** (`nb_neighbors` in 3..32 and a radius): r2_i = min(k-th smallest d2(i, .), R2), N(i) = { j : d2(i, j) <=
   r2_i }, ties included as before.  |N(i)| may now lie below k, down to 1 (the point itself, which then has no normal by
   step 5).  `nb_neighbors` stays in 3..32 -- the sorted register list of the search is 32 floats at the most -- so open3d's
   usual `max_nn=100` is not reachable; radius-only is the route to larger neighbourhoods.
 * **Radius-only** (`nb_neighbors=None` and a radius): r2_i = R2, that is hybrid with k = n.  |N(i)| has no cap; counts
   stay int32.  Every point of 27 grid cells of edge >= radius is visited per query: a very large radius on a large cloud
   is quadratic work per thread.
 * `radius=None` is the k-nearest definition above with the bits it always had.

Steps 3 to 7 are unchanged.  On the device the grid takes the radius into account (`outliers.grid_layout`): at the default
cell of a radius-only call no point is left to the whole-cloud scan, and there is no list and no first scan.

Device route (`csrc/normals.hip`): `outliers.sorted_batch` unchanged (bounds, the finite check with
its one host read, grid layout, keys, sort, gather), then `hfl_knn_normals`: the cell-start table; one thread per point
scanning the 3 x 3 x 3 cells round its own twice -- first for r2 with the sorted register list and the completeness bound
of `hfl_knn_mean_dist`, then for the float64 sums over every point with d2 <= r2 in sorted-position order -- and finishing
with the Jacobi, the sign rule and the stores; the points the bound cannot prove go to a whole-cloud scan, a wave per
point, whose lanes' sums are combined by the xor butterfly 32 .. 1.  counts and the set of zero normals equal the numpy
route's; the float64 sums are taken in another order (that of the sort and the grid; `torch.sort` on the device is a radix
sort whose result is a function of its input, so the order is fixed and two runs give the same bits), so normals and
curvature agree with the numpy route, and between two `cell_size`, to rounding: where (l1 - l0) / l2 > 1e-6 a sum-order
difference of about 1e-15 is amplified by at most 1e6, far below an fp32 ulp.

Batch limits as in `ragged.py`."""

from typing import Sequence

import numpy as np
import torch

from . import ops, outliers, ragged
from .registration import JACOBI_SWEEPS

MIN_NEIGHBOURS, MAX_NEIGHBOURS = 3, ops.KNN_MAX_NEIGHBOURS
RANK_TOL = 1e-12                       # l1 <= RANK_TOL x l2: no normal
_HOST_CHUNK = 1 << 21                  # point pairs of one temporary of the numpy route


def _check_neighbours(nb_neighbors) -> int:
    if isinstance(nb_neighbors, bool) or not isinstance(nb_neighbors, (int, np.integer)) or \
            not MIN_NEIGHBOURS <= int(nb_neighbors) <= MAX_NEIGHBOURS:
        raise ValueError('nb_neighbors must be an integer in %d..%d, got %r' % (MIN_NEIGHBOURS, MAX_NEIGHBOURS, nb_neighbors))
    return int(nb_neighbors)


def _check_viewpoint(viewpoint, batch: int):
    """None, or the (batch, 3) float64 viewpoints: one (3,) point serves every cloud"""
    if viewpoint is None:
        return None
    v = np.asarray(viewpoint.detach().cpu().numpy() if isinstance(viewpoint, torch.Tensor) else viewpoint, dtype=np.float64)
    if v.shape == (3,):
        v = np.tile(v, (batch, 1))
    if v.shape != (batch, 3):
        raise ValueError('viewpoint must be one (3,) point or (%d, 3), one per cloud, got shape %s' % (batch, v.shape))
    if not np.isfinite(v).all():
        raise ValueError('viewpoint holds a coordinate that is not finite')
    return np.ascontiguousarray(v)


# ------------------------------------------------------------------------------------------------ host route (numpy)
def _rotate(g, v, p, q):
    """`jacobi_rotate` of csrc/jacobi3.h on (n, 3, 3) stacks: where gamma == 0 a matrix is left alone"""
    alpha = g[:, 0, p] * g[:, 0, p] + g[:, 1, p] * g[:, 1, p] + g[:, 2, p] * g[:, 2, p]
    beta = g[:, 0, q] * g[:, 0, q] + g[:, 1, q] * g[:, 1, q] + g[:, 2, q] * g[:, 2, q]
    gamma = g[:, 0, p] * g[:, 0, q] + g[:, 1, p] * g[:, 1, q] + g[:, 2, p] * g[:, 2, q]
    live = gamma != 0.0
    zeta = (beta - alpha) / (2.0 * np.where(live, gamma, 1.0))
    t = np.where(zeta >= 0.0, 1.0, -1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
    c = 1.0 / np.sqrt(1.0 + t * t)
    s = c * t
    for m in (g, v):
        for i in range(3):
            mp, mq = m[:, i, p].copy(), m[:, i, q].copy()
            m[:, i, p] = np.where(live, c * mp - s * mq, mp)
            m[:, i, q] = np.where(live, s * mp + c * mq, mq)


def _eigen_host(s1, s2, m):
    """steps 3 to 5 for a stack of points: S1 (n, 3), S2 (n, 6: xx, xy, xz, yy, yz, zz), m (n,) -> (normal (n, 3) float64
    before the sign rule, zero where there is none; curvature (n,); the eigenvalues (n, 3) ascending, NaN where m < 3)"""
    n = m.shape[0]
    with np.errstate(all='ignore'):
        dm = m.astype(np.float64)
        mu = s1 / dm[:, None]
        g = np.empty((n, 3, 3), np.float64)
        for slot, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            g[:, a, b] = s2[:, slot] / dm - mu[:, a] * mu[:, b]
            g[:, b, a] = g[:, a, b]
        v = np.tile(np.eye(3), (n, 1, 1))
        for _ in range(JACOBI_SWEEPS):
            _rotate(g, v, 0, 1)
            _rotate(g, v, 0, 2)
            _rotate(g, v, 1, 2)
        w = np.sqrt(g[:, 0, :] * g[:, 0, :] + g[:, 1, :] * g[:, 1, :] + g[:, 2, :] * g[:, 2, :])
        i2 = np.where((w[:, 0] >= w[:, 1]) & (w[:, 0] >= w[:, 2]), 0, np.where(w[:, 1] >= w[:, 2], 1, 2))
        ja, jb = np.where(i2 == 0, 1, 0), np.where(i2 == 2, 1, 2)
        rows = np.arange(n)
        first = w[rows, ja] >= w[rows, jb]
        i1, i0 = np.where(first, ja, jb), np.where(first, jb, ja)
        l0, l1, l2 = w[rows, i0], w[rows, i1], w[rows, i2]
        good = (m >= 3) & (l1 > RANK_TOL * l2)
        normal = np.where(good[:, None], v[rows, :, i0], 0.0)
        total = (l0 + l1) + l2
        curvature = np.where(good & (total > 0.0), l0 / np.where(total > 0.0, total, 1.0), 0.0)
        lam = np.where((m >= 3)[:, None], np.stack([l0, l1, l2], 1), np.nan)
    return normal, curvature, lam


def _signed(normal, pts, view):
    """step 6 on float64 normals; a zero normal stays zero"""
    nx, ny, nz = normal[:, 0], normal[:, 1], normal[:, 2]
    if view is not None:
        p = pts.astype(np.float64)
        dot = (nx * (view[0] - p[:, 0]) + ny * (view[1] - p[:, 1])) + nz * (view[2] - p[:, 2])
        flip = dot < 0.0
    else:
        flip = (nz < 0.0) | ((nz == 0.0) & ((ny < 0.0) | ((ny == 0.0) & (nx < 0.0))))
    return np.where(flip[:, None], -normal, normal)


def _normals_host(a: np.ndarray, nb, view, cap=None):
    """steps 1 to 6 for one (n, 3) fp32 cloud by brute force in row chunks -> (normals, curvature, both float64: step 7
    rounds them; counts int32; eigenvalues (n, 3) float64).  `cap`: None or R2 (fp32); `nb` None: radius-only"""
    n = a.shape[0]
    k = n if nb is None else min(nb, n)
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    a64 = a.astype(np.float64)
    s1, s2, counts = np.empty((n, 3), np.float64), np.empty((n, 6), np.float64), np.empty(n, np.int32)
    chunk = max(1, _HOST_CHUNK // n)
    with np.errstate(over='ignore', invalid='ignore'):
        for s in range(0, n, chunk):
            e = min(n, s + chunk)
            dx, dy, dz = x[s:e, None] - x[None, :], y[s:e, None] - y[None, :], z[s:e, None] - z[None, :]
            d2 = (dx * dx + dy * dy) + dz * dz                   # fp32 arrays: every operation rounded once
            if nb is None:
                r2 = np.full(e - s, cap, np.float32)
            else:
                r2 = np.partition(d2, k - 1, axis=1)[:, k - 1]
                if cap is not None:
                    r2 = np.minimum(r2, cap)
            near = d2 <= r2[:, None]
            counts[s:e] = near.sum(1)
            diff = np.where(near[:, :, None], a64[None, :, :] - a64[s:e, None, :], 0.0)
            s1[s:e] = diff.sum(1)
            for slot, (p, q) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                s2[s:e, slot] = (diff[:, :, p] * diff[:, :, q]).sum(1)
    normal, curvature, lam = _eigen_host(s1, s2, counts)
    return _signed(normal, a, view), curvature, counts, lam


def estimate_normals_host(clouds: Sequence, nb_neighbors=30, *, radius=None, viewpoint=None, return_curvature: bool = False,
                          return_counts: bool = False, return_eigenvalues: bool = False):
    """The definition of the module docstring in numpy, fp32 for the distances and float64 for the rest: the route without
    a GPU and the yardstick of the tests.  Brute force, O(n^2): meant for tests and small clouds.  List of (n_i, 3) clouds
    -> list of (n_i, 3) float32 unit normals, zero where a point has none; with `return_curvature` also the (n_i,) float32
    surface variation, with `return_counts` the (n_i,) int32 neighbourhood sizes, with `return_eigenvalues` the (n_i, 3)
    float64 eigenvalues in ascending order (NaN where fewer than three neighbours), by which a caller judges how well a
    normal is determined.  `radius`: the hybrid neighbourhood, or, with `nb_neighbors=None`, the radius-only one."""
    nb, r = outliers.check_neighbourhood(nb_neighbors, radius, _check_neighbours)
    cap = None if r is None else outliers.radius2(r)
    arrays = outliers._checked_arrays(clouds)
    views = _check_viewpoint(viewpoint, len(arrays))
    parts = [_normals_host(a, nb, None if views is None else views[i], cap) for i, a in enumerate(arrays)]
    return ragged.results([p[0].astype(np.float32) for p in parts],
                          [p[1].astype(np.float32) for p in parts] if return_curvature else None,
                          [p[2] for p in parts] if return_counts else None,
                          [p[3] for p in parts] if return_eigenvalues else None)


# ------------------------------------------------------------------------------------------------ device route
def estimate_normals_packed(packed, nb, views=None, cell=None, radius=None):
    """the estimate on a packed batch -> (normals (P, 3) fp32, curvature (P,) fp32, counts (P,) int32, pending (1,) int32),
    everything on the device; `views` None or (B, 3) float64 numpy; `nb` and `radius` as `outliers.check_neighbourhood`
    returns them"""
    table, sorted_pts, sorted_keys, perm = outliers.sorted_batch(packed, nb, cell, radius)
    dev_views = None if views is None else torch.from_numpy(views).to(packed.pts.device)
    return ops.knn_normals(sorted_pts, sorted_keys, perm, packed.off, table, dev_views,
                           radius2=None if radius is None else outliers.radius2(radius), radius_only=nb is None)


def estimate_normals(clouds: Sequence, nb_neighbors=30, *, radius=None, viewpoint=None, device='cuda', cell_size=None,
                     return_curvature: bool = False, return_counts: bool = False, return_pending: bool = False):
    """`estimate_normals_host` on the device: list of raw (n_i, 3) clouds (numpy / torch, host or device) -> list of
    (n_i, 3) float32 device tensors, the unit normals of the module docstring, zero where a point has none.
    `viewpoint`: one (3,) point, or (B, 3) with one per cloud, towards which the normals are turned; None turns them
    upward.  `return_curvature`: also the (n_i,) float32 surface variation; `return_counts`: the (n_i,) int32 neighbourhood
    sizes, equal to the numpy route's; `return_pending`: the number of points of the batch that the whole-cloud scan
    finished (a debug counter).  `cell_size` sets the edge of the search grid's cells: it changes no count and no zero
    normal, and the rest only to rounding.  `radius`: the hybrid neighbourhood of the module docstring, or, with
    `nb_neighbors=None`, the radius-only one (no point pending at the default cell).  `ValueError` for a bad parameter or
    an empty cloud (before the device is touched) and, naming the cloud, for a coordinate that is not finite (before any
    kernel of the estimate runs)."""
    nb, r = outliers.check_neighbourhood(nb_neighbors, radius, _check_neighbours)
    cell = None if cell_size is None else ragged.check_positive('cell_size', cell_size)
    views = _check_viewpoint(viewpoint, len(clouds))
    with ragged.intake(clouds, device) as packed:
        if packed is None:
            return ragged.results([], [] if return_curvature else None, [] if return_counts else None,
                                  0 if return_pending else None)
        normals, curvature, counts, pending = estimate_normals_packed(packed, nb, views, cell, r)
        return ragged.results(packed.split(normals), packed.split(curvature) if return_curvature else None,
                              packed.split(counts) if return_counts else None,
                              int(pending.item()) if return_pending else None)
