"""Intrinsic Shape Signatures keypoints for a whole ragged batch of clouds on the device.

Every step from two raw submaps to a pose (`estimate_normals` -> `compute_fpfh` -> `feature_correspondences` ->
`ransac_registration` / `consensus_registration`, and `spectral_consistency` on the way back to the ranking) otherwise runs
on every point of every cloud, and matching and verification are quadratic in what they are given.  The usual detector in
front of a descriptor matcher for lidar is ISS (Zhong 2009; open3d's `compute_iss_keypoints`): it keeps the few per cent of
the points where the surface bends in all three directions.  open3d is not a dependency and works through a float64 k-d
tree, so this module DEFINES the detector, as `normals.py` defines its estimate.  **Parity with open3d is not claimed.**
The numpy route (`*_host`) is this definition; the device route is compared with it.

Definition, for one cloud of n finite fp32 points, `salient_radius` and `non_max_radius` positive and finite in fp32,
`gamma_21` and `gamma_32` in (0, 1], `min_neighbors` an integer >= 1:

 1. Squared distance: d2(i, j) exactly as in `outliers.py` step 1.  R2s = `inlier_d2(salient_radius)` and R2n =
    `inlier_d2(non_max_radius)`, the inclusive fp32 thresholds every other module uses: "within the radius" means what it
    means to `estimate_normals(radius=)`, `remove_radius_outliers` and the ICP.
 2. m_i = |{ j : d2(i, j) <= R2s }|, the point itself included: `radius_neighbour_counts(clouds, salient_radius)`.
 3. Covariance and eigenvalues l0 <= l1 <= l2 exactly as `normals.py` steps 3 and 4 over that neighbourhood: float64 sums
    about the query point, C = S2 / m - mu mu^T, the one-sided Jacobi with `JACOBI_SWEEPS`.  The saliency is the smallest
    eigenvalue of the covariance about the neighbourhood's MEAN, so it does not change when the cloud is shifted.  A
    neighbourhood of fewer than three points has no eigenvalues (NaN, as `estimate_normals_host(return_eigenvalues=True)`
    reports them).
 4. Saliency: s_i = float32(l0) where m_i >= `min_neighbors`, l1 < gamma_21 l2 and l0 < gamma_32 l1 all hold, and 0
    elsewhere.  The products are float64, nothing is divided, and a NaN fails the test.  **The rounding to fp32 is part of
    the definition**: two nearby points with the same neighbour set have mathematically equal saliency, their float64
    values differ by rounding only (on `tests/fpfh_cases.py`'s 'planes' cloud at radii 1.5 / 1.0, 30 pairs of ball
    neighbours are bit-equal in fp32), and a suppression that compared float64 values would let the order of a sum decide
    those pairs.
 5. Selection: c_i = |{ j : d2(i, j) <= R2n }|.  Point i is a keypoint iff s_i > 0, c_i >= `min_neighbors`, and no j of
    that ball has s_j > s_i, or s_j == s_i with j < i: ties go to the lower index.  Integers and comparisons only: the
    selection is a pure function of the points and the fp32 saliency (`iss_select` takes any fp32 saliency; a value that
    is not > 0, a NaN included, is no candidate, and a NaN beats nobody).
 6. Output: the keypoints' original indices, ascending, int64.

Device route (`csrc/keypoints.hip`).  ONE `outliers.sorted_batch` for the larger of the two radii
(the radius cell of `outliers.py`: at the default cell no point is pending in either launch, because the completeness
bound is asked per radius), then two radius-only scans on it: `hfl_iss_saliency` -- the search and the nine float64 sums
of `hfl_knn_normals_radius` with another finish (steps 3 and 4; the "sums -> ordered eigenvalues" code is one header for
both files) -- and `hfl_iss_select`, where a thread whose saliency is 0 returns at once and a candidate stops at the first
neighbour that beats it.  Both have the wave-per-point fallback over the whole cloud.  The index lists come from the mask
with `torch.nonzero` on the device; one host read gives their sizes, as in `remove_outliers`.  counts, the set of zeros
and the selection for a given saliency equal the numpy route's for any `cell_size`; the saliency values agree to an fp32
rounding of a float64 difference of about 1e-15 l2 (the sums run in the order of the sort and the grid, fixed for given
inputs, so two runs give the same bits).

Batch limits as in `ragged.py`."""

from typing import Sequence

import numpy as np
import torch

from . import normals, ops, outliers, ragged

GAMMA_21 = GAMMA_32 = 0.975            # open3d's defaults
MIN_NEIGHBOURS = 5
_HOST_CHUNK = 1 << 21                  # point pairs of one temporary of the numpy route


def _check_gamma(name: str, value) -> float:
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or not 0.0 < float(value) <= 1.0:
        raise ValueError('%s must be a number in (0, 1], got %r' % (name, value))
    return float(value)


def _check_min_neighbours(min_neighbors) -> int:
    if isinstance(min_neighbors, bool) or not isinstance(min_neighbors, (int, np.integer)) or \
            not 1 <= int(min_neighbors) < 2 ** 31:
        raise ValueError('min_neighbors must be an integer >= 1, got %r' % (min_neighbors,))
    return int(min_neighbors)


def check_params(gamma_21=GAMMA_21, gamma_32=GAMMA_32, min_neighbors=MIN_NEIGHBOURS):
    """the keyword parameters of the detector, checked -> (gamma_21, gamma_32, min_neighbors)"""
    return _check_gamma('gamma_21', gamma_21), _check_gamma('gamma_32', gamma_32), _check_min_neighbours(min_neighbors)


def check_radii(salient_radius, non_max_radius, what: str = 'iss_keypoints'):
    """The (salient_radius, non_max_radius) pair of `global_registration` and `rerank_candidates` -> None when both are
    None, else the two checked radii; only one of them is a `ValueError`."""
    if salient_radius is None and non_max_radius is None:
        return None
    if salient_radius is None or non_max_radius is None:
        raise ValueError('%s: salient_radius and non_max_radius come together: both, or neither' % what)
    return outliers.check_radius(salient_radius, 'salient_radius'), outliers.check_radius(non_max_radius, 'non_max_radius')


# ------------------------------------------------------------------------------------------------ host route (numpy)
def _saliency_host(a: np.ndarray, r2s, g21: float, g32: float, min_nb: int):
    """steps 1 to 4 for one (n, 3) fp32 cloud -> (saliency (n,) float32, counts (n,) int32): the neighbourhood, the sums
    and the eigenvalues are `normals._normals_host`'s"""
    _, _, counts, lam = normals._normals_host(a, None, None, r2s)
    with np.errstate(invalid='ignore', over='ignore'):
        salient = (counts >= min_nb) & (lam[:, 1] < g21 * lam[:, 2]) & (lam[:, 0] < g32 * lam[:, 1])
        return np.where(salient, lam[:, 0], 0.0).astype(np.float32), counts


def _select_host(a: np.ndarray, s: np.ndarray, r2n, min_nb: int) -> np.ndarray:
    """step 5 for one (n, 3) fp32 cloud and its (n,) float32 saliency by brute force in row chunks -> (n,) bool"""
    n = a.shape[0]
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    index = np.arange(n)
    keep = np.zeros(n, bool)
    chunk = max(1, _HOST_CHUNK // n)
    with np.errstate(over='ignore', invalid='ignore'):
        for b in range(0, n, chunk):
            e = min(n, b + chunk)
            dx, dy, dz = x[b:e, None] - x[None, :], y[b:e, None] - y[None, :], z[b:e, None] - z[None, :]
            near = ((dx * dx + dy * dy) + dz * dz) <= r2n            # fp32 arrays: every operation rounded once
            own = s[b:e, None]
            beats = (s[None, :] > own) | ((s[None, :] == own) & (index[None, :] < index[b:e, None]))
            keep[b:e] = (s[b:e] > 0) & (near.sum(1) >= min_nb) & ~(near & beats).any(1)
    return keep


def _saliency_arrays(saliency, sizes, xp):
    """the caller's saliency as one (n_i,) float32 array per cloud (`xp` numpy or torch), checked"""
    if not isinstance(saliency, (list, tuple)) or len(saliency) != len(sizes):
        raise ValueError('saliency: one (n_i,) float32 array per cloud expected (%d clouds)' % len(sizes))
    out = [torch.as_tensor(s) if xp is torch else np.asarray(s.detach().cpu().numpy() if isinstance(s, torch.Tensor) else s)
           for s in saliency]
    for i, (s, n) in enumerate(zip(out, sizes)):
        if s.dtype not in (torch.float32, np.dtype(np.float32)):
            raise TypeError('saliency %d: float32 expected, got %s' % (i, s.dtype))
        if tuple(s.shape) != (n,):
            raise ValueError('saliency %d: shape (%d,) expected, got %s' % (i, n, tuple(s.shape)))
    return out


def iss_saliency_host(clouds: Sequence, salient_radius: float, *, gamma_21=GAMMA_21, gamma_32=GAMMA_32,
                      min_neighbors=MIN_NEIGHBOURS, return_counts: bool = False):
    """Steps 1 to 4 of the module docstring in numpy, fp32 for the distances and float64 for the rest: the route without a
    GPU and the yardstick of the tests.  Brute force, O(n^2): meant for tests and small clouds.  List of (n_i, 3) clouds ->
    list of (n_i,) float32 saliencies, 0 where a point is not salient; with `return_counts` also the (n_i,) int32 sizes of
    the salient neighbourhoods, `radius_neighbour_counts_host(clouds, salient_radius)`."""
    r2s = outliers.radius2(outliers.check_radius(salient_radius, 'salient_radius'))
    params = check_params(gamma_21, gamma_32, min_neighbors)
    parts = [_saliency_host(a, r2s, *params) for a in outliers._checked_arrays(clouds)]
    return ragged.results([p[0] for p in parts], [p[1] for p in parts] if return_counts else None)


def iss_select_host(clouds: Sequence, saliency: Sequence, non_max_radius: float, *, min_neighbors=MIN_NEIGHBOURS,
                    return_mask: bool = False):
    """Step 5 of the module docstring in numpy on any float32 saliency, one (n_i,) array per cloud -> list of (k_i,) int64
    keypoint indices, ascending (k_i may be 0); with `return_mask` the (n_i,) bool masks instead."""
    r2n = outliers.radius2(outliers.check_radius(non_max_radius, 'non_max_radius'))
    min_nb = _check_min_neighbours(min_neighbors)
    arrays = outliers._checked_arrays(clouds)
    sal = _saliency_arrays(saliency, [a.shape[0] for a in arrays], np)
    masks = [_select_host(a, s, r2n, min_nb) for a, s in zip(arrays, sal)]
    return masks if return_mask else [np.nonzero(m)[0].astype(np.int64) for m in masks]


def iss_keypoints_host(clouds: Sequence, salient_radius: float, non_max_radius: float, *, gamma_21=GAMMA_21,
                       gamma_32=GAMMA_32, min_neighbors=MIN_NEIGHBOURS, return_saliency: bool = False):
    """The definition of the module docstring in numpy: `iss_saliency_host`, then `iss_select_host` on it -> list of (k_i,)
    int64 keypoint indices, ascending (k_i may be 0); with `return_saliency` also the (n_i,) float32 saliencies."""
    sal = iss_saliency_host(clouds, salient_radius, gamma_21=gamma_21, gamma_32=gamma_32, min_neighbors=min_neighbors)
    keys = iss_select_host(clouds, sal, non_max_radius, min_neighbors=min_neighbors)
    return ragged.results(keys, sal if return_saliency else None)


# ------------------------------------------------------------------------------------------------ device route
def _index_lists(packed, mask):
    """the (P,) uint8 mask of a packed batch -> the per-cloud lists of local row indices, int64 on the device: one
    `nonzero`, and one host read for the sizes"""
    index = torch.nonzero(mask).reshape(-1)                           # ascending: the order of the input
    off = ragged.compact_offsets(index.cpu().numpy(), packed.off_host)
    return [index[off[b]:off[b + 1]] - int(packed.off_host[b]) for b in range(packed.batch)]


def _cell(cell_size):
    return None if cell_size is None else ragged.check_positive('cell_size', cell_size)


def iss_saliency(clouds: Sequence, salient_radius: float, *, gamma_21=GAMMA_21, gamma_32=GAMMA_32,
                 min_neighbors=MIN_NEIGHBOURS, device='cuda', cell_size=None, return_counts: bool = False,
                 return_pending: bool = False):
    """`iss_saliency_host` on the device: list of raw (n_i, 3) clouds (numpy / torch, host or device) -> list of (n_i,)
    float32 device tensors.  The counts (`return_counts`, (n_i,) int32) and the set of zeros equal the numpy route's for
    any `cell_size` (the edge of the search grid's cells); the values agree to rounding.  `return_pending`: the number of
    points of the batch that the whole-cloud scan finished, 0 at the default cell (a debug counter).  `ValueError` as in
    `estimate_normals`."""
    r = outliers.check_radius(salient_radius, 'salient_radius')
    params, cell = check_params(gamma_21, gamma_32, min_neighbors), _cell(cell_size)
    with ragged.intake(clouds, device) as packed:
        if packed is None:
            return ragged.results([], [] if return_counts else None, 0 if return_pending else None)
        table, sorted_pts, sorted_keys, perm = outliers.sorted_batch(packed, None, cell, radius=r)
        sal, counts, _, pending = ops.iss_saliency(sorted_pts, sorted_keys, perm, packed.off, table, outliers.radius2(r), *params)
        return ragged.results(packed.split(sal), packed.split(counts) if return_counts else None,
                              int(pending.item()) if return_pending else None)


def iss_select(clouds: Sequence, saliency: Sequence, non_max_radius: float, *, min_neighbors=MIN_NEIGHBOURS, device='cuda',
               cell_size=None, return_mask: bool = False, return_pending: bool = False):
    """`iss_select_host` on the device, bit for bit for any `cell_size`: step 5 on any float32 saliency (one (n_i,) array
    or tensor per cloud, host or device) -> list of (k_i,) int64 device tensors, the keypoint indices in ascending order,
    or with `return_mask` the (n_i,) bool masks.  `return_pending`: also the number of candidates that the whole-cloud
    scan finished."""
    r = outliers.check_radius(non_max_radius, 'non_max_radius')
    min_nb, cell = _check_min_neighbours(min_neighbors), _cell(cell_size)
    sal = []
    with ragged.intake(clouds, device, check=lambda sizes: sal.extend(_saliency_arrays(saliency, sizes, torch))) as packed:
        if packed is None:
            return ragged.results([], 0 if return_pending else None)
        table, sorted_pts, sorted_keys, perm = outliers.sorted_batch(packed, None, cell, radius=r)
        flat = torch.cat([s.to(packed.pts.device) for s in sal])
        mask, pending = ops.iss_select(sorted_pts, sorted_keys, perm, flat[perm].contiguous(), packed.off, table,
                                       outliers.radius2(r), min_nb)
        return ragged.results(packed.split(mask.bool()) if return_mask else _index_lists(packed, mask),
                              int(pending.item()) if return_pending else None)


def iss_keypoints_packed(packed, salient_radius: float, non_max_radius: float, params=(GAMMA_21, GAMMA_32, MIN_NEIGHBOURS),
                         cell=None):
    """both steps on a packed batch and ONE sorted batch, parameters checked -> (mask (P,) uint8, saliency (P,) fp32,
    pending (2,) int32: of the saliency and of the selection launch), everything on the device"""
    table, sorted_pts, sorted_keys, perm = outliers.sorted_batch(packed, None, cell, radius=max(salient_radius, non_max_radius))
    ws = ops.KnnWorkspace(int(sorted_pts.shape[0]), table.cells, sorted_pts.device)
    sal, _, sorted_sal, counter = ops.iss_saliency(sorted_pts, sorted_keys, perm, packed.off, table,
                                                   outliers.radius2(salient_radius), *params, workspace=ws)
    first = counter.clone()                                           # the selection counts on the same workspace
    mask, counter = ops.iss_select(sorted_pts, sorted_keys, perm, sorted_sal, packed.off, table,
                                   outliers.radius2(non_max_radius), params[2],
                                   phases=ops.KNN_PHASE_QUERY | ops.KNN_PHASE_FALLBACK, workspace=ws)
    return mask, sal, torch.cat([first, counter])


def iss_keypoints(clouds: Sequence, salient_radius: float, non_max_radius: float, *, gamma_21=GAMMA_21, gamma_32=GAMMA_32,
                  min_neighbors=MIN_NEIGHBOURS, device='cuda', cell_size=None, return_saliency: bool = False,
                  return_pending: bool = False):
    """`iss_keypoints_host` on the device: list of raw (n_i, 3) clouds (numpy / torch, host or device) -> list of (k_i,)
    int64 device tensors, the original indices of the keypoints of the module docstring in ascending order (k_i may be 0):
    exactly `iss_select_host` of the saliency this call computes (`return_saliency`: the (n_i,) float32 tensors), and the
    numpy route's keypoints wherever no two ball neighbours have saliencies that float64 rounding alone tells apart.  One
    sorted batch for the larger radius, two launches.  `return_pending`: the points that the whole-cloud scans of the two
    launches finished, added; 0 at the default cell.  `ValueError` as in `estimate_normals`."""
    rs = outliers.check_radius(salient_radius, 'salient_radius')
    rn = outliers.check_radius(non_max_radius, 'non_max_radius')
    params, cell = check_params(gamma_21, gamma_32, min_neighbors), _cell(cell_size)
    with ragged.intake(clouds, device) as packed:
        if packed is None:
            return ragged.results([], [] if return_saliency else None, 0 if return_pending else None)
        mask, sal, pending = iss_keypoints_packed(packed, rs, rn, params, cell)
        return ragged.results(_index_lists(packed, mask), packed.split(sal) if return_saliency else None,
                              int(pending.sum().item()) if return_pending else None)
