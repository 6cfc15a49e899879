"""Statistical outlier removal and the radius trim for raw submaps, for a whole ragged batch on the device.

The reference cleans CS-Wild-Places submaps offline, on the host, one at a time, through open3d
(`datasets/CSWildPlaces/processing_utils.py:153-169` `remove_outliers`: `remove_statistical_outlier(nb_neighbors=20,
std_ratio=3.0)`), and cuts a Wild-Places ground scan to the submap footprint before anything else
(`postprocess_wildplaces_ground.py:146`: `pts[np.linalg.norm(pts[:, :2], axis=1) <= radius_max]`, 30 m).  Both sit in front
of the chain of `ground.py` and `voxel.py`: trim, outliers, ground, downsample, normalise.  Here a batch of raw submaps goes
to the GPU once; open3d is not needed.

open3d's KD-tree works in float64 on float64 points, and it is not a dependency, so this module DEFINES the filter, as
`ground.py` does for the cloth filter, following `PointCloud::RemoveStatisticalOutliers` step by step.  **Bit parity with
open3d is not claimed.**  The numpy route below (`*_host`) and the device route follow the definition operation for
operation and agree to the bit.

Definition, for one cloud of n fp32 points with k = min(`nb_neighbors`, n):

 1. Squared distances: for every point i, to all n points of the cloud, itself included (open3d's `SearchKNN` on its own
    tree includes it), in fp32 on the differences themselves, every operation rounded once, nothing fused:
    d2 = (dx dx + dy dy) + dz dz.
 2. Mean neighbour distance: the k smallest d2 of the point (only the multiset matters: ties at the k-th place change
    nothing), the correctly rounded fp32 root of each, added in ascending order in fp32 from 0, divided by float32(k):
    avg[i].
 3. A point is valid when avg[i] > 0.  A point with k coincident copies, itself among them, has avg = 0 and is never kept,
    as in open3d.
 4. Threshold, over the valid points in float64: mean = sum(avg) / n_valid, std = sqrt(sum((avg - mean)^2) / (n_valid - 1)),
    threshold = mean + `std_ratio` std.  No valid point keeps nothing; a single valid point gives std = 0 / 0 = NaN, so the
    threshold is NaN and nothing is kept either -- that is open3d's behaviour too.
 5. Keep i when it is valid and float64(avg[i]) < threshold.  The kept rows come back in input order, bit for bit.

`nb_neighbors` is an integer in 1..32, `std_ratio` finite and > 0; a cloud with a coordinate that is not finite raises
`ValueError` naming it.  The float64 sums of step 4 are taken in another order on the device (that of `hfl_pair_stats`,
fixed, so two runs give the same bits) than numpy's pairwise sum: mean, std and threshold agree to about 1e-15 relative,
the masks are equal unless a point's avg lies that close to the threshold.

Radius trim: keep a row when sqrt(x x + y y) <= `radius_max`, in float64 from the fp32 coordinates, every operation rounded
once -- exactly what `np.linalg.norm(pts[:, :2].astype(float64), axis=1) <= radius_max` computes, which the host route
calls.  Rows stay in input order; a cloud may come back empty.

Device route of steps 1 and 2 (`csrc/outliers.hip`).  The answer is a pure function of the input, so
the search structure is free: `hfl_voxel_bounds` and `hfl_cloud_nonfinite` with one host read, from which the host lays a
uniform grid of cubic cells over every cloud (`POINTS_PER_CELL` points per cell on average, the cell enlarged until the
cell-start tables of the batch fit `CELL_BUDGET_BYTES`; `cell_size=` overrides the choice); `hfl_knn_cell_keys`,
`torch.sort` (plumbing, as in `voxel.py`) and a gather put the points cell by cell; `hfl_knn_mean_dist` builds the dense
cell-start table, lets one thread per point scan the 3 x 3 x 3 cells round its own with the k smallest d2 in a sorted
register list, and proves the scan complete when the k-th smallest d2 lies strictly below the square of a conservative
distance to the nearest face of the block that has cells behind it.  The points it cannot prove -- the isolated ones the
filter exists to find, among others -- are finished by a whole-cloud scan, a wave per point.  With a cell so large that a
cloud is one cell the first scan is the brute force.  Then `hfl_outlier_threshold`, `hfl_outlier_mask`, and the compaction
of `ragged.compact`: `torch.nonzero`, `hfl_voxel_gather_rows`, one `searchsorted` on the host offsets.

Radius outlier removal, after open3d's `remove_radius_outlier`.  `radius` is a float, positive and
finite in fp32; R2 = `global_registration.inlier_d2(radius)` is the largest fp32 d2 whose correctly rounded fp32 root is <=
float32(radius), so "within the radius" means what "within `max_correspondence_distance`" means to ICP and RANSAC.
counts[i] = |{ j : d2(i, j) <= R2 }| with the d2 of step 1, the point itself included (int32, so always >= 1);
`remove_radius_outliers` keeps row i when counts[i] > `nb_points` (an integer >= 0), rows in input order.  Only integers
are written, so the device and the numpy route agree to the bit.  Device route: `sorted_batch` with the radius,
`hfl_knn_radius_count` (one pass over the 3 x 3 x 3 block, no list; the whole-cloud scan for a point whose block is not
proven to hold the ball), `hfl_count_mask`, `ragged.compact`.  A radius-only search visits every point of 27 cells of
edge >= radius per query: **a very large radius on a large cloud is quadratic work per thread**.

The search grid with a radius (`grid_layout(radius=...)`).  `knn_block_bound` proves a point resolved when r2 lies below
((gap - margin) (1 - 2^-20))^2, gap the fp32 distance to the nearest face of the block with cells behind it.  A point of
cell ix has a >= ix cell (1 - 2^-24) along an axis (the rounded division that assigned it) and the face lies at
fl((ix - 1) cell), so gap >= cell (1 - nx 2^-23); the margin is 2^-20 nx cell; three roundings and the shrink take less
than 2^-19 more.  With nmax the largest of nx, ny, nz the root of the bound is therefore above cell (1 - `RADIUS_LOSS`),
`RADIUS_LOSS` = 2^-20 (1.25 nmax + 4), and R2 <= radius^2 (1 + 2^-23): the **radius cell** radius / (1 - RADIUS_LOSS)
(doubled first while the loss is not below 1 / 2) leaves NO point pending, and a larger cell (the budget doubling) keeps
that, because nmax only falls.  Radius-only calls take the radius cell by default, hybrid calls the smaller of it and the
density cell; `cell_size=` still overrides, and still changes no count.

Batch limits as in `ragged.py`."""

import math
from typing import List, Sequence

import numpy as np
import torch

from . import ops, ragged

MAX_NEIGHBOURS = ops.KNN_MAX_NEIGHBOURS
POINTS_PER_CELL = 2.0                  # the average the default cell size aims at, empty cells counted
CELL_BUDGET_BYTES = 64 << 20           # the int32 cell-start tables of one batch
FACE_MARGIN = 2.0 ** -20               # of the grid's extent along an axis: the absolute margin of the completeness bound
_F = np.float32


def _check_neighbours(nb_neighbors) -> int:
    if isinstance(nb_neighbors, bool) or not isinstance(nb_neighbors, (int, np.integer)) or \
            not 1 <= int(nb_neighbors) <= MAX_NEIGHBOURS:
        raise ValueError('nb_neighbors must be an integer in 1..%d, got %r' % (MAX_NEIGHBOURS, nb_neighbors))
    return int(nb_neighbors)


def check_radius(radius, name: str = 'radius') -> float:
    """float(radius), positive and finite, also once rounded to float32"""
    if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)):
        raise ValueError('%s must be a positive, finite number, got %r' % (name, radius))
    return ragged.check_positive(name, radius, fp32=True)


def radius2(radius: float) -> np.float32:
    """R2 of the module docstring for a checked radius"""
    from .global_registration import inlier_d2       # that module imports nothing of this one
    return inlier_d2(radius)


def check_neighbourhood(nb_neighbors, radius, check_nb):
    """The (nb_neighbors, radius) pair of `estimate_normals` and `compute_fpfh` -> (nb or None, radius or None): k nearest
    (nb, None), hybrid (nb, radius), radius-only (None, radius); `check_nb` checks an integer nb_neighbors."""
    if nb_neighbors is None and radius is None:
        raise ValueError('nb_neighbors=None is the radius-only neighbourhood and needs a radius')
    return (None if nb_neighbors is None else check_nb(nb_neighbors)), (None if radius is None else check_radius(radius))


def _nonfinite_error(i: int):
    return ValueError('cloud %d holds a coordinate that is not finite' % i)


# ------------------------------------------------------------------------------------------------ host route (numpy)
def _knn_mean_host(a: np.ndarray, nb: int) -> np.ndarray:
    """steps 1 and 2 for one (n, 3) fp32 cloud by brute force in row chunks -> (n,) fp32"""
    n = a.shape[0]
    k = min(nb, n)
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    out = np.empty(n, dtype=np.float32)
    chunk = max(1, (1 << 23) // n)
    with np.errstate(over='ignore', invalid='ignore'):
        for s in range(0, n, chunk):
            e = min(n, s + chunk)
            dx, dy, dz = x[s:e, None] - x[None, :], y[s:e, None] - y[None, :], z[s:e, None] - z[None, :]
            d2 = (dx * dx + dy * dy) + dz * dz                   # fp32 arrays: every operation rounded once
            near = np.partition(d2, k - 1, axis=1)[:, :k]
            near.sort(axis=1)
            root = np.sqrt(near)
            acc = np.zeros(e - s, dtype=np.float32)
            for i in range(k):                                   # ascending, one rounded add at a time (np.sum adds pairwise)
                acc = acc + root[:, i]
            out[s:e] = acc / _F(k)
    return out


def _threshold_host(avg: np.ndarray, std_ratio: float):
    """steps 3 and 4 -> (mean, std, threshold, n_valid), float64"""
    v = avg[avg > 0].astype(np.float64)
    nv = int(v.shape[0])
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = np.float64(v.sum()) / np.float64(nv)
        std = np.sqrt(np.float64(((v - mean) ** 2).sum()) / np.float64(nv - 1))
    return float(mean), float(std), float(mean + std_ratio * std), nv


def _checked_arrays(clouds):
    arrays = ragged.as_arrays(clouds)
    for i, a in enumerate(arrays):
        if not np.isfinite(a).all():
            raise _nonfinite_error(i)
    return arrays


def knn_mean_distance_host(clouds: Sequence, nb_neighbors: int = 20) -> List[np.ndarray]:
    """Steps 1 and 2 of the module docstring in numpy fp32: per cloud the (n_i,) float32 mean distance to the
    k = min(nb_neighbors, n_i) nearest points of the cloud, the point itself included.  Plain brute force, O(n^2): meant for
    tests and small clouds."""
    nb = _check_neighbours(nb_neighbors)
    return [_knn_mean_host(a, nb) for a in _checked_arrays(clouds)]


def remove_outliers_host(clouds: Sequence, nb_neighbors: int = 20, std_ratio: float = 3.0, *, return_mask: bool = False,
                         return_distances: bool = False, return_stats: bool = False):
    """The definition of the module docstring in numpy, fp32 for steps 1-2 and float64 for step 4: the route without a GPU
    and the yardstick of the tests.  Brute force, O(n^2): meant for tests and small clouds.  List of (n_i, 3) clouds ->
    list of (k_i, 3) float32 arrays, the kept rows in input order (k_i may be 0); with `return_mask` also the (n_i,) bool
    masks, with `return_distances` the (n_i,) float32 avg, with `return_stats` per-cloud dicts 'mean', 'std', 'threshold'
    (floats; NaN as step 4 says) and 'n_valid' (int).  A single valid point keeps nothing, as in open3d."""
    nb = _check_neighbours(nb_neighbors)
    ratio = ragged.check_positive('std_ratio', std_ratio)
    arrays = _checked_arrays(clouds)
    avgs = [_knn_mean_host(a, nb) for a in arrays]
    stats = [_threshold_host(avg, ratio) for avg in avgs]
    with np.errstate(invalid='ignore'):
        masks = [(avg > 0) & (avg.astype(np.float64) < s[2]) for avg, s in zip(avgs, stats)]
    return ragged.results([a[m] for a, m in zip(arrays, masks)], masks if return_mask else None,
                          avgs if return_distances else None,
                          [dict(mean=s[0], std=s[1], threshold=s[2], n_valid=s[3]) for s in stats] if return_stats else None)


def _radius_counts_host(a: np.ndarray, r2) -> np.ndarray:
    """counts of the module docstring for one (n, 3) fp32 cloud by brute force in row chunks -> (n,) int32"""
    n = a.shape[0]
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    out = np.empty(n, dtype=np.int32)
    chunk = max(1, (1 << 23) // n)
    with np.errstate(over='ignore', invalid='ignore'):
        for s in range(0, n, chunk):
            e = min(n, s + chunk)
            dx, dy, dz = x[s:e, None] - x[None, :], y[s:e, None] - y[None, :], z[s:e, None] - z[None, :]
            out[s:e] = (((dx * dx + dy * dy) + dz * dz) <= r2).sum(1)
    return out


def _check_nb_points(nb_points) -> int:
    if isinstance(nb_points, bool) or not isinstance(nb_points, (int, np.integer)) or not 0 <= int(nb_points) < 2 ** 31:
        raise ValueError('nb_points must be an integer >= 0, got %r' % (nb_points,))
    return int(nb_points)


def radius_neighbour_counts_host(clouds: Sequence, radius: float) -> List[np.ndarray]:
    """The radius counts of the module docstring in numpy fp32: per cloud the (n_i,) int32 number of points of the cloud
    within `radius` of each point, the point itself included.  Brute force, O(n^2): meant for tests and small clouds."""
    r2 = radius2(check_radius(radius))
    return [_radius_counts_host(a, r2) for a in _checked_arrays(clouds)]


def remove_radius_outliers_host(clouds: Sequence, nb_points: int, radius: float, *, return_mask: bool = False):
    """Radius outlier removal in numpy: list of (n_i, 3) clouds -> list of (k_i, 3) float32 arrays, the rows with more than
    `nb_points` points of the cloud within `radius` (themselves included) in input order (k_i may be 0); with `return_mask`
    also the (n_i,) bool masks."""
    nb, r2 = _check_nb_points(nb_points), radius2(check_radius(radius))
    arrays = _checked_arrays(clouds)
    masks = [_radius_counts_host(a, r2) > nb for a in arrays]
    return ragged.results([a[m] for a, m in zip(arrays, masks)], masks if return_mask else None)


def trim_radius_host(clouds: Sequence, radius_max: float = 30.0, *, return_mask: bool = False):
    """The radius trim in numpy float64 -> list of (k_i, 3) float32 arrays, the rows with sqrt(x x + y y) <= radius_max in
    input order (k_i may be 0); with `return_mask` also the (n_i,) bool masks."""
    r = ragged.check_positive('radius_max', radius_max)
    arrays = ragged.as_arrays(clouds)
    with np.errstate(over='ignore', invalid='ignore'):
        masks = [np.linalg.norm(a[:, :2].astype(np.float64), axis=1) <= r for a in arrays]
    return ragged.results([a[m] for a, m in zip(arrays, masks)], masks if return_mask else None)


# ------------------------------------------------------------------------------------------------ device route
def _grid_dims(extent: np.ndarray, cell: float):
    return np.floor(extent / cell).astype(np.int64) + 1


def radius_loss(extent: np.ndarray, cell: float) -> float:
    """`RADIUS_LOSS` of the module docstring: the share of `cell` by which the root of `knn_block_bound` may lie below it"""
    return 2.0 ** -20 * (1.25 * float(_grid_dims(extent, cell).max()) + 4.0)


def radius_cell(extent: np.ndarray, radius: float) -> float:
    """the radius cell of the module docstring, as a float that fp32 holds: no point of a grid of this cell, or of a larger
    one, is pending in a search within `radius`"""
    cell = float(radius)
    while not radius_loss(extent, cell) < 0.5:
        cell *= 2.0
    cell = max(cell, float(radius) / (1.0 - radius_loss(extent, cell)))
    as32 = _F(min(cell, 1e30))
    return float(as32 if float(as32) >= cell else np.nextafter(as32, _F(np.inf)))


def grid_layout(lo_hi: np.ndarray, sizes, nb, cell_size=None, budget_bytes: int = CELL_BUDGET_BYTES, radius=None) -> np.ndarray:
    """The search grids of a batch from the fp32 bounds (B, 6) and the cloud sizes -> `ops.KNN_GRID_DTYPE` rows.  The
    default cell is the smallest at which a cloud has at most n / `POINTS_PER_CELL` cells; with a `radius`, the smaller of
    that and `radius_cell`, and for a radius-only search (`nb` None, the rows' k then unread) the radius cell.  Any cell,
    the caller's included, is doubled until the cloud's cells fit its share of `budget_bytes`.  The grid only decides the
    speed."""
    if nb is None and radius is None:
        raise ValueError('grid_layout: a number of neighbours, a radius, or both')
    batch = len(sizes)
    share = max(int(budget_bytes) // 4 // batch - 1, 1)
    grids = np.zeros(batch, dtype=np.dtype(ops.KNN_GRID_DTYPE))
    base = 0
    for b, n in enumerate(sizes):
        low = lo_hi[b, :3].astype(np.float64)
        extent = lo_hi[b, 3:].astype(np.float64) - low
        widest = float(extent.max())
        if cell_size is not None:
            cell = float(cell_size)
        elif not widest > 0.0:
            cell = 1.0
        elif nb is None:
            cell = radius_cell(extent, radius)
        else:
            want = max(min(n / POINTS_PER_CELL, share), 1.0)
            small, large = widest * 2.0 ** -24, widest * 2.0             # bisect the monotone cell count in log space
            for _ in range(48):
                mid = math.sqrt(small * large)
                if float(np.prod(_grid_dims(extent, mid).astype(np.float64))) <= want:
                    large = mid
                else:
                    small = mid
            cell = large if radius is None else min(large, radius_cell(extent, radius))
        cell = float(_F(min(max(cell, 1e-30), 1e30)))
        while float(np.prod(_grid_dims(extent, cell).astype(np.float64))) > share:
            cell = float(_F(cell * 2.0))
        nx, ny, nz = (int(d) for d in _grid_dims(extent, cell))
        margin = [float(_F(FACE_MARGIN * d * cell)) for d in (nx, ny, nz)]
        grids[b] = (lo_hi[b, 0], lo_hi[b, 1], lo_hi[b, 2], cell, margin[0], margin[1], margin[2],
                    min(MAX_NEIGHBOURS if nb is None else nb, n), nx, ny, nz, 0, base)
        base += nx * ny * nz
    return grids


def check_params(nb_neighbors: int = 20, std_ratio: float = 3.0, cell_size=None):
    """the keyword parameters of `remove_outliers`, checked -> (nb, ratio, cell)"""
    return (_check_neighbours(nb_neighbors), ragged.check_positive('std_ratio', std_ratio),
            None if cell_size is None else ragged.check_positive('cell_size', cell_size))


def sorted_batch(packed, nb, cell_size=None, radius=None):
    """bounds and the finite check (the one host read before the search), the grids (`grid_layout` with `nb`, `cell_size`
    and `radius`), keys, sort, gather -> (table, the points cell by cell, their ascending keys, the sort's permutation)"""
    pts, off, batch = packed.pts, packed.off, packed.batch
    bounds, flags = ops.voxel_bounds(pts, off), ops.cloud_nonfinite(pts, off)
    host = torch.cat([bounds.reshape(-1), flags]).cpu().numpy()
    lo_hi = ops.decode_voxel_bounds(host[:6 * batch])
    for i in range(batch):
        if host[6 * batch + i] or not np.isfinite(lo_hi[i]).all():
            raise _nonfinite_error(i)
    table = ops.KnnGridTable(grid_layout(lo_hi, packed.sizes(), nb, cell_size, radius=radius), pts.device)
    keys = ops.knn_cell_keys(pts, off, table)
    sorted_keys, perm = torch.sort(keys)
    return table, ops.voxel_gather_rows(pts, perm), sorted_keys, perm


def _knn_packed(packed, nb: int, cell_size):
    table, sorted_pts, sorted_keys, perm = sorted_batch(packed, nb, cell_size)
    return ops.knn_mean_dist(sorted_pts, sorted_keys, perm, packed.off, table)


def knn_mean_distance(clouds: Sequence, nb_neighbors: int = 20, *, device='cuda', cell_size=None,
                      return_pending: bool = False):
    """`knn_mean_distance_host` on the device: list of (n_i,) float32 device tensors, bit for bit what the numpy route
    returns, for any `cell_size` (the edge of the search grid's cells; the default is chosen per cloud).  With
    `return_pending` also the number of points of the batch that the 3 x 3 x 3 scan could not prove complete and the
    whole-cloud scan finished (a debug counter)."""
    nb, _, cell = check_params(nb_neighbors, cell_size=cell_size)
    with ragged.intake(clouds, device) as packed:
        if packed is None:
            return ([], 0) if return_pending else []
        avg, pending = _knn_packed(packed, nb, cell)
        return (packed.split(avg), int(pending.item())) if return_pending else packed.split(avg)


def remove_outliers_packed(packed, nb: int, ratio: float, cell=None):
    """the filter on a packed batch, parameters as `check_params` returns them -> (the kept rows as a `ragged.Packed`,
    keep (P,) uint8, avg (P,) fp32, stats (B, 4) float64), everything on the device"""
    avg, _ = _knn_packed(packed, nb, cell)
    stats = ops.outlier_threshold(avg, packed.off, ratio)
    keep = ops.outlier_mask(avg, packed.off, stats)
    return ragged.compact(packed, keep), keep, avg, stats


def remove_outliers(clouds: Sequence, nb_neighbors: int = 20, std_ratio: float = 3.0, *, device='cuda',
                    return_mask: bool = False, return_distances: bool = False, return_stats: bool = False, cell_size=None):
    """List of raw (n_i, 3) clouds (numpy / torch, host or device) -> list of (k_i, 3) float32 device tensors: the rows the
    statistical outlier filter of the module docstring keeps, in input order, bit for bit the rows `remove_outliers_host`
    returns (k_i may be 0).  `return_mask`: also the (n_i,) bool masks; `return_distances`: the (n_i,) float32 avg;
    `return_stats`: per-cloud dicts 'mean', 'std', 'threshold' (floats) and 'n_valid' (int).  A cloud with a single valid
    point keeps nothing (std = 0 / 0 = NaN), as in open3d.  `cell_size` sets the edge of the search grid's cells and
    changes no bit of any output.  `ValueError` for a bad parameter or an empty cloud (before the device is touched) and,
    naming the cloud, for a coordinate that is not finite (before any kernel of the filter runs)."""
    params = check_params(nb_neighbors, std_ratio, cell_size)
    with ragged.intake(clouds, device) as packed:
        if packed is None:
            return ragged.empty_results(return_mask, return_distances, return_stats)
        kept, keep, avg, stats = remove_outliers_packed(packed, *params)
        return ragged.results(kept.split(), packed.split(keep.bool()) if return_mask else None,
                              packed.split(avg) if return_distances else None,
                              [dict(mean=m, std=s, threshold=t, n_valid=int(v)) for m, s, t, v in stats.cpu().tolist()]
                              if return_stats else None)


def radius_counts_packed(packed, radius: float, cell=None):
    """the radius counts of a packed batch, `radius` checked -> (counts (P,) int32, pending (1,) int32), on the device"""
    table, sorted_pts, sorted_keys, perm = sorted_batch(packed, None, cell, radius)
    return ops.knn_radius_count(sorted_pts, sorted_keys, perm, packed.off, table, radius2(radius))


def radius_neighbour_counts(clouds: Sequence, radius: float, *, device='cuda', cell_size=None, return_pending: bool = False):
    """`radius_neighbour_counts_host` on the device: list of (n_i,) int32 device tensors, equal to the numpy route's for any
    `cell_size`.  With `return_pending` also the number of points of the batch that the whole-cloud scan finished: 0 at the
    default cell (a debug counter)."""
    r = check_radius(radius)
    cell = None if cell_size is None else ragged.check_positive('cell_size', cell_size)
    with ragged.intake(clouds, device) as packed:
        if packed is None:
            return ([], 0) if return_pending else []
        counts, pending = radius_counts_packed(packed, r, cell)
        return (packed.split(counts), int(pending.item())) if return_pending else packed.split(counts)


def remove_radius_outliers(clouds: Sequence, nb_points: int, radius: float, *, device='cuda', return_mask: bool = False,
                           cell_size=None):
    """`remove_radius_outliers_host` on the device: list of raw (n_i, 3) clouds -> list of (k_i, 3) float32 device tensors,
    the rows with more than `nb_points` points of their cloud within `radius` (themselves included), in input order, bit
    for bit the rows the numpy route returns (k_i may be 0); with `return_mask` also the (n_i,) bool masks.  `cell_size`
    changes no output."""
    nb, r = _check_nb_points(nb_points), check_radius(radius)
    cell = None if cell_size is None else ragged.check_positive('cell_size', cell_size)
    with ragged.intake(clouds, device) as packed:
        if packed is None:
            return ragged.empty_results(return_mask)
        counts, _ = radius_counts_packed(packed, r, cell)
        keep = ops.count_mask(counts, nb)
        return ragged.results(ragged.compact(packed, keep).split(), packed.split(keep.bool()) if return_mask else None)


def trim_radius_packed(packed, radius_max: float):
    """the radius trim on a packed batch -> (the kept rows as a `ragged.Packed`, keep (P,) uint8)"""
    keep = ops.radius_mask(packed.pts, radius_max)
    return ragged.compact(packed, keep), keep


def trim_radius(clouds: Sequence, radius_max: float = 30.0, *, device='cuda', return_mask: bool = False):
    """`trim_radius_host` on the device: list of (k_i, 3) float32 device tensors, the rows with sqrt(x x + y y) <=
    `radius_max` (float64) in input order, equal to the numpy route's; a cloud left empty comes back empty.  With
    `return_mask` also the (n_i,) bool masks."""
    r = ragged.check_positive('radius_max', radius_max)
    with ragged.intake(clouds, device) as packed:
        if packed is None:
            return ragged.empty_results(return_mask)
        kept, keep = trim_radius_packed(packed, r)
        return ragged.results(kept.split(), packed.split(keep.bool()) if return_mask else None)


def clean_batch(clouds: Sequence, device, radius_max=None, remove_outliers: bool = False, outlier_params=None,
                at_least: int = 1) -> List[torch.Tensor]:
    """The raw cleaning alone, as the submap entry points of `voxel.py` run it in front of everything else: `trim_radius`
    (when `radius_max` is given), then `remove_outliers(**outlier_params)`, the batch staying packed on the device between
    the two.  `ValueError` naming the first cloud a step leaves no point, or fewer than `at_least` points."""
    from .voxel import submap_chain                  # a public alias kept for callers: voxel.py holds the chain
    return submap_chain(clouds, device, radius_max=radius_max, remove_outliers=remove_outliers, outlier_params=outlier_params,
                        at_least=at_least)
