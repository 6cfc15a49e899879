"""FPFH descriptors of every point of a ragged batch of clouds, and correspondences matched in descriptor space, on the device.

ICP (`registration.icp_refine`) needs a starting pose.  For a query that has only been retrieved there is none, and the
classical source of one is a local geometric descriptor per point, matched between the two clouds, with a robust estimator
on the pairs (that estimator is not in this module).  open3d offers `compute_fpfh_feature` and
`correspondences_from_features`; it is not a dependency and works through a float64 k-d tree and `acos` / `atan2`, so this
module DEFINES what is computed, as `normals.py` and `outliers.py` do.  **Parity with open3d is not claimed.**  The numpy
routes (`compute_fpfh_host`, `feature_correspondences_host`) are this definition; the device routes are compared with them.

Definition of `compute_fpfh`, for one cloud of n finite fp32 points p with one fp32 normal row each (a zero row, or a row
with a component that is not finite, says "no normal", as `normals.py` marks it), `nb_neighbors` an integer in 3..32 and
k = min(`nb_neighbors`, n):

 1. Neighbourhood: exactly that of `normals.py` steps 1-2.  d2(i, j) in fp32 on the differences, (dx dx + dy dy) + dz dz,
    every operation rounded once; r2_i the k-th smallest d2(i, .), the point itself included; N(i) = { j : d2(i, j) <=
    r2_i }.  Ties at the k-th place are ALL included: N(i) is a pure function of the input, whatever the scan order or grid.
 2. Pair features, for every j in N(i) with j != i (by index), both normals present and p_j != p_i.  float64 from the fp32
    inputs, every operation rounded once, no contraction; sums of three products are (a + b) + c.  The PFH Darboux frame in
    open3d's order:  dp = p_j - p_i, d = sqrt(dp . dp) (d = 0: the pair is skipped);  a1 = (n_i . dp) / d,  a2 = (n_j . dp)
    / d.  If |a1| < |a2| the roles swap: source = j, destination = i, dp := -dp, f3 = -a2; else source = i and f3 = a1
    (open3d compares acos|a1| > acos|a2|: the same order, without the acos).  v = dp x n_src, |v| = sqrt(v . v) (0: the
    pair is skipped), v := v / |v|;  w = n_src x v;  f2 = v . n_dst;  theta is the angle of the direction (x, y) =
    (n_src . n_dst, w . n_dst).
 3. Bins: three groups of 11, in the order theta, f2, f3.  **No transcendental function decides a bin.**  f2 and f3:
    floor((11 (f + 1)) / 2) clamped to 0..10.  theta: the number of edges e_k = -pi + 2 pi k / 11, k = 1..10, with theta >=
    e_k, decided against `THETA_TABLE`, one float64 table of (c_k, s_k) = (cos e_k, sin e_k) that this module owns and
    hands to the kernel, so both routes use the same bits: with y >= 0 (the upper half-plane; -0.0 too) every k <= 5
    counts and k >= 6 counts iff c_k y >= s_k x; with y < 0 no k >= 6 counts and k <= 5 counts iff c_k y >= s_k x -- two
    products, each rounded once, then compared.  x = y = 0 is bin 5.
 4. SPFH: hist[i] = the 33 int32 counts over the pairs of i, pairs[i] = their number (int32; 0 for a point without a
    normal).  Integers: order-independent, so the two routes agree to the bit.
 5. FPFH, in float64: SPFH_i(b) = (100 hist_i(b)) / pairs_i, 0 where pairs_i = 0.  The neighbours' histograms are weighted by
    the inverse squared distance: W_i(b) = sum over j in N(i), j != i, d2(i, j) > 0, pairs_j > 0 of hist_j(b) omega_ij with
    omega_ij = (100 / pairs_j) / float64(d2(i, j)), that is SPFH_j(b) / d2 with one division per neighbour instead of one per
    bin.  Per group g: s_g = the sum of W_i(b) over the 11 bins in ascending b;  FPFH_i(b) = SPFH_i(b) + (100 / s_g if s_g >
    0 else 0) W_i(b), rounded once to fp32.  Every term is non-negative, so another summation order moves the float64
    value by about 1e-14 of itself and the fp32 result by at most one ulp.  A group with pairs sums to 100 before the
    weighted term and to 200 with it.

Radius and hybrid neighbourhoods (`radius=`): step 1 takes the neighbourhood of `normals.py` with
the same keyword -- hybrid (`nb_neighbors` in 3..32 and a radius) r2_i = min(k-th smallest d2(i, .), R2) with R2 =
`global_registration.inlier_d2(radius)`, radius-only (`nb_neighbors=None` and a radius) r2_i = R2 -- and steps 2 to 5 are
unchanged.  A histogram over a ball of fixed size describes the same patch of a surface in two clouds of different
density, which one over the k nearest points does not.  In hybrid mode `nb_neighbors` stays in 3..32 (open3d's usual
`max_nn=100` is not reachable; radius-only is the route to larger neighbourhoods), and a very large radius-only search
on a large cloud is quadratic work per thread.  `radius=None` is the k-nearest definition with the bits it always had.
On the device `hfl_fpfh_radius_capped` fills r2 and the proof (radius-only: no scan at all, and no point pending at the
default cell); `hfl_fpfh_spfh` and `hfl_fpfh_combine` read only those and run unchanged.

Device route (`csrc/fpfh.hip`): `outliers.sorted_batch` unchanged, the normals gathered by its
permutation, then `hfl_fpfh_radius` (r2 and whether the 3 x 3 x 3 completeness bound proves it; the others from a whole-cloud
scan, a wave per point), `hfl_fpfh_spfh` (one thread per point re-scans its cells, a wave per unproven point its cloud; 33
counters per thread in LDS) and `hfl_fpfh_combine` (the same scan, the float64 sums in sorted-position order, fp32 stores
at the input rows).  hist and pairs equal the numpy route's for any `cell_size`; FPFH agrees to one fp32 ulp; two runs give
the same bits.

Definition of `feature_correspondences`, for ragged pairs of (N, D) fp32 feature rows, 1 <= D <= 64: exact brute force.
d2 in fp32 on the differences as one fmaf chain over the columns in ascending order, d2 = d_0 d_0, then fmaf(d_c, d_c, d2)
for c = 1..D-1 (the convention of `hfl_nn_dist`, generalised; no norm trick, which cancels for near-identical histograms).
idx = the target row of the smallest d2, **the lowest index on a tie**, -1 and d2 = +inf for a pair without targets.  With
`mutual` also the mask of the rows i whose target's own nearest source row (the same rule, roles swapped) is i.  Features
must be finite.

Batch limits as in `ragged.py`."""

from typing import Sequence

import numpy as np
import torch

from . import _native, ops, outliers, ragged
from .normals import _check_neighbours
from .overlap import _as_numpy, _host_argmin32, _host_d2_32

BINS, DIM = 11, ops.FPFH_DIM
_EDGES = -np.pi + 2.0 * np.pi * np.arange(1, BINS, dtype=np.float64) / float(BINS)
THETA_TABLE = np.ascontiguousarray(np.stack([np.cos(_EDGES), np.sin(_EDGES)], 1))      # (10, 2): c_k, s_k for k = 1..10
MAX_FEATURE_DIM = ops.FEATURE_MAX_DIM
_HOST_CHUNK = 1 << 21                  # point pairs of one temporary of the numpy routes


# ------------------------------------------------------------------------------------------------ the definition (numpy)
def _has_normal(nrm: np.ndarray) -> np.ndarray:
    return np.isfinite(nrm).all(1) & (nrm != 0).any(1)


def _theta_bins(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """step 3 for float64 directions (x, y) -> the bin 0..10"""
    c, s = THETA_TABLE[:, 0], THETA_TABLE[:, 1]
    counts = (c[None, :] * y[:, None]) >= (s[None, :] * x[:, None])
    half = (BINS - 1) // 2
    low, high = counts[:, :half].sum(1), counts[:, half:].sum(1)
    return np.where((x == 0.0) & (y == 0.0), half, np.where(y < 0.0, low, half + high)).astype(np.int64)


def _linear_bins(f: np.ndarray) -> np.ndarray:
    return np.clip(np.floor((11.0 * (f + 1.0)) / 2.0), 0.0, 10.0).astype(np.int64)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]


def _pair_bins(pi, ni, pj, nj):
    """steps 2 and 3 for m pairs, everything (m, 3) float64 -> (valid (m,) bool, bins (m, 3) int64: theta, f2, f3)"""
    with np.errstate(all='ignore'):
        dp = [pj[:, a] - pi[:, a] for a in range(3)]
        n1, n2 = [ni[:, a] for a in range(3)], [nj[:, a] for a in range(3)]
        d = np.sqrt(_dot(dp, dp))
        valid = d > 0.0
        d = np.where(valid, d, 1.0)
        a1, a2 = _dot(n1, dp) / d, _dot(n2, dp) / d
        swap = np.abs(a1) < np.abs(a2)
        src = [np.where(swap, n2[a], n1[a]) for a in range(3)]
        dst = [np.where(swap, n1[a], n2[a]) for a in range(3)]
        e = [np.where(swap, -dp[a], dp[a]) for a in range(3)]
        f3 = np.where(swap, -a2, a1)
        v = _cross(e, src)
        vn = np.sqrt(_dot(v, v))
        valid = valid & (vn > 0.0)
        vn = np.where(valid, vn, 1.0)
        v = [v[a] / vn for a in range(3)]
        w = _cross(src, v)
        f2, x, y = _dot(v, dst), _dot(src, dst), _dot(w, dst)
        return valid, np.stack([_theta_bins(x, y), _linear_bins(f2), _linear_bins(f3)], 1)


def _d2_rows(a: np.ndarray, s: int, e: int) -> np.ndarray:
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    dx, dy, dz = x[s:e, None] - x[None, :], y[s:e, None] - y[None, :], z[s:e, None] - z[None, :]
    return (dx * dx + dy * dy) + dz * dz                         # fp32 arrays: every operation rounded once


def _fpfh_host(a: np.ndarray, nrm: np.ndarray, nb, cap=None):
    """the definition for one (n, 3) fp32 cloud by brute force in row chunks -> (fpfh (n, 33) float32, hist (n, 33) int32,
    pairs (n,) int32).  `cap`: None or R2 (fp32); `nb` None: radius-only"""
    n = a.shape[0]
    k = n if nb is None else min(nb, n)
    a64, n64, has = a.astype(np.float64), nrm.astype(np.float64), _has_normal(nrm)
    hist, pairs = np.zeros((n, DIM), np.int32), np.zeros(n, np.int32)
    r2 = np.empty(n, np.float32)
    chunk = max(1, _HOST_CHUNK // n)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        for s in range(0, n, chunk):
            e = min(n, s + chunk)
            d2 = _d2_rows(a, s, e)
            if nb is None:
                r2[s:e] = cap
            else:
                r2[s:e] = np.partition(d2, k - 1, axis=1)[:, k - 1]
                if cap is not None:
                    r2[s:e] = np.minimum(r2[s:e], cap)
            near = (d2 <= r2[s:e, None]) & has[s:e, None] & has[None, :]
            near[np.arange(e - s), np.arange(s, e)] = False
            i, j = np.nonzero(near)
            i += s
            valid, bins = _pair_bins(a64[i], n64[i], a64[j], n64[j])
            i, bins = i[valid], bins[valid]
            for g in range(3):
                np.add.at(hist, (i, g * BINS + bins[:, g]), 1)
            np.add.at(pairs, i, 1)
        share = np.where(pairs > 0, 100.0 / np.where(pairs > 0, pairs, 1).astype(np.float64), 0.0)
        h64 = hist.astype(np.float64)
        weighted = np.empty((n, DIM), np.float64)
        for s in range(0, n, chunk):
            e = min(n, s + chunk)
            d2 = _d2_rows(a, s, e)
            take = (d2 <= r2[s:e, None]) & (d2 > 0) & (pairs > 0)[None, :]
            take[np.arange(e - s), np.arange(s, e)] = False
            omega = np.where(take, share[None, :] / np.where(take, d2, 1).astype(np.float64), 0.0)
            weighted[s:e] = omega @ h64
        own = np.where((pairs > 0)[:, None], (100.0 * h64) / np.where(pairs > 0, pairs, 1).astype(np.float64)[:, None], 0.0)
        out = np.empty((n, DIM), np.float64)
        for g in range(3):
            cols = slice(g * BINS, (g + 1) * BINS)
            total = np.zeros(n, np.float64)
            for b in range(g * BINS, (g + 1) * BINS):           # ascending, one rounded add at a time
                total = total + weighted[:, b]
            scale = np.where(total > 0.0, 100.0 / np.where(total > 0.0, total, 1.0), 0.0)
            out[:, cols] = own[:, cols] + scale[:, None] * weighted[:, cols]
    return out.astype(np.float32), hist, pairs


def _checked_normals(normals, sizes):
    """the normals of a batch as (n_i, 3) float32 numpy arrays of the clouds' sizes"""
    if len(normals) != len(sizes):
        raise ValueError('%d clouds but %d sets of normals' % (len(sizes), len(normals)))
    arrays = []
    for i, (nr, n) in enumerate(zip(normals, sizes)):
        arr = np.asarray(nr.detach().cpu() if isinstance(nr, torch.Tensor) else nr, dtype=np.float32)
        if arr.shape != (n, 3):
            raise ValueError('normals of cloud %d: shape (%d, 3) expected, got %s' % (i, n, arr.shape))
        arrays.append(np.ascontiguousarray(arr))
    return arrays


def compute_fpfh_host(clouds: Sequence, normals: Sequence, nb_neighbors=30, *, radius=None,
                      return_histograms: bool = False):
    """The definition of the module docstring in numpy: the route without a GPU and the yardstick of the tests.  Brute
    force, O(n^2): meant for tests and small clouds.  Lists of (n_i, 3) clouds and normals -> list of (n_i, 33) float32
    arrays; with `return_histograms` also the lists of (n_i, 33) int32 SPFH histograms and (n_i,) int32 pair counts.
    `radius`: the hybrid neighbourhood, or, with `nb_neighbors=None`, the radius-only one."""
    nb, r = outliers.check_neighbourhood(nb_neighbors, radius, _check_neighbours)
    cap = None if r is None else outliers.radius2(r)
    arrays = outliers._checked_arrays(clouds)
    nrms = _checked_normals(normals, [a.shape[0] for a in arrays])
    parts = [_fpfh_host(a, nr, nb, cap) for a, nr in zip(arrays, nrms)]
    return ragged.results([p[0] for p in parts], [p[1] for p in parts] if return_histograms else None,
                          [p[2] for p in parts] if return_histograms else None)


# ------------------------------------------------------------------------------------------------ device route
def _normal_tensors(normals, sizes):
    """the normals as (n_i, 3) fp32 tensors where they lie, checked against the clouds' sizes before the device is touched"""
    if len(normals) != len(sizes):
        raise ValueError('%d clouds but %d sets of normals' % (len(sizes), len(normals)))
    ts = [torch.as_tensor(nr, dtype=torch.float32) for nr in normals]
    for i, (t, n) in enumerate(zip(ts, sizes)):
        if tuple(t.shape) != (n, 3):
            raise ValueError('normals of cloud %d: shape (%d, 3) expected, got %s' % (i, n, tuple(t.shape)))
    return ts


def compute_fpfh_packed(packed, normals: torch.Tensor, nb, cell=None, radius=None):
    """the descriptors of a packed batch and its (P, 3) fp32 device normals -> (fpfh (P, 33) fp32, hist (P, 33) int32, pairs
    (P,) int32, all in INPUT order, pending (1,) int32), everything on the device; `nb` and `radius` as
    `outliers.check_neighbourhood` returns them"""
    table, sorted_pts, sorted_keys, perm = outliers.sorted_batch(packed, nb, cell, radius)
    sorted_nrm = ops.voxel_gather_rows(normals, perm)
    ws = ops.FpfhWorkspace(int(sorted_pts.shape[0]), table.cells, sorted_pts.device)
    pending = ops.fpfh_radius(ws, sorted_pts, sorted_keys, packed.off, table,
                              radius2=None if radius is None else outliers.radius2(radius), radius_only=nb is None)
    ops.fpfh_spfh(ws, sorted_pts, sorted_nrm, sorted_keys, packed.off, table, THETA_TABLE)
    fpfh = ops.fpfh_combine(ws, sorted_pts, sorted_keys, perm, packed.off, table)
    hist, pairs = torch.empty_like(ws.hist), torch.empty_like(ws.pairs)
    hist[perm] = ws.hist                                         # perm is a permutation: one writer per row
    pairs[perm] = ws.pairs
    return fpfh, hist, pairs, pending


def compute_fpfh(clouds: Sequence, normals: Sequence, nb_neighbors=30, *, radius=None, device='cuda', cell_size=None,
                 return_histograms: bool = False, return_pending: bool = False):
    """`compute_fpfh_host` on the device: lists of raw (n_i, 3) clouds and their normals (numpy / torch, host or device; for
    instance what `estimate_normals` returned, which never leaves the device) -> list of (n_i, 33) float32 device tensors,
    the descriptors of the module docstring.  `return_histograms`: also the lists of (n_i, 33) int32 SPFH histograms and
    (n_i,) int32 pair counts, equal to the numpy route's; `return_pending`: the number of points of the batch that the
    whole-cloud scan finished (a debug counter).  `cell_size` sets the edge of the search grid's cells: it changes no
    histogram, and a descriptor by at most an fp32 ulp.  `radius`: the hybrid neighbourhood of the module docstring, or,
    with `nb_neighbors=None`, the radius-only one (no point pending at the default cell).  `ValueError` for a bad
    parameter, an empty cloud or normals of the wrong shape (before the device is touched) and, naming the cloud, for a
    coordinate that is not finite."""
    nb, r = outliers.check_neighbourhood(nb_neighbors, radius, _check_neighbours)
    cell = None if cell_size is None else ragged.check_positive('cell_size', cell_size)
    nrm_ts = _normal_tensors(normals, [int(t.shape[0]) for t in ragged.as_tensors(clouds)])
    with ragged.intake(clouds, device) as packed:
        if packed is None:
            return ragged.results([], [] if return_histograms else None, [] if return_histograms else None,
                                  0 if return_pending else None)
        nrm = ragged.upload(nrm_ts, packed.pts.device).pts
        fpfh, hist, pairs, pending = compute_fpfh_packed(packed, nrm, nb, cell, r)
        return ragged.results(packed.split(fpfh), packed.split(hist) if return_histograms else None,
                              packed.split(pairs) if return_histograms else None,
                              int(pending.item()) if return_pending else None)


# ------------------------------------------------------------------------------------------------ correspondences
def _feature_rows(batch, what: str):
    """(rows (N, D) float32 tensor, offsets (P + 1,) int64 numpy, was_list) of a list of (N_i, D) feature arrays or a
    `(rows, offsets)` tuple"""
    as_list = isinstance(batch, list)
    if not as_list and not (isinstance(batch, tuple) and len(batch) == 2):
        raise ValueError('%s: a list of (N_i, D) feature arrays or a (rows, offsets) tuple expected' % what)
    parts = [torch.as_tensor(c) for c in (batch if as_list else [batch[0]])]
    if not parts:
        raise ValueError('%s: no pairs' % what)
    for c in parts:
        if c.dim() != 2:
            raise ValueError('%s: (N, D) feature rows expected, got shape %s' % (what, tuple(c.shape)))
        if c.dtype != torch.float32:
            raise TypeError('%s: float32 features expected, got %s' % (what, c.dtype))
    dim = int(parts[0].shape[1])
    if any(int(c.shape[1]) != dim for c in parts) or not 1 <= dim <= MAX_FEATURE_DIM:
        raise ValueError('%s: one D in 1..%d for every row expected, got %s'
                         % (what, MAX_FEATURE_DIM, sorted({int(c.shape[1]) for c in parts})))
    if as_list:
        off = np.zeros(len(parts) + 1, np.int64)
        np.cumsum([c.shape[0] for c in parts], out=off[1:])
        return torch.cat(parts, 0).contiguous(), off, True
    offsets = batch[1]
    off = _as_numpy(offsets)
    if off.ndim != 1 or off.shape[0] < 2 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError('%s: (P + 1,) integer offsets with P >= 1 expected' % what)
    off = off.astype(np.int64)
    if off[0] != 0 or off[-1] != parts[0].shape[0] or (np.diff(off) < 0).any():
        raise ValueError('%s: offsets must start at 0, not decrease, and end at the number of rows (%d)'
                         % (what, parts[0].shape[0]))
    return parts[0].contiguous(), off, False


def _feature_pairs(source, target, what: str, device_route: bool):
    q, q_off, was_list = _feature_rows(source, what)
    t, t_off, _ = _feature_rows(target, what)
    if q_off.shape[0] != t_off.shape[0]:
        raise ValueError('%s: %d sources against %d targets: the two batches must pair up'
                         % (what, q_off.shape[0] - 1, t_off.shape[0] - 1))
    if q.shape[1] != t.shape[1]:
        raise ValueError('%s: source rows have D = %d, target rows D = %d' % (what, q.shape[1], t.shape[1]))
    if device_route and not (q.is_cuda and t.is_cuda):
        raise _native.NativeLibraryError('%s runs on the GPU and takes GPU tensors (%s_host is the CPU route)' % (what, what))
    return q, q_off, t, t_off, was_list


def _split(x, off, was_list):
    if not was_list:
        return x
    sizes = np.diff(off).tolist()
    return list(torch.split(x, sizes, 0)) if isinstance(x, torch.Tensor) else [x[s:e] for s, e in zip(off[:-1], off[1:])]


_host_feature_d2 = _host_d2_32           # the arithmetic of `hfl_feature_nn` is that of the pair scan at any D


def _host_feature_nn(q: np.ndarray, t: np.ndarray):
    """(idx (n,) int32, dist2 (n,) float32) of one pair, brute force, chunked over the rows"""
    dist2, idx = _host_argmin32(q, t, _HOST_CHUNK)
    return idx, dist2


def feature_correspondences_host(source_features, target_features, *, mutual: bool = False):
    """The definition of `feature_correspondences` in numpy, brute force: lists of (N_i, D) arrays (-> lists), or `(rows,
    offsets)` tuples (-> concatenated arrays) -> `(idx int32, dist2 float32)`, with `mutual` also the bool mask."""
    q, q_off, t, t_off, was_list = _feature_pairs(source_features, target_features, 'feature_correspondences', False)
    q, t = q.numpy(), t.numpy()
    if not (np.isfinite(q).all() and np.isfinite(t).all()):
        raise ValueError('feature_correspondences: features must be finite')
    idx, dist2 = np.empty(q.shape[0], np.int32), np.empty(q.shape[0], np.float32)
    mask = np.zeros(q.shape[0], bool)
    for p in range(q_off.shape[0] - 1):
        qs, ts = slice(q_off[p], q_off[p + 1]), slice(t_off[p], t_off[p + 1])
        idx[qs], dist2[qs] = _host_feature_nn(q[qs], t[ts])
        if mutual and t[ts].shape[0] and q[qs].shape[0]:
            back, _ = _host_feature_nn(t[ts], q[qs])
            mask[qs] = back[idx[qs]] == np.arange(q[qs].shape[0])
    return ragged.results(_split(idx, q_off, was_list), _split(dist2, q_off, was_list),
                          _split(mask, q_off, was_list) if mutual else None)


def feature_correspondences(source_features, target_features, *, mutual: bool = False):
    """Every source row's nearest target row in feature space, for ragged pairs on the device: lists of (N_i, D) float32
    GPU tensors (-> lists of per-pair tensors), or `(rows (N, D), offsets (P + 1,))` tuples (-> concatenated tensors), D in
    1..64 -> `(idx int32, dist2 float32)`: the row within the pair's target (the lowest index of equal distances, -1 for a
    pair without targets) and the squared distance (+inf there), as the module docstring defines them; with `mutual` also
    the bool mask of the rows whose target's own nearest source is that row -- the same launch with the roles swapped and a
    compare.  `ValueError` for D outside 1..64, sides that do not pair up or differ in D; `NativeLibraryError` for CPU
    tensors (`feature_correspondences_host` is the CPU route)."""
    q, q_off, t, t_off, was_list = _feature_pairs(source_features, target_features, 'feature_correspondences', True)
    with torch.cuda.device(q.device):
        q_dev, t_dev = torch.from_numpy(q_off).to(q.device), torch.from_numpy(t_off).to(q.device)
        tiles = torch.from_numpy(ops.feature_tiles(np.diff(q_off))).to(q.device)
        dist2, idx = ops.feature_nn(q, q_dev, t, t_dev, tiles)
        mask = None
        if mutual:
            back_tiles = torch.from_numpy(ops.feature_tiles(np.diff(t_off))).to(q.device)
            _, back = ops.feature_nn(t, t_dev, q, q_dev, back_tiles)
            lengths = torch.from_numpy(np.diff(q_off)).to(q.device)
            pair = torch.repeat_interleave(torch.arange(lengths.shape[0], device=q.device), lengths)
            local = torch.arange(q.shape[0], device=q.device) - q_dev[pair]
            has = idx >= 0
            where = (t_dev[pair] + idx.clamp(min=0).to(torch.int64)).clamp(max=max(int(t.shape[0]) - 1, 0))
            mask = has & (back[where].to(torch.int64) == local) if t.shape[0] else torch.zeros_like(has)
    return ragged.results(_split(idx, q_off, was_list), _split(dist2, q_off, was_list),
                          _split(mask, q_off, was_list) if mutual else None)
