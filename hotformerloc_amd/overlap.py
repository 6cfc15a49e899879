"""Ground-to-aerial submap overlap and Chamfer distance, on the GPU.

The reference's `misc/compute_ground_aerial_overlap.py` pairs every ground submap of CS-Wild-Places with its nearest aerial
(or airborne) submap within 10 m, builds both SE(3) poses, aligns the ground cloud into the aerial submap's frame -- and
stops at `TODO: dist = chamfer_distance(...)`, printing "Average chamfer distance for {split}: TO-DO".  This module is that
script's body with the distance filled in:

    match_nearest_pose   the `KDTree.query` over the aerial x, y and the `POSITIVE_MAX_THRESH` skip
    pose_matrix          `quaternion_to_rot` on the x, y, z, qx, qy, qz, qw columns of poses.csv
    relative_pose        `relative_pose`: inv(m_b) @ m_a in float64, frame a -> frame b
    transform_points     `apply_transform` on the float32 cast of that matrix           (hfl_transform_points)
    nn_distances         every point's nearest neighbour in the other cloud             (hfl_nn_dist)
    chamfer_distance     the mean nearest-neighbour distance, both ways, and their sum  (hfl_pair_stats)
    overlap_ratio        the share of each cloud's points with a neighbour within tau   (hfl_pair_stats)
    submap_overlap       all of it for already-matched pairs, with the per-split means the script meant to print

A batch of P pairs is ragged: a list of (N_i, 3) float32 clouds, or the pair `(points (N, 3), offsets (P + 1,))` with cloud
p at rows [offsets[p], offsets[p + 1]).  Poses are composed in float64 and only the relative pose is rounded to float32, as
the script does: a UTM northing (~6.9e6) never meets float32.  The search is brute force over LDS tiles (csrc/overlap.hip):
exact, the lowest index winning ties, two runs giving the same bits.  Coordinates must be finite; this is not checked.

The device functions raise `NativeLibraryError` on CPU tensors and launch on the current stream.  Each has a `*_host` twin in
numpy float64 (brute force, chunked so that no temporary exceeds about 64 MiB, no scipy): the route without a GPU and the
yardstick of the tests.  The host transform is the float64 product rounded once to float32; the host distances are float64
distances between the float32 points.
"""

from collections import namedtuple

import numpy as np
import torch

from . import _native

POSITIVE_MAX_THRESH = 10.0             # metres: the script's cut on the distance to the matched aerial submap
DEFAULT_TAU = 0.8                      # metres: the voxel size of the CS-Wild-Places submaps (postproc_voxel_0.80m)
_HOST_CHUNK_PAIRS = 1 << 23            # point pairs of one host chunk: (rows, M) float64 temporaries of 64 MiB

ChamferResult = namedtuple('ChamferResult', ['a_to_b', 'b_to_a', 'chamfer'])
SubmapOverlap = namedtuple('SubmapOverlap', ['transforms', 'chamfer', 'overlap', 'mean_a_to_b', 'mean_b_to_a', 'mean_chamfer',
                                             'mean_overlap', 'n_pairs'])
SubmapOverlap.__doc__ = """What `submap_overlap` returns.  transforms: (P, 4, 4) float64 numpy, ground frame -> aerial frame;
chamfer: the `ChamferResult` of the aligned pairs; overlap: the `overlap_ratio` of the aligned pairs; mean_a_to_b,
mean_b_to_a, mean_chamfer: floats, the means over the pairs that have both clouds (the split's "Average chamfer distance");
mean_overlap: (2,) or (2, K) float64 numpy, the same mean of the overlap; n_pairs: how many pairs the means cover."""


# ------------------------------------------------------------------------------------------------------------ pose helpers
def pose_matrix(xyzq):
    """(..., 7) rows of x, y, z, qx, qy, qz, qw -> (..., 4, 4) float64 SE(3) matrices [R | t; 0 0 0 1].  The quaternion is
    normalised first, as scipy's `Rotation.from_quat` (the reference's `quaternion_to_rot`) does; a zero quaternion is a
    ValueError."""
    p = np.asarray(xyzq, dtype=np.float64)
    if p.ndim < 1 or p.shape[-1] != 7:
        raise ValueError('pose_matrix: (..., 7) rows of x, y, z, qx, qy, qz, qw expected, got shape %s' % (p.shape,))
    q = p[..., 3:]
    norm = np.sqrt((q * q).sum(-1, keepdims=True))
    if not (norm > 0.0).all():
        raise ValueError('pose_matrix: a quaternion of zero norm')
    x, y, z, w = np.moveaxis(q / norm, -1, 0)
    m = np.zeros(p.shape[:-1] + (4, 4), np.float64)
    m[..., 0, 0] = 1.0 - 2.0 * (y * y + z * z)
    m[..., 0, 1] = 2.0 * (x * y - z * w)
    m[..., 0, 2] = 2.0 * (x * z + y * w)
    m[..., 1, 0] = 2.0 * (x * y + z * w)
    m[..., 1, 1] = 1.0 - 2.0 * (x * x + z * z)
    m[..., 1, 2] = 2.0 * (y * z - x * w)
    m[..., 2, 0] = 2.0 * (x * z - y * w)
    m[..., 2, 1] = 2.0 * (y * z + x * w)
    m[..., 2, 2] = 1.0 - 2.0 * (x * x + y * y)
    m[..., :3, 3] = p[..., :3]
    m[..., 3, 3] = 1.0
    return m


def relative_pose(m_a, m_b):
    """inv(m_b) @ m_a in float64, (..., 4, 4): coordinates in frame a -> coordinates in frame b, the reference script's
    convention (m_a, m_b map their frame to the world)."""
    m_a, m_b = np.asarray(m_a, dtype=np.float64), np.asarray(m_b, dtype=np.float64)
    if m_a.shape[-2:] != (4, 4) or m_b.shape[-2:] != (4, 4):
        raise ValueError('relative_pose: (..., 4, 4) matrices expected, got %s and %s' % (m_a.shape, m_b.shape))
    return np.linalg.inv(m_b) @ m_a


def match_nearest_pose(query_xy, database_xy, max_dist=POSITIVE_MAX_THRESH):
    """(Q,) int64: for every query position the index of the nearest database position, in float64, the lowest index on a
    tie; -1 where even that one is farther than `max_dist` (the script's `KDTree.query` and its POSITIVE_MAX_THRESH skip).
    Chunked numpy on the host: a few thousand poses, not a hot path."""
    q = np.ascontiguousarray(query_xy, dtype=np.float64)
    d = np.ascontiguousarray(database_xy, dtype=np.float64)
    if q.ndim != 2 or d.ndim != 2 or q.shape[1] != d.shape[1] or d.shape[0] < 1:
        raise ValueError('match_nearest_pose: (Q, D) queries and (N >= 1, D) database positions expected')
    out = np.empty(q.shape[0], np.int64)
    rows = max(1, _HOST_CHUNK_PAIRS // d.shape[0])
    for r0 in range(0, q.shape[0], rows):
        diff = q[r0:r0 + rows, None, :] - d[None, :, :]
        d2 = (diff * diff).sum(-1)
        k = d2.argmin(1)                                               # the first of equal minima
        near = np.sqrt(d2[np.arange(k.shape[0]), k]) <= float(max_dist)
        out[r0:r0 + rows] = np.where(near, k, -1)
    return out


# ------------------------------------------------------------------------------------------------------------ ragged batches
def _float32_points(x, what):
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError('%s: (N, 3) points expected, got shape %s' % (what, tuple(x.shape)))
    if x.dtype == torch.float64:
        raise TypeError('%s: float64 points: the kernels work in float32.  Compose the poses in float64 and hand the relative '
                        'pose to transform_points (or pass transforms=), then the points never need more than float32; cast '
                        'them yourself if that is what you mean' % what)
    if x.dtype != torch.float32:
        raise TypeError('%s: float32 points expected, got %s' % (what, x.dtype))
    return x


def _ragged(batch, what, device_route):
    """(points (N, 3) float32 tensor, offsets (P + 1,) int64 numpy, was_list).  `batch` is a list of (N_i, 3) clouds or a
    `(points, offsets)` pair; numpy arrays are taken on the host route only."""
    as_list = isinstance(batch, list)
    if not as_list and not (isinstance(batch, tuple) and len(batch) == 2):
        raise ValueError('%s: a list of (N_i, 3) clouds or a (points, offsets) tuple expected' % what)
    if as_list:
        clouds = [torch.as_tensor(c) for c in batch]
        if not clouds:
            raise ValueError('%s: no clouds' % what)
        for c in clouds:
            _float32_points(c, what)
        if device_route and not all(c.is_cuda for c in clouds):
            raise _native.NativeLibraryError('%s runs on the GPU and takes GPU tensors (%s_host is the CPU route)' % (what, what))
        off = np.zeros(len(clouds) + 1, np.int64)
        np.cumsum([c.shape[0] for c in clouds], out=off[1:])
        return torch.cat(clouds, 0).contiguous(), off, True
    points, offsets = batch
    points = _float32_points(torch.as_tensor(points), what)
    if device_route and not points.is_cuda:
        raise _native.NativeLibraryError('%s runs on the GPU and takes GPU tensors (%s_host is the CPU route)' % (what, what))
    off = _as_numpy(offsets)
    if off.ndim != 1 or off.shape[0] < 2 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError('%s: (P + 1,) integer offsets with P >= 1 expected' % what)
    off = off.astype(np.int64)
    if off[0] != 0 or off[-1] != points.shape[0] or (np.diff(off) < 0).any():
        raise ValueError('%s: offsets must start at 0, not decrease, and end at the number of points (%d)'
                         % (what, points.shape[0]))
    return points.contiguous(), off, False


def _unragged(points, off, was_list):
    if was_list:
        return list(torch.split(points, np.diff(off).tolist(), 0))
    return points


def _matrices(transforms, pairs, what):
    """(P, 3, 4) float64 numpy from (P, 4, 4) or (P, 3, 4) (a single matrix serves a single pair)"""
    m = _as_numpy(transforms)
    m = np.asarray(m, dtype=np.float64)
    if m.ndim == 2:
        m = m[None]
    if m.ndim != 3 or m.shape[0] != pairs or m.shape[1:] not in ((4, 4), (3, 4)):
        raise ValueError('%s: (%d, 4, 4) or (%d, 3, 4) transforms expected, got shape %s' % (what, pairs, pairs, m.shape))
    return np.ascontiguousarray(m[:, :3, :])


def _same_pairs(off_a, off_b, what):
    if off_a.shape[0] != off_b.shape[0]:
        raise ValueError('%s: %d clouds against %d: the two batches must pair up' % (what, off_a.shape[0] - 1, off_b.shape[0] - 1))


def _taus(tau):
    single = np.ndim(tau) == 0
    taus = [float(tau)] if single else [float(t) for t in tau]
    if not taus or not all(t >= 0.0 for t in taus):
        raise ValueError('tau: one threshold or a sequence of thresholds, each a number >= 0')
    return taus, single


# ------------------------------------------------------------------------------------------------------------ device route
def _device_transform(points, off, dev_off, matrices):
    from . import ops
    m32 = torch.from_numpy(matrices.reshape(-1, 12).astype(np.float32)).to(points.device)     # rounded once, after composing
    return ops.transform_points(points, dev_off, m32)


def _device_nn(q, q_off, q_dev_off, t, t_dev_off):
    from . import ops
    tiles = torch.from_numpy(ops.overlap_tiles(np.diff(q_off))).to(q.device)
    return ops.nn_dist(q, q_dev_off, t, t_dev_off, tiles)


def transform_points(clouds, transforms):
    """R_p x + t_p for every point of pair p: the reference script's `apply_transform` for a ragged batch, returned in the
    layout that came in (a list of clouds, or the (N, 3) tensor).  `transforms`: (P, 4, 4) or (P, 3, 4), numpy or tensor;
    they are taken in float64 and rounded to float32 here, once -- compose poses before, not after, this call.  Each
    coordinate is fmaf(r2, z, fmaf(r1, y, fmaf(r0, x, t))) in float32."""
    points, off, was_list = _ragged(clouds, 'transform_points', True)
    m = _matrices(transforms, off.shape[0] - 1, 'transform_points')
    with torch.cuda.device(points.device):
        out = _device_transform(points, off, torch.from_numpy(off).to(points.device), m)
    return _unragged(out, off, was_list)


def nn_distances(src, dst):
    """`(dist, idx, offsets)` on the device: for every point of src cloud p the distance to its nearest point in dst cloud p
    (float32) and that point's index within the cloud (int32; the lowest index of equal distances), concatenated over the
    pairs with `offsets` (P + 1,) int64 as src's.  +inf and -1 where the dst cloud is empty."""
    q, q_off, _ = _ragged(src, 'nn_distances', True)
    t, t_off, _ = _ragged(dst, 'nn_distances', True)
    _same_pairs(q_off, t_off, 'nn_distances')
    with torch.cuda.device(q.device):
        q_dev_off = torch.from_numpy(q_off).to(q.device)
        dist, idx = _device_nn(q, q_off, q_dev_off, t, torch.from_numpy(t_off).to(q.device))
    return dist, idx, q_dev_off


def _device_stats(a, b, transforms, taus, what):
    """Both directions of a batch: (sums (2, P, 2) float64, counts (2, P, K + 1) int64, lengths (2, P) int64), all on the
    device; direction 0 is a -> b."""
    from . import ops
    pa, a_off, _ = _ragged(a, what, True)
    pb, b_off, _ = _ragged(b, what, True)
    _same_pairs(a_off, b_off, what)
    with torch.cuda.device(pa.device):
        a_dev, b_dev = torch.from_numpy(a_off).to(pa.device), torch.from_numpy(b_off).to(pa.device)
        if transforms is not None:                                     # materialised once: both directions read this cloud
            pa = _device_transform(pa, a_off, a_dev, _matrices(transforms, a_off.shape[0] - 1, what))
        d_ab, _ = _device_nn(pa, a_off, a_dev, pb, b_dev)
        d_ba, _ = _device_nn(pb, b_off, b_dev, pa, a_dev)
        s_ab, c_ab = ops.pair_stats(d_ab, a_dev, taus)
        s_ba, c_ba = ops.pair_stats(d_ba, b_dev, taus)
        lengths = torch.from_numpy(np.stack([np.diff(a_off), np.diff(b_off)])).to(pa.device)
    return torch.stack([s_ab, s_ba]), torch.stack([c_ab, c_ba]), lengths


def _chamfer_from(sums, counts, lengths, squared):
    valid = (lengths - counts[..., -1]).to(torch.float64)             # rows that found a neighbour; 0 / 0 = NaN
    mean = sums[..., 1 if squared else 0] / valid
    return ChamferResult(mean[0], mean[1], mean[0] + mean[1])


def _overlap_from(counts, lengths, single):
    share = counts[..., :-1].to(torch.float64) / lengths.to(torch.float64)[..., None]      # (2, P, K); 0 / 0 = NaN
    share = share.permute(1, 0, 2).contiguous()
    return share[..., 0].contiguous() if single else share


def chamfer_distance(a, b, transforms=None, squared=False):
    """`ChamferResult(a_to_b, b_to_a, chamfer)`: per-pair (P,) float64 tensors on the device.  a_to_b is the mean distance
    from a point of cloud a to its nearest point of cloud b (the mean squared distance with `squared=True`), b_to_a the
    reverse, chamfer their sum.  `transforms` (see `transform_points`) are applied to `a` once and both directions run on
    the transformed cloud, so a matrix that is not rigid is handled as it stands.  A direction whose query or target cloud
    is empty is NaN.  The sums run in float64 over the float32 distances."""
    sums, counts, lengths = _device_stats(a, b, transforms, (), 'chamfer_distance')
    return _chamfer_from(sums, counts, lengths, squared)


def overlap_ratio(a, b, transforms=None, tau=DEFAULT_TAU):
    """(P, 2) float64 on the device: column 0 the share of cloud a's points whose nearest point of cloud b lies within
    `tau`, column 1 the same for cloud b's points against cloud a; a tuple of K thresholds (K <= ops.OVERLAP_MAX_TAUS)
    gives (P, 2, K).  `distance <= tau` in float32.  An empty cloud's own share is NaN; against an empty cloud it is 0."""
    taus, single = _taus(tau)
    _, counts, lengths = _device_stats(a, b, transforms, taus, 'overlap_ratio')
    return _overlap_from(counts, lengths, single)


def _poses(poses, pairs, what):
    p = _as_numpy(poses)
    p = np.asarray(p, dtype=np.float64)
    if p.shape == (pairs, 7):
        return pose_matrix(p)
    if p.shape == (pairs, 4, 4):
        return p
    raise ValueError('%s: (%d, 7) pose rows or (%d, 4, 4) matrices expected, got shape %s' % (what, pairs, pairs, p.shape))


def _summary(transforms, chamfer, overlap, to_numpy):
    a_to_b, b_to_a, both, ov = (to_numpy(x) for x in (chamfer.a_to_b, chamfer.b_to_a, chamfer.chamfer, overlap))
    full = np.isfinite(both)                                           # pairs with both clouds
    n = int(full.sum())
    mean = lambda x: float(x[full].mean()) if n else float('nan')      # noqa: E731
    mean_ov = ov[full].mean(0) if n else np.full(ov.shape[1:], np.nan)
    return SubmapOverlap(transforms, chamfer, overlap, mean(a_to_b), mean(b_to_a), mean(both), mean_ov, n)


def submap_overlap(ground, aerial, ground_poses, aerial_poses, tau=DEFAULT_TAU):
    """The body of the reference script for P already-matched pairs (`match_nearest_pose` finds them): the relative pose of
    every ground submap with respect to its aerial one in float64, the ground cloud aligned into the aerial frame, the
    Chamfer distance and the overlap at `tau` of the aligned pair -> `SubmapOverlap`.  Poses: (P, 7) rows of x, y, z, qx,
    qy, qz, qw as in poses.csv, or (P, 4, 4) matrices.  One read of the per-pair results for the split means."""
    taus, single = _taus(tau)
    pairs = len(ground) if isinstance(ground, list) else len(ground[1]) - 1
    transforms = relative_pose(_poses(ground_poses, pairs, 'submap_overlap'), _poses(aerial_poses, pairs, 'submap_overlap'))
    sums, counts, lengths = _device_stats(ground, aerial, transforms, taus, 'submap_overlap')
    return _summary(transforms, _chamfer_from(sums, counts, lengths, False), _overlap_from(counts, lengths, single),
                    lambda x: x.cpu().numpy())


# -------------------------------------------------------------------------------------------------------------- host route
def _as_numpy(x):
    """a tensor (wherever it lies) or anything array-like as a numpy array"""
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _host_ragged(batch, what):
    if isinstance(batch, list):
        batch = [torch.as_tensor(c).cpu() for c in batch]
    else:
        batch = (torch.as_tensor(batch[0]).cpu(), batch[1])
    points, off, was_list = _ragged(batch, what, False)
    return points.numpy(), off, was_list


def transform_points_host(clouds, transforms):
    """`transform_points` on the CPU: the float64 product R x + t of the float64 matrix and the float32 points, rounded once
    to float32.  The same layouts, as numpy arrays."""
    points, off, was_list = _host_ragged(clouds, 'transform_points')
    m = _matrices(transforms, off.shape[0] - 1, 'transform_points')
    per_point = np.repeat(m, np.diff(off), axis=0)                    # (N, 3, 4)
    out = (np.einsum('nij,nj->ni', per_point[:, :, :3], points.astype(np.float64)) + per_point[:, :, 3]).astype(np.float32)
    return [out[off[p]:off[p + 1]] for p in range(off.shape[0] - 1)] if was_list else out


def _host_nn_one(q, t, chunk_pairs):
    """float64 (dist (n,), idx (n,) int32) of one pair, chunked over query rows"""
    dist = np.full(q.shape[0], np.inf, np.float64)
    idx = np.full(q.shape[0], -1, np.int32)
    if q.shape[0] == 0 or t.shape[0] == 0:
        return dist, idx
    q, t = q.astype(np.float64), t.astype(np.float64)
    rows = max(1, int(chunk_pairs) // t.shape[0])
    for r0 in range(0, q.shape[0], rows):
        c = q[r0:r0 + rows]
        dx = c[:, None, 0] - t[None, :, 0]
        dy = c[:, None, 1] - t[None, :, 1]
        dz = c[:, None, 2] - t[None, :, 2]
        d2 = dx * dx + dy * dy + dz * dz
        k = d2.argmin(1)                                               # the first of equal minima: the lowest index
        dist[r0:r0 + rows] = np.sqrt(d2[np.arange(k.shape[0]), k])
        idx[r0:r0 + rows] = k
    return dist, idx


def _fmaf(a, b, c):
    """fmaf on float32 arrays: the product is exact in float64, the sum is rounded there and then to float32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _host_d2_32(q, t):
    """the (n, m) float32 squared distances between two sets of (., D) float32 rows with the arithmetic of the device's pair
    scan: d0 d0, then fmaf(dc, dc, acc) for c = 1 .. D - 1 (for D = 3 that is fmaf(dz, dz, fmaf(dy, dy, dx dx)))"""
    with np.errstate(over='ignore', invalid='ignore'):
        d = q[:, None, 0] - t[None, :, 0]                              # float32 throughout
        acc = d * d
        for col in range(1, q.shape[1]):
            d = q[:, None, col] - t[None, :, col]
            acc = _fmaf(d, d, acc)
    return acc


def _host_argmin32(q, t, chunk_pairs=_HOST_CHUNK_PAIRS // 2):
    """(dist2 (n,) float32, idx (n,) int32) of one pair by `_host_d2_32`, brute force, chunked over query rows: the twin of
    `hfl_nn_dist` before its square root (D = 3) and of `hfl_feature_nn`.  +inf and -1 without targets."""
    dist2 = np.full(q.shape[0], np.inf, np.float32)
    idx = np.full(q.shape[0], -1, np.int32)
    if q.shape[0] == 0 or t.shape[0] == 0:
        return dist2, idx
    rows = max(1, int(chunk_pairs) // t.shape[0])
    for r0 in range(0, q.shape[0], rows):
        d2 = _host_d2_32(q[r0:r0 + rows], t)
        k = d2.argmin(1)                                               # the first of equal minima: the lowest index
        dist2[r0:r0 + rows] = d2[np.arange(k.shape[0]), k]
        idx[r0:r0 + rows] = k
    return dist2, idx


def nn_distances_host(src, dst, chunk_pairs=_HOST_CHUNK_PAIRS):
    """`nn_distances` on the CPU, brute force in float64 between the float32 points: `(dist float64, idx int32, offsets
    int64)` as numpy arrays.  `chunk_pairs` bounds the point pairs of one temporary; the result does not depend on it."""
    q, q_off, _ = _host_ragged(src, 'nn_distances')
    t, t_off, _ = _host_ragged(dst, 'nn_distances')
    _same_pairs(q_off, t_off, 'nn_distances')
    parts = [_host_nn_one(q[q_off[p]:q_off[p + 1]], t[t_off[p]:t_off[p + 1]], chunk_pairs) for p in range(q_off.shape[0] - 1)]
    return np.concatenate([d for d, _ in parts]), np.concatenate([i for _, i in parts]), q_off


def _host_stats(a, b, transforms, what):
    """per direction the list of every pair's float64 distances"""
    pa, a_off, _ = _host_ragged(a, what)
    pb, b_off, _ = _host_ragged(b, what)
    _same_pairs(a_off, b_off, what)
    if transforms is not None:
        pa = transform_points_host((pa, a_off), transforms)
    d_ab, _, _ = nn_distances_host((pa, a_off), (pb, b_off))
    d_ba, _, _ = nn_distances_host((pb, b_off), (pa, a_off))
    pairs = range(a_off.shape[0] - 1)
    return [d_ab[a_off[p]:a_off[p + 1]] for p in pairs], [d_ba[b_off[p]:b_off[p + 1]] for p in pairs]


def _nan_mean(x):
    x = x[np.isfinite(x)]                                             # +inf: no target cloud
    return x.mean() if x.size else np.nan


def chamfer_distance_host(a, b, transforms=None, squared=False):
    """`chamfer_distance` on the CPU in float64: a `ChamferResult` of (P,) float64 numpy arrays."""
    power = 2 if squared else 1
    ab, ba = (np.array([_nan_mean(d ** power) for d in side], np.float64)
              for side in _host_stats(a, b, transforms, 'chamfer_distance'))
    return ChamferResult(ab, ba, ab + ba)


def overlap_ratio_host(a, b, transforms=None, tau=DEFAULT_TAU):
    """`overlap_ratio` on the CPU: float64 distances against the float64 thresholds, (P, 2) or (P, 2, K) float64 numpy."""
    taus, single = _taus(tau)
    sides = _host_stats(a, b, transforms, 'overlap_ratio')
    out = np.array([[[(d <= t).sum() / d.size if d.size else np.nan for t in taus] for d in side] for side in sides], np.float64)
    out = np.ascontiguousarray(out.transpose(1, 0, 2))
    return out[..., 0].copy() if single else out


def submap_overlap_host(ground, aerial, ground_poses, aerial_poses, tau=DEFAULT_TAU):
    """`submap_overlap` on the CPU, from the host twins."""
    pairs = len(ground) if isinstance(ground, list) else len(ground[1]) - 1
    transforms = relative_pose(_poses(ground_poses, pairs, 'submap_overlap'), _poses(aerial_poses, pairs, 'submap_overlap'))
    return _summary(transforms, chamfer_distance_host(ground, aerial, transforms), overlap_ratio_host(ground, aerial, transforms, tau),
                    lambda x: x)
