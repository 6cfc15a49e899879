"""Raw submaps -> the clouds `prepare_clouds` expects, for a whole ragged batch on the device.

The reference prepares CS-Wild-Places submaps offline, on the host, one at a time, through open3d
(`datasets/CSWildPlaces/postprocess_submaps.py`): a voxel-grid downsample at 0.8 m (`processing_utils.voxel_down_sample`,
which is open3d's `PointCloud.voxel_down_sample`), then the PointNetVLAD normalisation (`processing_utils.normalise_pcl`).
Here a batch of raw submaps goes to the GPU once and comes back as device tensors; open3d is not needed.

Downsample (open3d's definition, restated in float64 as open3d computes it; v = `voxel_size`), per cloud of fp32 points p:

    origin  = min(p, axis=0) as float64 - 0.5 v
    cell(p) = floor((float64(p) - origin) / v)              per axis: one float64 subtract and one divide
    output  = one point per occupied cell: the members' float64 sum / their count, rounded once to fp32

The device computes the cells in float64 too, so cell membership is bit-identical to the numpy route below, points that
sit exactly on a cell face included (they go to the upper cell).  open3d returns the cells in the order of its hash map;
this module defines the order as ascending (ix, iy, iz), ix most significant.  The float64 summation order differs between
the routes, which can move a mean's final rounding by at most one fp32 ulp; on the device the order is fixed, so two calls
give the same bits and a cloud gives the same bits alone or inside a batch.

Normalise (`normalise_pcl` with `downsample_number=None`: the voxel route never pads), in float64 per cloud of points q:

    c = mean(q, axis=0);  d = mean(|q - c|);  s = 0.5 / d;  q' = s (q - c)
    keep the rows with every |q'| <= 1, in order, rounded once to fp32

Device route: `hfl_voxel_keys` (per-cloud bounds, one int64 key per point: cloud << 48 | ix << 32 | iy << 16 | iz),
`torch.sort(keys, stable=True)` (plumbing, as `torch.topk` is in the loss), `hfl_voxel_reduce` (segment heads, scan,
float64 segment sums, compacted fp32 means, per-cloud output offsets) and `hfl_submap_normalise` (a workgroup per cloud);
`csrc/voxel.hip`.  Each public call uploads the batch once and reads counts and flags back once.

Limits: a cloud may span at most 65 535 cells along an axis (16 bits per axis in the key) and a batch may hold at most
32 767 clouds (15 bits, so the key stays a positive int64); both raise `ValueError`.  Non-finite coordinates give
undefined output (nothing is read or written out of bounds).

Out of scope: CSF ground removal (`postprocess_submaps.py --remove_ground`), the `random` and `pnvlad` downsamplers
(`--downsample_type`), and the padding branch of `normalise_pcl` (`downsample_number` set)."""

import math
from typing import List, Sequence

import numpy as np
import torch

from . import _native, ops

MAX_CLOUDS = ops.VOXEL_MAX_CLOUDS
MAX_CELLS = ops.VOXEL_MAX_CELLS


def _check_voxel_size(voxel_size) -> float:
    v = float(voxel_size)
    if not math.isfinite(v) or v <= 0.0:
        raise ValueError('voxel_size must be positive and finite, got %r' % (voxel_size,))
    return v


def _check_batch(sizes):
    if len(sizes) > MAX_CLOUDS:
        raise ValueError('a batch holds at most %d clouds, got %d' % (MAX_CLOUDS, len(sizes)))
    for i, n in enumerate(sizes):
        if n < 1:
            raise ValueError('cloud %d is empty' % i)


def _span_error(i: int):
    return ValueError('cloud %d spans %d or more voxels along an axis (at most %d fit the 16-bit cell index); '
                      'use a larger voxel_size' % (i, MAX_CELLS + 1, MAX_CELLS))


def _degenerate_error(i: int):
    return ValueError('cloud %d cannot be normalised: its mean distance to the centroid is zero (a single point)' % i)


def _empty_error(i: int):
    return ValueError('cloud %d has no point left inside [-1, 1]^3 after normalisation' % i)


# ------------------------------------------------------------------------------------------------ host route (numpy float64)
def _cell_means(cloud: np.ndarray, v: float, index: int):
    """one cloud -> (float64 means (m, 3), members (m,), cells ix << 32 | iy << 16 | iz (m,)) in ascending cell order"""
    p = cloud.astype(np.float64)
    origin = p.min(axis=0) - 0.5 * v
    cell = np.floor((p - origin) / v)
    if not cell.max() < MAX_CELLS:
        raise _span_error(index)
    cell = cell.astype(np.int64)
    key = (cell[:, 0] << 32) | (cell[:, 1] << 16) | cell[:, 2]
    uniq, inverse, cnt = np.unique(key, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    total = np.stack([np.bincount(inverse, weights=p[:, k], minlength=uniq.size) for k in range(3)], 1)
    return total / cnt[:, None], cnt, uniq.astype(np.int64)


def voxel_downsample_host(clouds: Sequence, voxel_size: float, return_counts: bool = False, return_keys: bool = False):
    """The definition above in numpy float64: the route without a GPU and the yardstick of the tests.  List of (n_i, 3)
    clouds -> list of (m_i, 3) float32 arrays in ascending (ix, iy, iz); with `return_counts` also the members of every
    output point (int32), with `return_keys` also its cell as ix << 32 | iy << 16 | iz (int64)."""
    v = _check_voxel_size(voxel_size)
    arrays = [np.asarray(c.cpu() if isinstance(c, torch.Tensor) else c, dtype=np.float32).reshape(-1, 3) for c in clouds]
    _check_batch([a.shape[0] for a in arrays])
    outs, counts, keys = [], [], []
    for i, a in enumerate(arrays):
        mean, cnt, uniq = _cell_means(a, v, i)
        outs.append(mean.astype(np.float32))
        counts.append(cnt.astype(np.int32))
        keys.append(uniq)
    res = (outs,) + ((counts,) if return_counts else ()) + ((keys,) if return_keys else ())
    return res[0] if len(res) == 1 else res


def normalise_submaps_host(clouds: Sequence) -> List[np.ndarray]:
    """`normalise_pcl` without padding in numpy float64 (see the module docstring) -> list of (k_i, 3) float32 arrays."""
    arrays = [np.asarray(c.cpu() if isinstance(c, torch.Tensor) else c, dtype=np.float32).reshape(-1, 3) for c in clouds]
    _check_batch([a.shape[0] for a in arrays])
    outs = []
    for i, a in enumerate(arrays):
        q = a.astype(np.float64)
        with np.errstate(invalid='ignore', over='ignore'):           # non-finite input ends in one of the errors below
            c = q.mean(axis=0)
            d = np.sqrt(((q - c) ** 2).sum(axis=1)).mean()
        if not d > 0.0:
            raise _degenerate_error(i)
        scaled = (0.5 / d) * (q - c)
        kept = scaled[np.all(np.abs(scaled) <= 1.0, axis=1)]
        if kept.shape[0] < 1:
            raise _empty_error(i)
        outs.append(kept.astype(np.float32))
    return outs


# ------------------------------------------------------------------------------------------------ device route
def _device(device):
    device = torch.device(device)
    if device.type != 'cuda':
        raise _native.NativeLibraryError('the device route runs on the GPU (no CPU fallback); use the *_host functions')
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    return device


def _as_tensors(clouds):
    """the batch as (n_i, 3) fp32 tensors where they lie, checked before the device is touched"""
    ts = [torch.as_tensor(c, dtype=torch.float32).reshape(-1, 3) for c in clouds]
    _check_batch([int(t.shape[0]) for t in ts])
    return ts


def _upload(ts, device):
    """one concatenated (P, 3) fp32 device tensor and the (B + 1,) offsets on both sides"""
    sizes = [int(t.shape[0]) for t in ts]
    off_host = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    if all(not t.is_cuda for t in ts):
        pts = torch.cat(ts).to(device, non_blocking=True).contiguous()           # one upload
    else:
        pts = torch.cat([t.to(device, non_blocking=True) for t in ts]).contiguous()
    return pts, torch.from_numpy(off_host).to(device, non_blocking=True), off_host


def _downsample_launch(pts, off, batch, v, return_counts, return_keys):
    """keys, sort, reduce: everything stays on the device"""
    keys, span_flags = ops.voxel_keys(pts, off, v)
    sorted_keys, perm = torch.sort(keys, stable=True)
    out, out_off, counts, okeys = ops.voxel_reduce(sorted_keys, perm, pts, batch, return_counts, return_keys)
    return out, out_off, span_flags, counts, okeys


def voxel_downsample(clouds: Sequence, voxel_size: float, device='cuda', return_counts: bool = False,
                     return_keys: bool = False):
    """List of raw (n_i, 3) clouds (numpy / torch) -> list of (m_i, 3) float32 device tensors, one point per occupied voxel
    in ascending (ix, iy, iz) (module docstring).  `return_counts`: also the number of members of every output point
    (list of (m_i,) int32 tensors); `return_keys`: also its cell as ix << 32 | iy << 16 | iz (list of (m_i,) int64).
    `ValueError` for a bad `voxel_size`, more than 32 767 clouds, an empty cloud, or -- naming the first such cloud, and
    returning none -- a cloud that spans 65 536 or more voxels along an axis."""
    v = _check_voxel_size(voxel_size)
    clouds = _as_tensors(clouds)
    device = _device(device)
    if not clouds:
        return tuple([] for _ in range(1 + bool(return_counts) + bool(return_keys))) if return_counts or return_keys else []
    with torch.cuda.device(device):
        pts, off, _ = _upload(clouds, device)
        batch = off.shape[0] - 1
        out, out_off, span_flags, counts, okeys = _downsample_launch(pts, off, batch, v, return_counts, return_keys)
        host = torch.cat([span_flags.to(torch.int64), out_off]).cpu().tolist()    # the one host read: flags and offsets
    flags, starts = host[:batch], host[batch:]
    for i, f in enumerate(flags):
        if f:
            raise _span_error(i)
    res = ([out[s:e] for s, e in zip(starts[:-1], starts[1:])],)
    if return_counts:
        res += ([counts[s:e] for s, e in zip(starts[:-1], starts[1:])],)
    if return_keys:
        res += ([okeys[s:e] & ((1 << 48) - 1) for s, e in zip(starts[:-1], starts[1:])],)
    return res[0] if len(res) == 1 else res


def _raise_normalise(flags, kept):
    for i, (f, k) in enumerate(zip(flags, kept)):
        if f:
            raise _degenerate_error(i)
        if k < 1:
            raise _empty_error(i)


def normalise_submaps(clouds: Sequence, device='cuda') -> List[torch.Tensor]:
    """List of (n_i, 3) clouds -> list of (k_i, 3) float32 device tensors: the PointNetVLAD normalisation of
    `normalise_pcl` without padding (module docstring), one HIP launch for the batch.  `ValueError`, naming the cloud, when
    a cloud's mean distance to its centroid is zero (a single point) or no point is left inside [-1, 1]^3."""
    clouds = _as_tensors(clouds)
    device = _device(device)
    if not clouds:
        return []
    with torch.cuda.device(device):
        pts, off, off_host = _upload(clouds, device)
        out, counts, flags = ops.submap_normalise(pts, off)
        host = torch.cat([flags, counts]).cpu().tolist()                          # the one host read
    batch = len(off_host) - 1
    _raise_normalise(host[:batch], host[batch:])
    return [out[s:s + k] for s, k in zip(off_host.tolist(), host[batch:])]


def prepare_submaps(clouds: Sequence, voxel_size: float, normalise: bool = True, device='cuda') -> List[torch.Tensor]:
    """`voxel_downsample` then (when `normalise`) `normalise_submaps` without leaving the device: the normalisation reads
    the downsampled batch and its per-cloud offsets where the reduction left them, and flags, offsets and counts come back
    in one host read.  The result is what `prepare_clouds` takes; it equals the two calls chained bit for bit."""
    if not normalise:
        return voxel_downsample(clouds, voxel_size, device=device)
    v = _check_voxel_size(voxel_size)
    clouds = _as_tensors(clouds)
    device = _device(device)
    if not clouds:
        return []
    with torch.cuda.device(device):
        pts, off, _ = _upload(clouds, device)
        batch = off.shape[0] - 1
        down, down_off, span_flags, _, _ = _downsample_launch(pts, off, batch, v, False, False)
        out, counts, flags = ops.submap_normalise(down, down_off)
        host = torch.cat([span_flags.to(torch.int64), flags.to(torch.int64), counts.to(torch.int64), down_off]).cpu().tolist()
    for i, f in enumerate(host[:batch]):
        if f:
            raise _span_error(i)
    kept, starts = host[2 * batch:3 * batch], host[3 * batch:]
    _raise_normalise(host[batch:2 * batch], kept)
    return [out[s:s + k] for s, k in zip(starts[:-1], kept)]
