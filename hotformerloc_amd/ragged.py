"""The ragged batch under the raw-submap steps (`voxel.py`, `ground.py`, `outliers.py`): intake, upload, compaction, results.

A batch of B clouds travels as one `Packed` record -- the concatenated (P, 3) fp32 points on the device and the (B + 1,)
int64 offsets on both sides -- from the upload to the last step; a step takes a `Packed` and returns one, and only the
public functions split it into the per-cloud list.  What every step needs round its kernels is here once.

Limits: a batch holds at most `MAX_CLOUDS` = 32 767 clouds (15 bits of the voxel key, so it stays a positive int64) and no
cloud is empty; both raise `ValueError` before the device is touched.  This module imports nothing of the package but
`_native` and `ops`."""

import contextlib
import math

import numpy as np
import torch

from . import _native, ops

MAX_CLOUDS = ops.VOXEL_MAX_CLOUDS


def check_batch(sizes):
    if len(sizes) > MAX_CLOUDS:
        raise ValueError('a batch holds at most %d clouds, got %d' % (MAX_CLOUDS, len(sizes)))
    for i, n in enumerate(sizes):
        if n < 1:
            raise ValueError('cloud %d is empty' % i)


def check_positive(name: str, value, fp32: bool = False) -> float:
    """float(value), positive and finite; with `fp32` its rounding to float32 is positive and finite too"""
    v = float(value)
    if not math.isfinite(v) or v <= 0.0 or (fp32 and not (math.isfinite(float(np.float32(v))) and float(np.float32(v)) > 0.0)):
        raise ValueError('%s must be positive and finite, got %r' % (name, value))
    return v


def require_points(clouds_or_packed, step_name: str, at_least: int = 1):
    """`ValueError` naming the first cloud that `step_name` left no point, or fewer than `at_least` points"""
    sizes = clouds_or_packed.sizes() if isinstance(clouds_or_packed, Packed) else [int(c.shape[0]) for c in clouds_or_packed]
    for i, n in enumerate(sizes):
        if n < 1:
            raise ValueError('cloud %d has no point left after %s' % (i, step_name))
        if n < at_least:
            raise ValueError('cloud %d has %d points left after %s, fewer than target = %d' % (i, n, step_name, at_least))


def results(first, *optional):
    """(result, optional extras...) -> the result alone, or the tuple of the parts that are not None"""
    res = (first,) + tuple(p for p in optional if p is not None)
    return res[0] if len(res) == 1 else res


def empty_results(*asked):
    """`results` of an empty batch: [] alone, or a tuple with one more [] for every extra that was asked for"""
    return results([], *([] if a else None for a in asked))


def as_arrays(clouds):
    """the batch as contiguous (n_i, 3) float32 numpy arrays, checked"""
    arrays = [np.ascontiguousarray(np.asarray(c.cpu() if isinstance(c, torch.Tensor) else c, dtype=np.float32).reshape(-1, 3))
              for c in clouds]
    check_batch([a.shape[0] for a in arrays])
    return arrays


def as_tensors(clouds):
    """the batch as (n_i, 3) fp32 tensors where they lie, checked before the device is touched"""
    ts = [torch.as_tensor(c, dtype=torch.float32).reshape(-1, 3) for c in clouds]
    check_batch([int(t.shape[0]) for t in ts])
    return ts


def device_of(device):
    device = torch.device(device)
    if device.type != 'cuda':
        raise _native.NativeLibraryError('the device route runs on the GPU (no CPU fallback); use the *_host functions')
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    return device


class Packed:
    """A ragged batch on the device: `pts` (P, 3) fp32 (rows past `off_host[-1]` are nobody's), `off_host` the (B + 1,) int64
    numpy offsets, `off` the same on the device (uploaded when a kernel first asks for them)."""
    __slots__ = ('pts', 'off_host', '_off')

    def __init__(self, pts, off_host, off=None):
        self.pts, self.off_host, self._off = pts, off_host, off

    @property
    def off(self):
        if self._off is None:
            self._off = torch.from_numpy(self.off_host).to(self.pts.device, non_blocking=True)
        return self._off

    @property
    def batch(self) -> int:
        return len(self.off_host) - 1

    def sizes(self):
        return np.diff(self.off_host).tolist()

    def split(self, x=None, counts=None):
        """`pts`, or any per-point tensor, as the per-cloud list; with `counts` only the first counts[b] rows of cloud b"""
        x = self.pts if x is None else x
        starts = self.off_host.tolist()
        ends = starts[1:] if counts is None else [s + int(k) for s, k in zip(starts, counts)]
        return [x[s:e] for s, e in zip(starts, ends)]


def upload(ts, device) -> Packed:
    """checked tensors -> one concatenated (P, 3) fp32 device tensor and the (B + 1,) offsets"""
    off_host = np.concatenate([[0], np.cumsum([int(t.shape[0]) for t in ts])]).astype(np.int64)
    if all(not t.is_cuda for t in ts):
        pts = torch.cat(ts).to(device, non_blocking=True).contiguous()           # one upload
    else:
        pts = torch.cat([t.to(device, non_blocking=True) for t in ts]).contiguous()
    return Packed(pts, off_host)


@contextlib.contextmanager
def intake(clouds, device, check=None, upload=upload):
    """What a public device function opens with: the batch checked (`check(sizes)` is a step's own check of the cloud
    sizes) before the device is touched, then uploaded by `upload`, the device current inside the block; None for an empty
    batch."""
    ts = as_tensors(clouds)
    if check is not None:
        check([int(t.shape[0]) for t in ts])
    device = device_of(device)
    if not ts:
        yield None
        return
    with torch.cuda.device(device):
        yield upload(ts, device)


def bounds_host(packed: Packed):
    """(bounds (B, 6) int32 on the device as `hfl_voxel_occupancy` takes them, (B, 6) float32 numpy min x, y, z, max x, y, z)"""
    bounds = ops.voxel_bounds(packed.pts, packed.off)
    return bounds, ops.decode_voxel_bounds(bounds.cpu().numpy())                  # the one host read of the bounds


def compact_offsets(index: np.ndarray, off_host: np.ndarray) -> np.ndarray:
    """the ascending indices of the kept rows and the old offsets -> the new offsets: the kept rows before every cloud's
    first point"""
    return np.searchsorted(index, off_host).astype(np.int64)


def compact(packed: Packed, keep) -> Packed:
    """the rows of `packed` where the (P,) mask `keep` is not zero, in input order; a cloud may come back empty"""
    index = torch.nonzero(keep).reshape(-1)                                       # ascending: the order of the input
    rows = ops.voxel_gather_rows(packed.pts, index)
    return Packed(rows, compact_offsets(index.cpu().numpy(), packed.off_host))
