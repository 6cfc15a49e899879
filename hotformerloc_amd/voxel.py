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

Fixed-size clouds (the Oxford / CS-Campus3D format, `target` = 4096 points; `postprocess_submaps.py --downsample_type
pnvlad|random --downsample_target N --normalise`):

    pnvlad   `processing_utils.pnvlad_down_sample`: v = 3.001, then v -= 0.01 until a voxel grid of size v has at least
             `target` occupied cells, then v += 0.01 / 5 until it has at most `target`; the cell means at that v, then
             `target - m` raw rows drawn by `np.random.default_rng(seed)`, a fresh generator per cloud.  The candidate sizes
             are formed on the host in float64 by the same repeated operations.  Counts are not monotone in v: the sequence
             is followed, never bisected.
    random   `random_down_sample`: `target` raw rows drawn with replacement by a fresh generator per cloud.
    padding  `normalise_pcl` with `downsample_number` set: after the normalisation above, raw rows are drawn, sent through
             the same c and s, kept when every |q'| <= 1 and appended, until the cloud has `target` rows; the generator
             continues across the iterations.  At most `PAD_MAX_ITERATIONS` iterations (the reference would loop for ever
             on a raw cloud that has no row inside), then `ValueError`.

Device route of the search: `hfl_voxel_bounds` once and one host read of the (B, 6) bounds; then rounds.  In a round the
host writes down the next `PNVLAD_K_ONE` = 64 phase-one (or `PNVLAD_K_TWO` = 8 phase-two, doubled per round up to 64)
candidates of every unfinished cloud with their grid dimensions, `hfl_voxel_occupancy` counts the occupied cells of all of them in one launch pair (a
bitmap per candidate, integer OR atomics, a popcount), and the counts come back in one read.  Launches of a round share a
bitmap budget of `OCCUPANCY_BUDGET_BYTES` = 64 MiB each; a single candidate whose bitmap is larger than the budget is
counted by the keys -> sort -> reduce route instead.  Random indices are drawn on the host (`rng.choice(points, size=k)`
and `points[rng.choice(len(points), size=k)]` draw the same rows) and gathered on the device (`hfl_voxel_gather_rows`);
padded rows are transformed by `hfl_submap_normalise_rows`, which shares its device code with `hfl_submap_normalise`.

Ground removal (`postprocess_submaps.py --remove_ground`, the step before the downsample) is `ground.py`; the entry points
`prepare_submaps` and `prepare_submaps_fixed` run it first with `remove_ground=True`.  The raw cleaning in front of it -- the
radius trim and the statistical outlier filter -- is `outliers.py`; the same entry points run it before everything else with
`radius_max=` / `remove_outliers=True`.  The order of the whole chain is written once, in `submap_chain`; the batch plumbing
under all three modules is `ragged.py`."""

from typing import List, Sequence

import numpy as np
import torch

from . import ground, ops, outliers, ragged
from .ragged import MAX_CLOUDS

MAX_CELLS = ops.VOXEL_MAX_CELLS


def _check_voxel_size(voxel_size) -> float:
    return ragged.check_positive('voxel_size', voxel_size)


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
    arrays = ragged.as_arrays(clouds)
    outs, counts, keys = [], [], []
    for i, a in enumerate(arrays):
        mean, cnt, uniq = _cell_means(a, v, i)
        outs.append(mean.astype(np.float32))
        counts.append(cnt.astype(np.int32))
        keys.append(uniq)
    return ragged.results(outs, counts if return_counts else None, keys if return_keys else None)


def _normalise_host(a: np.ndarray, index: int):
    """one cloud -> (the kept rows of s (q - c) in float64, c, s)"""
    q = a.astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):               # non-finite input ends in one of the errors below
        c = q.mean(axis=0)
        d = np.sqrt(((q - c) ** 2).sum(axis=1)).mean()
    if not d > 0.0:
        raise _degenerate_error(index)
    scaled = (0.5 / d) * (q - c)
    kept = scaled[np.all(np.abs(scaled) <= 1.0, axis=1)]
    if kept.shape[0] < 1:
        raise _empty_error(index)
    return kept, c, 0.5 / d


def normalise_submaps_host(clouds: Sequence) -> List[np.ndarray]:
    """`normalise_pcl` without padding in numpy float64 (see the module docstring) -> list of (k_i, 3) float32 arrays."""
    return [_normalise_host(a, i)[0].astype(np.float32) for i, a in enumerate(ragged.as_arrays(clouds))]


# ------------------------------------------------------------------------------------------------ device route
_upload = ragged.upload            # under the name the tests replace to prove that an error came before any upload


def _intake(clouds, device, check=None):
    return ragged.intake(clouds, device, check, _upload)


def _downsample_launch(pts, off, batch, v, return_counts, return_keys):
    """keys, sort, reduce: everything stays on the device"""
    keys, span_flags = ops.voxel_keys(pts, off, v)
    sorted_keys, perm = torch.sort(keys, stable=True)
    out, out_off, counts, okeys = ops.voxel_reduce(sorted_keys, perm, pts, batch, return_counts, return_keys)
    return out, out_off, span_flags, counts, okeys


def _raise_normalise(flags, kept):
    for i, (f, k) in enumerate(zip(flags, kept)):
        if f:
            raise _degenerate_error(i)
        if k < 1:
            raise _empty_error(i)


def _downsample_packed(packed, v, normalise: bool = False, return_counts: bool = False, return_keys: bool = False):
    """The voxel grid on a packed batch and, with `normalise`, the normalisation reading the downsampled rows and their
    offsets where the reduction left them; span flags, offsets, and the normalisation's flags and counts come back in the
    one host read.  -> (the rows as a `ragged.Packed`, kept (the rows of every cloud that the normalisation kept from its
    first row on, or None), cell counts or None, keys or None)"""
    batch = packed.batch
    out, out_off, span_flags, counts, okeys = _downsample_launch(packed.pts, packed.off, batch, v, return_counts, return_keys)
    parts = [span_flags.to(torch.int64), out_off]
    if normalise:
        out, kept, flags = ops.submap_normalise(out, out_off)
        parts += [flags.to(torch.int64), kept.to(torch.int64)]
    host = torch.cat(parts).cpu().tolist()                                        # the one host read
    for i, f in enumerate(host[:batch]):
        if f:
            raise _span_error(i)
    kept = None
    if normalise:
        kept = host[3 * batch + 1:]
        _raise_normalise(host[2 * batch + 1:3 * batch + 1], kept)
    return ragged.Packed(out, np.asarray(host[batch:2 * batch + 1], dtype=np.int64), out_off), kept, counts, okeys


def voxel_downsample(clouds: Sequence, voxel_size: float, device='cuda', return_counts: bool = False,
                     return_keys: bool = False):
    """List of raw (n_i, 3) clouds (numpy / torch) -> list of (m_i, 3) float32 device tensors, one point per occupied voxel
    in ascending (ix, iy, iz) (module docstring).  `return_counts`: also the number of members of every output point
    (list of (m_i,) int32 tensors); `return_keys`: also its cell as ix << 32 | iy << 16 | iz (list of (m_i,) int64).
    `ValueError` for a bad `voxel_size`, more than 32 767 clouds, an empty cloud, or -- naming the first such cloud, and
    returning none -- a cloud that spans 65 536 or more voxels along an axis."""
    v = _check_voxel_size(voxel_size)
    with _intake(clouds, device) as packed:
        if packed is None:
            return ragged.empty_results(return_counts, return_keys)
        down, _, counts, okeys = _downsample_packed(packed, v, False, return_counts, return_keys)
        return ragged.results(down.split(), down.split(counts) if return_counts else None,
                              down.split(okeys & ((1 << 48) - 1)) if return_keys else None)


def _normalise_packed(packed):
    """`hfl_submap_normalise` and its one host read -> (out (P, 3): cloud b's kept rows from row `off_host[b]` on, kept (B,))"""
    out, counts, flags = ops.submap_normalise(packed.pts, packed.off)
    host = torch.cat([flags, counts]).cpu().tolist()                              # the one host read
    _raise_normalise(host[:packed.batch], host[packed.batch:])
    return out, host[packed.batch:]


def normalise_submaps(clouds: Sequence, device='cuda') -> List[torch.Tensor]:
    """List of (n_i, 3) clouds -> list of (k_i, 3) float32 device tensors: the PointNetVLAD normalisation of
    `normalise_pcl` without padding (module docstring), one HIP launch for the batch.  `ValueError`, naming the cloud, when
    a cloud's mean distance to its centroid is zero (a single point) or no point is left inside [-1, 1]^3."""
    with _intake(clouds, device) as packed:
        if packed is None:
            return []
        out, kept = _normalise_packed(packed)
        return packed.split(out, kept)


def submap_chain(clouds: Sequence, device='cuda', *, radius_max=None, remove_outliers: bool = False, outlier_params=None,
                 remove_ground: bool = False, ground_params=None, voxel_size=None, target=None, downsample: str = 'pnvlad',
                 normalise: bool = False, seed=42, at_least=None) -> List[torch.Tensor]:
    """The raw-submap chain, the one place its order is written: the radius trim (`radius_max`), outlier removal
    (`remove_outliers`, `outlier_params`), ground removal (`remove_ground`, `ground_params`), then the voxel grid
    (`voxel_size`) or the fixed-size downsample (`target`, `downsample`, `seed`), then the normalisation (`normalise`: padded
    to `target` rows from the filtered cloud on the fixed-size path).  Every step is optional; with none the clouds come back
    as they are.  The batch is uploaded once and stays packed on the device (`ragged.Packed`); the result equals the public
    functions chained through lists bit for bit.  Parameters and emptiness are checked before the device is touched.  After a
    filter `ValueError` names the first cloud, by its index in `clouds`, with no point left or with fewer than `at_least`
    points: by default `target` where the 'pnvlad' search follows and after ground removal on the fixed-size path, else 1."""
    v = None if voxel_size is None else _check_voxel_size(voxel_size)
    if target is not None:
        if downsample not in ('pnvlad', 'random'):
            raise ValueError("downsample must be 'pnvlad' or 'random', got %r" % (downsample,))
        target = _check_target(target)
    r = None if radius_max is None else ragged.check_positive('radius_max', radius_max)
    outlier_params = outliers.check_params(**(outlier_params or {})) if remove_outliers else None
    cloth = ground.ClothParams(**(ground_params or {})) if remove_ground else None
    filters = r is not None or remove_outliers or remove_ground
    if not (filters or v is not None or target is not None or normalise):
        return clouds                                                             # no step asked for: nothing is touched
    cleaned_few = ground_few = at_least
    if at_least is None:
        cleaned_few = target if target is not None and downsample == 'pnvlad' else 1
        ground_few = 1 if target is None else target
    ts = ragged.as_tensors(clouds)
    if target is not None and downsample == 'pnvlad' and not filters:
        _check_enough_points([int(t.shape[0]) for t in ts], target)
    device = ragged.device_of(device)
    if not ts:
        return []
    with torch.cuda.device(device):
        packed = _upload(ts, device)
        if r is not None:
            packed = outliers.trim_radius_packed(packed, r)[0]
            ragged.require_points(packed, 'the radius trim', cleaned_few)
        if remove_outliers:
            packed = outliers.remove_outliers_packed(packed, *outlier_params)[0]
            ragged.require_points(packed, 'outlier removal', cleaned_few)
        if remove_ground:
            packed = ground.remove_ground_packed(packed, cloth)[0]
            ragged.require_points(packed, 'ground removal', ground_few)
        if v is not None:
            packed, kept, _, _ = _downsample_packed(packed, v, normalise)
            return packed.split(counts=kept)
        if target is not None:
            raw = packed
            packed = _pnvlad_packed(raw, target, seed)[0] if downsample == 'pnvlad' else _random_packed(raw, target, seed)
            return _normalise_padded_packed(packed, raw, target, seed) if normalise else packed.split()
        return packed.split(*_normalise_packed(packed)) if normalise else packed.split()


def prepare_submaps(clouds: Sequence, voxel_size: float, normalise: bool = True, device='cuda', *, remove_ground: bool = False,
                    ground_params=None, radius_max=None, remove_outliers: bool = False,
                    outlier_params=None) -> List[torch.Tensor]:
    """`submap_chain` with the voxel grid: `voxel_downsample` then (when `normalise`) `normalise_submaps` without leaving
    the device, flags, offsets and counts coming back in one host read.  The result is what `prepare_clouds` takes.  With
    `remove_ground` the raw batch first goes through `ground.remove_ground(**ground_params)` (the documented CS-Wild-Places
    order), with `radius_max` and / or `remove_outliers` through `trim_radius` and `remove_outliers(**outlier_params)`
    before that.  The result equals the public calls chained bit for bit; a cloud a filter leaves no point raises
    `ValueError` naming it."""
    return submap_chain(clouds, device, radius_max=radius_max, remove_outliers=remove_outliers, outlier_params=outlier_params,
                        remove_ground=remove_ground, ground_params=ground_params, voxel_size=_check_voxel_size(voxel_size),
                        normalise=normalise)


# ================================================================================================ fixed-size clouds
PNVLAD_START = 3.001                   # processing_utils.pnvlad_down_sample
PNVLAD_STEP = 0.01                     # VOXEL_STEP
PNVLAD_K_ONE = 64                      # candidates per unfinished cloud and round while v steps down by 0.01 ...
PNVLAD_K_TWO = 8                       # ... and while it steps back up by 0.002 (five steps undo one phase-one step);
                                       # doubled every round a cloud stays in phase two, up to PNVLAD_K_ONE
OCCUPANCY_BUDGET_BYTES = 64 << 20      # bitmap bytes of one hfl_voxel_occupancy call
PAD_MAX_ITERATIONS = 64                # of the padding loop of normalise_pcl


def _check_target(target) -> int:
    t = int(target)
    if t < 1 or t != target:
        raise ValueError('target must be a positive integer, got %r' % (target,))
    return t


def _check_enough_points(sizes, target):
    for i, n in enumerate(sizes):
        if n < target:
            raise ValueError('cloud %d has %d points, fewer than target = %d: no voxel size gives %d occupied cells'
                             % (i, n, target, target))


def _unreachable_error(i: int, target: int, why: str):
    return ValueError('cloud %d never reaches %d occupied voxels: %s' % (i, target, why))


def _pad_indices(seed, n: int, k: int) -> np.ndarray:
    """`rng.choice(points, size=k)` of a fresh generator, as row indices"""
    return np.random.default_rng(seed).choice(n, size=k).astype(np.int64)


# ------------------------------------------------------------------------------------------------ host route
def _host_counter(cloud: np.ndarray, index: int):
    """v -> the number of cells the cloud occupies at voxel size v (`_cell_means` without the means)"""
    p = cloud.astype(np.float64)
    low = p.min(axis=0)

    def count(v: float) -> int:
        cell = np.floor((p - (low - 0.5 * v)) / v)
        if not cell.max() < MAX_CELLS:
            raise _span_error(index)
        cell = cell.astype(np.int64)
        return int(np.unique((cell[:, 0] << 32) | (cell[:, 1] << 16) | cell[:, 2]).size)
    return count


def voxel_occupancy_host(clouds: Sequence, sizes: Sequence[float]) -> np.ndarray:
    """(B, S) int32: the number of occupied cells of every cloud at every voxel size, i.e.
    `len(voxel_downsample_host([cloud], v)[0])`, in numpy float64."""
    vs = [_check_voxel_size(v) for v in sizes]
    arrays = ragged.as_arrays(clouds)
    out = np.zeros((len(arrays), len(vs)), np.int32)
    for i, a in enumerate(arrays):
        count = _host_counter(a, i)
        for j, v in enumerate(vs):
            out[i, j] = count(v)
    return out


def pnvlad_search_host(clouds: Sequence, target: int = 4096) -> List[dict]:
    """The voxel-size search of `pnvlad_down_sample`, probe by probe as the reference runs it.  Per cloud a dict: 'voxel_size'
    (the float64 the search ends on), 'count' (occupied cells there, <= target), 'trace' (every (v, count) probed, in
    order), 'phase_one_steps', 'phase_two_steps'."""
    target = _check_target(target)
    arrays = ragged.as_arrays(clouds)
    _check_enough_points([a.shape[0] for a in arrays], target)
    res = []
    for i, a in enumerate(arrays):
        count = _host_counter(a, i)
        v = PNVLAD_START
        n = count(v)
        trace, one, two = [(v, n)], 0, 0
        while n < target:
            v -= PNVLAD_STEP
            one += 1
            if v <= 0:
                raise _unreachable_error(i, target, 'the voxel size reached zero')
            try:
                n = count(v)
            except ValueError:
                raise _unreachable_error(i, target, 'at voxel size %.3f it spans more than %d cells along an axis'
                                         % (v, MAX_CELLS)) from None
            trace.append((v, n))
        while n > target:
            v += PNVLAD_STEP / 5
            two += 1
            n = count(v)
            trace.append((v, n))
        res.append({'voxel_size': v, 'count': n, 'trace': trace, 'phase_one_steps': one, 'phase_two_steps': two})
    return res


def pnvlad_downsample_host(clouds: Sequence, target: int = 4096, seed=42, return_voxel_sizes: bool = False):
    """`pnvlad_down_sample` per cloud in numpy float64 (module docstring) -> list of (target, 3) float32 arrays: the cell
    means at the voxel size the search ends on, in ascending (ix, iy, iz), then `target - m` raw rows drawn by a fresh
    `default_rng(seed)`.  With `return_voxel_sizes` also the list of those sizes."""
    arrays = ragged.as_arrays(clouds)
    found = pnvlad_search_host(arrays, target)
    outs = []
    for i, (a, f) in enumerate(zip(arrays, found)):
        mean, _, _ = _cell_means(a, f['voxel_size'], i)
        idx = _pad_indices(seed, a.shape[0], target - mean.shape[0])
        outs.append(np.concatenate([mean.astype(np.float32), a[idx]]))
    return (outs, [f['voxel_size'] for f in found]) if return_voxel_sizes else outs


def random_downsample_host(clouds: Sequence, target: int, seed=42) -> List[np.ndarray]:
    """`random_down_sample`: `target` rows of every cloud drawn with replacement by a fresh `default_rng(seed)`."""
    target = _check_target(target)
    arrays = ragged.as_arrays(clouds)
    return [a[_pad_indices(seed, a.shape[0], target)] for a in arrays]


def _padding_error(i: int, target: int):
    return ValueError('cloud %d is still short of %d points after %d rounds of padding: hardly any raw point lies inside '
                      '[-1, 1]^3 after normalisation' % (i, target, PAD_MAX_ITERATIONS))


def _too_many_error(i: int, kept: int, target: int):
    return ValueError('cloud %d keeps %d points after normalisation, more than target = %d' % (i, kept, target))


def normalise_submaps_padded_host(downsampled: Sequence, raw: Sequence, target: int, seed=42) -> List[np.ndarray]:
    """`normalise_pcl` with `downsample_number = target` in numpy float64 -> list of (target, 3) float32 arrays: the rows of
    `normalise_submaps_host(downsampled)`, then rows of `raw` drawn by `default_rng(seed)` (one generator per cloud, carried
    across the iterations), sent through the same centroid and scale and kept when every |q'| <= 1."""
    target = _check_target(target)
    down, raws = ragged.as_arrays(downsampled), ragged.as_arrays(raw)
    if len(down) != len(raws):
        raise ValueError('%d downsampled clouds but %d raw clouds' % (len(down), len(raws)))
    outs = []
    for i, (a, r) in enumerate(zip(down, raws)):
        kept, c, scale = _normalise_host(a, i)
        if kept.shape[0] > target:
            raise _too_many_error(i, kept.shape[0], target)
        rng = np.random.default_rng(seed)
        r64 = r.astype(np.float64)
        extra, added, rounds, parts = target - kept.shape[0], 0, 0, [kept]
        while kept.shape[0] + added < target:
            if rounds == PAD_MAX_ITERATIONS:
                raise _padding_error(i, target)
            rounds += 1
            rows = scale * (r64[rng.choice(r.shape[0], size=extra - added)] - c)
            rows = rows[np.all(np.abs(rows) <= 1.0, axis=1)]
            added += rows.shape[0]
            parts.append(rows)
        outs.append(np.concatenate(parts).astype(np.float32))
    return outs


# ------------------------------------------------------------------------------------------------ device route
def grid_dims(lo_hi: np.ndarray, v: float):
    """(nx, ny, nz) of a cloud with bounds `lo_hi` = (min x, y, z, max x, y, z) fp32 at voxel size v, by the formula of the
    kernels, or None when it spans more than MAX_CELLS cells along an axis"""
    low, high = lo_hi[:3].astype(np.float64), lo_hi[3:].astype(np.float64)
    top = np.floor((high - (low - 0.5 * v)) / v)
    if not top.max() < MAX_CELLS:
        return None
    return tuple(int(t) + 1 for t in top)


def _count_by_sort(pts, start: int, end: int, v: float):
    """one cloud's occupied cells at v through keys -> sort -> reduce, as a (1,) int64 device tensor"""
    cloud = pts[start:end]
    if (start * 12) % 16:
        cloud = cloud.clone()                                                     # the kernels load 16 bytes at a time
    off = torch.tensor([0, end - start], dtype=torch.int64, device=pts.device)
    _, out_off, _, _, _ = _downsample_launch(cloud, off, 1, v, False, False)
    return out_off[1:] - out_off[:1]


def _count_candidates(packed, bounds, cands, budget_bytes: int, stats=None) -> List[int]:
    """cands: list of (cloud, v, (nx, ny, nz)) -> their occupied-cell counts, one host read.  Candidates are packed into
    `hfl_voxel_occupancy` calls of at most `budget_bytes` of bitmaps; one whose own bitmap is larger goes to the sort route."""
    pts, off, off_host = packed.pts, packed.off, packed.off_host
    budget_words = max(min(int(budget_bytes) // 4, ops.VOXEL_OCC_MAX_WORDS), 1)
    biggest = int(np.diff(off_host).max())
    parts, order, held = [], [], []
    table, words, members = [], 0, []

    def launch():
        nonlocal table, words, members
        if table:
            arr = np.array(table, dtype=np.dtype(ops.VOXEL_CANDIDATE_DTYPE))
            held.append(ops.voxel_occupancy(pts, off, bounds, arr, words, biggest))     # alive until the host read
            parts.append(held[-1].to(torch.int64))
            order.extend(members)
            if stats is not None:
                stats['occupancy_calls'] = stats.get('occupancy_calls', 0) + 1
        table, words, members = [], 0, []

    for k, (c, v, (nx, ny, nz)) in enumerate(cands):
        w = (nx * ny * nz + 31) // 32
        if w > budget_words:
            parts.append(_count_by_sort(pts, int(off_host[c]), int(off_host[c + 1]), v))
            order.append(k)
            if stats is not None:
                stats['sort_fallbacks'] = stats.get('sort_fallbacks', 0) + 1
            continue
        if words + w > budget_words or len(table) == ops.VOXEL_OCC_MAX_CANDIDATES:
            launch()
        table.append((c, nx, ny, nz, v, words))
        members.append(k)
        words += w
    launch()
    got = torch.cat(parts).cpu().tolist() if parts else []                        # the one host read
    counts = [0] * len(cands)
    for k, n in zip(order, got):
        counts[k] = int(n)
    return counts


def voxel_occupancy(clouds: Sequence, sizes: Sequence[float], device='cuda', budget_bytes: int = OCCUPANCY_BUDGET_BYTES):
    """(B, S) int32 device tensor: the number of occupied cells of every cloud at every voxel size -- what
    `voxel_downsample` would return rows for -- counted by `hfl_voxel_occupancy` without a sort.  `budget_bytes` bounds the
    bitmaps of one call (module docstring).  `ValueError` as `voxel_downsample`, the span limit included."""
    vs = [_check_voxel_size(v) for v in sizes]
    ts = ragged.as_tensors(clouds)
    if not ts or not vs:
        return torch.zeros((len(ts), len(vs)), dtype=torch.int32, device=ragged.device_of(device))
    with _intake(ts, device) as packed:
        bounds, lo_hi = ragged.bounds_host(packed)
        cands = []
        for c in range(packed.batch):
            for v in vs:
                dims = grid_dims(lo_hi[c], v)
                if dims is None:
                    raise _span_error(c)
                cands.append((c, v, dims))
        counts = _count_candidates(packed, bounds, cands, budget_bytes)
        return torch.tensor(counts, dtype=torch.int32).reshape(packed.batch, len(vs)).to(packed.pts.device)


def _pnvlad_search_device(packed, target: int, budget_bytes: int):
    """the search of `pnvlad_search_host` with the counts from the device, K candidates per cloud and round -> (per-cloud
    dicts as `pnvlad_search_host` returns them, stats: 'rounds', 'candidates' evaluated per cloud, calls and fallbacks)"""
    batch = packed.batch
    bounds, lo_hi = ragged.bounds_host(packed)
    state = [{'phase': 1, 'v': None, 'trace': [], 'one': 0, 'two': 0, 'count': None, 'k_two': PNVLAD_K_TWO} for _ in range(batch)]
    stats = {'rounds': 0, 'candidates': [0] * batch}
    while any(st['phase'] for st in state):
        cands, plan = [], []
        for c, st in enumerate(state):
            if not st['phase']:
                continue
            vs, end, v = [], None, st['v']
            ahead = PNVLAD_K_ONE
            if st['phase'] == 2:
                ahead, st['k_two'] = st['k_two'], min(2 * st['k_two'], PNVLAD_K_ONE)
            for _ in range(ahead):
                if st['phase'] == 2:
                    v += PNVLAD_STEP / 5
                elif v is None:
                    v = PNVLAD_START
                else:
                    v -= PNVLAD_STEP
                    if v <= 0:
                        end = 'the voxel size reached zero'
                        break
                dims = grid_dims(lo_hi[c], v)
                if dims is None:
                    end = 'at voxel size %.3f it spans more than %d cells along an axis' % (v, MAX_CELLS)
                    break
                vs.append(v)
                cands.append((c, v, dims))
            plan.append((c, vs, end))
        counts = iter(_count_candidates(packed, bounds, cands, budget_bytes, stats))
        stats['rounds'] += 1
        for c, vs, end in plan:
            st = state[c]
            stats['candidates'][c] += len(vs)
            got = [next(counts) for _ in vs]
            for v, n in zip(vs, got):
                if st['phase'] == 1:
                    st['one'] += bool(st['trace'])
                    st['trace'].append((v, n))
                    st['v'] = v
                    if n >= target:
                        st['phase'], st['count'] = (2 if n > target else 0), n
                        break                                                     # the rest was speculation
                else:
                    st['two'] += 1
                    st['trace'].append((v, n))
                    st['v'] = v
                    if n <= target:
                        st['phase'], st['count'] = 0, n
                        break
            else:
                if end is not None:
                    raise _unreachable_error(c, target, end)
    found = [{'voxel_size': st['v'], 'count': st['count'], 'trace': st['trace'], 'phase_one_steps': st['one'],
              'phase_two_steps': st['two']} for st in state]
    return found, stats


def pnvlad_search(clouds: Sequence, target: int = 4096, device='cuda', budget_bytes: int = OCCUPANCY_BUDGET_BYTES,
                  return_stats: bool = False):
    """`pnvlad_search_host` with the occupied cells counted on the device (module docstring): the same per-cloud dicts, the
    trace holding the probes the reference would have made (not the speculative ones past a stop).  With `return_stats` also
    {'rounds', 'candidates' (evaluated per cloud, speculation included), 'occupancy_calls', 'sort_fallbacks'}."""
    target = _check_target(target)
    with _intake(clouds, device, lambda sizes: _check_enough_points(sizes, target)) as packed:
        if packed is None:
            return ([], {'rounds': 0, 'candidates': []}) if return_stats else []
        found, stats = _pnvlad_search_device(packed, target, budget_bytes)
    return (found, stats) if return_stats else found


def _pnvlad_packed(packed, target: int, seed, budget_bytes: int = OCCUPANCY_BUDGET_BYTES):
    """the search, the cell means at the size it ends on and the raw rows that fill a cloud up to `target` -> (the batch of
    B x `target` rows as a `ragged.Packed`, the per-cloud dicts of the search)"""
    pts, off_host, device = packed.pts, packed.off_host, packed.pts.device
    found, _ = _pnvlad_search_device(packed, target, budget_bytes)
    means, index = [], []
    for c, f in enumerate(found):
        s, e = int(off_host[c]), int(off_host[c + 1])
        cloud = pts[s:e].clone() if (s * 12) % 16 else pts[s:e]                   # the kernels load 16 bytes at a time
        one = torch.tensor([0, e - s], dtype=torch.int64, device=device)
        out, _, _, _, _ = _downsample_launch(cloud, one, 1, f['voxel_size'], False, False)
        means.append(out[:f['count']])                                            # the count is the number of output rows
        index.append(s + _pad_indices(seed, e - s, target - f['count']))
    lens = [len(i) for i in index]
    rows = ops.voxel_gather_rows(pts, torch.from_numpy(np.concatenate(index)).to(device)) if sum(lens) else None
    parts, at = [], 0
    for m, k in zip(means, lens):
        parts += [m, rows[at:at + k]] if k else [m]
        at += k
    return _fixed(torch.cat(parts), packed.batch, target), found


def _fixed(rows, batch: int, target: int):
    return ragged.Packed(rows, np.arange(batch + 1, dtype=np.int64) * target)


def pnvlad_downsample(clouds: Sequence, target: int = 4096, seed=42, device='cuda', return_voxel_sizes: bool = False,
                      budget_bytes: int = OCCUPANCY_BUDGET_BYTES):
    """`pnvlad_down_sample` for a ragged batch on the device -> list of (target, 3) float32 device tensors: the cell means
    at the voxel size the reference's search ends on (the rows `voxel_downsample([cloud], v)` returns, bit for bit), then
    `target - m` raw rows at the indices a fresh `default_rng(seed)` draws per cloud.  With `return_voxel_sizes` also the
    list of float64 sizes.  `ValueError`, naming the cloud: fewer than `target` points (raised before any launch), or no
    voxel size down to zero / to the 65 535-cell span limit that gives `target` occupied cells."""
    target = _check_target(target)
    with _intake(clouds, device, lambda sizes: _check_enough_points(sizes, target)) as packed:
        if packed is None:
            return ragged.empty_results(return_voxel_sizes)
        down, found = _pnvlad_packed(packed, target, seed, budget_bytes)
        return ragged.results(down.split(), [f['voxel_size'] for f in found] if return_voxel_sizes else None)


def _random_packed(packed, target: int, seed):
    """`target` rows of every cloud at the indices drawn on the host, one gather launch -> a `ragged.Packed`"""
    index = np.concatenate([int(s) + _pad_indices(seed, int(n), target) for s, n in zip(packed.off_host, packed.sizes())])
    rows = ops.voxel_gather_rows(packed.pts, torch.from_numpy(index).to(packed.pts.device))
    return _fixed(rows, packed.batch, target)


def random_downsample(clouds: Sequence, target: int, seed=42, device='cuda') -> List[torch.Tensor]:
    """`random_down_sample` for a batch -> list of (target, 3) float32 device tensors: rows drawn with replacement by a
    fresh `default_rng(seed)` per cloud (indices on the host, one gather launch on the device)."""
    target = _check_target(target)
    with _intake(clouds, device) as packed:
        return [] if packed is None else _random_packed(packed, target, seed).split()


def _normalise_padded_packed(down, raw, target: int, seed) -> List[torch.Tensor]:
    """the normalisation of the packed batch `down` and its padding from the packed batch `raw` -> the per-cloud list"""
    batch, device = down.batch, down.pts.device
    out, kept = _normalise_packed(down)
    for i, k in enumerate(kept):
        if k > target:
            raise _too_many_error(i, k, target)
    rngs = [np.random.default_rng(seed) for _ in range(batch)]
    n_raw = raw.sizes()
    added, parts = [0] * batch, [[c] for c in down.split(out, kept)]
    for _ in range(PAD_MAX_ITERATIONS):
        want = [target - k - a for k, a in zip(kept, added)]                      # extra - added of the reference
        if not any(want):
            break
        index = [rngs[i].choice(n_raw[i], size=w).astype(np.int64) if w else np.zeros(0, np.int64)
                 for i, w in enumerate(want)]
        row_off = np.concatenate([[0], np.cumsum(want)]).astype(np.int64)
        rows, keep = ops.submap_normalise_rows(down.pts, down.off, raw.pts, raw.off,
                                               torch.from_numpy(np.concatenate(index)).to(device),
                                               torch.from_numpy(row_off).to(device))
        mask = keep.cpu().numpy() != 0                                            # the one host read of the iteration
        picked = ops.voxel_gather_rows(rows, torch.from_numpy(np.flatnonzero(mask)).to(device))
        at = 0
        for i in range(batch):
            n = int(mask[row_off[i]:row_off[i + 1]].sum())
            if n:
                parts[i].append(picked[at:at + n])
            at += n
            added[i] += n
    else:
        if any(k + a < target for k, a in zip(kept, added)):
            raise _padding_error([k + a < target for k, a in zip(kept, added)].index(True), target)
    return [torch.cat(p) if len(p) > 1 else p[0].clone() for p in parts]


def normalise_submaps_padded(downsampled: Sequence, raw: Sequence, target: int, seed=42, device='cuda') -> List[torch.Tensor]:
    """`normalise_pcl` with `downsample_number = target` for a batch -> list of (target, 3) float32 device tensors.  The
    first rows are `normalise_submaps(downsampled)` bit for bit; the rest are rows of `raw` drawn by `default_rng(seed)`
    (one generator per cloud, carried across the iterations), transformed by the same device code with the same centroid
    and scale, and kept when every |q'| <= 1.  One host read for the normalisation and one per padding iteration.
    `ValueError` as `normalise_submaps`, and when a cloud keeps more than `target` rows or the padding does not end."""
    target = _check_target(target)
    down, raws = ragged.as_tensors(downsampled), ragged.as_tensors(raw)
    if len(down) != len(raws):
        raise ValueError('%d downsampled clouds but %d raw clouds' % (len(down), len(raws)))
    with _intake(down, device) as dpacked, _intake(raws, device) as rpacked:
        return [] if dpacked is None else _normalise_padded_packed(dpacked, rpacked, target, seed)


def prepare_submaps_fixed(clouds: Sequence, target: int = 4096, downsample: str = 'pnvlad', normalise: bool = True, seed=42,
                          device='cuda', *, remove_ground: bool = False, ground_params=None, radius_max=None,
                          remove_outliers: bool = False, outlier_params=None) -> List[torch.Tensor]:
    """`submap_chain` with fixed-size clouds of `target` points (the Oxford / CS-Campus3D format): `pnvlad_downsample` or
    `random_downsample`, then (when `normalise`) `normalise_submaps_padded` against the raw clouds; the result equals the
    chained calls bit for bit.  With `remove_ground`, `radius_max` and / or `remove_outliers` the batch is filtered first as
    in `prepare_submaps`; the filtered cloud is then also the raw cloud the padding draws from, as in the reference, which
    reassigns its points.  `ValueError`, naming the cloud, when a filter leaves a cloud fewer than `target` points."""
    if downsample not in ('pnvlad', 'random'):
        raise ValueError("downsample must be 'pnvlad' or 'random', got %r" % (downsample,))
    return submap_chain(clouds, device, radius_max=radius_max, remove_outliers=remove_outliers, outlier_params=outlier_params,
                        remove_ground=remove_ground, ground_params=ground_params, target=_check_target(target),
                        downsample=downsample, normalise=normalise, seed=seed)
