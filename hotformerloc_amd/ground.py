"""Ground removal for raw submaps by the Cloth Simulation Filter, for a whole ragged batch on the device.

The reference removes the ground of CS-Wild-Places submaps offline, on the host, one submap at a time, through the pip `CSF`
package (`datasets/CSWildPlaces/postprocess_submaps.py --remove_ground`, `processing_utils.remove_ground`: rigidness 2,
threshold 0.5 m, cloth resolution 1.0 m, slope smoothing on, library defaults otherwise); it is the first link of the
documented post-processing, before the voxel downsample and the normalisation of `voxel.py`.  Here a batch of raw submaps
goes to the GPU once; the pip package and open3d are not needed.

The method is that of Zhang et al. 2016 ("An easy-to-use airborne LiDAR data filtering method based on cloth simulation")
with the library's parameter meanings.  The library runs its constraint sweep in place under an OpenMP `parallel for`, so
its own output depends on thread timing; there is no library order to reproduce.  This module therefore DEFINES the
filter, fixing every order the library leaves to chance.  **Bit parity with the pip `CSF` package is not claimed.**  The
numpy route below (`remove_ground_host`, `cloth_surface_host`) and the device route follow the definition operation for
operation and agree to the bit.

Definition.  fp32 throughout, z up, u = -z the inverted height; every operation is rounded once, nothing is fused
(`csrc/ground.hip` is built with `-ffp-contract=off`).  r = `cloth_resolution`.

 1. Cloth grid, per cloud, from its fp32 bounds: ox = xmin - 2 r, oy = ymin - 2 r, W = floor((xmax - xmin) / r) + 4,
    H = floor((ymax - ymin) / r) + 4.  Particle (i, j) stands at (ox + i r, oy + j r) and carries one height.
 2. Raster: a point maps to col = int((x - ox) / r + 0.5), row = int((y - oy) / r + 0.5) (clamped into the cloth, which
    changes nothing for finite input).  A particle's terrain value t is -z of the mapped point with the smallest squared
    horizontal distance dx dx + dy dy to it, ties to the lowest point index.
 3. A particle no point maps to takes the t of a rastered particle, never of a filled one: the first found scanning its row
    towards larger i, else towards smaller i, else its column towards smaller j, else towards larger j, else the rastered
    particle at the smallest squared index distance, ties to the lowest j, then the lowest i.
 4. Simulation: every particle starts movable with u = u_prev = max(-z) + 0.05.  A step is
      (a) movable particles: new = u + (u - u_prev) * f32(0.99) + g, g = f32(-(0.2 time_step^2)); u_prev = u; u = new
      (b) constraints: the offsets (1,0) (0,1) (1,1) (1,-1) (2,0) (0,2) (2,2) (2,-2) in this order; the pairs
          {(i, j), (i + dx, j + dy)} of an offset fall into two classes by the parity of i // max(|dx|, 1) when dx != 0, of
          j // |dy| otherwise; the pairs of a class share no particle; the even class, then the odd class, per offset -- 16
          sub-passes -- and the whole sweep twice per step.  Pair rule with d = u_q - u_p: both movable, m = f2 d,
          u_p += m, u_q -= m; one movable, it moves by f1 d towards the other; f1 = f32(1 - 0.7^rigidness),
          f2 = f32(0.5 (1 - 0.4^rigidness))
      (c) m = max |u - u_prev| over the movable particles
      (d) where u < t: u = t and the particle is unmovable for good
    and the run stops after (d) when m != 0 and m < 0.005, when no particle is movable any more (nothing can change: this
    only shortens the count of steps), or after `iterations` steps.
 5. Slope smoothing (`slope_smooth`), until nothing changes: a movable particle p with an unmovable 4-neighbour q, where
    |t_p - t_q| < 0.3 and |u_p - t_p| < 0.3, gets u_p = t_p and becomes unmovable.  The rule is monotone, so the result does
    not depend on the order.
 6. Classification, per point: fx = (x - ox) / r, c = min(int(fx), W - 2), tx = fx - c, likewise fy, w, ty; the cloth height
    h = u[c,w](1-tx)(1-ty) + u[c,w+1](1-tx)ty + u[c+1,w+1]tx ty + u[c+1,w]tx(1-ty), summed in this order; ground when
    |(-z) - h| < `class_threshold`.  The output is the non-ground points in their order; it may be empty.

Deviations from the library, on purpose: the fixed orders above (the library's are timing-dependent); the library applies
step 5 only to movable components of more than 50 particles, here every component is smoothed; the stop on "no movable
particle", which changes no height.

Device route: `hfl_voxel_bounds` and one host read of the (B, 6) bounds, from which the host lays out the cloths;
`hfl_cloth_raster` (a 64-bit integer atomic min per point, then the fill), `hfl_cloth_simulate` (one workgroup per cloud, the
state in LDS for the whole run) and `hfl_cloth_classify`; `csrc/ground.hip`.  The mask is compacted by `ragged.compact`
(`torch.nonzero`, plumbing as `torch.sort` is in `voxel.py`, and `hfl_voxel_gather_rows`).

Limits: a cloth holds at most `MAX_PARTICLES` = 10 240 particles (100 x 100 fits: a 96 m submap at r = 1 m), because its
state stays in the 160 KiB of LDS of one compute unit; a larger one raises `ValueError` naming the cloud, after the bounds
are known and before any cloth kernel runs.  Batch limits as in `ragged.py`.  Non-finite coordinates give undefined output
(nothing is read or written out of bounds) or that `ValueError`."""

from typing import List, Sequence

import numpy as np
import torch

from . import ops, ragged

MAX_PARTICLES = ops.CLOTH_MAX_PARTICLES
GRAVITY = 0.2
DAMPING = 0.01
BUFFER_CELLS = 2
CLEARANCE = np.float32(0.05)
STOP_MOVE = np.float32(0.005)
SMOOTH_THRESHOLD = np.float32(0.3)
OFFSETS = ((1, 0), (0, 1), (1, 1), (1, -1), (2, 0), (0, 2), (2, 2), (2, -2))
_F = np.float32


class ClothParams:
    """the checked keyword parameters and the fp32 factors both routes use"""

    def __init__(self, cloth_resolution=1.0, rigidness=2, class_threshold=0.5, slope_smooth=True, time_step=0.65,
                 iterations=500):
        if isinstance(rigidness, bool) or rigidness not in (1, 2, 3):
            raise ValueError('rigidness must be 1, 2 or 3, got %r' % (rigidness,))
        ragged.check_positive('cloth_resolution', cloth_resolution, fp32=True)
        ragged.check_positive('class_threshold', class_threshold, fp32=True)
        ragged.check_positive('time_step', time_step, fp32=True)
        if int(iterations) != iterations or iterations < 0:
            raise ValueError('iterations must be a non-negative integer, got %r' % (iterations,))
        self.rigidness = int(rigidness)
        self.r = _F(cloth_resolution)
        self.threshold = _F(class_threshold)
        self.slope_smooth = bool(slope_smooth)
        self.iterations = int(iterations)
        self.gravity_step = _F(-(GRAVITY * float(time_step) * float(time_step)))
        self.keep = _F(1.0 - DAMPING)
        self.f1 = _F(1.0 - 0.7 ** self.rigidness)
        self.f2 = _F(0.5 * (1.0 - 0.4 ** self.rigidness))


def _limit_error(i: int, w, h):
    return ValueError('cloud %d needs a cloth of %s x %s particles, more than the %d that fit the on-chip memory of one '
                      'compute unit; use a larger cloth_resolution or a smaller submap' % (i, w, h, MAX_PARTICLES))


def cloth_grid(lo_hi: np.ndarray, r, index: int = 0):
    """step 1 from a cloud's fp32 bounds (min x, y, z, max x, y, z) -> (W, H, ox, oy, u0); `ValueError` over the limit"""
    lo_hi = np.asarray(lo_hi, dtype=np.float32)
    r = _F(r)
    with np.errstate(invalid='ignore', over='ignore'):
        two_r = _F(BUFFER_CELLS) * r
        ox, oy = lo_hi[0] - two_r, lo_hi[1] - two_r
        span = [np.floor((lo_hi[3 + a] - lo_hi[a]) / r) for a in (0, 1)]
        u0 = -lo_hi[2] + CLEARANCE                           # max(-z) = -min(z)
    if not all(np.isfinite(v) for v in (ox, oy, u0, span[0], span[1])) or max(span) + 4 > MAX_PARTICLES:
        raise _limit_error(index, '%s' % (span[0] + 4), '%s' % (span[1] + 4))
    w, h = int(span[0]) + 2 * BUFFER_CELLS, int(span[1]) + 2 * BUFFER_CELLS
    if w * h > MAX_PARTICLES:
        raise _limit_error(index, w, h)
    return w, h, _F(ox), _F(oy), _F(u0)


# ------------------------------------------------------------------------------------------------ host route (numpy fp32)
def _cell_index(f: np.ndarray, top: int) -> np.ndarray:
    """int(f) clamped into [0, top]; a NaN gives 0"""
    with np.errstate(invalid='ignore'):
        f = np.where(f >= 0, f, _F(0))
        return np.minimum(f, _F(top)).astype(np.int64)


def raster_host(cloud: np.ndarray, r, index: int = 0):
    """steps 1 to 3 for one (n, 3) fp32 cloud -> (W, H, ox, oy, u0, t (H, W) fp32, rastered (H, W) bool)"""
    cloud = np.asarray(cloud, dtype=np.float32).reshape(-1, 3)
    r = _F(r)
    with np.errstate(invalid='ignore'):
        lo_hi = np.concatenate([np.fmin.reduce(cloud, axis=0), np.fmax.reduce(cloud, axis=0)])
    W, H, ox, oy, u0 = cloth_grid(lo_hi, r, index)
    x, y, z = cloud[:, 0], cloud[:, 1], cloud[:, 2]
    with np.errstate(invalid='ignore', over='ignore'):
        col = _cell_index((x - ox) / r + _F(0.5), W - 1)
        row = _cell_index((y - oy) / r + _F(0.5), H - 1)
        dx = x - (ox + col.astype(np.float32) * r)
        dy = y - (oy + row.astype(np.float32) * r)
        d2 = dx * dx + dy * dy
    key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(cloud.shape[0], dtype=np.uint64)
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    best = np.full(W * H, none, dtype=np.uint64)
    np.minimum.at(best, row * W + col, key)
    rastered = (best != none).reshape(H, W)
    winner = (best & np.uint64(0xFFFFFFFF)).astype(np.int64)
    own = np.where(rastered.reshape(-1), -z[np.minimum(winner, cloud.shape[0] - 1)], _F(0)).astype(np.float32).reshape(H, W)
    return W, H, ox, oy, u0, fill_host(own, rastered), rastered


def fill_host(own: np.ndarray, rastered: np.ndarray) -> np.ndarray:
    """step 3: `own` (H, W) holds t where `rastered`; the empty particles are filled from rastered ones only"""
    H, W = rastered.shape
    ii, jj = np.meshgrid(np.arange(W), np.arange(H))
    right = np.minimum.accumulate(np.where(rastered, ii, W)[:, ::-1], axis=1)[:, ::-1]      # first rastered at >= i
    left = np.maximum.accumulate(np.where(rastered, ii, -1), axis=1)                         # last rastered at <= i
    below = np.maximum.accumulate(np.where(rastered, jj, -1), axis=0)                        # towards smaller j
    above = np.minimum.accumulate(np.where(rastered, jj, H)[::-1], axis=0)[::-1]             # towards larger j
    src_i = np.where(right < W, right, np.where(left >= 0, left, ii))
    in_row = (right < W) | (left >= 0)
    src_j = np.where(in_row, jj, np.where(below >= 0, below, np.where(above < H, above, -1)))
    rj, ri = np.nonzero(rastered)                            # ascending j, then i: argmin keeps the first of equals
    for j, i in zip(*np.nonzero(src_j < 0)):
        k = int(np.argmin((ri - i) ** 2 + (rj - j) ** 2)) if ri.size else -1
        src_i[j, i], src_j[j, i] = (ri[k], rj[k]) if k >= 0 else (i, j)
    return own[src_j, src_i]


def constraint_passes(W: int, H: int):
    """the 16 sub-passes of one constraint sweep on a W x H cloth, in order: a list of (p, q) flat-index arrays
    (index = j W + i) of the pairs {(i, j), (i + dx, j + dy)} of one offset and class"""
    passes = []
    i, j = np.arange(W), np.arange(H)
    for dx, dy in OFFSETS:
        for cls in (0, 1):
            if dx:
                ic = i[((i // dx) % 2 == cls) & (i + dx < W)]
                jc = j[(j + dy >= 0) & (j + dy < H)]
            else:
                ic = i
                jc = j[((j // dy) % 2 == cls) & (j + dy < H)]
            p = (jc[:, None] * W + ic[None, :]).reshape(-1)
            passes.append((p, p + dy * W + dx))
    return passes


def _pair_pass(u, movable, p, q, f1, f2):
    a, b = u[p], u[q]
    mp, mq = movable[p], movable[q]
    d = b - a
    m2, m1 = f2 * d, f1 * d
    u[p] = np.where(mp & mq, a + m2, np.where(mp, a + m1, a))
    u[q] = np.where(mp & mq, b - m2, np.where(mq & ~mp, b - m1, b))


def constraint_sweep_host(u: np.ndarray, movable: np.ndarray, rigidness: int = 2) -> np.ndarray:
    """one sweep of step 4(b) -- 16 sub-passes -- on a copy of the (H, W) fp32 heights"""
    prm = ClothParams(rigidness=rigidness)
    H, W = u.shape
    flat = np.array(u, dtype=np.float32).reshape(-1)
    mv = np.asarray(movable, dtype=bool).reshape(-1)
    for p, q in constraint_passes(W, H):
        _pair_pass(flat, mv, p, q, prm.f1, prm.f2)
    return flat.reshape(H, W)


def slope_smooth_host(u: np.ndarray, t: np.ndarray, movable: np.ndarray):
    """step 5 on copies of the (H, W) state -> (u, movable)"""
    u, mv = np.array(u, dtype=np.float32), np.array(movable, dtype=bool)
    t = np.asarray(t, dtype=np.float32)
    while True:
        near = np.zeros_like(mv)
        for axis, back in ((1, False), (1, True), (0, False), (0, True)):
            tq, fixed = np.roll(t, 1 if back else -1, axis), np.roll(~mv, 1 if back else -1, axis)
            edge = [slice(None), slice(None)]
            edge[axis] = 0 if back else -1
            fixed[tuple(edge)] = False                       # no neighbour across the border
            with np.errstate(invalid='ignore'):
                near |= fixed & (np.abs(t - tq) < SMOOTH_THRESHOLD)
        with np.errstate(invalid='ignore'):
            take = mv & near & (np.abs(u - t) < SMOOTH_THRESHOLD)
        if not take.any():
            return u, mv
        u[take] = t[take]
        mv[take] = False


def simulate_host(t: np.ndarray, u0, prm: ClothParams):
    """steps 4 and 5 on the (H, W) terrain values -> (u (H, W) fp32, movable (H, W) bool, steps_run)"""
    H, W = t.shape
    tf = np.asarray(t, dtype=np.float32).reshape(-1)
    u = np.full(W * H, _F(u0), dtype=np.float32)
    up = u.copy()
    mv = np.ones(W * H, dtype=bool)
    passes = constraint_passes(W, H)
    steps = 0
    with np.errstate(invalid='ignore', over='ignore'):
        for _ in range(prm.iterations):
            new = (u + (u - up) * prm.keep) + prm.gravity_step
            up = np.where(mv, u, up)
            u = np.where(mv, new, u)
            for _sweep in range(2):
                for p, q in passes:
                    _pair_pass(u, mv, p, q, prm.f1, prm.f2)
            move = np.abs(u - up)[mv].max() if mv.any() else _F(0)
            hit = mv & (u < tf)
            u[hit] = tf[hit]
            mv &= ~hit
            steps += 1
            if (move != 0 and move < STOP_MOVE) or not mv.any():
                break
    u, mv = u.reshape(H, W), mv.reshape(H, W)
    if prm.slope_smooth:
        u, mv = slope_smooth_host(u, t, mv)
    return u, mv, steps


def classify_host(cloud: np.ndarray, u: np.ndarray, ox, oy, prm: ClothParams) -> np.ndarray:
    """step 6 -> (n,) bool, True where the point is NOT ground"""
    H, W = u.shape
    with np.errstate(invalid='ignore', over='ignore'):
        fx, fy = (cloud[:, 0] - ox) / prm.r, (cloud[:, 1] - oy) / prm.r
        c, w = _cell_index(fx, W - 2), _cell_index(fy, H - 2)
        tx, ty = fx - c.astype(np.float32), fy - w.astype(np.float32)
        sx, sy = _F(1) - tx, _F(1) - ty
        h = u[w, c] * sx * sy
        h = h + u[w + 1, c] * sx * ty
        h = h + u[w + 1, c + 1] * tx * ty
        h = h + u[w, c + 1] * tx * sy
        return ~(np.abs(-cloud[:, 2] - h) < prm.threshold)


def _cloth_host(arrays, prm):
    grids = [raster_host(a, prm.r, i) for i, a in enumerate(arrays)]         # every limit is checked before any simulation
    out = []
    for W, H, ox, oy, u0, t, _ in grids:
        u, mv, steps = simulate_host(t, u0, prm)
        out.append((u, mv, t, steps, ox, oy))
    return out


def cloth_surface_host(clouds: Sequence, **params):
    """The cloth of every cloud by the numpy route: a list of (u (H, W) fp32, movable (H, W) bool, t (H, W) fp32,
    steps_run)."""
    prm = ClothParams(**params)
    return [c[:4] for c in _cloth_host(ragged.as_arrays(clouds), prm)]


def remove_ground_host(clouds: Sequence, *, return_mask: bool = False, return_cloth: bool = False, **params):
    """The definition of the module docstring in numpy fp32: the route without a GPU and the yardstick of the tests.  List of
    (n_i, 3) clouds -> list of (k_i, 3) float32 arrays, the non-ground points in input order (k_i may be 0); with
    `return_mask` also the (n_i,) bool masks of the kept points, with `return_cloth` also what `cloth_surface_host` returns."""
    prm = ClothParams(**params)
    arrays = ragged.as_arrays(clouds)
    cloths = _cloth_host(arrays, prm)
    masks = [classify_host(a, c[0], c[4], c[5], prm) for a, c in zip(arrays, cloths)]
    return ragged.results([a[m] for a, m in zip(arrays, masks)], masks if return_mask else None,
                          [c[:4] for c in cloths] if return_cloth else None)


# ------------------------------------------------------------------------------------------------ device route
def cloth_device(packed, prm: ClothParams):
    """bounds -> table -> raster -> simulate, everything but the bounds staying on the device -> (table, terrain, heights,
    movable, steps_run)"""
    _, lo_hi = ragged.bounds_host(packed)                                     # the one host read before the cloths are laid out
    descs = np.zeros(packed.batch, dtype=np.dtype(ops.CLOTH_DESC_DTYPE))
    at = 0
    for i in range(descs.shape[0]):
        w, h, ox, oy, u0 = cloth_grid(lo_hi[i], prm.r, i)
        descs[i] = (ox, oy, u0, w, h, 0, at)
        at += w * h
    table = ops.ClothTable(descs, packed.pts.device)
    terrain = ops.cloth_raster(packed.pts, packed.off, table, float(prm.r))
    heights, movable, steps = ops.cloth_simulate(terrain, table, float(prm.f1), float(prm.f2), float(prm.gravity_step),
                                                 float(prm.keep), prm.iterations, prm.slope_smooth)
    return table, terrain, heights, movable, steps


def _split_cloths(table, terrain, heights, movable, steps):
    steps = steps.cpu().tolist()
    out = []
    for b in range(table.batch):
        w, h, s = int(table.host['width'][b]), int(table.host['height'][b]), int(table.host['cell_offset'][b])
        if steps[b] < 0:
            raise RuntimeError('hfl_cloth_simulate refused cloth %d (%d x %d)' % (b, w, h))
        out.append((heights[s:s + w * h].reshape(h, w), movable[s:s + w * h].reshape(h, w).bool(),
                    terrain[s:s + w * h].reshape(h, w), steps[b]))
    return out


def cloth_surface(clouds: Sequence, *, device='cuda', **params):
    """`cloth_surface_host` on the device: a list of (u (H, W) fp32, movable (H, W) bool, t (H, W) fp32 device tensors,
    steps_run), bit for bit what the numpy route returns."""
    prm = ClothParams(**params)
    with ragged.intake(clouds, device) as packed:
        return [] if packed is None else _split_cloths(*cloth_device(packed, prm))


def remove_ground_packed(packed, prm: ClothParams):
    """the filter on a packed batch -> (the kept rows as a `ragged.Packed`, keep (P,) uint8, what `cloth_device` returned)"""
    cloth = cloth_device(packed, prm)
    keep = ops.cloth_classify(packed.pts, packed.off, cloth[2], cloth[0], float(prm.r), float(prm.threshold))
    return ragged.compact(packed, keep), keep, cloth


def remove_ground(clouds: Sequence, *, device='cuda', return_mask: bool = False, return_cloth: bool = False, **params):
    """List of raw (n_i, 3) clouds (numpy / torch, host or device) -> list of (k_i, 3) float32 device tensors: the points
    the cloth filter of the module docstring does not call ground, in input order, bit for bit the rows `remove_ground_host`
    returns (k_i may be 0).  Keyword parameters, with the reference's values as defaults: `cloth_resolution` = 1.0,
    `rigidness` = 2, `class_threshold` = 0.5, `slope_smooth` = True, `time_step` = 0.65, `iterations` = 500.  `return_mask`:
    also the (n_i,) bool masks of the kept points; `return_cloth`: also what `cloth_surface` returns.  `ValueError` for a bad
    parameter or an empty cloud (before the device is touched) and, naming the cloud, for a cloth of more than 10 240
    particles (before any cloth kernel runs)."""
    prm = ClothParams(**params)
    with ragged.intake(clouds, device) as packed:
        if packed is None:
            return ragged.empty_results(return_mask, return_cloth)
        kept, keep, cloth = remove_ground_packed(packed, prm)
        return ragged.results(kept.split(), packed.split(keep.bool()) if return_mask else None,
                              _split_cloths(*cloth) if return_cloth else None)


def filter_batch(clouds: Sequence, device, ground_params=None, at_least: int = 1) -> List[torch.Tensor]:
    """`remove_ground` alone, as the submap entry points of `voxel.py` run it: the filtered batch on the device, `ValueError`
    naming the first cloud with no point left or with fewer than `at_least` points."""
    from .voxel import submap_chain                  # a public alias kept for callers: voxel.py holds the chain
    return submap_chain(clouds, device, remove_ground=True, ground_params=ground_params, at_least=at_least)
