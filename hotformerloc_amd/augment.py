"""Training augmentation for a whole batch on the device: raw clouds -> what `Points(...)` receives in training.

The reference augments every cloud on the host, in the dataloader: `TrainTransform`
(`datasets/CSWildPlaces/CSWildPlaces_train.py:19-57`, `datasets/pointnetvlad/pnv_train.py`) is Normalize -> JitterPoints
-> RemoveRandomPoints -> [RandomRotation about z, aug_mode 2] -> RandomTranslation -> RemoveRandomBlock, then
`base_datasets.py:77-83` masks |c| > 1 (and |xy| > 1), then the collate function applies one `TrainSetTransform` (z
rotation + flip, or flip) to the concatenated batch and the quantizer's cylindrical transform
(`dataset_utils.py:105-139`).  `augment_clouds` does all of it in ONE launch (`hfl_augment_clouds`, a workgroup per cloud,
csrc/augment.hip); `augment_clouds_host` restates the same chain in numpy / torch on the CPU with the same random
numbers -- it is what the GPU tests compare against and what runs where there is no GPU.

Random numbers are of two kinds.  The scalars per cloud and per batch (`AugmentParams`) are drawn on the host from a
`torch.Generator` by `draw_params` and go to the kernel as a small table; a caller may pass a table of its own.  The
numbers per point are Philox4x32-10, key = the 64-bit seed, counter = (point index in its cloud, cloud index + cloud_base,
stream, 0): stream 0 -> the three jitter normals (Box-Muller, uniform = (u32 + 0.5) * 2^-32), stream 1 word 0 -> the point's
selection key.  RemoveRandomPoints removes the k points with the smallest keys, ties to the lower index: a uniformly random
k-subset like the reference's `np.random.choice(replace=False)`."""

import math
from dataclasses import dataclass, field, replace
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _native

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_TWO_PI32 = np.float32(6.2831854820251465)
_INV32 = np.float32(2.0 ** -32)
_CYL_MODES = ('host', 'device', 'none')


# ---------------------------------------------------------------------------------------------- configuration
@dataclass(frozen=True)
class AugmentConfig:
    """What `TrainingParams` fixes (`misc/utils.py`), plus the constants the reference's transforms hard-code."""
    aug_mode: int = 1
    set_aug_mode: int = 1
    random_rot_theta: float = 5.0
    normalize_points: bool = True
    coordinates: str = 'cartesian'
    jitter_sigma: float = 0.001
    jitter_clip: float = 0.002
    remove_ratio: tuple = (0.0, 0.1)
    max_delta: float = 0.01
    block_p: float = 0.4
    block_scale: tuple = (0.02, 0.33)
    block_ratio: tuple = (0.3, 3.3)
    flip_p: tuple = (0.25, 0.25, 0.0)

    @classmethod
    def from_training_params(cls, aug_mode: int, set_aug_mode: int, random_rot_theta: float = 5.0,
                             normalize_points: bool = False, coordinates: str = 'cartesian', scale_factor=None,
                             unit_sphere_norm: bool = False, zero_mean: bool = True) -> 'AugmentConfig':
        if scale_factor is not None or unit_sphere_norm or not zero_mean:
            # same limits as prepare_clouds: these modes reduce with torch.mean / a division whose CPU summation order
            # is not reproducible on the device; no shipped config uses them
            raise NotImplementedError('only the bounding-box normalisation of the shipped configs runs on the device')
        if coordinates not in ('cartesian', 'cylindrical'):
            raise NotImplementedError('coordinates=%r' % coordinates)
        if aug_mode not in (0, 1, 2):
            raise NotImplementedError('Unknown aug_mode: {}'.format(aug_mode))
        if set_aug_mode not in (0, 1, 2):
            raise NotImplementedError('Unknown aug_mode: {}'.format(set_aug_mode))
        return cls(int(aug_mode), int(set_aug_mode), float(random_rot_theta), bool(normalize_points), coordinates)


def _cos_sin32(theta: float):
    return np.float32(math.cos(theta)), np.float32(math.sin(theta))


@dataclass
class AugmentParams:
    """The random scalars of one batch.  Per cloud (arrays of length B): `remove_k` = int(n * r) with r ~ U(remove_ratio)
    in `remove_r`; `theta` and its float32 cos / sin; `trans` = float32(max_delta * `trans_n`), trans_n ~ N(0,1)^3; `block`
    the coin (1 = erase) and `block_u` = U(scale), U(ratio), U(0,1), U(0,1).  Per batch: `set_theta` with cos / sin and
    `flip_axis` (-1 none, 0 x, 1 y, 2 z) from `flip_draw`.  The float64 fields are the draws themselves, kept so that the
    reference's classes can be fed the same numbers; the kernel reads the float32 / integer ones."""
    remove_k: np.ndarray
    remove_r: np.ndarray
    theta: np.ndarray
    rot_cos: np.ndarray
    rot_sin: np.ndarray
    trans_n: np.ndarray
    trans: np.ndarray
    block: np.ndarray
    block_coin: np.ndarray
    block_u: np.ndarray
    set_theta: float = 0.0
    set_cos: np.float32 = field(default_factory=lambda: np.float32(1.0))
    set_sin: np.float32 = field(default_factory=lambda: np.float32(0.0))
    flip_draw: float = 1.0
    flip_axis: int = -1

    def __len__(self):
        return len(self.remove_k)

    def slice(self, start: int, stop: int) -> 'AugmentParams':
        """Clouds [start, stop) with the batch-wide draw unchanged (one minibatch of a split batch)."""
        kw = {f: getattr(self, f)[start:stop] for f in self._ARRAYS}
        return replace(self, **kw)

    _ARRAYS = ('remove_k', 'remove_r', 'theta', 'rot_cos', 'rot_sin', 'trans_n', 'trans', 'block', 'block_coin', 'block_u')
    _SCALARS = ('set_theta', 'set_cos', 'set_sin', 'flip_draw', 'flip_axis')

    def to_arrays(self, prefix: str = '') -> dict:
        """Every field as a numpy array under `prefix + name` (what tests/golden/augment.npz stores)."""
        return {prefix + f: np.asarray(getattr(self, f)) for f in self._ARRAYS + self._SCALARS}

    @classmethod
    def from_arrays(cls, d, prefix: str = '') -> 'AugmentParams':
        kw = {f: np.array(d[prefix + f]) for f in cls._ARRAYS}
        kw.update(set_theta=float(d[prefix + 'set_theta']), set_cos=np.float32(d[prefix + 'set_cos']),
                  set_sin=np.float32(d[prefix + 'set_sin']), flip_draw=float(d[prefix + 'flip_draw']),
                  flip_axis=int(d[prefix + 'flip_axis']))
        return cls(**kw)

    def rows(self) -> np.ndarray:
        """(B, 12) uint32: the table in the layout of `hfl_augment_cloud`."""
        b = len(self)
        t = np.zeros((b, 12), dtype=np.uint32)
        t[:, 0] = np.asarray(self.remove_k, dtype=np.int32).view(np.uint32)
        t[:, 1] = np.asarray(self.block, dtype=np.int32).view(np.uint32)
        t[:, 2] = np.asarray(self.rot_cos, dtype=np.float32).view(np.uint32)
        t[:, 3] = np.asarray(self.rot_sin, dtype=np.float32).view(np.uint32)
        t[:, 4:7] = np.ascontiguousarray(self.trans, dtype=np.float32).view(np.uint32).reshape(b, 3)
        t[:, 7:11] = np.ascontiguousarray(self.block_u.astype(np.float32)).view(np.uint32).reshape(b, 4)
        return t


def identity_params(sizes: Sequence[int]) -> AugmentParams:
    """The table that changes nothing: k = 0, no rotation, no translation, coin down, no batch-wide transform."""
    b = len(sizes)
    return AugmentParams(remove_k=np.zeros(b, np.int64), remove_r=np.zeros(b), theta=np.zeros(b),
                         rot_cos=np.ones(b, np.float32), rot_sin=np.zeros(b, np.float32), trans_n=np.zeros((b, 3)),
                         trans=np.zeros((b, 3), np.float32), block=np.zeros(b, np.int32), block_coin=np.ones(b),
                         block_u=np.zeros((b, 4)))


def flip_axis_of(draw: float, flip_p=(0.25, 0.25, 0.0)) -> int:
    """`RandomFlip.__call__` (`augmentation.py:40-52`): the first axis whose cumulative probability reaches the draw."""
    cum = np.cumsum(flip_p)
    for axis in range(3):
        if draw <= cum[axis]:
            return axis
    return -1


def draw_params(sizes: Sequence[int], cfg: AugmentConfig, generator: Optional[torch.Generator] = None) -> AugmentParams:
    """Draw every scalar of one batch from `generator` (a CPU `torch.Generator`; None = torch's default one), in a fixed
    order: per cloud 8 uniforms and 3 normals when `aug_mode != 0`, then 2 uniforms per batch when `set_aug_mode != 0`.
    `aug_mode` 0 with `set_aug_mode` 0 draws nothing and leaves the generator untouched."""
    sizes = [int(s) for s in sizes]
    b = len(sizes)
    p = identity_params(sizes)
    if cfg.aug_mode != 0 and b > 0:
        u = torch.rand(b, 8, dtype=torch.float64, generator=generator).numpy()
        g = torch.randn(b, 3, dtype=torch.float64, generator=generator).numpy()
        lo, hi = cfg.remove_ratio
        for i, n in enumerate(sizes):
            r = lo + (hi - lo) * float(u[i, 0])                       # random.uniform(r_min, r_max)
            p.remove_r[i] = r
            p.remove_k[i] = int(n * r)
            if cfg.aug_mode == 2:
                theta = (np.pi * cfg.random_rot_theta / 180.) * 2. * (float(u[i, 1]) - 0.5)
                p.theta[i] = theta
                p.rot_cos[i], p.rot_sin[i] = _cos_sin32(theta)
            p.block_coin[i] = u[i, 2]
            p.block[i] = 1 if u[i, 2] < cfg.block_p else 0
            p.block_u[i, 0] = cfg.block_scale[0] + (cfg.block_scale[1] - cfg.block_scale[0]) * float(u[i, 3])
            p.block_u[i, 1] = cfg.block_ratio[0] + (cfg.block_ratio[1] - cfg.block_ratio[0]) * float(u[i, 4])
            p.block_u[i, 2] = u[i, 5]
            p.block_u[i, 3] = u[i, 6]
        p.trans_n = g
        p.trans = (cfg.max_delta * g).astype(np.float32)
    if cfg.set_aug_mode != 0:
        u = torch.rand(2, dtype=torch.float64, generator=generator).numpy()
        if cfg.set_aug_mode == 1:
            p.set_theta = (np.pi * cfg.random_rot_theta / 180.) * 2. * (float(u[0]) - 0.5)
            p.set_cos, p.set_sin = _cos_sin32(p.set_theta)
        p.flip_draw = float(u[1])
        p.flip_axis = flip_axis_of(p.flip_draw, cfg.flip_p)
    return p


# ---------------------------------------------------------------------------------------------- Philox, host side
def philox4x32_10(counter: np.ndarray, key) -> np.ndarray:
    """Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11).  counter (..., 4) and key
    (2,) of 32-bit words -> (..., 4) uint32."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    mask = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(_M0) * c[0]
        p1 = np.uint64(_M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0 = (k0 + _W0) & 0xFFFFFFFF
        k1 = (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def _point_words(n: int, seed: int, cloud_id: int, stream: int) -> np.ndarray:
    ctr = np.zeros((n, 4), dtype=np.uint32)
    ctr[:, 0] = np.arange(n, dtype=np.uint32)
    ctr[:, 1] = np.uint32(cloud_id & 0xFFFFFFFF)
    ctr[:, 2] = np.uint32(stream)
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def jitter_normals(n: int, seed: int, cloud_id: int) -> np.ndarray:
    """(n, 3) float32 standard normals of stream 0."""
    w = _point_words(n, seed, cloud_id, 0)
    u = (w.astype(np.float32) + np.float32(0.5)) * _INV32
    r0 = np.sqrt(np.float32(-2.0) * np.log(u[:, 0]))
    a0 = _TWO_PI32 * u[:, 1]
    r1 = np.sqrt(np.float32(-2.0) * np.log(u[:, 2]))
    a1 = _TWO_PI32 * u[:, 3]
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1)], axis=1).astype(np.float32)


def philox_selection_keys(n: int, seed: int, cloud_id: int) -> np.ndarray:
    """(n,) uint32 selection keys of stream 1."""
    return _point_words(n, seed, cloud_id, 1)[:, 0].copy()


def select_removed(keys: np.ndarray, k: int) -> np.ndarray:
    """Indices of the k smallest keys, ties to the lower index, ascending."""
    return np.sort(np.argsort(np.asarray(keys, dtype=np.uint32), kind='stable')[:k])


# ---------------------------------------------------------------------------------------------- the chain on the host
def _cylindrical_host(pc: np.ndarray) -> np.ndarray:
    """`synthetic.cylindrical` without its range assertion: the batch-wide rotation may leave a coordinate an ulp outside
    [-1, 1], which the reference hands to its transform as it is."""
    t = torch.from_numpy(np.ascontiguousarray(pc, dtype=np.float32))
    phi = torch.atan2(t[:, 1], t[:, 0])
    rho = torch.sqrt(t[:, 0] ** 2 + t[:, 1] ** 2)
    out = torch.stack([rho, phi, t[:, 2]], dim=1)
    out[:, 0] = torch.tensor(np.interp(out[:, 0].numpy(), [0, 1], [-1, 1]))
    out[:, 1] = torch.tensor(np.interp(out[:, 1].numpy(), [-np.pi, np.pi], [-1, 1]))
    return torch.clamp(out, -1.0, 1.0).numpy()


def _rotate_z(p: np.ndarray, c, s) -> np.ndarray:
    """coords @ R for R = float32(expm(cross(eye(3), (0, 0, theta)))): x' = x cos + y sin, y' = y cos - x sin, products
    rounded before the sum (the order the kernel fixes)."""
    c, s = np.float32(c), np.float32(s)
    out = p.copy()
    out[:, 0] = p[:, 0] * c + p[:, 1] * s
    out[:, 1] = p[:, 1] * c + -(p[:, 0] * s)
    return out


def block_rectangle(p: np.ndarray, block_u) -> tuple:
    """`RemoveRandomBlock.get_params` (`augmentation.py:160-176`) operation by operation: float32 tensors, Python doubles
    only inside `math.sqrt`, w and h rounded to float32 where they meet a tensor.  Returns (x0, x1, y0, y1), float32."""
    s, ar, ux, uy = (np.float32(v) for v in block_u)
    mn, mx = p[:, :2].min(0), p[:, :2].max(0)
    span = mx - mn
    area = span[0] * span[1]
    erase = s * area
    h = np.float32(math.sqrt(float(erase * ar)))
    w = np.float32(math.sqrt(float(erase / ar)))
    x0 = mn[0] + ux * (span[0] - w)
    y0 = mn[1] + uy * (span[1] - h)
    return x0, x0 + w, y0, y0 + h


def augment_cloud_host(raw, cfg: AugmentConfig, params: AugmentParams, i: int, seed: int, cloud_id: int,
                       keys: Optional[np.ndarray] = None, cylindrical: bool = True, stages: Optional[dict] = None):
    """One cloud through the whole chain on the CPU.  `params` row i, Philox cloud index `cloud_id`.  Returns (points
    (m, 3) float32, source index (m,) int32).  `stages`, if given, receives 'removed' (indices set to zero by step 3),
    'pre_mask' (all n points in front of the masks) and 'masked' (the kept points in front of the batch-wide transform)."""
    p = np.array(torch.as_tensor(raw, dtype=torch.float32).reshape(-1, 3).cpu().numpy(), dtype=np.float32)
    n = len(p)
    if cfg.normalize_points:
        mn, mx = p.min(0), p.max(0)
        center = (mn + mx) * np.float32(0.5)
        box = (mx - mn).max() + np.float32(1.0e-6)
        p = (p - center) * (np.float32(2.0) / box)
    removed = np.zeros(0, dtype=np.int64)
    if cfg.aug_mode != 0:
        jit = np.float32(cfg.jitter_sigma) * jitter_normals(n, seed, cloud_id)
        p = p + np.clip(jit, -np.float32(cfg.jitter_clip), np.float32(cfg.jitter_clip))
        k = int(params.remove_k[i])
        if k > 0:
            removed = select_removed(philox_selection_keys(n, seed, cloud_id) if keys is None else keys, k)
            p[removed] = 0.0
        if cfg.aug_mode == 2:
            p = _rotate_z(p, params.rot_cos[i], params.rot_sin[i])
        p = p + np.asarray(params.trans[i], dtype=np.float32)[None, :]
        if int(params.block[i]) != 0:
            x0, x1, y0, y1 = block_rectangle(p, params.block_u[i])
            inside = (x0 < p[:, 0]) & (p[:, 0] < x1) & (y0 < p[:, 1]) & (p[:, 1] < y1)
            p[inside] = 0.0
    keep = np.all(np.abs(p) <= np.float32(1.0), axis=1)
    if cfg.coordinates == 'cylindrical':
        norm = torch.linalg.norm(torch.from_numpy(np.ascontiguousarray(p[:, :2])), dim=1).numpy()
        keep &= norm <= np.float32(1.0)
    if stages is not None:
        stages['removed'] = removed
        stages['pre_mask'] = p.copy()
    idx = np.nonzero(keep)[0].astype(np.int32)
    p = p[keep]
    if stages is not None:
        stages['masked'] = p.copy()
    if cfg.set_aug_mode == 1:
        p = _rotate_z(p, params.set_cos, params.set_sin)
    if params.flip_axis >= 0:
        p[:, params.flip_axis] = -p[:, params.flip_axis]
    if cfg.coordinates == 'cylindrical' and cylindrical:
        p = _cylindrical_host(p)
    return np.ascontiguousarray(p, dtype=np.float32), idx


def _sizes(clouds):
    ts = [torch.as_tensor(c, dtype=torch.float32).reshape(-1, 3) for c in clouds]
    sizes = [int(t.shape[0]) for t in ts]
    if sizes and min(sizes) < 1:
        raise ValueError('empty point cloud')
    return ts, sizes


def _resolve_params(sizes, cfg, generator, params):
    if params is None:
        params = draw_params(sizes, cfg, generator)
    if len(params) != len(sizes):
        raise ValueError('params holds %d clouds, the batch %d' % (len(params), len(sizes)))
    return params


def augment_clouds_host(clouds: Sequence, cfg: AugmentConfig, *, seed: int, generator=None, params=None,
                        cloud_base: int = 0, selection_keys=None, cylindrical: str = 'host', return_index: bool = False):
    """`augment_clouds` on the CPU, cloud by cloud: list of (m_i, 3) float32 torch tensors (and the int32 source indices
    with `return_index`).  `selection_keys`: optional list of per-cloud uint32 keys replacing Philox stream 1.
    `cylindrical`: 'host' and 'device' both mean the reference's transform here; 'none' stops in front of it."""
    if cylindrical not in _CYL_MODES:
        raise ValueError("cylindrical must be 'host', 'device' or 'none'")
    ts, sizes = _sizes(clouds)
    params = _resolve_params(sizes, cfg, generator, params)
    pts, idx = [], []
    for i, t in enumerate(ts):
        p, ix = augment_cloud_host(t, cfg, params, i, seed, cloud_base + i,
                                   None if selection_keys is None else selection_keys[i], cylindrical != 'none')
        pts.append(torch.from_numpy(p))
        idx.append(torch.from_numpy(ix))
    if any(len(p) < 1 for p in pts):
        raise ValueError('a cloud has no point left inside the unit cube / cylinder')
    return (pts, idx) if return_index else pts


# ---------------------------------------------------------------------------------------------- the device path
def native_config(cfg: AugmentConfig, params: AugmentParams, cylindrical_on_device: bool) -> '_native.AugmentConfig':
    cyl = cfg.coordinates == 'cylindrical'
    return _native.AugmentConfig(int(cfg.normalize_points), int(cyl), int(cyl and cylindrical_on_device),
                                 int(cfg.aug_mode != 0), int(cfg.aug_mode == 2), int(cfg.set_aug_mode == 1),
                                 int(params.flip_axis), float(params.set_cos), float(params.set_sin),
                                 float(cfg.jitter_sigma), float(cfg.jitter_clip))


def augment_clouds(clouds: Sequence, cfg: AugmentConfig, *, seed: int, generator=None, params=None, cloud_base: int = 0,
                   cylindrical: str = 'device', return_index: bool = False, selection_keys=None,
                   device='cuda') -> List[torch.Tensor]:
    """List of raw (n_i, 3) clouds (numpy / torch, any device) -> list of (m_i, 3) float32 CUDA tensors, augmented, masked
    and (cylindrical configs) transformed: ready for `build_batch_octree`.  One launch for the batch.

    `seed`: the Philox key of the per-point numbers.  `params`: the scalar table (default: `draw_params(sizes, cfg,
    generator)`).  `cloud_base`: Philox index of the first cloud, so that a batch processed in pieces draws what it would
    draw in one call.  `cylindrical`: as in `prepare_clouds` ('host' runs the transform on the host with the reference's
    bits; 'none' stops in front of it: masked cartesian points).  `return_index`: also return, per cloud, the int32 index of every kept point in its input cloud.
    `selection_keys`: optional list of per-cloud uint32 arrays replacing Philox stream 1 in RemoveRandomPoints."""
    from . import ops
    if cylindrical not in _CYL_MODES:
        raise ValueError("cylindrical must be 'host', 'device' or 'none'")
    device = torch.device(device)
    if device.type != 'cuda':
        raise _native.NativeLibraryError('augment_clouds runs on the GPU (augment_clouds_host is the CPU restatement)')
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    if not clouds:
        return ([], []) if return_index else []
    ts, sizes = _sizes(clouds)
    params = _resolve_params(sizes, cfg, generator, params)
    pts = torch.cat([t.to(device, non_blocking=True) for t in ts]).contiguous()
    keys = None
    if selection_keys is not None:
        keys = np.concatenate([np.asarray(k, dtype=np.uint32).reshape(-1) for k in selection_keys])
        if len(keys) != sum(sizes):
            raise ValueError('selection keys: one per point')
        keys = torch.from_numpy(keys.view(np.int32)).to(device)
    out, counts, index = ops.augment_clouds(pts, sizes, params.rows(), native_config(cfg, params, cylindrical == 'device'),
                                            seed, cloud_base, keys, return_index)
    kept = counts.cpu().tolist()                               # the one host read: how many points survived
    starts = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    res = [out[s:s + k] for s, k in zip(starts, kept)]
    if cfg.coordinates == 'cylindrical' and cylindrical == 'host':
        res = [torch.from_numpy(_cylindrical_host(r.cpu().numpy())).to(device, non_blocking=True) for r in res]
    if any(k < 1 for k in kept):
        raise ValueError('a cloud has no point left inside the unit cube / cylinder')
    if return_index:
        return res, [index[s:s + k] for s, k in zip(starts, kept)]
    return res
