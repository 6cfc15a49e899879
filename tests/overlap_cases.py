"""Shared inputs of the overlap tests (tests/test_overlap_host.py, tests/test_gpu_overlap.py): seeded forest-like clouds,
ragged batches with empty clouds in the middle, exact duplicate points, rigid transforms, one matrix that is not rigid, and
the tolerances both files derive their checks from.  The reference never implemented the distance, so there is no golden
file: the float64 host route is the truth, and the host tests pin it against closed forms."""
import numpy as np

EXTENT = 64.0                          # every coordinate lies inside +-EXTENT metres
TAU = 0.8                              # the CS-Wild-Places voxel size
DIST_RTOL = 1e-6                       # |d_dev - d_host| <= DIST_RTOL * d_host: ~5x the 3 * 2^-24 of difference, fma sum, sqrt
TRANSFORM_ULPS = 4.0                   # per coordinate, in ulp32 of the largest coordinate magnitude after the transform


def ulp32(x):
    """the spacing of float32 at magnitude x"""
    return float(np.spacing(np.float32(abs(x))))


def forest(n, seed, extent=40.0):
    """n float32 points of a forest-like scene: a rough ground sheet, vertical trunks, canopy blobs on top of them"""
    rng = np.random.RandomState(seed)
    n_trunk, n_canopy = n // 3, n // 3
    n_ground = n - n_trunk - n_canopy
    trees = rng.uniform(-extent, extent, (max(1, n // 40), 2))
    ground = np.concatenate([rng.uniform(-extent, extent, (n_ground, 2)), rng.normal(0.0, 0.15, (n_ground, 1))], 1)
    t = trees[rng.randint(0, trees.shape[0], n_trunk)]
    trunk = np.concatenate([t + rng.normal(0.0, 0.2, t.shape), rng.uniform(0.0, 12.0, (n_trunk, 1))], 1)
    c = trees[rng.randint(0, trees.shape[0], n_canopy)]
    canopy = np.concatenate([c + rng.normal(0.0, 2.0, c.shape), rng.normal(15.0, 2.5, (n_canopy, 1))], 1)
    pts = np.concatenate([ground, trunk, canopy], 0)[rng.permutation(n)]
    return np.clip(pts, -EXTENT, EXTENT).astype(np.float32)


def with_duplicates(cloud, seed, share=0.1):
    """the cloud with about `share` of its points overwritten by exact copies of other points; returns (cloud, lowest):
    lowest[j] = the lowest index holding the same point as j"""
    rng = np.random.RandomState(seed)
    out = cloud.copy()
    n = out.shape[0]
    k = rng.choice(n, max(1, int(n * share)), replace=False)
    out[k] = out[rng.randint(0, n, k.shape[0])]
    _, first, inverse = np.unique(out, axis=0, return_index=True, return_inverse=True)
    lowest = first[inverse.ravel()]                                # np.unique reports a row's first occurrence
    assert np.array_equal(out[lowest], out) and (lowest <= np.arange(n)).all()
    return out, lowest


def rigid(seed, max_shift=4.0):
    """a 4 x 4 float64 SE(3): a rotation about z and a translation of a few metres"""
    rng = np.random.RandomState(seed)
    a = rng.uniform(-np.pi, np.pi)
    m = np.eye(4)
    m[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    m[:3, 3] = rng.uniform(-max_shift, max_shift, 3)
    return m


def non_rigid():
    """a slightly non-orthonormal 4 x 4, like the UTM alignment matrices of the ground post-processing: a rotation about z
    with 2 % anisotropic scale and a small shear"""
    m = rigid(77)
    m[:3, :3] = m[:3, :3] @ np.array([[1.02, 0.015, 0.0], [0.0, 0.985, 0.0], [0.01, 0.0, 1.01]])
    return m


def ragged_pairs(seed, sizes_a=(700, 0, 1300, 40, 515), sizes_b=(900, 300, 0, 2100, 64)):
    """P = 5 pairs of clouds (lists of float32 arrays): pair 1 has an empty a, pair 2 an empty b, in the middle of the batch;
    both clouds of a pair cover the same 24 m x 24 m, densely enough that a good share of the points has a neighbour within TAU"""
    a = [forest(n, seed + 10 * p, extent=12.0) for p, n in enumerate(sizes_a)]
    b = [forest(n, seed + 10 * p + 5, extent=12.0) for p, n in enumerate(sizes_b)]
    return a, b


def pair_scan_batches(rows, tile):
    """What the consumers of the pair scan are compared on (tests/test_gpu_pair_scan.py and its host twin): the ragged
    batch with a pair without source and a pair without target, and one pair of rows + 1 queries against 2 tile + 1 targets
    with exact duplicates, query 0 a copy of a target whose lowest copy lies before the first tile edge and itself after it.
    -> [(sources, targets), ...] and that query's expected index"""
    dst, lowest = with_duplicates(forest(2 * tile + 1, 7), 8)
    late = np.flatnonzero((lowest < tile) & (np.arange(dst.shape[0]) >= tile))
    assert late.size
    src = forest(rows + 1, 9)
    src[0] = dst[late[-1]]
    return [ragged_pairs(31), ([src], [dst])], int(lowest[late[-1]])


def mutual_from_indices(idx, back, q_off, t_off):
    """the mutual mask from both directions' nearest-neighbour indices (numpy, concatenated, local to the pair)"""
    mask = np.zeros(idx.shape[0], bool)
    for p in range(q_off.shape[0] - 1):
        k = idx[q_off[p]:q_off[p + 1]]
        if k.size and t_off[p + 1] > t_off[p]:
            mask[q_off[p]:q_off[p + 1]] = back[t_off[p] + k] == np.arange(k.shape[0])
    return mask


def max_abs_after(clouds, transforms):
    """L: the largest coordinate magnitude of the float64 transformed clouds"""
    big = 0.0
    for c, m in zip(clouds, transforms):
        if c.shape[0]:
            big = max(big, float(np.abs(c.astype(np.float64) @ m[:3, :3].T + m[:3, 3]).max()))
    return big


def clear_of_tau(dist, taus, rtol=DIST_RTOL):
    """no finite distance lies within rtol * tau of a threshold tau: there the float32 route may count differently"""
    d = dist[np.isfinite(dist)]
    return all((np.abs(d - t) > rtol * t).all() for t in np.atleast_1d(taus))
