"""Clouds, normals and independent transcriptions for the FPFH and feature-correspondence tests
(`tests/test_fpfh_host.py`, `tests/test_gpu_fpfh.py`).  Everything is seeded and float32; what costs something on the host
is computed once (`functools.lru_cache`) and must not be written to."""
import functools
import math

import numpy as np

from hotformerloc_amd import fpfh, normals
from tests import normals_cases as nc

VIEW = (20.0, 20.0, 20.0)              # the viewpoint the normals of the plane clouds are turned to


def three_planes(n_per_face=226, seed=4, noise=0.02):
    """3 x 226 = 678 points on three noisy planes that meet in a corner"""
    pts, _ = nc._corner_points(n_per_face, np.random.default_rng(seed), noise)
    return pts.astype(np.float32)


def planes_and_outliers(seed=4):
    """700 points: the three planes, two more points on them, and 20 far outliers 200 m to 400 m away"""
    rng = np.random.default_rng(seed + 100)
    extra, _ = nc._corner_points(1, rng, 0.01)
    far = rng.uniform(200.0, 400.0, (20, 3)) * rng.choice([-1.0, 1.0], (20, 3))
    return np.concatenate([three_planes(seed=seed), extra[:2].astype(np.float32), far.astype(np.float32)])


def lattice():
    """the 5 x 5 x 5 integer lattice: every distance exact, ties at the k-th place; normals along the axes, the axis chosen
    by (x + 2 y + 3 z) mod 3 and the sign by x + y + z: features at exactly 0 and +-1, directions at multiples of pi / 2
    and at (0, 0)"""
    g = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(5), indexing='ij'), -1).reshape(-1, 3)
    nrm = np.zeros((125, 3), np.float32)
    nrm[np.arange(125), (g[:, 0] + 2 * g[:, 1] + 3 * g[:, 2]) % 3] = np.where(g.sum(1) % 2 == 0, 1.0, -1.0)
    return g.astype(np.float32), nrm


def duplicated():
    """a noisy plane of 150 points, 12 more copies of its first point and 2 more of each of its next four"""
    p = nc.noisy_plane(150, 3)
    return np.concatenate([p, np.repeat(p[:1], 12, axis=0), np.repeat(p[1:5], 2, axis=0)])


def rotation_z(deg=40.0, shift=(3.0, 0.0, 0.0)):
    a = math.radians(deg)
    r = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    return r, np.asarray(shift, np.float64)


def moved(cloud, r, t):
    return (cloud.astype(np.float64) @ r.T + t).astype(np.float32)


@functools.lru_cache(maxsize=None)
def host_normals(key, nb=30, view=VIEW):
    """the numpy normals of a named cloud, shared and read-only"""
    out = normals.estimate_normals_host([cloud_of(key)], nb, viewpoint=None if view is None else np.array(view))[0]
    out.setflags(write=False)
    return out


CLOUDS = {
    'one': lambda: nc.noisy_plane(1, 11),
    'two': lambda: nc.noisy_plane(2, 12),
    'plane37': lambda: nc.noisy_plane(37, 13),
    'planes700': planes_and_outliers,
    'planes': three_planes,
    'planes_moved': lambda: moved(three_planes(), *rotation_z()),
    'duplicated': duplicated,
    'collinear': nc.collinear,
}


@functools.lru_cache(maxsize=None)
def cloud_of(key):
    c = CLOUDS[key]()
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def host_fpfh(key, nb=30):
    """(fpfh, hist, pairs) of a named cloud with its `host_normals`, shared and read-only"""
    view = VIEW if key != 'planes_moved' else tuple(rotation_z()[0] @ np.array(VIEW) + rotation_z()[1])
    out = fpfh.compute_fpfh_host([cloud_of(key)], [host_normals(key, nb, view)], nb, return_histograms=True)
    res = tuple(o[0] for o in out)
    for r in res:
        r.setflags(write=False)
    return res


# ------------------------------------------------------------------------------ the definition once more, one pair at a time
def theta_bin_scalar(x, y):
    if x == 0.0 and y == 0.0:
        return 5
    count = 0
    for k in range(1, 11):
        c, s = float(fpfh.THETA_TABLE[k - 1, 0]), float(fpfh.THETA_TABLE[k - 1, 1])
        if y < 0.0:
            count += 1 if (k <= 5 and c * y >= s * x) else 0
        else:
            count += 1 if (k <= 5 or c * y >= s * x) else 0
    return count


def linear_bin_scalar(f):
    return int(min(max(math.floor((11.0 * (f + 1.0)) / 2.0), 0), 10))


def pair_bins_scalar(pi, ni, pj, nj):
    """None where the pair is skipped, else (theta bin, f2 bin, f3 bin): Python floats are float64, one rounding each"""
    pi, ni, pj, nj = ([float(v) for v in a] for a in (pi, ni, pj, nj))

    def dot(a, b):
        return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    dp = [pj[a] - pi[a] for a in range(3)]
    d = math.sqrt(dot(dp, dp))
    if not d > 0.0:
        return None
    a1, a2 = dot(ni, dp) / d, dot(nj, dp) / d
    if abs(a1) < abs(a2):
        src, dst, dp, f3 = nj, ni, [-v for v in dp], -a2
    else:
        src, dst, f3 = ni, nj, a1
    v = cross(dp, src)
    vn = math.sqrt(dot(v, v))
    if not vn > 0.0:
        return None
    v = [c / vn for c in v]
    w = cross(src, v)
    return theta_bin_scalar(dot(src, dst), dot(w, dst)), linear_bin_scalar(dot(v, dst)), linear_bin_scalar(f3)


def spfh_scalar(cloud, nrm, nb):
    """(hist (n, 33) int32, pairs (n,) int32) by two Python loops over the points"""
    n = cloud.shape[0]
    k = min(nb, n)
    hist, pairs = np.zeros((n, 33), np.int32), np.zeros(n, np.int32)
    has = np.isfinite(nrm).all(1) & (nrm != 0).any(1)
    for i in range(n):
        d = cloud - cloud[i]                                       # float32
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        r2 = np.sort(d2)[k - 1]
        for j in np.nonzero(d2 <= r2)[0]:
            if j == i or not (has[i] and has[j]):
                continue
            bins = pair_bins_scalar(cloud[i], nrm[i], cloud[j], nrm[j])
            if bins is None:
                continue
            for g, b in enumerate(bins):
                hist[i, 11 * g + b] += 1
            pairs[i] += 1
    return hist, pairs


# ------------------------------------------------------------------------------------------------ feature rows
PAIR_SIZES = ((0, 5), (5, 0), (1, 1), (3, 1030), (1030, 3), (600, 700))


@functools.lru_cache(maxsize=None)
def integer_features(dim, seed=0):
    """(sources, targets): lists of (n, dim) float32 rows of `PAIR_SIZES` with integer entries 0..7 drawn from a small pool of
    distinct rows, so that most rows occur several times and every squared distance is exact: the tie rule decides"""
    rng = np.random.default_rng(seed + dim)
    out = ([], [])
    for ns, nt in PAIR_SIZES:
        pool = rng.integers(0, 8, (24, dim)).astype(np.float32)
        for side, n in zip(out, (ns, nt)):
            rows = pool[rng.integers(0, pool.shape[0], n)]
            rows.setflags(write=False)
            side.append(rows)
    return out


def ulp_gap_rows(q, t, ulps=4):
    """the mask of the rows of q whose best and second-best host d2 against t differ by more than `ulps` fp32 ulps"""
    d2 = np.sort(fpfh._host_feature_d2(q, t), axis=1)
    return (d2[:, 1] - d2[:, 0]) > ulps * np.spacing(d2[:, 1])
