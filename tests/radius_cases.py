"""Clouds, an independent transcription and the density case of the radius / hybrid neighbourhood tests
(`tests/test_radius_neighbourhoods_host.py`, `tests/test_gpu_radius_neighbourhoods.py`).  Everything is seeded and float32;
what costs something on the host is computed once (`functools.lru_cache`) and must not be written to."""
import functools

import numpy as np

from hotformerloc_amd import fpfh, normals
from hotformerloc_amd.global_registration import inlier_d2
from tests import fpfh_cases as fc
from tests import normals_cases as nc

KEYS = ('plane37', 'planes', 'planes700', 'duplicated', 'collinear')
# a radius per cloud at which some points have fewer than 30 points within it and others more: the three planes hold 3.5
# points a square metre (44 in a disc of 2 m, a quarter of that at a corner), 'plane37' 0.37, 'duplicated' 1.5, and
# 'collinear' 40 points on 18 m
RADIUS = {'one': 1.0, 'two': 1.0, 'plane37': 7.0, 'planes': 2.0, 'planes700': 2.0, 'duplicated': 3.5, 'collinear': 8.0}
LATTICE_RADII = (1.0, float(np.nextafter(np.float32(np.sqrt(2.0)), np.float32(np.inf))), 2.0)
# the points of the integer lattice within 1, sqrt 2 and 2 of an interior point, itself included: 1 + 6, + 12, + 8 + 6
LATTICE_INTERIOR = (7, 19, 33)
MODES = ('hybrid', 'radius_only')


def nb_of(mode, nb=30):
    return nb if mode == 'hybrid' else None


def cloud_of(key):
    return nc.noisy_plane(key, 100 + key) if isinstance(key, int) else fc.cloud_of(key)


def radius_of(key):
    return 1.5 if isinstance(key, int) else RADIUS[key]


def lattice_counts(radius):
    """the exact number of lattice points within `radius` (<=, on integers) of every point of the 5 x 5 x 5 lattice"""
    g = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(5), indexing='ij'), -1).reshape(-1, 3)
    d2 = ((g[:, None, :] - g[None, :, :]) ** 2).sum(-1)
    return (d2 <= int(np.floor(radius * radius + 1e-6))).sum(1).astype(np.int32)


# ------------------------------------------------------------------------------ the definition once more, one point at a time
def members_scalar(cloud, nb, radius):
    """N(i) of every point as index arrays, by a Python loop: the fp32 d2 of the definition, the k-th smallest by a full
    sort, the threshold by `inlier_d2`"""
    n = cloud.shape[0]
    cap = None if radius is None else inlier_d2(radius)
    out = []
    for i in range(n):
        d = cloud - cloud[i]                                       # float32
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        r2 = np.float32(np.inf) if nb is None else np.sort(d2)[min(nb, n) - 1]
        if cap is not None and cap < r2:
            r2 = cap
        out.append(np.nonzero(d2 <= r2)[0])
    return out


def zero_normal_scalar(cloud, members):
    """True where the definition gives no normal: fewer than three neighbours, or the neighbours' covariance about the point
    has rank < 2 (numpy's symmetric eigen-solver on the float64 covariance; the clouds of these tests lie far from the
    1e-12 threshold on either side, which `rank_margin` reports)"""
    zero, margin = np.zeros(len(members), bool), np.inf
    c64 = cloud.astype(np.float64)
    for i, idx in enumerate(members):
        if idx.shape[0] < 3:
            zero[i] = True
            continue
        e = c64[idx] - c64[i]
        mu = e.mean(0)
        lam = np.linalg.eigvalsh(e.T @ e / idx.shape[0] - np.outer(mu, mu))
        ratio = max(lam[1], 0.0) / lam[2] if lam[2] > 0.0 else 0.0
        zero[i] = not ratio > normals.RANK_TOL
        if ratio > 0.0:
            margin = min(margin, abs(np.log10(ratio) + 12.0))
    return zero, margin


def spfh_scalar(cloud, nrm, members):
    """(hist (n, 33) int32, pairs (n,) int32) over given neighbourhoods, pair by pair with `fpfh_cases.pair_bins_scalar`"""
    n = cloud.shape[0]
    hist, pairs = np.zeros((n, 33), np.int32), np.zeros(n, np.int32)
    has = np.isfinite(nrm).all(1) & (nrm != 0).any(1)
    for i, idx in enumerate(members):
        for j in idx:
            if j == i or not (has[i] and has[j]):
                continue
            bins = fc.pair_bins_scalar(cloud[i], nrm[i], cloud[j], nrm[j])
            if bins is None:
                continue
            for g, b in enumerate(bins):
                hist[i, 11 * g + b] += 1
            pairs[i] += 1
    return hist, pairs


# ------------------------------------------------------------------------------------------------ shared host results
@functools.lru_cache(maxsize=None)
def host_normals(key, mode, nb=30, radius=None):
    """(normals, curvature, counts, eigenvalues) of the numpy route, shared and read-only"""
    out = normals.estimate_normals_host([cloud_of(key)], nb_of(mode, nb), radius=radius_of(key) if radius is None else radius,
                                        viewpoint=np.array(fc.VIEW), return_curvature=True, return_counts=True,
                                        return_eigenvalues=True)
    res = tuple(o[0] for o in out)
    for r in res:
        r.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def host_fpfh(key, mode, nb=30, radius=None):
    """(fpfh, hist, pairs) of the numpy route on `host_normals`, shared and read-only"""
    r = radius_of(key) if radius is None else radius
    out = fpfh.compute_fpfh_host([cloud_of(key)], [host_normals(key, mode, nb, radius)[0]], nb_of(mode, nb), radius=r,
                                 return_histograms=True)
    res = tuple(o[0] for o in out)
    for r in res:
        r.setflags(write=False)
    return res


# ------------------------------------------------------------------------------------------------ the density case
DENSITY_SEEDS = ((4, 54), (5, 55), (6, 56))
DENSITY_RADIUS = 1.7
DENSITY_NB = 30


@functools.lru_cache(maxsize=None)
def density_pair(seeds):
    """(source, target, T): the corner of three planes sampled at 226 points a face, and an INDEPENDENT sample of 904 a
    face (a quarter of the spacing in area) moved by `fpfh_cases.rotation_z()`; T the 4 x 4 truth, source -> target"""
    src = fc.three_planes(226, seeds[0])
    r, t = fc.rotation_z()
    dst = fc.moved(fc.three_planes(904, seeds[1]), r, t)
    truth = np.eye(4)
    truth[:3, :3], truth[:3, 3] = r, t
    for a in (src, dst):
        a.setflags(write=False)
    return src, dst, truth


def density_errors(transform, truth):
    """(rotation error in degrees, |T[:3, 3] - t_true| in metres)"""
    m = np.asarray(transform, np.float64)
    cos = np.clip((np.trace(m[:3, :3] @ truth[:3, :3].T) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.degrees(np.arccos(cos))), float(np.linalg.norm(m[:3, 3] - truth[:3, 3]))
