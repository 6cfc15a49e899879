"""Clouds, an independent transcription, the guards and the shared host results of the ISS keypoint tests
(`tests/test_keypoints_host.py`, `tests/test_gpu_keypoints.py`).  Everything is seeded and float32; what costs something on
the host is computed once (`functools.lru_cache`) and must not be written to."""
import functools

import numpy as np

import hotformerloc_amd as hfl
from hotformerloc_amd import keypoints as kp
from hotformerloc_amd.global_registration import inlier_d2
from tests import fpfh_cases as fc
from tests import radius_cases as rc

NAMED = ('one', 'two', 'plane37', 'duplicated', 'collinear', 'planes', 'planes_moved', 'planes700')
SIZES = (1, 2, 4, 255, 256, 257)       # below `min_neighbors`, and round the 256 threads of a workgroup
RAGGED = (1, 257, 'plane37', 'planes')  # sizes 1, 257, 37 and 678 in one call
# 'collinear' is left out of the comparisons of saliency VALUES AND ZEROS: its points lie on a line up to their fp32
# rounding, so on the host 34 of its 37 rows with five neighbours have l1 == 0 exactly -- AT the threshold l0 < gamma_32 l1
# -- and the rest have an l1 that is rounding: `guard_gamma` fails on it, as it must.  Its counts, its selection for a given
# saliency and its keypoints from the device's own saliency are compared like every other cloud's.
GUARDED = tuple(k for k in NAMED if k != 'collinear') + SIZES
RADII = ((1.5, 1.0), (1.0, 0.7), (2.0, 1.5))                          # (salient_radius, non_max_radius)
PLANES_KEYPOINTS = {(1.5, 1.0): 38, (1.0, 0.7): 52, (2.0, 1.5): 16}  # measured on the host route
GUARD_REL = 1e-9
VALUE_REL = 1e-12                      # of l2: three orders over a Jacobi's error of about 1e-15 l2
LATTICE_RADIUS = float(np.sqrt(np.float32(5.0)))                      # fp32 sqrt 5: d2 == 5 is inside, inclusively
LATTICE_RADIUS_BELOW = float(np.nextafter(np.sqrt(np.float32(5.0)), np.float32(0.0)))


def cloud_of(key):
    return rc.cloud_of(key)


def integer_saliency(key, seed=0):
    """(n,) float32 drawn from {0, 1, 2, 3}: ties everywhere, the index rule decides"""
    n = cloud_of(key).shape[0]
    s = np.random.default_rng(seed + n).integers(0, 4, n).astype(np.float32)
    s.setflags(write=False)
    return s


# ------------------------------------------------------------------------------ the definition once more, one point at a time
def _d2(cloud, i):
    d = cloud - cloud[i]                                           # float32
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def saliency_scalar(cloud, salient_radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
    """steps 1 to 4 by a Python loop -> (saliency (n,) float64 BEFORE the rounding to fp32, counts (n,) int32, eigenvalues
    (n, 3) float64 ascending, NaN below three neighbours): the covariance about the neighbourhood's mean in float64 and
    numpy's symmetric eigen-solver, no code of the package but `inlier_d2`"""
    n, r2 = cloud.shape[0], inlier_d2(salient_radius)
    c64 = cloud.astype(np.float64)
    sal, counts, lam = np.zeros(n), np.zeros(n, np.int32), np.full((n, 3), np.nan)
    for i in range(n):
        idx = np.nonzero(_d2(cloud, i) <= r2)[0]
        counts[i] = idx.shape[0]
        if idx.shape[0] < 3:
            continue
        e = c64[idx] - c64[idx].mean(0)
        lam[i] = np.maximum(np.linalg.eigvalsh(e.T @ e / idx.shape[0]), 0.0)
        if idx.shape[0] >= min_neighbors and lam[i, 1] < gamma_21 * lam[i, 2] and lam[i, 0] < gamma_32 * lam[i, 1]:
            sal[i] = lam[i, 0]
    return sal, counts, lam


def select_scalar(cloud, saliency, non_max_radius, min_neighbors=5):
    """step 5 by two Python loops -> the keypoint indices, ascending, int64"""
    n, r2 = cloud.shape[0], inlier_d2(non_max_radius)
    out = []
    for i in range(n):
        if not saliency[i] > 0:
            continue
        ball = np.nonzero(_d2(cloud, i) <= r2)[0]
        beaten = any(saliency[j] > saliency[i] or (saliency[j] == saliency[i] and j < i) for j in ball)
        if ball.shape[0] >= min_neighbors and not beaten:
            out.append(i)
    return np.array(out, np.int64)


def lattice_select_exact(saliency, limit, min_neighbors=5):
    """step 5 on the 5 x 5 x 5 integer lattice with d2 <= `limit` on Python integers: no floating point at all"""
    g = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(5), indexing='ij'), -1).reshape(-1, 3).tolist()
    s = [int(v) for v in saliency]
    out = []
    for i, p in enumerate(g):
        ball = [j for j, q in enumerate(g) if sum((a - b) ** 2 for a, b in zip(p, q)) <= limit]
        if s[i] > 0 and len(ball) >= min_neighbors and not any(s[j] > s[i] or (s[j] == s[i] and j < i) for j in ball):
            out.append(i)
    return np.array(out, np.int64)


# ------------------------------------------------------------------------------------------------ shared host results
@functools.lru_cache(maxsize=None)
def host_saliency(key, salient_radius, min_neighbors=5):
    """(saliency float32, counts int32, eigenvalues (n, 3) float64) of the numpy route, shared and read-only"""
    cloud = cloud_of(key)
    sal, counts = hfl.iss_saliency_host([cloud], salient_radius, min_neighbors=min_neighbors, return_counts=True)
    lam = hfl.estimate_normals_host([cloud], None, radius=salient_radius, return_eigenvalues=True)[1]
    res = (sal[0], counts[0], lam[0])
    for r in res:
        r.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def host_keypoints(key, salient_radius, non_max_radius):
    out = hfl.iss_select_host([cloud_of(key)], [host_saliency(key, salient_radius)[0]], non_max_radius)[0]
    out.setflags(write=False)
    return out


# -------------------------------------------------------------------------------------------------------------------- guards
def _close(a, b, rel=GUARD_REL):
    return np.abs(a - b) <= rel * np.maximum(np.abs(a), np.abs(b))    # 0 against 0 is close


def guard_gamma(key, salient_radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
    """asserts on the host eigenvalues that NO row with `min_neighbors` points and eigenvalues lies within `GUARD_REL`
    relative of either gamma threshold: then the zero pattern of the saliency does not hang on a rounding"""
    _, counts, lam = host_saliency(key, salient_radius, min_neighbors)
    rows = np.isfinite(lam).all(1) & (counts >= min_neighbors)
    l0, l1, l2 = lam[rows, 0], lam[rows, 1], lam[rows, 2]
    assert not _close(l1, gamma_21 * l2).any(), '%s: an l1 at gamma_21 l2' % (key,)
    assert not _close(l0, gamma_32 * l1).any(), '%s: an l0 at gamma_32 l1' % (key,)


def guard_ties(key, salient_radius, non_max_radius):
    """asserts that NO two points within `non_max_radius` of one another have host float64 saliencies that agree within
    `GUARD_REL` relative yet round to different fp32 values: then the selection does not hang on the order of a sum"""
    cloud = cloud_of(key)
    s32, _, lam = host_saliency(key, salient_radius)
    s64 = np.where(s32 > 0, lam[:, 0], 0.0)
    r2 = inlier_d2(non_max_radius)
    for i in np.nonzero(s32 > 0)[0]:
        ball = np.nonzero((_d2(cloud, i) <= r2) & (s32 > 0))[0]
        bad = _close(s64[ball], s64[i]) & (s32[ball] != s32[i])
        assert not bad.any(), '%s: points %d and %s' % (key, i, ball[bad])


def fp32_ties(key, salient_radius, non_max_radius):
    """the number of pairs i < j within `non_max_radius` whose positive host saliencies are bit-equal in fp32"""
    cloud, s32 = cloud_of(key), host_saliency(key, salient_radius)[0]
    r2 = inlier_d2(non_max_radius)
    return sum(int(((_d2(cloud, i)[i + 1:] <= r2) & (s32[i + 1:] == s32[i])).sum()) for i in np.nonzero(s32 > 0)[0])


def value_bound(key, salient_radius):
    """(n,) float64: one fp32 spacing of the host saliency + `VALUE_REL` x the host's l2 (0 where there are no eigenvalues)"""
    s32, _, lam = host_saliency(key, salient_radius)
    return np.spacing(s32).astype(np.float64) + VALUE_REL * np.nan_to_num(lam[:, 2])


assert kp.GAMMA_21 == 0.975 and kp.GAMMA_32 == 0.975 and kp.MIN_NEIGHBOURS == 5      # the defaults the cases were measured at
