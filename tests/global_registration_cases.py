"""Seeded inputs, an exact case and the guard of the global-registration tests (`tests/test_global_registration_host.py`,
`tests/test_gpu_global_registration.py`).  Everything is float32 and read-only; what costs something on the host is
computed once (`functools.lru_cache`).

The module `hotformerloc_amd.global_registration` shares its name with the function the package exports, so it is taken from
`importlib.import_module` here (`GR`)."""
import functools
import importlib
import math

import numpy as np

from tests import fpfh_cases as fc

GR = importlib.import_module('hotformerloc_amd.global_registration')

TAU = 0.05                             # metres: far above the fp32 rounding of a true pair, far below the cloud's spacing
RATIO = 0.9
PURPOSE = dict(frac=0.6, seed=1, hypotheses=1024, ransac_seed=0)     # `purpose_figures` confirms them on the CPU
ANGLE_TOL_DEG, SHIFT_TOL = 0.01, 1e-3  # the recovered pose against the truth: 0.01 degrees, 1 mm


def truth():
    """(3, 4) float64: the 40 degree turn and 3 m shift of `fpfh_cases.rotation_z`"""
    r, t = fc.rotation_z()
    return np.concatenate([r, t[:, None]], 1)


def clouds():
    """(source, target): `three_planes` and its moved copy"""
    return fc.cloud_of('planes'), fc.cloud_of('planes_moved')


@functools.lru_cache(maxsize=None)
def rows(count, frac, seed):
    """(count, 2) int64 correspondences between the two clouds: source rows 0 .. count - 1 modulo the cloud (so that `count`
    may exceed it) against the same row of the target, `frac` of them redirected to a random OTHER target row"""
    n = clouds()[0].shape[0]
    rng = np.random.default_rng(seed)
    src = np.arange(count, dtype=np.int64) % n
    dst = src.copy()
    bad = rng.permutation(count)[:int(round(frac * count))]
    dst[bad] = (src[bad] + rng.integers(1, n, bad.shape[0])) % n
    out = np.stack([src, dst], 1)
    out.setflags(write=False)
    return out


def corrupted(frac, seed=PURPOSE['seed']):
    """(source, target, rows): every source row once, i -> i, `frac` of them redirected"""
    src, dst = clouds()
    return src, dst, rows(src.shape[0], frac, seed)


def true_rows(frac, seed=PURPOSE['seed']):
    """the mask of the rows of `corrupted` that were left i -> i"""
    r = rows(clouds()[0].shape[0], frac, seed)
    return r[:, 0] == r[:, 1]


def pose_error(m, ref=None):
    """(degrees, metres) between a (3+, 4) pose and the truth"""
    ref = truth() if ref is None else ref
    dr = m[:3, :3] @ ref[:3, :3].T
    # from the skew part: a pose that went through fp32 is orthonormal to 1e-7 only, which acos of the trace would magnify
    skew = 0.5 * np.array([dr[2, 1] - dr[1, 2], dr[0, 2] - dr[2, 0], dr[1, 0] - dr[0, 1]])
    return (math.degrees(math.atan2(float(np.linalg.norm(skew)), (np.trace(dr) - 1.0) / 2.0)),
            float(np.linalg.norm(m[:3, 3] - ref[:3, 3])))


# --------------------------------------------------------------------------------------------------------------- exact case
EXACT_OFFSETS = ((0, 0, 0), (1, 0, 0), (0, -1, 0), (1, 1, 1), (2, 0, 0), (1, 2, 0), (-2, 0, 1), (0, 1, -2), (2, 2, 0),
                 (0, 0, 3), (-1, -2, 2), (4, 0, 0))                    # squared lengths 0 1 1 3 4 5 5 5 8 9 9 16
EXACT_TAU = np.sqrt(np.float32(5.0))   # d == tau for the offsets of squared length 5: kept by the inclusive rule
EXACT_TAU_BELOW = np.nextafter(EXACT_TAU, np.float32(0.0))             # those offsets lie one fp32 step beyond it: dropped


def _integer_poses():
    """four integer poses, rotations by multiples of 90 degrees plus integer shifts, and one of NaNs"""
    rz = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    rx = [[1, 0, 0], [0, 0, -1], [0, 1, 0]]
    ry2 = [[-1, 0, 0], [0, 1, 0], [0, 0, -1]]
    eye = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    return [(rz, (1, 2, 3)), (eye, (0, 0, 0)), (rx, (-4, 0, 5)), (ry2, (7, -7, 1))]


@functools.lru_cache(maxsize=None)
def exact_case():
    """(source, target, rows, poses (1, 5, 3, 4) float32, counts {tau: (5,) int}): 48 integer source points, each paired with
    its image under the first pose plus one of `EXACT_OFFSETS`; the counts are by Python integers, -1 for the pose of NaNs"""
    rng = np.random.default_rng(7)
    src = rng.integers(-8, 9, (48, 3))
    (r0, t0), offsets = _integer_poses()[0], EXACT_OFFSETS
    dst = np.array([[sum(r0[a][b] * int(p[b]) for b in range(3)) + t0[a] + offsets[i % len(offsets)][a] for a in range(3)]
                    for i, p in enumerate(src)])
    counts = {}
    for name, limit in (('at', 5), ('below', 4)):                      # d2 <= 5 with tau = sqrtf(5), d2 <= 4 one step below
        per_pose = []
        for r, t in _integer_poses():
            n = 0
            for p, q in zip(src.tolist(), dst.tolist()):
                moved = [sum(r[a][b] * p[b] for b in range(3)) + t[a] for a in range(3)]
                n += sum((moved[a] - q[a]) ** 2 for a in range(3)) <= limit
            per_pose.append(n)
        counts[name] = np.array(per_pose + [-1])
    poses = np.full((1, 5, 3, 4), np.nan, np.float32)
    for h, (r, t) in enumerate(_integer_poses()):
        poses[0, h, :, :3], poses[0, h, :, 3] = r, t
    pairs = np.stack([np.arange(48), np.arange(48)], 1).astype(np.int64)
    return src.astype(np.float32), dst.astype(np.float32), pairs, poses, counts


# -------------------------------------------------------------------------------------------------------------------- guard
def _triples(p, q, draws):
    ok = (p.shape[0] >= 3) & (draws[:, 0] != draws[:, 1]) & (draws[:, 0] != draws[:, 2]) & (draws[:, 1] != draws[:, 2])
    at = np.nonzero(ok)[0]
    return at, [p[draws[at, k]].astype(np.float64) for k in range(3)], [q[draws[at, k]].astype(np.float64) for k in range(3)]


def rank_ratios(p, q, draws):
    """(H,) float64: second over largest singular value of H = sum (p - mean p)(q - mean q)^T of every drawn triple by
    `numpy.linalg.svd`, NaN where the triple has fewer than three distinct rows"""
    out = np.full(draws.shape[0], np.nan)
    at, ps, qs = _triples(p, q, draws)
    if at.shape[0]:
        pc, qc = np.stack(ps, 1), np.stack(qs, 1)                      # (n, 3 points, 3)
        h = np.einsum('nka,nkb->nab', pc - pc.mean(1, keepdims=True), qc - qc.mean(1, keepdims=True))
        s = np.linalg.svd(h, compute_uv=False)
        with np.errstate(all='ignore'):
            out[at] = s[:, 1] / s[:, 0]
    return out


def guard_draws(p, q, draws, ratio=RATIO, rel=1e-9):
    """asserts that no edge ratio and no rank ratio of a drawn triple lies within `rel` relative of its threshold"""
    at, ps, qs = _triples(p, q, draws)
    rho2 = np.float64(ratio) * np.float64(ratio)
    passed = np.ones(at.shape[0], bool)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        ls, lt = ((ps[a] - ps[b]) ** 2).sum(1), ((qs[a] - qs[b]) ** 2).sum(1)
        for x, y in ((ls, rho2 * lt), (lt, rho2 * ls)):
            scale = np.maximum(x, y)
            assert not ((np.abs(x - y) <= rel * scale) & (scale > 0)).any(), 'an edge ratio at its threshold'
            passed &= x >= y
    ratios = rank_ratios(p, q, draws)[at][passed]
    assert not (np.abs(ratios - GR.RANK_TOL) <= rel * GR.RANK_TOL).any(), 'a rank ratio at its threshold'
    # a ratio between the tolerance and what 12 Jacobi sweeps resolve would be decided by rounding as well
    assert not ((ratios > 0) & (ratios < 1e-9)).any(), 'a rank ratio that rounding decides'


def guard_d2(p, q, poses, tau, ulps=4):
    """asserts that no host d2 of the correspondences under the finite poses (H, 12) lies within `ulps` fp32 ulps of D2"""
    d2_max = GR.inlier_d2(tau)
    finite = np.isfinite(poses).all(1)
    d2 = GR._host_d2(p, q, np.ascontiguousarray(poses[finite]))
    assert not (np.abs(d2.astype(np.float64) - np.float64(d2_max)) <= ulps * np.float64(np.spacing(d2_max))).any(), \
        'a d2 within %d ulps of D2' % ulps


def gathered(src, dst, pairs):
    return src[pairs[:, 0]], dst[pairs[:, 1]]


# ------------------------------------------------------------------------------------------------------------------ purpose
@functools.lru_cache(maxsize=None)
def purpose_figures():
    """the host RANSAC on `corrupted(0.6)` with the Philox draws, H = 1024: dict(result, valid, good) -- `good` the number
    of hypotheses with more than half the true inliers.  The guard is asserted on the way."""
    src, dst, pairs = corrupted(PURPOSE['frac'])
    p, q = gathered(src, dst, pairs)
    poses, valid, draws = GR.ransac_hypotheses_host([src], [dst], [pairs], hypotheses=PURPOSE['hypotheses'],
                                                    seed=PURPOSE['ransac_seed'], edge_length_ratio=RATIO)
    guard_draws(p, q, draws[0])
    guard_d2(p, q, poses[0].reshape(-1, 12), TAU)
    counts = GR.score_hypotheses_host([src], [dst], [pairs], poses, TAU, valid)[0]
    result = GR.ransac_registration_host([src], [dst], [pairs], max_correspondence_distance=TAU,
                                         hypotheses=PURPOSE['hypotheses'], seed=PURPOSE['ransac_seed'],
                                         edge_length_ratio=RATIO)
    return dict(result=result, valid=int(valid.sum()), good=int((counts > 0.5 * true_rows(PURPOSE['frac']).sum()).sum()),
                counts=counts)
