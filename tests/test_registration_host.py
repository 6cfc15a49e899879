"""`icp_refine_host` and its single-step twins (hotformerloc_amd/registration.py) against closed forms: a known rigid motion,
an exact inlier count, `numpy.linalg.svd`.  No GPU.  Bounds: the exact family recovers G to 1e-6 -- the source is the float32
rounding of inv(G) . target (half an ulp32 at 8 m is 5e-7 m per point) and the least-squares pose of 1025 well-spread points
averages that down; rotations and translations against numpy's SVD to 1e-12, three orders above float64 rounding of
well-conditioned 3 x 3 problems with coordinates of a few metres."""
import os

import numpy as np
import pytest

import hotformerloc_amd
import registration_cases as rc
from hotformerloc_amd import (evaluate_registration_host, icp_correspondences_host, icp_refine_host, kabsch_update_host, ops,
                              registration as reg)

_CACHE = {}


def family(name):
    """(src, dst, G, max_dist, trace, result) of a family, computed once"""
    if name not in _CACHE:
        src, dst, g, max_dist = rc.pair(rc.EXACT if name == 'exact' else rc.NOISY)
        _CACHE[name] = (src, dst, g, max_dist, rc.trace(src, dst, max_dist), icp_refine_host([src], [dst],
                        max_correspondence_distance=max_dist))
    return _CACHE[name]


def same_as_trace(result, tr, p=0):
    assert result.status[p] == tr['status'] and result.iterations[p] == tr['iterations']
    assert result.fitness[p] == tr['fitness'] or (np.isnan(result.fitness[p]) and np.isnan(tr['fitness']))
    assert np.abs(result.transforms[p] - tr['transform']).max() <= 1e-12
    assert abs(result.inlier_rmse[p] - tr['rmse']) <= 1e-12 or (np.isnan(result.inlier_rmse[p]) and np.isnan(tr['rmse']))


def test_exact_family_finds_the_motion():
    src, dst, g, max_dist, tr, r = family('exact')
    same_as_trace(r, tr)
    assert r.transforms.shape == (1, 4, 4) and r.transforms.dtype == np.float64
    assert r.status[0] == reg.CONVERGED and r.fitness[0] == 1.0
    assert np.abs(r.transforms[0] - g).max() <= 1e-6
    assert np.array_equal(r.transforms[0, 3], [0.0, 0.0, 0.0, 1.0])
    assert r.iterations[0] == 2                                          # one update lands on G, the second changes nothing
    assert r.inlier_rmse[0] < 1e-6


def test_outliers_do_not_count():
    src, dst, g, max_dist, _, _ = family('exact')
    src = np.concatenate([src, rc.far_points(300, 5)])
    tr = rc.trace(src, dst, max_dist)
    r = icp_refine_host([src], [dst], max_correspondence_distance=max_dist)
    same_as_trace(r, tr)
    assert r.fitness[0] == 1025 / 1325 and r.status[0] == reg.CONVERGED
    assert np.abs(r.transforms[0] - g).max() <= 1e-6


def test_noisy_family_takes_several_updates():
    src, dst, g, max_dist, tr, r = family('noisy')
    same_as_trace(r, tr)
    assert r.status[0] == reg.CONVERGED and r.iterations[0] > 2
    assert tr['history'][0][0] < 1.0                                     # an outlier exists at k = 0
    rmse = [h[1] for h in tr['history']]
    assert all(b <= a for a, b in zip(rmse[1:], rmse[2:]))               # non-increasing after k = 1
    # sigma = 0.02 m of noise on 1025 points: the pose is G to a few sigma / sqrt(n)
    assert np.abs(r.transforms[0] - g).max() <= 5e-3 and abs(r.inlier_rmse[0] - 0.02 * np.sqrt(3.0)) < 5e-3


def test_float32_and_float64_routes_choose_the_same_correspondences():
    src, dst, g, max_dist, tr, _ = family('noisy')
    pose = np.eye(4)
    for k, (_, _, idx, inl) in enumerate(tr['history'][:3]):
        moved = src.astype(np.float64) @ pose[:3, :3].T + pose[:3, 3]
        d = np.sqrt(((moved[:, None, :] - dst.astype(np.float64)[None, :, :]) ** 2).sum(-1))
        assert np.array_equal(d.argmin(1), idx) and np.array_equal(d.min(1) <= max_dist, inl)
        r, t, _ = kabsch_update_host(icp_correspondences_host([src], [dst], pose[None], max_dist)[3])
        step = np.eye(4)
        step[:3, :3], step[:3, 3] = r[0], t[0]
        pose = step @ pose


def test_kabsch_update_against_numpy_svd():
    sums, kinds = rc.kabsch_cases()
    r, t, status = kabsch_update_host(sums)
    assert r.shape == (len(kinds), 3, 3) and t.shape == (len(kinds), 3) and status.dtype == np.int32
    for k, kind in enumerate(kinds):
        if kind == 'line':
            assert status[k] == reg.DEGENERATE
        elif kind == 'few':
            assert status[k] == reg.TOO_FEW
        if kind in ('line', 'few'):
            assert np.array_equal(r[k], np.eye(3)) and np.array_equal(t[k], np.zeros(3))
            continue
        want_r, want_t = rc.kabsch_by_svd(sums[k])
        assert status[k] == reg.RUNNING
        assert np.abs(r[k] - want_r).max() <= 1e-12 and np.abs(t[k] - want_t).max() <= 1e-12, kind
        assert np.abs(r[k].T @ r[k] - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(r[k]) - 1.0) <= 1e-12, kind
    planar = sums[list(kinds).index('planar')]
    h = planar[7:16].reshape(3, 3) - np.outer(planar[1:4], planar[4:7]) / planar[0]
    u, _, vt = np.linalg.svd(h)
    assert np.linalg.det(vt.T @ u.T) < 0.0                               # the unconstrained optimum is a reflection


def test_collinear_points_are_degenerate():
    line = (np.linspace(-5.0, 5.0, 41)[:, None] * np.array([[1.0, 0.5, 0.25]])).astype(np.float32)
    init = rc.rigid(0.5, 0.01)
    r = icp_refine_host([line], [line], init=init[None], max_correspondence_distance=1.0)
    assert r.status[0] == reg.DEGENERATE and r.iterations[0] == 0
    assert np.array_equal(r.transforms[0], init) and r.fitness[0] == 1.0 and np.isfinite(r.inlier_rmse[0])


def test_two_inliers_are_too_few():
    dst = rc.target(500)
    src = np.concatenate([dst[:2] + np.float32(0.01), rc.far_points(20, 3)])
    r = icp_refine_host([src], [dst], max_correspondence_distance=0.5)
    assert r.status[0] == reg.TOO_FEW and r.iterations[0] == 0 and r.fitness[0] == 2 / 22 and np.isnan(r.inlier_rmse[0])
    assert np.array_equal(r.transforms[0], np.eye(4))
    both = icp_refine_host([src, src], [dst, dst], max_correspondence_distance=0.5, min_correspondences=2)
    assert (both.status != reg.TOO_FEW).all()


def test_empty_clouds():
    dst = rc.target(100)
    none = np.zeros((0, 3), np.float32)
    r = icp_refine_host([none, dst[:10], dst[:10]], [dst, none, dst], max_correspondence_distance=0.5, max_iterations=2)
    assert r.status[0] == reg.TOO_FEW and np.isnan(r.fitness[0]) and np.isnan(r.inlier_rmse[0])
    assert r.status[1] == reg.TOO_FEW and r.fitness[1] == 0.0 and np.isnan(r.inlier_rmse[1])
    assert r.status[2] != reg.TOO_FEW and r.fitness[2] == 1.0


def test_zero_iterations_return_init_with_its_evaluation():
    src, dst, g, max_dist, tr, _ = family('noisy')
    init = rc.rigid(2.0, 0.1)
    r = icp_refine_host([src], [dst], init=init[None], max_correspondence_distance=max_dist, max_iterations=0)
    assert r.status[0] == reg.MAX_ITERATIONS and r.iterations[0] == 0 and np.array_equal(r.transforms[0], init)
    fitness, rmse = evaluate_registration_host([src], [dst], init[None], max_dist)
    assert fitness[0] == r.fitness[0] and rmse[0] == r.inlier_rmse[0]
    # and iteration 0 of a full run is the evaluation of the identity
    fitness, rmse = evaluate_registration_host([src], [dst], np.eye(4)[None], max_dist)
    assert fitness[0] == tr['history'][0][0] and abs(rmse[0] - tr['history'][0][1]) <= 1e-15
    # (P, 3, 4) init and the concatenated layout give the same result
    flat = icp_refine_host((src, np.array([0, len(src)])), (dst, np.array([0, len(dst)])), init=init[None, :3],
                           max_correspondence_distance=max_dist, max_iterations=0)
    assert np.array_equal(flat.transforms, r.transforms) and flat.fitness[0] == r.fitness[0]


def test_correspondences_host_layout_and_sums():
    src, dst, g, max_dist, _, _ = family('noisy')
    dist, idx, inl, sums = icp_correspondences_host([src, src[:7]], [dst, dst[:1]], np.stack([np.eye(4), g]), max_dist)
    assert dist.dtype == np.float32 and idx.dtype == np.int32 and inl.dtype == bool and sums.shape == (2, reg.N_SUMS)
    assert dist.shape == (len(src) + 7,) and (idx[len(src):] == 0).all()
    first, _ = rc.two_nearest(src, dst)
    assert (np.abs(dist[:len(src)] - first) <= 1e-6 * first).all()
    p, q = src[inl[:len(src)]], dst[idx[:len(src)][inl[:len(src)]]]
    want = rc.sums_of(p, q)
    assert sums[0, 0] == want[0] and (np.abs(sums[0, :16] - want[:16]) <= 1e-12 * np.abs(want[:16]).max()).all()
    assert abs(sums[0, 16] - (dist[:len(src)][inl[:len(src)]].astype(np.float64) ** 2).sum()) <= 1e-12 * sums[0, 16]


def test_arguments():
    dst = rc.target(50)
    with pytest.raises(TypeError, match='float64 points'):
        icp_refine_host([dst.astype(np.float64)], [dst])
    with pytest.raises(ValueError):
        icp_refine_host([dst], [dst, dst])
    with pytest.raises(ValueError):
        icp_refine_host([dst], [dst], init=np.eye(4)[None].repeat(2, 0))
    with pytest.raises(ValueError):
        icp_refine_host([dst], [dst], max_iterations=-1)
    with pytest.raises(TypeError):
        kabsch_update_host(np.zeros((1, 16)))


def test_package_exports_the_new_names():
    for name in ('icp_refine', 'icp_refine_host', 'icp_correspondences', 'icp_correspondences_host', 'evaluate_registration',
                 'evaluate_registration_host', 'kabsch_update', 'kabsch_update_host', 'RegistrationResult'):
        assert getattr(hotformerloc_amd, name) is getattr(reg, name)
    assert (reg.RUNNING, reg.CONVERGED, reg.MAX_ITERATIONS, reg.TOO_FEW, reg.DEGENERATE) == (0, 1, 2, 3, 4)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'hotformerloc_hip.h')).read()
    for name, value in (('SUMS', reg.N_SUMS), ('RUNNING', reg.RUNNING), ('CONVERGED', reg.CONVERGED),
                        ('MAX_ITERATIONS', reg.MAX_ITERATIONS), ('TOO_FEW', reg.TOO_FEW), ('DEGENERATE', reg.DEGENERATE)):
        assert '#define HFL_ICP_%s %d\n' % (name, value) in header
    assert ops.ICP_SUMS == reg.N_SUMS
    assert hotformerloc_amd.RegistrationResult._fields == ('transforms', 'fitness', 'inlier_rmse', 'iterations', 'status')
