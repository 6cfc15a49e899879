"""The generalized (plane-to-plane) estimator on the host route: the definition in `hotformerloc_amd/registration.py`.

Rows.  The fixed-order row of the host route against `numpy.linalg.inv(C)` and explicit J^T M J, J^T M r in float64, each
block (M, g, A) to 1e-12 / eps of its largest entry: cond(C) <= 1 / eps (the eigenvalues of C lie in [2 eps, 2]) times
float64 eps with four digits of slack, the slack tests/test_gpu_registration_plane.py takes.  Closed forms: a = b = n gives
M = (I + ((1 - eps) / (1 - (1 - eps) |n|^2)) n n^T) / 2, which for |n| = 1 exactly (the axis normals here) is (I + ((1 - eps)
/ eps) n n^T) / 2; both normals zero gives I / 2.

Purpose, measured with this route (normals from `estimate_normals_host(., 20)`, max_correspondence_distance 1.0, from the
identity; rotation error, translation error, updates):

    case                                       point-to-plane            generalized
    corner_pair()                              0.0947 deg 0.0170 m  7    0.0412 deg 0.0042 m  4
    corner_pair(n_source=1500, n_target=600)   0.1648 deg 0.0234 m  5    0.0768 deg 0.0120 m  4
    corner_pair(seed=3)                        0.0511 deg 0.0056 m  4    0.0238 deg 0.0027 m  5

All three hold under the fp32 definition; none was dropped.  `global_registration_host(estimation='generalized')` on the raw
plane clouds ends 9.57e-07 degrees and 1.22e-07 m from the truth, inside the point-to-plane entry of `GLOBAL_BOUNDS`
(1.91e-06, 2.42e-07)."""
import inspect
import os
import re

import numpy as np
import pytest

import hotformerloc_amd as hfl
from hotformerloc_amd import _native
from hotformerloc_amd import registration as reg
from tests import generalized_cases as gcs
from tests import global_registration_cases as gc
from tests import normals_cases as nc
from tests import registration_cases as rc
from tests.test_gpu_global_registration import GLOBAL_BOUNDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_names_and_the_header():
    assert reg.ESTIMATIONS == ('point_to_point', 'point_to_plane', 'generalized')
    header = open(os.path.join(ROOT, 'include', 'hotformerloc_hip.h')).read()
    assert re.search(r'\bint hfl_icp_correspond_generalized\(', header)
    sig = _native.SIGNATURES
    assert len(sig['hfl_icp_correspond_generalized'][1]) == len(sig['hfl_icp_correspond_plane'][1]) + 2
    for call in (hfl.icp_refine, hfl.icp_refine_host, hfl.icp_correspondences, hfl.icp_correspondences_host,
                 hfl.global_registration, hfl.global_registration_host, hfl.rerank_candidates, hfl.rerank_candidates_host):
        assert inspect.signature(call).parameters['covariance_epsilon'].default == 1e-3


def row_inputs(kind, rows=40, seed=5):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-8.0, 8.0, (rows, 3)).astype(np.float32)
    q = (p + rng.normal(0.0, 0.2, (rows, 3))).astype(np.float32)
    a, b = gcs.unit_normals(rows, seed + 1), gcs.unit_normals(rows, seed + 2)
    if kind == 'parallel':
        b = a.copy()
    elif kind == 'axes':
        a = np.eye(3, dtype=np.float32)[np.arange(rows) % 3] * np.float32([1.0, -1.0, 1.0])
        b = a.copy()
    elif kind == 'zero_source':
        a[:] = 0.0
    elif kind == 'zero_target':
        b[:] = 0.0
    elif kind == 'zero_both':
        a[:], b[:] = 0.0, 0.0
    d = np.sqrt(((p - q).astype(np.float64) ** 2).sum(1)).astype(np.float32)
    return p, q, a, b, d


@pytest.mark.parametrize('eps', [1e-3, 1e-2, 1.0])
@pytest.mark.parametrize('kind', ['general', 'parallel', 'axes', 'zero_source', 'zero_target', 'zero_both'])
def test_rows_against_linear_algebra(kind, eps):
    p, q, a, b, d = row_inputs(kind)
    got = reg._host_generalized_rows(p, q, a, b, d, eps)
    assert got.shape == (len(p), reg.N_SUMS_PLANE) and got.dtype == np.float64
    assert (got[:, 0] == 1.0).all() and np.array_equal(got[:, 1], d.astype(np.float64) ** 2)
    tol = 1e-12 / eps
    worst = 0.0
    for row, (m, g, big_a), aa in zip(got, gcs.rows_by_linear_algebra(p, q, a, b, eps), a.astype(np.float64)):
        got_g, got_a, got_m = gcs.blocks_of(row)
        for have, want in ((got_m, m), (got_g, g), (got_a, big_a)):
            err = np.abs(have - want).max() / np.abs(want).max()
            worst = max(worst, err)
            assert err <= tol, (kind, eps, err)
        if kind in ('parallel', 'axes'):
            k = 1.0 - eps
            closed = 0.5 * (np.eye(3) + (k / (1.0 - k * (aa @ aa))) * np.outer(aa, aa))
            assert np.abs(got_m - closed).max() <= tol * np.abs(closed).max()
        if kind == 'axes':                                               # |n| = 1 exactly: the form of the definition
            closed = 0.5 * (np.eye(3) + ((1.0 - eps) / eps) * np.outer(aa, aa))
            assert np.abs(got_m - closed).max() <= tol * np.abs(closed).max()
        if kind == 'zero_both':
            assert np.array_equal(got_m, np.eye(3) / 2.0)
    print('%s eps %g: worst relative error %.3g (bound %.3g)' % (kind, eps, worst, tol))


def test_covariance_eigenvalues_lie_in_the_stated_range():
    p, q, a, b, d = row_inputs('general', rows=200)
    a[::5], b[2::5] = 0.0, 0.0
    b[1::7] = a[1::7]
    for aa, bb in zip(a, b):
        w = np.linalg.eigvalsh(gcs.covariance(aa, bb))
        assert w.min() >= 2.0 * gcs.EPS * (1.0 - 1e-3) and w.max() <= 2.0 + 1e-12      # fp32 normals: |n|^2 = 1 +- 2^-23


def test_generalized_sums_of_the_host_route_match_matrix_products():
    src, dst, g = nc.corner_pair(300, 600)
    ns, nt = (n.copy() for n in hfl.estimate_normals_host([src, dst], 12))
    ns[::5], nt[2::7] = 0.0, 0.0                                         # "no normal" rows on either side
    pose = rc.rigid(1.0, 0.05)
    dist, idx, inl, sums = reg.icp_correspondences_host([src], [dst], pose[None], 0.6, target_normals=[nt],
                                                        source_normals=[ns])
    plain = reg.icp_correspondences_host([src], [dst], pose[None], 0.6)
    assert all(np.array_equal(x, y) for x, y in zip((dist, idx, inl), plain[:3]))
    assert sums.shape == (1, 29) and 0 < inl.sum() < len(src) and sums[0, 0] == inl.sum()
    moved = reg._host_move(src, pose[:3])
    turned = (ns.astype(np.float64) @ pose[:3, :3].astype(np.float32).astype(np.float64).T)
    assert np.abs(reg._host_turn(ns, pose[:3]) - turned).max() <= 2e-7   # the fp32 chain against the float64 product
    a, b = reg._host_turn(ns, pose[:3])[inl], nt[idx[inl]]
    zero_a, zero_b = ~a.any(1), ~b.any(1)
    assert all((x & y).any() for x in (zero_a, ~zero_a) for y in (zero_b, ~zero_b))
    parts = gcs.rows_by_linear_algebra(moved[inl], dst[idx[inl]], a, b)
    want_g, want_a = sum(x[1] for x in parts), sum(x[2] for x in parts)
    got_g, got_a, _ = gcs.blocks_of(sums[0])
    tol = 1e-12 / gcs.EPS
    assert np.abs(got_g - want_g).max() <= tol * np.abs(want_g).max()
    assert np.abs(got_a - want_a).max() <= tol * np.abs(want_a).max()
    assert sums[0, 1] == (dist[inl].astype(np.float64) ** 2).sum()
    # and the sums are the sum of the route's own rows, in numpy's order
    rows = reg._host_generalized_rows(moved[inl], dst[idx[inl]], a, b, dist[inl], gcs.EPS)
    assert np.array_equal(np.delete(sums[0], 1), np.delete(rows.sum(0), 1))
    assert sums[0, 1] == plain[3][0, 16]                                 # sum d^2: the bits of the point-to-point sums
    # the solve that point-to-plane uses takes them
    r, t, status = reg.plane_update_host(sums)
    assert status.tolist() == [reg.RUNNING] and gcs.orthonormal(r[0])


@pytest.mark.parametrize('case', range(len(gcs.CORNERS)))
def test_purpose_nearer_the_truth_than_point_to_plane(case):
    g, plane, gen = gcs.corner_runs(**gcs.CORNERS[case])
    e_plane, e_gen = nc.pose_errors(plane.transforms[0], g), nc.pose_errors(gen.transforms[0], g)
    print('%s: point-to-plane %.4f deg %.4f m %d updates, generalized %.4f deg %.4f m %d updates'
          % (gcs.CORNERS[case], e_plane[0], e_plane[1], plane.iterations[0], e_gen[0], e_gen[1], gen.iterations[0]))
    assert gen.status.tolist() == [reg.CONVERGED] and plane.status.tolist() == [reg.CONVERGED]
    assert e_gen[0] < e_plane[0] and e_gen[1] < e_plane[1]
    assert gcs.orthonormal(gen.transforms[0, :3, :3])
    assert np.array_equal(gen.transforms[0, 3], [0.0, 0.0, 0.0, 1.0])


def test_flat_target_far_points_and_empty_clouds():
    c = gcs.loop_batch()
    assert c['plane'].status.tolist() == [reg.CONVERGED, reg.CONVERGED, reg.TOO_FEW, reg.DEGENERATE]
    host = c['host']
    assert host.status.tolist()[:3] == [reg.CONVERGED, reg.CONVERGED, reg.TOO_FEW] and host.status[3] != reg.DEGENERATE
    assert host.status[3] == reg.CONVERGED and host.iterations[3] >= 1 and host.fitness[3] == 1.0
    assert np.array_equal(host.transforms[2], np.eye(4)) and host.iterations[2] == 0 and np.isnan(host.inlier_rmse[2])
    assert np.abs(host.transforms[3] - np.eye(4)).max() <= 1e-12         # the source is a subset of the target: nothing to move
    empty = np.zeros((0, 3), np.float32)
    dst, nrm = rc.target(64), gcs.unit_normals(64, 2)
    kw = dict(max_correspondence_distance=1.0)
    for est, more in (('generalized', dict(source_normals=[empty, nrm])), ('point_to_plane', dict())):
        res = hfl.icp_refine_host([empty, dst], [dst, empty], estimation=est, target_normals=[nrm, empty], **more, **kw)
        assert res.status.tolist() == [reg.TOO_FEW, reg.TOO_FEW] and res.iterations.tolist() == [0, 0]
        assert np.isnan(res.fitness[0]) and res.fitness[1] == 0.0 and np.isnan(res.inlier_rmse).all()
        assert np.array_equal(res.transforms, np.tile(np.eye(4), (2, 1, 1)))
    point = hfl.icp_refine_host([empty, dst], [dst, empty], **kw)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(point, res))


def test_arguments_are_refused():
    dst = rc.target(50)
    nrm = gcs.unit_normals(50, 1)
    good = dict(estimation='generalized', target_normals=[nrm], source_normals=[nrm])
    hfl.icp_refine_host([dst], [dst], max_iterations=0, **good)
    bad = [dict(estimation='generalized'), dict(estimation='generalized', target_normals=[nrm]),
           dict(estimation='generalized', source_normals=[nrm]), dict(source_normals=[nrm]),
           dict(estimation='point_to_plane', target_normals=[nrm], source_normals=[nrm]),
           dict(good, source_normals=[nrm[:-1]]), dict(good, source_normals=nrm), dict(good, target_normals=nrm),
           dict(good, source_normals=[nrm, nrm]), dict(estimation='plane_to_plane')]
    bad += [dict(good, covariance_epsilon=e) for e in (0.0, -1e-3, 1.0 + 1e-9, float('nan'))]
    for kw in bad:
        with pytest.raises(ValueError):
            hfl.icp_refine_host([dst], [dst], **kw)
    with pytest.raises(ValueError):
        hfl.icp_correspondences_host([dst], [dst], np.eye(4)[None], 1.0, source_normals=[nrm])
    with pytest.raises(ValueError):
        hfl.icp_correspondences_host([dst], [dst], np.eye(4)[None], 1.0, target_normals=[nrm], source_normals=[nrm],
                                     covariance_epsilon=2.0)
    src, dst2 = gc.clouds()
    for call, args in ((hfl.global_registration_host, ([src[:50]], [dst2[:50]])),
                       (hfl.rerank_candidates_host, ([src[:50]], [dst2[:50]], np.zeros((1, 1), np.int64)))):
        with pytest.raises(ValueError):
            call(*args, estimation='generalized', covariance_epsilon=0.0)
        with pytest.raises(ValueError):
            call(*args, estimation='plane_to_plane')
    # the packed layout takes packed normals on both sides
    packed = hfl.icp_refine_host((dst, np.array([0, 50])), (dst, np.array([0, 50])), estimation='generalized',
                                 target_normals=nrm, source_normals=nrm, max_iterations=2)
    listed = hfl.icp_refine_host([dst], [dst], max_iterations=2, **good)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(packed, listed))


def test_the_defaults_and_point_to_plane_keep_their_bits():
    src, dst, g, ns, nt = gcs.corner()
    default = hfl.icp_refine_host([src], [dst], max_correspondence_distance=gcs.MAX_DIST)
    named = hfl.icp_refine_host([src], [dst], max_correspondence_distance=gcs.MAX_DIST, estimation='point_to_point',
                                covariance_epsilon=0.5)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(default, named))
    # point-to-plane: the arrays this route gave before the generalized estimator existed
    golden = np.load(gcs.GOLDEN)
    plane = gcs.corner_runs()[1]
    for name in ('transforms', 'fitness', 'inlier_rmse', 'iterations', 'status'):
        assert getattr(plane, name).tobytes() == golden[name].tobytes(), name
    dist, idx, inl, sums = hfl.icp_correspondences_host([src], [dst], np.eye(4)[None], gcs.MAX_DIST, target_normals=[nt])
    assert sums.tobytes() == golden['sums'].tobytes() and dist.tobytes() == golden['dist'].tobytes()
    assert idx.tobytes() == golden['idx'].tobytes()
    # and epsilon = 1 (both covariances the identity, M = I / 2) is point-to-point's normal equations, not its bits
    gen = hfl.icp_correspondences_host([src], [dst], np.eye(4)[None], gcs.MAX_DIST, target_normals=[nt], source_normals=[ns],
                                       covariance_epsilon=1.0)
    assert all(np.array_equal(x, y) for x, y in zip(gen[:3], (dist, idx, inl)))
    assert np.array_equal(gen[3][0, 23:], 0.5 * inl.sum() * np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0]))


def test_global_registration_in_one_call():
    src, dst = gc.clouds()
    coarse, fine = hfl.global_registration_host([src], [dst], estimation='generalized')
    angle, shift = gc.pose_error(fine.transforms[0])
    print('coarse %.3g degrees %.3g m, fine %.3g degrees %.3g m, %d updates'
          % (gc.pose_error(coarse.transforms[0]) + (angle, shift, fine.iterations[0])))
    assert coarse.status.tolist() == [reg.MAX_ITERATIONS] and fine.status.tolist() == [reg.CONVERGED]
    assert angle <= GLOBAL_BOUNDS['point_to_plane'][0] and shift <= GLOBAL_BOUNDS['point_to_plane'][1]
    assert angle <= GLOBAL_BOUNDS['point_to_point'][0] and shift <= GLOBAL_BOUNDS['point_to_point'][1]
