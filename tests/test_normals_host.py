"""The numpy routes of the normal estimate (`hotformerloc_amd/normals.py`) and of the point-to-plane update
(`hotformerloc_amd/registration.py`), the definitions the device routes are held to, against independent restatements
written here: argsort neighbourhoods, a mean-centred covariance and `numpy.linalg.eigh`; `numpy.linalg.solve` on the
assembled 6 x 6.

Bounds.  Normals: |n . n_ref| >= 1 - 1e-12 wherever (l1 - l0) / l2 > 1e-6 -- an eigenvector moves by about eps x |C| / gap
<= 1e-10 rad there, and 1 - cos of that is 5e-21.  Curvature: 1e-12.  Both bounds are far below an fp32 ulp, so they are
asserted on the float64 values of steps 1 to 6 (`normals._normals_host`), and the public fp32 outputs are asserted to be
exactly those values rounded once (step 7).  The 6 x 6 solve: 1e-12 x cond_2 of the diagonally
scaled A x |x|_inf, the backward-error bound of a stable solve at float64 eps with four decimal digits of slack, on cases
whose cond is asserted <= 1e6."""
import functools
import os
import re

import numpy as np
import pytest

import hotformerloc_amd as hfl
from hotformerloc_amd import normals, ops
from hotformerloc_amd import registration as reg
from tests import normals_cases as nc
from tests import registration_cases as rc


def restated(cloud, nb):
    """-> (counts, unit normals up to sign (n, 3) float64, curvature, eigenvalues ascending) by argsort, a centred
    covariance and eigh"""
    p32 = np.asarray(cloud, np.float32)
    p = p32.astype(np.float64)
    n = p.shape[0]
    k = min(nb, n)
    d = p32[:, None, :] - p32[None, :, :]
    d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
    order = np.argsort(d2, axis=1, kind='stable')
    counts, nrm, curv, lam = np.zeros(n, np.int32), np.zeros((n, 3)), np.zeros(n), np.full((n, 3), np.nan)
    for i in range(n):
        r2 = d2[i, order[i, k - 1]]
        members = order[i, :np.searchsorted(d2[i, order[i]], r2, side='right')]      # ties at the k-th place all included
        counts[i] = members.shape[0]
        if counts[i] < 3:
            continue
        q = p[members]
        c = (q - q.mean(0)).T @ (q - q.mean(0)) / counts[i]
        w, v = np.linalg.eigh(c)
        lam[i] = w
        if w[1] > 1e-12 * w[2]:
            nrm[i], curv[i] = v[:, 0], w[0] / w.sum()
    return counts, nrm, curv, lam


CLOUDS = {
    'noisy_plane': lambda: nc.noisy_plane(700, 1),
    'plane_offset': lambda: nc.noisy_plane(500, 2, offset=(100.0, -80.0, 30.0)),
    'sphere': lambda: nc.sphere_shell(800),
    'forest': lambda: nc.forest(900),
    'tie_lattice': nc.tie_lattice,
    'duplicated': nc.duplicated,
}


@functools.lru_cache(maxsize=None)
def both(name, nb):
    cloud = CLOUDS[name]()
    host = normals.estimate_normals_host([cloud], nb, return_curvature=True, return_counts=True, return_eigenvalues=True)
    return cloud, [h[0] for h in host], restated(cloud, nb)


@pytest.mark.parametrize('name,nb', [('noisy_plane', 30), ('noisy_plane', 3), ('plane_offset', 16), ('sphere', 20),
                                     ('forest', 30), ('tie_lattice', 30), ('duplicated', 30)])
def test_against_the_restatement(name, nb):
    cloud, (nrm, curv, counts, lam), (r_counts, r_nrm, r_curv, r_lam) = both(name, nb)
    assert nrm.dtype == np.float32 and curv.dtype == np.float32 and counts.dtype == np.int32
    assert nrm.shape == cloud.shape and curv.shape == counts.shape == (len(cloud),)
    assert np.array_equal(counts, r_counts)
    assert np.array_equal((nrm != 0).any(1), (r_nrm != 0).any(1))
    # steps 1 to 6 in float64, which the bounds are about; the outputs are those values rounded once (step 7)
    n64, c64, _, l64 = normals._normals_host(cloud, nb, None)
    assert np.array_equal(nrm, n64.astype(np.float32)) and np.array_equal(curv, c64.astype(np.float32))
    assert np.array_equal(lam, l64, equal_nan=True)
    sure = nc.undetermined_share(r_nrm, r_lam)[1]
    assert sure.sum() >= (1.0 - nc.MAX_SHARE) * (r_nrm != 0).any(1).sum() and sure.any()
    assert (np.abs((n64 * r_nrm).sum(1))[sure] >= 1.0 - 1e-12).all()
    assert np.abs(c64 - r_curv)[sure].max() <= 1e-12
    assert np.abs(np.linalg.norm(n64[sure], axis=1) - 1.0).max() <= 1e-14


def test_noise_free_tilted_plane_and_both_sign_rules():
    a, b, c = 0.3, -0.2, 1.5
    cloud = nc.tilted_plane(24, a, b, c)
    want = np.array([a, b, -1.0]) / np.linalg.norm([a, b, -1.0])
    up, curv = normals.estimate_normals_host([cloud], 9, return_curvature=True)
    assert np.abs(up[0] + want).max() <= 1e-6                            # upward: n_z > 0, so -(a, b, -1) / |.|
    assert (up[0][:, 2] > 0).all() and curv[0].max() <= 1e-10
    below = np.array([0.0, 0.0, -50.0])
    down = normals.estimate_normals_host([cloud], 9, viewpoint=below)[0]
    assert np.abs(down - want).max() <= 1e-6
    assert (((below - cloud.astype(np.float64)) * down).sum(1) >= 0).all()
    two = normals.estimate_normals_host([cloud, cloud], 9, viewpoint=np.array([[0.0, 0.0, -50.0], [0.0, 0.0, 50.0]]))
    assert np.array_equal(two[0], down) and np.array_equal(two[1], up[0])


def test_upward_rule_falls_through_the_axes():
    flat_xz = np.array([[x, 2.0, z] for x in range(4) for z in range(4)], np.float32)       # normal (0, +-1, 0)
    flat_yz = np.array([[-1.0, y, z] for y in range(4) for z in range(4)], np.float32)      # normal (+-1, 0, 0)
    n_y, n_x = normals.estimate_normals_host([flat_xz, flat_yz], 9)
    assert np.array_equal(n_y, np.tile(np.float32([0, 1, 0]), (16, 1)))
    assert np.array_equal(n_x, np.tile(np.float32([1, 0, 0]), (16, 1)))


def test_ties_at_the_kth_place_are_all_included():
    _, (nrm, curv, counts, lam), (r_counts, _, _, _) = both('tie_lattice', 30)
    assert np.array_equal(counts, r_counts)
    assert (counts[:-1] > 30).any() and counts[:-1].max() == 33 and counts.min() >= 30


@pytest.mark.parametrize('cloud', [np.zeros((1, 3), np.float32), np.float32([[0, 0, 0], [1, 2, 3]]), nc.collinear(),
                                   np.tile(np.float32([[4.0, -2.0, 7.0]]), (35, 1))],
                         ids=['one', 'two', 'collinear', 'coincident'])
def test_degenerate_points_have_a_zero_normal(cloud):
    nrm, curv, counts = normals.estimate_normals_host([cloud], 30, return_curvature=True, return_counts=True)
    assert not nrm[0].any() and not curv[0].any()
    assert (counts[0] == min(30, len(cloud))).all() or len(cloud) > 30


def test_argument_refusals():
    cloud = nc.noisy_plane(50)
    for nb in (2, 33, 0, -1, 3.0, True, None):
        with pytest.raises(ValueError, match='nb_neighbors'):
            normals.estimate_normals_host([cloud], nb)
        with pytest.raises(ValueError, match='nb_neighbors'):
            normals.estimate_normals([cloud], nb)                        # before the device is touched
    with pytest.raises(ValueError, match='cloud 1 is empty'):
        normals.estimate_normals_host([cloud, np.zeros((0, 3), np.float32)])
    with pytest.raises(ValueError, match='cloud 1 is empty'):
        normals.estimate_normals([cloud, np.zeros((0, 3), np.float32)])
    bad = cloud.copy()
    bad[7, 1] = np.nan
    with pytest.raises(ValueError, match='cloud 1 holds a coordinate that is not finite'):
        normals.estimate_normals_host([cloud, bad])
    for view in (np.zeros(2), np.zeros((2, 3)), np.zeros((1, 4)), [np.inf, 0.0, 0.0]):
        with pytest.raises(ValueError, match='viewpoint'):
            normals.estimate_normals_host([cloud], viewpoint=view)
        with pytest.raises(ValueError, match='viewpoint'):
            normals.estimate_normals([cloud], viewpoint=view)
    with pytest.raises(ValueError, match='cell_size'):
        normals.estimate_normals([cloud], cell_size=0.0)


def test_package_exports_and_header_constants():
    for name in ('estimate_normals', 'estimate_normals_host', 'plane_update', 'plane_update_host'):
        assert callable(getattr(hfl, name))
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'hotformerloc_hip.h')).read()
    assert re.search(r'#define HFL_ICP_PLANE_SUMS 29\b', header)
    assert ops.ICP_PLANE_SUMS == reg.N_SUMS_PLANE == 29
    assert 'hfl_knn_normals' in header and 'hfl_icp_correspond_plane' in header and 'hfl_icp_solve_plane' in header


# --------------------------------------------------------------------------------------------- the point-to-plane update
def test_plane_update_against_numpy_solve():
    sums, kinds = nc.plane_cases()
    r, t, status = reg.plane_update_host(sums)
    assert r.shape == (len(sums), 3, 3) and t.shape == (len(sums), 3) and status.dtype == np.int32
    for i, kind in enumerate(kinds):
        if kind == 'parallel':
            assert status[i] == reg.DEGENERATE and np.array_equal(r[i], np.eye(3)) and not t[i].any()
            continue
        if kind == 'few':
            assert status[i] == reg.TOO_FEW and np.array_equal(r[i], np.eye(3)) and not t[i].any()
            continue
        assert status[i] == reg.RUNNING
        a, g = nc.system_of(sums[i])
        cond = nc.scaled_cond(a)
        assert cond <= 1e6
        x = np.linalg.solve(a, -g)
        bound = 1e-12 * cond * np.abs(x).max()
        assert np.abs(t[i] - x[3:]).max() <= bound
        assert np.abs(r[i] - nc.rotation_of(x)).max() <= bound + 1e-15
        assert np.abs(r[i] @ r[i].T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(r[i]) - 1.0) <= 1e-12
    assert reg.plane_update_host(sums[:1], min_correspondences=10 ** 6)[2][0] == reg.TOO_FEW
    with pytest.raises(TypeError):
        reg.plane_update_host(np.zeros((2, 17)))


def test_plane_sums_of_the_host_route_match_matrix_products():
    src, dst, g = nc.corner_pair(300, 600)
    nrm = normals.estimate_normals_host([dst], 12)[0]
    nrm[::7] = 0                                                         # "no normal" rows add nothing
    dist, idx, inl, sums = reg.icp_correspondences_host([src], [dst], np.eye(4)[None], 0.6, target_normals=[nrm])
    plain = reg.icp_correspondences_host([src], [dst], np.eye(4)[None], 0.6)
    assert all(np.array_equal(x, y) for x, y in zip((dist, idx, inl), plain[:3]))
    assert sums.shape == (1, 29) and 0 < inl.sum() < len(src)
    moved = reg._host_move(src, np.eye(4)[:3])
    want = nc.plane_sums_of(moved[inl], dst[idx[inl]], nrm[idx[inl]])
    want[1] = (dist[inl].astype(np.float64) ** 2).sum()
    assert np.abs(sums[0] - want).max() <= 1e-12 * np.abs(want).max()


@functools.lru_cache(maxsize=None)
def corner_runs():
    src, dst, g = nc.corner_pair()
    nrm = normals.estimate_normals_host([dst], 20)[0]
    point = reg.icp_refine_host([src], [dst], max_correspondence_distance=1.0)
    plane = reg.icp_refine_host([src], [dst], max_correspondence_distance=1.0, estimation='point_to_plane',
                                target_normals=[nrm])
    return g, point, plane


def test_point_to_plane_beats_point_to_point_on_a_corner():
    g, point, plane = corner_runs()
    assert plane.status[0] == reg.CONVERGED and plane.iterations[0] >= 2
    e_point, e_plane = nc.pose_errors(point.transforms[0], g), nc.pose_errors(plane.transforms[0], g)
    print('corner: point-to-point %.4f deg %.4f m, point-to-plane %.4f deg %.4f m' % (e_point + e_plane))
    assert e_plane[0] < e_point[0] and e_plane[1] < e_point[1]
    r = plane.transforms[0, :3, :3]
    assert np.abs(r @ r.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(r) - 1.0) <= 1e-12


def test_estimation_argument_refusals():
    src, dst, _, _ = rc.pair(rc.EXACT, 50, 100)
    nrm = np.zeros_like(dst)
    for kw in (dict(estimation='point_to_line'), dict(estimation='point_to_plane'), dict(target_normals=[nrm]),
               dict(estimation='point_to_plane', target_normals=[nrm[:-1]]),
               dict(estimation='point_to_plane', target_normals=nrm),
               dict(estimation='point_to_plane', target_normals=[nrm, nrm])):
        with pytest.raises(ValueError):
            reg.icp_refine_host([src], [dst], **kw)
    packed = reg.icp_refine_host((src, np.array([0, len(src)])), (dst, np.array([0, len(dst)])), max_iterations=1,
                                 estimation='point_to_plane', target_normals=nrm)
    assert packed.status[0] == reg.DEGENERATE                            # zero normals determine nothing


def test_the_default_mode_is_unchanged():
    src, dst, g, max_dist = rc.pair(rc.NOISY, 300, 700)
    want = rc.trace(src, dst, max_dist)
    for kw in ({}, dict(estimation='point_to_point')):
        got = reg.icp_refine_host([src], [dst], max_correspondence_distance=max_dist, **kw)
        assert np.array_equal(got.transforms[0], want['transform']) and got.iterations[0] == want['iterations']
        assert got.status[0] == want['status'] and got.fitness[0] == want['fitness'] and got.inlier_rmse[0] == want['rmse']
