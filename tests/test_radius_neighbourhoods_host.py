"""Radius and hybrid neighbourhoods on the CPU: the numpy routes of `normals.py`, `fpfh.py` and `outliers.py` with `radius=`
against an independent transcription, one point at a time (`tests/radius_cases.py`), their limits, their refusals, and the
case they exist for: two samplings of one surface at a density of 1 : 4."""
import os

import numpy as np
import pytest

import hotformerloc_amd as hfl
from hotformerloc_amd import build, fpfh, normals, outliers
from hotformerloc_amd import registration as reg
from hotformerloc_amd.global_registration import inlier_d2
from tests import fpfh_cases as fc
from tests import radius_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ brute-force parity
@pytest.mark.parametrize('mode', rc.MODES)
@pytest.mark.parametrize('key', rc.KEYS)
def test_against_the_transcription_point_by_point(key, mode):
    cloud, radius, nb = rc.cloud_of(key), rc.radius_of(key), rc.nb_of(mode)
    members = rc.members_scalar(cloud, nb, radius)
    sizes = np.array([m.shape[0] for m in members], np.int32)
    nrm, _, counts, _ = rc.host_normals(key, mode)
    assert counts.dtype == np.int32 and np.array_equal(counts, sizes)
    zero, margin = rc.zero_normal_scalar(cloud, members)
    assert margin > 2.0, 'a rank ratio within a factor of 100 of the threshold: the transcription cannot judge it'
    assert np.array_equal(~(nrm != 0).any(1), zero)
    _, hist, pairs = rc.host_fpfh(key, mode)
    t_hist, t_pairs = rc.spfh_scalar(cloud, nrm, members)
    assert np.array_equal(hist, t_hist) and np.array_equal(pairs, t_pairs)
    if mode == 'radius_only':
        ball = np.array([m.shape[0] for m in rc.members_scalar(cloud, None, radius)], np.int32)
        assert np.array_equal(outliers.radius_neighbour_counts_host([cloud], radius)[0], ball)
        kept, mask = outliers.remove_radius_outliers_host([cloud], 4, radius, return_mask=True)
        assert np.array_equal(mask[0], ball > 4) and np.array_equal(kept[0], cloud[ball > 4])
    else:                                                             # both kinds of point occur: capped by k, capped by R
        ball = outliers.radius_neighbour_counts_host([cloud], radius)[0]
        assert (ball > 30).any() and (ball < 30).any() and (counts <= np.maximum(ball, 1)).all()


def test_far_points_stand_alone():
    """the 20 far points of 'planes700': one neighbour (themselves), no normal, no pairs, removed by the radius filter"""
    cloud, radius = rc.cloud_of('planes700'), rc.radius_of('planes700')
    for mode in rc.MODES:
        nrm, curv, counts, _ = rc.host_normals('planes700', mode)
        assert (counts[-20:] == 1).all() and not nrm[-20:].any() and not curv[-20:].any()
        feat, hist, pairs = rc.host_fpfh('planes700', mode)
        assert not pairs[-20:].any() and not hist[-20:].any() and not feat[-20:].any()
    kept, mask = outliers.remove_radius_outliers_host([cloud], 1, radius, return_mask=True)
    assert not mask[0][-20:].any() and mask[0][:-20].sum() > 600 and kept[0].shape[0] == mask[0].sum()
    assert outliers.remove_radius_outliers_host([cloud], 0, radius)[0].shape[0] == 700      # counts >= 1 everywhere


# ------------------------------------------------------------------------------------------------ the boundary is inclusive
@pytest.mark.parametrize('radius, interior', zip(rc.LATTICE_RADII, rc.LATTICE_INTERIOR))
def test_lattice_counts_are_the_exact_ones(radius, interior):
    cloud, nrm = fc.lattice()
    want = rc.lattice_counts(radius)
    assert want[62] == interior and want[0] < interior               # the centre (2, 2, 2) and a corner
    assert np.array_equal(outliers.radius_neighbour_counts_host([cloud], radius)[0], want)
    assert np.array_equal(normals.estimate_normals_host([cloud], None, radius=radius, return_counts=True)[1][0], want)
    hybrid = normals.estimate_normals_host([cloud], 9, radius=radius, return_counts=True)[1][0]
    knn = normals.estimate_normals_host([cloud], 9, return_counts=True)[1][0]
    assert np.array_equal(hybrid, np.minimum(want, knn))              # nested sets: the smaller of the two balls
    _, hist, pairs = fpfh.compute_fpfh_host([cloud], [nrm], None, radius=radius, return_histograms=True)
    t_hist, t_pairs = rc.spfh_scalar(cloud, nrm, rc.members_scalar(cloud, None, radius))
    assert np.array_equal(hist[0], t_hist) and np.array_equal(pairs[0], t_pairs)


def test_threshold_is_the_one_of_icp_and_ransac():
    for radius in (0.8, 1.0, 1.7, 1e-3, 1e30):
        r2 = outliers.radius2(outliers.check_radius(radius))
        assert r2.dtype == np.float32 and r2 == inlier_d2(radius)
        above = np.nextafter(r2, np.float32(np.inf))
        assert np.sqrt(r2) <= np.float32(radius) and (radius > 1e19 or np.sqrt(above) > np.float32(radius))


# ------------------------------------------------------------------------------------------------ limits of the radius
@pytest.mark.parametrize('key', ('plane37', 'duplicated'))
def test_hybrid_with_a_huge_radius_is_the_k_nearest_result_bit_for_bit(key):
    cloud = rc.cloud_of(key)
    kw = dict(viewpoint=np.array(fc.VIEW), return_curvature=True, return_counts=True, return_eigenvalues=True)
    plain = normals.estimate_normals_host([cloud], 30, **kw)
    capped = normals.estimate_normals_host([cloud], 30, radius=1e30, **kw)
    for a, b in zip(plain, capped):
        assert np.array_equal(a[0], b[0], equal_nan=True)
    for a, b in zip(fpfh.compute_fpfh_host([cloud], [plain[0][0]], 30, return_histograms=True),
                    fpfh.compute_fpfh_host([cloud], [plain[0][0]], 30, radius=1e30, return_histograms=True)):
        assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32))


def test_a_radius_below_the_spacing_leaves_every_point_alone():
    cloud = rc.cloud_of('plane37')
    nrm, curv, counts = normals.estimate_normals_host([cloud], None, radius=1e-3, return_curvature=True, return_counts=True)
    assert (counts[0] == 1).all() and not nrm[0].any() and not curv[0].any()
    feat, hist, pairs = fpfh.compute_fpfh_host([cloud], [fc.host_normals('plane37')], None, radius=1e-3, return_histograms=True)
    assert not pairs[0].any() and not hist[0].any() and not feat[0].any()
    assert (outliers.radius_neighbour_counts_host([cloud], 1e-3)[0] == 1).all()
    assert outliers.remove_radius_outliers_host([cloud], 1, 1e-3)[0].shape == (0, 3)


def test_a_radius_above_the_diameter_is_hybrid_with_k_equal_n():
    cloud = rc.cloud_of('plane37')[:32]
    kw = dict(viewpoint=np.array(fc.VIEW), return_curvature=True, return_counts=True)
    alone = normals.estimate_normals_host([cloud], None, radius=100.0, **kw)
    hybrid = normals.estimate_normals_host([cloud], 32, radius=100.0, **kw)
    assert (alone[2][0] == 32).all()
    for a, b in zip(alone, hybrid):
        assert np.array_equal(a[0], b[0])
    for a, b in zip(fpfh.compute_fpfh_host([cloud], [alone[0][0]], None, radius=100.0, return_histograms=True),
                    fpfh.compute_fpfh_host([cloud], [alone[0][0]], 32, radius=100.0, return_histograms=True)):
        assert np.array_equal(a[0], b[0])


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize('radius', (0.0, -1.0, float('nan'), float('inf'), 1e-60, True, '1.0'))
def test_bad_radii_are_refused(radius):
    cloud, nrm = rc.cloud_of('plane37'), fc.host_normals('plane37')
    for call in (lambda: normals.estimate_normals_host([cloud], 30, radius=radius),
                 lambda: normals.estimate_normals([cloud], 30, radius=radius),
                 lambda: fpfh.compute_fpfh_host([cloud], [nrm], None, radius=radius),
                 lambda: fpfh.compute_fpfh([cloud], [nrm], None, radius=radius),
                 lambda: outliers.radius_neighbour_counts_host([cloud], radius),
                 lambda: outliers.radius_neighbour_counts([cloud], radius),
                 lambda: outliers.remove_radius_outliers_host([cloud], 2, radius),
                 lambda: outliers.remove_radius_outliers([cloud], 2, radius)):
        with pytest.raises(ValueError):
            call()


def test_no_neighbour_count_needs_a_radius_and_hybrid_keeps_its_range():
    cloud, nrm = rc.cloud_of('plane37'), fc.host_normals('plane37')
    for call in (lambda **kw: normals.estimate_normals_host([cloud], **kw), lambda **kw: normals.estimate_normals([cloud], **kw),
                 lambda **kw: fpfh.compute_fpfh_host([cloud], [nrm], **kw), lambda **kw: fpfh.compute_fpfh([cloud], [nrm], **kw)):
        with pytest.raises(ValueError):
            call(nb_neighbors=None)
        for nb in (2, 33, 100):                                       # open3d's max_nn = 100 is not reachable
            with pytest.raises(ValueError):
                call(nb_neighbors=nb, radius=1.0)
    for bad in (-1, 1.5, None, True):
        with pytest.raises(ValueError):
            outliers.remove_radius_outliers_host([cloud], bad, 1.0)
    src, dst, _ = rc.density_pair(rc.DENSITY_SEEDS[0])
    for kw in (dict(), dict(normal_radius=1.0), dict(feature_radius=1.0)):
        with pytest.raises(ValueError):
            hfl.global_registration_host([src], [dst], nb_neighbors=None, **kw)
        with pytest.raises(ValueError):
            hfl.rerank_candidates_host([src], [dst], np.zeros((1, 1), np.int64), nb_neighbors=None, **kw)


def test_pass_through_reaches_both_steps():
    """`global_registration_host` and `rerank_candidates_host` with the two radii compute what the steps compute"""
    src, dst = rc.cloud_of('planes'), fc.cloud_of('planes_moved')
    coarse, fine = hfl.global_registration_host([src], [dst], nb_neighbors=None, normal_radius=1.2, feature_radius=1.5)
    nrm = hfl.estimate_normals_host([src, dst], None, radius=1.2)
    feat = hfl.compute_fpfh_host([src, dst], nrm, None, radius=1.5)
    idx, _, mask = hfl.feature_correspondences_host([feat[0]], [feat[1]], mutual=True)
    want = hfl.ransac_registration_host([src], [dst], hfl.correspondence_pairs_host(idx, mask))
    assert np.array_equal(coarse.transforms, want.transforms) and np.array_equal(coarse.inliers, want.inliers)
    assert fine.status.tolist() == [reg.CONVERGED]
    ranked = hfl.rerank_candidates_host([src], [dst], np.zeros((1, 1), np.int64), nb_neighbors=None, normal_radius=1.2,
                                        feature_radius=1.5)
    idx, _ = hfl.feature_correspondences_host([feat[0]], [feat[1]])
    score = hfl.spectral_consistency_host([src], [dst], hfl.correspondence_pairs_host(idx)).score
    assert np.array_equal(ranked.scores[0], score)


# ------------------------------------------------------------------------------------------------ the grid rule
def test_radius_cell_covers_the_ball_and_only_grows():
    """`outliers.radius_cell` against a float64 transcription of `knn_block_bound`'s worst case: a point on the low edge of
    its cell, the face one cell below, the margin and the shrink taken off -- at the radius cell and at its doublings"""
    for extent, radius in (((8.0, 8.0, 8.0), 1.7), ((500.0, 3.0, 0.0), 0.05), ((1e6, 1e6, 10.0), 1e-3), ((7.0, 0.0, 0.0), 7.0)):
        extent = np.array(extent)
        cell = outliers.radius_cell(extent, radius)
        assert np.float32(cell) == cell and cell >= radius
        for grown in (cell, 2 * cell, 64 * cell):
            nmax = float(np.floor(extent / grown).max() + 1)
            gap = grown * (1.0 - nmax * 2.0 ** -23) * (1.0 - 2.0 ** -24) - outliers.FACE_MARGIN * nmax * grown * (1 + 2.0 ** -24)
            root = gap * (1.0 - 2.0 ** -24) * (1.0 - 2.0 ** -20) * (1.0 - 2.0 ** -24) ** 1.5
            assert root * root > float(inlier_d2(radius)) * (1.0 + 2.0 ** -23)
    lo_hi = np.array([[0, 0, 0, 8, 8, 8]], np.float32)
    only = outliers.grid_layout(lo_hi, [700], None, radius=1.7)
    hybrid = outliers.grid_layout(lo_hi, [700], 30, radius=1.7)
    plain = outliers.grid_layout(lo_hi, [700], 30)
    assert only['cell'][0] == np.float32(outliers.radius_cell(np.array([8.0, 8.0, 8.0]), 1.7))
    assert hybrid['cell'][0] == min(only['cell'][0], plain['cell'][0]) and plain['cell'][0] < only['cell'][0]
    fine = outliers.grid_layout(lo_hi, [700], None, radius=0.1)
    assert outliers.grid_layout(lo_hi, [700], 30, radius=0.1)['cell'][0] == fine['cell'][0]
    assert outliers.grid_layout(lo_hi, [700], None, cell_size=0.5, radius=1.7)['cell'][0] == np.float32(0.5)
    tight = outliers.grid_layout(lo_hi, [700], None, budget_bytes=4 * 9, radius=0.01)      # eight cells at the most
    assert tight['cell'][0] > 1.7 and int(tight['nx'][0]) * int(tight['ny'][0]) * int(tight['nz'][0]) <= 8


def test_abi_and_build_flags():
    header = open(os.path.join(ROOT, 'include', 'hotformerloc_hip.h')).read()
    for name in ('hfl_knn_normals_radius', 'hfl_fpfh_radius_capped', 'hfl_knn_radius_count', 'hfl_count_mask'):
        assert 'int %s(' % name in header
    for src in ('outliers.hip', 'normals.hip', 'fpfh.hip'):          # everything that includes knn_common.h
        assert '-ffp-contract=off' in build.EXTRA_FLAGS[src]


# ------------------------------------------------------------------------------------------------ the density case
def coarse_pose(src, dst, nb, radius):
    nrm = hfl.estimate_normals_host([src, dst], nb, radius=radius)
    feat = hfl.compute_fpfh_host([src, dst], nrm, nb, radius=radius)
    idx, _, mask = hfl.feature_correspondences_host([feat[0]], [feat[1]], mutual=True)
    corr = hfl.correspondence_pairs_host(idx, mask)
    return hfl.consensus_registration_host([src], [dst], corr, distance_threshold=0.4, max_correspondence_distance=0.8), nrm


@pytest.mark.parametrize('seeds', rc.DENSITY_SEEDS)
def test_density_case_radius_beats_k_nearest(seeds):
    """A source of 226 points a face against an independent target of 904 a face, 40 degrees and 3 m apart.  Coarse pose
    errors (rotation, translation) of this route, `nb_neighbors=30` then radius 1.7 m (upward normals, mutual
    correspondences, `consensus_registration_host(distance_threshold=0.4, max_correspondence_distance=0.8)`):
        seeds (4, 54): 6.93 deg 1.43 m, then 0.412 deg 0.0431 m; refined from there 0.0945 deg 0.00687 m
        seeds (5, 55): 30.1 deg 2.71 m, then 5.25 deg 0.717 m; refined 0.143 deg 0.0131 m
        seeds (6, 56): 8.76 deg 0.719 m, then 2.13 deg 0.292 m; refined 0.144 deg 0.0191 m"""
    src, dst, truth = rc.density_pair(seeds)
    knn, _ = coarse_pose(src, dst, rc.DENSITY_NB, None)
    ball, nrm = coarse_pose(src, dst, None, rc.DENSITY_RADIUS)
    e_knn, e_ball = rc.density_errors(knn.transforms[0], truth), rc.density_errors(ball.transforms[0], truth)
    print('seeds %s: nb_neighbors=30 %.3g deg %.3g m, radius %.1f m %.3g deg %.3g m'
          % ((seeds,) + e_knn + (rc.DENSITY_RADIUS,) + e_ball))
    assert e_ball[0] < e_knn[0] and e_ball[1] < e_knn[1]
    fine = hfl.icp_refine_host([src], [dst], init=ball.transforms, estimation='point_to_plane', target_normals=[nrm[1]])
    print('refined: %.3g deg %.3g m' % rc.density_errors(fine.transforms[0], truth))
    assert fine.status.tolist() == [reg.CONVERGED]
