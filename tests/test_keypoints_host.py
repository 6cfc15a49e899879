"""ISS keypoints on the CPU: the numpy routes of `keypoints.py` against an independent transcription of the six steps, one
point at a time (`tests/keypoint_cases.py`), the figures the definition was measured at, its guards, its refusals, and the
wiring into `global_registration_host` and `rerank_candidates_host`."""
import importlib

import numpy as np
import pytest

import hotformerloc_amd as hfl
from hotformerloc_amd import build, keypoints
from tests import fpfh_cases as fc
from tests import global_registration_cases as gc
from tests import keypoint_cases as kc
from tests import spectral_cases as sc

GR = importlib.import_module('hotformerloc_amd.global_registration')


# ------------------------------------------------------------------------------------------------ the transcription
@pytest.mark.parametrize('key, radii', [('plane37', (3.0, 2.0)), ('duplicated', (1.5, 1.0)), (257, (1.5, 1.0)),
                                        ('planes', (1.5, 1.0)), ('planes', (1.0, 1.5)), (4, (1.5, 1.0))])
def test_twins_against_the_transcription_point_by_point(key, radii):
    cloud = kc.cloud_of(key)
    kc.guard_gamma(key, radii[0])
    sal, counts, _ = kc.host_saliency(key, radii[0])
    t_sal, t_counts, _ = kc.saliency_scalar(cloud, radii[0])
    assert sal.dtype == np.float32 and counts.dtype == np.int32
    assert np.array_equal(counts, t_counts)
    assert np.array_equal(sal > 0, t_sal > 0)
    assert (np.abs(sal.astype(np.float64) - t_sal.astype(np.float32)) <= kc.value_bound(key, radii[0])).all()
    keys = hfl.iss_select_host([cloud], [sal], radii[1])[0]
    assert keys.dtype == np.int64 and np.array_equal(keys, kc.select_scalar(cloud, sal, radii[1]))
    both, both_sal = hfl.iss_keypoints_host([cloud], *radii, return_saliency=True)
    assert np.array_equal(both[0], keys) and np.array_equal(both_sal[0].view(np.int32), sal.view(np.int32))
    mask = hfl.iss_select_host([cloud], [sal], radii[1], return_mask=True)[0]
    assert mask.dtype == bool and np.array_equal(np.nonzero(mask)[0], keys)


@pytest.mark.parametrize('key', kc.NAMED + kc.SIZES)
def test_counts_are_the_radius_counts(key):
    for rs, _ in kc.RADII:
        assert np.array_equal(kc.host_saliency(key, rs)[1], hfl.radius_neighbour_counts_host([kc.cloud_of(key)], rs)[0])


@pytest.mark.parametrize('n', [1, 2, 4])
def test_clouds_below_min_neighbors_have_no_keypoint(n):
    keys, sal = hfl.iss_keypoints_host([kc.cloud_of(n)], 1e4, 1e4, return_saliency=True)
    assert keys[0].shape == (0,) and keys[0].dtype == np.int64 and not sal[0].any()


def test_other_parameters_against_the_transcription():
    cloud = kc.cloud_of('planes')
    for g21, g32, nb in ((0.8, 0.5, 5), (1.0, 1.0, 1), (0.975, 0.975, 40)):
        kc.guard_gamma('planes', 1.5, g21, g32, nb)
        sal = hfl.iss_saliency_host([cloud], 1.5, gamma_21=g21, gamma_32=g32, min_neighbors=nb)[0]
        assert np.array_equal(sal > 0, kc.saliency_scalar(cloud, 1.5, g21, g32, nb)[0] > 0)
        keys = hfl.iss_keypoints_host([cloud], 1.5, 1.0, gamma_21=g21, gamma_32=g32, min_neighbors=nb)[0]
        assert np.array_equal(keys, kc.select_scalar(cloud, sal, 1.0, nb))


# ------------------------------------------------------------------------------------------------ the measured figures
@pytest.mark.parametrize('radii', kc.RADII)
def test_planes_keypoints_and_their_guards(radii):
    keys = kc.host_keypoints('planes', *radii)
    assert keys.shape[0] == kc.PLANES_KEYPOINTS[radii]
    assert np.array_equal(kc.host_keypoints('planes_moved', *radii), keys)      # the saliency is translation invariant
    for key in ('planes', 'planes_moved'):
        kc.guard_gamma(key, radii[0])
        kc.guard_ties(key, *radii)
    # the finding behind the fp32 rounding and the index rule: ball neighbours with bit-equal fp32 saliency exist
    ties = kc.fp32_ties('planes', *radii)
    print('%s: %d keypoints, %d fp32 ties' % (radii, keys.shape[0], ties))
    assert ties > 0


def test_guards_hold_on_every_cloud_the_device_is_compared_on():
    for key in kc.GUARDED:
        for rs, rn in kc.RADII:
            kc.guard_gamma(key, rs)
            kc.guard_ties(key, rs, rn)
    kc.guard_gamma('planes', 3.0)
    with pytest.raises(AssertionError):
        kc.guard_gamma('collinear', 1.5)


# ------------------------------------------------------------------------------------------------ ties and the boundary
@pytest.mark.parametrize('key', ['planes', 'duplicated', 'collinear', 257, 2])
def test_integer_saliency_the_index_rule_decides(key):
    cloud, sal = kc.cloud_of(key), kc.integer_saliency(key)
    for rn in (1.0, 2.5):
        keys = hfl.iss_select_host([cloud], [sal], rn)[0]
        assert np.array_equal(keys, kc.select_scalar(cloud, sal, rn))
    ones = np.ones(cloud.shape[0], np.float32)                       # all tied: the lowest index of every ball
    keys = hfl.iss_select_host([cloud], [ones], 1e4, min_neighbors=1)[0]
    assert keys.tolist() == [0]


def test_lattice_boundary_is_inclusive():
    cloud, _ = fc.lattice()
    sal = np.random.default_rng(5).integers(0, 4, 125).astype(np.float32)
    at = hfl.iss_select_host([cloud], [sal], kc.LATTICE_RADIUS)[0]
    below = hfl.iss_select_host([cloud], [sal], kc.LATTICE_RADIUS_BELOW)[0]
    assert np.array_equal(at, kc.lattice_select_exact(sal, 5)) and np.array_equal(below, kc.lattice_select_exact(sal, 4))
    assert not np.array_equal(at, below)


def test_a_nan_saliency_is_no_candidate_and_beats_nobody():
    cloud = kc.cloud_of('plane37')
    sal = np.full(37, np.nan, np.float32)
    sal[7], sal[11] = 1.0, -1.0
    assert hfl.iss_select_host([cloud], [sal], 1e4)[0].tolist() == [7]


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    cloud = kc.cloud_of('plane37')
    for bad in (0.0, -1.0, float('nan'), float('inf'), 1e39, 'a', None, True):
        with pytest.raises(ValueError):
            hfl.iss_saliency_host([cloud], bad)
        with pytest.raises(ValueError):
            hfl.iss_select_host([cloud], [np.zeros(37, np.float32)], bad)
        with pytest.raises(ValueError):
            hfl.iss_keypoints_host([cloud], 1.0, bad)
    for bad in (0.0, 1.5, -0.1, float('nan'), 'a', True):
        with pytest.raises(ValueError):
            hfl.iss_saliency_host([cloud], 1.0, gamma_21=bad)
        with pytest.raises(ValueError):
            hfl.iss_keypoints_host([cloud], 1.0, 1.0, gamma_32=bad)
    for bad in (0, -3, 2.5, True, 2 ** 31):
        with pytest.raises(ValueError):
            hfl.iss_saliency_host([cloud], 1.0, min_neighbors=bad)
        with pytest.raises(ValueError):
            hfl.iss_select_host([cloud], [np.zeros(37, np.float32)], 1.0, min_neighbors=bad)
    with pytest.raises(ValueError):
        hfl.iss_select_host([cloud], [np.zeros(36, np.float32)], 1.0)
    with pytest.raises(ValueError):
        hfl.iss_select_host([cloud], [], 1.0)
    with pytest.raises(TypeError):
        hfl.iss_select_host([cloud], [np.zeros(37, np.float64)], 1.0)
    with pytest.raises(ValueError):
        hfl.iss_keypoints_host([np.zeros((0, 3), np.float32)], 1.0, 1.0)
    with pytest.raises(ValueError):
        hfl.iss_keypoints_host([np.array([[0, 0, np.inf]], np.float32)], 1.0, 1.0)
    assert hfl.iss_keypoints_host([], 1.0, 1.0) == []


def test_the_kernels_are_built_like_the_search_they_share():
    assert 'keypoints.hip' in build.SOURCES and build.EXTRA_FLAGS['keypoints.hip'] == build.EXTRA_FLAGS['normals.hip']


# ------------------------------------------------------------------------------------------------ the wiring
def test_global_registration_on_keypoints():
    src, dst = gc.clouds()
    coarse, fine = hfl.global_registration_host([src], [dst], salient_radius=1.5, non_max_radius=1.0)
    angle, shift = gc.pose_error(fine.transforms[0])
    print('%.3g degrees, %.3g m, %d inliers of the coarse pose' % (angle, shift, coarse.inliers[0]))
    assert angle <= gc.ANGLE_TOL_DEG and shift <= gc.SHIFT_TOL
    # the coarse pose rests on the keypoints' correspondences alone: 38 mutual ones, every one of them true
    keys = [kc.host_keypoints('planes', 1.5, 1.0), kc.host_keypoints('planes_moved', 1.5, 1.0)]
    feats = [fc.host_fpfh(k)[0][rows] for k, rows in zip(('planes', 'planes_moved'), keys)]
    matched = hfl.feature_correspondences_host([feats[0]], [feats[1]], mutual=True)
    pairs = hfl.correspondence_pairs_host(matched[0], matched[2])[0]
    assert pairs.shape[0] == 38 and np.array_equal(keys[0][pairs[:, 0]], keys[1][pairs[:, 1]])
    assert coarse.inliers[0] == 38 and coarse.fitness[0] == 1.0


def test_a_cloud_without_a_keypoint_ends_no_hypothesis_and_enters_the_icp_at_the_identity():
    src = kc.cloud_of('plane37')
    assert kc.host_keypoints('plane37', 1.5, 1.0).shape[0] == 0
    coarse, fine = hfl.global_registration_host([src, gc.clouds()[0]], [src, gc.clouds()[1]], salient_radius=1.5,
                                                non_max_radius=1.0)
    assert coarse.status.tolist()[0] == GR.NO_HYPOTHESIS and np.array_equal(coarse.transforms[0], np.eye(4))
    assert gc.pose_error(fine.transforms[0], np.eye(4)[:3])[0] <= gc.ANGLE_TOL_DEG      # the cloud against itself
    assert gc.pose_error(fine.transforms[1])[0] <= gc.ANGLE_TOL_DEG                     # the other pair is untouched


def test_rerank_on_keypoints_keeps_the_true_candidate_first():
    queries, database, cand = sc.rerank_inputs()
    res = hfl.rerank_candidates_host(queries, database, cand, salient_radius=1.5, non_max_radius=1.0)
    assert sc.DATABASE[res.indices[0, 0]] == 'planes' and res.indices[0, -1] == -1
    # the query's number of keypoints takes the place of its size: 38 of 38 consistent correspondences score near 1
    assert 0.9 < res.scores[0, 0] <= 1.0
    ranked, coarse, fine = hfl.rerank_candidates_host(queries, database, cand, salient_radius=1.5, non_max_radius=1.0,
                                                      register=True)
    assert np.array_equal(ranked.indices, res.indices)
    angle, shift = gc.pose_error(fine.transforms[0], sc.rerank_truth())
    assert angle <= gc.ANGLE_TOL_DEG and shift <= gc.SHIFT_TOL


def test_wiring_refusals():
    src, dst = gc.clouds()
    queries, database, cand = sc.rerank_inputs()
    for kw in (dict(salient_radius=1.5), dict(non_max_radius=1.0), dict(salient_radius=0.0, non_max_radius=1.0),
               dict(salient_radius=1.5, non_max_radius=float('nan')), dict(salient_radius='a', non_max_radius=1.0)):
        with pytest.raises(ValueError):
            hfl.global_registration_host([src], [dst], **kw)
        with pytest.raises(ValueError):
            hfl.rerank_candidates_host(queries, database, cand, **kw)
    assert keypoints.check_radii(None, None) is None
