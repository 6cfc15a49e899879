"""The definition of `hotformerloc_amd/fpfh.py` on the host: argument checks, the defined edge cases, the bin rules against
independent transcriptions, and the brute-force matcher.  No GPU."""
import math

import numpy as np
import pytest
import torch

import hotformerloc_amd as hfl
from hotformerloc_amd import _native, fpfh
from tests import fpfh_cases as fc


def host(cloud, nrm, nb=30):
    out = fpfh.compute_fpfh_host([cloud], [nrm], nb, return_histograms=True)
    return tuple(o[0] for o in out)


# ------------------------------------------------------------------------------------------------ arguments
def test_public_names():
    for name in ('compute_fpfh', 'compute_fpfh_host', 'feature_correspondences', 'feature_correspondences_host'):
        assert getattr(hfl, name) is getattr(fpfh, name)


@pytest.mark.parametrize('nb', [2, 33, 0, -1, True, 30.0, '30'])
def test_rejects_bad_neighbour_counts(nb):
    cloud, nrm = fc.cloud_of('plane37'), fc.host_normals('plane37')
    with pytest.raises(ValueError):
        fpfh.compute_fpfh_host([cloud], [nrm], nb)
    with pytest.raises(ValueError):
        fpfh.compute_fpfh([cloud], [nrm], nb)                       # before the device is touched


@pytest.mark.parametrize('route', [fpfh.compute_fpfh_host, fpfh.compute_fpfh])
def test_rejects_bad_clouds_and_normals(route):
    cloud, nrm = fc.cloud_of('plane37'), fc.host_normals('plane37')
    with pytest.raises(ValueError):
        route([cloud], [nrm[:-1]])
    with pytest.raises(ValueError):
        route([cloud], [nrm[:, :2]])
    with pytest.raises(ValueError):
        route([cloud, cloud], [nrm])
    with pytest.raises(ValueError):
        route([np.zeros((0, 3), np.float32)], [np.zeros((0, 3), np.float32)])


def test_rejects_non_finite_coordinates():
    cloud = fc.cloud_of('plane37').copy()
    cloud[5, 1] = np.inf
    with pytest.raises(ValueError, match='cloud 0'):
        fpfh.compute_fpfh_host([cloud], [fc.host_normals('plane37')])


def test_device_route_refuses_the_cpu():
    cloud, nrm = fc.cloud_of('plane37'), fc.host_normals('plane37')
    with pytest.raises(_native.NativeLibraryError):
        fpfh.compute_fpfh([cloud], [nrm], device='cpu')
    with pytest.raises(_native.NativeLibraryError):
        fpfh.feature_correspondences([torch.zeros(3, 4)], [torch.zeros(2, 4)])


@pytest.mark.parametrize('route', [fpfh.feature_correspondences_host, fpfh.feature_correspondences])
def test_rejects_bad_feature_rows(route):
    rows = lambda n, d: torch.zeros((n, d), dtype=torch.float32)      # noqa: E731
    with pytest.raises(ValueError):
        route([rows(3, 0)], [rows(2, 0)])
    with pytest.raises(ValueError):
        route([rows(3, 65)], [rows(2, 65)])
    with pytest.raises(ValueError):
        route([rows(3, 4), rows(1, 4)], [rows(2, 4)])
    with pytest.raises(ValueError):
        route([rows(3, 4)], [rows(2, 5)])
    with pytest.raises(ValueError):
        route((rows(3, 4), np.array([0, 2])), (rows(2, 4), np.array([0, 2])))
    with pytest.raises(TypeError):
        route([rows(3, 4).double()], [rows(2, 4).double()])


# ------------------------------------------------------------------------------------------------ defined edge cases
def test_single_point_has_no_pairs():
    out, hist, pairs = host(np.array([[1.0, 2.0, 3.0]], np.float32), np.array([[0.0, 0.0, 1.0]], np.float32))
    assert out.shape == (1, 33) and out.dtype == np.float32 and hist.dtype == np.int32 and pairs.dtype == np.int32
    assert not out.any() and not hist.any() and pairs[0] == 0


def test_two_points():
    cloud = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], np.float32)
    nrm = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0]], np.float32)
    out, hist, pairs = host(cloud, nrm)
    assert pairs.tolist() == [1, 1] and hist.sum(1).tolist() == [3, 3]
    # a1 = a2 = 0: no swap; v = dp x n = (0, -1, 0) for point 0; f2 = 0 and f3 = 0: bin 5; x = 1, y = 0: theta = 0, bin 5
    assert np.array_equal(hist[0], hist[1]) and hist[0, 5] == 1 and hist[0, 16] == 1 and hist[0, 27] == 1
    assert np.allclose(out.reshape(2, 3, 11).sum(2), 200.0, atol=1e-3)


def test_fewer_points_than_neighbours():
    cloud, nrm = fc.cloud_of('plane37')[:9], fc.host_normals('plane37')[:9]
    _, hist, pairs = host(cloud, nrm, 30)                          # k = 9: every point is every point's neighbour
    s_hist, s_pairs = fc.spfh_scalar(cloud, nrm, 30)
    assert np.array_equal(hist, s_hist) and np.array_equal(pairs, s_pairs)
    assert (pairs == 8).all()


def test_duplicated_points_are_skipped_and_weightless():
    cloud = fc.cloud_of('duplicated')
    nrm = fc.host_normals('duplicated')
    out, hist, pairs = fc.host_fpfh('duplicated')
    assert np.isfinite(out).all()
    # the 13 copies of point 0 are each other's nearest neighbours and form no pair with each other
    copies = np.nonzero((cloud == cloud[0]).all(1))[0]
    assert len(copies) == 13
    s_hist, s_pairs = fc.spfh_scalar(cloud, nrm, 30)
    assert np.array_equal(hist, s_hist) and np.array_equal(pairs, s_pairs)
    assert np.array_equal(hist[copies], np.repeat(hist[copies[:1]], 13, 0))
    assert np.all(np.abs(out[copies].astype(np.float64) - out[copies[:1]]) <= np.spacing(out[copies[:1]]))
    groups = out.reshape(-1, 3, 11).sum(2)
    assert np.all((np.abs(groups - 200.0) <= 1e-3) | (np.abs(groups - 100.0) <= 1e-3) | (groups == 0.0))


def test_collinear_cloud_is_all_zero():
    assert not fc.host_normals('collinear').any()
    out, hist, pairs = fc.host_fpfh('collinear')
    assert not out.any() and not hist.any() and not pairs.any()


def test_one_point_without_a_normal():
    cloud, nrm = fc.cloud_of('plane37'), fc.host_normals('plane37').copy()
    full_hist = fc.host_fpfh('plane37')[1]
    nrm[7] = 0.0
    out, hist, pairs = host(cloud, nrm)
    assert pairs[7] == 0 and not hist[7].any()
    assert out[7].any()                                            # its neighbours' histograms still reach it
    assert np.allclose(out[7].reshape(3, 11).sum(1), 100.0, atol=1e-3)
    assert (hist.sum(1) == 3 * pairs).all() and (hist <= full_hist).all()
    nrm[7] = np.nan                                                # a row that is not finite says the same
    assert np.array_equal(host(cloud, nrm)[1], hist)


@pytest.mark.parametrize('key', ['plane37', 'planes700', 'duplicated'])
def test_groups_sum_to_100_and_200(key):
    out, hist, pairs = fc.host_fpfh(key)
    assert (hist.reshape(-1, 3, 11).sum(2) == pairs[:, None]).all()
    spfh = np.where(pairs[:, None] > 0, 100.0 * hist / np.maximum(pairs, 1)[:, None], 0.0)
    own = spfh.reshape(-1, 3, 11).sum(2)
    assert np.all((np.abs(own - 100.0) <= 1e-3) | (own == 0.0))
    weighted = (out.astype(np.float64) - spfh).reshape(-1, 3, 11).sum(2)
    assert np.all((np.abs(weighted - 100.0) <= 1e-3) | (np.abs(weighted) <= 1e-3))
    assert (np.abs(weighted - 100.0) <= 1e-3).any() and (pairs > 0).any()


def test_lattice_ties_edges_and_row_order():
    cloud, nrm = fc.lattice()
    out, hist, pairs = host(cloud, nrm, 7)
    s_hist, s_pairs = fc.spfh_scalar(cloud, nrm, 7)
    assert np.array_equal(hist, s_hist) and np.array_equal(pairs, s_pairs)
    # an interior point has six neighbours at distance 1: with k = 5 they tie at the k-th place and all are taken, so its
    # neighbourhood, and its histogram, is that of k = 7
    inner = np.nonzero(((cloud >= 1) & (cloud <= 3)).all(1))[0]
    assert len(inner) == 27 and pairs[inner].min() > 0
    assert np.array_equal(host(cloud, nrm, 5)[1][inner], hist[inner])
    assert not np.array_equal(host(cloud, nrm, 5)[1], hist)        # a corner has three at distance 1 and three at sqrt 2
    perm = np.random.default_rng(0).permutation(125)
    p_out, p_hist, p_pairs = host(cloud[perm], nrm[perm], 7)
    assert np.array_equal(p_hist, hist[perm]) and np.array_equal(p_pairs, pairs[perm])
    assert np.all(np.abs(p_out.astype(np.float64) - out[perm]) <= np.spacing(np.maximum(out[perm], p_out)))


# ------------------------------------------------------------------------------------------------ the bin rules
def test_theta_rule_agrees_with_atan2():
    rng = np.random.default_rng(5)
    edges = -math.pi + 2.0 * math.pi * np.arange(0, 12) / 11.0
    theta = np.concatenate([rng.uniform(-math.pi, math.pi, 20000), [0.0, math.pi / 2, -math.pi / 2, math.pi - 1e-6],
                            (edges[:, None] + np.array([-2e-9, 2e-9])[None, :]).reshape(-1)])
    theta = theta[(np.abs(theta[:, None] - edges[None, :]).min(1) >= 1e-9) & (np.abs(theta) <= math.pi)]
    radius = rng.uniform(1e-3, 2.0, theta.shape)
    x, y = radius * np.cos(theta), radius * np.sin(theta)
    want = np.floor(11.0 * (np.arctan2(y, x) + math.pi) / (2.0 * math.pi)).astype(np.int64)
    got = fpfh._theta_bins(x, y)
    assert np.array_equal(got, want)
    assert got.min() == 0 and got.max() == 10
    assert np.array_equal(got, [fc.theta_bin_scalar(a, b) for a, b in zip(x.tolist(), y.tolist())])
    zero = np.array([0.0, -0.0])
    assert fpfh._theta_bins(zero, zero).tolist() == [5, 5]
    assert fpfh._theta_bins(np.array([1.0, -1.0, 1.0]), np.array([0.0, 0.0, -0.0])).tolist() == [5, 10, 5]


def test_swap_rule_against_the_scalar_transcription():
    rng = np.random.default_rng(9)
    m = 4000
    pi, pj = rng.normal(0.0, 1.0, (m, 3)).astype(np.float32), rng.normal(0.0, 1.0, (m, 3)).astype(np.float32)
    ni, nj = rng.normal(0.0, 1.0, (m, 3)), rng.normal(0.0, 1.0, (m, 3))
    ni, nj = (ni / np.linalg.norm(ni, axis=1, keepdims=True)).astype(np.float32), \
        (nj / np.linalg.norm(nj, axis=1, keepdims=True)).astype(np.float32)
    pj[:50] = pi[:50]                                               # coincident points: skipped
    ni[50:100] = ((pj[50:100] - pi[50:100]) * 2.0).astype(np.float32)
    nj[50:100] = ni[50:100] * 0.25                                  # dp parallel to the source normal: often |v| = 0
    valid, bins = fpfh._pair_bins(*(a.astype(np.float64) for a in (pi, ni, pj, nj)))
    want = [fc.pair_bins_scalar(pi[r], ni[r], pj[r], nj[r]) for r in range(m)]
    assert valid.tolist() == [w is not None for w in want]
    assert not valid[:50].any() and valid[100:].all()
    assert bins[valid].tolist() == [list(w) for w in want if w is not None]
    swapped = np.abs(((ni * (pj - pi)).sum(1))) < np.abs(((nj * (pj - pi)).sum(1)))
    assert 0.3 < swapped.mean() < 0.7                               # both branches are taken


def test_spfh_against_the_scalar_transcription():
    cloud, nrm = fc.cloud_of('plane37'), fc.host_normals('plane37')
    for nb in (3, 10, 32):
        _, hist, pairs = host(cloud, nrm, nb)
        s_hist, s_pairs = fc.spfh_scalar(cloud, nrm, nb)
        assert np.array_equal(hist, s_hist) and np.array_equal(pairs, s_pairs)


# ------------------------------------------------------------------------------------------------ the matcher
def test_matcher_ties_go_to_the_lowest_index():
    src = np.array([[1.0, 1.0], [5.0, 5.0], [3.0, 3.0]], np.float32)
    dst = np.array([[2.0, 2.0], [0.0, 0.0], [2.0, 2.0], [1.0, 1.0], [1.0, 1.0], [4.0, 4.0]], np.float32)
    idx, dist2 = fpfh.feature_correspondences_host([src], [dst])
    assert idx[0].tolist() == [3, 5, 0] and idx[0].dtype == np.int32
    assert dist2[0].tolist() == [0.0, 2.0, 2.0] and dist2[0].dtype == np.float32


def test_matcher_identical_rows_and_empty_sides():
    same = np.tile(np.arange(33, dtype=np.float32), (7, 1))
    idx, dist2 = fpfh.feature_correspondences_host([same, same[:3], same[:0]], [same, same[:0], same[:2]])
    assert idx[0].tolist() == [0] * 7 and dist2[0].tolist() == [0.0] * 7
    assert idx[1].tolist() == [-1] * 3 and np.isposinf(dist2[1]).all()
    assert idx[2].shape == (0,) and dist2[2].shape == (0,)
    rows = np.concatenate([same, same[:3]])
    flat_idx, flat_d2, mask = fpfh.feature_correspondences_host((rows, np.array([0, 7, 10, 10])),
                                                                (rows[:9], np.array([0, 7, 7, 9])), mutual=True)
    assert flat_idx.tolist() == [0] * 7 + [-1] * 3 and flat_d2.shape == (10,)
    assert mask.tolist() == [True] + [False] * 9                   # target 0's nearest source is row 0, the lowest index


def test_matcher_mutual_mask_by_hand():
    src = np.array([[0.0], [10.0], [4.0]], np.float32)
    dst = np.array([[1.0], [9.0], [2.0]], np.float32)
    # source -> target: 0 -> 0 (1), 10 -> 1 (1), 4 -> 2 (4);  target -> source: 1 -> 0, 9 -> 1, 2 -> both 0 and 4 at 4: row 0
    idx, dist2, mask = fpfh.feature_correspondences_host([src], [dst], mutual=True)
    assert idx[0].tolist() == [0, 1, 2] and dist2[0].tolist() == [1.0, 1.0, 4.0]
    assert mask[0].tolist() == [True, True, False]


def test_matcher_chain_is_the_fmaf_chain():
    rng = np.random.default_rng(2)
    q, t = rng.normal(0, 1, (5, 33)).astype(np.float32), rng.normal(0, 1, (9, 33)).astype(np.float32)
    idx, dist2 = fpfh.feature_correspondences_host([q], [t])
    for r in range(5):
        d = q[r] - t[idx[0][r]]
        acc = np.float32(d[0] * d[0])
        for c in range(1, 33):
            acc = np.float32(np.float64(d[c]) * np.float64(d[c]) + np.float64(acc))
        assert acc == dist2[0][r]
    exact = ((q[:, None, :].astype(np.float64) - t[None].astype(np.float64)) ** 2).sum(2)
    assert np.array_equal(idx[0], exact.argmin(1))


def test_real_fpfh_rows_meet_the_gap_condition():
    """what `tests/test_gpu_fpfh.py` asks of its real-descriptor case, checked where no GPU is needed: at most 1 % of the rows
    have a best and a second-best squared distance within 4 fp32 ulps"""
    src, dst = fc.host_fpfh('planes')[0], fc.host_fpfh('planes_moved')[0]
    sure = fc.ulp_gap_rows(src, dst)
    print('rows within 4 ulps: %d of %d' % ((~sure).sum(), sure.shape[0]))
    assert (~sure).mean() <= 0.01
