"""FPFH descriptors and feature correspondences on the device (`csrc/fpfh.hip`, `hotformerloc_amd/fpfh.py`) against the
numpy routes of the same module.

Comparison rule.  hist and pairs: EQUAL to the bit -- integers over a neighbourhood that is a pure function of the input.
FPFH: within one fp32 ulp -- the float64 sums are taken in another order, about 1e-14 of a sum of non-negative terms, and
the result is rounded once.  Correspondences: idx equal and dist2 bit-equal; on real descriptors idx is compared on the rows
whose best and second-best host d2 differ by more than 4 ulps, at most 1 % are left out, which is asserted."""
import numpy as np
import pytest
import torch

from hotformerloc_amd import fpfh, normals, outliers
from tests import fpfh_cases as fc

pytestmark = pytest.mark.gpu

BATCH = ('one', 'two', 'plane37', 'planes700')
SMALL_CELL = 0.25                      # the outliers of 'planes700' sit alone in their 3 x 3 x 3 blocks


def within_one_ulp(device, host):
    d, h = device.astype(np.float64), host.astype(np.float64)
    return bool(np.all(np.abs(d - h) <= np.spacing(np.maximum(np.abs(device), np.abs(host)))))


def run(keys, nb=30, **kw):
    out = fpfh.compute_fpfh([fc.cloud_of(k) for k in keys], [fc.host_normals(k, nb) for k in keys], nb,
                            return_histograms=True, return_pending=True, **kw)
    return [[t.cpu().numpy() for t in part] for part in out[:3]] + [out[3]]


def check(out, keys, nb=30):
    feat, hist, pairs, _ = out
    for i, key in enumerate(keys):
        h_feat, h_hist, h_pairs = fc.host_fpfh(key, nb)
        assert feat[i].dtype == np.float32 and hist[i].dtype == np.int32 and pairs[i].dtype == np.int32
        assert feat[i].shape == h_feat.shape
        assert np.array_equal(hist[i], h_hist), key
        assert np.array_equal(pairs[i], h_pairs), key
        err = np.abs(feat[i].astype(np.float64) - h_feat) / np.spacing(np.maximum(np.abs(h_feat), np.float32(1e-30)))
        print('%s nb=%d: fpfh off by at most %.3g ulp' % (key, nb, err.max()))
        assert within_one_ulp(feat[i], h_feat), key


def test_ragged_batch_default_and_small_cells():
    default, small = run(BATCH), run(BATCH, cell_size=SMALL_CELL)
    check(default, BATCH)
    check(small, BATCH)
    assert small[3] > 0                                            # the whole-cloud scan finished the outliers
    for a, b in zip(default[1] + default[2], small[1] + small[2]):
        assert np.array_equal(a, b)
    for a, b in zip(default[0], small[0]):
        assert within_one_ulp(a, b)
    again = run(BATCH, cell_size=SMALL_CELL)
    for part, part_again in zip(small[:3], again[:3]):
        for a, b in zip(part, part_again):
            assert np.array_equal(a, b)                            # two runs, the same bits
    assert again[3] == small[3]


@pytest.mark.parametrize('nb', [3, 8, 9, 16, 17, 32])
def test_every_list_length(nb):
    keys = ('plane37', 'duplicated')
    check(run(keys, nb), keys, nb)


def test_lattice_and_duplicates_bit_equal():
    cloud, nrm = fc.lattice()
    clouds, nrms = [cloud, fc.cloud_of('duplicated')], [nrm, fc.host_normals('duplicated', 7)]
    for cell in (None, 0.75):
        feat, hist, pairs = fpfh.compute_fpfh(clouds, nrms, 7, cell_size=cell, return_histograms=True)
        h_feat, h_hist, h_pairs = fpfh.compute_fpfh_host(clouds, nrms, 7, return_histograms=True)
        for i in range(2):
            assert np.array_equal(hist[i].cpu().numpy(), h_hist[i]) and np.array_equal(pairs[i].cpu().numpy(), h_pairs[i])
            assert within_one_ulp(feat[i].cpu().numpy(), h_feat[i])
    perm = np.random.default_rng(1).permutation(125)
    _, p_hist, _ = fpfh.compute_fpfh([cloud[perm]], [nrm[perm]], 7, return_histograms=True)
    assert np.array_equal(p_hist[0].cpu().numpy(), h_hist[0][perm])


def test_points_without_normals_and_collinear():
    nrm = fc.host_normals('plane37').copy()
    nrm[7], nrm[20] = 0.0, np.nan
    clouds, nrms = [fc.cloud_of('plane37'), fc.cloud_of('collinear')], [nrm, fc.host_normals('collinear')]
    feat, hist, pairs = fpfh.compute_fpfh(clouds, nrms, return_histograms=True)
    h_feat, h_hist, h_pairs = fpfh.compute_fpfh_host(clouds, nrms, return_histograms=True)
    for i in range(2):
        assert np.array_equal(hist[i].cpu().numpy(), h_hist[i]) and np.array_equal(pairs[i].cpu().numpy(), h_pairs[i])
        assert within_one_ulp(feat[i].cpu().numpy(), h_feat[i])
    assert pairs[0][7] == 0 and pairs[0][20] == 0 and feat[0][7].any()
    assert not feat[1].any()


def test_device_normals_feed_straight_in():
    keys = ('plane37', 'planes700')
    clouds = [torch.from_numpy(np.array(fc.cloud_of(k))).cuda() for k in keys]
    nrm = normals.estimate_normals(clouds, 30, viewpoint=np.array(fc.VIEW))
    assert all(n.is_cuda for n in nrm)
    feat, hist, pairs = fpfh.compute_fpfh(clouds, nrm, return_histograms=True)
    h_feat, h_hist, h_pairs = fpfh.compute_fpfh_host([fc.cloud_of(k) for k in keys], [n.cpu().numpy() for n in nrm],
                                                     return_histograms=True)
    for i in range(2):
        assert feat[i].is_cuda and feat[i].shape == (clouds[i].shape[0], 33)
        assert np.array_equal(hist[i].cpu().numpy(), h_hist[i]) and np.array_equal(pairs[i].cpu().numpy(), h_pairs[i])
        assert within_one_ulp(feat[i].cpu().numpy(), h_feat[i])


def test_non_finite_coordinates_name_the_cloud():
    bad = fc.cloud_of('plane37').copy()
    bad[3, 2] = np.nan
    with pytest.raises(ValueError, match='cloud 1'):
        fpfh.compute_fpfh([fc.cloud_of('plane37'), bad], [fc.host_normals('plane37')] * 2)


# ------------------------------------------------------------------------------------------------ correspondences
@pytest.mark.parametrize('dim', [1, 4, 33, 64])
def test_correspondences_on_integer_rows(dim):
    src, dst = fc.integer_features(dim)
    h_idx, h_d2, h_mask = fpfh.feature_correspondences_host(list(src), list(dst), mutual=True)
    idx, d2, mask = fpfh.feature_correspondences([torch.from_numpy(np.array(s)).cuda() for s in src],
                                                 [torch.from_numpy(np.array(t)).cuda() for t in dst], mutual=True)
    for p in range(len(fc.PAIR_SIZES)):
        assert idx[p].dtype == torch.int32 and d2[p].dtype == torch.float32 and mask[p].dtype == torch.bool
        assert np.array_equal(idx[p].cpu().numpy(), h_idx[p]), p
        assert np.array_equal(d2[p].cpu().numpy().view(np.uint32), h_d2[p].view(np.uint32)), p
        assert np.array_equal(mask[p].cpu().numpy(), h_mask[p]), p
    assert (h_idx[1] == -1).all() and np.isposinf(h_d2[1]).all() and not h_mask[1].any()
    # the ragged layout gives the same answer as the lists
    rows = lambda parts: torch.from_numpy(np.concatenate(parts)).cuda()       # noqa: E731
    off = lambda parts: np.concatenate([[0], np.cumsum([len(x) for x in parts])])  # noqa: E731
    flat_idx, flat_d2 = fpfh.feature_correspondences((rows(src), off(src)), (rows(dst), torch.from_numpy(off(dst))))
    assert torch.equal(flat_idx, torch.cat(idx)) and torch.equal(flat_d2, torch.cat(d2))


def test_correspondences_on_real_descriptors():
    src, dst = fc.host_fpfh('planes')[0], fc.host_fpfh('planes_moved')[0]
    h_idx, h_d2 = fpfh.feature_correspondences_host([src], [dst])
    idx, d2 = fpfh.feature_correspondences([torch.from_numpy(np.array(src)).cuda()], [torch.from_numpy(np.array(dst)).cuda()])
    assert np.array_equal(d2[0].cpu().numpy().view(np.uint32), h_d2[0].view(np.uint32))
    sure = fc.ulp_gap_rows(src, dst)
    assert (~sure).mean() <= 0.01
    assert np.array_equal(idx[0].cpu().numpy()[sure], h_idx[0][sure])


def test_descriptors_find_the_moved_copy():
    """two copies of the three-plane cloud, the second turned by 40 degrees about z and shifted by 3 m: mutual FPFH matches
    land within the point spacing of the truth, matches by nearest coordinates do not"""
    r, t = fc.rotation_z()
    src, dst = fc.cloud_of('planes'), fc.cloud_of('planes_moved')
    clouds = [torch.from_numpy(np.array(c)).cuda() for c in (src, dst)]
    views = np.stack([np.array(fc.VIEW), r @ np.array(fc.VIEW) + t])
    nrm = normals.estimate_normals(clouds, 30, viewpoint=views)
    feat = fpfh.compute_fpfh(clouds, nrm)
    truth = torch.from_numpy(src.astype(np.float64) @ r.T + t).cuda()
    target = clouds[1].double()

    def median_error(a, b):
        idx, _, mask = fpfh.feature_correspondences([a], [b], mutual=True)
        assert int(mask[0].sum()) >= 20
        return float((truth[mask[0]] - target[idx[0][mask[0]].long()]).norm(dim=1).median())

    spacing = 2.0 * float(outliers.knn_mean_distance([clouds[0]], 2)[0].mean())       # k = 2: the point itself and its nearest
    by_features, by_coordinates = median_error(feat[0], feat[1]), median_error(clouds[0], clouds[1])
    print('spacing %.4f m, median error by features %.3g m, by coordinates %.3g m' % (spacing, by_features, by_coordinates))
    assert by_features < spacing
    assert by_coordinates > by_features
