"""The numpy route of the statistical outlier filter and of the radius trim (`hotformerloc_amd/outliers.py`), the
definition the device route is held to, against an independent float64 route written here: `scipy.spatial.cKDTree.query`
on the fp32 inputs promoted to float64, then steps 2 to 5 of the definition in float64.

Bounds.  avg: 1e-5 relative -- about 25 fp32 roundings of 6e-8 each (three differences, five operations of a squared
distance, a root, up to 32 adds, a divide) on differences of fp32 inputs that are themselves exact to half an ulp.
mean / std / threshold: 1e-6 relative, averages of thousands of such values.  Masks: EQUAL, under a condition asserted on
the float64 side first: no point's float64 avg lies within 1e-5 relative of the float64 threshold (then an fp32 avg within
1e-5 of it cannot fall on the other side of a threshold that moved by 1e-6).  If a seed violates the condition, the seed
changes, never the band."""
import functools

import numpy as np
import pytest
from scipy.spatial import cKDTree

from hotformerloc_amd import outliers
from tests import ground_cases as gc
from tests import outlier_cases as oc

BAND = 1e-5


def reference64(cloud, nb=20, ratio=3.0):
    """-> (avg (n,) float64, mean, std, threshold, mask) by the KD-tree in float64"""
    p = np.asarray(cloud, np.float32).astype(np.float64)
    k = min(nb, p.shape[0])
    dist = np.asarray(cKDTree(p).query(p, k=k)[0], np.float64).reshape(p.shape[0], k)
    avg = dist.sum(axis=1) / k
    valid = avg > 0
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = avg[valid].sum() / valid.sum()
        std = np.sqrt(((avg[valid] - mean) ** 2).sum() / (valid.sum() - 1))
        threshold = mean + ratio * std
        return avg, mean, std, threshold, valid & (avg < threshold)


CASES = {
    'gauss': lambda: oc.gauss(3000),
    'gauss_offset': lambda: oc.gauss(3000, (100.0, -80.0, 30.0)),
    'duplicates': oc.duplicates,
    'lattice_ties': oc.lattice_ties,
    'gauss19': lambda: oc.gauss(19),
    'forest': lambda: gc.forest(0)[0],
}


@functools.lru_cache(maxsize=None)
def host_result(name):
    cloud = CASES[name]()
    kept, mask, avg, stats = outliers.remove_outliers_host([cloud], return_mask=True, return_distances=True,
                                                           return_stats=True)
    return cloud, kept[0], mask[0], avg[0], stats[0]


@pytest.mark.parametrize('name', list(CASES))
def test_host_route_against_float64_kdtree(name):
    cloud, kept, mask, avg, stats = host_result(name)
    ref_avg, mean, std, threshold, ref_mask = reference64(cloud)
    gap = np.abs(ref_avg[ref_avg > 0] - threshold).min() / threshold
    pos = ref_avg > 0
    err = (np.abs(avg[pos] - ref_avg[pos]) / ref_avg[pos]).max()
    print('%s: n %d removed %d closest to threshold %.3g avg err %.3g threshold err %.3g'
          % (name, len(cloud), int((~mask).sum()), gap, err, abs(stats['threshold'] - threshold) / threshold))
    assert gap > BAND                                                       # the condition under which the masks must be equal
    np.testing.assert_allclose(avg, ref_avg, rtol=1e-5, atol=0)
    assert avg.dtype == np.float32
    for key, want in (('mean', mean), ('std', std), ('threshold', threshold)):
        assert abs(stats[key] - want) <= 1e-6 * abs(want), key
    assert stats['n_valid'] == int((ref_avg > 0).sum())
    assert np.array_equal(mask, ref_mask)
    assert kept.dtype == np.float32 and np.array_equal(kept, cloud[mask])


def test_special_clouds_remove_what_they_should():
    assert int((~host_result('lattice_ties')[2]).sum()) == 1 and not host_result('lattice_ties')[2][-1]
    cloud, _, mask, avg, stats = host_result('duplicates')
    assert int((avg == 0).sum()) == 78 and stats['n_valid'] == len(cloud) - 78
    assert not mask[avg == 0].any()
    assert host_result('gauss19')[2].all()


def test_strays_go_and_the_forest_stays():
    cloud, is_stray = oc.forest_with_strays(0, 20.0)
    assert cloud.shape == (4340, 3) and int(is_stray.sum()) == oc.N_STRAYS
    mask = outliers.remove_outliers_host([cloud], return_mask=True)[1][0]
    assert not mask[is_stray].any()
    assert mask[~is_stray].mean() >= 0.98


def test_knn_mean_distance_host_is_steps_one_and_two():
    cloud = host_result('gauss')[0]
    assert np.array_equal(outliers.knn_mean_distance_host([cloud])[0], host_result('gauss')[3])
    few = outliers.knn_mean_distance_host([cloud[:200]], 5)[0]
    np.testing.assert_allclose(few, reference64(cloud[:200], 5)[0], rtol=1e-5)


def test_edge_sizes():
    one = outliers.remove_outliers_host([oc.gauss(1)], return_mask=True, return_stats=True)
    assert one[0][0].shape == (0, 3) and not one[1][0].any() and one[2][0]['n_valid'] == 0
    kept, mask, avg, stats = outliers.remove_outliers_host([oc.gauss(2)], return_mask=True, return_distances=True,
                                                           return_stats=True)
    # both valid, avg = half their distance each (the point itself is one of its two neighbours); one degree of freedom:
    # std = 0, the threshold is the mean, and `<` keeps neither
    assert stats[0]['n_valid'] == 2 and avg[0][0] == avg[0][1] > 0 and stats[0]['std'] == 0.0
    assert stats[0]['threshold'] == stats[0]['mean'] and not mask[0].any() and kept[0].shape == (0, 3)
    for n in (19, 20, 21):
        cloud = oc.gauss(n, seed=n)
        avg = outliers.knn_mean_distance_host([cloud])[0]
        np.testing.assert_allclose(avg, reference64(cloud)[0], rtol=1e-5)     # k = min(20, n)
    nothing = outliers.remove_outliers_host([oc.gauss(50)], 1, return_mask=True, return_distances=True, return_stats=True)
    assert not nothing[2][0].any() and not nothing[1][0].any() and nothing[3][0]['n_valid'] == 0
    assert np.isnan(nothing[3][0]['threshold'])


def test_single_valid_point_keeps_nothing():
    cloud = np.concatenate([np.zeros((30, 3), np.float32), [[5.0, 0.0, 0.0]]]).astype(np.float32)
    _, mask, stats = outliers.remove_outliers_host([cloud], return_mask=True, return_stats=True)
    assert stats[0]['n_valid'] == 1 and np.isnan(stats[0]['std']) and np.isnan(stats[0]['threshold']) and not mask[0].any()


def test_argument_errors():
    cloud = oc.gauss(30)
    for nb in (0, 33, 2.5, True):
        with pytest.raises(ValueError, match='nb_neighbors'):
            outliers.remove_outliers_host([cloud], nb)
        with pytest.raises(ValueError, match='nb_neighbors'):
            outliers.knn_mean_distance_host([cloud], nb)
    for ratio in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='std_ratio'):
            outliers.remove_outliers_host([cloud], 20, ratio)
    bad = cloud.copy()
    bad[7, 1] = np.nan
    with pytest.raises(ValueError, match='cloud 1 holds a coordinate that is not finite'):
        outliers.remove_outliers_host([cloud, bad])
    with pytest.raises(ValueError, match='cloud 1 is empty'):
        outliers.remove_outliers_host([cloud, np.zeros((0, 3), np.float32)])
    with pytest.raises(ValueError, match='cloud 0 is empty'):
        outliers.trim_radius_host([np.zeros((0, 3), np.float32)])
    for r in (0.0, -3.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='radius_max'):
            outliers.trim_radius_host([cloud], r)


def test_trim_radius_host():
    cloud, keep = oc.trim_boundary_cloud()
    out, mask = outliers.trim_radius_host([cloud, cloud[::-1], cloud[~keep]], 30.0, return_mask=True)
    assert np.array_equal(mask[0], keep) and np.array_equal(mask[1], keep[::-1])
    assert np.array_equal(out[0], cloud[keep]) and np.array_equal(out[1], cloud[::-1][keep[::-1]])      # order kept
    assert out[2].shape == (0, 3) and out[2].dtype == np.float32                                        # all outside
    assert np.array_equal(outliers.trim_radius_host([cloud])[0], cloud[keep])                           # 30 m by default
