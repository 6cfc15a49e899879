"""The statistical outlier filter and the radius trim on the device (`csrc/outliers.hip`, `hotformerloc_amd/outliers.py`)
against the numpy route of the same module.  There is NO tolerance on avg, masks and rows: both routes follow one
definition in fp32, every operation rounded once, and the k smallest squared distances are found exactly whatever the
search grid.  mean / std / threshold are float64 sums taken in another fixed order: 1e-12 relative."""
import functools

import numpy as np
import pytest
import torch

from hotformerloc_amd import ground, load_config, model_factory, outliers, retrieval, voxel
from hotformerloc_amd import synthetic as syn
from tests import outlier_cases as oc

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 19, 20, 21, 63, 64, 65, 255, 256, 257)
NEIGHBOURS = (1, 2, 8, 9, 16, 17, 20, 32)
SPECIAL = {
    'lattice_ties': oc.lattice_ties,
    'duplicates': oc.duplicates,
    'gauss_offset': lambda: oc.gauss(3000, (100.0, -80.0, 30.0)),
    'flat': oc.flat,
    'clump_and_far': oc.clump_and_far,
    'gauss5000': lambda: oc.gauss(5003, seed=11),
}


@functools.lru_cache(maxsize=None)
def sized(n):
    return oc.gauss(n, seed=100 + n)


@functools.lru_cache(maxsize=None)
def host(key, nb=20):
    """the numpy route, computed once per cloud and shared: (cloud, kept, mask, avg, stats)"""
    cloud = sized(key) if isinstance(key, int) else SPECIAL[key]() if key in SPECIAL else RAGGED[key]()
    kept, mask, avg, stats = outliers.remove_outliers_host([cloud], nb, return_mask=True, return_distances=True,
                                                           return_stats=True)
    return cloud, kept[0], mask[0], avg[0], stats[0]


RAGGED = {'ragged1': lambda: sized(1), 'ragged300': lambda: oc.gauss(300, seed=7),
          'ragged4340': lambda: oc.forest_with_strays(0, 20.0)[0], 'ragged20': lambda: sized(20)}


def same_stat(got, want):
    if np.isnan(want):
        return np.isnan(got)
    return abs(got - want) <= 1e-12 * abs(want)


def check(device_out, keys, nb=20):
    kept, mask, avg, stats = device_out
    for i, key in enumerate(keys):
        cloud, h_kept, h_mask, h_avg, h_stats = host(key, nb)
        assert avg[i].dtype == torch.float32 and np.array_equal(avg[i].cpu().numpy().view(np.uint32), h_avg.view(np.uint32)), key
        assert mask[i].dtype == torch.bool and np.array_equal(mask[i].cpu().numpy(), h_mask), key
        assert kept[i].dtype == torch.float32 and tuple(kept[i].shape) == h_kept.shape, key
        assert np.array_equal(kept[i].cpu().numpy().view(np.uint32), h_kept.view(np.uint32)), key
        assert stats[i]['n_valid'] == h_stats['n_valid'], key
        for name in ('mean', 'std', 'threshold'):
            assert same_stat(stats[i][name], h_stats[name]), (key, name, stats[i][name], h_stats[name])


def run(clouds, nb=20, **kw):
    return outliers.remove_outliers(clouds, nb, return_mask=True, return_distances=True, return_stats=True, **kw)


# ---------------------------------------------------------------------------------------------- the filter
@pytest.mark.parametrize('n', SIZES)
def test_sizes_at_the_launch_boundaries(n):
    check(run([sized(n)]), [n])


def test_ragged_batch_in_one_call():
    keys = ['ragged1', 'ragged300', 'ragged4340', 'ragged20']
    check(run([host(k)[0] for k in keys]), keys)


@pytest.mark.parametrize('nb', NEIGHBOURS)
def test_both_sides_of_every_list_length(nb):
    cloud = oc.gauss(700, seed=21)
    kept, mask, avg, stats = run([cloud], nb)
    h_kept, h_mask, h_avg, h_stats = outliers.remove_outliers_host([cloud], nb, return_mask=True, return_distances=True,
                                                                   return_stats=True)
    assert np.array_equal(avg[0].cpu().numpy().view(np.uint32), h_avg[0].view(np.uint32))
    assert np.array_equal(mask[0].cpu().numpy(), h_mask[0]) and np.array_equal(kept[0].cpu().numpy(), h_kept[0])
    assert stats[0]['n_valid'] == h_stats[0]['n_valid']
    assert all(same_stat(stats[0][k], h_stats[0][k]) for k in ('mean', 'std', 'threshold'))


@pytest.mark.parametrize('name', list(SPECIAL))
def test_special_clouds(name):
    check(run([host(name)[0]]), [name])


def test_isolated_point_goes_through_the_whole_cloud_scan():
    cloud = host('clump_and_far')[0]
    avg, pending = outliers.knn_mean_distance([cloud], return_pending=True)
    assert pending >= 1
    assert np.array_equal(avg[0].cpu().numpy().view(np.uint32), host('clump_and_far')[3].view(np.uint32))
    one_cell, none = outliers.knn_mean_distance([cloud], cell_size=1e6, return_pending=True)
    assert none == 0 and torch.equal(one_cell[0], avg[0])                    # one cell: the block scan is the brute force


def test_cell_size_changes_no_bit():
    clouds = [host('ragged4340')[0], host('duplicates')[0]]
    base = run(clouds)
    check(base, ['ragged4340', 'duplicates'])
    for cell in (0.25, 4.0, 1e6):
        other = run(clouds, cell_size=cell)
        for i in range(2):
            assert torch.equal(base[0][i], other[0][i]) and torch.equal(base[1][i], other[1][i]), cell
            assert torch.equal(base[2][i].view(torch.int32), other[2][i].view(torch.int32)), cell
            assert base[3][i] == other[3][i], cell


def test_two_runs_give_the_same_bits():
    clouds = [host('ragged4340')[0], host('gauss_offset')[0]]
    a, b = run(clouds), run(clouds)
    for i in range(2):
        assert torch.equal(a[0][i], b[0][i]) and torch.equal(a[1][i], b[1][i])
        assert torch.equal(a[2][i].view(torch.int32), b[2][i].view(torch.int32)) and a[3][i] == b[3][i]


def test_device_resident_input_and_plain_return():
    cloud = host('ragged300')[0]
    out = outliers.remove_outliers([torch.from_numpy(cloud).cuda()])
    assert isinstance(out, list) and np.array_equal(out[0].cpu().numpy(), host('ragged300')[1])
    avg = outliers.knn_mean_distance([cloud, torch.from_numpy(cloud).cuda()])
    assert torch.equal(avg[0], avg[1]) and np.array_equal(avg[0].cpu().numpy(), host('ragged300')[3])


def test_errors_before_any_filter_kernel():
    cloud = sized(64)
    bad = cloud.copy()
    bad[5, 2] = np.nan
    with pytest.raises(ValueError, match='cloud 1 holds a coordinate that is not finite'):
        outliers.remove_outliers([cloud, bad])
    worse = cloud.copy()
    worse[0, 0] = np.inf
    with pytest.raises(ValueError, match='cloud 0 holds a coordinate that is not finite'):
        outliers.knn_mean_distance([worse, cloud])
    for nb in (0, 33):
        with pytest.raises(ValueError, match='nb_neighbors'):
            outliers.remove_outliers([cloud], nb)
    for ratio in (0.0, float('nan')):
        with pytest.raises(ValueError, match='std_ratio'):
            outliers.remove_outliers([cloud], 20, ratio)
    with pytest.raises(ValueError, match='cloud 1 is empty'):
        outliers.remove_outliers([cloud, np.zeros((0, 3), np.float32)])


# ---------------------------------------------------------------------------------------------- the radius trim
def test_trim_radius_boundary_and_empty_cloud():
    cloud, keep = oc.trim_boundary_cloud()
    batch = [cloud, cloud[~keep], cloud[::-1].copy()]
    out, mask = outliers.trim_radius(batch, 30.0, return_mask=True)
    h_out, h_mask = outliers.trim_radius_host(batch, 30.0, return_mask=True)
    assert np.array_equal(mask[0].cpu().numpy(), keep)
    for i in range(3):
        assert mask[i].dtype == torch.bool and np.array_equal(mask[i].cpu().numpy(), h_mask[i])
        assert tuple(out[i].shape) == h_out[i].shape and np.array_equal(out[i].cpu().numpy(), h_out[i])
    assert tuple(out[1].shape) == (0, 3)                                     # all outside: returned empty
    big = oc.gauss(5000, (10.0, 5.0, 0.0), seed=9) * np.float32(2.5)
    got = outliers.trim_radius([big])[0]
    assert np.array_equal(got.cpu().numpy(), outliers.trim_radius_host([big])[0]) and 0 < got.shape[0] < 5000


# ---------------------------------------------------------------------------------------------- the pipelines
@functools.lru_cache(maxsize=None)
def raw_submaps():
    """two forests with strays, moved so that the 30 m trim cuts a part of each"""
    a, b = oc.forest_with_strays(0, 20.0)[0], oc.forest_with_strays(1, 20.0)[0]
    return [a + np.array([12.0, 8.0, 0.0], np.float32), b + np.array([-30.0, -28.0, 2.0], np.float32)]


def cleaned(raw, radius=30.0):
    return outliers.remove_outliers(outliers.trim_radius(raw, radius))


def test_prepare_submaps_equals_the_chained_calls():
    raw = raw_submaps()
    got = voxel.prepare_submaps(raw, 0.8, radius_max=30, remove_outliers=True, remove_ground=True)
    trimmed = outliers.trim_radius(raw, 30)
    assert all(0 < t.shape[0] < r.shape[0] for t, r in zip(trimmed, raw))
    want = voxel.normalise_submaps(voxel.voxel_downsample(ground.remove_ground(outliers.remove_outliers(trimmed)), 0.8))
    assert len(got) == 2 and all(torch.equal(x, y) for x, y in zip(got, want))
    params = dict(nb_neighbors=8, std_ratio=1.5)
    got = voxel.prepare_submaps(raw, 0.8, normalise=False, remove_outliers=True, outlier_params=params)
    want = voxel.voxel_downsample(outliers.remove_outliers(raw, **params), 0.8)
    assert all(torch.equal(x, y) for x, y in zip(got, want))


def test_prepare_submaps_fixed_equals_the_chained_calls():
    from tests import ground_cases as gc
    raw = [gc.forest(0)[0] - np.array([20.0, 20.0, 0.0], np.float32)]
    got = voxel.prepare_submaps_fixed(raw, 4096, radius_max=25, remove_outliers=True, remove_ground=True)
    filtered = ground.remove_ground(cleaned(raw, 25))
    assert 4096 < filtered[0].shape[0] < raw[0].shape[0]
    want = voxel.normalise_submaps_padded(voxel.pnvlad_downsample(filtered, 4096), filtered, 4096)
    assert tuple(got[0].shape) == (4096, 3) and torch.equal(got[0], want[0])


def test_encode_clouds_cleans_the_raw_submaps_first():
    params, depth = load_config('wild-places')
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'stress')
    model = model.cuda()
    raw = raw_submaps()
    kw = dict(coordinates=params.coordinates, normalize=True, octree_depth=depth)
    got = retrieval.encode_clouds(model, raw, 2, radius_max=30, remove_outliers=True, voxel_size=0.8, normalise_submaps=True,
                                  **kw)
    want = retrieval.encode_clouds(model, cleaned(raw), 2, voxel_size=0.8, normalise_submaps=True, **kw)
    assert tuple(got.shape) == (2, 256) and bool(torch.isfinite(got).all())
    assert torch.equal(got, want)


PACKED_SIZES = (257, 1031, 643)             # odd: packed, the clouds start at rows that are no multiple of 4 (16 bytes)
PACKED_SHIFTS = ((6.0, 4.0, 0.0), (14.0, -30.0, 1.0), (-30.0, -28.0, 2.0))


@functools.lru_cache(maxsize=None)
def packed_submaps():
    """three 20 m forests cut to `PACKED_SIZES` rows, three in ten of them floor so that more than 128 rows outlast the
    cloth, and moved so that the 30 m trim cuts a part of each"""
    from tests import ground_cases as gc
    raw = []
    for seed, (n, shift) in enumerate(zip(PACKED_SIZES, PACKED_SHIFTS)):
        pts, is_ground, _ = gc.forest(seed, size=20.0, trunks_per_m2=10 / 400.0, blobs_per_m2=2 / 400.0)
        floor = int(n * 0.3)
        rows = np.sort(np.concatenate([np.flatnonzero(is_ground)[:floor], np.flatnonzero(~is_ground)[:n - floor]]))
        raw.append(pts[rows] + np.array(shift, np.float32))
    return raw


def test_packed_chain_equals_the_calls_chained_through_lists():
    """The chain keeps the batch packed between its steps, so a cloud starts wherever the compaction before it ends: after
    the trim the clouds start at rows 0, 250, 792, after the outlier filter at 0, 247, 779, after the cloth at 0, 208, 645,
    and a start at a row that is no multiple of 4 is not 16-byte aligned.  A chain through lists starts every cloud in a
    tensor of its own."""
    raw = packed_submaps()
    trimmed = outliers.trim_radius(raw, 30)
    assert all(128 < t.shape[0] < r.shape[0] for t, r in zip(trimmed, raw))   # the chain runs, no error path; some rows go
    filtered = ground.remove_ground(outliers.remove_outliers(trimmed))
    kw = dict(radius_max=30, remove_outliers=True, remove_ground=True)

    def both(chain, **more):
        """the batch through `chain`, after checking that every cloud alone gives the rows it gives in the batch"""
        got = chain(raw, **more, **kw)
        assert len(got) == 3 and all(torch.equal(chain([cloud], **more, **kw)[0], g) for cloud, g in zip(raw, got))
        return got

    got = both(voxel.prepare_submaps, voxel_size=0.8)
    want = voxel.normalise_submaps(voxel.voxel_downsample(filtered, 0.8))
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    got = both(voxel.prepare_submaps_fixed, target=128, downsample='pnvlad')
    want = voxel.normalise_submaps_padded(voxel.pnvlad_downsample(filtered, 128), filtered, 128)
    assert all(tuple(x.shape) == (128, 3) and torch.equal(x, y) for x, y in zip(got, want))
    got = both(voxel.prepare_submaps_fixed, target=128, downsample='random')
    want = voxel.normalise_submaps_padded(voxel.random_downsample(filtered, 128), filtered, 128)
    assert all(tuple(x.shape) == (128, 3) and torch.equal(x, y) for x, y in zip(got, want))

    params, depth = load_config('wild-places')                               # the branch only `encode_clouds` has: no downsample
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'stress')
    model = model.cuda()
    enc = dict(coordinates=params.coordinates, normalize=True, octree_depth=depth)
    got = retrieval.encode_clouds(model, raw, 3, remove_ground=True, normalise_submaps=True, **enc)
    want = retrieval.encode_clouds(model, voxel.normalise_submaps(ground.remove_ground(raw)), 3, **enc)
    assert tuple(got.shape) == (3, 256) and bool(torch.isfinite(got).all()) and torch.equal(got, want)


def test_pipeline_names_the_cloud_left_empty():
    raw = [raw_submaps()[0], raw_submaps()[1] + np.array([-100.0, 0.0, 0.0], np.float32)]
    with pytest.raises(ValueError, match='cloud 1 has no point left after the radius trim'):
        voxel.prepare_submaps(raw, 0.8, radius_max=30)
    lone = [sized(64), np.zeros((1, 3), np.float32)]                          # a single point is never kept
    with pytest.raises(ValueError, match='cloud 1 has no point left after outlier removal'):
        voxel.prepare_submaps(lone, 0.8, remove_outliers=True)
    with pytest.raises(ValueError, match='cloud 0 has .* points left after outlier removal, fewer than target = 65'):
        voxel.prepare_submaps_fixed(lone[:1], 65, remove_outliers=True)


def test_defaults_change_nothing():
    raw = raw_submaps()
    a = voxel.prepare_submaps(raw, 0.8)
    b = voxel.prepare_submaps(raw, 0.8, radius_max=None, remove_outliers=False, outlier_params=None)
    want = voxel.normalise_submaps(voxel.voxel_downsample(raw, 0.8))
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a, b, want))
