"""Fixed-size submaps on the device (`hfl_voxel_occupancy`, `hfl_voxel_gather_rows`, `hfl_submap_normalise_rows` in
`csrc/voxel.hip`; `voxel_occupancy`, `pnvlad_downsample`, `random_downsample`, `normalise_submaps_padded`,
`prepare_submaps_fixed` in `hotformerloc_amd/voxel.py`) against the numpy float64 route of the same module.

  * Occupied-cell counts, the voxel size a search ends on (a float64 formed on the host by the same operations) and every
    probe of the search are exact: cell membership is bit-identical between the routes (tests/test_gpu_voxel.py).
  * Rows gathered from the raw cloud are copies: bit-equal.
  * Voxel means and normalised rows follow the rule of tests/test_gpu_voxel.py: the same cells / the same keep-mask, values
    within one fp32 ulp of the yardstick (the routes differ by float64 summation order only).  For the mask to be
    comparable, no scaled coordinate of the yardstick -- of the downsampled rows and of every raw row the padding could
    draw -- may lie within 1e-9 of +-1; that is asserted on the yardstick alone."""
import functools

import numpy as np
import pytest
import torch

from hotformerloc_amd import load_config, model_factory, ops, retrieval, voxel
from hotformerloc_amd import synthetic as syn
from tests import fixed_submaps_cases as fc
from tests.test_gpu_voxel import assert_within_one_ulp

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def occupancy_table():
    clouds = fc.occupancy_batch()
    return clouds, voxel.voxel_occupancy_host(clouds, fc.OCCUPANCY_SIZES)


@functools.lru_cache(maxsize=None)
def searched(name):
    """(clouds, target, host search, host downsample), computed once and shared"""
    clouds, target = fc.PNVLAD_CASES[name]()
    return clouds, target, voxel.pnvlad_search_host(clouds, target), voxel.pnvlad_downsample_host(clouds, target)


def bitmap_bytes(cloud, v):
    p = cloud.astype(np.float64)
    dims = np.floor((p.max(0) - (p.min(0) - 0.5 * v)) / v) + 1
    return 4 * ((int(np.prod(dims)) + 31) // 32)


# ---------------------------------------------------------------------------------------------- occupancy
def test_occupancy_matches_host():
    clouds, want = occupancy_table()
    got = voxel.voxel_occupancy(clouds, fc.OCCUPANCY_SIZES)
    assert got.is_cuda and got.dtype == torch.int32
    print(got.cpu().numpy())
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    faces = voxel.voxel_occupancy([fc.quarter_grid()], fc.FACE_SIZES)
    np.testing.assert_array_equal(faces.cpu().numpy(), voxel.voxel_occupancy_host([fc.quarter_grid()], fc.FACE_SIZES))


def test_occupancy_of_a_cloud_alone_equals_its_row_of_the_batch():
    clouds, want = occupancy_table()
    for i, cloud in enumerate(clouds):
        np.testing.assert_array_equal(voxel.voxel_occupancy([cloud], fc.OCCUPANCY_SIZES).cpu().numpy()[0], want[i])


def test_occupancy_across_the_budget_boundary(monkeypatch):
    clouds, want = occupancy_table()
    calls = {'sort': 0, 'bitmap': 0}
    by_sort, by_bitmap = voxel._count_by_sort, ops.voxel_occupancy
    monkeypatch.setattr(voxel, '_count_by_sort', lambda *a: (calls.__setitem__('sort', calls['sort'] + 1), by_sort(*a))[1])
    monkeypatch.setattr(ops, 'voxel_occupancy', lambda *a: (calls.__setitem__('bitmap', calls['bitmap'] + 1), by_bitmap(*a))[1])
    # 4 KiB: the candidates at 3.001 .. 1.0 fit (several per call, several calls), the finer ones go through the sort
    got = voxel.voxel_occupancy(clouds, fc.OCCUPANCY_SIZES, budget_bytes=4096)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert calls['sort'] >= 5 and calls['bitmap'] >= 2, calls
    # exactly at the boundary: a budget of the bitmap's own size takes the bitmap, four bytes less take the sort
    cloud, v = clouds[4], fc.OCCUPANCY_SIZES[3]
    nbytes = bitmap_bytes(cloud, v)
    for budget, route in ((nbytes, 'bitmap'), (nbytes - 4, 'sort')):
        calls.update(sort=0, bitmap=0)
        got = voxel.voxel_occupancy([cloud], [v], budget_bytes=budget)
        assert int(got[0, 0]) == int(want[4, 3]) and calls[route] == 1 and sum(calls.values()) == 1, (budget, calls)


def test_occupancy_span_error_names_the_cloud():
    wide = np.array([[0.0, 0.0, 0.0], [70000.0, 0.0, 0.0]], np.float32)
    with pytest.raises(ValueError, match=r'cloud 1 spans 65536 or more'):
        voxel.voxel_occupancy([fc.scene(5, 300), wide], [3.001, 1.0])


# ---------------------------------------------------------------------------------------------- pnvlad
@pytest.mark.parametrize('name', list(fc.PNVLAD_CASES))
def test_pnvlad_matches_host(name):
    clouds, target, found, want = searched(name)
    got, sizes = voxel.pnvlad_downsample(clouds, target, return_voxel_sizes=True)
    dev_found, stats = voxel.pnvlad_search(clouds, target, return_stats=True)
    print(name, 'rounds', stats['rounds'], 'candidates', stats['candidates'])
    for i, (cloud, g, v, f, d, w) in enumerate(zip(clouds, got, sizes, found, dev_found, want)):
        assert v == f['voxel_size'] == d['voxel_size'] and isinstance(v, float)  # the same float64
        assert d['trace'] == f['trace'] and d['count'] == f['count']             # every probe the reference makes
        assert (d['phase_one_steps'], d['phase_two_steps']) == (f['phase_one_steps'], f['phase_two_steps'])
        m = f['count']
        assert g.is_cuda and g.dtype == torch.float32 and tuple(g.shape) == (target, 3)
        means, keys = voxel.voxel_downsample([cloud], v, return_keys=True)
        assert torch.equal(g[:m], means[0])                                       # the same device route
        _, host_keys = voxel.voxel_downsample_host([cloud], v, return_keys=True)
        np.testing.assert_array_equal(keys[0].cpu().numpy(), host_keys[0])
        assert_within_one_ulp(g[:m].cpu().numpy(), w[:m], '%s cloud %d means' % (name, i))
        index = np.random.default_rng(42).choice(len(cloud), size=target - m)
        np.testing.assert_array_equal(g[m:].cpu().numpy(), cloud[index])
        np.testing.assert_array_equal(g[m:].cpu().numpy(), w[m:])
    if name == 'mixed_rounds_64':
        assert stats['candidates'][0] == voxel.PNVLAD_K_ONE and stats['rounds'] > 4        # one round against many
    if name == 'general_1024':
        assert stats['rounds'] >= 3


def test_pnvlad_search_through_the_sort_fallback():
    clouds, target, found, _ = searched('general_256')
    # 64 bytes hold 512 cells: the coarse candidates of these 20 - 30 m scenes fit, the finer ones go through the sort
    dev, stats = voxel.pnvlad_search(clouds, target, budget_bytes=64, return_stats=True)
    print(stats)
    assert stats['sort_fallbacks'] > 0 and stats['occupancy_calls'] > 0
    assert [d['trace'] for d in dev] == [f['trace'] for f in found]


def test_pnvlad_seed_and_two_calls():
    clouds, target, _, _ = searched('general_256')
    a = voxel.pnvlad_downsample(clouds, target, seed=7)
    b = voxel.pnvlad_downsample(clouds, target, seed=7)
    want = voxel.pnvlad_downsample_host(clouds, target, seed=7)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    for x, w in zip(a, want):
        assert_within_one_ulp(x.cpu().numpy(), w, 'seed 7')


# ---------------------------------------------------------------------------------------------- random
def test_random_downsample_is_bit_equal_to_host():
    clouds = fc.occupancy_batch()
    for target in (64, 1024):
        got = voxel.random_downsample(clouds, target)
        want = voxel.random_downsample_host(clouds, target)
        for g, w in zip(got, want):
            assert g.is_cuda and tuple(g.shape) == (target, 3)
            np.testing.assert_array_equal(g.cpu().numpy(), w)


# ---------------------------------------------------------------------------------------------- padded normalisation
@pytest.mark.parametrize('downsample', ['pnvlad', 'random'])
def test_normalise_padded_matches_host(downsample):
    raw, target = fc.with_outliers()
    down = voxel.pnvlad_downsample_host(raw, target) if downsample == 'pnvlad' else voxel.random_downsample_host(raw, target)
    for q32, r32 in zip(down, raw):                              # the yardstick alone: no scaled coordinate near +-1
        q = q32.astype(np.float64)
        c = q.mean(0)
        s = 0.5 / np.sqrt(((q - c) ** 2).sum(1)).mean()
        assert np.abs(np.abs(s * (q - c)) - 1.0).min() > 1e-9
        assert np.abs(np.abs(s * (r32.astype(np.float64) - c)) - 1.0).min() > 1e-9
    want = voxel.normalise_submaps_padded_host(down, raw, target)
    got = voxel.normalise_submaps_padded(down, raw, target)
    plain = voxel.normalise_submaps(down)
    assert sum(int(p.shape[0]) < target for p in plain) >= 2
    for i, (g, w, p) in enumerate(zip(got, want, plain)):
        assert g.is_cuda and g.dtype == torch.float32 and tuple(g.shape) == (target, 3)
        assert torch.equal(g[:p.shape[0]], p)                                     # the unpadded call, bit for bit
        assert float(g.abs().max()) <= 1.0
        assert_within_one_ulp(g.cpu().numpy(), w, '%s padded cloud %d' % (downsample, i))
    again = voxel.normalise_submaps_padded(down, raw, target)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def test_normalise_padded_errors():
    good = fc.scene(5, 300, extent=20.0)
    with pytest.raises(ValueError, match='cloud 1 cannot be normalised'):
        voxel.normalise_submaps_padded([good, good[:1]], [good, good], 512)
    with pytest.raises(ValueError, match='cloud 0 keeps .* more than target'):
        voxel.normalise_submaps_padded([good], [good], 8)


# ---------------------------------------------------------------------------------------------- the chain
@pytest.mark.parametrize('downsample', ['pnvlad', 'random'])
def test_prepare_submaps_fixed_equals_the_chained_calls(downsample):
    raw, target = fc.with_outliers()
    fused = voxel.prepare_submaps_fixed(raw, target, downsample=downsample)
    down = voxel.pnvlad_downsample(raw, target) if downsample == 'pnvlad' else voxel.random_downsample(raw, target)
    chained = voxel.normalise_submaps_padded(down, raw, target)
    assert len(fused) == len(raw) and all(tuple(f.shape) == (target, 3) for f in fused)
    assert all(torch.equal(a, b) for a, b in zip(fused, chained))
    again = voxel.prepare_submaps_fixed(raw, target, downsample=downsample)
    assert all(torch.equal(a, b) for a, b in zip(fused, again))
    only = voxel.prepare_submaps_fixed(raw, target, downsample=downsample, normalise=False)
    assert all(torch.equal(a, b) for a, b in zip(only, down))
    with pytest.raises(ValueError, match="'pnvlad' or 'random'"):
        voxel.prepare_submaps_fixed(raw, target, downsample='voxel')


def test_encode_clouds_from_fixed_size_submaps():
    params, depth = load_config('wild-places')
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'stress')
    model = model.cuda()
    raw = [syn.raw_submap(100 + i, n, extent=60.0) for i, n in enumerate((6000, 4500, 7001))]
    kw = dict(coordinates=params.coordinates, normalize=True, octree_depth=depth)
    got = retrieval.encode_clouds(model, raw, 2, downsample_target=1024, normalise_submaps=True, **kw)
    prepared = voxel.prepare_submaps_fixed(raw[:2], 1024) + voxel.prepare_submaps_fixed(raw[2:], 1024)
    want = retrieval.encode_clouds(model, prepared, 2, **kw)
    assert tuple(got.shape) == (3, 256) and bool(torch.isfinite(got).all())
    assert torch.equal(got, want)
    rand = retrieval.encode_clouds(model, raw, 3, downsample_target=1024, downsample_type='random', normalise_submaps=True, **kw)
    assert torch.equal(rand, retrieval.encode_clouds(model, voxel.prepare_submaps_fixed(raw, 1024, downsample='random'), 3, **kw))
    # the default call is unchanged: no target, no fixed-size route
    assert torch.equal(want, retrieval.encode_clouds(model, prepared, 2, downsample_target=None, **kw))
    with pytest.raises(ValueError, match='exclude each other'):
        retrieval.encode_clouds(model, raw, 2, downsample_target=1024, voxel_size=0.8, **kw)


# ---------------------------------------------------------------------------------------------- errors before any launch
def test_errors_are_raised_before_anything_is_uploaded(monkeypatch):
    def no_upload(*args):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(voxel, '_upload', no_upload)
    good = fc.scene(5, 300, extent=20.0)
    with pytest.raises(ValueError, match='cloud 1 has 63 points, fewer than target = 64'):
        voxel.pnvlad_downsample([good, good[:63]], 64)
    with pytest.raises(ValueError, match='cloud 0 has 1 points'):
        voxel.prepare_submaps_fixed([good[:1]], 64)
    for bad in (0, -1):
        with pytest.raises(ValueError, match='target must be a positive integer'):
            voxel.pnvlad_downsample([good], bad)
        with pytest.raises(ValueError, match='target must be a positive integer'):
            voxel.random_downsample([good], bad)
        with pytest.raises(ValueError, match='target must be a positive integer'):
            voxel.normalise_submaps_padded([good], [good], bad)


def test_search_that_cannot_reach_the_target_names_the_cloud():
    good = fc.scene(5, 300, extent=20.0)
    tight = np.concatenate([np.zeros((299, 3), np.float32), np.float32([[40.0, 0, 0]])])
    with pytest.raises(ValueError, match='cloud 1 never reaches 64 occupied voxels'):
        voxel.pnvlad_downsample([good, tight], 64)
