"""Voxel-grid downsampling and submap normalisation on the device (`csrc/voxel.hip`, `hotformerloc_amd/voxel.py`) against
the numpy float64 route of the same module.  The margins are derived, not measured:

  * Cell membership is exact: both routes compute floor((float64(p) - origin) / v) with one float64 subtract and one
    divide, so the number of output points, the cells and the members per cell must match.
  * A mean may differ from the yardstick by at most one fp32 ulp (`np.spacing` of the yardstick value): both sum the same
    float64 terms, only the order is free, and its error of n 2^-53 relative to the largest partial sum -- 2^-29 times the
    fp32 spacing for the longest segment here -- can only move the final rounding to fp32 by one step.
  * Normalisation: the same one-ulp bound, plus an identical keep-mask.  The cases are built so that, in the yardstick
    alone, no scaled coordinate lies within 1e-9 of +-1 (asserted here, so that a flipped mask cannot be excused): the two
    routes' c and s differ by summation order only, about 1e-13 relative.  The one-ulp bound is met by coordinates whose
    distance to the centroid exceeds 2^24 times the difference of the two routes' centroids (about 1e-13 of the cloud's
    extent for these sums of up to 1.6e5 terms), i.e. a few micrometres in these clouds."""
import functools

import numpy as np
import pytest
import torch

from hotformerloc_amd import load_config, model_factory, retrieval, voxel
from hotformerloc_amd import synthetic as syn
from tests import voxel_cases as vc

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def downsample_case(name):
    """(clouds, v, yardstick means, counts, keys), computed once and shared"""
    clouds, v = vc.DOWNSAMPLE_CASES[name]()
    means, counts, keys = voxel.voxel_downsample_host(clouds, v, return_counts=True, return_keys=True)
    return clouds, v, means, counts, keys


@functools.lru_cache(maxsize=None)
def normalise_case(name):
    """(downsampled yardstick clouds, their yardstick normalisation)"""
    clouds, v = vc.normalise_case(name)
    down = voxel.voxel_downsample_host(clouds, v)
    return down, voxel.normalise_submaps_host(down)


def assert_within_one_ulp(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, what
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    worst = float((err / ulp).max()) if err.size else 0.0
    print('%s: %d values, %d differ, worst %.2f ulp' % (what, err.size, int((err > 0).sum()), worst))
    assert np.all(err <= ulp), '%s: worst %.2f ulp' % (what, worst)


# ---------------------------------------------------------------------------------------------- downsample against the host
@pytest.mark.parametrize('name', list(vc.DOWNSAMPLE_CASES))
def test_downsample_matches_host(name):
    clouds, v, means, counts, keys = downsample_case(name)
    got, got_counts, got_keys = voxel.voxel_downsample(clouds, v, return_counts=True, return_keys=True)
    assert len(got) == len(clouds)
    for i in range(len(clouds)):
        assert got[i].is_cuda and got[i].dtype == torch.float32 and got_counts[i].dtype == torch.int32
        assert tuple(got[i].shape) == means[i].shape, 'cloud %d: %d output points, yardstick %d' % (i, got[i].shape[0], len(means[i]))
        np.testing.assert_array_equal(got_keys[i].cpu().numpy(), keys[i])
        np.testing.assert_array_equal(got_counts[i].cpu().numpy(), counts[i])
        assert int(got_counts[i].sum()) == len(clouds[i])
        assert_within_one_ulp(got[i].cpu().numpy(), means[i], '%s cloud %d' % (name, i))


def test_cases_cover_what_they_claim():
    _, _, means, counts, _ = downsample_case('five_in_one_cell')
    assert counts[0].tolist() == [5]
    _, _, means, counts, _ = downsample_case('single_point')
    assert counts[0].tolist() == [1]
    _, _, _, counts, _ = downsample_case('long_segment_300')
    assert sorted(counts[0].tolist()) == [1, 1, 1, 300]
    _, _, _, counts, _ = downsample_case('threshold_segments')
    assert sorted(counts[0].tolist()) == sorted(vc.SEGMENT_LENGTHS)
    clouds, v, _, counts, _ = downsample_case('quarter_grid_faces')
    p = clouds[0].astype(np.float64)
    q = (p - (p.min(0) - 0.5 * v)) / v
    assert np.all(q * 2 == np.round(q * 2)) and int((q == np.floor(q)).sum()) > 1000 and p.min() < 0
    _, _, _, counts, _ = downsample_case('big_200k')
    assert 100000 < len(counts[0]) < 200000


def test_each_cloud_alone_equals_its_slice_of_the_batch():
    clouds, v, _, _, _ = downsample_case('ragged_1_257_4099')
    batched, batched_counts = voxel.voxel_downsample(clouds, v, return_counts=True)
    for i, cloud in enumerate(clouds):
        alone, alone_counts = voxel.voxel_downsample([cloud], v, return_counts=True)
        assert torch.equal(alone[0], batched[i]) and torch.equal(alone_counts[0], batched_counts[i])


@pytest.mark.parametrize('name', ['ragged_1_257_4099', 'big_200k'])
def test_two_calls_give_the_same_bits(name):
    clouds, v, _, _, _ = downsample_case(name)
    a = voxel.prepare_submaps(clouds[-1:], v)
    b = voxel.prepare_submaps(clouds[-1:], v)
    c = voxel.voxel_downsample(clouds, v)
    d = voxel.voxel_downsample(clouds, v)
    assert all(torch.equal(x, y) for x, y in zip(a + c, b + d))


@pytest.mark.parametrize('name', ['ragged_1_257_4099', 'utm_offset', 'with_outliers'])
def test_output_keys_strictly_ascending(name):
    clouds, v, _, _, _ = downsample_case(name)
    _, keys = voxel.voxel_downsample(clouds, v, return_keys=True)
    for k in keys:
        k = k.cpu().numpy()
        assert np.all(np.diff(k) > 0) and k.min() >= 0 and k.max() < (1 << 48)
        cells = np.stack([k >> 32, (k >> 16) & 0xFFFF, k & 0xFFFF], 1)
        assert np.array_equal(np.lexsort((cells[:, 2], cells[:, 1], cells[:, 0])), np.arange(len(k)))


def test_span_overflow_raises_and_returns_nothing():
    clouds, v = vc.overflow_batch()
    with pytest.raises(ValueError, match=r'cloud 1 spans 65536 or more'):
        voxel.voxel_downsample(clouds, v)
    with pytest.raises(ValueError, match=r'cloud 1 spans 65536 or more'):
        voxel.prepare_submaps(clouds, v)
    # the neighbours of the offending cloud are fine on their own, and the largest span that fits does fit
    ok = voxel.voxel_downsample([clouds[0], clouds[2]], v)
    want = voxel.voxel_downsample_host([clouds[0], clouds[2]], v)
    assert [tuple(t.shape) for t in ok] == [w.shape for w in want]
    edge = np.array([[0.0, 0, 0], [65534.0, 0, 0]], np.float32)
    assert voxel.voxel_downsample([edge], 1.0)[0].shape[0] == 2
    with pytest.raises(ValueError, match=r'cloud 0 spans'):
        voxel.voxel_downsample([edge + np.float32([[0, 0, 0], [1, 0, 0]])], 1.0)


# ---------------------------------------------------------------------------------------------- normalisation
@pytest.mark.parametrize('name', vc.NORMALISE_CASES)
def test_normalise_matches_host(name):
    down, want = normalise_case(name)
    for q32 in down:                                             # the yardstick alone: no scaled coordinate near +-1
        q = q32.astype(np.float64)
        c = q.mean(0)
        s = 0.5 / np.sqrt(((q - c) ** 2).sum(1)).mean()
        assert np.abs(np.abs(s * (q - c)) - 1.0).min() > 1e-9
    got = voxel.normalise_submaps(down)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert tuple(g.shape) == w.shape, 'cloud %d: kept %d, yardstick %d' % (i, g.shape[0], len(w))
        assert_within_one_ulp(g.cpu().numpy(), w, '%s normalised cloud %d' % (name, i))
    if name == 'with_outliers':
        assert all(len(w) < len(d) for w, d in zip(want, down))  # the mask does something here


def test_normalise_single_point_raises():
    good = vc.box_cloud(5, 100)
    with pytest.raises(ValueError, match='cloud 1 cannot be normalised'):
        voxel.normalise_submaps([good, np.ones((1, 3), np.float32), good])
    clouds, v = vc.single_point()
    with pytest.raises(ValueError, match='cloud 0 cannot be normalised'):
        voxel.prepare_submaps(clouds, v)


@pytest.mark.parametrize('name', ['ragged_257_4099', 'with_outliers'])
def test_prepare_submaps_equals_the_two_calls(name):
    clouds, v = vc.normalise_case(name)
    fused = voxel.prepare_submaps(clouds, v)
    chained = voxel.normalise_submaps(voxel.voxel_downsample(clouds, v))
    assert len(fused) == len(chained) == len(clouds)
    assert all(torch.equal(a, b) for a, b in zip(fused, chained))
    only = voxel.prepare_submaps(clouds, v, normalise=False)
    assert all(torch.equal(a, b) for a, b in zip(only, voxel.voxel_downsample(clouds, v)))


# ---------------------------------------------------------------------------------------------- up to the descriptors
def test_encode_clouds_from_raw_submaps():
    params, depth = load_config('wild-places')
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'stress')
    model = model.cuda()
    raw = [syn.raw_submap(100 + i, n, extent=60.0) for i, n in enumerate((6000, 4500, 7001))]
    kw = dict(coordinates=params.coordinates, normalize=True, octree_depth=depth)
    got = retrieval.encode_clouds(model, raw, 2, voxel_size=0.8, normalise_submaps=True, **kw)
    prepared = voxel.prepare_submaps(raw[:2], 0.8) + voxel.prepare_submaps(raw[2:], 0.8)
    assert all(300 < p.shape[0] < 6000 for p in prepared)
    want = retrieval.encode_clouds(model, prepared, 2, **kw)
    assert tuple(got.shape) == (3, 256) and bool(torch.isfinite(got).all())
    assert torch.equal(got, want)
