"""The numpy float64 route of the fixed-size submap functions (`hotformerloc_amd/voxel.py`: `voxel_occupancy_host`,
`pnvlad_downsample_host`, `random_downsample_host`, `normalise_submaps_padded_host`) against literal, loop-by-loop
transcriptions of the reference's `processing_utils.pnvlad_down_sample`, `random_down_sample` and `normalise_pcl`, kept
here.  In the transcriptions `voxel_downsample_host` stands for open3d's `voxel_down_sample` and the module's s (q - c) for
open3d's `transform`; open3d's row order is unspecified, so voxel means are compared as sets of rows.  No GPU."""
import functools

import numpy as np
import pytest

from hotformerloc_amd import voxel
from tests import fixed_submaps_cases as fc

VOXEL_STEP = 0.01


# ---------------------------------------------------------------------------------------------- transcriptions
def ref_pnvlad_down_sample(points, downsample_number, random_seed=42):
    rng = np.random.default_rng(seed=random_seed)
    voxel_size = 3.001
    trace = []

    def down(v):
        out = voxel.voxel_downsample_host([points], v)[0]
        trace.append((v, len(out)))
        return out
    cloud_downsampled = down(voxel_size)
    while len(cloud_downsampled) < downsample_number:
        voxel_size -= VOXEL_STEP
        if voxel_size <= 0:
            raise AssertionError('cloud smaller than the target with 1cm voxels')
        cloud_downsampled = down(voxel_size)
    while len(cloud_downsampled) > downsample_number:
        voxel_size += VOXEL_STEP / 5
        cloud_downsampled = down(voxel_size)
    num_extra_points = downsample_number - len(cloud_downsampled)
    rand_points = rng.choice(points, size=num_extra_points)
    return cloud_downsampled, rand_points, voxel_size, trace


def ref_random_down_sample(points, downsample_number, random_seed=42):
    rng = np.random.default_rng(seed=random_seed)
    return rng.choice(points, downsample_number)


def ref_normalise_pcl(points_downsampled, points, downsample_number, random_seed=42):
    rng = np.random.default_rng(seed=random_seed)
    points_downsampled = points_downsampled.astype(np.float64)
    points = points.astype(np.float64)
    centroid = np.mean(points_downsampled, 0)
    d = np.sqrt(((points_downsampled - centroid) ** 2).sum(axis=1)).mean()
    s = 0.5 / d
    transform = lambda q: s * (q - centroid)                                      # noqa: E731
    pts_scaled = transform(points_downsampled)
    pts_final = pts_scaled[np.all(np.abs(pts_scaled) <= 1, axis=1)]
    iterations = 0
    if downsample_number is not None:
        num_extra_points = downsample_number - len(pts_final)
        pts_final = np.copy(pts_final)
        points_added = 0
        while len(pts_final) < downsample_number:
            rand_points = rng.choice(points, size=(num_extra_points - points_added))
            rand_points = transform(rand_points)
            rand_points = rand_points[np.all(np.abs(rand_points) <= 1, axis=1)]
            points_added += len(rand_points)
            pts_final = np.concatenate((pts_final, rand_points))
            iterations += 1
        assert len(pts_final) == downsample_number
    assert pts_final.min() >= -1 and pts_final.max() <= 1
    return pts_final.astype(np.float32), iterations


def as_row_set(a):
    return set(map(tuple, np.asarray(a).tolist()))


@functools.lru_cache(maxsize=None)
def searched(name):
    clouds, target = fc.PNVLAD_CASES[name]()
    return clouds, target, voxel.pnvlad_search_host(clouds, target)


# ---------------------------------------------------------------------------------------------- occupancy
def test_occupancy_is_the_length_of_the_downsample():
    clouds = fc.occupancy_batch()
    got = voxel.voxel_occupancy_host(clouds, fc.OCCUPANCY_SIZES)
    assert got.dtype == np.int32 and got.shape == (len(clouds), len(fc.OCCUPANCY_SIZES))
    for j, v in enumerate(fc.OCCUPANCY_SIZES):
        want = [len(d) for d in voxel.voxel_downsample_host(clouds, v)]
        assert got[:, j].tolist() == want
    faces = voxel.voxel_occupancy_host([fc.quarter_grid()], fc.FACE_SIZES)
    assert faces[0].tolist() == [len(voxel.voxel_downsample_host([fc.quarter_grid()], v)[0]) for v in fc.FACE_SIZES]


def test_occupancy_cases_cover_what_they_claim():
    clouds = fc.occupancy_batch()
    offsets = np.cumsum([0] + [len(c) for c in clouds])
    assert any(o % 4 for o in offsets[1:-1]) and max(len(c) for c in clouds) > 2 * 8192
    big = clouds[1].astype(np.float64)
    cells = lambda v: np.prod(np.floor((big.max(0) - big.min(0) + 0.5 * v) / v) + 1)        # noqa: E731
    assert cells(1.0) <= 8192 * 32 < cells(0.25)                                 # both sides of the LDS bitmap
    p = fc.quarter_grid().astype(np.float64)
    for v in fc.FACE_SIZES:
        q = (p - (p.min(0) - 0.5 * v)) / v
        assert np.all(q * 8 == np.round(q * 8)) and int((q == np.floor(q)).sum()) > 500
    assert np.abs(clouds[2]).max() > 6.0e6


# ---------------------------------------------------------------------------------------------- pnvlad
@pytest.mark.parametrize('name', list(fc.PNVLAD_CASES))
def test_pnvlad_matches_the_transcription(name):
    clouds, target, found = searched(name)
    got, sizes = voxel.pnvlad_downsample_host(clouds, target, return_voxel_sizes=True)
    for cloud, g, v, f in zip(clouds, got, sizes, found):
        means, rand, ref_v, trace = ref_pnvlad_down_sample(cloud, target)
        assert v == ref_v == f['voxel_size'] and f['trace'] == trace              # the same float64, probe by probe
        m = len(means)
        assert g.dtype == np.float32 and g.shape == (target, 3) and m == f['count'] <= target
        assert as_row_set(g[:m]) == as_row_set(means) and len(as_row_set(means)) == m
        np.testing.assert_array_equal(g[m:], rand)
        np.testing.assert_array_equal(g[:m], voxel.voxel_downsample_host([cloud], v)[0])       # ascending cell order


def test_pnvlad_cases_cover_what_they_claim():
    for name in fc.GENERAL_CASES:
        for f in searched(name)[2]:
            assert f['phase_one_steps'] >= 3 and f['phase_two_steps'] >= 2, (name, f['phase_one_steps'], f['phase_two_steps'])
            assert f['voxel_size'] < 3.0
    assert max(f['phase_one_steps'] for f in searched('general_1024')[2]) > 2 * voxel.PNVLAD_K_ONE
    f = searched('over_at_start_64')[2][0]
    assert f['phase_one_steps'] == 0 and f['phase_two_steps'] > 100 and f['trace'][0][1] > 64
    f = searched('lattice_exact_64')[2][0]
    assert f['trace'] == [(3.001, 64)]
    f = searched('exact_hit_64')[2][0]
    assert f['phase_one_steps'] >= 3 and f['phase_two_steps'] == 0 and f['count'] == 64
    first, long, _ = searched('mixed_rounds_64')[2]
    assert len(first['trace']) == 1 and long['phase_two_steps'] > 4 * voxel.PNVLAD_K_ONE
    assert np.abs(searched('utm_256')[0][0]).max() > 6.0e6


def test_candidate_sizes_are_formed_by_repeated_steps():
    f = searched('general_256')[2][0]
    v, want = 3.001, []
    for _ in range(f['phase_one_steps']):
        v -= 0.01
        want.append(v)
    for _ in range(f['phase_two_steps']):
        v += 0.01 / 5
        want.append(v)
    assert [t[0] for t in f['trace'][1:]] == want
    assert want[f['phase_one_steps'] - 1] != 3.001 - 0.01 * f['phase_one_steps']  # not the closed form


def test_pnvlad_seed_and_fresh_generator_per_cloud():
    clouds, target, found = searched('general_256')
    a = voxel.pnvlad_downsample_host(clouds, target, seed=7)
    b = voxel.pnvlad_downsample_host(clouds[1:], target, seed=7)
    assert all(np.array_equal(x, y) for x, y in zip(a[1:], b))
    m = found[0]['count']
    assert m < target
    np.testing.assert_array_equal(a[0][m:], clouds[0][np.random.default_rng(7).choice(len(clouds[0]), size=target - m)])


# ---------------------------------------------------------------------------------------------- random, padding
def test_random_matches_the_transcription():
    clouds, _ = fc.general_256()
    for target in (64, 1024):
        got = voxel.random_downsample_host(clouds, target)
        for g, cloud in zip(got, clouds):
            assert g.dtype == np.float32 and g.shape == (target, 3)
            np.testing.assert_array_equal(g, ref_random_down_sample(cloud, target))


@pytest.mark.parametrize('downsample', ['pnvlad', 'random'])
def test_padded_normalisation_matches_the_transcription(downsample):
    raw, target = fc.with_outliers()
    down = voxel.pnvlad_downsample_host(raw, target) if downsample == 'pnvlad' else voxel.random_downsample_host(raw, target)
    got = voxel.normalise_submaps_padded_host(down, raw, target)
    plain = voxel.normalise_submaps_host(down)
    iterations = []
    for g, d, r, k in zip(got, down, raw, plain):
        want, its = ref_normalise_pcl(d, r, target)
        iterations.append(its)
        assert g.dtype == np.float32 and g.shape == (target, 3) and np.abs(g).max() <= 1.0
        np.testing.assert_array_equal(g, want)                                    # generator state across iterations included
        np.testing.assert_array_equal(g[:len(k)], k)
    assert sum(len(k) < target for k in plain) >= 2                               # the normalisation drops rows here ...
    assert max(iterations) >= 2                                                   # ... and the loop did loop


def test_padded_normalisation_without_anything_to_pad():
    clouds, target = fc.lattice_exact_64()
    down = voxel.pnvlad_downsample_host(clouds, target)
    got = voxel.normalise_submaps_padded_host(down, clouds, target)
    np.testing.assert_array_equal(got[0], voxel.normalise_submaps_host(down)[0])


# ---------------------------------------------------------------------------------------------- errors
def test_errors():
    good = fc.scene(5, 300, extent=20.0)
    with pytest.raises(ValueError, match='cloud 1 has 63 points, fewer than target = 64'):
        voxel.pnvlad_downsample_host([good, good[:63]], 64)
    with pytest.raises(ValueError, match='cloud 0 has 1 points'):
        voxel.pnvlad_downsample_host([good[:1]], 64)
    with pytest.raises(ValueError, match='cloud 0 cannot be normalised'):
        voxel.normalise_submaps_padded_host([good[:1]], [good], 64)
    for bad in (0, -3):
        with pytest.raises(ValueError, match='target must be a positive integer'):
            voxel.pnvlad_downsample_host([good], bad)
        with pytest.raises(ValueError, match='target must be a positive integer'):
            voxel.random_downsample_host([good], bad)
        with pytest.raises(ValueError, match='target must be a positive integer'):
            voxel.normalise_submaps_padded_host([good], [good], bad)
    with pytest.raises(ValueError, match='cloud 0 is empty'):
        voxel.random_downsample_host([np.zeros((0, 3), np.float32)], 4)
    # 300 coincident-cell points can never occupy 64 cells: the search runs into the span limit and says so
    tight = np.concatenate([np.zeros((299, 3), np.float32), np.float32([[40.0, 0, 0]])])
    with pytest.raises(ValueError, match='cloud 0 never reaches 64 occupied voxels'):
        voxel.pnvlad_downsample_host([tight], 64)
    with pytest.raises(ValueError, match='cloud 0 keeps .* more than target'):
        voxel.normalise_submaps_padded_host([good], [good], 8)
    assert len(voxel.pnvlad_downsample_host([good[:1]], 1)[0]) == 1               # a single point is its own downsample
