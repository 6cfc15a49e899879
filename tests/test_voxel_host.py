"""The numpy float64 route of hotformerloc_amd/voxel.py (`voxel_downsample_host`, `normalise_submaps_host`): hand-computed
cases, an independent check against scipy's binned statistics, the normalisation formula transcribed literally, and every
`ValueError` of the contract.  No GPU."""
import inspect

import numpy as np
import pytest
from scipy import stats

from hotformerloc_amd import retrieval, voxel
from tests import voxel_cases as vc


# ---------------------------------------------------------------------------------------------- hand-computed
def test_five_points_in_one_cell():
    clouds, v = vc.five_in_one_cell()
    out, counts, keys = voxel.voxel_downsample_host(clouds, v, return_counts=True, return_keys=True)
    assert len(out) == 1 and out[0].dtype == np.float32 and out[0].shape == (1, 3)
    want = (clouds[0].astype(np.float64).sum(0) / 5.0).astype(np.float32)
    np.testing.assert_array_equal(out[0][0], want)
    assert counts[0].tolist() == [5] and keys[0].tolist() == [0]


def test_two_cells_split_by_a_face():
    # v = 1, min x = 0 -> origin -0.5 -> faces at x = 0.5, 1.5: {0, 0.25, 0.49} | {0.51, 1.0}
    p = np.array([[0.0, 0, 0], [0.51, 0, 0], [0.25, 0, 0], [1.0, 0, 0], [0.49, 0, 0]], np.float32)
    out, counts, keys = voxel.voxel_downsample_host([p], 1.0, return_counts=True, return_keys=True)
    assert counts[0].tolist() == [3, 2] and keys[0].tolist() == [0, 1 << 32]
    want = np.array([[(0.0 + np.float64(np.float32(0.25)) + np.float64(np.float32(0.49))) / 3, 0, 0],
                     [(np.float64(np.float32(0.51)) + 1.0) / 2, 0, 0]]).astype(np.float32)
    np.testing.assert_array_equal(out[0], want)


def test_a_point_on_a_face_goes_to_the_upper_cell():
    # origin = -0.5: x = 0.5 is exactly the face between cells 0 and 1, and (0.5 + 0.5) / 1 = 1 exactly
    p = np.array([[0.0, 0, 0], [0.5, 0, 0], [0.75, 0, 0]], np.float32)
    out, counts, keys = voxel.voxel_downsample_host([p], 1.0, return_counts=True, return_keys=True)
    assert counts[0].tolist() == [1, 2] and keys[0].tolist() == [0, 1 << 32]
    np.testing.assert_array_equal(out[0], np.array([[0, 0, 0], [0.625, 0, 0]], np.float32))
    # the same along z, the least significant axis of the order
    out, counts, keys = voxel.voxel_downsample_host([p[:, ::-1].copy()], 1.0, return_counts=True, return_keys=True)
    assert counts[0].tolist() == [1, 2] and keys[0].tolist() == [0, 1]


def test_output_order_is_ascending_ix_iy_iz():
    clouds, v = vc.ragged()
    out, keys = voxel.voxel_downsample_host(clouds, v, return_keys=True)
    for o, k in zip(out, keys):
        assert np.all(np.diff(k) > 0) and len(o) == len(k)
    k = keys[2]
    cells = np.stack([k >> 32, (k >> 16) & 0xFFFF, k & 0xFFFF], 1)
    assert np.array_equal(np.lexsort((cells[:, 2], cells[:, 1], cells[:, 0])), np.arange(len(k)))


# ---------------------------------------------------------------------------------------------- scipy
@pytest.mark.parametrize('name', ['ragged_1_257_4099', 'quarter_grid_faces', 'utm_offset', 'threshold_segments'])
def test_against_scipy_binned_statistic(name):
    """Counts exact and float64 means to 1e-12 against `binned_statistic_dd(statistic='mean')` on the edges origin + k v,
    extended one cell past the maximum so that no point lands in scipy's closed last bin.  C order of scipy's grid is
    ascending (ix, iy, iz)."""
    clouds, v = vc.DOWNSAMPLE_CASES[name]()
    outs, counts = voxel.voxel_downsample_host(clouds, v, return_counts=True)
    for i, (cloud, out, cnt) in enumerate(zip(clouds, outs, counts)):
        p = cloud.astype(np.float64)
        origin = p.min(0) - 0.5 * v
        n_cells = np.floor((p.max(0) - origin) / v).astype(int) + 2
        edges = [origin[a] + np.arange(n_cells[a] + 1) * v for a in range(3)]
        occ = stats.binned_statistic_dd(p, None, statistic='count', bins=edges).statistic
        np.testing.assert_array_equal(cnt, occ[occ > 0].astype(np.int64))
        mean64, cnt64, _ = voxel._cell_means(cloud, v, i)
        np.testing.assert_array_equal(cnt64, cnt)
        for a in range(3):
            m = stats.binned_statistic_dd(p, p[:, a], statistic='mean', bins=edges).statistic[occ > 0]
            np.testing.assert_allclose(mean64[:, a], m, rtol=1e-12, atol=1e-12)
        np.testing.assert_array_equal(out, mean64.astype(np.float32))


# ---------------------------------------------------------------------------------------------- normalisation
def test_normalise_against_the_formula():
    clouds, v = vc.with_outliers()
    down = voxel.voxel_downsample_host(clouds, v)
    got = voxel.normalise_submaps_host(down)
    assert len(got) == 3
    for q32, g in zip(down, got):
        q = q32.astype(np.float64)
        n = len(q)
        c = np.array([q[:, 0].sum() / n, q[:, 1].sum() / n, q[:, 2].sum() / n])
        total = 0.0
        for i in range(n):
            total += np.sqrt((q[i, 0] - c[0]) ** 2 + (q[i, 1] - c[1]) ** 2 + (q[i, 2] - c[2]) ** 2)
        d = total / n
        s = 0.5 / d
        rows = [s * (q[i] - c) for i in range(n)]
        want = np.array([r for r in rows if np.all(np.abs(r) <= 1)])
        assert 0 < len(want) < n                                 # the case does drop points
        assert g.dtype == np.float32 and g.shape == want.shape
        # the serial sum above and numpy's pairwise sum differ by a few float64 ulps of c and d
        np.testing.assert_allclose(g.astype(np.float64), want, rtol=1e-6, atol=1e-12)


# ---------------------------------------------------------------------------------------------- errors
@pytest.mark.parametrize('v', [0.0, -0.8, float('nan'), float('inf')])
def test_bad_voxel_size(v):
    with pytest.raises(ValueError, match='voxel_size'):
        voxel.voxel_downsample_host([np.zeros((2, 3), np.float32)], v)
    with pytest.raises(ValueError, match='voxel_size'):
        voxel.voxel_downsample([np.zeros((2, 3), np.float32)], v)         # raised before the device is touched
    with pytest.raises(ValueError, match='voxel_size'):
        voxel.prepare_submaps([np.zeros((2, 3), np.float32)], v)


def test_span_overflow_names_the_first_offending_cloud():
    clouds, v = vc.overflow_batch()
    with pytest.raises(ValueError, match=r'cloud 1 spans 65536 or more'):
        voxel.voxel_downsample_host(clouds, v)
    # 65 535 cells fit, 65 536 do not: the maximum sits in cell floor(k + 0.5) = k
    ok = np.array([[0.0, 0, 0], [65534.0, 0, 0]], np.float32)
    assert len(voxel.voxel_downsample_host([ok], 1.0)[0]) == 2
    with pytest.raises(ValueError, match=r'cloud 0 spans'):
        voxel.voxel_downsample_host([ok + np.float32([[0, 0, 0], [1, 0, 0]])], 1.0)


def test_too_many_clouds():
    one = np.zeros((1, 3), np.float32)
    with pytest.raises(ValueError, match='at most 32767 clouds'):
        voxel.voxel_downsample_host([one] * 32768, 1.0)
    with pytest.raises(ValueError, match='at most 32767 clouds'):
        voxel.voxel_downsample([one] * 32768, 1.0)                        # raised before the device is touched
    assert len(voxel.voxel_downsample_host([one] * 3, 1.0)) == 3


def test_normalise_degenerate_and_empty():
    good = vc.box_cloud(5, 100)
    with pytest.raises(ValueError, match='cloud 1 cannot be normalised'):
        voxel.normalise_submaps_host([good, np.ones((1, 3), np.float32), good])
    with pytest.raises(ValueError, match='cloud 0 cannot be normalised'):
        voxel.normalise_submaps_host([np.ones((4, 3), np.float32)])
    # two points: d = half their distance, so both sit at |q'| = 0.5 and stay; nothing can empty a finite cloud, the
    # error exists for non-finite input
    assert len(voxel.normalise_submaps_host([np.array([[0, 0, 0], [2, 0, 0]], np.float32)])[0]) == 2
    with pytest.raises(ValueError, match='cloud 0'):
        voxel.normalise_submaps_host([np.array([[0, 0, 0], [np.inf, 0, 0]], np.float32)])
    with pytest.raises(ValueError, match='cloud 2 is empty'):
        voxel.normalise_submaps_host([good, good, np.zeros((0, 3), np.float32)])


def test_encode_clouds_keywords_default_to_off():
    sig = inspect.signature(retrieval.encode_clouds)
    for name, default in (('voxel_size', None), ('normalise_submaps', False)):
        p = sig.parameters[name]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is default


def test_package_exports():
    import hotformerloc_amd as h
    for name in ('voxel_downsample', 'normalise_submaps', 'prepare_submaps', 'voxel_downsample_host', 'normalise_submaps_host'):
        assert getattr(h, name) is getattr(voxel, name)
