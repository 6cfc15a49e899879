"""The ragged-batch layer under the raw-submap steps (`hotformerloc_amd/ragged.py`), as far as it runs without a GPU: the
batch intake, the packing of optional results, the two shared checks and the host half of the mask compaction."""
import numpy as np
import pytest
import torch

from hotformerloc_amd import ragged


def cloud(n, seed=0):
    return np.random.default_rng(seed).standard_normal((n, 3)).astype(np.float32)


# ---------------------------------------------------------------------------------------------- intake
def test_intake_of_numpy_torch_and_lists():
    a, b = cloud(5), cloud(3, 1)
    batch = [a, torch.from_numpy(b), b.astype(np.float64).tolist()]
    arrays, tensors = ragged.as_arrays(batch), ragged.as_tensors(batch)
    for got, want in zip(arrays, (a, b, b)):
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.flags['C_CONTIGUOUS']
        assert np.array_equal(got, want)
    for got, want in zip(tensors, (a, b, b)):
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and not got.is_cuda
        assert np.array_equal(got.numpy(), want)
    assert ragged.as_arrays([]) == [] and ragged.as_tensors([]) == []
    flat = ragged.as_arrays([a.reshape(-1)])[0]                              # 3 n values are n rows
    assert flat.shape == (5, 3) and np.array_equal(flat, a)


@pytest.mark.parametrize('intake', [ragged.as_arrays, ragged.as_tensors])
def test_intake_rejects_what_is_no_batch(intake):
    with pytest.raises((ValueError, RuntimeError)):                          # numpy and torch word the reshape differently
        intake([np.zeros((4, 2), np.float32)])                               # 8 values are no rows of 3
    with pytest.raises(ValueError, match='cloud 1 is empty'):
        intake([cloud(2), np.zeros((0, 3), np.float32)])
    one = np.zeros((1, 3), np.float32)
    assert len(intake([one] * ragged.MAX_CLOUDS)) == 32767
    with pytest.raises(ValueError, match='a batch holds at most 32767 clouds'):
        intake([one] * 32768)


def test_packed_splits_points_and_per_point_tensors():
    pts = torch.arange(18, dtype=torch.float32).reshape(6, 3)
    packed = ragged.Packed(pts, np.array([0, 1, 4, 6], np.int64))
    assert packed.batch == 3 and packed.sizes() == [1, 3, 2]
    assert [tuple(c.shape) for c in packed.split()] == [(1, 3), (3, 3), (2, 3)]
    assert torch.equal(torch.cat(packed.split()), pts)
    flags = torch.arange(6)
    assert [c.tolist() for c in packed.split(flags)] == [[0], [1, 2, 3], [4, 5]]
    assert [c.tolist() for c in packed.split(flags, counts=[1, 2, 0])] == [[0], [1, 2], []]


# ---------------------------------------------------------------------------------------------- results
def test_results_with_no_one_and_two_extras():
    first, mask, stats = [1, 2], [True, False], [{}]
    assert ragged.results(first) is first
    assert ragged.results(first, None, None) is first
    assert ragged.results(first, mask) == (first, mask)
    assert ragged.results(first, None, stats) == (first, stats)
    assert ragged.results(first, mask, stats) == (first, mask, stats)
    assert ragged.empty_results() == [] and ragged.empty_results(False, False) == []
    assert ragged.empty_results(True) == ([], []) and ragged.empty_results(False, True) == ([], [])
    assert ragged.empty_results(True, True) == ([], [], [])


# ---------------------------------------------------------------------------------------------- checks
def test_check_positive():
    assert ragged.check_positive('voxel_size', 0.8) == 0.8 and ragged.check_positive('voxel_size', np.float32(2)) == 2.0
    for bad in (0, 0.0, -1.5, float('inf'), float('-inf'), float('nan')):
        for fp32 in (False, True):
            with pytest.raises(ValueError, match=r'std_ratio must be positive and finite, got '):
                ragged.check_positive('std_ratio', bad, fp32=fp32)
    assert ragged.check_positive('time_step', 1e-50) == 1e-50                # positive in float64 ...
    with pytest.raises(ValueError, match=r'time_step must be positive and finite, got 1e-50'):
        ragged.check_positive('time_step', 1e-50, fp32=True)                 # ... and zero in float32
    with np.errstate(over='ignore'), pytest.raises(ValueError, match='cloth_resolution must be positive and finite'):
        ragged.check_positive('cloth_resolution', 1e39, fp32=True)           # infinite in float32
    assert ragged.check_positive('cloth_resolution', 1e39) == 1e39


def test_require_points_names_the_cloud_and_the_step():
    clouds = [torch.zeros(5, 3), torch.zeros(0, 3), torch.zeros(2, 3)]
    ragged.require_points([clouds[0], clouds[2]], 'ground removal')
    ragged.require_points([clouds[0], clouds[2]], 'ground removal', 2)
    with pytest.raises(ValueError, match='cloud 1 has no point left after ground removal'):
        ragged.require_points(clouds, 'ground removal')
    with pytest.raises(ValueError, match='cloud 1 has no point left after the radius trim'):
        ragged.require_points(clouds, 'the radius trim', 4)                  # an empty cloud comes before a short one
    with pytest.raises(ValueError, match='cloud 1 has 2 points left after outlier removal, fewer than target = 4'):
        ragged.require_points([clouds[0], clouds[2]], 'outlier removal', 4)
    packed = ragged.Packed(torch.zeros(7, 3), np.array([0, 5, 7], np.int64))
    ragged.require_points(packed, 'outlier removal', 2)
    with pytest.raises(ValueError, match='cloud 1 has 2 points left after outlier removal, fewer than target = 3'):
        ragged.require_points(packed, 'outlier removal', 3)


# ---------------------------------------------------------------------------------------------- compaction, the host half
def test_compact_offsets():
    off = np.array([0, 3, 7, 9], np.int64)

    def offsets(mask):
        got = ragged.compact_offsets(np.flatnonzero(mask), off)
        assert got.dtype == np.int64
        return got.tolist()

    assert offsets(np.ones(9, bool)) == [0, 3, 7, 9]                         # everything kept: the offsets stay
    middle = np.ones(9, bool)
    middle[3:7] = False
    assert offsets(middle) == [0, 3, 3, 5]                                   # the middle cloud emptied: equal offsets
    last = np.zeros(9, bool)
    last[8] = True
    assert offsets(last) == [0, 0, 0, 1]                                     # only the last row of the last cloud
    assert offsets(np.zeros(9, bool)) == [0, 0, 0, 0]
