"""Host side of the pose tuples (`hotformerloc_amd.tuples`): `radius_lists_host`, `tuple_index_from_poses(device='cpu')` and
`truth_from_poses` against the lists the reference's own generator functions produced (tests/golden/pose_tuples.npz,
tools/gen_golden_pose_tuples.py), with no tolerance; the exact-boundary group, the float64-only pair, the list invariants,
the batch masks and the metric built on them, and the argument errors.  No GPU."""
import numpy as np
import pytest
import torch

import pose_tuples_cases as pc
from hotformerloc_amd import (TupleIndex, batch_masks_host, radius_counts_host, radius_lists_host, retrieval,
                              truth_from_poses, tuple_index_from_poses)


@pytest.mark.parametrize('name', pc.CASE_NAMES)
def test_host_lists_equal_the_reference(name):
    c = pc.golden()[name]
    off_a, idx_a, off_b, idx_b = radius_lists_host(c.positions, c.positions, c.pos_thresh, c.neg_thresh, exclude_self=True)
    assert off_a.dtype == np.int64 and off_b.dtype == np.int64 and idx_a.dtype == np.int32 and idx_b.dtype == np.int32
    assert np.array_equal(off_a, c.pos_off) and np.array_equal(idx_a, c.pos_idx)
    assert np.array_equal(off_b, c.nn_off) and np.array_equal(idx_b, c.nn_idx)
    # each radius on its own, and the self join spelled with None
    for r, off, idx, drop in ((c.pos_thresh, c.pos_off, c.pos_idx, True), (c.neg_thresh, c.nn_off, c.nn_idx, False)):
        one = radius_lists_host(c.positions, None, r, exclude_self=drop)
        assert len(one) == 2 and np.array_equal(one[0], off) and np.array_equal(one[1], idx)
    assert np.array_equal(radius_counts_host(c.positions, c.positions, c.neg_thresh), np.diff(c.nn_off))
    assert radius_counts_host(c.positions, c.positions, c.neg_thresh).dtype == np.int32


@pytest.mark.parametrize('name', pc.CASE_NAMES)
def test_index_from_poses_equals_the_reference(name):
    c = pc.golden()[name]
    index = tuple_index_from_poses(c.positions, c.pos_thresh, c.neg_thresh, device='cpu')
    assert isinstance(index, TupleIndex) and len(index) == c.n and index.dev is None
    assert np.array_equal(index.pos_off, c.pos_off) and np.array_equal(index.pos_idx, c.pos_idx)
    assert np.array_equal(index.nn_off, c.nn_off) and np.array_equal(index.nn_idx, c.nn_idx)
    for k in range(c.n):                                                    # the invariants of the reference's tuples
        assert k not in index.get_positives(k) and k in index.get_non_negatives(k)
    assert pc.strictly_ascending(index.pos_off, index.pos_idx) and pc.strictly_ascending(index.nn_off, index.nn_idx)
    # a CPU tensor and the swapped column order give the same index
    for other in (torch.from_numpy(c.positions), c.positions[:, ::-1]):
        again = tuple_index_from_poses(other, c.pos_thresh, c.neg_thresh, device='cpu')
        assert np.array_equal(again.pos_idx, c.pos_idx) and np.array_equal(again.nn_idx, c.nn_idx)


def test_exact_boundary_group():
    c = pc.golden()['exact']
    assert c.exact
    ip = np.rint(c.positions - pc.UTM).astype(np.int64)
    d2 = ((ip[:, None, :] - ip[None, :, :]) ** 2).sum(-1)                     # integers: nothing rounds
    assert (d2 == 25).sum() >= 8 and (d2 == 225).sum() >= 8                  # 3-4-5 and 9-12-15 pairs are there ...
    assert ((d2 > 25) & (d2 <= 36)).any() and ((d2 > 225) & (d2 <= 256)).any()        # ... and one lattice step beyond
    assert (d2 == 0).sum() > c.n                                             # duplicated positions
    off_a, idx_a, off_b, idx_b = radius_lists_host(c.positions, None, 5.0, 15.0, exclude_self=True)
    for k in range(c.n):
        a, b = idx_a[off_a[k]:off_a[k + 1]], idx_b[off_b[k]:off_b[k + 1]]
        want_a = np.nonzero(d2[k] <= 25)[0]
        assert np.array_equal(a, want_a[want_a != k])                        # at the radius: in; a step beyond: out
        assert np.array_equal(b, np.nonzero(d2[k] <= 225)[0])
    dup = np.nonzero((d2 == 0).sum(1) > 1)[0]
    zero = radius_lists_host(c.positions, None, 0.0)                         # radius 0: the duplicates of each position
    for k in dup:
        assert np.array_equal(zero[1][zero[0][k]:zero[0][k + 1]], np.nonzero(d2[k] == 0)[0])


def test_float64_only_pair():
    c = pc.golden()['f64pair']
    p = c.positions
    assert p[0, 0] == 500000.25 and p[1, 0] == p[0, 0] + 15.0 - 2.0 ** -16 and p[2, 0] == p[0, 0] + 15.0 + 2.0 ** -16
    as32 = p.astype(np.float32)
    assert as32[1, 0] == as32[2, 0]                                          # float32 cannot tell the two apart
    off, idx = radius_lists_host(p, None, 15.0, exclude_self=True)
    assert idx[off[0]:off[1]].tolist() == [1, 3, 5]                          # 2^-16 inside: in; 2^-16 outside: out
    # float32 input is widened, not rejected: the lists are those of the widened values
    wide = radius_lists_host(as32.astype(np.float64), None, 15.0, exclude_self=True)
    got = radius_lists_host(as32, None, 15.0, exclude_self=True)
    assert np.array_equal(got[0], wide[0]) and np.array_equal(got[1], wide[1])
    assert not np.array_equal(got[1], idx)


@pytest.mark.parametrize('name', pc.CASE_NAMES)
def test_truth_from_poses_equals_the_reference(name):
    c = pc.golden()[name]
    off, idx = truth_from_poses(c.query_positions, c.database_positions, c.eval_thresh)
    assert isinstance(off, torch.Tensor) and off.dtype == torch.int64 and idx.dtype == torch.int64 and not off.is_cuda
    assert np.array_equal(off.numpy(), c.truth_off)
    assert np.array_equal(idx.numpy(), pc.sorted_rows(c.truth_off, c.truth_idx))
    assert pc.strictly_ascending(off.numpy(), idx.numpy())
    want_off, want_idx = retrieval.truth_csr(c.query_sets(), 1, 0)           # the dict form, the tree's order
    assert torch.equal(off, want_off) and off.dtype == want_off.dtype and idx.dtype == want_idx.dtype
    n_db = c.database_positions.shape[0]
    result = pc.search_result(c.query_positions.shape[0], n_db)
    got = retrieval.recall_from_indices(result, off, idx, n_db)
    want = retrieval.recall_from_indices(result, want_off, want_idx, n_db)
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2]
    if name in ('wild', 'oxford'):
        assert 0.0 < want[0][-1] <= 100.0 and want[2] > 0.0                   # the metric is not trivially zero here


@pytest.mark.parametrize('name', ('wild', 'exact'))
def test_batch_masks_on_the_index_from_poses(name):
    c = pc.golden()[name]
    index = tuple_index_from_poses(c.positions, c.pos_thresh, c.neg_thresh, device='cpu')
    rng = np.random.RandomState(3)
    labels = np.concatenate([[0, c.n - 1, 0], rng.randint(0, c.n, 61)]).astype(np.int64)
    pos, neg = batch_masks_host(index, labels)
    want_pos, want_neg = batch_masks_host(c.tuples(), labels)
    assert np.array_equal(pos, want_pos) and np.array_equal(neg, want_neg)
    assert want_pos.any() and want_neg.any()


def test_chunked_host_route(monkeypatch):
    from hotformerloc_amd import tuples
    c = pc.golden()['oxford']
    monkeypatch.setattr(tuples, '_HOST_CHUNK_PAIRS', 7 * c.n)                # 7 rows per chunk: 260 is no multiple of 7
    off_a, idx_a, off_b, idx_b = radius_lists_host(c.positions, None, c.pos_thresh, c.neg_thresh, exclude_self=True)
    assert np.array_equal(off_a, c.pos_off) and np.array_equal(idx_a, c.pos_idx)
    assert np.array_equal(off_b, c.nn_off) and np.array_equal(idx_b, c.nn_idx)
    assert np.array_equal(radius_counts_host(c.positions, None, c.pos_thresh), np.diff(c.pos_off) + 1)


def test_empty_and_full_lists():
    p = pc.positions(37, 4)
    off, idx = radius_lists_host(p, None, 1.0e4)
    assert np.array_equal(off, 37 * np.arange(38)) and np.array_equal(idx, np.tile(np.arange(37), 37))
    far = radius_lists_host(p + 5.0e4, p, 10.0, 20.0)
    assert all(a.shape == (n,) and not a.any() for a, n in zip(far, (38, 0, 38, 0)))


def test_argument_errors():
    p = pc.positions(12, 1)
    for bad in (np.zeros((5, 3)), np.zeros(4), np.zeros((0, 2)), np.zeros((2, 2, 2)), torch.zeros(5, 3), torch.zeros(0, 2)):
        with pytest.raises(ValueError):                                      # D != 2, empty input
            radius_lists_host(bad, p, 1.0)
        with pytest.raises(ValueError):
            radius_lists_host(p, bad, 1.0)
        with pytest.raises(ValueError):
            radius_counts_host(bad, p, 1.0)
    with pytest.raises(ValueError, match='exceeds'):                         # r_a > r_b
        radius_lists_host(p, p, 2.0, 1.0)
    for r in (float('nan'), -1.0):
        with pytest.raises(ValueError):
            radius_lists_host(p, p, r)
        with pytest.raises(ValueError):
            radius_lists_host(p, p, 1.0, r)
        with pytest.raises(ValueError):
            radius_counts_host(p, p, r)
        with pytest.raises(ValueError):
            tuple_index_from_poses(p, r, 5.0, device='cpu')
        with pytest.raises(ValueError):
            truth_from_poses(p, p, r)
    with pytest.raises(ValueError, match='exclude_self'):                    # distinct arrays, even with equal contents
        radius_lists_host(p, p.copy(), 1.0, exclude_self=True)
    with pytest.raises(ValueError):
        tuple_index_from_poses(p, 5.0, 1.0, device='cpu')
    with pytest.raises(ValueError):
        tuple_index_from_poses(np.zeros((4, 3)), 1.0, 5.0, device='cpu')
    with pytest.raises(ValueError):
        truth_from_poses(np.zeros((0, 2)), p, 1.0)
