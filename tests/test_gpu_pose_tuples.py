"""`hfl_radius_lists` (hotformerloc_amd/csrc/radius.hip) through `tuples.radius_lists` / `radius_counts` against the numpy
route `radius_lists_host`, bit for bit: every golden case, database sizes around a wave and the LDS tile, query counts around
a workgroup's rows, radius 0, all-covering and all-excluding radii, `exclude_self`, repeatability, float32 input, and the
two consumers (`TupleIndex` + `batch_masks`, `truth_from_poses`)."""
import numpy as np
import pytest
import torch

import pose_tuples_cases as pc
from hotformerloc_amd import (TupleIndex, batch_masks, batch_masks_host, ops, radius_counts, radius_counts_host, radius_lists,
                              radius_lists_host, truth_from_poses, tuple_index_from_poses)

pytestmark = pytest.mark.gpu

T, R = ops.RADIUS_TILE, ops.RADIUS_ROWS


def check(queries, database, r_a, r_b, exclude_self=False):
    """device == host for both families; returns the host lists"""
    want = radius_lists_host(queries, database, r_a, r_b, exclude_self=exclude_self)
    got = radius_lists(queries, database, r_a, r_b, exclude_self=exclude_self)
    torch.cuda.synchronize()
    assert len(got) == len(want) == 4
    for f in (0, 2):
        off, idx, w_off, w_idx = got[f], got[f + 1], want[f], want[f + 1]
        assert off.is_cuda and idx.is_cuda and off.dtype == torch.int64 and idx.dtype == torch.int32
        assert off.is_contiguous() and idx.is_contiguous()
        assert np.array_equal(off.cpu().numpy(), w_off)
        if w_idx.size:
            assert np.array_equal(idx.cpu().numpy(), w_idx)
        else:
            assert tuple(idx.shape) == (1,) and idx.data_ptr() != 0 and int(idx[0]) == 0      # one element of storage
        assert pc.strictly_ascending(w_off, w_idx)
    return want


@pytest.mark.parametrize('name', pc.CASE_NAMES)
def test_golden_cases(name):
    c = pc.golden()[name]
    off_a, idx_a, off_b, idx_b = check(c.positions, None, c.pos_thresh, c.neg_thresh, exclude_self=True)
    assert np.array_equal(off_a, c.pos_off) and np.array_equal(idx_a, c.pos_idx)          # and so the reference's lists
    assert np.array_equal(off_b, c.nn_off) and np.array_equal(idx_b, c.nn_idx)
    check(c.query_positions, c.database_positions, c.eval_thresh, c.eval_thresh)
    single = radius_lists(c.positions, None, c.neg_thresh)                               # one radius: one family
    assert len(single) == 2 and np.array_equal(single[1].cpu().numpy(), c.nn_idx)


@pytest.mark.parametrize('n', [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1])
def test_database_sizes_around_the_tile(n):
    db = pc.positions(n, 10 + n)
    q = pc.positions(R + 1, 20 + n)
    q[0] = db[0]                                                   # the first and the last id of the database are hit
    q[1] = db[n - 1]
    want = check(q, db, 30.0, 120.0)
    assert want[1].size > 0 and 0 in want[1] and n - 1 in want[1]
    if n > 64:
        assert want[2][-1] < q.shape[0] * n                        # and not everything is


@pytest.mark.parametrize('n_q', [1, R - 1, R, R + 1, 3 * R + 1])
def test_query_counts_around_the_workgroup(n_q):
    db = pc.positions(T + 70, 31)
    q = pc.positions(n_q, 40 + n_q, duplicates=False)
    q[n_q - 1] = db[T + 69]                                        # the last row finds the last id, past the tile's edge
    want = check(q, db, 25.0, 90.0)
    assert want[1][-1] == T + 69 and (np.diff(want[2]) > 0).all()


@pytest.mark.parametrize('n', [65, T + 1])
def test_self_join_excludes_exactly_the_diagonal(n):
    p = pc.positions(n, 50 + n, extent=300.0)
    with_self = check(p, None, 12.0, 40.0)
    without = check(p, None, 12.0, 40.0, exclude_self=True)
    assert np.array_equal(without[2], with_self[2]) and np.array_equal(without[3], with_self[3])      # list B keeps it
    assert np.array_equal(np.diff(without[0]), np.diff(with_self[0]) - 1)
    rows = np.repeat(np.arange(n), np.diff(with_self[0]))
    assert np.array_equal(with_self[1][with_self[1] != rows], without[1])
    same_object = radius_lists(p, p, 12.0, exclude_self=True)                            # `database is queries` as well
    assert np.array_equal(same_object[1].cpu().numpy(), without[1])


def test_radius_zero_all_and_none():
    p = pc.positions(T + 5, 61)
    d = (p[:, None, :] == p[None, :, :]).all(-1)
    assert (d.sum(1) > 1).any()                                    # there are duplicated positions
    zero = check(p, None, 0.0, 0.0)
    assert np.array_equal(np.diff(zero[0]), d.sum(1)) and np.array_equal(zero[1], np.nonzero(d)[1])
    n = p.shape[0]
    q = pc.positions(R + 1, 62)
    full = check(q, p, 1.0e4, 1.0e5)                               # every list is 0..N-1
    assert np.array_equal(full[1], np.tile(np.arange(n), R + 1)) and np.array_equal(full[3], full[1])
    check(q + 5.0e4, p, 10.0, 20.0)                                # every list empty, both families
    mixed = check(q + 600.0, p, 10.0, 1.0e4)                       # A empty, B full
    assert mixed[1].size == 0 and mixed[3].size == (R + 1) * n


def test_counts_are_the_row_lengths():
    p = pc.positions(T + 300, 71)
    q = pc.positions(3 * R + 1, 72)
    for queries, database, r in ((q, p, 45.0), (p, None, 20.0), (q, p, 0.0)):
        off, _ = radius_lists(queries, database, r)
        cnt = radius_counts(queries, database, r)
        assert cnt.is_cuda and cnt.dtype == torch.int32 and tuple(cnt.shape) == (queries.shape[0],)
        assert torch.equal(cnt.long(), off[1:] - off[:-1])
        assert np.array_equal(cnt.cpu().numpy(), radius_counts_host(queries, database, r))


def test_two_calls_give_the_same_bits():
    p = pc.positions(2 * T + 1, 81)
    a = radius_lists(p, None, 15.0, 60.0, exclude_self=True)
    b = radius_lists(p, None, 15.0, 60.0, exclude_self=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and a[1].numel() > 0


def test_index_from_poses_feeds_batch_masks():
    c = pc.golden()['wild']
    index = tuple_index_from_poses(c.positions, c.pos_thresh, c.neg_thresh, device='cuda')
    assert isinstance(index, TupleIndex) and index.dev is not None and len(index) == c.n
    assert np.array_equal(index.pos_idx, c.pos_idx) and np.array_equal(index.nn_idx, c.nn_idx)
    rng = np.random.RandomState(3)
    labels = np.concatenate([[0, c.n - 1, 0], rng.randint(0, c.n, 61)]).astype(np.int64)
    pos, neg = batch_masks(index, labels)
    want_pos, want_neg = batch_masks_host(c.tuples(), labels)
    assert np.array_equal(pos.cpu().numpy(), want_pos) and np.array_equal(neg.cpu().numpy(), want_neg)
    assert want_pos.any() and want_neg.any()


@pytest.mark.parametrize('name', ('wild', 'exact'))
def test_truth_from_poses_on_device_tensors(name):
    c = pc.golden()[name]
    want_off, want_idx = truth_from_poses(c.query_positions, c.database_positions, c.eval_thresh)
    off, idx = truth_from_poses(torch.from_numpy(c.query_positions).cuda(), torch.from_numpy(c.database_positions).cuda(),
                                c.eval_thresh)
    assert off.is_cuda and idx.is_cuda and off.dtype == torch.int64 and idx.dtype == torch.int64
    assert torch.equal(off.cpu(), want_off) and torch.equal(idx.cpu(), want_idx)
    mixed = truth_from_poses(c.query_positions, torch.from_numpy(c.database_positions).cuda(), c.eval_thresh)
    assert mixed[0].is_cuda and torch.equal(mixed[1], idx)                  # one tensor on the GPU is enough


def test_float32_positions_are_widened():
    p32 = pc.positions(T + 9, 91).astype(np.float32)
    want = radius_lists_host(p32.astype(np.float64), None, 15.0, 60.0, exclude_self=True)
    for src in (p32, torch.from_numpy(p32), torch.from_numpy(p32).cuda()):
        got = radius_lists(src, None, 15.0, 60.0, exclude_self=True)
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))
    assert want[1].size > 0


def test_argument_errors_come_before_any_launch(monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError('launched')
    monkeypatch.setattr(ops, 'radius_counts', no_launch)
    p = torch.from_numpy(pc.positions(9, 1)).cuda()
    for call in (lambda: radius_lists(p, p, 2.0, 1.0), lambda: radius_lists(p, p, float('nan')),
                 lambda: radius_lists(p, p.clone(), 1.0, exclude_self=True), lambda: radius_lists(p[:, :1], p, 1.0),
                 lambda: radius_lists(p, p[:0], 1.0), lambda: radius_counts(p, p, -1.0)):
        with pytest.raises(ValueError):
            call()
