"""Prefix-limited streamed search (`hfl_flat_l2_topk_prefix`, `FlatL2Index.search(limits=)`) and the intra-sequence
evaluation on the GPU.

The kernel's yardstick is the unrestricted search itself: a (query, row) pair's distance does not depend on the tile, the
segment or the limit, so row q of the prefix search must carry the bits `ops.flat_l2_topk` returns for that query against
`database[:limits[q]]`.  The refined search and the protocol are compared with numpy float64 (tests/intra_sequence_cases.py,
`evaluate_intra_sequence_host`) on inputs that pass the gap guard of `FlatL2Index.search`."""
import math

import numpy as np
import pytest
import torch

from hotformerloc_amd import load_config, model_factory, ops, retrieval
from hotformerloc_amd import synthetic as syn
from hotformerloc_amd._native import NativeLibraryError

import intra_sequence_cases as ic

pytestmark = pytest.mark.gpu

DEV = 'cuda'
INF = float('inf')


def on_device(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV) if dtype is None else \
        torch.as_tensor(np.ascontiguousarray(x), device=DEV, dtype=dtype)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                                                     b.contiguous().view(torch.int32))


def expected_by_prefix(q, db, limits, k):
    """(Q, k) from one unrestricted search per query against its own prefix"""
    want_d = torch.full((q.shape[0], k), INF, dtype=torch.float32, device=DEV)
    want_i = torch.full((q.shape[0], k), -1, dtype=torch.int32, device=DEV)
    for row, lim in enumerate(int(v) for v in limits):
        if lim > 0:
            d, i = ops.flat_l2_topk(q[row:row + 1], db[:lim], k)
            assert tuple(d.shape) == (1, min(k, lim))
            want_d[row, :d.shape[1]], want_i[row, :d.shape[1]] = d[0], i[0]
    return want_d, want_i


def check_prefix(q, db, limits, k):
    q, db = on_device(q), on_device(db)
    got_d, got_i = ops.flat_l2_topk_prefix(q, db, on_device(limits), k)
    assert got_d.dtype == torch.float32 and got_i.dtype == torch.int32 and got_d.is_cuda and got_i.is_cuda
    assert tuple(got_d.shape) == (q.shape[0], k) and tuple(got_i.shape) == (q.shape[0], k)
    want_d, want_i = expected_by_prefix(q, db, limits, k)
    assert torch.equal(got_i, want_i)
    assert same_bits(got_d, want_d)
    filled = torch.as_tensor(np.minimum(np.asarray(limits), k), device=DEV)[:, None]
    unused = torch.arange(k, device=DEV)[None, :] >= filled
    assert bool((got_i[unused] == -1).all()) and bool((got_d[unused] == INF).all())
    assert bool((got_i[~unused] >= 0).all()) and bool((got_i.long() < torch.as_tensor(limits, device=DEV)[:, None]).all())
    again_d, again_i = ops.flat_l2_topk_prefix(q, db, on_device(limits), k)         # no atomics: the same bits twice
    assert torch.equal(again_i, got_i) and same_bits(again_d, got_d)
    return got_d, got_i


SECOND = (70, 647, 64, 32)              # two query tiles, six database tiles with a 7-row tail


def second_shape():
    q_rows, n, d, _ = SECOND
    return ic.descriptors(41, q_rows, d), ic.descriptors(42, n, d), ic.random_limits(43, q_rows, n)


def test_causal_limits_inside_one_query_tile():
    """(200, 200, 8, 25), limits[i] = max(0, i - 5): limits of 0, below k and below the list length, the 128-row tile crossed
    inside a query tile, sixteen different limits in every wavefront."""
    limits = np.maximum(0, np.arange(200) - 5)
    check_prefix(ic.descriptors(31, 200, 8), ic.descriptors(32, 200, 8), limits, 25)


def test_random_limits_over_segments():
    """Non-monotone limits with 0 and N among them: segments wholly beyond a query's limit, the 7-row tail tile."""
    q, db, limits = second_shape()
    assert limits.min() == 0 and limits.max() == SECOND[1] and (np.diff(limits) < 0).any()
    check_prefix(q, db, limits, SECOND[3])


def test_all_limits_zero_and_all_limits_n():
    q, db = ic.descriptors(51, 64, 256), ic.descriptors(52, 647, 256)
    got_d, got_i = check_prefix(q, db, np.zeros(64, dtype=np.int64), 1)
    assert bool((got_i == -1).all()) and bool((got_d == INF).all())
    got_d, got_i = check_prefix(q, db, np.full(64, 647, dtype=np.int64), 1)
    full_d, full_i = ops.flat_l2_topk(on_device(q), on_device(db), 1)
    assert torch.equal(got_i, full_i) and same_bits(got_d, full_d)


@pytest.mark.parametrize('shape', [(33, 300, 72, 25), (5, 129, 4, 32), (70, 100, 36, 32)],
                         ids=lambda s: 'Q%d-N%d-D%d-k%d' % s)
def test_column_chunk_edges_and_one_segment(shape):
    """D = 72 is a 64-column chunk and an 8-column rest, D = 4 a quarter of one 16-column block.  N = 100 is a single
    database tile: one segment, whose kernel writes the result itself, without the merge."""
    q_rows, n, d, k = shape
    check_prefix(ic.descriptors(61 + d, q_rows, d), ic.descriptors(62 + d, n, d), ic.random_limits(63 + d, q_rows, n), k)


def test_ties_on_both_sides_of_a_limit():
    """Rows 150..299 repeat rows 0..149.  With limit 160 the copies 150..159 of rows 0..9 are inside the prefix: equal
    distances, the lower index first.  The copies of rows 10..149 are at or past the limit and never appear.  With limit 150
    no copy appears, with limit 300 every row comes with its copy."""
    base = ic.descriptors(71, 150, 32)
    db = np.concatenate([base, base], 0)
    q = base[:40] + 0.001 * ic.descriptors(72, 40, 32)                      # query r is nearest to rows r and r + 150
    limits = np.array([160] * 20 + [150] * 10 + [300] * 10)
    got_d, got_i = check_prefix(q, db, limits, 25)
    got_d, got_i = got_d.cpu().numpy(), got_i.cpu().numpy().astype(np.int64)
    for row in range(40):
        assert (got_i[row] < limits[row]).all()
        same = got_d[row, 1:] == got_d[row, :-1]
        assert (np.diff(got_i[row])[same] > 0).all()
        members = set(got_i[row].tolist())
        if limits[row] == 160:
            inside = row < 10
            assert got_i[row, :2].tolist() == [row, row + 150] if inside else got_i[row, 0] == row
            assert got_d[row, 0] == got_d[row, 1] if inside else row + 150 not in members
            assert all(j - 150 in members for j in members if j >= 150)     # a copy never without its lower original
        elif limits[row] == 150:
            assert got_i[row, 0] == row and max(members) < 150
        else:
            assert got_i[row, :2].tolist() == [row, row + 150] and got_d[row, 0] == got_d[row, 1]


def test_result_does_not_depend_on_the_launch_shape():
    q, db, limits = second_shape()
    q, db, lim = on_device(q), on_device(db), on_device(limits)
    full_d, full_i = ops.flat_l2_topk_prefix(q, db, lim, 32)
    for a, b in ((0, 64), (64, 70), (13, 14)):
        d, i = ops.flat_l2_topk_prefix(q[a:b], db, lim[a:b], 32)
        assert torch.equal(i, full_i[a:b]) and same_bits(d, full_d[a:b])
    d25, i25 = ops.flat_l2_topk_prefix(q, db, lim, 25, ops.row_sq_norms(db))
    assert torch.equal(i25, full_i[:, :25]) and same_bits(d25, full_d[:, :25])


def test_validation():
    q, db = torch.zeros((6, 16), device=DEV), torch.zeros((40, 16), device=DEV)
    good = torch.arange(6, device=DEV)
    d, i = ops.flat_l2_topk_prefix(q, db, good, 5)
    assert tuple(d.shape) == (6, 5) and tuple(i.shape) == (6, 5)
    for limits in (good.int(), good.cpu(), np.arange(6), np.arange(6, dtype=np.int32), list(range(6))):   # accepted forms
        assert torch.equal(ops.flat_l2_topk_prefix(q, db, limits, 5)[1], i)
    for bad in (good[:5], torch.arange(7, device=DEV), good[:, None], good.float(), np.arange(6, dtype=np.float64),
                torch.tensor([0, 1, 2, -1, 4, 5], device=DEV), torch.tensor([0, 1, 2, 41, 4, 5], device=DEV),
                np.array([0, 1, 2, 3, 4, -1]), np.array([41, 1, 2, 3, 4, 5])):
        with pytest.raises(ValueError):
            ops.flat_l2_topk_prefix(q, db, bad, 5)
    assert int(ops.flat_l2_topk_prefix(q, db, torch.full((6,), 40, device=DEV), 5)[1].max()) == 4         # N itself is fine
    with pytest.raises(ValueError):
        ops.flat_l2_topk_prefix(q, db, good, 33)
    with pytest.raises(ValueError):
        ops.flat_l2_topk_prefix(torch.zeros((6, 12), device=DEV), db, good, 5)
    with pytest.raises(NativeLibraryError):
        ops.flat_l2_topk_prefix(q.cpu(), db.cpu(), good, 5)
    d, i = ops.flat_l2_topk_prefix(q[:0], db, good[:0], 5)
    assert tuple(d.shape) == (0, 5) and tuple(i.shape) == (0, 5)


# ------------------------------------------------------------------------------------------------- FlatL2Index.search
def parent_search(index, q, k, refine):
    """`FlatL2Index.search` as it stood before `limits`: `ops.flat_l2_topk` and the f64 re-ranking of its candidates"""
    n = len(index)
    kk, kp = min(k, n), min(retrieval.MAX_K, n)
    if not refine:
        return ops.flat_l2_topk(q, index.database, kk, index.sq_norms)
    _, cand = ops.flat_l2_topk(q, index.database, kp, index.sq_norms)
    cand = torch.sort(cand.long(), dim=1).values
    d2 = torch.empty((q.shape[0], kp), dtype=torch.float64, device=q.device)
    chunk = max(1, retrieval.REFINE_SCRATCH_BYTES // (kp * index.dim * 20))
    for s in range(0, q.shape[0], chunk):
        diff = index.database[cand[s:s + chunk]].double()
        diff -= q[s:s + chunk].double()[:, None, :]
        diff *= diff
        torch.sum(diff, dim=2, out=d2[s:s + chunk])
    order = torch.argsort(d2, dim=1, stable=True)[:, :kk]
    return d2.gather(1, order), cand.gather(1, order)


@pytest.mark.parametrize('shape', [(70, 647, 64), (17, 7, 32)], ids=lambda s: 'Q%d-N%d-D%d' % s)
def test_search_without_limits_is_unchanged(shape):
    q_rows, n, d = shape
    q, db = on_device(ic.descriptors(81, q_rows, d)), on_device(ic.descriptors(82, n, d))
    index = retrieval.FlatL2Index(db)
    for k in (25, 32):
        for refine in (False, True):
            want_d, want_i = parent_search(index, q, k, refine)
            for got_d, got_i in (index.search(q, k=k, refine=refine), index.search(q, k=k, refine=refine, limits=None)):
                assert tuple(got_d.shape) == (q_rows, min(k, n))
                assert got_d.dtype == want_d.dtype and got_i.dtype == want_i.dtype
                assert torch.equal(got_i, want_i) and torch.equal(got_d, want_d)


@pytest.mark.parametrize('case', ['causal', 'random', 'short'])
def test_refined_search_with_limits_equals_numpy(case):
    if case == 'causal':
        q = db = ic.descriptors(91, 300, 32)
        limits, k = np.maximum(0, np.arange(300) - 20), 25
    elif case == 'random':
        q, db, limits = second_shape()
        k = 32
    else:                                                                     # fewer rows than k: width k all the same
        q, db = ic.descriptors(92, 9, 16), ic.descriptors(93, 7, 16)
        limits, k = np.array([0, 1, 2, 3, 4, 5, 6, 7, 7]), 25
    want_d, want_i, guard = ic.host_prefix_topk(q, db, limits, k)
    assert guard.all(), 'the generator no longer separates the k-th from the 33rd neighbour of a prefix'
    index = retrieval.FlatL2Index(db)
    got_d, got_i = index.search(q, k=k, refine=True, limits=limits)
    assert got_d.dtype == torch.float64 and got_i.dtype == torch.int64 and tuple(got_d.shape) == (q.shape[0], k)
    got_d, got_i = got_d.cpu().numpy(), got_i.cpu().numpy()
    assert np.array_equal(got_i, want_i)
    unused = want_i < 0
    assert unused.sum() == (k - np.minimum(limits, k)).sum()
    assert (got_d[unused] == np.inf).all() and (got_i[unused] == -1).all()
    assert (np.abs(got_d[~unused] - want_d[~unused]) <= 1e-12 * np.abs(want_d[~unused])).all()
    raw_d, raw_i = index.search(q, k=k, refine=False, limits=on_device(limits))
    assert raw_d.dtype == torch.float32 and raw_i.dtype == torch.int32 and tuple(raw_i.shape) == (q.shape[0], k)
    assert np.array_equal(raw_i.cpu().numpy() < 0, unused)


def test_search_with_limits_never_allocates_a_distance_matrix():
    """Q = N = 8192, D = 256, causal limits: the peak of allocated device memory rises by less than 64 MiB across a refined
    search; the dense float64 matrix alone would be 512 MiB."""
    n, d = 8192, 256
    gen = torch.Generator(device=DEV).manual_seed(5)
    db = torch.rand((n, d), device=DEV, generator=gen) - 0.5
    limits = retrieval.causal_limits(torch.arange(n, device=DEV, dtype=torch.float64), 600.0)
    index = retrieval.FlatL2Index(db)
    index.search(db[:8], k=25, limits=limits[:8])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    dist, idx = index.search(db, k=25, limits=limits)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print('peak growth across the search: %.1f MiB' % (growth / 2.0 ** 20))
    assert growth < 64 << 20
    assert tuple(idx.shape) == (n, 25)
    valid = idx >= 0
    assert torch.equal(valid.sum(1), limits.clamp(max=25)) and bool((idx < limits[:, None]).all())
    assert bool((dist[valid] < INF).all()) and bool((dist[~valid] == INF).all())


# ------------------------------------------------------------------------------------------------------- the protocol
INT_KEYS = ('tp', 'fp', 'fn', 'tn')
CURVE_KEYS = ('precision', 'recall_curve', 'f1')


def close(a, b):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-12 * max(1.0, abs(b))


def check_against_host(got, want):
    assert set(got) == set(want)
    assert got['num_evaluated'] == want['num_evaluated'] and got['num_revisits'] == want['num_revisits']
    for key in INT_KEYS:
        assert got[key].dtype == np.int64 and np.array_equal(got[key], want[key]), key
    assert got['recall'].shape == want['recall'].shape
    np.testing.assert_allclose(got['recall'], want['recall'], rtol=1e-12, atol=0, equal_nan=True)
    assert close(got['mrr'], want['mrr']) and close(got['f1_max'], want['f1_max'])
    np.testing.assert_allclose(got['thresholds'], want['thresholds'], rtol=1e-12, atol=0)
    assert close(got['f1_max_threshold'], want['f1_max_threshold'])
    for key in CURVE_KEYS:
        np.testing.assert_allclose(got[key], want[key], rtol=1e-12, atol=0, err_msg=key)


@pytest.mark.parametrize('name', ['loop', 'perturbed', 'line'])
def test_device_protocol_equals_the_host_twin(name):
    emb, pos, ts = ic.run(name)
    limits = retrieval.causal_limits(ts, ic.TIME_THRESH)
    _, _, guard = ic.host_prefix_topk(emb, emb, limits, 25)
    assert guard.all(), 'the run no longer separates the 25th from the 33rd neighbour of a prefix'
    want = ic.host_result(name)
    got = retrieval.evaluate_intra_sequence(emb, pos, ts, time_thresh=ic.TIME_THRESH, world_thresh=ic.WORLD_THRESH)
    check_against_host(got, want)
    if name == 'perturbed':
        assert got['fp'][-1] > 0 and got['fn'][0] > 0 and 0.0 < got['f1_max'] < 1.0
    if name == 'line':
        assert got['num_revisits'] == 0 and np.isnan(got['recall']).all() and math.isnan(got['mrr']) and got['f1_max'] == 0.0

    cuts = np.linspace(0.0, 2.0, 201)
    s = np.unique(want['thresholds'])                                       # the default cuts are the distinct s_i
    assert np.abs(s[:, None] - cuts[None, :]).min() > 1e-9, 'a top-1 distance lies on a cut'
    want = ic.host_result(name, cuts)
    got = retrieval.evaluate_intra_sequence(on_device(emb), on_device(pos), on_device(ts), time_thresh=ic.TIME_THRESH,
                                            world_thresh=ic.WORLD_THRESH, thresholds=cuts)
    assert np.array_equal(got['thresholds'], cuts)
    check_against_host(got, want)


def test_evaluate_intra_dataset_composes_encoding_and_protocol():
    params, depth = load_config('wild-places')
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'stress')
    model = model.cuda()
    kw = dict(coordinates=params.coordinates, normalize=True, octree_depth=depth)
    clouds = syn.make_clouds(9, 12, 900, n_points_max=1100)
    pos = ic.UTM + np.array([[0, 0], [2, 0], [4, 0], [6, 0], [8, 0], [10, 0], [8, 1], [6, 1], [4, 1], [2, 1], [0, 1], [0, 3]], float)
    ts = ic.EPOCH + 10.0 * np.arange(12)
    keys = np.array([5, 0, 11, 3, 8, 1, 10, 2, 7, 4, 9, 6])                  # the scan recorded r-th is stored under keys[r]
    run_set = ic.run_set_from(pos, ts, keys)
    got = retrieval.evaluate_intra_dataset(model, clouds, run_set, 5, time_thresh=30.0, num_neighbors=4, **kw)
    emb = retrieval.encode_clouds(model, [clouds[int(i)] for i in keys], 5, **kw)
    want = retrieval.evaluate_intra_sequence(emb, pos, ts, time_thresh=30.0, num_neighbors=4)
    assert want['num_evaluated'] == 9 and want['num_revisits'] > 0 and want['recall'].shape == (4,)
    assert set(got) == set(want)
    for key in want:
        assert np.array_equal(np.asarray(got[key]), np.asarray(want[key]), equal_nan=True), key
