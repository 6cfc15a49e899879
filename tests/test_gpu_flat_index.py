"""Streamed flat-L2 search (`hfl_flat_l2_topk`, `retrieval.FlatL2Index`) and the whole-dataset evaluation on the GPU.

Error bound of the kernel's distance (derived, not measured): an fmaf chain of D terms, two norm chains of D terms and two
additions, against the f64 distance of the same fp32 inputs:  b(q, d) = 2^-23 (D + 4) (|q|^2 + |d|^2).  Order statistics of
two arrays that differ element-wise by <= b differ by <= b, so the true distance of the j-th returned row is within 2 b of the
j-th smallest true distance, and re-ranking the fp32 top-32 in f64 gives the exact f64 top-25 whenever the 25th and the 33rd
smallest true distance differ by more than 2 b."""

import os

import numpy as np
import pytest
import torch

from hotformerloc_amd import load_config, model_factory, ops, retrieval
from hotformerloc_amd import synthetic as syn
from oracle.gen_golden_retrieval import make_sets

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'retrieval.npz')
DEV = 'cuda'


def descriptors(seed, rows, dim, scale=1.0):
    return ((syn.hash_uniform(seed, rows * dim).reshape(rows, dim) - 0.5) * scale).astype(np.float32)


def true_distances(q, db):
    """(Q, N) f64 squared distances of fp32 inputs, on the GPU in row chunks, and the bound b of the module docstring"""
    qd = torch.as_tensor(q, device=DEV).double()
    dd = torch.as_tensor(db, device=DEV).double()
    out = torch.empty((qd.shape[0], dd.shape[0]), dtype=torch.float64, device=DEV)
    step = max(1, (1 << 25) // max(1, dd.shape[0] * dd.shape[1]))
    for s in range(0, qd.shape[0], step):
        out[s:s + step] = ((qd[s:s + step, None, :] - dd[None, :, :]) ** 2).sum(-1)
    bound = 2.0 ** -23 * (qd.shape[1] + 4) * ((qd * qd).sum(1)[:, None] + (dd * dd).sum(1)[None, :])
    return out, bound


def check_contract(q, db, k):
    index = retrieval.FlatL2Index(db)
    dist, idx = index.search(q, k=k, refine=False)
    n = db.shape[0]
    kc = min(k, n)
    assert dist.dtype == torch.float32 and idx.dtype == torch.int32 and dist.is_cuda and idx.is_cuda
    assert tuple(dist.shape) == (q.shape[0], kc) and tuple(idx.shape) == (q.shape[0], kc)
    true, bound = true_distances(q, db)
    li = idx.long()
    assert int(li.min()) >= 0 and int(li.max()) < n
    assert bool((torch.sort(li, dim=1).values.diff(dim=1) > 0).all()), 'indices repeat'
    t_at, b_at = true.gather(1, li), bound.gather(1, li)
    err = (dist.double() - t_at).abs()
    print('k=%d Q=%d N=%d D=%d: worst |d - D| / b = %.3f' % (k, q.shape[0], n, q.shape[1],
                                                            float((err / b_at.clamp_min(1e-300)).max())))
    assert bool((err <= b_at).all()), 'distance off by more than b'
    rank_err = (t_at - torch.sort(true, dim=1).values[:, :kc]).abs()
    # b of the order-statistics argument: the largest b(q, d) over the query's row of the matrix
    assert bool((rank_err <= 2 * bound.max(1, keepdim=True).values).all()), 'not the j-th nearest within 2 b'
    assert bool((dist.diff(dim=1) >= 0).all()), 'distances decrease'
    assert bool(((dist.diff(dim=1) > 0) | (li.diff(dim=1) > 0)).all()), 'equal distances out of index order'


CONTRACT_SHAPES = [   # (Q, N, D, k): tile and list edges, a sample of the product
    (1, 1, 4, 1), (1, 7, 32, 25), (15, 31, 36, 32), (16, 32, 256, 25), (17, 33, 1024, 32), (65, 63, 4, 25), (16, 64, 36, 1),
    (65, 65, 32, 32), (17, 257, 256, 25), (1, 257, 1024, 1), (15, 257, 36, 32), (65, 257, 32, 25), (16, 33, 4, 32),
    (17, 64, 1024, 25), (65, 31, 256, 1)]


@pytest.mark.parametrize('shape', CONTRACT_SHAPES, ids=lambda s: 'Q%d-N%d-D%d-k%d' % s)
def test_kernel_contract(shape):
    q_rows, n, d, k = shape
    check_contract(descriptors(11 + q_rows, q_rows, d), descriptors(29 + n, n, d), k)


def test_kernel_contract_scaled_and_zero_row():
    """|q|^2 + |d|^2 2500 times larger, and an all-zero database row and query: the bound scales with the norms."""
    check_contract(descriptors(3, 65, 256, 50.0), descriptors(4, 257, 256, 50.0), 25)
    q, db = descriptors(5, 17, 36), descriptors(6, 257, 36)
    db[130] = 0.0
    q[3] = 0.0
    check_contract(q, db, 32)
    _, idx = retrieval.FlatL2Index(db).search(q, k=1, refine=False)
    assert int(idx[3, 0]) == 130                      # the zero query's nearest row is the zero row, at distance exactly 0


def test_fewer_rows_than_k():
    q, db = descriptors(7, 17, 32), descriptors(8, 7, 32)
    index = retrieval.FlatL2Index(db)
    for refine in (False, True):
        dist, idx = index.search(q, k=25, refine=refine)
        assert tuple(dist.shape) == (17, 7) and tuple(idx.shape) == (17, 7)
        assert torch.sort(idx.long(), dim=1).values.tolist() == [list(range(7))] * 17
    d32, i32 = ops.flat_l2_topk(torch.as_tensor(q, device=DEV), torch.as_tensor(db, device=DEV), 32)
    assert tuple(d32.shape) == (17, 7) and tuple(i32.shape) == (17, 7)


TRIPLE_ROWS = (9, 101, 257, 300, 511, 699)          # rows whose three copies the 40-fold row does not overwrite


def test_ties_come_in_index_order():
    """Every row three times, a database tile (128 rows) and more apart, and one row 40 times all over the database: identical
    rows give bitwise identical distances, so the order among them is the index order, through every tile, segment and merge."""
    base = descriptors(12, 700, 32)
    db = np.concatenate([base, base, base], 0)                          # copies of row r at r, r + 700, r + 1400
    special = descriptors(13, 1, 32)[0]
    where = np.sort((np.arange(40) * 53 + 5) % 2100)
    assert len(set(where.tolist())) == 40
    db[where] = special
    q = descriptors(14, 20, 32)
    q[:6] = special + 0.01 * descriptors(15, 6, 32)                     # nearest row of the first six queries
    assert not {r + o for r in TRIPLE_ROWS for o in (0, 700, 1400)} & set(where.tolist())
    q[6:12] = base[list(TRIPLE_ROWS)] + 0.01 * descriptors(16, 6, 32)
    index = retrieval.FlatL2Index(db)
    for k in (25, 32):
        for queries in (q, q[:3]):                                        # two launch shapes
            dist, idx = index.search(queries, k=k, refine=False)
            dist, idx = dist.cpu().numpy(), idx.cpu().numpy().astype(np.int64)
            for row in range(idx.shape[0]):
                same = dist[row, 1:] == dist[row, :-1]
                assert (np.diff(idx[row])[same] > 0).all()
                groups = {}
                for j in idx[row]:
                    groups.setdefault(db[j].tobytes(), []).append(j)
                for key, members in groups.items():                       # a returned duplicate: the lowest copies, ascending
                    copies = np.nonzero((db == np.frombuffer(key, dtype=np.float32)).all(1))[0]
                    assert members == copies[:len(members)].tolist()
            for row in range(min(6, idx.shape[0])):
                assert idx[row].tolist() == where[:k].tolist()
    _, idx = index.search(q[6:12], k=3, refine=False)
    assert idx.cpu().tolist() == [[r, r + 700, r + 1400] for r in TRIPLE_ROWS]


def test_result_does_not_depend_on_the_launch_shape():
    """Q = 600 against N = 20 000 and a 3-row slice of the same queries: the slice runs more database segments (fewer query
    tiles to fill the chip).  Same bits, and the same bits again on a second run."""
    db, q = descriptors(21, 20000, 64), descriptors(22, 600, 64)
    index = retrieval.FlatL2Index(db)
    full_d, full_i = index.search(q, k=32, refine=False)
    for a, b in ((298, 301), (0, 3), (597, 600)):
        d, i = index.search(q[a:b], k=32, refine=False)
        assert torch.equal(d, full_d[a:b]) and torch.equal(i, full_i[a:b])
    again_d, again_i = index.search(q, k=32, refine=False)
    assert torch.equal(again_d, full_d) and torch.equal(again_i, full_i)
    d25, i25 = index.search(q, k=25, refine=False)
    assert torch.equal(d25, full_d[:, :25]) and torch.equal(i25, full_i[:, :25])


def test_input_forms_agree():
    db, q = descriptors(31, 300, 36), descriptors(32, 40, 36)
    want_d, want_i = retrieval.FlatL2Index(torch.as_tensor(db, device=DEV)).search(torch.as_tensor(q, device=DEV), k=25,
                                                                                  refine=False)
    wide_db = torch.zeros((300, 72), device=DEV)
    wide_db[:, ::2] = torch.as_tensor(db, device=DEV)
    wide_q = np.zeros((80, 36), dtype=np.float32)
    wide_q[::2] = q
    forms = [(db, q), (db.astype(np.float64), q.astype(np.float64)), (torch.from_numpy(db), torch.from_numpy(q)),
             (wide_db[:, ::2], wide_q[::2]), (torch.from_numpy(db).double(), torch.as_tensor(q, device=DEV).double())]
    for database, queries in forms:
        d, i = retrieval.FlatL2Index(database).search(queries, k=25, refine=False)
        assert torch.equal(d, want_d) and torch.equal(i, want_i)
    want_rd, want_ri = retrieval.FlatL2Index(db).search(q, k=25)
    assert want_rd.dtype == torch.float64 and want_ri.dtype == torch.int64 and want_rd.is_cuda and want_ri.is_cuda


def test_validation_on_the_device():
    db = torch.zeros((8, 16), device=DEV)
    index = retrieval.FlatL2Index(db)
    with pytest.raises(ValueError):
        index.search(torch.zeros((2, 12), device=DEV))
    with pytest.raises(ValueError):
        index.search(torch.zeros((2, 16), device=DEV), k=33)
    with pytest.raises(ValueError):
        ops.flat_l2_topk(torch.zeros((2, 6), device=DEV), torch.zeros((8, 6), device=DEV), 5)
    with pytest.raises(ValueError):
        ops.flat_l2_topk(torch.zeros((2, 16), device=DEV), db, 0)
    dist, idx = index.search(torch.zeros((0, 16), device=DEV), k=5)
    assert tuple(dist.shape) == (0, 5) and tuple(idx.shape) == (0, 5)


# ------------------------------------------------------------------------------------ refined search and the metric
SETS = {}


def sets(cfg):
    if cfg not in SETS:
        SETS[cfg] = make_sets(*cfg)
    return SETS[cfg]


@pytest.mark.parametrize('cfg', [(5, 3, 60, 32, 40), (6, 2, 400, 256, 150), (9, 2, 333, 64, 100), (10, 2, 2051, 128, 700),
                                 (7, 3, 1500, 256, 500)], ids=lambda c: 'sets%d' % c[0])
def test_refined_search_equals_flat_l2_topk(cfg):
    vecs, _ = sets(cfg)
    indexes = [retrieval.FlatL2Index(v) for v in vecs]
    for m in range(len(vecs)):
        for n in range(len(vecs)):
            if m == n:
                continue
            true, bound = true_distances(vecs[n], vecs[m])
            ordered = torch.sort(true, dim=1).values
            gap = float((ordered[:, 32] - ordered[:, 24] - 2 * bound.max(1).values).min())
            print('sets %s pair (%d, %d): smallest D(33) - D(25) - 2 b = %.3e' % (cfg, m, n, gap))
            assert gap > 0, 'the generator no longer separates the 25th from the 33rd neighbour by 2 b'
            db, qs = torch.as_tensor(vecs[m], device=DEV), torch.as_tensor(vecs[n], device=DEV)
            want_d, want_i = retrieval.flat_l2_topk(db, qs, 25)
            got_d, got_i = indexes[m].search(vecs[n], k=25)
            assert torch.equal(got_i, want_i)
            assert bool(((got_d - want_d).abs() <= 1e-12 * want_d.abs()).all())


@pytest.mark.parametrize('name', ['small', 'wide'])
def test_metric_reproduces_the_golden(name):
    g = np.load(GOLDEN)
    cfg = tuple(int(v) for v in g[name + '.cfg'])
    vecs, qsets = sets(cfg)
    for m in range(cfg[1]):
        index = retrieval.FlatL2Index(vecs[m])
        for n in range(cfg[1]):
            if m == n:
                continue
            _, idx = index.search(vecs[n], k=25)
            recall, opr, mrr = retrieval.recall_from_indices(idx, *retrieval.truth_csr(qsets, n, m), len(vecs[m]))
            np.testing.assert_allclose(recall, g['%s.%d.%d.recall' % (name, m, n)], rtol=0, atol=1e-9)
            np.testing.assert_allclose([opr, mrr], g['%s.%d.%d.opr_mrr' % (name, m, n)], rtol=0, atol=1e-9)


def test_evaluate_embeddings_equals_the_sum_of_get_recall():
    vecs, qsets = sets((7, 3, 1500, 256, 500))
    got = retrieval.evaluate_embeddings(vecs, vecs, qsets)
    recall, oprs, mrrs = np.zeros(25), [], []
    for i in range(3):
        for j in range(3):
            if i != j:
                r, o, m = retrieval.get_recall(i, j, vecs, vecs, qsets)
                recall += r
                oprs.append(o)
                mrrs.append(m)
    np.testing.assert_allclose(got['ave_recall'], recall / 6, rtol=0, atol=1e-9)
    assert abs(got['ave_one_percent_recall'] - np.mean(oprs)) <= 1e-9 and abs(got['ave_mrr'] - np.mean(mrrs)) <= 1e-9


def test_search_never_allocates_a_distance_matrix():
    """Q = 4096, N = 16384, D = 256: the peak of allocated device memory grows by less than the Q x N x 4 bytes (256 MiB) of
    the fp32 distance matrix across a refined search (workspace, results and the 32 MiB-capped refine scratch)."""
    q_rows, n, d = 4096, 16384, 256
    gen = torch.Generator(device=DEV).manual_seed(5)
    db = torch.rand((n, d), device=DEV, generator=gen) - 0.5
    q = torch.rand((q_rows, d), device=DEV, generator=gen) - 0.5
    index = retrieval.FlatL2Index(db)
    index.search(q[:8], k=25)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    dist, idx = index.search(q, k=25)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print('peak growth across search: %.1f MiB' % (growth / 2.0 ** 20))
    assert growth < q_rows * n * 4
    assert tuple(idx.shape) == (q_rows, 25) and int(idx.min()) >= 0 and int(idx.max()) < n
    assert bool((dist.diff(dim=1) >= 0).all())


# ------------------------------------------------------------------------------------ encoding and the whole loop
@pytest.fixture(scope='module')
def encoder():
    params, depth = load_config('wild-places')
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'stress')
    return model.cuda(), params, depth


def test_encode_clouds_equals_one_forward_per_batch(encoder):
    from hotformerloc_amd import build_batch_octree
    from hotformerloc_amd.preprocess import prepare_clouds
    model, params, depth = encoder
    clouds = syn.make_clouds(9, 11, 900, n_points_max=1100)
    model.train()
    got = retrieval.encode_clouds(model, iter(clouds), 4, coordinates=params.coordinates, normalize=True, octree_depth=depth)
    assert not model.training
    assert tuple(got.shape) == (11, 256) and got.dtype == torch.float32 and got.is_cuda
    want = []
    with torch.inference_mode():
        for s in range(0, 11, 4):
            pts = prepare_clouds(clouds[s:s + 4], coordinates=params.coordinates, normalize=True)
            want.append(model({'octree': build_batch_octree(pts, depth, 2, DEV)})['global'])
    assert torch.equal(got, torch.cat(want, 0))


def test_evaluate_dataset_composes_encoding_and_metric(encoder):
    model, params, depth = encoder
    kw = dict(coordinates=params.coordinates, normalize=True, octree_depth=depth)
    cloud_sets = [syn.make_clouds(9, 11, 900, n_points_max=1100), syn.make_clouds(9, 9, 900, n_points_max=1100, first_index=20)]
    sizes = [11, 9]
    qsets = [{i: {m: ([] if i % 4 == 3 else [(i + s) % sizes[m] for s in range(2)]) for m in range(2)} for i in range(sizes[n])}
             for n in range(2)]
    got = retrieval.evaluate_dataset(model, cloud_sets, cloud_sets, qsets, 4, **kw)
    emb = [retrieval.encode_clouds(model, c, 4, **kw) for c in cloud_sets]
    want = retrieval.evaluate_embeddings(emb, emb, qsets)
    np.testing.assert_array_equal(got['ave_recall'], want['ave_recall'])
    assert got['ave_one_percent_recall'] == want['ave_one_percent_recall'] and got['ave_mrr'] == want['ave_mrr']
    assert got['ave_recall'].shape == (25,) and np.isfinite(got['ave_recall']).all()
