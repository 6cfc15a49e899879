"""Host side of the whole-dataset evaluation (`hotformerloc_amd.retrieval`), no GPU: the CSR ground truth and the metric
computed from search indices against the CPU restatement of the reference's `get_recall` and its pinned values
(tests/golden/retrieval.npz), the pair loop of `evaluate_embeddings` with the search injected, and argument validation."""

import os

import numpy as np
import pytest
import torch

from hotformerloc_amd import retrieval
from oracle import retrieval_ref
from oracle.gen_golden_retrieval import make_sets

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'retrieval.npz')


def exact_search(database, queries, k):
    """f64 exact ranking on the host, as the oracle does it: (Q, k) indices"""
    db = np.asarray(database, dtype=np.float32).astype(np.float64)
    qs = np.asarray(queries, dtype=np.float32).astype(np.float64)
    d2 = ((qs[:, None, :] - db[None, :, :]) ** 2).sum(-1)
    return torch.from_numpy(np.argsort(d2, axis=1, kind='stable')[:, :k])


def host_metric(m, n, vecs, qsets, num_neighbors=25):
    idx = exact_search(vecs[m], vecs[n], min(num_neighbors, len(vecs[m])))
    offsets, indices = retrieval.truth_csr(qsets, n, m)
    return retrieval.recall_from_indices(idx, offsets, indices, len(vecs[m]), num_neighbors)


@pytest.mark.parametrize('name', ['small', 'wide'])
def test_csr_metric_equals_the_oracle_and_the_golden(name):
    g = np.load(GOLDEN)
    seed, n_sets, per_set, dim, places = (int(v) for v in g[name + '.cfg'])
    vecs, qsets = make_sets(seed, n_sets, per_set, dim, places)
    for m in range(n_sets):
        for n in range(n_sets):
            if m == n:
                continue
            recall, opr, mrr = host_metric(m, n, vecs, qsets)
            w_recall, w_opr, w_mrr = retrieval_ref.get_recall(m, n, vecs, vecs, qsets)
            assert recall.shape == (25,)
            np.testing.assert_allclose(recall, w_recall, rtol=0, atol=1e-9)
            assert abs(opr - w_opr) <= 1e-9 and abs(mrr - w_mrr) <= 1e-9
            np.testing.assert_allclose(recall, g['%s.%d.%d.recall' % (name, m, n)], rtol=0, atol=1e-9)
            np.testing.assert_allclose([opr, mrr], g['%s.%d.%d.opr_mrr' % (name, m, n)], rtol=0, atol=1e-9)


def test_truth_csr_layout():
    qsets = [{0: {0: [], 1: [4, 2]}, 1: {0: [1], 1: []}, 2: {0: [], 1: [0, 1, 2]}}]
    offsets, indices = retrieval.truth_csr(qsets, 0, 1)
    assert offsets.dtype == torch.int64 and indices.dtype == torch.int64
    assert offsets.tolist() == [0, 2, 2, 5] and indices.tolist() == [4, 2, 0, 1, 2]
    offsets, indices = retrieval.truth_csr(qsets, 0, 0)
    assert offsets.tolist() == [0, 0, 1, 1] and indices.tolist() == [1]


def test_queries_without_truth_are_skipped():
    """Four queries, two of them without a true neighbour: every figure is a fraction of the two evaluated ones, and a
    result that happens to carry another query's true index does not count."""
    idx = torch.tensor([[3, 1, 0], [5, 4, 3], [0, 1, 2], [2, 0, 1]])
    offsets = torch.tensor([0, 1, 1, 1, 2])
    indices = torch.tensor([1, 5])                       # query 0 -> {1} (found second), query 3 -> {5} (not found)
    recall, opr, mrr = retrieval.recall_from_indices(idx, offsets, indices, 6, num_neighbors=3)
    np.testing.assert_allclose(recall, [0.0, 50.0, 50.0], atol=1e-12)
    assert opr == 0.0                                    # threshold = 1: only the first result counts
    assert abs(mrr - 50.0) <= 1e-12                      # mean over the queries that found one: 1 / 2


def test_one_percent_threshold_is_cut_at_k():
    """n_database = 1000 gives a top-1 % threshold of 10; with k = 3 results it is the first 3 that count (`min(threshold,
    k)`), exactly as slicing a 3-column result by [:10] does in the reference."""
    idx = torch.tensor([[7, 8, 9], [1, 2, 3]])
    offsets = torch.tensor([0, 1, 2])
    indices = torch.tensor([9, 999])
    recall, opr, mrr = retrieval.recall_from_indices(idx, offsets, indices, 1000, num_neighbors=25)
    assert recall.shape == (25,)
    np.testing.assert_allclose(recall[:3], [0.0, 0.0, 50.0], atol=1e-12)
    np.testing.assert_allclose(recall[3:], 50.0, atol=1e-12)
    assert opr == 50.0
    assert abs(mrr - 100.0 / 3.0) <= 1e-12


def oracle_pairs(vecs_db, vecs_q, qsets, pairs):
    recall, oprs, mrrs = np.zeros(25), [], []
    for i, j in pairs:
        r, o, m = retrieval_ref.get_recall(i, j, vecs_db, vecs_q, qsets)
        recall += r
        oprs.append(o)
        mrrs.append(m)
    return recall / len(pairs), np.mean(oprs), np.mean(mrrs)


@pytest.mark.parametrize('case', ['skip_same_run', 'all_pairs', 'only_database', 'none_embedding'])
def test_pair_loop_matches_the_hand_summed_oracle(case):
    vecs, qsets = make_sets(5, 3, 60, 32, 40)
    db, qs = list(vecs), list(vecs)
    kwargs = {}
    if case == 'skip_same_run':
        pairs = [(i, j) for i in range(3) for j in range(3) if i != j]
    elif case == 'all_pairs':
        kwargs['skip_same_run'] = False
        pairs = [(i, j) for i in range(3) for j in range(3)]
    elif case == 'only_database':
        kwargs['only_database'] = 1
        pairs = [(1, 0), (1, 2)]
    else:
        db[2] = None
        qs[0] = None
        pairs = [(0, 1), (0, 2), (1, 2)]
    built = []

    def build_index(embeddings):
        built.append(embeddings)
        return embeddings

    got = retrieval.evaluate_embeddings(db, qs, qsets, build_index=build_index, search=exact_search, **kwargs)
    w_recall, w_opr, w_mrr = oracle_pairs(vecs, vecs, qsets, pairs)
    assert set(got) == {'ave_one_percent_recall', 'ave_recall', 'ave_mrr'}
    np.testing.assert_allclose(got['ave_recall'], w_recall, rtol=0, atol=1e-9)
    assert abs(got['ave_one_percent_recall'] - w_opr) <= 1e-9 and abs(got['ave_mrr'] - w_mrr) <= 1e-9
    assert len(built) == len({i for i, _ in pairs})          # one index per database set, reused for its query sets


def test_argument_validation():
    """Shapes the kernel does not take are refused in Python, before anything is launched or moved to a device."""
    with pytest.raises(ValueError):
        retrieval.FlatL2Index(np.zeros((8, 6), dtype=np.float32))            # D % 4
    with pytest.raises(ValueError):
        retrieval.FlatL2Index(np.zeros((8, 1028), dtype=np.float32))         # D > 1024
    with pytest.raises(ValueError):
        retrieval.FlatL2Index(np.zeros((0, 8), dtype=np.float32))
    with pytest.raises(ValueError):
        retrieval.FlatL2Index(np.zeros(8, dtype=np.float32))
    index = retrieval.FlatL2Index.__new__(retrieval.FlatL2Index)              # an index without its device copy
    index.database = torch.zeros((8, 16))
    index.sq_norms = torch.zeros(8)
    for k in (0, 33, -1):
        with pytest.raises(ValueError):
            index.search(torch.zeros((2, 16)), k=k)
    with pytest.raises(ValueError):
        index.search(torch.zeros((2, 12)), k=5)                               # mismatched D
    with pytest.raises(ValueError):
        index.search(torch.zeros((2, 18)), k=5)                               # D % 4
    from hotformerloc_amd import ops
    cpu = torch.zeros((2, 16))
    with pytest.raises(Exception) as e:
        ops.flat_l2_topk(cpu, cpu, 5)                                         # CPU tensors: no fallback
    assert 'GPU' in str(e.value)
    with pytest.raises(ValueError):
        retrieval.recall_from_indices(torch.zeros((3, 2), dtype=torch.long), torch.tensor([0, 0]), torch.tensor([]), 5)


def test_workspace_query_and_einval_from_the_library():
    """`hfl_flat_l2_topk_workspace` is a host function: O(Q x segments x 32) bytes, far below a (Q, N) matrix, and -1 for
    every shape the kernel refuses; the launcher itself returns HFL_EINVAL for those before it touches the GPU."""
    from hotformerloc_amd import _native
    lib = _native.load()
    q, n, d = 4096, 16384, 256
    ws = lib.hfl_flat_l2_topk_workspace(q, n, d, 32)
    assert 0 < ws <= (q + n) * 4 + 32 + q * 64 * 32 * 8 and ws < q * n * 4 // 4
    assert lib.hfl_flat_l2_topk_workspace(3, 20000, 128, 25) <= (3 + 20000) * 4 + 32 + 3 * 64 * 32 * 8 + 32
    for bad in ((q, n, 6, 25), (q, n, 0, 25), (q, n, 1028, 25), (q, n, d, 0), (q, n, d, 33), (q, 0, d, 25)):
        assert lib.hfl_flat_l2_topk_workspace(*bad) == -1, bad
        assert lib.hfl_flat_l2_topk(None, None, None, None, None, bad[0], bad[1], bad[2], bad[3], None, 0, None) == -1, bad
    assert lib.hfl_row_sq_norms(None, None, 10, 6, None) == -1
