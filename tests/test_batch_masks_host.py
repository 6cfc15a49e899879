"""Host side of the batch masks (`hotformerloc_amd.batch_masks`): `batch_masks_host` against a brute-force set-membership
double loop and against masks produced by the reference's own `in_sorted_array` (`tools/gen_golden_batch_masks.py`), the
validation of `TupleIndex`, and the CSR round trip.  No GPU."""
import os

import numpy as np
import pytest
import torch

import batch_masks_cases as bc
from hotformerloc_amd import TupleIndex, _native, batch_masks, batch_masks_host, training

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'batch_masks.npz')
N = 40


@pytest.mark.parametrize('batch', [1, 4, 7])
def test_host_masks_equal_brute_force(batch):
    q = bc.small_queries(N)
    labels = {1: [2], 4: [0, 1, 2, N - 1], 7: [3, 1, 3, 0, N - 1, 2, 17]}[batch]          # repeats; empty, full, repeated lists
    want_pos, want_neg = bc.brute_force(q, labels)
    for source in (q, TupleIndex(q, device='cpu'), [q[k] for k in range(N)]):
        pos, neg = batch_masks_host(source, labels)
        assert pos.dtype == np.bool_ and neg.dtype == np.bool_ and pos.shape == (batch, batch)
        assert np.array_equal(pos, want_pos) and np.array_equal(neg, want_neg)
    if batch > 1:                                                          # both answers occur in both masks
        assert want_pos.any() and want_neg.any() and not want_pos.all() and not want_neg.all()


def test_host_masks_reproduce_the_reference_fixture():
    z = np.load(GOLDEN)
    index = TupleIndex.from_csr(z['pos_off'], z['pos_idx'], z['nn_off'], z['nn_idx'], device='cpu')
    cases = sorted(k[:-len('.labels')] for k in z.files if k.endswith('.labels'))
    assert len(cases) >= 4
    for c in cases:
        pos, neg = batch_masks_host(index, z[c + '.labels'])
        assert np.array_equal(pos, z[c + '.pos']) and np.array_equal(neg, z[c + '.neg']), c


def _with(q, k, positives=None, non_negatives=None):
    q = dict(q)
    q[k] = bc.Tup(q[k].positives if positives is None else positives,
                  q[k].non_negatives if non_negatives is None else non_negatives)
    return q


def test_tuple_index_rejects_bad_input():
    q = bc.small_queries(N)
    TupleIndex(q, device='cpu')
    with pytest.raises(ValueError, match='positives of element 7 is not sorted'):
        TupleIndex(_with(q, 7, positives=[4, 9, 8]), device='cpu')
    with pytest.raises(ValueError, match='non_negatives of element 11 is not sorted'):
        TupleIndex(_with(q, 11, non_negatives=[4, 3]), device='cpu')
    with pytest.raises(ValueError, match='non_negatives of element 5: id 40 outside'):
        TupleIndex(_with(q, 5, non_negatives=[1, N]), device='cpu')
    with pytest.raises(ValueError, match='positives of element 6: id -1 outside'):
        TupleIndex(_with(q, 6, positives=[-1, 3]), device='cpu')
    missing = {k: v for k, v in q.items() if k != 9}                    # a missing key
    with pytest.raises(ValueError, match='key 9 is missing'):
        TupleIndex(missing, device='cpu')
    shifted = {k + 1: v for k, v in q.items()}                          # non-consecutive with 0..N-1: starts at 1
    with pytest.raises(ValueError, match='key 0 is missing'):
        TupleIndex(shifted, device='cpu')
    gap = {2 * k: v for k, v in q.items()}
    with pytest.raises(ValueError, match='key 1 is missing'):
        TupleIndex(gap, device='cpu')
    # a list that ends high followed by a list that starts low is two sorted lists, not an unsorted one
    TupleIndex(_with(_with(q, 7, positives=[N - 1]), 8, positives=[0]), device='cpu')
    with pytest.raises(ValueError):
        TupleIndex.from_csr([0, 2, 1], [0, 1], [0, 0, 0], [], device='cpu')


def test_from_csr_round_trip_and_sampler_interface():
    q = bc.small_queries(N)
    a = TupleIndex(q, device='cpu')
    b = TupleIndex.from_csr(a.pos_off, a.pos_idx, a.nn_off, a.nn_idx, device='cpu')
    assert len(a) == len(b) == N and list(a.queries) == list(range(N))
    assert a.pos_off.dtype == np.int64 and a.pos_idx.dtype == np.int32
    for k in range(N):
        for idx in (a, b):
            assert np.array_equal(idx.get_positives(k), q[k].positives)
            assert np.array_equal(idx.get_non_negatives(k), q[k].non_negatives)
    # torch tensors are as good as arrays
    c = TupleIndex.from_csr(*(torch.from_numpy(x) for x in (a.pos_off, a.pos_idx, a.nn_off, a.nn_idx)), device='cpu')
    assert np.array_equal(c.get_non_negatives(2), q[2].non_negatives)


def test_labels_are_validated_on_the_host():
    index = TupleIndex(bc.small_queries(N), device='cpu')
    for bad in ([0, N], [-1, 2], [], [[0, 1]], [0.5, 1.0]):
        with pytest.raises(ValueError):
            batch_masks_host(index, bad)


def test_no_cpu_fallback():
    index = TupleIndex(bc.small_queries(N), device='cpu')
    with pytest.raises(_native.NativeLibraryError):
        batch_masks(index, [0, 1])
    with pytest.raises(ValueError):                                       # the length check comes before any device work
        training.make_training_batch([np.zeros((4, 3), np.float32)] * 3, [0, 1], index, 2, None, 7)
    if not torch.cuda.is_available():
        with pytest.raises(_native.NativeLibraryError):
            TupleIndex(bc.small_queries(N))
