"""The `(B, B)` positives / negatives masks of a training batch, made on the GPU.

The reference's collate function (`datasets/dataset_utils.py:118-123`) builds them with two nested Python list
comprehensions over `in_sorted_array` (one `np.searchsorted` per pair, `:201-206`) from each element's sorted `positives` and
`non_negatives` arrays (`TrainingTuple`, `datasets/base_datasets.py:11-28`), copies them to the device, and the loss turns
them into `uint8` again.  Here the lists are uploaded once per dataset as CSR (`TupleIndex`) and a batch's two masks are ONE
launch (`hfl_batch_masks`, csrc/batch_masks.hip) over labels that may already be on the device:

    positives_mask[i, j] = labels[j] in positives[labels[i]]
    negatives_mask[i, j] = labels[j] not in non_negatives[labels[i]]

with no special case for the diagonal or for repeated labels, as in the reference.  `batch_masks_host` restates the same in
numpy on the CPU: the route without a GPU and the yardstick of the tests.
"""

import numpy as np
import torch

from . import _native


def _ids(a, what: str, elem: int) -> np.ndarray:
    a = np.asarray(a)
    if a.size == 0:
        return np.zeros(0, np.int64)
    if a.ndim != 1:
        raise ValueError('%s of element %d: a 1-D array of ids expected, got shape %s' % (what, elem, a.shape))
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError('%s of element %d: integer ids expected, got %s' % (what, elem, a.dtype))
    return a.astype(np.int64, copy=False)


def _check_csr(off: np.ndarray, idx: np.ndarray, n: int, what: str):
    """Every list non-decreasing with ids in [0, n): ValueError naming the first offending element otherwise."""
    if off.shape != (n + 1,) or off[0] != 0 or off[-1] != idx.shape[0] or np.any(np.diff(off) < 0):
        raise ValueError('%s: offsets must be %d non-decreasing values from 0 to %d' % (what, n + 1, idx.shape[0]))
    if np.any(np.diff(off) >= 2 ** 31):
        raise ValueError('%s of element %d: 2**31 or more entries' % (what, int(np.argmax(np.diff(off) >= 2 ** 31))))
    if idx.size == 0:
        return
    bad = (idx < 0) | (idx >= n)
    if bad.any():
        k = int(np.argmax(bad))
        owner = int(np.searchsorted(off, k, side='right') - 1)
        raise ValueError('%s of element %d: id %d outside [0, %d)' % (what, owner, int(idx[k]), n))
    drop = np.diff(idx) < 0                                       # entry k + 1 below entry k ...
    starts = np.zeros(idx.shape[0], bool)
    starts[off[:-1][off[:-1] < idx.shape[0]]] = True              # ... unless k + 1 opens another list
    drop &= ~starts[1:]
    if drop.any():
        k = int(np.argmax(drop))
        owner = int(np.searchsorted(off, k, side='right') - 1)
        raise ValueError('%s of element %d is not sorted (%d before %d)' % (what, owner, int(idx[k]), int(idx[k + 1])))


class TupleIndex:
    """The `positives` and `non_negatives` lists of a whole training set, validated on the host and held as CSR (int64
    offsets, int32 ids) on `device` next to the host copies.  Built once per dataset.

    `queries`: the reference's `TrainingDataset.queries` -- a dict keyed 0..N-1, or a sequence -- whose values carry the
    sorted integer arrays `.positives` and `.non_negatives`.  Keys must be exactly 0..N-1, every list non-decreasing
    (repeats are allowed: `np.union1d` / `np.sort` outputs), every id in [0, N), N < 2**31; anything else raises ValueError
    naming the first offending element.  `__len__`, `get_positives` and `get_non_negatives` are what the reference's
    `BatchSampler` asks of a dataset.  `device='cpu'` builds a host-only index (for `batch_masks_host`)."""

    def __init__(self, queries, device='cuda'):
        if isinstance(queries, dict):
            n = len(queries)
            for k in range(n):
                if k not in queries:
                    raise ValueError('queries must be keyed 0..%d: key %d is missing (keys %r...)'
                                     % (n - 1, k, sorted(queries, key=repr)[:4]))
            items = [queries[k] for k in range(n)]
        else:
            items = list(queries)
        n = len(items)
        pos = [_ids(e.positives, 'positives', k) for k, e in enumerate(items)]
        nn = [_ids(e.non_negatives, 'non_negatives', k) for k, e in enumerate(items)]
        self._init(*self._csr(pos), *self._csr(nn), device)

    @staticmethod
    def _csr(lists):
        off = np.zeros(len(lists) + 1, np.int64)
        if lists:
            np.cumsum([len(a) for a in lists], out=off[1:])
        idx = np.concatenate(lists) if lists else np.zeros(0, np.int64)
        return off, idx.astype(np.int64, copy=False)

    @classmethod
    def from_csr(cls, pos_off, pos_idx, nn_off, nn_idx, device='cuda'):
        """From ready arrays: (N + 1,) offsets and the concatenated ids of both list families (validated like `queries`)."""
        self = cls.__new__(cls)
        arrs = []
        for name, a in (('pos_off', pos_off), ('pos_idx', pos_idx), ('nn_off', nn_off), ('nn_idx', nn_idx)):
            a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
            if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
                raise ValueError('%s: a 1-D integer array expected' % name)
            arrs.append(a.astype(np.int64))
        self._init(*arrs, device)
        return self

    def _init(self, pos_off, pos_idx, nn_off, nn_idx, device):
        n = pos_off.shape[0] - 1
        if n < 1:
            raise ValueError('an index needs at least one element')
        if n >= 2 ** 31:
            raise ValueError('%d elements: ids must fit int32' % n)
        if nn_off.shape[0] != n + 1:
            raise ValueError('positives list %d elements, non_negatives %d' % (n, nn_off.shape[0] - 1))
        _check_csr(pos_off, pos_idx, n, 'positives')
        _check_csr(nn_off, nn_idx, n, 'non_negatives')
        self.n = n
        self.pos_off, self.nn_off = np.ascontiguousarray(pos_off), np.ascontiguousarray(nn_off)
        self.pos_idx, self.nn_idx = pos_idx.astype(np.int32), nn_idx.astype(np.int32)
        self.device = torch.device(device)
        self.dev = None
        if self.device.type == 'cuda':
            if not torch.cuda.is_available():
                raise _native.NativeLibraryError("TupleIndex(device='cuda') needs a GPU (device='cpu' builds a host-only index)")
            if self.device.index is None:
                self.device = torch.device('cuda', torch.cuda.current_device())
            # the kernel takes no null pointer: an id tensor keeps one element of storage even when every list is empty
            pad = lambda a: torch.from_numpy(a if a.size else np.zeros(1, np.int32)).to(self.device)      # noqa: E731
            self.dev = (torch.from_numpy(self.pos_off).to(self.device), pad(self.pos_idx),
                        torch.from_numpy(self.nn_off).to(self.device), pad(self.nn_idx))
        elif self.device.type != 'cpu':
            raise ValueError("device must be 'cuda' or 'cpu'")

    def __len__(self):
        return self.n

    @property
    def queries(self):
        """The element ids, as `list(dataset.queries)` enumerates them in the reference's `BatchSampler`."""
        return range(self.n)

    def get_positives(self, ndx: int) -> np.ndarray:
        return self.pos_idx[self.pos_off[ndx]:self.pos_off[ndx + 1]]

    def get_non_negatives(self, ndx: int) -> np.ndarray:
        return self.nn_idx[self.nn_off[ndx]:self.nn_off[ndx + 1]]


def _host_labels(labels, n: int) -> np.ndarray:
    a = labels.detach().cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)
    if a.ndim != 1 or a.shape[0] < 1:
        raise ValueError('labels: a non-empty 1-D sequence of element ids expected, got shape %s' % (a.shape,))
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError('labels: integer element ids expected, got %s' % a.dtype)
    a = a.astype(np.int64)
    bad = (a < 0) | (a >= n)
    if bad.any():
        k = int(np.argmax(bad))
        raise ValueError('labels[%d] = %d lies outside [0, %d)' % (k, int(a[k]), n))
    return a


def batch_masks(index: TupleIndex, labels, return_counts: bool = False):
    """`(positives_mask, negatives_mask)` of the batch `labels` (B element ids, repeats allowed): contiguous (B, B)
    `torch.bool` tensors on the index's device, written by one `hfl_batch_masks` launch on the current stream.  `labels`: a
    list, a numpy array or a tensor on either device; host labels are copied to the device, a device tensor is used as it
    is (one min / max read checks its range).  Labels outside [0, len(index)) raise ValueError before any launch.
    `return_counts`: also the (B, 2) int32 row sums of both masks.  No CPU fallback: NativeLibraryError off the GPU
    (`batch_masks_host` is the CPU route)."""
    from . import ops
    if not isinstance(index, TupleIndex):
        raise TypeError('batch_masks takes a TupleIndex (build it once per dataset)')
    if index.dev is None:
        raise _native.NativeLibraryError('batch_masks runs on the GPU (batch_masks_host is the CPU route)')
    n = len(index)
    if isinstance(labels, torch.Tensor) and labels.is_cuda:
        if labels.dim() != 1 or labels.shape[0] < 1:
            raise ValueError('labels: a non-empty 1-D tensor of element ids expected, got shape %s' % (tuple(labels.shape),))
        if labels.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
            raise ValueError('labels: integer element ids expected, got %s' % labels.dtype)
        if labels.device != index.device:
            raise _native.NativeLibraryError('labels on %s, the index on %s' % (labels.device, index.device))
        lo, hi = (int(v) for v in torch.stack(torch.aminmax(labels)).tolist())
        if lo < 0 or hi >= n:
            raise ValueError('labels span [%d, %d], outside [0, %d)' % (lo, hi, n))
        dev_labels = labels.to(torch.int64).contiguous()
    else:
        dev_labels = torch.from_numpy(_host_labels(labels, n)).to(index.device)
    with torch.cuda.device(index.device):
        pos, neg, counts = ops.batch_masks(dev_labels, *index.dev, n, return_counts=return_counts)
    return (pos, neg, counts) if return_counts else (pos, neg)


def batch_masks_host(index_or_queries, labels):
    """The same two masks as (B, B) numpy bool arrays, on the CPU: `np.isin` of the labels in each row's lists."""
    index = index_or_queries if isinstance(index_or_queries, TupleIndex) else TupleIndex(index_or_queries, device='cpu')
    lab = _host_labels(labels, len(index))
    pos = np.stack([np.isin(lab, index.get_positives(l)) for l in lab])
    neg = np.stack([~np.isin(lab, index.get_non_negatives(l)) for l in lab])
    return pos, neg
