"""Build container only: the reference's own batch masks -> tests/golden/batch_masks.npz.

Calls `in_sorted_array` of the reference's `datasets/dataset_utils.py` (:201-206) in the two nested list comprehensions of
its collate function (:120-121) on a small synthetic index, through the unchanged `oracle.ref_import.install()`.
`dataset_utils` imports the whole data pipeline at module level; third-party packages that are absent here (torchvision,
open3d, ...) are stood in for by empty module objects whose attributes are placeholder classes, at generation time only.
Nothing of them is called.  The file holds arrays only: the CSR of both list families, the labels and the two masks per case.

Usage:  python tools/gen_golden_batch_masks.py"""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_import                                  # noqa: E402


class _StandIn(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return type(name, (), {})


def reference_in_sorted_array():
    ref_import.install()
    for _ in range(64):
        try:
            return importlib.import_module('datasets.dataset_utils').in_sorted_array
        except ModuleNotFoundError as e:
            top = e.name.split('.')[0]
            if os.path.exists(os.path.join(ref_import.REFERENCE_ROOT, top)) or os.path.exists(
                    os.path.join(ref_import.REFERENCE_ROOT, top + '.py')):
                raise                                               # the reference's own module: not ours to replace
            print('stand-in for missing third-party module', e.name)
            sys.modules[e.name] = _StandIn(e.name)
            for name in [m for m in sys.modules if m.startswith(('datasets.', 'misc.', 'models.'))]:
                del sys.modules[name]
    raise RuntimeError('datasets.dataset_utils does not import')


def make_index(n, seed):
    """Sorted lists of every kind the product accepts: empty, full, repeated entries, ids 0 and n - 1, random."""
    rng = np.random.RandomState(seed)
    pos, nn = [], []
    for k in range(n):
        p = np.sort(rng.choice(n, rng.randint(0, 6), replace=False))
        q = np.union1d(p, rng.choice(n, rng.randint(0, 15), replace=False))
        pos.append(p.astype(np.int64))
        nn.append(q.astype(np.int64))
    pos[0], nn[0] = np.zeros(0, np.int64), np.zeros(0, np.int64)
    pos[1], nn[1] = np.arange(n), np.arange(n)
    pos[2], nn[2] = np.array([0, 0, 5, 5, 5, n - 1, n - 1]), np.array([0, 0, 2, 5, 5, 5, 9, n - 1, n - 1])
    pos[3], nn[3] = np.array([0]), np.array([0, n - 1])
    pos[n - 1], nn[n - 1] = np.array([n - 1]), np.array([n - 2, n - 1])
    return pos, nn


def csr(lists):
    off = np.concatenate([[0], np.cumsum([len(a) for a in lists])]).astype(np.int64)
    return off, np.concatenate(lists).astype(np.int32)


def main():
    in_sorted_array = reference_in_sorted_array()
    n = 40
    pos, nn = make_index(n, 20260)
    out = {}
    out['pos_off'], out['pos_idx'] = csr(pos)
    out['nn_off'], out['nn_idx'] = csr(nn)
    rng = np.random.RandomState(7)
    cases = {'b1': [2], 'b4': [0, 1, 2, n - 1], 'b7': [3, 1, 3, 0, n - 1, 2, 17],
             'b33': [int(v) for v in rng.randint(0, n, 33)]}
    for name, labels in cases.items():
        # the collate function's two comprehensions (dataset_utils.py:120-121), verbatim in structure
        positives_mask = [[in_sorted_array(e, pos[label]) for e in labels] for label in labels]
        negatives_mask = [[not in_sorted_array(e, nn[label]) for e in labels] for label in labels]
        out[name + '.labels'] = np.asarray(labels, np.int64)
        out[name + '.pos'] = np.asarray(positives_mask, dtype=bool)
        out[name + '.neg'] = np.asarray(negatives_mask, dtype=bool)
    path = os.path.join(ROOT, 'tests', 'golden', 'batch_masks.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
