"""Shared inputs of the pose-tuple tests (tests/test_pose_tuples_host.py, tests/test_gpu_pose_tuples.py): the golden cases
of tests/golden/pose_tuples.npz (tools/gen_golden_pose_tuples.py: the reference's own generator functions), generated
position sets for the kernel's tiling edges, and a fixed search result for the metric."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pose_tuples.npz')
UTM = np.array([5.0e5, 6.9e6])
_CACHE = {}


class Tup:
    """What the product reads of the reference's `TrainingTuple`."""

    def __init__(self, positives, non_negatives):
        self.positives = np.asarray(positives, dtype=np.int64)
        self.non_negatives = np.asarray(non_negatives, dtype=np.int64)


class Case:
    """One golden case: positions, (pos, neg, eval) thresholds, the reference's lists as CSR, the evaluation split."""

    def __init__(self, z, name):
        self.name = name
        for key in ('positions', 'pos_off', 'pos_idx', 'nn_off', 'nn_idx', 'query_positions', 'database_positions',
                    'truth_off', 'truth_idx'):
            setattr(self, key, z['%s.%s' % (name, key)])
        self.pos_thresh, self.neg_thresh, self.eval_thresh = (float(v) for v in z[name + '.thresholds'])
        self.exact = bool(z[name + '.exact'])
        self.n = self.positions.shape[0]

    def tuples(self):
        """dict 0..N-1 -> Tup, the form `TupleIndex(queries)` takes"""
        return {k: Tup(self.pos_idx[self.pos_off[k]:self.pos_off[k + 1]], self.nn_idx[self.nn_off[k]:self.nn_off[k + 1]])
                for k in range(self.n)}

    def truth_rows(self):
        """the reference's lists of true neighbours, in the order it stored them"""
        return [self.truth_idx[self.truth_off[k]:self.truth_off[k + 1]] for k in range(self.truth_off.shape[0] - 1)]

    def query_sets(self):
        """the dict form `retrieval.truth_csr(query_sets, 1, 0)` walks: query set 1 against database set 0"""
        return [{}, {k: {0: row.tolist()} for k, row in enumerate(self.truth_rows())}]


def golden():
    """name -> Case, loaded once"""
    if 'golden' not in _CACHE:
        z = np.load(GOLDEN)
        _CACHE['golden'] = {str(name): Case(z, str(name)) for name in z['cases']}
        _CACHE['source'] = str(z['source'])
    return _CACHE['golden']


CASE_NAMES = ('wild', 'oxford', 'exact', 'f64pair')


def sorted_rows(off, idx):
    """every list sorted: the reference stores evaluation truth in the tree's order"""
    return np.concatenate([np.sort(idx[off[k]:off[k + 1]]) for k in range(off.shape[0] - 1)] + [np.zeros(0, idx.dtype)])


def strictly_ascending(off, idx):
    if idx.size < 2:
        return True
    rises = np.diff(idx.astype(np.int64)) > 0
    starts = np.zeros(idx.shape[0], bool)
    starts[off[:-1][off[:-1] < idx.shape[0]]] = True
    return bool((rises | starts[1:]).all())


def positions(n, seed, extent=400.0, duplicates=True):
    """n positions at UTM magnitudes scattered over extent x extent metres; about a tenth repeat an earlier position"""
    rng = np.random.RandomState(seed)
    p = UTM + rng.uniform(0.0, extent, (n, 2))
    if duplicates and n > 3:
        k = rng.choice(n, max(1, n // 10), replace=False)
        p[k] = p[rng.randint(0, n, k.shape[0])]
    return p


def search_result(n_queries, n_database, seed=5, k=25):
    """a fixed (Q, 25) index array standing for a search result"""
    return np.random.RandomState(seed).randint(0, n_database, (n_queries, k)).astype(np.int64)
