"""Shared inputs of the batch-mask tests (tests/test_batch_masks_host.py, tests/test_gpu_batch_masks.py): small indexes with
every kind of list the product accepts, label vectors that hit list ends, and a brute-force set-membership reference."""
import numpy as np


class Tup:
    """What the product reads of the reference's `TrainingTuple`."""

    def __init__(self, positives, non_negatives):
        self.positives = np.asarray(positives, dtype=np.int64)
        self.non_negatives = np.asarray(non_negatives, dtype=np.int64)


def small_queries(n=40, seed=3):
    """dict 0..n-1 -> Tup: random short sorted lists, plus an empty list, a full one (all n ids), one with repeated entries
    and lists holding ids 0 and n - 1."""
    rng = np.random.RandomState(seed)
    q = {}
    for k in range(n):
        p = np.sort(rng.choice(n, rng.randint(0, 6), replace=False))
        q[k] = Tup(p, np.union1d(p, rng.choice(n, rng.randint(0, 15), replace=False)))
    q[0] = Tup([], [])
    q[1] = Tup(np.arange(n), np.arange(n))
    q[2] = Tup([0, 0, 5, 5, 5, n - 1, n - 1], [0, 0, 2, 5, 5, 5, 9, n - 1, n - 1])
    q[3] = Tup([0], [0, n - 1])
    q[n - 1] = Tup([n - 1], [n - 2, n - 1])
    return q


def random_queries(n, seed):
    """Random sorted lists of every length 0..n (list 0 empty, list 1 full, list 2 with both ends 0 and n - 1)."""
    rng = np.random.RandomState(seed)
    q = [Tup(np.sort(rng.choice(n, rng.randint(0, n + 1), replace=False)),
             np.sort(rng.choice(n, rng.randint(0, n + 1), replace=False))) for _ in range(n)]
    q[0] = Tup([], [])
    q[1] = Tup(np.arange(n), np.arange(n))
    q[2] = Tup([0, n // 2, n - 1], [0, 1, n - 1])
    return q


def labels_hitting_ends(queries, n, batch, seed, e=None):
    """`batch` labels: element e, the first and last entry of both its lists, e again (a repeat, and a label equal to its
    own row's label), 0 and n - 1, then random ids."""
    rng = np.random.RandomState(seed)
    if e is None:
        e = next(k for k in range(3, n) if len(queries[k].positives) > 1 and len(queries[k].non_negatives) > 1)
    t = queries[e]
    head = [e, t.positives[0], t.positives[-1], t.non_negatives[0], t.non_negatives[-1], e, 0, n - 1]
    lab = [int(v) for v in head[:batch]] + [int(v) for v in rng.randint(0, n, max(0, batch - len(head)))]
    return np.asarray(lab, np.int64)


def brute_force(queries, labels):
    """labels[j] in set(list_i), as a double Python loop."""
    b = len(labels)
    pos, neg = np.zeros((b, b), bool), np.zeros((b, b), bool)
    for i, li in enumerate(labels):
        sp = set(int(v) for v in queries[int(li)].positives)
        sn = set(int(v) for v in queries[int(li)].non_negatives)
        for j, lj in enumerate(labels):
            pos[i, j] = int(lj) in sp
            neg[i, j] = int(lj) not in sn
    return pos, neg


def long_queries(cap, family, seed=11):
    """n = cap + 300 elements; elements 0..5 carry a `family` list ('positives' or 'non_negatives') of length
    0, 1, cap - 1, cap, cap + 1 and n, every other list is short."""
    n = cap + 300
    rng = np.random.RandomState(seed)
    q = []
    for k in range(n):
        q.append(Tup(np.sort(rng.choice(n, rng.randint(0, 6), replace=False)),
                     np.sort(rng.choice(n, rng.randint(0, 6), replace=False))))
    for k, length in enumerate((0, 1, cap - 1, cap, cap + 1, n)):
        long = np.sort(rng.choice(n, length, replace=False))
        q[k] = Tup(long, q[k].non_negatives) if family == 'positives' else Tup(q[k].positives, long)
    return q, n


def long_labels(queries, n, family, batch=65, seed=12):
    """The six long-list elements, the first and last entry of each of their lists, then random ids."""
    rng = np.random.RandomState(seed)
    lab = list(range(6))
    for k in range(1, 6):
        a = getattr(queries[k], family)
        lab += [int(a[0]), int(a[-1])]
    lab += [int(v) for v in rng.randint(0, n, batch - len(lab))]
    return np.asarray(lab, np.int64)
