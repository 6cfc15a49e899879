"""Shared inputs of the intra-sequence tests (tests/test_intra_sequence_host.py, tests/test_gpu_intra_sequence.py): seeded
descriptors and limits for the prefix search, the numpy float64 search inside a prefix with the gap guard of
`FlatL2Index.search`, and the synthetic runs of the protocol tests."""
import numpy as np

UTM = np.array([5.0e5, 6.9e6])
EPOCH = 1.6e9
LAP, LAPS = 400, 2                      # a closed 400 m loop walked twice at 1 m/s, one scan per second
TIME_THRESH, WORLD_THRESH = 100.0, 3.0
DIM = 64
_CACHE = {}


def descriptors(seed, rows, dim, scale=1.0):
    return ((np.random.RandomState(seed).uniform(0.0, 1.0, (rows, dim)) - 0.5) * scale).astype(np.float32)


def random_limits(seed, n_queries, n_database):
    """non-monotone limits in [0, N] with 0 and N forced in"""
    lim = np.random.RandomState(seed).randint(0, n_database + 1, n_queries).astype(np.int64)
    lim[n_queries // 3] = 0
    lim[(2 * n_queries) // 3] = n_database
    return lim


# ------------------------------------------------------------------------------------------ numpy search inside a prefix
def host_prefix_topk(queries, database, limits, k):
    """(d2 (Q, k) float64, idx (Q, k) int64, guard (Q,) bool): per query the k nearest rows of database[:limits[q]] by the
    f64 distance ((q - d)^2).sum() of the fp32 values, stable (equal distances by lower index), +inf / -1 past the prefix.
    guard[q]: the k-th and the 33rd smallest distance inside the prefix differ by more than 2^-22 (D + 4) (|q|^2 + |d|^2),
    |d|^2 the largest of the prefix -- or the prefix has no 33rd row, so that every row is a candidate."""
    q = np.asarray(queries, dtype=np.float32).astype(np.float64)
    db = np.asarray(database, dtype=np.float32).astype(np.float64)
    dim = q.shape[1]
    d2 = np.full((q.shape[0], k), np.inf)
    idx = np.full((q.shape[0], k), -1, dtype=np.int64)
    guard = np.ones(q.shape[0], dtype=bool)
    dn = (db * db).sum(1)
    for i in range(q.shape[0]):
        lim = int(limits[i])
        if lim == 0:
            continue
        diff = db[:lim] - q[i]
        dist = (diff * diff).sum(1)
        order = np.argsort(dist, kind='stable')
        kc = min(k, lim)
        d2[i, :kc], idx[i, :kc] = dist[order[:kc]], order[:kc]
        if lim > 32:
            bound = 2.0 ** -22 * (dim + 4) * ((q[i] * q[i]).sum() + dn[:lim].max())
            guard[i] = dist[order[32]] - dist[order[kc - 1]] > bound
    return d2, idx, guard


# ------------------------------------------------------------------------------------------------------ the synthetic runs
def loop_positions():
    """(800, 2) float64: the perimeter of a 100 m square from its corner, one metre a scan, twice round; whole metres on
    top of a UTM offset, so every squared distance is exact in float64"""
    s = np.arange(LAP * LAPS) % LAP
    side, along = s // 100, (s % 100).astype(np.float64)
    x = np.select([side == 0, side == 1, side == 2, side == 3], [along, 100.0, 100.0 - along, 0.0])
    y = np.select([side == 0, side == 1, side == 2, side == 3], [0.0, along, 100.0, 100.0 - along])
    return UTM + np.stack([x, y], 1)


def embed(positions, seed=7, noise=0.01):
    """a fixed random projection of (x, y, 1) to D = 64, seeded noise, L2-normalised; fp32"""
    rng = np.random.RandomState(seed)
    local = (positions - UTM) / 100.0
    feat = np.concatenate([local, np.ones((local.shape[0], 1))], 1)
    e = feat @ rng.standard_normal((3, DIM)) + noise * rng.standard_normal((local.shape[0], DIM))
    return (e / np.linalg.norm(e, axis=1, keepdims=True)).astype(np.float32)


def run(name):
    """name -> (embeddings (N, 64) fp32, positions (N, 2), timestamps (N,)), built once, shared and left as they are:
    'loop' the two laps; 'perturbed' the same with every tenth embedding of the second lap replaced by noise (false
    positives and misses); 'line' 300 m straight ahead, no revisit."""
    if name not in _CACHE:
        if name == 'line':
            pos = UTM + np.stack([np.arange(300.0), np.zeros(300)], 1)
        else:
            pos = loop_positions()
        emb = embed(pos)
        if name == 'perturbed':
            rows = np.arange(LAP, LAP * LAPS, 10)
            junk = np.random.RandomState(11).standard_normal((rows.shape[0], DIM))
            emb[rows] = (junk / np.linalg.norm(junk, axis=1, keepdims=True)).astype(np.float32)
        ts = EPOCH + np.arange(pos.shape[0], dtype=np.float64)
        _CACHE[name] = (emb, pos, ts)
    return _CACHE[name]


def host_result(name, thresholds=None):
    """`evaluate_intra_sequence_host` of a run at the tests' thresholds, computed once per (run, cuts)"""
    from hotformerloc_amd import retrieval
    key = (name, None if thresholds is None else tuple(np.asarray(thresholds).tolist()))
    if key not in _CACHE:
        emb, pos, ts = run(name)
        _CACHE[key] = retrieval.evaluate_intra_sequence_host(emb, pos, ts, time_thresh=TIME_THRESH,
                                                             world_thresh=WORLD_THRESH, thresholds=thresholds)
    return _CACHE[key]


def run_set_from(positions, timestamps, keys):
    """the reference's per-run dict: scan r of the time-ordered run stored under keys[r]"""
    return {int(key): {'query': 'clouds/%.3f.pcd' % timestamps[r], 'northing': float(positions[r, 1]),
                       'easting': float(positions[r, 0]), 'pose': np.zeros(7), 'timestamp': float(timestamps[r])}
            for r, key in enumerate(keys)}
