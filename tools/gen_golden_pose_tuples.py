"""Build container only: the reference's own tuple lists and evaluation truth -> tests/golden/pose_tuples.npz.

Drives `construct_training_query_dict` and `construct_query_and_database_sets` of the reference's
`datasets/CSWildPlaces/generate_train_test_tuples.py` (:92-212) on small synthetic position sets, through the unchanged
`oracle.ref_import.install()`.  The module is imported as it is; third-party packages that are absent here (shapely, ...)
are stood in for by empty module objects whose attributes are placeholder classes that swallow their arguments (the module
builds its test polygons at import time), at generation time only -- nothing of them is used by the two functions.  The
module-level `args` the functions read is set to the thresholds of the case, with none of the generator's optional
variants, and `output_to_file` is replaced by a capture, so nothing is pickled.  The file holds arrays only: per case the
positions, the three thresholds, the CSR of `positives` and `non_negatives` of every `TrainingTuple`, and query / database
positions with the lists `test_sets[1][i][0]` in the order `query_radius` returned them.

Every case that is not on exact integer coordinates is redrawn until no pair has |d^2 - r^2| <= 1e-9 r^2 for any radius it
is queried at, so that sklearn's node bounds and the plain product cannot disagree and the tests compare without tolerance.

Usage:  python tools/gen_golden_pose_tuples.py"""
import importlib
import os
import sys
import types

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_import                                  # noqa: E402

UTM = np.array([5.0e5, 6.9e6])
SOURCE = "reference construct_training_query_dict / construct_query_and_database_sets (sklearn KDTree.query_radius inside)"


class _StandIn(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return type(name, (), {'__init__': lambda self, *a, **k: None})


def reference_generator():
    ref_import.install()
    for _ in range(64):
        try:
            return importlib.import_module('datasets.CSWildPlaces.generate_train_test_tuples')
        except ModuleNotFoundError as e:
            top = e.name.split('.')[0]
            if os.path.exists(os.path.join(ref_import.REFERENCE_ROOT, top)) or os.path.exists(
                    os.path.join(ref_import.REFERENCE_ROOT, top + '.py')):
                raise                                               # the reference's own module: not ours to replace
            print('stand-in for missing third-party module', e.name)
            sys.modules[e.name] = _StandIn(e.name)
            for name in [m for m in sys.modules if m.startswith(('datasets.', 'misc.', 'models.'))]:
                del sys.modules[name]
    raise RuntimeError('datasets.CSWildPlaces.generate_train_test_tuples does not import')


def csr(lists):
    off = np.concatenate([[0], np.cumsum([len(a) for a in lists])]).astype(np.int64)
    idx = np.concatenate([np.asarray(a, np.int64).reshape(-1) for a in lists]) if lists else np.zeros(0, np.int64)
    return off, idx.astype(np.int32)


def reference_lists(gen, positions, pos_thresh, neg_thresh):
    """positives / non_negatives of every TrainingTuple the reference builds for `positions`."""
    gen.args = types.SimpleNamespace(pos_thresh=pos_thresh, neg_thresh=neg_thresh, query_requires_ground=False,
                                     ground_aerial_positives_only=False)
    captured = {}
    gen.output_to_file = lambda output, filename: captured.__setitem__(filename, output)
    df = pd.DataFrame({'file': ['Karawatha/%s_01/clouds/%06d.pcd' % ('ground' if k % 3 else 'aerial', k)
                                for k in range(len(positions))],
                       'easting': positions[:, 0], 'northing': positions[:, 1]})
    gen.construct_training_query_dict(df, 'q_', test_set=False, v2_only=True)
    queries = captured['q_v2.pickle']
    assert sorted(queries) == list(range(len(positions)))
    for k in range(len(positions)):
        assert np.array_equal(queries[k].position, positions[k])
    return [queries[k].positives for k in range(len(positions))], [queries[k].non_negatives for k in range(len(positions))]


def reference_truth(gen, query_positions, database_positions, eval_thresh):
    """test_sets[1][i][0]: the database ids within eval_thresh of query i, as the reference stores them."""
    from sklearn.neighbors import KDTree
    gen.args = types.SimpleNamespace(eval_thresh=eval_thresh)
    captured = {}
    gen.output_to_file = lambda output, filename: captured.__setitem__(filename, output)
    rec = lambda p, k: {'query': '%06d' % k, 'easting': p[0], 'northing': p[1]}     # noqa: E731
    database_sets = [{k: rec(p, k) for k, p in enumerate(database_positions)}, {}]
    test_sets = [{}, {k: rec(p, k) for k, p in enumerate(query_positions)}]
    trees = [KDTree(pd.DataFrame(database_positions, columns=['easting', 'northing'])), None]
    gen.construct_query_and_database_sets(trees, database_sets, test_sets, 'e')
    out = captured['e_query.pickle']
    return [out[1][k][0] for k in range(len(query_positions))]


def margin_ok(a, b, radii):
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    d2 = dx * dx + dy * dy
    return all((np.abs(d2 - r * r) > 1e-9 * r * r).all() for r in radii)


def trajectory(n, seed):
    """A noisy figure-of-eight driven twice with a lateral offset: revisits, crossings and near misses at every threshold."""
    rng = np.random.RandomState(seed)
    t = np.linspace(0.0, 4.0 * np.pi, n, endpoint=False)
    lap = (t >= 2.0 * np.pi).astype(np.float64)
    xy = np.stack([220.0 * np.sin(t), 130.0 * np.sin(2.0 * t) + 7.0 * lap], 1)
    return UTM + xy + rng.normal(0.0, 2.5, xy.shape)


def exact_group():
    """Integer coordinates, where nothing rounds: around two hubs, pairs at exactly 5 (3-4-5) and exactly 15 (9-12-15), one
    lattice step beyond each, and duplicated positions."""
    hub = [(0, 0), (100, 40)]
    rel = [(0, 0), (0, 0),                                         # the hub twice: duplicates at distance 0
           (3, 4), (-4, 3), (5, 0), (0, -5), (3, 4),               # at 5 exactly (one of them twice)
           (4, 4), (3, 5), (6, 0), (-4, -4),                       # one step beyond 5
           (9, 12), (-12, 9), (15, 0), (0, -15),                   # at 15 exactly
           (9, 13), (10, 12), (16, 0), (-12, -10)]                 # one step beyond 15
    pts = np.array([(hx + rx, hy + ry) for hx, hy in hub for rx, ry in rel], np.float64)
    return UTM + pts


def f64_pair():
    """x1 = x0 + 15 -+ 2^-16 at x0 = 500000.25, r = 15, along either axis: float32 cannot tell these from x0 + 15."""
    x0, y0, e = 500000.25, 6900000.5, 2.0 ** -16
    return np.array([(x0, y0), (x0 + 15.0 - e, y0), (x0 + 15.0 + e, y0), (x0, y0 + 15.0 - e), (x0, y0 + 15.0 + e),
                     (x0 - 15.0 + e, y0), (x0 - 15.0 - e, y0)], np.float64)


def split_eval(positions, seed):
    """every third position is a query, the rest the database, queries nudged off their track"""
    rng = np.random.RandomState(seed)
    q = positions[::3] + rng.normal(0.0, 3.0, positions[::3].shape)
    return q, np.delete(positions, np.arange(0, len(positions), 3), axis=0)


def main():
    gen = reference_generator()
    out = {'source': np.array(SOURCE)}
    cases = []

    def add(name, positions, thresholds, queries, database, exact):
        pos_t, neg_t, eval_t = thresholds
        pos, nn = reference_lists(gen, positions, pos_t, neg_t)
        truth = reference_truth(gen, queries, database, eval_t)
        out[name + '.positions'] = positions
        out[name + '.thresholds'] = np.asarray(thresholds, np.float64)
        out[name + '.pos_off'], out[name + '.pos_idx'] = csr(pos)
        out[name + '.nn_off'], out[name + '.nn_idx'] = csr(nn)
        out[name + '.query_positions'], out[name + '.database_positions'] = queries, database
        out[name + '.truth_off'], out[name + '.truth_idx'] = csr(truth)
        out[name + '.exact'] = np.array(exact)
        cases.append(name)
        print('%-8s N %4d  positives %5d  non_negatives %6d  Q %3d  truth %5d' % (
            name, len(positions), out[name + '.pos_idx'].size, out[name + '.nn_idx'].size, len(queries),
            out[name + '.truth_idx'].size))

    for name, n, thresholds in (('wild', 300, (15.0, 60.0, 30.0)), ('oxford', 260, (10.0, 50.0, 25.0))):
        for seed in range(1000):
            p = trajectory(n, 100 * len(name) + seed)
            q, d = split_eval(p, seed)
            if margin_ok(p, p, thresholds[:2]) and margin_ok(q, d, thresholds[2:]):
                break
        else:
            raise RuntimeError('no seed satisfies the margin condition')
        print(name, 'seed offset', seed)
        add(name, p, thresholds, q, d, False)

    p = exact_group()
    add('exact', p, (5.0, 15.0, 5.0), p[::2].copy(), p[1::2].copy(), True)
    # the reference agrees with integer arithmetic on the exact group: the boundary is inside
    ip = np.rint(p - UTM).astype(np.int64)
    d2 = ((ip[:, None, :] - ip[None, :, :]) ** 2).sum(-1)
    for fam, r, drop_self in (('pos', 5, True), ('nn', 15, False)):
        m = d2 <= r * r
        if drop_self:
            np.fill_diagonal(m, False)
        off, idx = out['exact.%s_off' % fam], out['exact.%s_idx' % fam]
        for k in range(len(ip)):
            assert np.array_equal(idx[off[k]:off[k + 1]], np.nonzero(m[k])[0]), (fam, k)
    assert (d2 == 25).sum() > 0 and (d2 == 225).sum() > 0 and ((d2 > 25) & (d2 <= 36)).sum() > 0

    p = f64_pair()
    assert margin_ok(p, p, (15.0, 60.0))
    add('f64pair', p, (15.0, 60.0, 15.0), p[:1].copy(), p[1:].copy(), False)
    off, idx = out['f64pair.pos_off'], out['f64pair.pos_idx']
    assert idx[off[0]:off[1]].tolist() == [1, 3, 5], idx[off[0]:off[1]]
    as32 = p.astype(np.float32)
    assert as32[1, 0] == as32[2, 0] and as32[3, 1] == as32[4, 1]            # float32 cannot classify the pair

    out['cases'] = np.array(cases)
    path = os.path.join(ROOT, 'tests', 'golden', 'pose_tuples.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
