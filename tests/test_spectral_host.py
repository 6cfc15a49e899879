"""The definition of `hotformerloc_amd/spectral.py` on the CPU: the numpy twins against an independent dense yardstick, an
exact case, the purpose they exist for and their refusals.  `tests/test_gpu_spectral.py` holds the device against these
twins.

Yardstick: M built densely in float64 and `numpy.linalg.eigvalsh`.  The host eigenvalue after 10 rounds must lie within 1e-5
relative of lambda_max.  Seen on `corrupted(frac)`, sigma = 0.2: 4.9e-06 (frac 0.0, 678 equal terms added in fp32), 4.1e-08
(0.6), 6.6e-09 (0.9), 4.0e-08 (1.0); second-to-first eigenvalue ratios -0.0015, 0.048, 0.26, 0.42."""
import os
import re

import numpy as np
import pytest

import hotformerloc_amd as hfl
from hotformerloc_amd import _native, build, ops
from hotformerloc_amd import spectral as sp
from tests import global_registration_cases as gc
from tests import spectral_cases as sc
from tests.test_gpu_global_registration import GLOBAL_BOUNDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_and_constants_mirror_the_header():
    for name in ('spectral_consistency', 'prune_correspondences', 'rerank_candidates'):
        assert callable(getattr(hfl, name)) and callable(getattr(hfl, name + '_host'))
    assert hfl.SpectralResult._fields == ('eigenvalue', 'score', 'weights')
    assert hfl.RerankResult._fields == ('indices', 'scores', 'order')
    header = open(os.path.join(ROOT, 'include', 'hotformerloc_hip.h')).read()
    for name, value in (('ROWS', ops.SPECTRAL_ROWS), ('TILE', ops.SPECTRAL_TILE), ('SUMS', ops.SPECTRAL_SUMS)):
        assert int(re.search(r'#define HFL_SPECTRAL_%s (\d+)' % name, header).group(1)) == value
    assert ops.SPECTRAL_TILE * 7 * 4 <= 32 * 1024 and ops.SPECTRAL_TILE % ops.SPECTRAL_ROWS == 0
    assert 'spectral.hip' in build.SOURCES and '-ffp-contract=off' in build.EXTRA_FLAGS['spectral.hip']
    for symbol in ('hfl_spectral_matvec', 'hfl_spectral_finish'):
        assert symbol in _native.SIGNATURES


def test_spectral_tiles():
    r = ops.SPECTRAL_ROWS
    tiles, off = ops.spectral_tiles([0, 1, r, r + 1, 0])
    assert off.tolist() == [0, 0, 1, 2, 4, 4]
    assert tiles.tolist() == [[1, 0], [2, 1], [3, r + 1], [3, 2 * r + 1]]


@pytest.mark.parametrize('frac', sc.FRACTIONS)
def test_eigenvalue_against_the_dense_float64_eigensolver(frac):
    src, dst, rows = gc.corrupted(frac)
    res = sc.host_corrupted(frac)
    ev = sc.dense_eigenvalues(src, dst, rows, sc.SIGMA)
    rel = abs(res.eigenvalue[0] - ev[-1]) / ev[-1]
    print('frac %.1f: eigenvalue %.9g, lambda_max %.9g, relative %.3g, second / first %.3g'
          % (frac, res.eigenvalue[0], ev[-1], rel, ev[-2] / ev[-1]))
    assert rel <= 1e-5
    w = res.weights[0]
    assert w.dtype == np.float32 and (w >= 0).all() and abs(np.linalg.norm(w.astype(np.float64)) - 1.0) < 1e-6
    assert res.score[0] == res.eigenvalue[0] / src.shape[0]


def test_the_matrix_is_symmetric_to_the_bit_with_a_zero_diagonal():
    src, dst, rows = gc.corrupted(0.6)
    m = sp._host_matrix(src[rows[:300, 0]], dst[rows[:300, 1]], np.float32(1.0 / sc.SIGMA ** 2))
    assert m.dtype == np.float32 and np.array_equal(m, m.T) and not m.diagonal().any() and m.max() <= 1.0 and m.min() >= 0.0


def test_purpose_the_score_separates_and_the_weights_find_the_true_rows():
    assert sc.host_corrupted(0.9).score[0] > 2.0 * sc.host_corrupted(1.0).score[0]
    for frac in (0.6, 0.9):
        true = gc.true_rows(frac)
        top = np.argsort(-sc.host_corrupted(frac).weights[0], kind='stable')[:int(true.sum())]
        print('frac %.1f: score %.4f, %d true rows, share of true rows among the largest weights %.3f'
              % (frac, sc.host_corrupted(frac).score[0], int(true.sum()), true[top].mean()))
        assert true[top].all()


def test_purpose_pruned_correspondences_give_the_pose_at_ninety_percent_wrong():
    src, dst, rows = gc.corrupted(0.9)
    true = gc.true_rows(0.9)
    kept = hfl.prune_correspondences_host([rows], sc.host_corrupted(0.9).weights, int(true.sum()))
    assert np.array_equal(kept[0], rows[true])
    res = hfl.ransac_registration_host([src], [dst], kept, max_correspondence_distance=gc.TAU,
                                       hypotheses=gc.PURPOSE['hypotheses'], seed=gc.PURPOSE['ransac_seed'])
    angle, shift = gc.pose_error(res.transforms[0])
    print('pose error %.3g degrees, %.3g m' % (angle, shift))
    assert angle < gc.ANGLE_TOL_DEG and shift < gc.SHIFT_TOL


@pytest.mark.parametrize('iterations', (1, 2, 10))
def test_exact_case(iterations):
    src, dst, rows, true = sc.exact_case()
    n_true = int(true.sum())
    m = sp._host_matrix(src, dst, np.float32(1.0 / 0.4 ** 2))
    assert np.array_equal(m, (true[:, None] & true[None, :] & ~np.eye(true.shape[0], dtype=bool)).astype(np.float32))
    res = hfl.spectral_consistency_host([src], [dst], [rows], iterations=iterations)
    w = res.weights[0]
    assert not w[~true].any()                                          # exactly 0 outside the block
    assert (w[true] == w[true][0]).all() and w[true][0] == np.float32(1.0 / np.sqrt(n_true))
    # the first Rayleigh quotient is that of the all-ones vector over every row; from the second on it is the block's
    want = n_true * (n_true - 1) / true.shape[0] if iterations == 1 else n_true - 1
    assert abs(res.eigenvalue[0] - want) <= 1e-12 * want
    assert res.score[0] == res.eigenvalue[0] / src.shape[0]


def test_degenerate_inputs():
    src, dst = gc.clouds()
    batch = ([src] * 4, [dst] * 4, [gc.rows(c, 0.0, 1) for c in (0, 1, 2)] + [np.array([[0, 0], [1, 400], [2, 200]])])
    res = hfl.spectral_consistency_host(*batch, distance_threshold=0.05)
    # no rows; one row supports nothing; two true rows support each other fully; three rows of which no two agree
    assert res.eigenvalue.tolist() == [0.0, 0.0, res.eigenvalue[2], 0.0] and abs(res.eigenvalue[2] - 1.0) < 1e-6
    assert [w.shape[0] for w in res.weights] == [0, 1, 2, 3] and all(w.dtype == np.float32 for w in res.weights)
    assert not res.weights[1].any() and not res.weights[3].any()
    assert res.weights[2][0] == res.weights[2][1] and abs(float(res.weights[2][0]) - np.sqrt(0.5)) < 1e-7
    assert res.score.tolist() == (res.eigenvalue / src.shape[0]).tolist()
    # the (rows, offsets) form: the same figures, the weights concatenated
    off = np.cumsum([0] + [r.shape[0] for r in batch[2]])
    packed = hfl.spectral_consistency_host(*batch[:2], (np.concatenate(batch[2]), off), distance_threshold=0.05)
    assert np.array_equal(packed.eigenvalue, res.eigenvalue) and np.array_equal(packed.weights, np.concatenate(res.weights))


def test_refusals():
    src, dst, rows = gc.corrupted(0.6)
    host = hfl.spectral_consistency_host
    for kw in (dict(distance_threshold=0.0), dict(distance_threshold=-1.0), dict(distance_threshold=np.nan),
               dict(distance_threshold=np.inf), dict(distance_threshold=1e-30), dict(iterations=0), dict(iterations=2.5)):
        with pytest.raises(ValueError):
            host([src], [dst], [rows], **kw)
    with pytest.raises(ValueError):
        host([src, src], [dst], [rows, rows])                          # the clouds do not pair up
    with pytest.raises(ValueError):
        host([src], [dst], [rows, rows])                               # nor do the correspondences
    with pytest.raises(ValueError):
        host([src], [dst], rows)                                       # neither a list nor a (rows, offsets) tuple
    with pytest.raises(ValueError):
        host([src], [dst], [rows[:, :1]])
    with pytest.raises(TypeError):
        host([src], [dst], [rows.astype(np.float32)])
    with pytest.raises(ValueError):
        host([src], [dst], [np.array([[0, dst.shape[0]]])])            # a row outside its cloud
    with pytest.raises(ValueError):
        host((src, np.array([0, src.shape[0]])), (dst, np.array([0, dst.shape[0]])), (rows, np.array([0, 5])))
    with pytest.raises(TypeError):
        host([src.astype(np.float64)], [dst], [rows])
    w = np.ones(rows.shape[0], np.float32)
    prune = hfl.prune_correspondences_host
    for bad in (lambda: prune([rows], [w], -1), lambda: prune([rows], [w], 1.5), lambda: prune([rows], w, 3),
                lambda: prune([rows], [w[:5]], 3), lambda: prune(rows, w, 3), lambda: prune([rows], [w, w], 3)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        prune([rows], [w.astype(np.float64)], 3)
    with pytest.raises(_native.NativeLibraryError):
        hfl.spectral_consistency([src], [dst], [rows])                 # CPU clouds on the device route


def test_prune_keeps_the_largest_the_lower_row_of_a_tie_and_no_zero():
    rows = [np.stack([np.arange(6), np.arange(6) + 10], 1), np.zeros((0, 2), np.int64), np.stack([np.arange(3), np.arange(3)], 1)]
    weights = [np.array([0.5, 0.0, 0.7, 0.5, 0.5, 0.1], np.float32), np.zeros(0, np.float32), np.array([0.0, 0.0, 0.3], np.float32)]
    kept = hfl.prune_correspondences_host(rows, weights, 3)
    assert [k.tolist() for k in kept] == [[[0, 10], [2, 12], [3, 13]], [], [[2, 2]]]   # original order; the tie: rows 0, 3 before 4
    assert [k.tolist() for k in hfl.prune_correspondences_host(rows, weights, 0)] == [[], [], []]
    assert [k.shape[0] for k in hfl.prune_correspondences_host(rows, weights, 100)] == [5, 0, 1]
    packed, off = hfl.prune_correspondences_host((np.concatenate(rows), np.array([0, 6, 6, 9])), np.concatenate(weights), 3)
    assert np.array_equal(packed, np.concatenate(kept)) and off.tolist() == [0, 3, 3, 4] and off.dtype == np.int64
    import torch
    t_kept = hfl.prune_correspondences([torch.from_numpy(r) for r in rows], [torch.from_numpy(w) for w in weights], 3)
    assert all(np.array_equal(a.numpy(), b) for a, b in zip(t_kept, kept))       # the torch route, here on CPU tensors


def test_rerank_orders_by_geometry():
    res = sc.host_rerank()
    print('scores', res.scores[0])
    assert [sc.DATABASE[i] for i in res.indices[0, :5]] == list(sc.EXPECTED_ORDER) and res.indices[0, 5] == -1
    assert res.scores[0, 5] == -1.0 and (np.diff(res.scores[0]) <= 0).all()
    assert res.scores[0, 0] > 10.0 * res.scores[0, 2]
    assert res.indices.dtype == np.int64 and res.order.dtype == np.int64 and res.scores.dtype == np.float64
    assert np.array_equal(res.indices[0], sc.rerank_inputs()[2][0][res.order[0]])


def test_rerank_with_registration_of_the_top_candidate():
    ranked, coarse, fine = sc.host_rerank(register=True)
    assert np.array_equal(ranked.indices, sc.host_rerank().indices) and np.array_equal(ranked.scores, sc.host_rerank().scores)
    angle, shift = gc.pose_error(fine.transforms[0], sc.rerank_truth())
    print('coarse %.3g degrees %.3g m, fine %.3g degrees %.3g m'
          % (gc.pose_error(coarse.transforms[0], sc.rerank_truth()) + (angle, shift)))
    assert coarse.transforms.shape == fine.transforms.shape == (1, 4, 4)
    assert angle <= GLOBAL_BOUNDS['point_to_plane'][0] and shift <= GLOBAL_BOUNDS['point_to_plane'][1]


def test_rerank_computes_features_once_per_distinct_cloud_and_keeps_ties_and_unused_slots(monkeypatch):
    from hotformerloc_amd import normals as normals_module
    seen = []
    real = normals_module.estimate_normals_host
    monkeypatch.setattr(normals_module, 'estimate_normals_host', lambda clouds, nb: seen.append(len(clouds)) or real(clouds, nb))
    names = ('plane37', 'collinear', 'duplicated', 'one')
    from tests import fpfh_cases as fc
    database = [fc.cloud_of(n) for n in names]
    queries = [fc.cloud_of('plane37'), fc.cloud_of('duplicated'), fc.cloud_of('collinear')]
    cand = np.array([[2, 0, 0], [0, 2, -1], [-1, -1, -1]])             # database row 3 is named by nobody; row 0 twice by query 0
    res = hfl.rerank_candidates_host(queries, database, cand, keep=20)
    assert seen == [3 + 2]                                             # three queries and the two distinct named rows, once
    assert res.indices.tolist() == [[0, 0, 2], [2, 0, -1], [-1, -1, -1]]
    assert res.order.tolist() == [[1, 2, 0], [1, 0, 2], [0, 1, 2]]     # equal scores keep their retrieval order
    assert res.scores[0, 0] == res.scores[0, 1] > res.scores[0, 2] >= 0.0 and res.scores[2].tolist() == [-1.0] * 3
    with pytest.raises(ValueError):
        hfl.rerank_candidates_host(queries, database, cand, register=True)         # query 2 has no candidate
    for bad in (np.array([[4, 0, 0]] * 3), np.array([[-2, 0, 0]] * 3), cand[:2], cand.astype(np.float32)):
        with pytest.raises(ValueError):
            hfl.rerank_candidates_host(queries, database, bad)
    with pytest.raises(ValueError):
        hfl.rerank_candidates_host(queries, database, cand, estimation='nonsense')
