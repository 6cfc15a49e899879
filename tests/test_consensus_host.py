"""The definition of `hotformerloc_amd/consensus.py` on the CPU: the numpy twins against hand values, an independent dense
float64 construction, the purpose they exist for and their refusals.  `tests/test_gpu_consensus.py` holds the device against
these twins.

Purpose, on `corrupted(frac)` (678 correspondences, 40 degrees / 3 m), d = 0.1, tau = `gc.TAU`, 64 seeds of 10 members, against
`ransac_registration_host(hypotheses=4096, seed=0)`:

    wrong rows  true rows  random triples, 4 096             consensus, 64 seeds x 10 members
    60 %        271        3.4e-07 deg, 271 inliers          4.3e-07 deg / 1.6e-07 m, 271 inliers
    90 %        68         1.4e-06 deg, 68 inliers           2.7e-06 deg / 1.5e-07 m, 68 inliers
    95 %        34         8.6 deg / 0.78 m, 0 inliers       3.2e-06 deg / 1.2e-07 m, 34 inliers
    97 %        20         134 deg / 3.9 m, 0 inliers        1.2e-06 deg / 1.7e-07 m, 20 inliers
    98 %        14         134 deg / 3.9 m, 0 inliers        9.8e-07 deg / 2.6e-07 m, 14 inliers
    99 %        7          134 deg / 3.9 m, 0 inliers        8.5 deg / 0.58 m, 1 inlier: beyond both

`global_registration_host(estimator='consensus')` on the two raw plane clouds ends 1.30e-06 degrees / 6.79e-08 m (point to
plane) and 1.16e-06 degrees / 7.54e-08 m (point to point) from the truth, inside `GLOBAL_BOUNDS` (1.91e-06 / 2.42e-07 and
1.89e-06 / 3.30e-07); its coarse pose, 1.77e-07 degrees / 1.31e-07 m with all 678 mutual matches as inliers."""
import os
import re

import numpy as np
import pytest

import hotformerloc_amd as hfl
from hotformerloc_amd import _native, build, ops
from hotformerloc_amd import consensus as cs
from hotformerloc_amd import registration as reg
from tests import consensus_cases as cc
from tests import global_registration_cases as gc
from tests import spectral_cases as sc
from tests.test_gpu_global_registration import GLOBAL_BOUNDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GR = gc.GR


def test_exports_and_constants_mirror_the_header():
    for name in ('consensus_hypotheses', 'consensus_registration'):
        assert callable(getattr(hfl, name)) and callable(getattr(hfl, name + '_host'))
    header = open(os.path.join(ROOT, 'include', 'hotformerloc_hip.h')).read()
    for name, value in (('ROWS', ops.CONSENSUS_ROWS), ('TILE', ops.CONSENSUS_TILE),
                        ('MAX_CORRESPONDENCES', ops.CONSENSUS_MAX_CORRESPONDENCES), ('MAX_SIZE', ops.CONSENSUS_MAX_SIZE)):
        assert int(re.search(r'#define HFL_CONSENSUS_%s (\d+)' % name, header).group(1)) == value
    assert cs.CONSENSUS_MAX_CORRESPONDENCES == ops.CONSENSUS_MAX_CORRESPONDENCES == 16384
    assert cs.CONSENSUS_MAX_SIZE == ops.CONSENSUS_MAX_SIZE == 64 and cs.GRAPH_BUDGET_BYTES == 1 << 30
    assert ops.CONSENSUS_TILE * 6 * 4 <= 32 * 1024 and ops.CONSENSUS_TILE % 128 == 0
    assert 'consensus.hip' in build.SOURCES and '-ffp-contract=off' in build.EXTRA_FLAGS['consensus.hip']
    for symbol in ('hfl_consensus_graph', 'hfl_consensus_poses'):
        assert symbol in _native.SIGNATURES
    assert GR.ESTIMATORS == ('ransac', 'consensus')


def test_tiles_and_word_offsets():
    r = ops.CONSENSUS_ROWS
    tiles, off = ops.consensus_tiles([0, 1, r, r + 1, 0])
    assert off.tolist() == [0, 0, 1, 2, 4, 4]
    assert tiles.tolist() == [[1, 0], [2, 1], [3, r + 1], [3, 2 * r + 1]]
    word_off, row_words = ops.consensus_words([0, 1, 128, 129, 10000])
    assert row_words.tolist() == [0, 4, 4, 8, 316]                     # whole 128-bit groups
    assert word_off.tolist() == [0, 0, 4, 4 + 512, 4 + 512 + 1032, 4 + 512 + 1032 + 3160000]
    assert 4 * 3160000 == 12640000                                     # the 12.6 MB of a pair of 10 000


def test_exact_case_against_the_hand_values():
    src, dst, rows, true = sc.exact_case()
    want = cc.exact_expected()
    poses, valid, seeds, members, support, degree, ratios = hfl.consensus_hypotheses_host(
        [src], [dst], [rows], distance_threshold=cc.EXACT_DISTANCE, return_details=True)
    assert poses.shape == (1, cc.SEEDS, 3, 4) and poses.dtype == np.float32 and valid.dtype == bool
    assert seeds.dtype == members.dtype == support.dtype == np.int64 and degree[0].dtype == np.int32
    assert np.array_equal(degree[0], want['degree']) and np.array_equal(seeds[0], want['seeds'])
    assert np.array_equal(valid[0], want['valid']) and np.array_equal(members[0], want['members'])
    assert np.array_equal(support[0], want['support'])
    assert valid[0].sum() == 16 and (seeds[0, 40:] == -1).all() and np.isnan(poses[0][~valid[0]]).all()
    assert np.isnan(ratios[0][~valid[0]]).all() and (ratios[0][valid[0]] > 1e-3).all()
    # every valid hypothesis is the 90 degree turn and the shift (1, 2, 3), exactly: integers throughout
    turn = np.array([[0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3]], np.float32)
    assert np.abs(poses[0][valid[0]] - turn).max() <= 2.0 ** -20
    # the graph itself
    graph = cs._host_graph(src, dst, np.float32(cc.EXACT_DISTANCE))
    assert np.array_equal(graph, true[:, None] & true[None, :] & ~np.eye(true.shape[0], dtype=bool))


def test_graph_degree_and_second_order_counts_against_the_dense_float64_construction():
    d32 = np.float32(cc.DISTANCE)
    host = cc.host_ragged()
    for i, (src, dst, rows) in enumerate(zip(*cc.ragged_batch())):
        n_corr = rows.shape[0]
        cc.guard_lengths(src, dst, rows, cc.DISTANCE)                  # excludes nothing: it is an assertion on the fixture
        graph, degree, second = cc.dense_graph(src, dst, rows, cc.DISTANCE)
        got = cs._host_graph(src[rows[:, 0]], dst[rows[:, 1]], d32) if n_corr else np.zeros((0, 0), bool)
        assert np.array_equal(got, graph) and np.array_equal(got, got.T) and not got.diagonal().any(), n_corr
        assert np.array_equal(host[5][i], degree) and host[5][i].dtype == np.int32, n_corr
        # seeds: (degree descending, index ascending); sets: the largest n_sj >= 1, the lower j of equal ones
        used = min(cc.SEEDS, n_corr)
        order = sorted(range(n_corr), key=lambda c: (-int(degree[c]), c))[:used]
        assert host[2][i, :used].tolist() == order and (host[2][i, used:] == -1).all(), n_corr
        for h, s in enumerate(order):
            partners = sorted((j for j in range(n_corr) if second[s, j] >= 1), key=lambda j: (-int(second[s, j]), j))[:cc.SIZE - 1]
            if host[1][i, h]:
                assert host[3][i, h, :len(partners) + 1].tolist() == sorted(partners + [s]), (n_corr, h)
                assert (host[3][i, h, len(partners) + 1:] == -1).all()
                assert host[4][i, h] == min(int(second[s, j]) for j in partners)
            else:
                assert len(partners) + 1 < 3 or not host[6][i, h] > reg.RANK_TOL, (n_corr, h)
                assert (host[3][i, h] == -1).all() and host[4][i, h] == 0 and np.isnan(host[0][i, h]).all()
    valid = host[1]
    assert not valid[:4].any() and valid[4:, 0].all()                  # C = 0 .. 3 with 30 % wrong rows: nothing to agree on


def test_poses_are_the_kabsch_solution_of_their_sets():
    """a float64 SVD Kabsch on the members, no package code: the pose of every firm set within 1e-6 of it"""
    host = cc.host_ragged()
    checked = 0
    for i, (src, dst, rows) in enumerate(zip(*cc.ragged_batch())):
        for h in np.nonzero(host[1][i] & (host[6][i] > 1e-3))[0][:8]:
            mem = host[3][i, h][host[3][i, h] >= 0]
            p, q = src[rows[mem, 0]].astype(np.float64), dst[rows[mem, 1]].astype(np.float64)
            u, _, vt = np.linalg.svd((p - p.mean(0)).T @ (q - q.mean(0)))
            r = vt.T @ np.diag([1.0, 1.0, np.sign(np.linalg.det(vt.T @ u.T))]) @ u.T
            t = q.mean(0) - r @ p.mean(0)
            assert np.abs(host[0][i, h] - np.concatenate([r, t[:, None]], 1)).max() <= 1e-6 * max(1.0, np.abs(t).max())
            checked += 1
    assert checked > 50


def test_options_and_limits_are_refused():
    src, dst, rows = gc.corrupted(0.6)
    for host in (hfl.consensus_hypotheses_host, hfl.consensus_registration_host):
        for kw in (dict(distance_threshold=0.0), dict(distance_threshold=-1.0), dict(distance_threshold=np.nan),
                   dict(distance_threshold=np.inf), dict(distance_threshold=1e-50), dict(seeds=0), dict(seeds=2.5),
                   dict(consensus_size=2), dict(consensus_size=65), dict(consensus_size=9.5)):
            with pytest.raises(ValueError):
                host([src], [dst], [rows], **kw)
        with pytest.raises(ValueError):
            host([src, src], [dst], [rows, rows])                      # the clouds do not pair up
        with pytest.raises(ValueError):
            host([src], [dst], rows)                                   # neither a list nor a (rows, offsets) tuple
        with pytest.raises(TypeError):
            host([src], [dst], [rows.astype(np.float32)])
        with pytest.raises(ValueError):
            host([src], [dst], [np.array([[0, dst.shape[0]]])])        # a row outside its cloud
    for kw in (dict(max_correspondence_distance=-1.0), dict(refine_iterations=-1), dict(min_correspondences=-1)):
        with pytest.raises(ValueError):
            hfl.consensus_registration_host([src], [dst], [rows], **kw)
    # the two limits, before anything is built: one pair too long; a batch whose bit matrices pass 1 GiB (32 MiB each)
    long_rows = np.zeros((cs.CONSENSUS_MAX_CORRESPONDENCES + 1, 2), np.int64)
    with pytest.raises(ValueError, match='at most 16384'):
        hfl.consensus_hypotheses_host([src], [dst], [long_rows])
    many = 33
    with pytest.raises(ValueError, match='split the batch'):
        hfl.consensus_registration_host([src] * many, [dst] * many, [long_rows[:-1]] * many)
    assert ops.consensus_words([cs.CONSENSUS_MAX_CORRESPONDENCES] * 32)[0][-1] * 4 == cs.GRAPH_BUDGET_BYTES   # 32 still fit
    with pytest.raises(_native.NativeLibraryError):
        hfl.consensus_hypotheses([src], [dst], [rows])                 # CPU clouds on the device route
    with pytest.raises(_native.NativeLibraryError):
        hfl.consensus_registration([src], [dst], [rows])
    for name in ('global_registration_host', 'global_registration'):
        with pytest.raises(ValueError, match='estimator'):
            getattr(hfl, name)([src], [dst], estimator='teaser')
    queries, database, cand = sc.rerank_inputs()
    for name in ('rerank_candidates_host', 'rerank_candidates'):
        with pytest.raises(ValueError, match='estimator'):
            getattr(hfl, name)(queries, database, cand, estimator='teaser')


def test_the_ragged_batch_equals_the_single_pairs_and_the_packed_form_the_lists():
    sizes = (0, 2, 3, 33, 129, 513)
    batch = cc.ragged_batch(sizes)
    kw = dict(distance_threshold=cc.DISTANCE, seeds=40, consensus_size=7, return_details=True)
    whole = hfl.consensus_hypotheses_host(*batch, **kw)
    for i in range(len(sizes)):
        one = hfl.consensus_hypotheses_host([batch[0][i]], [batch[1][i]], [batch[2][i]], **kw)
        for k in (0, 1, 2, 3, 4, 6):
            assert np.array_equal(one[k][0], whole[k][i], equal_nan=True), (sizes[i], k)
        assert np.array_equal(one[5][0], whole[5][i])
    off = np.cumsum([0] + [r.shape[0] for r in batch[2]])
    cat = lambda parts: (np.concatenate(parts), np.cumsum([0] + [p.shape[0] for p in parts]))          # noqa: E731
    packed = hfl.consensus_hypotheses_host(cat(batch[0]), cat(batch[1]), (np.concatenate(batch[2]), off), **kw)
    for k in (0, 1, 2, 3, 4, 6):
        assert np.array_equal(packed[k], whole[k], equal_nan=True), k
    assert np.array_equal(packed[5], np.concatenate(whole[5])) and packed[5].dtype == np.int32
    reg_kw = dict(distance_threshold=cc.DISTANCE, max_correspondence_distance=gc.TAU)
    lists = hfl.consensus_registration_host(*batch, **reg_kw)
    both = hfl.consensus_registration_host(cat(batch[0]), cat(batch[1]), (np.concatenate(batch[2]), off), **reg_kw)
    for a, b in zip(lists, both):
        assert np.array_equal(a, b, equal_nan=True)
    assert lists.status.tolist() == [GR.NO_HYPOTHESIS] * 3 + [reg.MAX_ITERATIONS] * 3
    assert lists.hypothesis[:3].tolist() == [-1] * 3 and lists.valid_hypotheses[:3].tolist() == [0] * 3
    assert np.array_equal(lists.transforms[1], np.eye(4)) and lists.fitness[1] == 0.0 and np.isnan(lists.inlier_rmse[1])


def test_registration_is_the_tail_of_ransac_registration_on_the_consensus_poses():
    src, dst, rows = gc.corrupted(0.9)
    poses, valid, _ = hfl.consensus_hypotheses_host([src], [dst], [rows], distance_threshold=cc.DISTANCE)
    assert np.array_equal(valid, np.isfinite(poses).all((2, 3)))       # NaN exactly where invalid: the hook's own rule
    given = hfl.ransac_registration_host([src], [dst], [rows], poses=poses, max_correspondence_distance=gc.TAU)
    for a, b in zip(cc.host_purpose(0.9), given):
        assert np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize('frac', cc.PURPOSE_FRACTIONS)
def test_purpose_consensus_finds_the_pose_where_drawn_triples_do_not(frac):
    src, dst, rows = gc.corrupted(frac)
    n_true = int(gc.true_rows(frac).sum())
    res = cc.host_purpose(frac)
    angle, shift = gc.pose_error(res.transforms[0])
    print('frac %.2f, %d true rows: consensus %.3g degrees, %.3g m, %d inliers, slot %d'
          % (frac, n_true, angle, shift, res.inliers[0], res.hypothesis[0]))
    assert angle < gc.ANGLE_TOL_DEG and shift < gc.SHIFT_TOL
    assert res.inliers.tolist() == [n_true] and res.status.tolist() == [reg.MAX_ITERATIONS]
    if frac in cc.RANSAC_FAILS_AT:
        ransac = hfl.ransac_registration_host([src], [dst], [rows], max_correspondence_distance=gc.TAU, hypotheses=4096, seed=0)
        r_angle, r_shift = gc.pose_error(ransac.transforms[0])
        print('    random triples, 4 096: %.3g degrees, %.3g m, %d inliers' % (r_angle, r_shift, ransac.inliers[0]))
        assert not (r_angle < gc.ANGLE_TOL_DEG and r_shift < gc.SHIFT_TOL)


@pytest.mark.parametrize('estimation', sorted(GLOBAL_BOUNDS))
def test_purpose_two_raw_clouds_in_one_call_by_consensus(estimation):
    src, dst = gc.clouds()
    coarse, fine = hfl.global_registration_host([src], [dst], estimation=estimation, estimator='consensus')
    angle, shift = gc.pose_error(fine.transforms[0])
    print('coarse %.3g degrees %.3g m (slot %d, %d inliers), fine %.3g degrees %.3g m'
          % (gc.pose_error(coarse.transforms[0]) + (coarse.hypothesis[0], coarse.inliers[0], angle, shift)))
    assert coarse.status.tolist() == [reg.MAX_ITERATIONS] and fine.status.tolist() == [reg.CONVERGED]
    assert angle <= GLOBAL_BOUNDS[estimation][0] and shift <= GLOBAL_BOUNDS[estimation][1]


def test_the_default_estimator_is_the_call_without_the_keyword():
    src, dst = gc.clouds()
    small = ([src[:300]], [dst[:300]])
    for a, b in zip(hfl.global_registration_host(*small, hypotheses=256),
                    hfl.global_registration_host(*small, hypotheses=256, estimator='ransac', consensus_distance=0.1, seeds=3,
                                                 consensus_size=5)):
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True)
    plain = sc.host_rerank(register=True)
    named = hfl.rerank_candidates_host(*sc.rerank_inputs(), register=True, estimator='ransac')
    for a, b in zip(plain, named):
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True)


def test_rerank_with_registration_by_consensus():
    ranked, coarse, fine = hfl.rerank_candidates_host(*sc.rerank_inputs(), register=True, estimator='consensus')
    assert np.array_equal(ranked.indices, sc.host_rerank().indices) and np.array_equal(ranked.scores, sc.host_rerank().scores)
    angle, shift = gc.pose_error(fine.transforms[0], sc.rerank_truth())
    print('coarse %.3g degrees %.3g m, fine %.3g degrees %.3g m'
          % (gc.pose_error(coarse.transforms[0], sc.rerank_truth()) + (angle, shift)))
    assert angle <= GLOBAL_BOUNDS['point_to_plane'][0] and shift <= GLOBAL_BOUNDS['point_to_plane'][1]
