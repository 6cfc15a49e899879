"""Consensus registration on the device (`csrc/consensus.hip`, `hotformerloc_amd/consensus.py`) against the numpy twins of the
same module.

Comparison rule.  Degrees, seeds, flags, members and supports: EQUAL, with no guard -- they are integer or boolean functions of
singly rounded fp32 operations.  Poses: NaN exactly where invalid; on firm sets (the host solver's rank ratio above 1e-3)
within 2^-23 max(1, max |t|) per entry, the rule of `test_hypotheses_of_a_ragged_batch`; the file is built without
contraction and follows numpy operation for operation, so bit equality is expected and its share is printed.  A second run
equals the first and a pair alone equals the pair in a batch, bit for bit, poses included.  The whole call: against
`ransac_registration_host` on the DEVICE's poses (the consensus call is that tail on its own candidates), by the rule of
`tests/test_gpu_global_registration.py` and under its d2 guard.  Re-ranking: order and indices equal the host's; the scores
are those of `spectral_consistency`, which this estimator does not touch -- bit for bit those of the default estimator on
the device, and against the host within the 1e-5 `test_rerank_on_the_device` holds them to.  Shapes: a word, a 128-bit
group, a workgroup's rows and an LDS tile with both neighbours each; S and k1 round their limits."""
import numpy as np
import pytest
import torch

import hotformerloc_amd as hfl
from hotformerloc_amd import _native
from hotformerloc_amd import registration as reg
from tests import consensus_cases as cc
from tests import global_registration_cases as gc
from tests import spectral_cases as sc
from tests.test_gpu_global_registration import (GLOBAL_BOUNDS, assert_result_of_the_host, batch_of, dev, guarded_counts,
                                                  on_device)

pytestmark = pytest.mark.gpu

GR = gc.GR


def details(on, **kw):
    """`consensus_hypotheses(return_details=True)` as numpy: (poses, valid, seeds, members, support, [degree per pair])"""
    out = hfl.consensus_hypotheses(*on, return_details=True, **kw)
    assert all(t.is_cuda for t in out[:5]) and all(t.is_cuda for t in out[5])
    assert out[0].dtype == torch.float32 and out[1].dtype == torch.bool and out[5][0].dtype == torch.int32
    assert out[2].dtype == out[3].dtype == out[4].dtype == torch.int64
    return tuple(t.cpu().numpy() for t in out[:5]) + ([t.cpu().numpy() for t in out[5]],)


def assert_hypotheses_of_the_host(got, host, label):
    """the rule of the module docstring; `host` with its rank ratios"""
    poses, valid, seeds, members, support, degree = got
    for name, a, b in (('seeds', seeds, host[2]), ('valid', valid, host[1]), ('members', members, host[3]),
                       ('support', support, host[4])):
        assert a.shape == b.shape and np.array_equal(a, b), '%s: %s differ' % (label, name)
    assert len(degree) == len(host[5]) and all(np.array_equal(a, b) for a, b in zip(degree, host[5])), '%s: degree' % label
    assert poses.shape == host[0].shape and np.isnan(poses[~valid]).all() and np.isfinite(poses[valid]).all()
    firm = valid & (host[6] > 1e-3)
    if firm.any():
        bound = 2.0 ** -23 * np.maximum(1.0, np.abs(host[0][firm][:, :, 3]).max(1))[:, None, None]
        worst = (np.abs(poses[firm].astype(np.float64) - host[0][firm]) / bound).max()
        print('%s: %d of %d firm poses bit-equal (%d valid), largest |dpose| %.3g of the bound'
              % (label, int((poses[firm] == host[0][firm]).all((1, 2)).sum()), int(firm.sum()), int(valid.sum()), worst))
        assert worst <= 1.0


def assert_same_bits(a, b):
    for x, y in zip(a[:5], b[:5]):
        assert np.array_equal(x, y, equal_nan=True)
    assert all(np.array_equal(x, y) for x, y in zip(a[5], b[5]))


def test_ragged_batch_and_single_pairs():
    batch = cc.ragged_batch()
    on = on_device(batch)
    kw = dict(distance_threshold=cc.DISTANCE)
    got = details(on, **kw)
    host = cc.host_ragged()
    assert got[0].shape == (len(cc.C_SIZES), cc.SEEDS, 3, 4) and got[3].shape == (len(cc.C_SIZES), cc.SEEDS, cc.SIZE)
    assert_hypotheses_of_the_host(got, host, 'ragged batch')
    assert not got[1][:4].any() and got[1][4:, 0].all()
    assert_same_bits(got, details(on, **kw))                           # two runs, the same bits
    plain = hfl.consensus_hypotheses(*on, **kw)                        # without details: the first three, the same bits
    assert len(plain) == 3 and all(np.array_equal(p.cpu().numpy(), g, equal_nan=True) for p, g in zip(plain, got))
    for i, n_corr in enumerate(cc.C_SIZES):                            # a pair alone: the same bits
        one = details(([on[0][i]], [on[1][i]], [on[2][i]]), **kw)
        for k in range(5):
            assert np.array_equal(one[k][0], got[k][i], equal_nan=True), (n_corr, k)
        assert np.array_equal(one[5][0], got[5][i]), n_corr


def test_packed_layout():
    batch = cc.ragged_batch((3, 0, 129, 513))
    on = on_device(batch)
    lists = details(on, distance_threshold=cc.DISTANCE)
    off = np.cumsum([0] + [r.shape[0] for r in batch[2]])
    cat = lambda parts: (torch.cat(parts, 0), np.cumsum([0] + [int(p.shape[0]) for p in parts]))       # noqa: E731
    packed = hfl.consensus_hypotheses(cat(on[0]), cat(on[1]), (torch.cat(on[2], 0), off), distance_threshold=cc.DISTANCE,
                                      return_details=True)
    for k in range(5):
        assert np.array_equal(packed[k].cpu().numpy(), lists[k], equal_nan=True), k
    assert np.array_equal(packed[5].cpu().numpy(), np.concatenate(lists[5]))


@pytest.mark.parametrize('n_corr', (700, 40))
@pytest.mark.parametrize('seeds', cc.S_SIZES)
def test_seed_counts(seeds, n_corr):
    on = on_device(cc.ragged_batch((n_corr,)))
    got = details(on, distance_threshold=cc.DISTANCE, seeds=seeds)
    assert_hypotheses_of_the_host(got, cc.host_sized((n_corr,), seeds, cc.SIZE), 'S = %d, C = %d' % (seeds, n_corr))
    used = min(seeds, n_corr)                                          # S > C leaves slots unused
    assert (got[2][0, :used] >= 0).all() and (got[2][0, used:] == -1).all() and not got[1][0, used:].any()
    assert len(set(got[2][0, :used].tolist())) == used


@pytest.mark.parametrize('size', cc.K_SIZES)
def test_consensus_sizes(size):
    sizes = (700, 40, 2)
    on = on_device(cc.ragged_batch(sizes))
    got = details(on, distance_threshold=cc.DISTANCE, consensus_size=size)
    assert_hypotheses_of_the_host(got, cc.host_sized(sizes, cc.SEEDS, size), 'k1 = %d' % size)
    assert (got[3][0] >= 0).sum(1).max() == size and got[3].shape[2] == size and not got[1][2].any()


def test_exact_case_matches_the_hand_values():
    src, dst, rows, _ = sc.exact_case()
    want = cc.exact_expected()
    poses, valid, seeds, members, support, degree = details(([dev(src)], [dev(dst)], [dev(rows)]),
                                                            distance_threshold=cc.EXACT_DISTANCE)
    assert np.array_equal(degree[0], want['degree']) and np.array_equal(seeds[0], want['seeds'])
    assert np.array_equal(valid[0], want['valid']) and np.array_equal(members[0], want['members'])
    assert np.array_equal(support[0], want['support']) and np.isnan(poses[0][~valid[0]]).all()
    turn = np.array([[0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3]], np.float32)
    assert np.abs(poses[0][valid[0]] - turn).max() <= 2.0 ** -20
    host = hfl.consensus_hypotheses_host([src], [dst], [rows], distance_threshold=cc.EXACT_DISTANCE)
    print('exact case: %d of 16 poses bit-equal' % int((poses[0][valid[0]] == host[0][0][valid[0]]).all((1, 2)).sum()))


def compare_whole_call(batch, **kw):
    """`consensus_registration` against the host's score, select and polish on the device's own poses"""
    on = on_device(batch)
    poses, valid, _ = hfl.consensus_hypotheses(*on, distance_threshold=cc.DISTANCE)
    res = hfl.consensus_registration(*on, distance_threshold=cc.DISTANCE, max_correspondence_distance=gc.TAU, **kw)
    again = hfl.consensus_registration(*on, distance_threshold=cc.DISTANCE, max_correspondence_distance=gc.TAU, **kw)
    for a, b in zip(res, again):
        assert np.array_equal(a, b, equal_nan=True)                    # two runs, the same bits
    counts = guarded_counts(batch, poses.cpu().numpy(), valid.cpu().numpy(), gc.TAU)
    host = hfl.ransac_registration_host(*batch, poses=poses.cpu().numpy(), max_correspondence_distance=gc.TAU, **kw)
    assert_result_of_the_host(res, host)
    assert np.array_equal(res.hypothesis, np.where(counts.max(1) >= 0, counts.argmax(1), -1))
    assert np.array_equal(res.valid_hypotheses, valid.cpu().numpy().sum(1))
    return res


def test_whole_call_with_an_empty_pair_in_the_middle_and_a_pair_of_two():
    src, dst, rows = gc.corrupted(0.6)
    more = batch_of((0, 2, 1025), frac=0.5)
    batch = ([src] + more[0], [dst] + more[1], [rows] + more[2])
    res = compare_whole_call(batch)
    assert res.status.tolist() == [reg.MAX_ITERATIONS, GR.NO_HYPOTHESIS, GR.NO_HYPOTHESIS, reg.MAX_ITERATIONS]
    for i in (1, 2):                                                   # no correspondence; two of them: no set of three
        assert np.array_equal(res.transforms[i], np.eye(4)) and res.fitness[i] == 0.0 and np.isnan(res.inlier_rmse[i])
        assert res.hypothesis[i] == -1 and res.hypothesis_inliers[i] == -1 and res.valid_hypotheses[i] == 0
    hyp = details(on_device(batch), distance_threshold=cc.DISTANCE)
    assert (hyp[2][1] == -1).all() and not hyp[1][1].any() and hyp[5][1].shape == (0,)
    assert hyp[2][2, :2].tolist() == [0, 1] and (hyp[2][2, 2:] == -1).all() and not hyp[1][2].any()


def test_whole_call_too_few_and_no_refinement():
    res = compare_whole_call(batch_of((3, 40), frac=0.0), min_correspondences=4, refine_iterations=0)
    assert res.status.tolist() == [reg.TOO_FEW, reg.MAX_ITERATIONS]


@pytest.mark.parametrize('frac', cc.RANSAC_FAILS_AT)
def test_purpose_ninety_five_and_more_percent_wrong_correspondences(frac):
    src, dst, rows = gc.corrupted(frac)
    res = hfl.consensus_registration([dev(src)], [dev(dst)], [dev(rows)], distance_threshold=cc.DISTANCE, seeds=cc.SEEDS,
                                     consensus_size=cc.SIZE, max_correspondence_distance=gc.TAU)
    angle, shift = gc.pose_error(res.transforms[0])
    print('frac %.2f: pose error %.3g degrees, %.3g m, %d inliers, slot %d' % (frac, angle, shift, res.inliers[0], res.hypothesis[0]))
    assert angle < gc.ANGLE_TOL_DEG and shift < gc.SHIFT_TOL
    assert res.inliers.tolist() == [int(gc.true_rows(frac).sum())]
    host = cc.host_purpose(frac)
    assert np.array_equal(res.hypothesis, host.hypothesis) and np.array_equal(res.inliers, host.inliers)


@pytest.mark.parametrize('estimation', sorted(GLOBAL_BOUNDS))
def test_two_raw_clouds_in_one_call_by_consensus(estimation):
    src, dst = gc.clouds()
    coarse, fine = hfl.global_registration([dev(src)], [dev(dst)], estimation=estimation, estimator='consensus')
    h_coarse, h_fine = hfl.global_registration_host([src], [dst], estimation=estimation, estimator='consensus')
    angle, shift = gc.pose_error(fine.transforms[0])
    print('coarse %.3g degrees %.3g m, fine %.3g degrees %.3g m; host fine %.3g degrees %.3g m'
          % (gc.pose_error(coarse.transforms[0]) + (angle, shift) + gc.pose_error(h_fine.transforms[0])))
    assert coarse.status.tolist() == h_coarse.status.tolist() == [reg.MAX_ITERATIONS]
    assert fine.status.tolist() == h_fine.status.tolist() == [reg.CONVERGED]
    assert coarse.hypothesis.tolist() == h_coarse.hypothesis.tolist() and coarse.inliers.tolist() == h_coarse.inliers.tolist()
    assert angle <= GLOBAL_BOUNDS[estimation][0] and shift <= GLOBAL_BOUNDS[estimation][1]


def test_rerank_with_registration_by_consensus():
    queries, database, cand = sc.rerank_inputs()
    on = ([dev(c) for c in queries], [dev(c) for c in database], dev(cand))
    ranked, coarse, fine = hfl.rerank_candidates(*on, register=True, estimator='consensus')
    host, h_coarse, h_fine = hfl.rerank_candidates_host(queries, database, cand, register=True, estimator='consensus')
    assert np.array_equal(ranked.indices.cpu().numpy(), host.indices) and np.array_equal(ranked.order.cpu().numpy(), host.order)
    plain = hfl.rerank_candidates(*on)
    assert torch.equal(ranked.scores, plain.scores) and torch.equal(ranked.indices, plain.indices)
    print('largest |score - host score| %.3g' % np.abs(ranked.scores.cpu().numpy() - host.scores).max())
    assert np.abs(ranked.scores.cpu().numpy() - host.scores).max() <= 1e-5
    assert coarse.status.tolist() == h_coarse.status.tolist() and coarse.hypothesis.tolist() == h_coarse.hypothesis.tolist()
    angle, shift = gc.pose_error(fine.transforms[0], sc.rerank_truth())
    print('coarse %.3g degrees %.3g m, fine %.3g degrees %.3g m; host fine %.3g degrees %.3g m'
          % (gc.pose_error(coarse.transforms[0], sc.rerank_truth()) + (angle, shift)
             + gc.pose_error(h_fine.transforms[0], sc.rerank_truth())))
    assert angle <= GLOBAL_BOUNDS['point_to_plane'][0] and shift <= GLOBAL_BOUNDS['point_to_plane'][1]


def test_cpu_tensors_and_limits_are_refused():
    src, dst, rows = gc.corrupted(0.6)
    for call in (hfl.consensus_hypotheses, hfl.consensus_registration):
        with pytest.raises(_native.NativeLibraryError):
            call([torch.from_numpy(src.copy())], [torch.from_numpy(dst.copy())], [dev(rows)])
        with pytest.raises(ValueError, match='at most 16384'):
            call([dev(src)], [dev(dst)], [torch.zeros((16385, 2), dtype=torch.int64, device='cuda')])
        with pytest.raises(ValueError):
            call([dev(src)], [dev(dst)], [dev(rows)], consensus_size=65)
    with pytest.raises(_native.NativeLibraryError):
        hfl.global_registration([torch.from_numpy(src.copy())], [dev(dst)], estimator='consensus')
