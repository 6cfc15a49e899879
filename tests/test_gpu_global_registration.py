"""Global registration on the device (`csrc/global_registration.hip`, `hotformerloc_amd/global_registration.py`) against the
numpy twins of the same module.

Comparison rule.  Draws: EQUAL (integer arithmetic).  Flags: equal under the guard of `tests/global_registration_cases.py`
(no edge or rank ratio of a drawn triple within 1e-9 relative of its threshold).  Poses of hypotheses whose rank ratio
exceeds 1e-3: within 2^-23 max(1, |t|) per entry; the file is built without contraction and follows numpy operation for
operation, so bit equality is expected and its share is printed.  Counts: EQUAL to the host's counts on the DEVICE's poses,
under the guard that no host d2 lies within 4 fp32 ulps of D2.  The whole call: integers and statuses equal, fitness equal,
the float64 pose within 1e-9 (the same sums in another order), rmse within 1e-6 absolute (the bound of
`tests/test_gpu_registration.py`).  Shapes: R = ops.RANSAC_ROWS hypotheses and T = ops.RANSAC_TILE correspondences per
workgroup, and every size around them."""
import numpy as np
import pytest
import torch

import hotformerloc_amd as hfl
from hotformerloc_amd import ops
from hotformerloc_amd import registration as reg
from tests import global_registration_cases as gc

pytestmark = pytest.mark.gpu

GR = gc.GR
R, T = ops.RANSAC_ROWS, ops.RANSAC_TILE
H_SIZES = (1, R - 1, R, R + 1, 2 * R + 1)
C_SIZES = (1, T - 1, T, T + 1, 2 * T + 1)
# `global_registration_host` on 'planes' against 'planes_moved' reaches, of the truth, 9.55e-07 degrees and 1.21e-07 m with
# the point-to-plane ICP and 9.47e-07 degrees and 1.65e-07 m with the point-to-point one on the CPU (the fp32 rounding of the
# moved cloud); the device may take twice that.  The point-to-point ICP from the identity ends 22.2 degrees and 1.88 m off.
GLOBAL_BOUNDS = {'point_to_plane': (2 * 9.55e-07, 2 * 1.21e-07), 'point_to_point': (2 * 9.47e-07, 2 * 1.65e-07)}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def batch_of(counts, frac=0.3, seed=5):
    """(sources, targets, rows) numpy lists: the two plane clouds with `counts[i]` correspondences each"""
    src, dst = gc.clouds()
    return [src] * len(counts), [dst] * len(counts), [gc.rows(c, frac, seed + i) for i, c in enumerate(counts)]


def on_device(batch):
    return [dev(c) for c in batch[0]], [dev(c) for c in batch[1]], [dev(r) for r in batch[2]]


def guarded_counts(batch, poses, valid, tau):
    """the host counts on the given poses, with the d2 guard asserted pair by pair"""
    for src, dst, rows, m in zip(*batch, poses):
        gc.guard_d2(*gc.gathered(src, dst, rows), m.reshape(-1, 12), tau)
    return hfl.score_hypotheses_host(*batch, poses, tau, valid)


@pytest.mark.parametrize('n_hyp', H_SIZES)
def test_hypotheses_of_a_ragged_batch(n_hyp):
    batch = batch_of((0, 1, 2, 3, 700))
    poses, valid, draws = (t.cpu().numpy() for t in hfl.ransac_hypotheses(*on_device(batch), hypotheses=n_hyp, seed=11))
    h_poses, h_valid, h_draws = hfl.ransac_hypotheses_host(*batch, hypotheses=n_hyp, seed=11)
    assert poses.shape == (5, n_hyp, 3, 4) and poses.dtype == np.float32 and valid.dtype == bool and draws.dtype == np.int32
    assert np.array_equal(draws, h_draws)
    for src, dst, rows, d in zip(*batch, h_draws):
        gc.guard_draws(*gc.gathered(src, dst, rows), d)
    assert np.array_equal(valid, h_valid)
    assert not valid[:3].any() and (n_hyp < R or valid[4].any())
    assert np.isnan(poses[~valid]).all()
    ratios = np.stack([gc.rank_ratios(*gc.gathered(src, dst, rows), d) for src, dst, rows, d in zip(*batch, h_draws)])
    firm = valid & (ratios > 1e-3)
    if firm.any():
        bound = 2.0 ** -23 * np.maximum(1.0, np.abs(h_poses[firm][:, :, 3]).max(1))[:, None, None]
        assert (np.abs(poses[firm].astype(np.float64) - h_poses[firm]) <= bound).all()
        print('H = %d: %d of %d firm poses bit-equal' % (n_hyp, int((poses[firm] == h_poses[firm]).all((1, 2)).sum()),
                                                          int(firm.sum())))


def score_case(counts, n_hyp, tau=gc.TAU):
    batch = batch_of(counts)
    on = on_device(batch)
    poses, valid, _ = hfl.ransac_hypotheses(*on, hypotheses=n_hyp, seed=3)
    got = hfl.score_hypotheses(*on, poses, tau, valid)
    again = hfl.score_hypotheses(*on, poses, tau, valid)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(counts), n_hyp)
    assert torch.equal(got, again)                                     # two runs, the same bits
    host = guarded_counts(batch, poses.cpu().numpy(), valid.cpu().numpy(), tau)
    assert torch.equal(got.cpu(), torch.from_numpy(host))
    assert (got.cpu()[~valid.cpu()] == -1).all() and (got.cpu()[valid.cpu()] >= 0).all()
    return got.cpu().numpy(), valid.cpu().numpy()


@pytest.mark.parametrize('n_corr', C_SIZES)
def test_score_correspondence_sizes(n_corr):
    got, valid = score_case((n_corr,), R + 1)
    assert n_corr < 3 or (valid.any() and got.max() > 0.5 * n_corr)    # C = 2T + 1: three workgroups add to one count


@pytest.mark.parametrize('n_hyp', H_SIZES)
def test_score_hypothesis_sizes(n_hyp):
    score_case((T + 1,), n_hyp)


def test_score_batch_with_an_empty_pair_in_the_middle():
    got, valid = score_case((700, 0, T + 1), R + 1)
    assert not valid[1].any() and valid[0].any() and valid[2].any()
    # without flags a finite pose is valid: the empty pair then scores 0, not -1
    batch = batch_of((700, 0, T + 1))
    on = on_device(batch)
    poses = torch.zeros((3, 4, 3, 4), dtype=torch.float32, device='cuda')
    poses[:, 1] = float('nan')
    got = hfl.score_hypotheses(*on, poses, gc.TAU).cpu().numpy()
    assert np.array_equal(got, hfl.score_hypotheses_host(*batch, poses.cpu().numpy(), gc.TAU))
    assert got[1].tolist() == [0, -1, 0, 0]


def test_score_exact_case_matches_hand_counts():
    src, dst, rows, poses, counts = gc.exact_case()
    for name, tau in (('at', gc.EXACT_TAU), ('below', gc.EXACT_TAU_BELOW)):
        got = hfl.score_hypotheses([dev(src)], [dev(dst)], [dev(rows)], dev(poses), tau)
        assert np.array_equal(got.cpu().numpy()[0], counts[name]), name


def assert_result_of_the_host(res, host):
    """the rule of the module docstring for a whole call"""
    for name in ('hypothesis', 'hypothesis_inliers', 'inliers', 'status', 'valid_hypotheses'):
        assert getattr(res, name).dtype == np.int64
        assert np.array_equal(getattr(res, name), getattr(host, name)), name
    assert np.abs(res.transforms - host.transforms).max() <= 1e-9
    assert np.array_equal(res.fitness, host.fitness, equal_nan=True)
    assert np.array_equal(np.isnan(res.inlier_rmse), np.isnan(host.inlier_rmse))
    assert np.nanmax(np.abs(res.inlier_rmse - host.inlier_rmse), initial=0.0) <= 1e-6


def compare_whole_call(batch, n_hyp, **kw):
    on = on_device(batch)
    poses, valid, _ = hfl.ransac_hypotheses(*on, hypotheses=n_hyp)
    res = hfl.ransac_registration(*on, hypotheses=n_hyp, max_correspondence_distance=gc.TAU, **kw)
    given = hfl.ransac_registration(*on, poses=poses, max_correspondence_distance=gc.TAU, **kw)
    for a, b in zip(res, given):
        assert np.array_equal(a, b, equal_nan=True)                    # drawn or handed in: the same candidates, the same bits
    guarded_counts(batch, poses.cpu().numpy(), valid.cpu().numpy(), gc.TAU)
    host = hfl.ransac_registration_host(*batch, poses=poses.cpu().numpy(), max_correspondence_distance=gc.TAU, **kw)
    assert_result_of_the_host(res, host)
    counts = hfl.score_hypotheses(*on, poses, gc.TAU, valid).cpu().numpy()
    best = counts.argmax(1)                                            # the first of equal maxima: the lowest h
    assert np.array_equal(res.hypothesis, np.where(counts.max(1) >= 0, best, -1))
    return res


def test_whole_call_against_the_host_on_the_same_candidates():
    src, dst, rows = gc.corrupted(gc.PURPOSE['frac'])
    more = batch_of((0, 2, T + 1), frac=0.5)
    batch = ([src] + more[0], [dst] + more[1], [rows] + more[2])
    res = compare_whole_call(batch, 1024)
    assert res.status.tolist() == [reg.MAX_ITERATIONS, GR.NO_HYPOTHESIS, GR.NO_HYPOTHESIS, reg.MAX_ITERATIONS]
    assert np.array_equal(res.transforms[1], np.eye(4)) and res.fitness[1] == 0.0 and np.isnan(res.inlier_rmse[1])


def test_whole_call_too_few_and_no_refinement():
    batch = batch_of((3, 40), frac=0.0)
    res = compare_whole_call(batch, 64, min_correspondences=4, refine_iterations=0)
    assert res.status.tolist() == [reg.TOO_FEW, reg.MAX_ITERATIONS]


def polish_case(n_corr):
    """(batch, poses (1, 2, 3, 4), options, the host's result): one pair of `n_corr` correspondences, 30 % of them wrong,
    polished once from the truth rounded to fp32; the second candidate is a pose of NaNs.  min_correspondences = 0, so that
    the sums are taken and solved at any size.  The d2 guard is asserted on the handed-in pose."""
    batch = batch_of((n_corr,), frac=0.3)
    poses = np.full((1, 2, 3, 4), np.nan, np.float32)
    poses[0, 0] = gc.truth().astype(np.float32)
    kw = dict(max_correspondence_distance=gc.TAU, refine_iterations=1, min_correspondences=0)
    gc.guard_d2(*gc.gathered(batch[0][0], batch[1][0], batch[2][0]), poses[0].reshape(-1, 12), gc.TAU)
    return batch, poses, kw, hfl.ransac_registration_host(*batch, poses=poses, **kw)


@pytest.mark.parametrize('n_corr', C_SIZES)
def test_polish_correspondence_sizes(n_corr):
    """`hfl_ransac_sums` round its tile: one correspondence, a partial last tile, a whole one, one row more, three
    workgroups.  A single correspondence has H = 0: the host ends DEGENERATE after one evaluation with one inlier, and
    the device must end as the host does."""
    batch, poses, kw, host = polish_case(n_corr)
    on = on_device(batch)
    res = hfl.ransac_registration(*on, poses=dev(poses), **kw)
    again = hfl.ransac_registration(*on, poses=dev(poses), **kw)
    for a, b in zip(res, again):
        assert np.array_equal(a, b, equal_nan=True)                    # two runs, the same bits
    assert res.hypothesis.tolist() == [0] and res.valid_hypotheses.tolist() == [1]
    assert_result_of_the_host(res, host)


def test_purpose_sixty_percent_wrong_correspondences():
    src, dst, rows = gc.corrupted(gc.PURPOSE['frac'])
    res = hfl.ransac_registration([dev(src)], [dev(dst)], [dev(rows)], max_correspondence_distance=gc.TAU,
                                  hypotheses=gc.PURPOSE['hypotheses'], seed=gc.PURPOSE['ransac_seed'])
    angle, shift = gc.pose_error(res.transforms[0])
    print('pose error %.3g degrees, %.3g m' % (angle, shift))
    assert angle < gc.ANGLE_TOL_DEG and shift < gc.SHIFT_TOL
    assert res.inliers.tolist() == [int(gc.true_rows(gc.PURPOSE['frac']).sum())]


@pytest.mark.parametrize('estimation', sorted(GLOBAL_BOUNDS))
def test_purpose_two_raw_clouds_in_one_call(estimation):
    src, dst = gc.clouds()
    coarse, fine = hfl.global_registration([dev(src)], [dev(dst)], estimation=estimation)
    angle, shift = gc.pose_error(fine.transforms[0])
    print('coarse %.3g degrees %.3g m, fine %.3g degrees %.3g m' % (gc.pose_error(coarse.transforms[0]) + (angle, shift)))
    assert coarse.status.tolist() == [reg.MAX_ITERATIONS] and fine.status.tolist() == [reg.CONVERGED]
    assert angle <= GLOBAL_BOUNDS[estimation][0] and shift <= GLOBAL_BOUNDS[estimation][1]


def test_purpose_the_identity_start_fails_where_the_global_start_converges():
    """the case this exists for: the point-to-point refinement of the same pair from the identity does not get there (the
    point-to-plane one happens to on this corner of three planes, whose basin is wide; it is not asserted either way)"""
    src, dst = gc.clouds()
    blind = hfl.icp_refine([dev(src)], [dev(dst)])
    angle, shift = gc.pose_error(blind.transforms[0])
    print('from the identity: %.3g degrees, %.3g m' % (angle, shift))
    assert angle > GLOBAL_BOUNDS['point_to_point'][0] and shift > GLOBAL_BOUNDS['point_to_point'][1]
    assert angle > 1.0 and shift > 0.1
