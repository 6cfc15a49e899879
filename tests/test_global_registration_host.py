"""The definition of `hotformerloc_amd/global_registration.py` on the CPU: the numpy twins against hand-made cases, Python
integers and the pieces they are built from.  `tests/test_gpu_global_registration.py` holds the device against these twins."""
import os
import re

import numpy as np
import pytest
import torch

import hotformerloc_amd as hfl
from hotformerloc_amd import _native, augment, build, ops
from hotformerloc_amd import registration as reg
from tests import global_registration_cases as gc

GR = gc.GR
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIANGLE = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 1.0, 0.5]], np.float32)
EYE3 = np.stack([np.arange(3), np.arange(3)], 1)


def run3(src, dst, hypotheses=64, **kw):
    """the hypotheses of one pair whose three points correspond row by row"""
    poses, valid, draws = hfl.ransac_hypotheses_host([src], [dst], [EYE3], hypotheses=hypotheses, **kw)
    return poses[0], valid[0], draws[0]


def distinct(draws):
    return (draws[:, 0] != draws[:, 1]) & (draws[:, 0] != draws[:, 2]) & (draws[:, 1] != draws[:, 2])


def test_exports_and_constants_mirror_the_header():
    for name in ('correspondence_pairs', 'ransac_hypotheses', 'score_hypotheses', 'ransac_registration', 'global_registration'):
        assert callable(getattr(hfl, name)) and callable(getattr(hfl, name + '_host'))
    assert hfl.RansacResult._fields == ('transforms', 'fitness', 'inlier_rmse', 'inliers', 'hypothesis', 'hypothesis_inliers',
                                        'valid_hypotheses', 'status')
    header = open(os.path.join(ROOT, 'include', 'hotformerloc_hip.h')).read()
    for name, value in (('ROWS', ops.RANSAC_ROWS), ('TILE', ops.RANSAC_TILE), ('NO_HYPOTHESIS', GR.NO_HYPOTHESIS)):
        assert int(re.search(r'#define HFL_RANSAC_%s (\d+)' % name, header).group(1)) == value
    assert ops.RANSAC_NO_HYPOTHESIS == GR.NO_HYPOTHESIS == 5 and GR.NO_HYPOTHESIS not in range(reg.DEGENERATE + 1)
    assert ops.RANSAC_ROWS == 512 and ops.RANSAC_TILE == 1024
    assert 'global_registration.hip' in build.SOURCES
    assert '-ffp-contract=off' in build.EXTRA_FLAGS['global_registration.hip']
    for symbol in ('hfl_ransac_hypotheses', 'hfl_ransac_score', 'hfl_ransac_select', 'hfl_ransac_sums'):
        assert symbol in _native.SIGNATURES


def test_shared_headers_hold_the_one_copy():
    csrc = os.path.join(ROOT, 'hotformerloc_amd', 'csrc')
    text = {f: open(os.path.join(csrc, f)).read() for f in os.listdir(csrc) if f.endswith(('.hip', '.h'))}
    assert [f for f, t in text.items() if re.search(r'\bU4 philox4x32_10\(', t)] == ['philox.h']
    assert [f for f, t in text.items() if re.search(r'\bbool kabsch_solve\(', t)] == ['kabsch.h']
    assert [f for f, t in text.items() if re.search(r'\bvoid icp_point_row\(', t)] == ['icp_sums.h']
    assert [f for f, t in text.items() if re.search(r'\bvoid icp_reduce_partials\(', t)] == ['icp_sums.h']
    # and nobody writes the row step or the reduction out beside them
    assert [f for f, t in text.items() if re.search(r'acc\[7 \+ 3 \* a \+ b\] \+=', t)] == ['icp_sums.h']
    assert [f for f, t in text.items() if re.search(r'red\[\w+ \* \w+ \+ threadIdx\.x\]', t)] == ['icp_sums.h']


def test_ransac_tiles():
    tiles, off = ops.ransac_tiles([0, 1, 1024, 1025, 0, 2049])
    assert off.tolist() == [0, 0, 1, 2, 4, 4, 7]
    assert tiles.tolist() == [[1, 0], [2, 1], [3, 1025], [3, 2049], [5, 2050], [5, 3074], [5, 4098]]
    tiles, off = ops.ransac_tiles([0])
    assert tiles.shape == (0, 2) and off.tolist() == [0, 0]


def test_refusals():
    src, dst, pairs = gc.corrupted(0.6)
    host, call = hfl.ransac_registration_host, lambda **kw: hfl.ransac_registration_host([src], [dst], [pairs], **kw)
    for kw in (dict(hypotheses=0), dict(hypotheses=2.5), dict(seed=-1), dict(seed=2 ** 64), dict(edge_length_ratio=1.5),
               dict(edge_length_ratio=-0.1), dict(max_correspondence_distance=-1.0), dict(max_correspondence_distance=np.nan),
               dict(refine_iterations=-1), dict(min_correspondences=-1)):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError):
        host([src, src], [dst], [pairs, pairs])                       # the clouds do not pair up
    with pytest.raises(ValueError):
        host([src], [dst], [pairs, pairs])                            # nor do the correspondences
    with pytest.raises(ValueError):
        host((src, np.array([0, src.shape[0]])), (dst, np.array([0, dst.shape[0]])), (pairs, np.array([0, 5])))
    with pytest.raises(ValueError):
        host([src], [dst], [pairs[:, :1]])
    with pytest.raises(TypeError):
        host([src], [dst], [pairs.astype(np.float32)])
    with pytest.raises(TypeError):
        host([src.astype(np.float64)], [dst], [pairs])
    for bad in ([[0, dst.shape[0]]], [[-1, 0]], [[src.shape[0], 0]]):
        with pytest.raises(ValueError):
            host([src], [dst], [np.array(bad)])
    with pytest.raises(ValueError):
        call(poses=np.zeros((1, 4, 4, 4), np.float32))
    with pytest.raises(ValueError):
        call(poses=np.zeros((2, 4, 3, 4), np.float32))
    with pytest.raises(TypeError):
        call(poses=np.zeros((1, 4, 3, 4), np.float64))
    with pytest.raises(ValueError):
        hfl.score_hypotheses_host([src], [dst], [pairs], np.zeros((1, 4, 3, 4), np.float32), 0.1, valid=np.ones((1, 5), bool))
    with pytest.raises(TypeError):
        hfl.score_hypotheses_host([src], [dst], [pairs], np.zeros((1, 4, 3, 4), np.float32), 0.1, valid=np.ones((1, 4)))
    with pytest.raises(ValueError):
        hfl.global_registration_host([src], [dst, dst])
    with pytest.raises(ValueError):
        hfl.global_registration_host([src], [dst], estimation='point_to_line')


def test_device_functions_refuse_cpu_tensors():
    src, dst, pairs = gc.corrupted(0.6)
    poses = np.zeros((1, 2, 3, 4), np.float32)
    for call in (lambda: hfl.ransac_hypotheses([src], [dst], [pairs]),
                 lambda: hfl.score_hypotheses([src], [dst], [pairs], poses, 0.1),
                 lambda: hfl.ransac_registration([src], [dst], [pairs]),
                 lambda: hfl.global_registration([torch.from_numpy(src.copy())], [torch.from_numpy(dst.copy())])):
        with pytest.raises(_native.NativeLibraryError):
            call()


def test_philox_draws_and_the_sample_index_rule():
    seed = 0x123456789ABCDEF
    key = (seed & 0xFFFFFFFF, seed >> 32)
    for pair, count in ((0, 678), (3, 1), (7, 2 ** 31 - 1), (2, 0), (5, 3)):
        draws = GR._host_draws(pair, 50, count, seed)
        assert draws.dtype == np.int32 and draws.shape == (50, 3)
        for h in (0, 1, 17, 49):
            words = augment.philox4x32_10(np.array([h, pair, 0, 0], np.uint32), key)
            assert draws[h].tolist() == [(int(w) * count) >> 32 for w in words[:3]]
        assert ((draws >= 0) & (draws < max(count, 1))).all()
    src, dst = gc.clouds()
    pairs = gc.rows(700, 0.5, 3)
    _, _, draws = hfl.ransac_hypotheses_host([src, src], [dst, dst], [pairs[:10], pairs], hypotheses=20, seed=seed)
    assert np.array_equal(draws[1], GR._host_draws(1, 20, 700, seed)) and np.array_equal(draws[0], GR._host_draws(0, 20, 10, seed))
    assert not np.array_equal(GR._host_draws(0, 20, 700, seed), GR._host_draws(0, 20, 700, seed + 2 ** 32))   # the high key word


def test_d2_threshold_against_a_sweep_of_neighbouring_floats():
    for tau in (0.8, 0.05, 1.0, 2.0, 3.0, gc.EXACT_TAU, gc.EXACT_TAU_BELOW, 1e-3, 123.456, 1e-30, 0.0):
        d2 = GR.inlier_d2(tau)
        assert d2.dtype == np.float32
        near = [d2]
        for _ in range(8):
            near = [np.nextafter(near[0], np.float32(-np.inf))] + near + [np.nextafter(near[-1], np.float32(np.inf))]
        admitted = [x for x in near if x >= 0 and np.sqrt(np.float32(x)) <= np.float32(tau)]
        assert max(admitted) == d2, tau
    assert GR.inlier_d2(np.inf) == np.finfo(np.float32).max == GR.inlier_d2(1e30)
    assert GR.inlier_d2(gc.EXACT_TAU) >= 5.0 > GR.inlier_d2(gc.EXACT_TAU_BELOW)


def test_kabsch_of_many_has_the_bits_of_kabsch_of_one():
    """The array solver, and `_host_kabsch_one` row by row, against the scalar transcription of csrc/kabsch.h that stood in
    `registration.py` until the array form became the only one.  `tests/golden/kabsch_scalar.npz` holds what that scalar
    `_host_kabsch_one` (numpy float64 scalars, one Python statement per line of `kabsch_solve`) returned on the 60 rows
    built below, recorded on the last commit that had it: `solved` (60,) bool, `r` (60, 3, 3) and `t` (60, 3) float64,
    zeros where a row is not solved."""
    golden = np.load(os.path.join(ROOT, 'tests', 'golden', 'kabsch_scalar.npz'))
    rng = np.random.default_rng(5)
    sums = []
    for kind in range(60):
        p = rng.normal(0.0, 3.0, (3, 3)).astype(np.float32).astype(np.float64)
        q = rng.normal(0.0, 3.0, (3, 3)).astype(np.float32).astype(np.float64)
        if kind % 4 == 1:
            p[2] = 2.0 * p[1] - p[0]                                   # collinear
        if kind % 4 == 2:
            q = p.copy()
        if kind % 4 == 3:
            p[:, 2] = q[:, 2] = 0.0                                    # exact zeros: rotations that are skipped
        sums.append(GR._host_triple_sums([p[k:k + 1] for k in range(3)], [q[k:k + 1] for k in range(3)])[0])
    sums = np.stack(sums)
    r, t, solved = reg._host_kabsch_many(sums)
    assert solved.any() and not solved.all()
    assert golden['solved'].shape == (60,) and np.array_equal(solved, golden['solved'])
    for i in range(sums.shape[0]):
        one = reg._host_kabsch_one(sums[i])
        assert (one is not None) == bool(golden['solved'][i])
        if one is not None:
            assert np.array_equal(golden['r'][i], r[i]) and np.array_equal(golden['t'][i], t[i])
            assert np.array_equal(golden['r'][i], one[0]) and np.array_equal(golden['t'][i], one[1])


def test_fewer_than_three_correspondences():
    src, dst = gc.clouds()
    for count in (0, 1, 2):
        pairs = gc.rows(count, 0.0, 0)
        poses, valid, draws = hfl.ransac_hypotheses_host([src], [dst], [pairs], hypotheses=32)
        assert not valid.any() and np.isnan(poses).all()
        assert ((draws >= 0) & (draws <= max(count - 1, 0))).all()
        assert (hfl.score_hypotheses_host([src], [dst], [pairs], poses, 0.1, valid) == -1).all()
        res = hfl.ransac_registration_host([src], [dst], [pairs], hypotheses=32)
        assert res.status.tolist() == [GR.NO_HYPOTHESIS] and res.hypothesis.tolist() == [-1]
        assert res.hypothesis_inliers.tolist() == [-1] and res.valid_hypotheses.tolist() == [0] and res.inliers.tolist() == [0]
        assert np.array_equal(res.transforms[0], np.eye(4)) and res.fitness.tolist() == [0.0] and np.isnan(res.inlier_rmse[0])


def test_three_correspondences_repeated_rows_and_a_mirrored_triple():
    r, t = gc.fc.rotation_z()
    poses, valid, draws = run3(TRIANGLE, gc.fc.moved(TRIANGLE, r, t))
    assert np.array_equal(valid, distinct(draws)) and valid.any() and not valid.all()      # a repeated row: invalid
    assert np.isnan(poses[~valid]).all()
    for m in poses[valid].reshape(-1, 3, 4).astype(np.float64):
        assert gc.pose_error(m)[0] < 1e-4 and gc.pose_error(m)[1] < 1e-5
    res = hfl.ransac_registration_host([TRIANGLE], [gc.fc.moved(TRIANGLE, r, t)], [EYE3], hypotheses=64,
                                       max_correspondence_distance=0.01)
    assert res.status.tolist() == [reg.MAX_ITERATIONS] and res.inliers.tolist() == [3] and res.fitness.tolist() == [1.0]
    assert res.hypothesis[0] == np.nonzero(valid)[0][0] and res.valid_hypotheses[0] == valid.sum()

    mirrored = TRIANGLE * np.array([-1.0, 1.0, 1.0], np.float32)       # congruent triangles: a proper rotation maps them
    poses, valid, draws = run3(TRIANGLE, mirrored)
    assert np.array_equal(valid, distinct(draws))
    for m in poses[valid].reshape(-1, 3, 4).astype(np.float64):
        assert abs(np.linalg.det(m[:, :3]) - 1.0) < 1e-6
        assert np.abs(TRIANGLE.astype(np.float64) @ m[:, :3].T + m[:, 3] - mirrored).max() < 1e-5


def test_a_collinear_triple_is_invalid():
    line = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [2.5, 5.0, 7.5]], np.float32)
    poses, valid, draws = run3(line, line + np.float32(1.0))
    assert distinct(draws).any() and not valid.any() and np.isnan(poses).all()
    poses, valid, _ = run3(line, line + np.float32(1.0), edge_length_ratio=0.0)
    assert not valid.any()


def test_edge_length_check_on_and_off():
    small = (TRIANGLE * np.float32(0.8)).astype(np.float32)            # every edge 0.8 of its partner: below the ratio 0.9
    _, valid, draws = run3(TRIANGLE, small)
    assert distinct(draws).any() and not valid.any()
    _, valid, _ = run3(small, TRIANGLE)                                # and the other way round
    assert not valid.any()
    _, valid, draws = run3(TRIANGLE, small, edge_length_ratio=0.0)
    assert np.array_equal(valid, distinct(draws))
    _, valid, draws = run3(TRIANGLE, small, edge_length_ratio=0.75)
    assert np.array_equal(valid, distinct(draws))
    one_edge = TRIANGLE.copy()
    one_edge[2] = [0.0, 3.0, 1.5]                                      # edges (0,2) and (1,2) change, (0,1) does not
    _, valid, draws = run3(TRIANGLE, one_edge)
    assert distinct(draws).any() and not valid.any()


def test_exact_case_counts_and_the_inclusive_threshold():
    src, dst, pairs, poses, counts = gc.exact_case()
    for name, tau in (('at', gc.EXACT_TAU), ('below', gc.EXACT_TAU_BELOW)):
        got = hfl.score_hypotheses_host([src], [dst], [pairs], poses, tau)
        assert got.dtype == np.int32 and np.array_equal(got[0], counts[name]), name
    assert counts['at'][0] == 32 and counts['below'][0] == 20          # 8 and 5 of the 12 offsets, four points each
    flags = np.array([[True, False, True, True, True]])                # the caller's flags override the finiteness rule
    got = hfl.score_hypotheses_host([src], [dst], [pairs], poses, gc.EXACT_TAU, valid=flags)
    assert got[0, 1] == -1 and got[0, 0] == 32 and got[0, 4] == 0


def test_select_takes_the_lowest_of_equal_counts():
    src, dst, pairs, poses, counts = gc.exact_case()
    cand = np.ascontiguousarray(poses[:, [4, 1, 0, 2, 0]])             # NaNs, a poor one, the best one, a poor one, the best again
    res = hfl.ransac_registration_host([src], [dst], [pairs], max_correspondence_distance=gc.EXACT_TAU, poses=cand,
                                       refine_iterations=0)
    assert res.hypothesis.tolist() == [2] and res.hypothesis_inliers.tolist() == [32] and res.valid_hypotheses.tolist() == [4]
    assert res.status.tolist() == [reg.MAX_ITERATIONS] and res.inliers.tolist() == [32]
    assert np.array_equal(res.transforms[0, :3], poses[0, 0].astype(np.float64))
    assert res.fitness[0] == 32 / 48
    d2 = np.array([sum(c * c for c in o) for o in gc.EXACT_OFFSETS if sum(c * c for c in o) <= 5], np.float64)
    assert abs(res.inlier_rmse[0] - np.sqrt(4 * d2.sum() / 32)) < 1e-6


def test_too_few_and_degenerate_ends():
    r, t = gc.fc.rotation_z()
    res = hfl.ransac_registration_host([TRIANGLE], [gc.fc.moved(TRIANGLE, r, t)], [EYE3], hypotheses=64,
                                       max_correspondence_distance=0.01, min_correspondences=4)
    assert res.status.tolist() == [reg.TOO_FEW] and res.inliers.tolist() == [3] and res.fitness.tolist() == [1.0]
    assert np.isnan(res.inlier_rmse[0]) and res.hypothesis[0] >= 0
    assert gc.pose_error(res.transforms[0])[0] < 1e-4                  # the pose is the selected hypothesis

    line = (np.arange(5, dtype=np.float32)[:, None] * np.array([1.0, 2.0, 3.0], np.float32)).astype(np.float32)
    eye = np.eye(4, dtype=np.float32)[None, None, :3]
    res = hfl.ransac_registration_host([line], [line], [np.stack([np.arange(5), np.arange(5)], 1)], poses=eye,
                                       max_correspondence_distance=0.5)
    assert res.status.tolist() == [reg.DEGENERATE] and res.inliers.tolist() == [5] and res.inlier_rmse.tolist() == [0.0]
    assert np.array_equal(res.transforms[0], np.eye(4))


def test_correspondence_pairs_by_hand():
    idx = [np.array([2, -1, 0, 5], np.int32), np.zeros(0, np.int32), np.array([-1, 3], np.int32)]
    mask = [np.array([True, True, False, True]), np.zeros(0, bool), np.array([True, True])]
    got = hfl.correspondence_pairs_host(idx)
    assert [g.tolist() for g in got] == [[[0, 2], [2, 0], [3, 5]], [], [[1, 3]]]
    assert all(g.dtype == np.int64 and g.shape[1] == 2 for g in got)
    got = hfl.correspondence_pairs_host(idx, mask)
    assert [g.tolist() for g in got] == [[[0, 2], [3, 5]], [], [[1, 3]]]
    rows, off = hfl.correspondence_pairs_host((np.concatenate(idx), np.array([0, 4, 4, 6])), np.concatenate(mask))
    assert rows.tolist() == [[0, 2], [3, 5], [1, 3]] and off.tolist() == [0, 2, 2, 3]
    got = hfl.correspondence_pairs([torch.from_numpy(i) for i in idx], [torch.from_numpy(m) for m in mask])
    assert all(isinstance(g, torch.Tensor) and g.dtype == torch.int64 for g in got)
    assert [g.tolist() for g in got] == [[[0, 2], [3, 5]], [], [[1, 3]]]
    with pytest.raises(ValueError):
        hfl.correspondence_pairs_host(idx, np.concatenate(mask))
    with pytest.raises(TypeError):
        hfl.correspondence_pairs_host([np.zeros(3, np.float32)])


def test_both_layouts_and_a_ragged_batch_agree():
    src, dst = gc.clouds()
    a, b = gc.rows(40, 0.5, 2), gc.rows(0, 0.0, 0)
    as_list = hfl.ransac_registration_host([src, src, dst], [dst, dst, src], [a, b, a], hypotheses=256,
                                           max_correspondence_distance=gc.TAU)
    n = src.shape[0]
    packed = hfl.ransac_registration_host((np.concatenate([src, src, dst]), np.array([0, n, 2 * n, 3 * n])),
                                          (np.concatenate([dst, dst, src]), np.array([0, n, 2 * n, 3 * n])),
                                          (np.concatenate([a, b, a]), np.array([0, 40, 40, 80])), hypotheses=256,
                                          max_correspondence_distance=gc.TAU)
    for x, y in zip(as_list, packed):
        assert np.array_equal(x, y, equal_nan=True)
    assert as_list.status.tolist() == [reg.MAX_ITERATIONS, GR.NO_HYPOTHESIS, reg.MAX_ITERATIONS]
    assert gc.pose_error(as_list.transforms[0])[0] < gc.ANGLE_TOL_DEG
    inverse = np.linalg.inv(np.concatenate([gc.truth(), [[0.0, 0.0, 0.0, 1.0]]]))
    assert gc.pose_error(as_list.transforms[2], inverse)[0] < gc.ANGLE_TOL_DEG


def test_purpose_sixty_percent_wrong_correspondences():
    """The trial of the issue with another generator gave 78-97 valid hypotheses of 1024 and 62-79 with more than half the true
    inliers at 60 % corruption; the Philox draws of the fixed seed give 87 and 69."""
    figures = gc.purpose_figures()
    res = figures['result']
    print('valid hypotheses %d, with more than half the true inliers %d' % (figures['valid'], figures['good']))
    assert 60 <= figures['valid'] <= 120 and 40 <= figures['good'] <= figures['valid']
    angle, shift = gc.pose_error(res.transforms[0])
    print('pose error %.3g degrees, %.3g m' % (angle, shift))
    assert res.status.tolist() == [reg.MAX_ITERATIONS]
    assert angle < gc.ANGLE_TOL_DEG and shift < gc.SHIFT_TOL
    true = gc.true_rows(gc.PURPOSE['frac'])
    src, dst, pairs = gc.corrupted(gc.PURPOSE['frac'])
    moved = src[pairs[:, 0]].astype(np.float64) @ gc.truth()[:, :3].T + gc.truth()[:, 3]
    admitted = np.linalg.norm(moved - dst[pairs[:, 1]], axis=1) <= gc.TAU
    assert admitted[true].all() and not admitted[~true].any()          # the threshold admits the uncorrupted rows, no other
    assert res.inliers.tolist() == [int(true.sum())] and res.fitness[0] == true.sum() / true.shape[0]
    assert res.valid_hypotheses.tolist() == [figures['valid']]
    assert res.hypothesis_inliers[0] == figures['counts'].max() and res.hypothesis[0] == figures['counts'].argmax()


def test_purpose_eighty_percent_wrong_correspondences():
    src, dst, pairs = gc.corrupted(0.8)
    res = hfl.ransac_registration_host([src], [dst], [pairs], max_correspondence_distance=gc.TAU, hypotheses=4096)
    angle, shift = gc.pose_error(res.transforms[0])
    assert angle < gc.ANGLE_TOL_DEG and shift < gc.SHIFT_TOL
    assert res.inliers.tolist() == [int(gc.true_rows(0.8).sum())]
