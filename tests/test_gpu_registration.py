"""`hfl_icp_correspond` and `hfl_icp_solve` (hotformerloc_amd/csrc/registration.hip) through `hotformerloc_amd.registration`.

Correspondences: bit-equal to the existing kernels, `nn_distances(transform_points(src, T), dst)`, at the sizes where the
tiling can go wrong (512 source rows per workgroup, 2048 targets per LDS tile).  Sums: against numpy float64 on the device's
own rows, n equal, every sum to 1e-12 of its scale (the sum of the magnitudes of its terms): the orders differ, the terms do
not.  Solve: against `kabsch_update_host` to 1e-12 (the same algorithm; the device may contract a product into a sum).  Whole
loop against `icp_refine_host` under the guards of tests/registration_cases.py: status, iterations, fitness and the final
correspondences equal; poses to 1e-5 -- the routes' moved coordinates differ by at most the 4 ulp32 that
tests/test_gpu_overlap.py allows the transform (3.8e-6 m at |x| <= 16 m), times about 2.5 for the least-squares solve of a
well-spread cloud; rmse to 1e-6 absolute."""
import numpy as np
import pytest
import torch

import overlap_cases as oc
import registration_cases as rc
from hotformerloc_amd import (_native, evaluate_registration, icp_correspondences,
                              icp_correspondences_host, icp_refine, icp_refine_host, kabsch_update, kabsch_update_host,
                              nn_distances, ops, submap_overlap, transform_points, registration as reg)

pytestmark = pytest.mark.gpu

T, Q = ops.OVERLAP_TILE, ops.OVERLAP_ROWS
MOVE = rc.rigid(6.0, 0.3)
_CACHE = {}


def dev(clouds):
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in clouds]


def back(m, pts):
    """the float32 points that `m` moves onto `pts`, to rounding"""
    mi = np.linalg.inv(m)
    return (pts.astype(np.float64) @ mi[:3, :3].T + mi[:3, 3]).astype(np.float32)


def check_bits(srcs, dsts, ms, max_dist=0.8):
    """`icp_correspondences` against the existing kernels; returns the device's (dist, idx, inlier, sums, moved) as numpy"""
    dist, idx, inl, sums = icp_correspondences(dev(srcs), dev(dsts), ms, max_dist)
    moved = transform_points(dev(srcs), ms)
    want_d, want_i, _ = nn_distances(moved, dev(dsts))
    torch.cuda.synchronize()
    assert dist.dtype == torch.float32 and idx.dtype == torch.int32 and inl.dtype == torch.bool and sums.dtype == torch.float64
    assert torch.equal(dist.view(torch.int32), want_d.view(torch.int32)) and torch.equal(idx, want_i)
    assert torch.equal(inl, (want_i >= 0) & (want_d <= float(np.float32(max_dist))))
    return dist.cpu().numpy(), idx.cpu().numpy(), inl.cpu().numpy(), sums.cpu().numpy(), [m.cpu().numpy() for m in moved]


def check_sums(sums, dist, idx, inl, moved, dsts):
    """the device's 17 sums per pair against numpy float64 on the device's own rows"""
    off = np.concatenate([[0], np.cumsum([len(m) for m in moved])])
    for p, (m, dst) in enumerate(zip(moved, dsts)):
        rows = slice(off[p], off[p + 1])
        keep = inl[rows]
        pp, qq = m[keep].astype(np.float64), dst[idx[rows][keep]].astype(np.float64).reshape(-1, 3)
        d = dist[rows][keep].astype(np.float64)
        terms = [np.ones(len(pp))] + [pp[:, a] for a in range(3)] + [qq[:, a] for a in range(3)] + \
                [pp[:, a] * qq[:, b] for a in range(3) for b in range(3)] + [d * d]
        assert sums[p, 0] == keep.sum()
        for k, term in enumerate(terms):
            assert abs(sums[p, k] - term.sum()) <= 1e-12 * np.abs(term).sum(), (p, k)


@pytest.mark.parametrize('n', [1, Q - 1, Q, Q + 1, 2 * Q + 1])
def test_source_counts_around_the_workgroup(n):
    dst = rc.target(2118)
    src = back(MOVE, dst[np.random.default_rng(n).permutation(len(dst))[:n]])
    src[n - 1] = back(MOVE, dst[-1:])[0]                                 # the last row hits the last target, past a tile edge
    dist, idx, inl, sums, moved = check_bits([src], [dst], MOVE[None])
    assert idx[n - 1] == len(dst) - 1 and dist[n - 1] < 1e-5 and inl.all()
    check_sums(sums, dist, idx, inl, moved, [dst])


@pytest.mark.parametrize('m', [1, T - 1, T, T + 1, 2 * T + 1])
def test_target_counts_around_the_tile(m):
    dst = rc.target(m)
    src = rc.source_of(dst, Q + 1, MOVE, 100 + m, noise=0.05)
    src[0] = back(MOVE, dst[-1:])[0]                                     # a hit on the last target of a tile
    src[1] = back(MOVE, dst[:1])[0]
    dist, idx, inl, sums, moved = check_bits([src], [dst], MOVE[None])
    assert idx[0] == m - 1 and idx[1] == 0 and dist[0] < 1e-5 and dist[1] < 1e-5
    check_sums(sums, dist, idx, inl, moved, [dst])


def test_duplicate_targets_take_the_lowest_index():
    dst, lowest = oc.with_duplicates(rc.target(T + 300), 8)              # copies on both sides of the tile edge
    assert (lowest < np.arange(len(dst))).sum() > 100 and (lowest[T:] < T).any()
    src = back(MOVE, dst)                                                # every duplicate is somebody's nearest target
    dist, idx, inl, sums, moved = check_bits([src], [dst], MOVE[None])
    assert np.array_equal(lowest[idx], idx) and (idx != np.arange(len(dst))).sum() > 100
    check_sums(sums, dist, idx, inl, moved, [dst])


def test_sums_of_a_ragged_batch_with_empty_clouds():
    a, b = oc.ragged_pairs(31)                                           # pair 1 has no source, pair 2 no target
    ms = np.stack([oc.rigid(50 + p, max_shift=0.3) for p in range(5)])
    dist, idx, inl, sums, moved = check_bits(a, b, ms)
    assert 0 < inl.sum() < len(inl)                                      # inliers and outliers both
    check_sums(sums, dist, idx, inl, moved, b)
    assert (sums[1] == 0.0).all() and (sums[2] == 0.0).all()
    # the figures of one evaluation are those sums' (one float64 division and square root)
    fitness, rmse = evaluate_registration(dev(a), dev(b), ms, 0.8, min_correspondences=1)
    fitness, rmse = fitness.cpu().numpy(), rmse.cpu().numpy()
    assert np.isnan(fitness[1]) and fitness[2] == 0.0 and np.isnan(rmse[1]) and np.isnan(rmse[2])
    keep = [0, 3, 4]
    assert (sums[keep, 0] >= 1).all()
    assert (fitness[keep] == sums[keep, 0] / [len(a[p]) for p in keep]).all()
    assert (np.abs(rmse[keep] - np.sqrt(sums[keep, 16] / sums[keep, 0])) <= 1e-14).all()


def test_kabsch_update_against_the_host():
    sums, kinds = rc.kabsch_cases()
    want_r, want_t, want_s = kabsch_update_host(sums)
    r, t, status = kabsch_update(torch.from_numpy(sums).cuda())
    assert r.is_cuda and r.dtype == torch.float64 and tuple(r.shape) == (len(kinds), 3, 3) and tuple(t.shape) == (len(kinds), 3)
    r, t, status = r.cpu().numpy(), t.cpu().numpy(), status.cpu().numpy()
    assert np.array_equal(status, want_s)
    assert status[list(kinds).index('line')] == reg.DEGENERATE and status[list(kinds).index('few')] == reg.TOO_FEW
    assert np.abs(r - want_r).max() <= 1e-12 and np.abs(t - want_t).max() <= 1e-12
    assert np.abs(np.einsum('kij,kil->kjl', r, r) - np.eye(3)).max() <= 1e-12
    assert (np.abs(np.linalg.det(r) - 1.0) <= 1e-12).all()              # the mirror and the planar case included


def loop_batch():
    """P = 5: an exact pair, a noisy pair, a pair with outliers (4913 targets: three LDS tiles), a pair whose every point is
    beyond the distance, an empty pair; the host route's results and every pair's guarded trace, computed once"""
    if 'loop' not in _CACHE:
        exact_s, dst, g_exact, _ = rc.pair(rc.EXACT)
        noisy_s, _, g_noisy, max_dist = rc.pair(rc.NOISY, seed=3)
        big = rc.target(4913)
        out_s = np.concatenate([rc.source_of(big, 513, g_exact, 7), rc.far_points(300, 5)])
        srcs = [exact_s, noisy_s, out_s, rc.far_points(100, 9), np.zeros((0, 3), np.float32)]
        dsts = [dst, dst, big, rc.target(300), rc.target(64)]
        traces = [rc.trace(s, d, max_dist) for s, d in zip(srcs, dsts)]
        _CACHE['loop'] = dict(srcs=srcs, dsts=dsts, max_dist=max_dist, g=[g_exact, g_noisy, g_exact], traces=traces,
                              host=icp_refine_host(srcs, dsts, max_correspondence_distance=max_dist))
    return _CACHE['loop']


def test_whole_loop_against_the_host():
    c = loop_batch()
    host, max_dist = c['host'], c['max_dist']
    for p, tr in enumerate(c['traces']):                                 # the host route is what the guarded replay says
        assert host.status[p] == tr['status'] and host.iterations[p] == tr['iterations']
    assert list(host.status) == [reg.CONVERGED, reg.CONVERGED, reg.CONVERGED, reg.TOO_FEW, reg.TOO_FEW]
    assert len(set(host.iterations)) >= 3                                # pairs stop while others run on
    got = icp_refine(dev(c['srcs']), dev(c['dsts']), max_correspondence_distance=max_dist)
    assert isinstance(got, reg.RegistrationResult) and got.transforms.shape == (5, 4, 4) and got.transforms.dtype == np.float64
    assert np.array_equal(got.status, host.status) and np.array_equal(got.iterations, host.iterations)
    assert np.array_equal(got.fitness, host.fitness, equal_nan=True)
    assert got.fitness[2] == 513 / 813 and got.fitness[3] == 0.0 and np.isnan(got.fitness[4])
    assert np.abs(got.transforms - host.transforms).max() <= 1e-5
    assert np.array_equal(np.isnan(got.inlier_rmse), np.isnan(host.inlier_rmse)) and np.isnan(got.inlier_rmse[3:]).all()
    assert (np.abs(got.inlier_rmse[:3] - host.inlier_rmse[:3]) <= 1e-6).all()
    assert np.abs(got.transforms[0] - c['g'][0]).max() <= 1e-5 and np.abs(got.transforms[2] - c['g'][2]).max() <= 1e-5
    assert np.array_equal(got.transforms[3], np.eye(4)) and np.array_equal(got.transforms[4], np.eye(4))
    # the correspondences of the final evaluation
    _, idx, inl, _ = icp_correspondences(dev(c['srcs']), dev(c['dsts']), got.transforms, max_dist)
    _, want_idx, want_inl, _ = icp_correspondences_host(c['srcs'], c['dsts'], host.transforms, max_dist)
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(inl.cpu().numpy(), want_inl)
    # the reported figures belong to the reported pose
    fitness, rmse = evaluate_registration(dev(c['srcs']), dev(c['dsts']), got.transforms, max_dist)
    assert np.array_equal(fitness.cpu().numpy(), got.fitness, equal_nan=True)
    assert np.array_equal(rmse.cpu().numpy(), got.inlier_rmse, equal_nan=True)


def test_iteration_limit_and_degenerate_pairs():
    c = loop_batch()
    line = (np.linspace(-5.0, 5.0, 41)[:, None] * np.array([[1.0, 0.5, 0.25]])).astype(np.float32)
    srcs, dsts = [c['srcs'][1], line, c['srcs'][1]], [c['dsts'][1], line, c['dsts'][1]]
    for limit in (0, 2):
        host = icp_refine_host(srcs, dsts, max_correspondence_distance=c['max_dist'], max_iterations=limit)
        got = icp_refine(dev(srcs), dev(dsts), max_correspondence_distance=c['max_dist'], max_iterations=limit)
        # the evaluate-only round k == max_iterations never reaches the solve: at limit 0 the line is not found out
        assert list(got.status) == [reg.MAX_ITERATIONS, reg.DEGENERATE if limit else reg.MAX_ITERATIONS, reg.MAX_ITERATIONS]
        assert np.array_equal(got.status, host.status) and np.array_equal(got.iterations, host.iterations)
        assert list(got.iterations) == [limit, 0, limit] and np.array_equal(got.fitness, host.fitness)
        assert np.abs(got.transforms - host.transforms).max() <= 1e-5
        assert (np.abs(got.inlier_rmse - host.inlier_rmse) <= 1e-6).all()
    assert np.array_equal(got.transforms[1], np.eye(4))


def test_two_runs_give_the_same_bits():
    c = loop_batch()
    runs = [icp_refine(dev(c['srcs']), dev(c['dsts']), max_correspondence_distance=c['max_dist']) for _ in range(2)]
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()
    ms = runs[0].transforms
    one = [icp_correspondences(dev(c['srcs']), dev(c['dsts']), ms, c['max_dist']) for _ in range(2)]
    for a, b in zip(*one):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_init_from_submap_overlap_at_utm_poses():
    """poses of UTM magnitude (a northing of 6.9e6 m) never meet float32: `submap_overlap` composes the relative pose in
    float64 and `icp_refine` starts from it"""
    c = loop_batch()
    src, dst, g = c['srcs'][0], c['dsts'][0], c['g'][0]
    m_b = oc.rigid(3)
    m_b[:3, 3] = [4.71e5, 6.93e6, 87.0]
    surveyed = rc.rigid(0.6, 0.03)                                       # the survey says this; the clouds say G
    m_a = m_b @ surveyed
    o = submap_overlap(dev([src]), dev([dst]), m_a[None], m_b[None])
    assert np.abs(o.transforms[0] - surveyed).max() <= 1e-8
    got = icp_refine(dev([src]), dev([dst]), init=o.transforms, max_correspondence_distance=c['max_dist'])
    host = icp_refine_host([src], [dst], init=o.transforms, max_correspondence_distance=c['max_dist'])
    assert got.status[0] == reg.CONVERGED and np.array_equal(got.status, host.status)
    assert np.array_equal(got.iterations, host.iterations) and np.array_equal(got.fitness, host.fitness)
    assert np.abs(got.transforms - host.transforms).max() <= 1e-5 and np.abs(got.transforms[0] - g).max() <= 1e-5
    # the tensor form and the concatenated layout
    flat = icp_refine((torch.from_numpy(src).cuda(), torch.tensor([0, len(src)])), (torch.from_numpy(dst).cuda(), [0, len(dst)]),
                      init=torch.from_numpy(o.transforms[:, :3]), max_correspondence_distance=c['max_dist'])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(flat, got))


def test_arguments_are_refused():
    dst = rc.target(50)
    with pytest.raises(_native.NativeLibraryError):
        icp_refine([torch.from_numpy(dst)], dev([dst]))
    with pytest.raises(_native.NativeLibraryError):
        icp_correspondences(dev([dst]), [torch.from_numpy(dst)], np.eye(4)[None], 0.8)
    with pytest.raises(_native.NativeLibraryError):
        evaluate_registration([torch.from_numpy(dst)], [torch.from_numpy(dst)], np.eye(4)[None], 0.8)
    with pytest.raises(_native.NativeLibraryError):
        kabsch_update(torch.zeros((1, 17), dtype=torch.float64))
    with pytest.raises(TypeError, match='float64 points'):
        icp_refine([torch.from_numpy(dst).double().cuda()], dev([dst]))
    with pytest.raises(TypeError):
        kabsch_update(torch.zeros((1, 17), dtype=torch.float32).cuda())
    with pytest.raises(ValueError):
        icp_refine(dev([dst]), dev([dst, dst]))
