"""The generalized (plane-to-plane) estimator on the device: `hfl_icp_correspond_generalized` and `hfl_icp_solve_plane`
(hotformerloc_amd/csrc/registration.hip) through `hotformerloc_amd.registration`.

Correspondences: dist, idx and the inlier flags have the bits of the call without normals, n is equal.  Sums: against numpy
float64 on the device's own rows -- `transform_points` for the moved points and, with the translation zeroed, for the moved
source normals; the device's idx; the host row function of the definition (`registration._host_generalized_rows`) -- each
of the 29 sums to 1e-12 of its scale, the sum of the magnitudes of its terms: the rule of `check_plane_sums` in
tests/test_gpu_registration_plane.py.  The kernel's row is compiled without contraction, so its rows are the host's to the
bit and only the order of the sums differs; the bound is not widened.  Whole loop against
`icp_refine_host(estimation='generalized')`: status, iterations and fitness equal, poses to 1e-5 and rmse to 1e-6, the
bounds tests/test_gpu_registration.py uses for the same two routes."""
import numpy as np
import pytest
import torch

import hotformerloc_amd as hfl
from hotformerloc_amd import (_native, estimate_normals, icp_correspondences, icp_refine, ops, transform_points,
                              registration as reg)
from tests import generalized_cases as gcs
from tests import global_registration_cases as gc
from tests import normals_cases as nc
from tests import registration_cases as rc
from tests import spectral_cases as sc
from tests.test_gpu_global_registration import GLOBAL_BOUNDS

pytestmark = pytest.mark.gpu

T, Q = ops.OVERLAP_TILE, ops.OVERLAP_ROWS
MOVE = rc.rigid(6.0, 0.3)


def dev(clouds):
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in clouds]


def check_generalized_sums(srcs, dsts, n_s, n_t, ms, max_dist=0.8, eps=gcs.EPS):
    """one evaluation with both sets of normals: the rows' bits against the call without, the 29 sums against the host row
    on the device's own rows -> (dist, idx, inlier, sums, zero source normal, zero target normal) over the inliers"""
    dist, idx, inl, sums = icp_correspondences(dev(srcs), dev(dsts), ms, max_dist, target_normals=dev(n_t),
                                               source_normals=dev(n_s), covariance_epsilon=eps)
    plain = icp_correspondences(dev(srcs), dev(dsts), ms, max_dist)
    moved = transform_points(dev(srcs), ms)                              # the device's own moved rows
    turn = np.array(ms, np.float64)
    turn[:, :3, 3] = 0.0
    turned = transform_points(dev(n_s), turn)                            # fmaf(r0, x, 0) is r0 * x rounded once
    assert dist.dtype == torch.float32 and idx.dtype == torch.int32 and inl.dtype == torch.bool
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (len(srcs), reg.N_SUMS_PLANE)
    assert torch.equal(dist.view(torch.int32), plain[0].view(torch.int32)) and torch.equal(idx, plain[1])
    assert torch.equal(inl, plain[2])
    dist, idx, inl, sums = dist.cpu().numpy(), idx.cpu().numpy(), inl.cpu().numpy(), sums.cpu().numpy()
    assert np.array_equal(sums[:, 0], plain[3][:, 0].cpu().numpy())
    off = np.concatenate([[0], np.cumsum([len(s) for s in srcs])])
    zero_a, zero_b, worst = [], [], 0.0
    for p, (src, dst, nrm) in enumerate(zip(srcs, dsts, n_t)):
        rows = slice(off[p], off[p + 1])
        keep = inl[rows]
        pp = moved[p].cpu().numpy()[keep].reshape(-1, 3)
        aa = turned[p].cpu().numpy()[keep].reshape(-1, 3)
        qq, bb = dst[idx[rows][keep]].reshape(-1, 3), nrm[idx[rows][keep]].reshape(-1, 3)
        terms = reg._host_generalized_rows(pp, qq, aa, bb, dist[rows][keep], eps)
        assert sums[p, 0] == keep.sum()
        for k in range(reg.N_SUMS_PLANE):
            scale = np.abs(terms[:, k]).sum()
            assert abs(sums[p, k] - terms[:, k].sum()) <= 1e-12 * scale, (p, k, sums[p, k], terms[:, k].sum())
            if scale > 0:
                worst = max(worst, abs(sums[p, k] - terms[:, k].sum()) / scale)
        zero_a.append(~aa.any(1))
        zero_b.append(~bb.any(1))
    print('sums differ from the host rows by at most %.3g of their scale' % worst)
    return dist, idx, inl, sums, np.concatenate(zero_a), np.concatenate(zero_b)


@pytest.mark.parametrize('n', [Q - 1, Q, Q + 1])
def test_source_counts_around_the_workgroup(n):
    dst = rc.target(T + 1)                                               # one target past an LDS tile
    mi = np.linalg.inv(MOVE)
    src = (dst[np.random.default_rng(n).permutation(len(dst))[:n]].astype(np.float64) @ mi[:3, :3].T + mi[:3, 3] +
           np.random.default_rng(n + 1).normal(0.0, 0.05, (n, 3))).astype(np.float32)
    src[n - 1] = (dst[-1:].astype(np.float64) @ mi[:3, :3].T + mi[:3, 3]).astype(np.float32)[0]
    n_s, n_t = gcs.unit_normals(n, n + 2, 5, 1), gcs.unit_normals(len(dst), n, 5, 3)
    dist, idx, inl, sums, zero_a, zero_b = check_generalized_sums([src], [dst], [n_s], [n_t], MOVE[None])
    assert idx[n - 1] == len(dst) - 1 and inl.all()
    for a in (zero_a, ~zero_a):                                          # all four zero / non-zero combinations occur
        for b in (zero_b, ~zero_b):
            assert (a & b).any()


def test_ragged_batch_with_empty_clouds_and_outliers():
    dst = rc.target(700)
    srcs = [np.concatenate([rc.source_of(dst, 300, MOVE, 3, noise=0.05), rc.far_points(40, 4)]),
            np.zeros((0, 3), np.float32), rc.source_of(dst, 50, MOVE, 5), rc.source_of(dst, Q + 7, MOVE, 6, noise=0.05)]
    dsts = [dst, rc.target(64), np.zeros((0, 3), np.float32), rc.target(T + 300)]
    n_t = [gcs.unit_normals(len(d), 10 + i, 3 if i == 3 else 0) for i, d in enumerate(dsts)]
    n_s = [gcs.unit_normals(len(s), 20 + i, 4 if i == 3 else 0, 1) for i, s in enumerate(srcs)]
    dist, idx, inl, sums, zero_a, zero_b = check_generalized_sums(srcs, dsts, n_s, n_t, np.stack([MOVE] * 4))
    assert 0 < inl[:340].sum() < 340 and (sums[1] == 0.0).all() and (sums[2] == 0.0).all() and sums[3, 0] > 0
    assert (zero_a & zero_b).any() and (~zero_a & ~zero_b).any()
    # another epsilon reaches the kernel
    other = icp_correspondences(dev(srcs), dev(dsts), np.stack([MOVE] * 4), 0.8, target_normals=dev(n_t),
                                source_normals=dev(n_s), covariance_epsilon=0.25)[3].cpu().numpy()
    assert np.array_equal(other[:, :2], sums[:, :2]) and not np.array_equal(other[0, 2:], sums[0, 2:])
    check_generalized_sums(srcs[:1], dsts[:1], n_s[:1], n_t[:1], MOVE[None], eps=0.25)


def test_whole_loop_against_the_host():
    c = gcs.loop_batch()
    host = c['host']
    assert list(host.status) == [reg.CONVERGED, reg.CONVERGED, reg.TOO_FEW, reg.CONVERGED]
    kw = dict(max_correspondence_distance=gcs.MAX_DIST, estimation='generalized')
    got = icp_refine(dev(c['srcs']), dev(c['dsts']), target_normals=dev(c['n_t']), source_normals=dev(c['n_s']), **kw)
    assert isinstance(got, reg.RegistrationResult) and got.transforms.shape == (4, 4, 4) and got.transforms.dtype == np.float64
    assert np.array_equal(got.status, host.status) and np.array_equal(got.iterations, host.iterations)
    assert np.array_equal(got.fitness, host.fitness, equal_nan=True)
    print('poses differ by %.3g, rmse by %.3g' % (np.abs(got.transforms - host.transforms).max(),
                                                  np.nanmax(np.abs(got.inlier_rmse - host.inlier_rmse))))
    assert np.abs(got.transforms - host.transforms).max() <= 1e-5
    assert np.array_equal(np.isnan(got.inlier_rmse), np.isnan(host.inlier_rmse))
    ok = ~np.isnan(host.inlier_rmse)
    assert (np.abs(got.inlier_rmse[ok] - host.inlier_rmse[ok]) <= 1e-6).all()
    assert np.array_equal(got.transforms[2], np.eye(4))
    assert all(gcs.orthonormal(got.transforms[p, :3, :3]) for p in range(4))
    # the flat pair is DEGENERATE for point-to-plane and is not here; both corners end nearer the truth
    plane = icp_refine(dev(c['srcs']), dev(c['dsts']), max_correspondence_distance=gcs.MAX_DIST, estimation='point_to_plane',
                       target_normals=dev(c['n_t']))
    assert plane.status[3] == reg.DEGENERATE and got.status[3] != reg.DEGENERATE
    for p in range(2):
        e_gen, e_plane = nc.pose_errors(got.transforms[p], c['g'][p]), nc.pose_errors(plane.transforms[p], c['g'][p])
        print('pair %d: generalized %.4f deg %.4f m, point-to-plane %.4f deg %.4f m' % ((p,) + e_gen + e_plane))
        assert e_gen[0] < e_plane[0] and e_gen[1] < e_plane[1]
    # the packed layout: one (N, 3) tensor of normals under each side's offsets
    s_off = np.concatenate([[0], np.cumsum([len(s) for s in c['srcs']])])
    t_off = np.concatenate([[0], np.cumsum([len(d) for d in c['dsts']])])
    flat = icp_refine((torch.cat(dev(c['srcs'])), s_off), (torch.cat(dev(c['dsts'])), t_off),
                      target_normals=torch.cat(dev(c['n_t'])), source_normals=torch.cat(dev(c['n_s'])), **kw)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(flat, got))


def test_normals_straight_from_the_device():
    c = gcs.loop_batch()
    srcs, dsts = dev(c['srcs'][:2]), dev(c['dsts'][:2])
    nrms = estimate_normals(srcs + dsts, gcs.NB)
    assert all(n.is_cuda and n.dtype == torch.float32 for n in nrms)
    got = icp_refine(srcs, dsts, max_correspondence_distance=gcs.MAX_DIST, estimation='generalized', target_normals=nrms[2:],
                     source_normals=nrms[:2])
    assert list(got.status) == [reg.CONVERGED, reg.CONVERGED]
    assert np.abs(got.transforms - c['host'].transforms[:2]).max() <= 1e-5


def test_two_runs_give_the_same_bits_and_the_other_modes_keep_theirs():
    c = gcs.loop_batch()
    args = (dev(c['srcs']), dev(c['dsts']))
    plane_kw = dict(max_correspondence_distance=gcs.MAX_DIST, estimation='point_to_plane', target_normals=dev(c['n_t']))
    plane_before = icp_refine(*args, **plane_kw)
    runs = [icp_refine(*args, max_correspondence_distance=gcs.MAX_DIST, estimation='generalized', target_normals=dev(c['n_t']),
                       source_normals=dev(c['n_s'])) for _ in range(2)]
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()
    one = [icp_correspondences(*args, runs[0].transforms, gcs.MAX_DIST, target_normals=dev(c['n_t']),
                               source_normals=dev(c['n_s'])) for _ in range(2)]
    for a, b in zip(*one):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    default = icp_refine(*args, max_correspondence_distance=gcs.MAX_DIST)
    named = icp_refine(*args, max_correspondence_distance=gcs.MAX_DIST, estimation='point_to_point')
    for a, b in zip(default, named):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(plane_before, icp_refine(*args, **plane_kw)):        # next to generalized runs in the same process
        assert a.tobytes() == b.tobytes()
    assert not np.array_equal(plane_before.transforms[0], runs[0].transforms[0])
    assert np.abs(plane_before.transforms - c['plane'].transforms).max() <= 1e-5


def test_global_registration_and_rerank_end_where_the_host_ends():
    src, dst = gc.clouds()
    coarse, fine = hfl.global_registration([dev([src])[0]], [dev([dst])[0]], estimation='generalized')
    h_coarse, h_fine = hfl.global_registration_host([src], [dst], estimation='generalized')
    angle, shift = gc.pose_error(fine.transforms[0])
    print('global: fine %.3g degrees %.3g m; host fine %.3g degrees %.3g m'
          % ((angle, shift) + gc.pose_error(h_fine.transforms[0])))
    assert coarse.status.tolist() == h_coarse.status.tolist() == [reg.MAX_ITERATIONS]
    assert fine.status.tolist() == h_fine.status.tolist() == [reg.CONVERGED]
    assert angle <= GLOBAL_BOUNDS['point_to_plane'][0] and shift <= GLOBAL_BOUNDS['point_to_plane'][1]
    queries, database, cand = sc.rerank_inputs()
    on = (dev(queries), dev(database), torch.from_numpy(cand).cuda())
    ranked, coarse, fine = hfl.rerank_candidates(*on, register=True, estimation='generalized')
    host, h_coarse, h_fine = hfl.rerank_candidates_host(queries, database, cand, register=True, estimation='generalized')
    assert np.array_equal(ranked.indices.cpu().numpy(), host.indices)
    assert fine.status.tolist() == h_fine.status.tolist() == [reg.CONVERGED]
    angle, shift = gc.pose_error(fine.transforms[0], sc.rerank_truth())
    print('rerank: fine %.3g degrees %.3g m; host fine %.3g degrees %.3g m'
          % ((angle, shift) + gc.pose_error(h_fine.transforms[0], sc.rerank_truth())))
    assert angle <= GLOBAL_BOUNDS['point_to_plane'][0] and shift <= GLOBAL_BOUNDS['point_to_plane'][1]


def test_arguments_are_refused(monkeypatch):
    dst = rc.target(50)
    nrm = gcs.unit_normals(50, 1)
    good = dict(estimation='generalized', target_normals=dev([nrm]), source_normals=dev([nrm]))
    with pytest.raises(_native.NativeLibraryError):
        icp_refine(dev([dst]), dev([dst]), **dict(good, source_normals=[torch.from_numpy(nrm)]))
    with pytest.raises(_native.NativeLibraryError):
        icp_refine(dev([dst]), dev([dst]), **dict(good, target_normals=[torch.from_numpy(nrm)]))
    with pytest.raises(_native.NativeLibraryError):
        icp_refine([torch.from_numpy(dst)], [torch.from_numpy(dst)], **good)
    launched = []
    real = ops.icp_correspond
    monkeypatch.setattr(ops, 'icp_correspond', lambda *a, **k: launched.append(1) or real(*a, **k))
    bad = [dict(estimation='generalized'), dict(estimation='generalized', target_normals=dev([nrm])),
           dict(estimation='generalized', source_normals=dev([nrm])), dict(source_normals=dev([nrm])),
           dict(estimation='point_to_plane', target_normals=dev([nrm]), source_normals=dev([nrm])),
           dict(good, source_normals=dev([nrm[:-1]])), dict(good, source_normals=dev([nrm])[0]),
           dict(good, covariance_epsilon=0.0), dict(good, covariance_epsilon=1.5), dict(good, covariance_epsilon=float('nan'))]
    for kw in bad:
        with pytest.raises(ValueError):
            icp_refine(dev([dst]), dev([dst]), **kw)
    with pytest.raises(ValueError):
        icp_correspondences(dev([dst]), dev([dst]), np.eye(4)[None], 1.0, source_normals=dev([nrm]))
    assert not launched                                                  # every one of them before a launch
    icp_refine(dev([dst]), dev([dst]), max_iterations=1, **good)
    assert launched
    # the entry point itself: a null normals pointer, an epsilon outside (0, 1]
    lib = _native.load()
    d = dev([dst])[0]
    n = dev([nrm])[0]
    off = torch.tensor([0, 50], dtype=torch.int64).cuda()
    tiles = torch.tensor([[0, 0]], dtype=torch.int64).cuda()
    state, istate = reg._device_state(np.eye(4)[None, :3], d.device)
    partials = torch.zeros((1, 29), dtype=torch.float64).cuda()

    def call(s_normals, t_normals, eps):
        return lib.hfl_icp_correspond_generalized(partials.data_ptr(), None, None, d.data_ptr(), s_normals, off.data_ptr(), 50,
                                                  d.data_ptr(), t_normals, off.data_ptr(), 50, tiles.data_ptr(), 1,
                                                  state.data_ptr(), istate.data_ptr(), 1.0, eps, 1, None)
    einval = call(None, n.data_ptr(), 1e-3)
    assert einval != 0 and call(n.data_ptr(), None, 1e-3) == einval
    assert call(n.data_ptr(), n.data_ptr(), 0.0) == einval and call(n.data_ptr(), n.data_ptr(), 1.0 + 1e-9) == einval
    assert call(n.data_ptr(), n.data_ptr(), float('nan')) == einval
    assert call(n.data_ptr(), n.data_ptr(), 1.0) == 0 and partials[0, 0].item() == 50.0
