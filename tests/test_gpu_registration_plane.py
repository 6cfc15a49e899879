"""The point-to-plane estimator on the device: `hfl_icp_correspond_plane` and `hfl_icp_solve_plane`
(hotformerloc_amd/csrc/registration.hip) through `hotformerloc_amd.registration`.

Correspondences: dist, idx and the inlier flags have the bits of the call without normals.  Sums: against numpy float64 on
the device's own rows, n equal, each of the 29 sums to 1e-12 of its scale (the sum of the magnitudes of its terms): the
orders differ, the terms do not -- the rule of `check_sums` in tests/test_gpu_registration.py.  Solve: status equal to
`plane_update_host`, (R, t) within 1e-12 x cond_2 of the diagonally scaled A x |x|_inf (the backward-error bound of a
stable solve at float64 eps with four digits of slack; cond <= 1e6 asserted).  Whole loop against
`icp_refine_host(estimation='point_to_plane')`: status, iterations and fitness equal, poses to 1e-5 and rmse to 1e-6, the
bounds tests/test_gpu_registration.py uses for the same two routes."""
import functools

import numpy as np
import pytest
import torch

from hotformerloc_amd import (_native, estimate_normals, estimate_normals_host, icp_correspondences, icp_refine,
                              icp_refine_host, ops, plane_update, plane_update_host, transform_points,
                              registration as reg)
from tests import normals_cases as nc
from tests import registration_cases as rc

pytestmark = pytest.mark.gpu

T, Q = ops.OVERLAP_TILE, ops.OVERLAP_ROWS
MOVE = rc.rigid(6.0, 0.3)


def dev(clouds):
    return [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in clouds]


def unit_normals(rows, seed, zero_every=0):
    """seeded unit vectors rounded to fp32; every `zero_every`-th row the "no normal" marker"""
    v = np.random.default_rng(seed).normal(0.0, 1.0, (rows, 3))
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    if zero_every:
        v[::zero_every] = 0.0
    return v


def check_plane_sums(srcs, dsts, nrms, ms, max_dist=0.8):
    """one evaluation with normals: the rows' bits against the call without, the 29 sums against numpy on those rows"""
    dist, idx, inl, sums = icp_correspondences(dev(srcs), dev(dsts), ms, max_dist, target_normals=dev(nrms))
    plain = icp_correspondences(dev(srcs), dev(dsts), ms, max_dist)
    moved = transform_points(dev(srcs), ms)                             # the device's own moved rows
    assert dist.dtype == torch.float32 and idx.dtype == torch.int32 and inl.dtype == torch.bool
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (len(srcs), reg.N_SUMS_PLANE)
    assert torch.equal(dist.view(torch.int32), plain[0].view(torch.int32)) and torch.equal(idx, plain[1])
    assert torch.equal(inl, plain[2])
    dist, idx, inl, sums = dist.cpu().numpy(), idx.cpu().numpy(), inl.cpu().numpy(), sums.cpu().numpy()
    assert np.array_equal(sums[:, 0], plain[3][:, 0].cpu().numpy())
    off = np.concatenate([[0], np.cumsum([len(s) for s in srcs])])
    for p, (src, dst, nrm) in enumerate(zip(srcs, dsts, nrms)):
        rows = slice(off[p], off[p + 1])
        keep = inl[rows]
        pp = moved[p].cpu().numpy()[keep].astype(np.float64)
        qq = dst[idx[rows][keep]].astype(np.float64).reshape(-1, 3)
        nn = nrm[idx[rows][keep]].astype(np.float64).reshape(-1, 3)
        d = dist[rows][keep].astype(np.float64)
        e = pp - qq
        r = (e[:, 0] * nn[:, 0] + e[:, 1] * nn[:, 1]) + e[:, 2] * nn[:, 2]
        jac = [pp[:, 1] * nn[:, 2] - pp[:, 2] * nn[:, 1], pp[:, 2] * nn[:, 0] - pp[:, 0] * nn[:, 2],
               pp[:, 0] * nn[:, 1] - pp[:, 1] * nn[:, 0], nn[:, 0], nn[:, 1], nn[:, 2]]
        terms = [np.ones(len(pp)), d * d] + [j * r for j in jac] + [jac[a] * jac[b] for a in range(6) for b in range(a, 6)]
        assert len(terms) == reg.N_SUMS_PLANE and sums[p, 0] == keep.sum()
        for k, term in enumerate(terms):
            assert abs(sums[p, k] - term.sum()) <= 1e-12 * np.abs(term).sum(), (p, k, sums[p, k], term.sum())
    return dist, idx, inl, sums


@pytest.mark.parametrize('n', [Q - 1, Q, Q + 1])
def test_source_counts_around_the_workgroup(n):
    dst = rc.target(T + 1)                                               # one target past an LDS tile
    mi = np.linalg.inv(MOVE)
    src = (dst[np.random.default_rng(n).permutation(len(dst))[:n]].astype(np.float64) @ mi[:3, :3].T + mi[:3, 3] +
           np.random.default_rng(n + 1).normal(0.0, 0.05, (n, 3))).astype(np.float32)
    src[n - 1] = (dst[-1:].astype(np.float64) @ mi[:3, :3].T + mi[:3, 3]).astype(np.float32)[0]
    dist, idx, inl, sums = check_plane_sums([src], [dst], [unit_normals(len(dst), n, zero_every=5)], MOVE[None])
    assert idx[n - 1] == len(dst) - 1 and inl.all()
    assert (idx % 5 == 0).any() and (idx % 5 != 0).any()                 # zero normals mixed in among the winners


def test_ragged_batch_with_empty_clouds_and_outliers():
    dst = rc.target(700)
    srcs = [np.concatenate([rc.source_of(dst, 300, MOVE, 3, noise=0.05), rc.far_points(40, 4)]),
            np.zeros((0, 3), np.float32), rc.source_of(dst, 50, MOVE, 5), rc.source_of(dst, Q + 7, MOVE, 6, noise=0.05)]
    dsts = [dst, rc.target(64), np.zeros((0, 3), np.float32), rc.target(T + 300)]
    nrms = [unit_normals(len(d), 10 + i, zero_every=3 if i == 3 else 0) for i, d in enumerate(dsts)]
    dist, idx, inl, sums = check_plane_sums(srcs, dsts, nrms, np.stack([MOVE] * 4))
    assert 0 < inl[:340].sum() < 340 and (sums[1] == 0.0).all() and (sums[2] == 0.0).all() and sums[3, 0] > 0


def test_plane_update_against_the_host():
    sums, kinds = nc.plane_cases()
    want_r, want_t, want_s = plane_update_host(sums)
    r, t, status = plane_update(torch.from_numpy(sums).cuda())
    assert r.is_cuda and r.dtype == torch.float64 and tuple(r.shape) == (len(kinds), 3, 3) and tuple(t.shape) == (len(kinds), 3)
    r, t, status = r.cpu().numpy(), t.cpu().numpy(), status.cpu().numpy()
    assert np.array_equal(status, want_s)
    assert status[list(kinds).index('parallel')] == reg.DEGENERATE and status[list(kinds).index('few')] == reg.TOO_FEW
    for i, kind in enumerate(kinds):
        if kind != 'corner':
            assert np.array_equal(r[i], np.eye(3)) and not t[i].any()
            continue
        a, g = nc.system_of(sums[i])
        cond = nc.scaled_cond(a)
        assert cond <= 1e6
        bound = 1e-12 * cond * np.abs(np.linalg.solve(a, -g)).max()
        assert np.abs(r[i] - want_r[i]).max() <= bound + 1e-15 and np.abs(t[i] - want_t[i]).max() <= bound
    assert np.abs(np.einsum('kij,kil->kjl', r, r) - np.eye(3)).max() <= 1e-12
    assert (np.abs(np.linalg.det(r) - 1.0) <= 1e-12).all()
    assert plane_update(torch.from_numpy(sums[:1]).cuda(), min_correspondences=10 ** 6)[2].item() == reg.TOO_FEW


@functools.lru_cache(maxsize=None)
def loop_batch():
    """P = 4: two corners (different seeds and motions), a pair whose every point is beyond the distance (TOO_FEW), and a
    flat target under exactly vertical normals, whose A has three zero rows (DEGENERATE); the host route's results"""
    c0, c1 = nc.corner_pair(seed=0), nc.corner_pair(600, 2100, seed=4, deg=-2.0, shift=0.1)
    flat = rc.target(400) * np.float32([1.0, 1.0, 0.0])
    srcs = [c0[0], c1[0], rc.far_points(100, 9), flat[:150].copy()]
    dsts = [c0[1], c1[1], rc.target(300), flat]
    nrms = list(estimate_normals_host(dsts[:3], 20)) + [np.tile(np.float32([0.0, 0.0, 1.0]), (len(flat), 1))]
    host = icp_refine_host(srcs, dsts, max_correspondence_distance=1.0, estimation='point_to_plane', target_normals=nrms)
    return dict(srcs=srcs, dsts=dsts, nrms=nrms, g=[c0[2], c1[2]], host=host)


def test_whole_loop_against_the_host():
    c = loop_batch()
    host = c['host']
    assert list(host.status) == [reg.CONVERGED, reg.CONVERGED, reg.TOO_FEW, reg.DEGENERATE]
    got = icp_refine(dev(c['srcs']), dev(c['dsts']), max_correspondence_distance=1.0, estimation='point_to_plane',
                     target_normals=dev(c['nrms']))
    assert isinstance(got, reg.RegistrationResult) and got.transforms.shape == (4, 4, 4) and got.transforms.dtype == np.float64
    assert np.array_equal(got.status, host.status) and np.array_equal(got.iterations, host.iterations)
    assert np.array_equal(got.fitness, host.fitness, equal_nan=True)
    print('poses differ by %.3g, rmse by %.3g' % (np.abs(got.transforms - host.transforms).max(),
                                                  np.nanmax(np.abs(got.inlier_rmse - host.inlier_rmse))))
    assert np.abs(got.transforms - host.transforms).max() <= 1e-5
    assert np.array_equal(np.isnan(got.inlier_rmse), np.isnan(host.inlier_rmse))
    ok = ~np.isnan(host.inlier_rmse)
    assert (np.abs(got.inlier_rmse[ok] - host.inlier_rmse[ok]) <= 1e-6).all()
    assert np.array_equal(got.transforms[2], np.eye(4)) and np.array_equal(got.transforms[3], np.eye(4))
    for p in range(2):                                                   # and the registration is right
        deg, metres = nc.pose_errors(got.transforms[p], c['g'][p])
        assert deg < 0.3 and metres < 0.05
    # the packed layout: one (M, 3) tensor of normals under the target's offsets
    s_off = np.concatenate([[0], np.cumsum([len(s) for s in c['srcs']])])
    t_off = np.concatenate([[0], np.cumsum([len(d) for d in c['dsts']])])
    flat = icp_refine((torch.cat(dev(c['srcs'])), s_off), (torch.cat(dev(c['dsts'])), t_off), max_correspondence_distance=1.0,
                      estimation='point_to_plane', target_normals=torch.cat(dev(c['nrms'])))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(flat, got))


def test_normals_straight_from_the_device():
    c = loop_batch()
    srcs, dsts = dev(c['srcs'][:2]), dev(c['dsts'][:2])
    nrms = estimate_normals(dsts, 20)
    assert all(n.is_cuda and n.dtype == torch.float32 for n in nrms)
    got = icp_refine(srcs, dsts, max_correspondence_distance=1.0, estimation='point_to_plane', target_normals=nrms)
    assert list(got.status) == [reg.CONVERGED, reg.CONVERGED]
    assert np.abs(got.transforms - c['host'].transforms[:2]).max() <= 1e-5
    point = icp_refine(srcs, dsts, max_correspondence_distance=1.0)
    for p in range(2):
        e_plane, e_point = nc.pose_errors(got.transforms[p], c['g'][p]), nc.pose_errors(point.transforms[p], c['g'][p])
        assert e_plane[0] < e_point[0] and e_plane[1] < e_point[1]


def test_two_runs_give_the_same_bits_and_the_default_is_point_to_point():
    c = loop_batch()
    args = (dev(c['srcs']), dev(c['dsts']))
    runs = [icp_refine(*args, max_correspondence_distance=1.0, estimation='point_to_plane', target_normals=dev(c['nrms']))
            for _ in range(2)]
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()
    one = [icp_correspondences(*args, runs[0].transforms, 1.0, target_normals=dev(c['nrms'])) for _ in range(2)]
    for a, b in zip(*one):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    default = icp_refine(*args, max_correspondence_distance=1.0)
    named = icp_refine(*args, max_correspondence_distance=1.0, estimation='point_to_point')
    for a, b in zip(default, named):
        assert a.tobytes() == b.tobytes()
    assert not np.array_equal(default.transforms[0], runs[0].transforms[0])


def test_arguments_are_refused():
    dst = rc.target(50)
    nrm = unit_normals(50, 1)
    with pytest.raises(_native.NativeLibraryError):
        icp_refine(dev([dst]), dev([dst]), estimation='point_to_plane', target_normals=[torch.from_numpy(nrm)])
    with pytest.raises(_native.NativeLibraryError):
        plane_update(torch.zeros((1, 29), dtype=torch.float64))
    with pytest.raises(TypeError):
        plane_update(torch.zeros((1, 17), dtype=torch.float64).cuda())
    for kw in (dict(estimation='plane'), dict(estimation='point_to_plane'), dict(target_normals=dev([nrm])),
               dict(estimation='point_to_plane', target_normals=dev([nrm[:-1]])),
               dict(estimation='point_to_plane', target_normals=dev([nrm])[0])):
        with pytest.raises(ValueError):
            icp_refine(dev([dst]), dev([dst]), **kw)
