"""`hfl_transform_points`, `hfl_nn_dist` and `hfl_pair_stats` (hotformerloc_amd/csrc/overlap.hip) through
`hotformerloc_amd.overlap` against the numpy float64 route.

Distances: |d_dev - d_host| <= 1e-6 d_host.  The difference, the three-term fma sum and the square root carry under
3 * 2^-24 relative error; 1e-6 is about 5x that.  Exact zeros are exactly zero.  Indices: the float64 distance from the
query to dst[idx_dev] meets the same bound against the host minimum; on exact duplicates the index is the lowest one.
Transform: <= 4 ulp32(L) per coordinate, L the case's largest coordinate magnitude after the transform (three fmaf roundings
on intermediates of at most 2L are at most 3 ulp).  Chamfer with transforms: both routes start from their own transformed
cloud, a point of which differs by at most sqrt(3) * 4 ulp32(L) between them, and a nearest-neighbour distance moves by no
more than its query and its target do: the sum of the two bounds per direction.  Sums and counts of `hfl_pair_stats`:
against numpy on the device's own float32 distances, counts equal, sums to 1e-12; against the host route a count may
differ only by points whose host distance lies within 1e-6 tau of tau -- the seeds leave none there, which is asserted, so
the shares are compared for equality."""
import numpy as np
import pytest
import torch

import overlap_cases as oc
from hotformerloc_amd import (chamfer_distance, chamfer_distance_host, nn_distances, nn_distances_host, ops, overlap_ratio,
                              overlap_ratio_host, pose_matrix, relative_pose, submap_overlap, transform_points,
                              transform_points_host)

pytestmark = pytest.mark.gpu

T, Q = ops.OVERLAP_TILE, ops.OVERLAP_ROWS
TAUS = (0.4, oc.TAU, 2.0)
_CACHE = {}


def dev(clouds):
    return [torch.from_numpy(c).cuda() for c in clouds]


def check_nn(src, dst):
    """device against host for one ragged batch of pairs; returns (host dist, device dist, device idx) as numpy"""
    want_d, want_i, want_off = nn_distances_host(src, dst)
    dist, idx, off = nn_distances(dev(src), dev(dst))
    torch.cuda.synchronize()
    assert dist.is_cuda and dist.dtype == torch.float32 and idx.dtype == torch.int32 and off.dtype == torch.int64
    assert np.array_equal(off.cpu().numpy(), want_off)
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    assert dist.shape == want_d.shape and idx.shape == want_i.shape
    empty = np.isinf(want_d)
    assert np.array_equal(np.isinf(dist), empty) and (idx[empty] == -1).all()
    assert (np.abs(dist[~empty] - want_d[~empty]) <= oc.DIST_RTOL * want_d[~empty]).all()          # zero stays zero
    for p in range(len(src)):                                            # the index names a point at that distance
        rows = slice(want_off[p], want_off[p + 1])
        if len(dst[p]) and len(src[p]):
            k = idx[rows]
            assert (k >= 0).all() and (k < len(dst[p])).all()
            at = np.sqrt(((src[p].astype(np.float64) - dst[p][k].astype(np.float64)) ** 2).sum(1))
            assert (np.abs(at - want_d[rows]) <= oc.DIST_RTOL * want_d[rows]).all()
    return want_d, dist, idx


@pytest.mark.parametrize('m', [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1])
def test_target_sizes_around_the_tile(m):
    dst = oc.forest(m, 100 + m)
    src = oc.forest(Q + 1, 200 + m)
    src[0] = dst[m - 1]                                                  # a hit on the last target: past a tile edge
    src[1] = dst[0]
    want, dist, idx = check_nn([src], [dst])
    assert dist[0] == 0.0 and dist[1] == 0.0 and (dst[idx[:2]] == src[:2]).all()


@pytest.mark.parametrize('n', [1, Q - 1, Q, Q + 1, 3 * Q + 1])
def test_query_counts_around_the_workgroup(n):
    dst = oc.forest(T + 70, 300 + n)
    src = oc.forest(n, 400 + n)
    src[n - 1] = dst[T + 69]                                             # the last query hits the last target
    want, dist, idx = check_nn([src], [dst])
    assert dist[n - 1] == 0.0 and (dst[idx[n - 1]] == src[n - 1]).all()


def test_duplicates_take_the_lowest_index():
    dst, lowest = oc.with_duplicates(oc.forest(T + 300, 7), 8)           # copies on both sides of the tile edge
    assert (lowest < np.arange(dst.shape[0])).sum() > 100 and (lowest[T:] < T).any()
    want, dist, idx = check_nn([dst], [dst])
    assert (dist == 0.0).all() and np.array_equal(idx, lowest)
    # and between two different clouds: equal distances to two copies of one target
    src = oc.forest(700, 9)
    _, _, idx = check_nn([src], [dst])
    assert np.array_equal(idx, nn_distances_host([src], [dst])[1]) and np.array_equal(lowest[idx], idx)


def ragged():
    """the P = 5 batch (an empty query cloud and an empty target cloud in the middle), its rigid transforms and the host
    route's figures, computed once"""
    if 'ragged' not in _CACHE:
        a, b = oc.ragged_pairs(31)
        ms = np.stack([oc.rigid(50 + p, max_shift=0.3) for p in range(5)])
        moved = transform_points_host(a, ms)
        _CACHE['ragged'] = dict(a=a, b=b, ms=ms, moved=moved, chamfer=chamfer_distance_host(a, b, ms),
                                chamfer2=chamfer_distance_host(a, b, squared=True), plain=chamfer_distance_host(a, b),
                                overlap=overlap_ratio_host(a, b, ms, TAUS),
                                d_ab=nn_distances_host(moved, b)[0], d_ba=nn_distances_host(b, moved)[0])
    return _CACHE['ragged']


def test_ragged_batch_with_empty_clouds():
    r = ragged()
    check_nn(r['a'], r['b'])
    check_nn(r['b'], r['a'])
    check_nn(r['a'][:1], r['b'][:1])                                     # P = 1
    points = torch.from_numpy(np.concatenate(r['a'])).cuda()             # the concatenated layout
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum([len(c) for c in r['a']])]))
    dist, idx, _ = nn_distances((points, offsets), dev(r['b']))
    want = nn_distances(dev(r['a']), dev(r['b']))
    assert torch.equal(dist, want[0]) and torch.equal(idx, want[1])


def transform_bound(clouds, ms):
    return oc.TRANSFORM_ULPS * oc.ulp32(oc.max_abs_after(clouds, ms))


def test_transform_points():
    r = ragged()
    got = transform_points(dev(r['a']), r['ms'])
    assert isinstance(got, list) and [tuple(g.shape) for g in got] == [c.shape for c in r['a']]
    bound = transform_bound(r['a'], r['ms'])
    for g, c, m in zip(got, r['a'], r['ms']):
        exact = c.astype(np.float64) @ m[:3, :3].T + m[:3, 3]
        assert g.dtype == torch.float32 and (np.abs(g.cpu().numpy().astype(np.float64) - exact) <= bound).all()
    # clouds at the +-64 m edge, a larger shift, (P, 3, 4) matrices as a tensor, the concatenated layout
    big = [oc.forest(3000, 60, extent=64.0), oc.forest(257, 61, extent=64.0)]
    ms = np.stack([oc.rigid(62), oc.non_rigid()])
    flat = transform_points((torch.from_numpy(np.concatenate(big)).cuda(), torch.tensor([0, 3000, 3257])),
                            torch.from_numpy(ms[:, :3]))
    exact = np.concatenate([c.astype(np.float64) @ m[:3, :3].T + m[:3, 3] for c, m in zip(big, ms)])
    assert tuple(flat.shape) == (3257, 3)
    assert (np.abs(flat.cpu().numpy().astype(np.float64) - exact) <= transform_bound(big, ms)).all()
    eye = transform_points(dev(big), np.tile(np.eye(4), (2, 1, 1)))      # the identity moves nothing
    assert all(np.array_equal(e.cpu().numpy(), c) for e, c in zip(eye, big))


def chamfer_close(got, want, slack):
    """per direction |got - want| <= 1e-6 want + slack, NaN where the host has NaN"""
    for g, w, n in ((got.a_to_b, want.a_to_b, 1), (got.b_to_a, want.b_to_a, 1), (got.chamfer, want.chamfer, 2)):
        assert g.is_cuda and g.dtype == torch.float64
        g = g.cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(w))
        ok = ~np.isnan(w)
        assert (np.abs(g[ok] - w[ok]) <= oc.DIST_RTOL * w[ok] + n * slack).all(), (g, w)


def test_chamfer_distance():
    r = ragged()
    a, b = dev(r['a']), dev(r['b'])
    chamfer_close(chamfer_distance(a, b), r['plain'], 0.0)
    assert np.isnan(r['plain'].chamfer[[1, 2]]).all()                    # the empty clouds of pairs 1 and 2
    got, want = chamfer_distance(a, b, squared=True), r['chamfer2']      # (1 + 1e-6)^2 - 1 on a squared distance
    for g, w in zip(got, want):
        ok = ~np.isnan(w)
        assert (np.abs(g.cpu().numpy()[ok] - w[ok]) <= ((1 + oc.DIST_RTOL) ** 2 - 1) * w[ok]).all()
    shift = np.sqrt(3.0) * transform_bound(r['a'], r['ms'])              # how far a transformed point differs between routes
    chamfer_close(chamfer_distance(a, b, r['ms']), r['chamfer'], shift)


def test_pair_stats_and_overlap_ratio():
    r = ragged()
    moved = transform_points(dev(r['a']), r['ms'])
    b = dev(r['b'])
    for src, dst in ((moved, b), (b, moved)):
        dist, _, off = nn_distances(src, dst)
        sums, counts = ops.pair_stats(dist, off, TAUS)
        d, off_h = dist.cpu().numpy(), off.cpu().numpy()
        for p in range(5):                                               # numpy on the device's own float32 distances
            row = d[off_h[p]:off_h[p + 1]]
            fin = row[np.isfinite(row)]
            assert counts[p].tolist() == [int((fin <= np.float32(t)).sum()) for t in TAUS] + [int(np.isinf(row).sum())]
            for got, want in zip(sums[p].tolist(), (fin.astype(np.float64).sum(), (fin.astype(np.float64) ** 2).sum())):
                assert abs(got - want) <= 1e-12 * want
    # against the host route: no host distance lies within 1e-6 tau of a tau, so the counts cannot differ
    for t in TAUS:
        assert oc.clear_of_tau(r['d_ab'], t) and oc.clear_of_tau(r['d_ba'], t)
    got = overlap_ratio(dev(r['a']), b, r['ms'], TAUS)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (5, 2, 3)
    assert np.array_equal(got.cpu().numpy(), r['overlap'], equal_nan=True)
    assert np.isnan(r['overlap'][1, 0]).all() and (r['overlap'][1, 1] == 0).all()      # empty a: NaN its share, 0 against it
    one = overlap_ratio(dev(r['a']), b, r['ms'])                         # the default tau: one threshold, (P, 2)
    assert tuple(one.shape) == (5, 2) and np.array_equal(one.cpu().numpy(), r['overlap'][:, :, 1], equal_nan=True)
    some = r['overlap'][[0, 3, 4]]
    assert (some[..., 2] > 0.05).all() and (some[..., 0] < some[..., 2]).all()         # the thresholds tell points apart


def test_non_rigid_matrix_is_applied_once():
    """b -> a must run against the transformed cloud a; with the inverse matrix on b instead, distances come out in a's
    stretched frame and differ far beyond the tolerance"""
    a, b = [oc.forest(1500, 70, extent=12.0)], [oc.forest(1100, 71, extent=12.0)]
    m = oc.non_rigid()[None]
    want = chamfer_distance_host(a, b, m)
    wrong = chamfer_distance_host(b, a, np.linalg.inv(m)).a_to_b         # b pulled into a's frame
    shift = np.sqrt(3.0) * transform_bound(a, m)
    assert abs(wrong[0] - want.b_to_a[0]) > 100 * (oc.DIST_RTOL * want.b_to_a[0] + shift)       # the case tells them apart
    chamfer_close(chamfer_distance(dev(a), dev(b), m), want, shift)
    d_ab, d_ba = nn_distances_host(transform_points_host(a, m), b)[0], nn_distances_host(b, transform_points_host(a, m))[0]
    assert oc.clear_of_tau(d_ab, oc.TAU) and oc.clear_of_tau(d_ba, oc.TAU)
    assert np.array_equal(overlap_ratio(dev(a), dev(b), m).cpu().numpy(), overlap_ratio_host(a, b, m))


def test_two_runs_give_the_same_bits():
    r = ragged()
    a, b = dev(r['a']), dev(r['b'])

    def run():
        moved = transform_points(a, r['ms'])
        dist, idx, off = nn_distances(moved, b)
        sums, counts = ops.pair_stats(dist, off, TAUS)
        c = chamfer_distance(a, b, r['ms'])
        return [torch.cat(moved), dist, idx, sums, counts, c.a_to_b, c.b_to_a, overlap_ratio(a, b, r['ms'], TAUS)]

    first, second = run(), run()
    for x, y in zip(first, second):
        assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))


def test_submap_overlap_end_to_end():
    """three pairs built from one cloud each, seen from two poses at UTM magnitudes: the ground submap aligned into the
    aerial frame is the aerial submap again, up to the float32 rounding of the ground points (half an ulp per coordinate,
    carried through a rotation) and of the transform (4 ulp): overlap 1, Chamfer below sqrt(3) * 4.5 ulp32(L) per direction"""
    rng = np.random.RandomState(5)
    aerial = [oc.forest(n, 80 + p) for p, n in enumerate((1200, 2500, 600))]
    utm = np.array([5.0e5, 6.9e6, 40.0])
    yaw = rng.uniform(-np.pi, np.pi, (2, 3))
    quat = lambda a: np.stack([0 * a, 0 * a, np.sin(a / 2), np.cos(a / 2)], 1)            # noqa: E731
    aerial_poses = np.concatenate([utm + rng.uniform(0, 300, (3, 3)), quat(yaw[0])], 1)
    ground_poses = np.concatenate([aerial_poses[:, :3] + rng.uniform(-5, 5, (3, 3)), quat(yaw[1])], 1)
    to_ground = relative_pose(pose_matrix(aerial_poses), pose_matrix(ground_poses))            # float64, rounded once
    ground = transform_points_host(aerial, to_ground)
    res = submap_overlap(dev(ground), dev(aerial), ground_poses, aerial_poses)
    assert res.n_pairs == 3 and res.transforms.shape == (3, 4, 4)
    assert np.abs(res.transforms @ to_ground - np.eye(4)).max() <= 1e-7                        # see test_overlap_host
    big = max(oc.max_abs_after(ground, res.transforms), max(float(np.abs(g).max()) for g in ground))
    bound = np.sqrt(3.0) * 4.5 * oc.ulp32(big) + 1e-7
    for side in (res.chamfer.a_to_b, res.chamfer.b_to_a):
        assert (side.cpu().numpy() <= bound * (1 + oc.DIST_RTOL)).all()
    assert (res.chamfer.chamfer.cpu().numpy() <= 2 * bound * (1 + oc.DIST_RTOL)).all()
    assert np.array_equal(res.overlap.cpu().numpy(), np.ones((3, 2)))
    assert res.mean_chamfer <= 2 * bound * (1 + oc.DIST_RTOL) and np.array_equal(res.mean_overlap, [1.0, 1.0])
    assert res.mean_chamfer == float(res.chamfer.chamfer.cpu().numpy().mean())
