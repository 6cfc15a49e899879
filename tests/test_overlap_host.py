"""Host side of the submap overlap (`hotformerloc_amd.overlap`): the pose helpers against hand-computed quaternions and a
grid at UTM magnitudes, and the numpy float64 route -- the truth of tests/test_gpu_overlap.py -- against closed forms: a
lattice with known distances, a cloud against itself, a copy shifted by s along x, the empty-cloud conventions, chunked
against unchunked.  The reference stops at `TODO: dist = chamfer_distance(...)`, so there is no golden file.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import overlap_cases as oc
from hotformerloc_amd import (_native, chamfer_distance, chamfer_distance_host, feature_correspondences_host,
                              icp_correspondences_host, match_nearest_pose, nn_distances, nn_distances_host, ops, overlap_ratio,
                              overlap_ratio_host, pose_matrix, relative_pose, submap_overlap, submap_overlap_host,
                              transform_points, transform_points_host)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UTM = np.array([5.0e5, 6.9e6])


def lattice(n_side, spacing):
    g = np.arange(n_side) * spacing
    return np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- poses
def test_pose_matrix_hand_computed():
    h = np.sqrt(0.5)
    m = pose_matrix([[1.0, 2.0, 3.0, 0.0, 0.0, 0.0, 1.0],                 # identity rotation
                     [4.0, 5.0, 6.0, 0.0, 0.0, h, h],                     # 90 degrees about z
                     [7.0, 8.0, 9.0, 0.0, 0.0, 3.0, 3.0]])                # the same rotation, not normalised
    assert m.shape == (3, 4, 4) and m.dtype == np.float64
    assert np.array_equal(m[0], [[1, 0, 0, 1], [0, 1, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]])
    quarter = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    assert np.abs(m[1, :3, :3] - quarter).max() <= 1e-15 and np.array_equal(m[1, :3, 3], [4, 5, 6])
    assert np.abs(m[2, :3, :3] - quarter).max() <= 1e-15 and np.array_equal(m[2, :3, 3], [7, 8, 9])
    assert np.array_equal(m[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (3, 1)))
    # a general unit quaternion: 120 degrees about (1, 1, 1) sends x -> y -> z -> x
    cyc = pose_matrix([0.0, 0.0, 0.0, 0.5, 0.5, 0.5, 0.5])
    assert np.abs(cyc[:3, :3] - np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]])).max() <= 1e-15
    assert pose_matrix(np.zeros((2, 5, 7)) + [0, 0, 0, 0, 0, 0, 1]).shape == (2, 5, 4, 4)
    with pytest.raises(ValueError):
        pose_matrix([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        pose_matrix(np.zeros((3, 6)))


def test_relative_pose_identities():
    rng = np.random.RandomState(3)
    rows = np.concatenate([rng.uniform(0, 500, (2, 2)), rng.uniform(0, 50, (2, 1)), rng.normal(size=(2, 4))], 1)
    a, b = pose_matrix(rows)
    assert np.abs(relative_pose(a, a) - np.eye(4)).max() <= 1e-12
    assert np.abs(relative_pose(a, b) @ relative_pose(b, a) - np.eye(4)).max() <= 1e-12
    # the same poses at UTM magnitudes: inv(m) @ m carries the northing's float64 rounding, 6.9e6 * 2^-52 = 1.5e-9 m per
    # operation, through a handful of operations -- 1e-7 m is far below a float32 ulp of any submap coordinate (4e-6 m at 40 m)
    rows[:, :2] += UTM
    a, b = pose_matrix(rows)
    assert np.abs(relative_pose(a, a) - np.eye(4)).max() <= 1e-7
    assert np.abs(relative_pose(a, b) @ relative_pose(b, a) - np.eye(4)).max() <= 1e-7
    # frame a -> frame b: a point given in a, taken to the world and back into b
    p = np.array([3.0, -2.0, 1.0, 1.0])
    assert np.abs(relative_pose(a, b) @ p - np.linalg.solve(b, a @ p)).max() <= 1e-7
    assert relative_pose(np.stack([a, b]), np.stack([b, a])).shape == (2, 4, 4)      # batched


def test_match_nearest_pose_at_utm_magnitudes():
    gx, gy = np.meshgrid(np.arange(6) * 25.0, np.arange(5) * 25.0, indexing='ij')
    database = UTM + np.stack([gx.ravel(), gy.ravel()], 1)                            # 30 poses on a 25 m grid
    database[7, 1] += 0.35
    database = np.concatenate([database, database[[7]] + [0.0, 0.3]])                 # and one 0.3 m north of pose 7
    assert np.array_equal(database.astype(np.float32)[7], database.astype(np.float32)[30])    # which float32 would merge
    queries = np.stack([database[7] + [0.0, 0.1],                  # nearer pose 7 (0.1 m) than its neighbour (0.2 m)
                        database[7] + [0.0, 0.2],                  # nearer the neighbour
                        database[12] + [3.0, -4.0],                # 5 m from pose 12
                        database[29] + [8.0, 6.0],                 # 10 m from pose 29: on the cut, kept
                        database[29] + [8.0, 6.1],                 # just past it
                        UTM + [12.5, 0.0]])                        # midway between poses 0 and 5: the lower index
    got = match_nearest_pose(queries, database)
    assert got.dtype == np.int64 and got.tolist() == [7, 30, 12, 29, -1, -1]           # the midway query is 12.5 m from both
    assert match_nearest_pose(queries, database, max_dist=12.5).tolist() == [7, 30, 12, 29, 29, 0]
    assert match_nearest_pose(queries, database, max_dist=4.0).tolist() == [7, 30, -1, -1, -1, -1]
    assert match_nearest_pose(queries[:0], database).shape == (0,)


# ------------------------------------------------------------------------------------------------------------- host route
def test_nn_distances_host_on_a_lattice():
    t = lattice(5, 2.0)                                                     # 125 points, 2 m apart
    offsets = np.array([[0.5, 0.0, 0.0], [0.0, -0.75, 0.0], [0.25, 0.25, 0.5], [1.0, 0.0, 0.0]], np.float32)
    want = [0.5, 0.75, np.sqrt(0.375), 1.0]
    for shift, d in zip(offsets, want):
        inner = t[(t.min(1) >= 2.0) & (t.max(1) <= 6.0)]                    # queries next to interior points
        dist, idx, off = nn_distances_host([inner + shift], [t])
        assert dist.dtype == np.float64 and idx.dtype == np.int32 and off.tolist() == [0, inner.shape[0]]
        assert np.abs(dist - d).max() <= 1e-12
        # the lattice point each query was shifted from; the last shift lies midway between that point and its x neighbour,
        # which has the higher index (x is the slowest axis): the lower index of the two
        assert np.array_equal(t[idx], inner)


def test_chamfer_of_a_cloud_with_itself_and_with_a_shifted_copy():
    a = oc.forest(900, 1)
    r = chamfer_distance_host([a], [a])
    assert r.a_to_b[0] == 0.0 and r.b_to_a[0] == 0.0 and r.chamfer[0] == 0.0
    assert np.array_equal(overlap_ratio_host([a], [a], tau=0.0), [[1.0, 1.0]])
    s = 0.25                                                                # exact in float32; spacing 1 > 2 s
    t = lattice(6, 1.0)
    shifted = t + np.array([s, 0, 0], np.float32)
    r = chamfer_distance_host([t], [shifted])
    assert r.a_to_b[0] == s and r.b_to_a[0] == s and r.chamfer[0] == 2 * s
    r = chamfer_distance_host([t], [shifted], squared=True)
    assert r.a_to_b[0] == s * s and r.chamfer[0] == 2 * s * s
    # the same through `transforms`: the shift as a matrix on a
    m = np.eye(4)
    m[0, 3] = s
    assert chamfer_distance_host([t], [t], transforms=m[None]).chamfer[0] == 2 * s
    assert np.array_equal(overlap_ratio_host([t], [shifted], tau=s + 0.01), [[1.0, 1.0]])
    assert np.array_equal(overlap_ratio_host([t], [shifted], tau=s - 0.01), [[0.0, 0.0]])
    both = overlap_ratio_host([t], [shifted], tau=(s - 0.01, s, 1.0))       # d <= tau: the threshold itself counts
    assert both.shape == (1, 2, 3) and np.array_equal(both[0], [[0, 1, 1], [0, 1, 1]])


def test_empty_cloud_conventions():
    a, b = oc.ragged_pairs(4)                                               # pair 1: a empty, pair 2: b empty
    dist, idx, off = nn_distances_host(a, b)
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(c) for c in a])]).tolist()
    assert np.isinf(dist[off[2]:off[3]]).all() and (idx[off[2]:off[3]] == -1).all()
    assert np.isfinite(np.delete(dist, np.arange(off[2], off[3]))).all() and off[1] == off[2]
    r = chamfer_distance_host(a, b)
    assert np.isnan(r.chamfer[[1, 2]]).all() and np.isfinite(r.chamfer[[0, 3, 4]]).all()
    assert np.isnan(r.a_to_b[[1, 2]]).all() and np.isnan(r.b_to_a[[1, 2]]).all()
    ov = overlap_ratio_host(a, b, tau=oc.TAU)
    assert ov.shape == (5, 2)
    assert np.isnan(ov[1, 0]) and ov[1, 1] == 0.0                           # an empty cloud's share; a share against nothing
    assert ov[2, 0] == 0.0 and np.isnan(ov[2, 1])
    assert ((ov[[0, 3, 4]] > 0.0) & (ov[[0, 3, 4]] <= 1.0)).all()
    poses = np.tile(np.eye(4), (5, 1, 1))
    res = submap_overlap_host(a, b, poses, poses)
    assert res.n_pairs == 3 and res.mean_chamfer == r.chamfer[[0, 3, 4]].mean()
    assert np.array_equal(res.mean_overlap, ov[[0, 3, 4]].mean(0))


def test_chunked_equals_unchunked():
    a, b = oc.ragged_pairs(6)
    whole = nn_distances_host(a, b)
    for chunk in (1, 777, 5000):
        part = nn_distances_host(a, b, chunk_pairs=chunk)
        assert all(np.array_equal(x, y) for x, y in zip(part, whole))
    # and the concatenated form equals the list form
    cat = lambda cl: (np.concatenate(cl), np.concatenate([[0], np.cumsum([len(c) for c in cl])]))      # noqa: E731
    assert all(np.array_equal(x, y) for x, y in zip(nn_distances_host(cat(a), cat(b)), whole))


def test_duplicates_take_the_lowest_index():
    t, lowest = oc.with_duplicates(oc.forest(600, 8), 9)
    assert (lowest < np.arange(600)).sum() >= 30
    dist, idx, _ = nn_distances_host([t], [t])
    assert (dist == 0.0).all() and np.array_equal(idx, lowest)


def test_transform_points_host_rounds_once():
    a, _ = oc.ragged_pairs(11)
    ms = np.stack([oc.rigid(20 + p) for p in range(5)])
    out = transform_points_host(a, ms)
    assert [o.shape for o in out] == [c.shape for c in a] and all(o.dtype == np.float32 for o in out)
    for c, m, o in zip(a, ms, out):
        assert np.array_equal(o, (c.astype(np.float64) @ m[:3, :3].T + m[:3, 3]).astype(np.float32))
    flat = transform_points_host((np.concatenate(a), np.concatenate([[0], np.cumsum([len(c) for c in a])])), ms[:, :3])
    assert np.array_equal(flat, np.concatenate(out))                        # (P, 3, 4) matrices, the concatenated layout


def test_tile_table():
    q = ops.OVERLAP_ROWS
    tiles = ops.overlap_tiles([0, 1, q, q + 1, 0, 2 * q + 1])
    assert tiles.dtype == np.int64
    assert tiles.tolist() == [[1, 0], [2, 1], [3, q + 1], [3, 2 * q + 1], [5, 2 * q + 2], [5, 3 * q + 2], [5, 4 * q + 2]]
    assert ops.overlap_tiles([0, 0]).shape == (0, 2)
    header = open(os.path.join(ROOT, 'include', 'hotformerloc_hip.h')).read()
    for name in ('ROWS', 'TILE', 'MAX_TAUS'):                               # the constants ops exports are the header's
        assert int(re.search(r'#define HFL_OVERLAP_%s (\d+)' % name, header).group(1)) == getattr(ops, 'OVERLAP_' + name)
    assert ops.OVERLAP_ROWS % 256 == 0 and ops.OVERLAP_TILE * 12 <= 32 * 1024
    # `feature_tiles` is this table: the workgroups of hfl_feature_nn own the rows of those of hfl_nn_dist
    assert ops.FEATURE_ROWS == ops.OVERLAP_ROWS
    assert ops.feature_tiles([3, 0, q + 1]).tolist() == ops.overlap_tiles([3, 0, q + 1]).tolist()
    assert int(re.search(r'#define HFL_FEATURE_ROWS (\d+)', header).group(1)) == ops.OVERLAP_ROWS
    both, tile_off = ops.pair_tiles([0, 1, q, q + 1, 0, 2 * q + 1])        # the table and every pair's rows in it
    assert np.array_equal(both, tiles) and tile_off.tolist() == [0, 0, 1, 2, 4, 4, 7]


def test_host_twins_of_the_pair_scan_agree_bit_for_bit():
    """The host side of tests/test_gpu_pair_scan.py: the fp32 twin of `hfl_nn_dist` (through `icp_correspondences_host` at
    the identity pose) and the twin of `hfl_feature_nn` at D = 3 pick the same rows at the same distances, and so give the
    same mutual mask."""
    bits = lambda x: np.ascontiguousarray(x, np.float32).view(np.uint32)      # noqa: E731
    offsets = lambda clouds: np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)      # noqa: E731
    batches, lowest = oc.pair_scan_batches(ops.OVERLAP_ROWS, ops.OVERLAP_TILE)
    for src, dst in batches:
        eye = np.tile(np.eye(4), (len(src), 1, 1))
        dist, idx, _, _ = icp_correspondences_host(src, dst, eye, 1.0)
        back = icp_correspondences_host(dst, src, eye, 1.0)[1]
        f_idx, f_d2, f_mask = (np.concatenate(x) for x in feature_correspondences_host(src, dst, mutual=True))
        assert dist.dtype == np.float32 and f_d2.dtype == np.float32 and np.array_equal(f_idx, idx)
        assert np.array_equal(bits(np.sqrt(f_d2)), bits(dist))
        want = oc.mutual_from_indices(idx, back, offsets(src), offsets(dst))
        assert np.array_equal(f_mask, want) and want.any() and not want.all()
        empty = np.repeat([len(c) == 0 for c in dst], [len(c) for c in src])
        assert np.array_equal(idx == -1, empty) and np.array_equal(np.isinf(dist), empty)
    assert idx[0] == lowest and dist[0] == 0.0                              # the tie across a tile edge: the lowest copy


def test_device_functions_refuse_cpu_tensors_and_float64_points():
    a, b = oc.ragged_pairs(2)
    ta, tb = [torch.from_numpy(c) for c in a], [torch.from_numpy(c) for c in b]
    eye = np.tile(np.eye(4), (5, 1, 1))
    for call in (lambda: transform_points(ta, eye), lambda: nn_distances(ta, tb), lambda: chamfer_distance(ta, tb),
                 lambda: overlap_ratio(ta, tb), lambda: submap_overlap(ta, tb, eye, eye),
                 lambda: nn_distances((torch.cat(ta), torch.tensor([0, 700, 700, 2000, 2040, 2555])), tb)):
        with pytest.raises(_native.NativeLibraryError):
            call()
    with pytest.raises(TypeError, match='transform_points'):                # float64 points: an error that says what to do
        chamfer_distance([c.double() for c in ta], tb)
    with pytest.raises(TypeError, match='transform_points'):
        nn_distances_host([c.astype(np.float64) for c in a], b)
    with pytest.raises(ValueError):
        nn_distances_host(a[:4], b)                                         # the batches do not pair up
    with pytest.raises(ValueError):
        nn_distances_host((np.concatenate(a), np.array([0, 10, 5, 2555])), b[:3])       # decreasing offsets
    with pytest.raises(ValueError):
        transform_points_host(a, eye[:4])
    with pytest.raises(ValueError):
        overlap_ratio_host(a, b, tau=-1.0)
