"""Time rigid ICP of a split's worth of submap pairs by three routes: 64 pairs of 30 000 x 30 000 points.

Synthetic only: the forest-like scenes of tools/submap_overlap_probe.py, the target cloud one sampling of a scene, the source
another sampling of it given in a frame a degree and a few decimetres away, as a ground submap is after its surveyed pose.

  fused      one iteration of `icp_refine`: `hfl_icp_correspond` + `hfl_icp_solve` for the whole batch, every pair RUNNING,
             `--launches` iterations back to back between two HIP events.
  assembled  the same iteration from the public pieces that predate the fused kernels: `ops.transform_points`, `ops.nn_dist`,
             a torch gather of the winners and torch reductions to the 17 sums per pair, all on the device, between the same
             events.  The solve is NOT included (it would be a host SVD and a synchronisation), so this route is timed to its
             advantage.
  call       the whole `icp_refine(source, target)` from device clouds with its defaults: uploads, max_iterations + 1 rounds,
             one read of the results; wall clock with a device synchronisation on both sides.
  ckdtree    point-to-point ICP with `scipy.spatial.cKDTree` and `numpy.linalg.svd` on the first `--tree-pairs` pairs, in
             float64, the same stop rules, scaled to the whole batch (every pair has the same size); where scipy is importable.

Median / min / max of `--repeats` measurements after `--warmup`; the CPU route runs once.  The fused route's poses of the
timed pairs are compared with the tree route's.  One JSON line.  Run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hotformerloc_amd import icp_refine, ops, transform_points_host      # noqa: E402
from hotformerloc_amd import registration as reg                         # noqa: E402
from submap_overlap_probe import scene, spread                           # noqa: E402

MAX_DIST = 0.8


def small_motion(seed):
    """a degree about a seeded axis and 0.3 m"""
    rng = np.random.RandomState(seed)
    k = rng.normal(size=3)
    k /= np.linalg.norm(k)
    kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    a = np.radians(1.0)
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(a) * kx + (1.0 - np.cos(a)) * (kx @ kx)
    m[:3, 3] = 0.3 * rng.normal(size=3) / np.sqrt(3.0)
    return m


def tree_icp(src, dst, max_iterations=30, tol=1e-6):
    """float64 point-to-point ICP with a k-d tree: (pose, fitness, rmse, iterations)"""
    from scipy.spatial import cKDTree
    src, dst = src.astype(np.float64), dst.astype(np.float64)
    tree, pose, prev = cKDTree(dst), np.eye(4), None
    for k in range(max_iterations + 1):
        moved = src @ pose[:3, :3].T + pose[:3, 3]
        d, j = tree.query(moved)
        inl = d <= MAX_DIST
        n = int(inl.sum())
        fitness, rmse = n / len(src), float(np.sqrt((d[inl] ** 2).sum() / max(n, 1)))
        if n < 3 or k == max_iterations or (prev is not None and abs(fitness - prev[0]) < tol and abs(rmse - prev[1]) < tol):
            break
        prev = (fitness, rmse)
        p, q = moved[inl], dst[j[inl]]
        h = (p - p.mean(0)).T @ (q - q.mean(0))
        u, _, vt = np.linalg.svd(h)
        r = vt.T @ np.diag([1.0, 1.0, np.sign(np.linalg.det(vt.T @ u.T))]) @ u.T
        step = np.eye(4)
        step[:3, :3], step[:3, 3] = r, q.mean(0) - r @ p.mean(0)
        pose = step @ pose
    return pose, fitness, rmse, k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=64)
    ap.add_argument('--points', type=int, default=30000)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--launches', type=int, default=3)
    ap.add_argument('--tree-pairs', type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('registration_probe needs a GPU: nothing is timed without one')
    n, pairs = args.points, args.pairs
    source, target = [], []
    for p in range(pairs):
        air, seen = scene(n, p)
        source.append(transform_points_host([seen], np.linalg.inv(small_motion(1000 + p))[None])[0])
        target.append(air)
    d_source, d_target = [torch.from_numpy(c).cuda() for c in source], [torch.from_numpy(c).cuda() for c in target]
    res = {'pairs': pairs, 'points_per_cloud': n, 'pair_tests_per_iteration': pairs * n * n, 'max_correspondence_distance': MAX_DIST}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(body):
        per = []
        for i in range(args.warmup + args.repeats):
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.launches):
                body()
            e1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                per.append(e0.elapsed_time(e1) / args.launches)
        out = spread(per)
        out.update({'Tpairs_per_s': round(pairs * n * n / (statistics.median(per) * 1e-3) / 1e12, 3),
                    'how': '%d back-to-back iterations between two HIP events' % args.launches})
        return out

    # one fused iteration, every pair RUNNING at the identity
    batch = reg._Batch(d_source, d_target, 'registration_probe')
    identity = np.tile(np.eye(4)[:3], (pairs, 1, 1))
    state, istate = batch.state(identity)

    def fused():
        istate.zero_()                                                   # an update leaves the pair RUNNING; keep k = 0
        batch.correspond(state, istate, MAX_DIST)
        batch.solve(state, istate, 3, 1e-6, 1e-6, False)

    res['fused_iteration'] = timed(fused)
    res['fused_iteration']['workgroups'] = batch.n_tiles

    # the same iteration from transform_points + nn_dist + torch
    q, t = batch.s, batch.t
    m32 = torch.from_numpy(identity.reshape(pairs, 12).astype(np.float32)).cuda()
    tiles = batch.tiles
    owner = torch.repeat_interleave(torch.arange(pairs, device='cuda'), n)
    t_first = batch.t_dev[:-1][owner]
    sums = {}

    def assembled():
        moved = ops.transform_points(q, batch.s_dev, m32)
        dist, idx = ops.nn_dist(moved, batch.s_dev, t, batch.t_dev, tiles)
        inl = ((idx >= 0) & (dist <= MAX_DIST)).to(torch.float64)[:, None]
        won = t[(t_first + idx.clamp(min=0)).long()].to(torch.float64) * inl
        mv = moved.to(torch.float64) * inl
        d = dist.to(torch.float64)[:, None] * inl
        rows = torch.cat([inl, mv, won, (mv[:, :, None] * won[:, None, :]).reshape(-1, 9), d * d], 1)
        sums['assembled'] = rows.reshape(pairs, n, reg.N_SUMS).sum(1)

    res['assembled_iteration'] = timed(assembled)
    res['assembled_over_fused'] = round(res['assembled_iteration']['median_ms'] / res['fused_iteration']['median_ms'], 3)
    # the two routes reduce the same rows
    istate.zero_()
    state.copy_(batch.state(identity)[0])
    batch.correspond(state, istate, MAX_DIST)
    fused_sums = batch.solve(state, istate, 3, 1e-6, 1e-6, True, want_sums=True)
    scale = sums['assembled'].abs().amax(0).clamp(min=1.0)
    res['routes_agree'] = {'inlier_counts_equal': bool((fused_sums[:, 0] == sums['assembled'][:, 0]).all()),
                           'max_sum_difference_over_scale': float(((fused_sums - sums['assembled']).abs() / scale).max())}

    # the whole call
    ms = []
    for i in range(args.warmup + args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = icp_refine(d_source, d_target, max_correspondence_distance=MAX_DIST)
        torch.cuda.synchronize()
        if i >= args.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    res['icp_refine_call'] = spread(ms)
    res['icp_refine_call'].update({'rounds': 31, 'iterations_min': int(got.iterations.min()), 'iterations_max': int(got.iterations.max()),
                                   'status_counts': np.bincount(got.status, minlength=5).tolist(),
                                   'mean_fitness': round(float(got.fitness.mean()), 4),
                                   'mean_inlier_rmse': round(float(np.nanmean(got.inlier_rmse)), 4)})

    try:
        import scipy.spatial      # noqa: F401
    except ImportError:
        res['ckdtree'] = 'scipy is not importable'
    else:
        k = min(args.tree_pairs, pairs)
        t0 = time.perf_counter()
        tree = [tree_icp(source[p], target[p]) for p in range(k)]
        tree_ms = (time.perf_counter() - t0) * 1e3
        res['ckdtree'] = {'pairs': k, 'ms': round(tree_ms, 1), 'ms_scaled_to_batch': round(tree_ms * pairs / k, 1),
                          'iterations': [x[3] for x in tree],
                          'max_pose_difference_to_device': float(max(np.abs(x[0] - got.transforms[p]).max() for p, x in enumerate(tree)))}
        res['speedup_vs_ckdtree'] = round(res['ckdtree']['ms_scaled_to_batch'] / res['icp_refine_call']['median_ms'], 1)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
