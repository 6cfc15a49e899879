"""Time the Chamfer distance of a split's worth of ground/aerial pairs by three routes: 64 pairs of 30 000 x 30 000 points.

Synthetic only: forest-like clouds inside +-40 m (a rough ground sheet, trunks, canopy), the aerial cloud a re-sampling of
the same scene, the ground cloud given in its own frame a few metres and a yaw away, as a CS-Wild-Places pair is.

  device   `hfl_nn_dist` alone: `--launches` back-to-back launches of one direction of the whole batch between two HIP
           events, against the point pairs tested (sum of N_p * M_p) -- a pair-test rate, not a share of peak.  And the
           whole `chamfer_distance(ground, aerial, transforms)` from device clouds: the offset and tile-table uploads, the
           transform, both directions, both reductions; wall clock with a device synchronisation on both sides.
  host     `chamfer_distance_host` on the first `--host-pairs` pairs: the same brute force in numpy float64.
  ckdtree  `scipy.spatial.cKDTree` on the first `--tree-pairs` pairs, both directions (build + query), where scipy is
           importable; on the float32 points widened to float64, after the host transform.

Median / min / max of `--repeats` calls after `--warmup`; the CPU routes run once.  The per-pair times of the CPU routes are
scaled to the whole batch for the speed-up figures (every pair has the same size).  The device Chamfer of the timed pairs is
compared with the host's.  One JSON line.  Run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hotformerloc_amd import chamfer_distance, chamfer_distance_host, ops, transform_points_host      # noqa: E402


def scene(n, seed, extent=40.0):
    """two samplings (n points each, float32) of one forest-like scene"""
    rng = np.random.RandomState(seed)
    trees = rng.uniform(-extent, extent, (400, 2))

    def sample():
        k = n // 3
        ground = np.concatenate([rng.uniform(-extent, extent, (n - 2 * k, 2)), rng.normal(0.0, 0.15, (n - 2 * k, 1))], 1)
        t = trees[rng.randint(0, 400, k)]
        trunk = np.concatenate([t + rng.normal(0.0, 0.2, t.shape), rng.uniform(0.0, 12.0, (k, 1))], 1)
        c = trees[rng.randint(0, 400, k)]
        canopy = np.concatenate([c + rng.normal(0.0, 2.0, c.shape), rng.normal(15.0, 2.5, (k, 1))], 1)
        return np.concatenate([ground, trunk, canopy], 0)[rng.permutation(n)]

    return sample().astype(np.float32), sample().astype(np.float32)


def yaw_shift(seed):
    rng = np.random.RandomState(seed)
    a = rng.uniform(-np.pi, np.pi)
    m = np.eye(4)
    m[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    m[:3, 3] = rng.uniform(-5.0, 5.0, 3)
    return m


def spread(ms):
    return {'median_ms': round(statistics.median(ms), 3), 'min_ms': round(min(ms), 3), 'max_ms': round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=64)
    ap.add_argument('--points', type=int, default=30000)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--launches', type=int, default=3)
    ap.add_argument('--host-pairs', type=int, default=1)
    ap.add_argument('--tree-pairs', type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('submap_overlap_probe needs a GPU: nothing is timed without one')
    n, pairs = args.points, args.pairs
    aerial, ground, to_aerial = [], [], []
    for p in range(pairs):
        air, seen = scene(n, p)
        m = yaw_shift(1000 + p)                                          # ground frame -> aerial frame
        ground.append(transform_points_host([seen], np.linalg.inv(m)[None])[0])
        aerial.append(air)
        to_aerial.append(m)
    to_aerial = np.stack(to_aerial)
    d_ground, d_aerial = [torch.from_numpy(c).cuda() for c in ground], [torch.from_numpy(c).cuda() for c in aerial]
    res = {'pairs': pairs, 'points_per_cloud': n, 'pair_tests_per_direction': pairs * n * n}

    # the whole call
    ms = []
    for i in range(args.warmup + args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = chamfer_distance(d_ground, d_aerial, to_aerial)
        torch.cuda.synchronize()
        if i >= args.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    res['device_chamfer_call'] = spread(ms)
    res['device_chamfer_call']['Tpairs_per_s'] = round(2 * pairs * n * n / (statistics.median(ms) * 1e-3) / 1e12, 3)

    # hfl_nn_dist alone, one direction of the whole batch
    q, t = torch.cat(d_ground), torch.cat(d_aerial)
    off = torch.arange(pairs + 1, dtype=torch.int64, device='cuda') * n
    tiles = torch.from_numpy(ops.overlap_tiles([n] * pairs)).cuda()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = []
    for i in range(args.warmup + args.repeats):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.launches):
            ops.nn_dist(q, off, t, off, tiles)
        e1.record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            per.append(e0.elapsed_time(e1) / args.launches)
    res['nn_dist_launch'] = spread(per)
    res['nn_dist_launch'].update({'workgroups': int(tiles.shape[0]),
                                  'Tpairs_per_s': round(pairs * n * n / (statistics.median(per) * 1e-3) / 1e12, 3),
                                  'how': '%d back-to-back launches between two HIP events' % args.launches})

    # numpy brute force on a subset
    k = min(args.host_pairs, pairs)
    t0 = time.perf_counter()
    want = chamfer_distance_host(ground[:k], aerial[:k], to_aerial[:k])
    host_ms = (time.perf_counter() - t0) * 1e3
    res['host_numpy'] = {'pairs': k, 'ms': round(host_ms, 1), 'ms_scaled_to_batch': round(host_ms * pairs / k, 1)}
    dev = got.chamfer[:k].cpu().numpy()
    res['chamfer_first_pair'] = {'device': float(dev[0]), 'host': float(want.chamfer[0])}
    # both routes start from their own transformed cloud: 1e-6 relative plus sqrt(3) * 4 ulp32(64 m) per direction
    assert (np.abs(dev - want.chamfer) <= 1e-6 * want.chamfer + 2 * np.sqrt(3.0) * 4 * 7.63e-6).all(), (dev, want.chamfer)
    res['speedup_vs_host'] = round(res['host_numpy']['ms_scaled_to_batch'] / res['device_chamfer_call']['median_ms'], 1)

    try:
        from scipy.spatial import cKDTree
    except ImportError:
        res['ckdtree'] = 'scipy is not importable'
    else:
        k = min(args.tree_pairs, pairs)
        t0 = time.perf_counter()
        moved = transform_points_host(ground[:k], to_aerial[:k])
        tree = []
        for g, a in zip(moved, aerial[:k]):
            g, a = g.astype(np.float64), a.astype(np.float64)
            tree.append(cKDTree(a).query(g)[0].mean() + cKDTree(g).query(a)[0].mean())
        tree_ms = (time.perf_counter() - t0) * 1e3
        res['ckdtree'] = {'pairs': k, 'ms': round(tree_ms, 1), 'ms_scaled_to_batch': round(tree_ms * pairs / k, 1)}
        assert (np.abs(np.array(tree) - got.chamfer[:k].cpu().numpy()) <= 1e-4).all()
        res['speedup_vs_ckdtree'] = round(res['ckdtree']['ms_scaled_to_batch'] / res['device_chamfer_call']['median_ms'], 1)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
