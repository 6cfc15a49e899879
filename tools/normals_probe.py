"""Time normal estimation and the point-to-plane iteration against the two existing kernels they are built on.

  normals   `estimate_normals` (nb_neighbors = 30) on 8 synthetic raw submaps of 100 000 and of 500 000 points each
            (`synthetic.raw_submap` at `--extent` 86, the clouds of tools/outlier_probe.py without its strays), device-resident,
            against `knn_mean_distance` at the same nb_neighbors: the search alone, the parent's cost for the same scan.  Both
            are whole calls (bounds, the host read, keys, sort, gather, the three launches); wall clock with a device
            synchronisation on both sides.  Also `hfl_knn_normals` and `hfl_knn_mean_dist` alone on the sorted batch between
            two HIP events, and the share of points the whole-cloud scan finished.
  plane     one point-to-plane iteration (`hfl_icp_correspond_plane` + `hfl_icp_solve_plane`) against one point-to-point
            iteration (`hfl_icp_correspond` + `hfl_icp_solve`) on 64 pairs of 30 000 x 30 000 points, the scenes of
            tools/registration_probe.py, every pair RUNNING, `--launches` iterations back to back between two HIP events.
            The target normals are `estimate_normals` of the targets.  A third leg times the generalized iteration
            (`hfl_icp_correspond_generalized` + `hfl_icp_solve_plane`) on the same pairs with `estimate_normals` of the
            sources as well, and a whole `icp_refine` call of each mode with the updates it needed.  `--only-plane` leaves
            the normals part out.

  radius    with `--radius R` (0: the radius at which a ball holds about nb_neighbors points, found by bisection on
            `radius_neighbour_counts`): `estimate_normals` with the k nearest, with the hybrid and with the radius-only
            neighbourhood on the same batches, the three whole calls ALTERNATING in every round; the mean |N(i)| and the
            number of points the whole-cloud scan finished for each.  `--only-radius` runs this leg alone.

No throughput target is set: the figures to report are the two ratios, each measured in one run.  Median / min / max of
`--repeats` measurements after `--warmup`.  One JSON line.  Run it under `timeout`."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hotformerloc_amd import estimate_normals, knn_mean_distance, ops, outliers, ragged, transform_points_host   # noqa: E402
from hotformerloc_amd import registration as reg                                                                # noqa: E402
from hotformerloc_amd import synthetic as syn                                                                   # noqa: E402
import radius_legs                                                                                              # noqa: E402
from registration_probe import MAX_DIST, small_motion                                                           # noqa: E402
from submap_overlap_probe import scene, spread                                                                  # noqa: E402

NB = 30


def wall(fn, repeats, warmup):
    ms = []
    for i in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return spread(ms)


def events(fn, repeats, warmup, launches=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for i in range(warmup + repeats):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1) / launches)
    return spread(ms)


def probe_normals(args, points):
    device = torch.device('cuda', torch.cuda.current_device())
    resident = [torch.from_numpy(syn.raw_submap(700 + i, points, extent=args.extent)).to(device) for i in range(args.clouds)]
    res = {'points_per_cloud': points, 'clouds': args.clouds, 'nb_neighbors': NB}
    normals, counts, pending = estimate_normals(resident, NB, return_counts=True, return_pending=True)
    total = points * args.clouds
    res['pending_share'] = round(pending / total, 6)
    res['zero_normals'] = int(sum(int((~n.any(1)).sum()) for n in normals))
    res['mean_neighbourhood'] = round(float(sum(int(c.sum()) for c in counts)) / total, 4)
    res['estimate_normals_call'] = wall(lambda: estimate_normals(resident, NB), args.repeats, args.warmup)
    res['knn_mean_distance_call'] = wall(lambda: knn_mean_distance(resident, NB), args.repeats, args.warmup)
    res['call_ratio'] = round(res['estimate_normals_call']['median_ms'] / res['knn_mean_distance_call']['median_ms'], 3)
    packed = ragged.upload(resident, device)
    table, sorted_pts, sorted_keys, perm = outliers.sorted_batch(packed, NB)
    ws = ops.KnnWorkspace(total, table.cells, device)
    out = torch.empty(total, dtype=torch.float32, device=device)
    res['hfl_knn_normals'] = events(lambda: ops.knn_normals(sorted_pts, sorted_keys, perm, packed.off, table, None,
                                                            ops.KNN_PHASE_ALL, ws), args.repeats, args.warmup)
    res['hfl_knn_mean_dist'] = events(lambda: ops.knn_mean_dist(sorted_pts, sorted_keys, perm, packed.off, table,
                                                                ops.KNN_PHASE_ALL, ws, out), args.repeats, args.warmup)
    res['kernel_ratio'] = round(res['hfl_knn_normals']['median_ms'] / res['hfl_knn_mean_dist']['median_ms'], 3)
    return res


def probe_radius(args, points):
    device = torch.device('cuda', torch.cuda.current_device())
    resident = [torch.from_numpy(syn.raw_submap(700 + i, points, extent=args.extent)).to(device) for i in range(args.clouds)]
    total = points * args.clouds
    radius, how = radius_legs.radius_of(args, resident, NB)
    res = {'points_per_cloud': points, 'clouds': args.clouds, 'nb_neighbors': NB, 'radius_m': round(radius, 4), 'radius': how}
    for name, nb, r in (('k_nearest', NB, None), ('hybrid', NB, radius), ('radius_only', None, radius)):
        normals, counts, pending = estimate_normals(resident, nb, radius=r, return_counts=True, return_pending=True)
        res[name] = {'mean_neighbourhood': round(float(sum(int(c.sum()) for c in counts)) / total, 4), 'pending': pending,
                     'zero_normals': int(sum(int((~n.any(1)).sum()) for n in normals))}
    timed = radius_legs.alternate({'k_nearest': lambda: estimate_normals(resident, NB),
                                   'hybrid': lambda: estimate_normals(resident, NB, radius=radius),
                                   'radius_only': lambda: estimate_normals(resident, None, radius=radius)},
                                  args.repeats, args.warmup)
    for name, t in timed.items():
        res[name]['estimate_normals_call'] = t
    return res


def probe_plane(args):
    n, pairs = args.pair_points, args.pairs
    source, target = [], []
    for p in range(pairs):
        air, seen = scene(n, p)
        source.append(transform_points_host([seen], np.linalg.inv(small_motion(1000 + p))[None])[0])
        target.append(air)
    d_source, d_target = [torch.from_numpy(c).cuda() for c in source], [torch.from_numpy(c).cuda() for c in target]
    res = {'pairs': pairs, 'points_per_cloud': n, 'max_correspondence_distance': MAX_DIST}
    t0 = time.perf_counter()
    d_normals = estimate_normals(d_target, NB)
    torch.cuda.synchronize()
    res['estimate_normals_of_the_targets_ms'] = round((time.perf_counter() - t0) * 1e3, 3)
    s_normals = estimate_normals(d_source, NB)
    identity = np.tile(np.eye(4)[:3], (pairs, 1, 1))
    for name, normals, more in (('point_to_point_iteration', None, None), ('point_to_plane_iteration', d_normals, None),
                                ('generalized_iteration', d_normals, s_normals)):
        batch = reg._Batch(d_source, d_target, 'normals_probe', normals, more)
        state, istate = batch.state(identity)

        def iteration():
            istate.zero_()                                               # an update leaves the pair RUNNING; keep k = 0
            batch.correspond(state, istate, MAX_DIST)
            batch.solve(state, istate, 3, 1e-6, 1e-6, False)

        res[name] = events(iteration, args.repeats, args.warmup, args.launches)
    res['plane_over_point'] = round(res['point_to_plane_iteration']['median_ms'] / res['point_to_point_iteration']['median_ms'], 3)
    res['generalized_over_plane'] = round(res['generalized_iteration']['median_ms'] /
                                          res['point_to_plane_iteration']['median_ms'], 3)
    for name, kw in (('icp_refine_point_to_point', {}),
                     ('icp_refine_point_to_plane', dict(estimation='point_to_plane', target_normals=d_normals)),
                     ('icp_refine_generalized', dict(estimation='generalized', target_normals=d_normals,
                                                     source_normals=s_normals))):
        got = {}
        res[name] = wall(lambda: got.update(r=reg.icp_refine(d_source, d_target, max_correspondence_distance=MAX_DIST, **kw)),
                         max(args.repeats // 2, 1), 1)
        r = got['r']
        res[name].update({'iterations_min': int(r.iterations.min()), 'iterations_max': int(r.iterations.max()),
                          'iterations_mean': round(float(r.iterations.mean()), 3),
                          'status_counts': np.bincount(r.status, minlength=5).tolist(),
                          'mean_fitness': round(float(r.fitness.mean()), 4),
                          'mean_inlier_rmse': round(float(np.nanmean(r.inlier_rmse)), 4)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clouds', type=int, default=8)
    ap.add_argument('--points', type=int, nargs='+', default=[100000, 500000])
    ap.add_argument('--extent', type=float, default=86.0)
    ap.add_argument('--pairs', type=int, default=64)
    ap.add_argument('--pair-points', type=int, default=30000)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--launches', type=int, default=3)
    ap.add_argument('--only-plane', action='store_true', help='the ICP iterations alone, without the normals part')
    radius_legs.add_arguments(ap)
    args = ap.parse_args()
    if args.only_radius and args.radius is None:
        ap.error('--only-radius needs --radius')
    if not torch.cuda.is_available():
        raise SystemExit('normals_probe needs a GPU: nothing is timed without one')
    res = {}
    if not args.only_radius:
        res = {'normals': [] if args.only_plane else [probe_normals(args, points) for points in args.points],
               'plane': probe_plane(args)}
    if args.radius is not None:
        res['radius'] = [probe_radius(args, points) for points in args.points]
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
