"""Time the statistical outlier filter (`hotformerloc_amd/outliers.py`) on 8 synthetic raw submaps of 100 000 and of
500 000 points each (`synthetic.raw_submap` at `--extent` 86, a forest scene 60 m wide) with `--strays` uniform stray
returns 15 to 40 m above each.

  device       `outliers.remove_outliers` on host clouds (one upload) and on device-resident clouds: `hfl_voxel_bounds`,
               `hfl_cloud_nonfinite` and a host read, `hfl_knn_cell_keys`, `torch.sort`, a gather, `hfl_knn_mean_dist` (cell
               starts, 3 x 3 x 3 query, whole-cloud scan of the pending points), `hfl_outlier_threshold`, `hfl_outlier_mask`,
               `torch.nonzero`, `hfl_voxel_gather_rows`.  Also each launch alone between two HIP events, and the share of the
               points the 3 x 3 x 3 block resolved / the whole-cloud scan finished.
  brute force  the same call with `cell_size` so large that every cloud is one cell: the query launch then scans the whole
               cloud for every point.  Only up to `--brute-max-points` points per cloud (it grows with the square).
  host         `scipy.spatial.cKDTree(p).query(p, k=20, workers=16)` in float64 per cloud, where scipy imports: the
               neighbour search alone, the yardstick for steps 1-2.

  radius       with `--radius R` (0: the radius at which a ball holds about 20 points): `radius_neighbour_counts` and
               `remove_radius_outliers(nb_points=2)` against `knn_mean_distance` and `remove_outliers` on the same resident
               clouds, the whole calls ALTERNATING in every round; the mean count and the pending points.  `--only-radius`
               runs this leg alone.

Wall clock with a device synchronisation on both sides, median / min / max of `--repeats` calls after `--warmup`; the
device avg is compared with the KD-tree's (1e-5 relative) before anything is timed.  One JSON line.  Run it under
`timeout`."""
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
from hotformerloc_amd import ops, outliers, ragged                              # noqa: E402
from hotformerloc_amd import synthetic as syn                                   # noqa: E402
import radius_legs                                                              # noqa: E402


def submap(seed, points, extent, strays):
    rng = np.random.default_rng(seed)
    base = syn.raw_submap(seed, points - strays, extent=extent)
    lo, hi = base.min(axis=0), base.max(axis=0)
    stray = np.stack([rng.uniform(lo[0], hi[0], strays), rng.uniform(lo[1], hi[1], strays),
                      lo[2] + rng.uniform(15.0, 40.0, strays)], 1).astype(np.float32)
    return np.concatenate([base, stray])[rng.permutation(points)]


def timed(fn, repeats, warmup):
    ms = []
    for i in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {'median_ms': round(statistics.median(ms), 3), 'min_ms': round(min(ms), 3), 'max_ms': round(max(ms), 3)}


def probe(args, points):
    raw = [submap(700 + i, points, args.extent, args.strays) for i in range(args.clouds)]
    res = {'points_per_cloud': points}
    device = torch.device('cuda', torch.cuda.current_device())
    resident = [torch.from_numpy(r).to(device) for r in raw]

    kept, avg, stats = outliers.remove_outliers(raw, return_distances=True, return_stats=True)
    res['kept_points'] = [int(k.shape[0]) for k in kept]
    res['threshold_m'] = [round(s['threshold'], 4) for s in stats]
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    if cKDTree is not None:
        p = raw[0].astype(np.float64)
        want = cKDTree(p).query(p, k=20, workers=16)[0].sum(axis=1) / 20
        got = avg[0].cpu().numpy()
        assert np.allclose(got, want, rtol=1e-5, atol=0), float(np.abs(got - want).max())

    res['device_call_host_clouds'] = timed(lambda: outliers.remove_outliers(raw), args.repeats, args.warmup)
    res['device_call_resident_clouds'] = timed(lambda: outliers.remove_outliers(resident), args.repeats, args.warmup)
    res['knn_only_resident_clouds'] = timed(lambda: outliers.knn_mean_distance(resident), args.repeats, args.warmup)
    if points <= args.brute_max_points:
        brute = outliers.knn_mean_distance(resident, cell_size=1e6)
        assert all(torch.equal(a, b) for a, b in zip(brute, avg))
        res['knn_only_one_cell_brute_force'] = timed(lambda: outliers.knn_mean_distance(resident, cell_size=1e6),
                                                     max(args.repeats // 3, 1), 1)

    # the launches alone, on device-resident data
    packed = ragged.upload(resident, device)
    pts, off, off_host = packed.pts, packed.off, packed.off_host
    table, sorted_pts, sorted_keys, perm = outliers.sorted_batch(packed, 20)
    res['cell_m'] = [round(float(c), 4) for c in table.host['cell']]
    res['cells'] = int(table.cells)
    ws = ops.KnnWorkspace(int(pts.shape[0]), table.cells, device)
    out = torch.empty(int(pts.shape[0]), dtype=torch.float32, device=device)
    state = {}

    def knn_phase(phase):
        return lambda: ops.knn_mean_dist(sorted_pts, sorted_keys, perm, off, table, phase, ws, out)

    def stage_sort():
        state['sort'] = torch.sort(state['keys'])

    def stage_threshold():
        state['stats'] = ops.outlier_threshold(out, off, 3.0)

    def stage_mask():
        state['keep'] = ops.outlier_mask(out, off, state['stats'])

    stages = {}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, fn in (('voxel_bounds', lambda: ops.voxel_bounds(pts, off)),
                     ('cloud_nonfinite', lambda: ops.cloud_nonfinite(pts, off)),
                     ('knn_cell_keys', lambda: state.__setitem__('keys', ops.knn_cell_keys(pts, off, table))),
                     ('torch_sort', stage_sort),
                     ('gather_sorted', lambda: ops.voxel_gather_rows(pts, perm)),
                     ('knn_cell_starts', knn_phase(ops.KNN_PHASE_STARTS)),
                     ('knn_query', knn_phase(ops.KNN_PHASE_QUERY)),
                     ('knn_fallback', knn_phase(ops.KNN_PHASE_FALLBACK)),
                     ('outlier_threshold', stage_threshold),
                     ('outlier_mask', stage_mask),
                     ('nonzero_and_gather', lambda: ops.voxel_gather_rows(pts, torch.nonzero(state['keep']).reshape(-1)))):
        per = []
        for i in range(args.warmup + args.repeats):
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                per.append(e0.elapsed_time(e1))
        stages[name] = {'median_ms': round(statistics.median(per), 4), 'min_ms': round(min(per), 4), 'max_ms': round(max(per), 4)}
    res['stages'] = stages
    res['stages_total_ms'] = round(sum(s['median_ms'] for s in stages.values()), 4)
    pending = int(ws.counter.item())
    res['pending_points'] = pending
    res['share_resolved_in_block'] = round(1.0 - pending / float(pts.shape[0]), 5)
    res['share_whole_cloud_scan'] = round(pending / float(pts.shape[0]), 5)
    assert all(torch.equal(a, b) for a, b in zip(out.split(np.diff(off_host).tolist()), avg))

    if cKDTree is not None:
        def kdtree():
            for r in raw:
                p = r.astype(np.float64)
                cKDTree(p).query(p, k=20, workers=16)
        res['scipy_ckdtree_float64_16_workers'] = timed(kdtree, args.host_repeats, 0)
        res['knn_speedup_vs_ckdtree'] = round(res['scipy_ckdtree_float64_16_workers']['median_ms']
                                              / res['knn_only_resident_clouds']['median_ms'], 1)
    return res


def probe_radius(args, points):
    device = torch.device('cuda', torch.cuda.current_device())
    resident = [torch.from_numpy(submap(700 + i, points, args.extent, args.strays)).to(device) for i in range(args.clouds)]
    radius, how = radius_legs.radius_of(args, resident, 20)
    mean, pending = radius_legs.mean_count(resident, radius, with_pending=True)
    res = {'points_per_cloud': points, 'nb_neighbors': 20, 'radius_m': round(radius, 4), 'radius': how,
           'mean_count': round(mean, 4), 'pending': pending,
           'kept_points': [int(k.shape[0]) for k in outliers.remove_radius_outliers(resident, 2, radius)]}
    res.update(radius_legs.alternate({'knn_mean_distance_call': lambda: outliers.knn_mean_distance(resident),
                                      'radius_neighbour_counts_call': lambda: outliers.radius_neighbour_counts(resident, radius),
                                      'remove_outliers_call': lambda: outliers.remove_outliers(resident),
                                      'remove_radius_outliers_call': lambda: outliers.remove_radius_outliers(resident, 2, radius)},
                                     args.repeats, args.warmup))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clouds', type=int, default=8)
    ap.add_argument('--points', type=int, nargs='+', default=[100000, 500000])
    ap.add_argument('--extent', type=float, default=86.0)
    ap.add_argument('--strays', type=int, default=200)
    ap.add_argument('--brute-max-points', type=int, default=100000)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--host-repeats', type=int, default=1)
    ap.add_argument('--warmup', type=int, default=2)
    radius_legs.add_arguments(ap)
    args = ap.parse_args()
    if args.only_radius and args.radius is None:
        ap.error('--only-radius needs --radius')
    if not torch.cuda.is_available():
        raise SystemExit('outlier_probe needs a GPU: nothing is timed without one')
    res = {'clouds': args.clouds, 'extent_m': args.extent, 'strays': args.strays}
    if not args.only_radius:
        res['runs'] = [probe(args, n) for n in args.points]
    if args.radius is not None:
        res['radius'] = [probe_radius(args, n) for n in args.points]
    print(json.dumps(res))


if __name__ == '__main__':
    main()
