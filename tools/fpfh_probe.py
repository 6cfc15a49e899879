"""Time the FPFH descriptors and the feature matcher against the two existing kernels they are modelled on.

  fpfh      `compute_fpfh` (nb_neighbors = 30) on 8 synthetic raw submaps of 100 000 and of 500 000 points each
            (`synthetic.raw_submap` at `--extent` 86, the clouds of tools/normals_probe.py), device-resident, with the normals
            of `estimate_normals` on the same batch; against that `estimate_normals` call.  Both are whole calls (bounds, the
            host read, keys, sort, gather, the launches); wall clock with a device synchronisation on both sides.  Also
            `hfl_fpfh_radius`, `hfl_fpfh_spfh` and `hfl_fpfh_combine` each alone on the sorted batch between two HIP events,
            `hfl_knn_normals` alone the same way, and the share of points the whole-cloud scans finished.
  matcher   `hfl_feature_nn` on 64 pairs of 30 000 x 30 000 rows of D = 33 (FPFH-like rows: non-negative, three groups that
            sum to 200), one direction of the whole batch, `--launches` launches back to back between two HIP events, against
            `hfl_nn_dist` on 64 pairs of 30 000 x 30 000 points measured the same way; pairs per second for both, and the
            whole `feature_correspondences(mutual=True)` call.

  radius    with `--radius R` (0: the radius at which a ball holds about nb_neighbors points): `compute_fpfh` with the k
            nearest, the hybrid and the radius-only neighbourhood on the same batches and the same normals, the three whole
            calls ALTERNATING in every round; mean pairs and pending points of each.  `--only-radius` runs this leg alone.

No time is fixed in advance: the yardsticks are `estimate_normals` and `hfl_nn_dist` in the same run.  Median / min / max of
`--repeats` measurements after `--warmup`.  One JSON line.  Run it under `timeout`."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hotformerloc_amd import compute_fpfh, estimate_normals, feature_correspondences, fpfh, ops, outliers, ragged  # noqa: E402
from hotformerloc_amd import synthetic as syn                                                                     # noqa: E402
import radius_legs                                                                                                # noqa: E402
from normals_probe import NB, events, wall                                                                        # noqa: E402

DIM = 33


def probe_fpfh(args, points):
    device = torch.device('cuda', torch.cuda.current_device())
    resident = [torch.from_numpy(syn.raw_submap(700 + i, points, extent=args.extent)).to(device) for i in range(args.clouds)]
    total = points * args.clouds
    res = {'points_per_cloud': points, 'clouds': args.clouds, 'nb_neighbors': NB}
    normals = estimate_normals(resident, NB)
    feat, hist, pairs, pending = compute_fpfh(resident, normals, NB, return_histograms=True, return_pending=True)
    res['pending_share'] = round(pending / total, 6)
    res['mean_pairs'] = round(float(sum(int(p.sum()) for p in pairs)) / total, 4)
    res['points_without_pairs'] = int(sum(int((p == 0).sum()) for p in pairs))
    res['estimate_normals_call'] = wall(lambda: estimate_normals(resident, NB), args.repeats, args.warmup)
    res['compute_fpfh_call'] = wall(lambda: compute_fpfh(resident, normals, NB), args.repeats, args.warmup)
    res['call_ratio'] = round(res['compute_fpfh_call']['median_ms'] / res['estimate_normals_call']['median_ms'], 3)
    packed = ragged.upload(resident, device)
    nrm = ragged.upload(normals, device).pts
    table, sorted_pts, sorted_keys, perm = outliers.sorted_batch(packed, NB)
    sorted_nrm = ops.voxel_gather_rows(nrm, perm)
    ws = ops.FpfhWorkspace(total, table.cells, device)
    out = torch.empty((total, ops.FPFH_DIM), dtype=torch.float32, device=device)
    # each call needs what the one before it left in the workspace: timed in this order
    res['hfl_fpfh_radius'] = events(lambda: ops.fpfh_radius(ws, sorted_pts, sorted_keys, packed.off, table),
                                    args.repeats, args.warmup)
    res['hfl_fpfh_spfh'] = events(lambda: ops.fpfh_spfh(ws, sorted_pts, sorted_nrm, sorted_keys, packed.off, table,
                                                        fpfh.THETA_TABLE), args.repeats, args.warmup)
    res['hfl_fpfh_combine'] = events(lambda: ops.fpfh_combine(ws, sorted_pts, sorted_keys, perm, packed.off, table, out),
                                     args.repeats, args.warmup)
    knn_ws = ops.KnnWorkspace(total, table.cells, device)
    res['hfl_knn_normals'] = events(lambda: ops.knn_normals(sorted_pts, sorted_keys, perm, packed.off, table, None,
                                                            ops.KNN_PHASE_ALL, knn_ws), args.repeats, args.warmup)
    three = sum(res[k]['median_ms'] for k in ('hfl_fpfh_radius', 'hfl_fpfh_spfh', 'hfl_fpfh_combine'))
    res['kernel_ratio'] = round(three / res['hfl_knn_normals']['median_ms'], 3)
    return res


def probe_radius(args, points):
    device = torch.device('cuda', torch.cuda.current_device())
    resident = [torch.from_numpy(syn.raw_submap(700 + i, points, extent=args.extent)).to(device) for i in range(args.clouds)]
    total = points * args.clouds
    radius, how = radius_legs.radius_of(args, resident, NB)
    res = {'points_per_cloud': points, 'clouds': args.clouds, 'nb_neighbors': NB, 'radius_m': round(radius, 4), 'radius': how}
    normals = estimate_normals(resident, NB)
    for name, nb, r in (('k_nearest', NB, None), ('hybrid', NB, radius), ('radius_only', None, radius)):
        _, _, pairs, pending = compute_fpfh(resident, normals, nb, radius=r, return_histograms=True, return_pending=True)
        res[name] = {'mean_pairs': round(float(sum(int(p.sum()) for p in pairs)) / total, 4), 'pending': pending}
    timed = radius_legs.alternate({'k_nearest': lambda: compute_fpfh(resident, normals, NB),
                                   'hybrid': lambda: compute_fpfh(resident, normals, NB, radius=radius),
                                   'radius_only': lambda: compute_fpfh(resident, normals, None, radius=radius)},
                                  args.repeats, args.warmup)
    for name, t in timed.items():
        res[name]['compute_fpfh_call'] = t
    return res


def fpfh_like_rows(rng, n):
    """(n, 33) float32 rows shaped like descriptors: three groups of 11 non-negative bins, each summing to 200"""
    rows = rng.gamma(0.6, 1.0, (n, 3, 11))
    return (200.0 * rows / rows.sum(2, keepdims=True)).reshape(n, DIM).astype(np.float32)


def probe_matcher(args):
    n, pairs = args.pair_points, args.pairs
    rng = np.random.default_rng(5)
    device = torch.device('cuda', torch.cuda.current_device())
    off = torch.arange(pairs + 1, dtype=torch.int64, device=device) * n
    res = {'pairs': pairs, 'rows_per_side': n, 'dim': DIM, 'tests': pairs * n * n}
    q = torch.from_numpy(fpfh_like_rows(rng, pairs * n)).to(device)
    t = torch.from_numpy(fpfh_like_rows(rng, pairs * n)).to(device)
    tiles = torch.from_numpy(ops.feature_tiles(np.full(pairs, n))).to(device)
    res['hfl_feature_nn'] = events(lambda: ops.feature_nn(q, off, t, off, tiles), args.repeats, args.warmup, args.launches)
    res['hfl_feature_nn']['pairs_per_s'] = round(res['tests'] / (res['hfl_feature_nn']['median_ms'] * 1e-3), 0)
    qp = torch.from_numpy(rng.uniform(-30.0, 30.0, (pairs * n, 3)).astype(np.float32)).to(device)
    tp = torch.from_numpy(rng.uniform(-30.0, 30.0, (pairs * n, 3)).astype(np.float32)).to(device)
    point_tiles = torch.from_numpy(ops.overlap_tiles(np.full(pairs, n))).to(device)
    res['hfl_nn_dist'] = events(lambda: ops.nn_dist(qp, off, tp, off, point_tiles), args.repeats, args.warmup, args.launches)
    res['hfl_nn_dist']['pairs_per_s'] = round(res['tests'] / (res['hfl_nn_dist']['median_ms'] * 1e-3), 0)
    res['feature_over_point'] = round(res['hfl_feature_nn']['median_ms'] / res['hfl_nn_dist']['median_ms'], 3)
    res['feature_correspondences_mutual_call'] = wall(lambda: feature_correspondences((q, off), (t, off), mutual=True),
                                                      max(args.repeats // 2, 1), 1)
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
    radius_legs.add_arguments(ap)
    args = ap.parse_args()
    if args.only_radius and args.radius is None:
        ap.error('--only-radius needs --radius')
    if not torch.cuda.is_available():
        raise SystemExit('fpfh_probe needs a GPU: nothing is timed without one')
    res = {}
    if not args.only_radius:
        res = {'fpfh': [probe_fpfh(args, points) for points in args.points], 'matcher': probe_matcher(args)}
    if args.radius is not None:
        res['radius'] = [probe_radius(args, points) for points in args.points]
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
