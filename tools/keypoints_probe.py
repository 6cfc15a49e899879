"""Time the ISS keypoint detector, what it saves the steps behind it, and the whole calls with and without it.

  detector  `iss_keypoints` on 8 synthetic raw submaps of 100 000 and of 500 000 points each (`synthetic.raw_submap` at
            `--extent` 86, the clouds of tools/normals_probe.py), device-resident, at the salient radius at which a ball holds
            about 30 points (bisection on `radius_neighbour_counts`; `--radius` sets it) and a non-maximum radius of
            `--non-max-ratio` times that, against `estimate_normals(nb_neighbors=None, radius=)` on the same batch: the same
            scan and sums with the other finish.  Whole calls, ALTERNATING, wall clock with a device synchronisation on both
            sides; and `hfl_iss_saliency`, `hfl_iss_select` and `hfl_knn_normals_radius` alone on one sorted batch between two
            HIP events.  The share of points with a saliency, the share kept, the points left to the whole-cloud scans.
  matching  on `--pairs` pairs of `--pair-points` points (two samplings of one scene, tools/submap_overlap_probe.py; the
            source moved by a small motion): `feature_correspondences` (the `hfl_feature_nn` launches), one
            `spectral_consistency` step and `consensus_registration` on all rows and on the keypoints' rows, the routes
            alternating.  Normals and FPFH are computed once, on all points, for both.
  whole     `global_registration` on those pairs and `rerank_candidates` on `--queries` x `--candidates` clouds of
            `--rerank-points` points, with and without the two radii, alternating.  `--baseline` runs the calls without
            keypoints alone and imports nothing this probe's commit added, so the same file times an earlier checkout.

No time is fixed in advance.  Median / min / max of `--repeats` measurements after `--warmup`.  One JSON line.  Run it under
`timeout`."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hotformerloc_amd as hfl                                                                                     # noqa: E402
from hotformerloc_amd import ops, outliers, ragged                                                                 # noqa: E402
from hotformerloc_amd import synthetic as syn                                                                      # noqa: E402
import radius_legs                                                                                                 # noqa: E402
from normals_probe import events                                                                                   # noqa: E402
from registration_probe import small_motion                                                                        # noqa: E402
from submap_overlap_probe import scene                                                                             # noqa: E402

BALL = 30


def radii_of(args, resident):
    rs = float(args.radius) if args.radius > 0.0 else radius_legs.pick_radius(resident, BALL)
    return rs, rs * args.non_max_ratio


def probe_detector(args, points):
    device = torch.device('cuda', torch.cuda.current_device())
    resident = [torch.from_numpy(syn.raw_submap(700 + i, points, extent=args.extent)).to(device) for i in range(args.clouds)]
    total = points * args.clouds
    rs, rn = radii_of(args, resident)
    keys, sal, pending = hfl.iss_keypoints(resident, rs, rn, return_saliency=True, return_pending=True)
    res = {'points_per_cloud': points, 'clouds': args.clouds, 'salient_radius_m': round(rs, 4), 'non_max_radius_m': round(rn, 4),
           'mean_ball': round(radius_legs.mean_count(resident, rs), 3), 'pending': pending,
           'salient_share': round(sum(int((s > 0).sum()) for s in sal) / total, 5),
           'kept_share': round(sum(int(k.shape[0]) for k in keys) / total, 5)}
    res.update(radius_legs.alternate({'iss_keypoints_call': lambda: hfl.iss_keypoints(resident, rs, rn),
                                      'estimate_normals_radius_call': lambda: hfl.estimate_normals(resident, None, radius=rs)},
                                     args.repeats, args.warmup))
    packed = ragged.upload(resident, device)
    table, sorted_pts, sorted_keys, perm = outliers.sorted_batch(packed, None, None, radius=max(rs, rn))
    ws = ops.KnnWorkspace(total, table.cells, device)
    r2s, r2n = outliers.radius2(rs), outliers.radius2(rn)
    sorted_sal = ops.iss_saliency(sorted_pts, sorted_keys, perm, packed.off, table, r2s, 0.975, 0.975, 5, workspace=ws)[2]
    res['hfl_iss_saliency'] = events(lambda: ops.iss_saliency(sorted_pts, sorted_keys, perm, packed.off, table, r2s, 0.975,
                                                              0.975, 5, workspace=ws), args.repeats, args.warmup)
    res['hfl_iss_select'] = events(lambda: ops.iss_select(sorted_pts, sorted_keys, perm, sorted_sal, packed.off, table, r2n, 5,
                                                          workspace=ws), args.repeats, args.warmup)
    res['hfl_knn_normals_radius'] = events(lambda: ops.knn_normals(sorted_pts, sorted_keys, perm, packed.off, table, None,
                                                                   ops.KNN_PHASE_ALL, ws, radius2=r2s, radius_only=True),
                                           args.repeats, args.warmup)
    res['saliency_over_normals'] = round(res['hfl_iss_saliency']['median_ms'] / res['hfl_knn_normals_radius']['median_ms'], 3)
    res['select_over_saliency'] = round(res['hfl_iss_select']['median_ms'] / res['hfl_iss_saliency']['median_ms'], 3)
    return res


def pair_clouds(args, device):
    source, target = [], []
    for p in range(args.pairs):
        air, seen = scene(args.pair_points, p)
        source.append(hfl.transform_points_host([seen], np.linalg.inv(small_motion(1000 + p))[None])[0])
        target.append(air)
    return [torch.from_numpy(c).to(device) for c in source], [torch.from_numpy(c).to(device) for c in target]


def probe_matching(args, source, target):
    pairs = len(source)
    clouds = source + target
    rs, rn = radii_of(args, clouds[:8])
    normals = hfl.estimate_normals(clouds, 30)
    features = hfl.compute_fpfh(clouds, normals, 30)
    keys = hfl.iss_keypoints(clouds, rs, rn)
    total = sum(int(c.shape[0]) for c in clouds)
    res = {'pairs': pairs, 'points_per_cloud': args.pair_points, 'salient_radius_m': round(rs, 4),
           'non_max_radius_m': round(rn, 4), 'kept_share': round(sum(int(k.shape[0]) for k in keys) / total, 5),
           'keypoints_per_cloud': round(sum(int(k.shape[0]) for k in keys) / len(clouds), 1)}
    sets = {'all_points': (clouds, features),
            'keypoints': ([c[k] for c, k in zip(clouds, keys)], [f[k] for f, k in zip(features, keys)])}
    routes, corr = {}, {}
    for name, (pts, rows) in sets.items():
        matched = hfl.feature_correspondences(rows[:pairs], rows[pairs:], mutual=True)
        corr[name] = hfl.correspondence_pairs(matched[0], matched[2])
        res[name] = {'mutual_correspondences_per_pair': round(sum(int(c.shape[0]) for c in corr[name]) / pairs, 1)}
        routes['feature_correspondences/' + name] = \
            lambda rows=rows: hfl.feature_correspondences(rows[:pairs], rows[pairs:], mutual=True)
        routes['spectral_step/' + name] = \
            lambda pts=pts, c=corr[name]: hfl.spectral_consistency(pts[:pairs], pts[pairs:], c, iterations=1)
        routes['consensus_registration/' + name] = \
            lambda pts=pts, c=corr[name]: hfl.consensus_registration(pts[:pairs], pts[pairs:], c)
    for name, t in radius_legs.alternate(routes, args.repeats, args.warmup).items():
        step, which = name.split('/')
        res[which][step] = t
    return res, (rs, rn)


def probe_whole(args, source, target, radii, rng, device):
    n_db = max(args.candidates * 2, 2)
    queries = [torch.from_numpy(syn.raw_submap(900 + i, args.rerank_points, extent=args.extent)).to(device)
               for i in range(args.queries)]
    database = [torch.from_numpy(syn.raw_submap(1900 + i, args.rerank_points, extent=args.extent)).to(device)
                for i in range(n_db)]
    cand = np.stack([rng.permutation(n_db)[:args.candidates] for _ in range(args.queries)])
    routes = {'global_registration': lambda: hfl.global_registration(source, target),
              'rerank_candidates': lambda: hfl.rerank_candidates(queries, database, cand)}
    res = {'pairs': len(source), 'points_per_cloud': args.pair_points, 'queries': args.queries, 'candidates': args.candidates,
           'rerank_points': args.rerank_points}
    if radii is not None:
        kw = dict(salient_radius=radii[0], non_max_radius=radii[1])
        r_radii = radii_of(args, queries)
        r_kw = dict(salient_radius=r_radii[0], non_max_radius=r_radii[1])
        res['rerank_radii_m'] = [round(r, 4) for r in r_radii]
        routes['global_registration_on_keypoints'] = lambda: hfl.global_registration(source, target, **kw)
        routes['rerank_candidates_on_keypoints'] = lambda: hfl.rerank_candidates(queries, database, cand, **r_kw)
    res.update(radius_legs.alternate(routes, args.whole_repeats, args.whole_warmup))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clouds', type=int, default=8)
    ap.add_argument('--points', type=int, nargs='+', default=[100000, 500000])
    ap.add_argument('--extent', type=float, default=86.0)
    ap.add_argument('--radius', type=float, default=0.0, help='the salient radius; 0 picks the one with a mean ball of 30')
    ap.add_argument('--non-max-ratio', type=float, default=0.75)
    ap.add_argument('--pairs', type=int, default=64)
    ap.add_argument('--pair-points', type=int, default=30000)
    ap.add_argument('--queries', type=int, default=8)
    ap.add_argument('--candidates', type=int, default=25)
    ap.add_argument('--rerank-points', type=int, default=4096)
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--whole-repeats', type=int, default=15)
    ap.add_argument('--whole-warmup', type=int, default=3)
    ap.add_argument('--baseline', action='store_true', help='the whole calls without keypoints alone')
    ap.add_argument('--skip-detector', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('keypoints_probe needs a GPU: nothing is timed without one')
    device = torch.device('cuda', torch.cuda.current_device())
    rng = np.random.default_rng(9)
    source, target = pair_clouds(args, device)
    res, radii = {}, None
    if not args.baseline:
        if not args.skip_detector:
            res['detector'] = [probe_detector(args, points) for points in args.points]
        res['matching'], radii = probe_matching(args, source, target)
    res['whole'] = probe_whole(args, source, target, radii, rng, device)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
