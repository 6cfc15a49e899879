"""Time the PointNetVLAD downsampler (`voxel.pnvlad_downsample`, target 4096) by two routes, on 8 synthetic raw submaps of
500 000 points each (`synthetic.raw_submap`, a 100 m forest scene: surfaces, not a filled box).

  device   `voxel.pnvlad_downsample` on host clouds: one upload, `hfl_voxel_bounds`, then rounds of `hfl_voxel_occupancy`
           (64 / 8..64 speculative candidates per unfinished cloud) with one host read each, the voxel means at the size
           found (keys, sort, reduce per cloud) and one gather of the random rows.  Also the search alone, its rounds and
           the candidates it evaluated per cloud, and one `hfl_voxel_occupancy` call on device-resident data between two
           HIP events, as nanoseconds per (candidate, point) pair.
  host     `voxel.pnvlad_downsample_host`, numpy float64: the reference's loop, one `np.unique` over the raw cloud per
           probe.  It takes minutes, so it runs once on the first `--host-clouds` clouds and is reported per cloud.

Wall clock with a device synchronisation on both sides, median / min / max of `--repeats` calls after `--warmup`; the two
routes' voxel sizes and probe traces are compared before anything is timed.  One JSON line.  Run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hotformerloc_amd import ops, ragged, voxel                                 # noqa: E402
from hotformerloc_amd import synthetic as syn                                   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clouds', type=int, default=8)
    ap.add_argument('--points', type=int, default=500000)
    ap.add_argument('--target', type=int, default=4096)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--host-clouds', type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('fixed_submaps_probe needs a GPU: nothing is timed without one')
    raw = [syn.raw_submap(700 + i, args.points, extent=100.0) for i in range(args.clouds)]
    res = {'clouds': args.clouds, 'points_per_cloud': args.points, 'target': args.target,
           'k_one': voxel.PNVLAD_K_ONE, 'k_two': voxel.PNVLAD_K_TWO}

    found, stats = voxel.pnvlad_search(raw, args.target, return_stats=True)
    res.update(rounds=stats['rounds'], candidates_evaluated=stats['candidates'], occupancy_calls=stats['occupancy_calls'],
               sort_fallbacks=stats.get('sort_fallbacks', 0), probes_of_the_reference=[len(f['trace']) for f in found],
               voxel_sizes=[round(f['voxel_size'], 3) for f in found], cells=[f['count'] for f in found])
    print('device search done: %s' % json.dumps(res), file=sys.stderr, flush=True)

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

    res['device_call'] = timed(lambda: voxel.pnvlad_downsample(raw, args.target), args.repeats, args.warmup)
    res['device_search_only'] = timed(lambda: voxel.pnvlad_search(raw, args.target), args.repeats, args.warmup)

    # one occupancy call: the first phase-one round of every cloud, on device-resident data
    packed = ragged.upload(ragged.as_tensors(raw), torch.device('cuda', torch.cuda.current_device()))
    pts, off = packed.pts, packed.off
    bounds, lo_hi = ragged.bounds_host(packed)
    table, words, pairs = [], 0, 0
    for c in range(args.clouds):
        v = voxel.PNVLAD_START
        for _ in range(voxel.PNVLAD_K_ONE):
            nx, ny, nz = voxel.grid_dims(lo_hi[c], v)
            table.append((c, nx, ny, nz, v, words))
            words += (nx * ny * nz + 31) // 32
            pairs += args.points
            v -= voxel.PNVLAD_STEP
    table = np.array(table, dtype=np.dtype(ops.VOXEL_CANDIDATE_DTYPE))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = []
    for i in range(args.warmup + args.repeats):
        torch.cuda.synchronize()
        e0.record()
        ops.voxel_occupancy(pts, off, bounds, table, words, args.points)
        e1.record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            per.append(e0.elapsed_time(e1))
    res['occupancy_call'] = {'candidates': len(table), 'bitmap_bytes': 4 * words, 'median_ms': round(statistics.median(per), 4),
                             'min_ms': round(min(per), 4), 'max_ms': round(max(per), 4),
                             'ns_per_candidate_point': round(statistics.median(per) * 1e6 / pairs, 5)}
    print('device timings done: %s' % json.dumps(res), file=sys.stderr, flush=True)

    k = max(min(args.host_clouds, args.clouds), 1)
    t0 = time.perf_counter()
    host_found = voxel.pnvlad_search_host(raw[:k], args.target)
    search_s = time.perf_counter() - t0
    assert [f['trace'] for f in host_found] == [f['trace'] for f in found[:k]]
    t0 = time.perf_counter()
    for i in range(k):
        voxel.voxel_downsample_host([raw[i]], host_found[i]['voxel_size'])
    means_s = time.perf_counter() - t0
    res['host'] = {'clouds': k, 'ms_per_cloud': round((search_s + means_s) * 1e3 / k, 1),
                   'search_ms_per_cloud': round(search_s * 1e3 / k, 1)}
    res['device_ms_per_cloud'] = round(res['device_call']['median_ms'] / args.clouds, 3)
    res['speedup_vs_host_per_cloud'] = round(res['host']['ms_per_cloud'] / res['device_ms_per_cloud'], 1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
