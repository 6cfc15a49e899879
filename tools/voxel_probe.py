"""Time the submap front end (voxel-grid downsample at v = 0.8, then the PointNetVLAD normalisation) by two routes, on 8
synthetic raw submaps of 500 000 points each (`synthetic.raw_submap`, a 100 m forest scene).

  device   `voxel.prepare_submaps` on host clouds: one upload, `hfl_voxel_keys`, `torch.sort(stable=True)`,
           `hfl_voxel_reduce`, `hfl_submap_normalise`, one host read.  Also each stage alone on device-resident data between
           two HIP events, so that the sort's share of the device time is on file (DESIGN.md names the sort as the next step).
  host     `voxel.normalise_submaps_host(voxel.voxel_downsample_host(...))`, numpy float64, plus the upload of the result.

Wall clock with a device synchronisation on both sides, median / min / max of `--repeats` calls after `--warmup`; the two
routes' point counts are compared before anything is timed.  One JSON line.  Run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hotformerloc_amd import ops, ragged, voxel                                 # noqa: E402
from hotformerloc_amd import synthetic as syn                                   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clouds', type=int, default=8)
    ap.add_argument('--points', type=int, default=500000)
    ap.add_argument('--voxel-size', type=float, default=0.8)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--host-repeats', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('voxel_probe needs a GPU: nothing is timed without one')
    v = args.voxel_size
    raw = [syn.raw_submap(700 + i, args.points, extent=100.0) for i in range(args.clouds)]
    res = {'clouds': args.clouds, 'points_per_cloud': args.points, 'voxel_size': v}

    dev = voxel.prepare_submaps(raw, v)
    host = voxel.normalise_submaps_host(voxel.voxel_downsample_host(raw, v))
    assert [int(d.shape[0]) for d in dev] == [len(h) for h in host]
    res['output_points'] = [len(h) for h in host]

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

    res['device_call'] = timed(lambda: voxel.prepare_submaps(raw, v), args.repeats, args.warmup)
    res['host_call_and_upload'] = timed(
        lambda: [torch.from_numpy(h).cuda() for h in voxel.normalise_submaps_host(voxel.voxel_downsample_host(raw, v))],
        args.host_repeats, 0)
    res['speedup_vs_host'] = round(res['host_call_and_upload']['median_ms'] / res['device_call']['median_ms'], 1)

    # the stages alone, on device-resident data
    ts = ragged.as_tensors(raw)
    packed = ragged.upload(ts, torch.device('cuda', torch.cuda.current_device()))
    pts, off = packed.pts, packed.off
    batch = len(raw)
    state = {}

    def stage_keys():
        state['keys'] = ops.voxel_keys(pts, off, v)[0]

    def stage_sort():
        state['sorted'], state['perm'] = torch.sort(state['keys'], stable=True)

    def stage_reduce():
        state['down'], state['down_off'], _, _ = ops.voxel_reduce(state['sorted'], state['perm'], pts, batch)

    def stage_normalise():
        ops.submap_normalise(state['down'], state['down_off'])

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stages = {}
    for name, fn in (('voxel_keys', stage_keys), ('sort', stage_sort), ('voxel_reduce', stage_reduce),
                     ('submap_normalise', stage_normalise)):
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
    total = sum(s['median_ms'] for s in stages.values())
    res['stages'] = stages
    res['stages_total_ms'] = round(total, 4)
    res['sort_share'] = round(stages['sort']['median_ms'] / total, 3)
    res['kernels_ms'] = round(total - stages['sort']['median_ms'], 4)
    upload = timed(lambda: ragged.upload(ts, pts.device).off, args.repeats, 1)
    res['upload'] = upload
    print(json.dumps(res))


if __name__ == '__main__':
    main()
