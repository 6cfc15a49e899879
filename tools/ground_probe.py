"""Time the cloth-filter ground removal (`hotformerloc_amd/ground.py`) by two routes, on 8 synthetic raw submaps of 500 000
points each (`synthetic.raw_submap` at `--extent` 86, which is a forest scene 60 m wide: a cloth of 64 x 64 particles at
the 1 m resolution).

  device   `ground.remove_ground` on host clouds: one upload, `hfl_voxel_bounds` and a host read, `hfl_cloth_raster`,
           `hfl_cloth_simulate`, `hfl_cloth_classify`, `torch.nonzero`, `hfl_voxel_gather_rows`.  Also each launch alone on
           device-resident data between two HIP events: the simulate launch is the one bound by barriers, not by the points.
  host     `ground.remove_ground_host`, numpy fp32 to the same definition, plus the upload of the result.

Wall clock with a device synchronisation on both sides, median / min / max of `--repeats` calls after `--warmup`; the two
routes' outputs are compared bit for bit before anything is timed.  One JSON line.  Run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hotformerloc_amd import ground, ops, ragged                                # noqa: E402
from hotformerloc_amd import synthetic as syn                                   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clouds', type=int, default=8)
    ap.add_argument('--points', type=int, default=500000)
    ap.add_argument('--extent', type=float, default=86.0)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--host-repeats', type=int, default=2)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ground_probe needs a GPU: nothing is timed without one')
    raw = [syn.raw_submap(900 + i, args.points, extent=args.extent) for i in range(args.clouds)]
    res = {'clouds': args.clouds, 'points_per_cloud': args.points, 'extent_m': args.extent}

    dev, dev_cloth = ground.remove_ground(raw, return_cloth=True)
    host, host_cloth = ground.remove_ground_host(raw, return_cloth=True)
    for d, h, dc, hc in zip(dev, host, dev_cloth, host_cloth):
        assert np.array_equal(d.cpu().numpy().view(np.uint32), h.view(np.uint32))
        assert np.array_equal(dc[0].cpu().numpy().view(np.uint32), hc[0].view(np.uint32)) and dc[3] == hc[3]
    res['kept_points'] = [len(h) for h in host]
    res['cloth'] = [list(hc[0].shape) for hc in host_cloth]
    res['steps_run'] = [hc[3] for hc in host_cloth]

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

    res['device_call'] = timed(lambda: ground.remove_ground(raw), args.repeats, args.warmup)
    res['host_call_and_upload'] = timed(lambda: [torch.from_numpy(h).cuda() for h in ground.remove_ground_host(raw)],
                                        args.host_repeats, 0)
    res['speedup_vs_host'] = round(res['host_call_and_upload']['median_ms'] / res['device_call']['median_ms'], 1)

    # the launches alone, on device-resident data
    prm = ground.ClothParams()
    ts = ragged.as_tensors(raw)
    packed = ragged.upload(ts, torch.device('cuda', torch.cuda.current_device()))
    pts, off = packed.pts, packed.off
    table = ground.cloth_device(packed, prm)[0]
    state = {}

    def stage_bounds():
        ops.voxel_bounds(pts, off)

    def stage_raster():
        state['t'] = ops.cloth_raster(pts, off, table, float(prm.r))

    def stage_simulate():
        state['u'] = ops.cloth_simulate(state['t'], table, float(prm.f1), float(prm.f2), float(prm.gravity_step),
                                        float(prm.keep), prm.iterations, prm.slope_smooth)[0]

    def stage_classify():
        state['keep'] = ops.cloth_classify(pts, off, state['u'], table, float(prm.r), float(prm.threshold))

    def stage_compact():
        ops.voxel_gather_rows(pts, torch.nonzero(state['keep']).reshape(-1))

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stages = {}
    for name, fn in (('voxel_bounds', stage_bounds), ('cloth_raster', stage_raster), ('cloth_simulate', stage_simulate),
                     ('cloth_classify', stage_classify), ('nonzero_and_gather', stage_compact)):
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
    steps = max(res['steps_run'])
    res['simulate_us_per_step'] = round(stages['cloth_simulate']['median_ms'] * 1e3 / max(steps, 1), 2)
    res['upload'] = timed(lambda: ragged.upload(ts, pts.device).off, args.repeats, 1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
