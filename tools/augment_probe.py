"""Time one training batch through the augmentation, on the device and by the host route it replaces.

  device   `augment.augment_clouds` on 128 clouds of the CS-Wild-Places sizes (10-20 k points, aug_mode 2, set_aug_mode 1,
           cylindrical): the upload of the raw batch, ONE `hfl_augment_clouds` launch, the read of the 128 counts.  Also the
           launch alone, between two HIP events over 20 back-to-back launches, and its algorithmic traffic -- 12 B read per
           point and pass over the points (the Normalize bounding box, the block's bounding box where the coin came up, the
           final pass; the radix select regenerates keys and reads no point) plus 12 B written per kept point -- against the
           8 TB/s HBM peak.
  host     the only route without the kernel: `augment.augment_clouds_host` cloud by cloud (numpy / torch CPU, the same
           chain as the reference's transforms), then the upload of the results.

Wall clock with a device synchronisation on both sides, median / min / max of `--repeats` calls after `--warmup`; one JSON
line.  Run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hotformerloc_amd import augment as A, ops            # noqa: E402
from hotformerloc_amd import synthetic as syn             # noqa: E402

HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--clouds', type=int, default=128)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--host-repeats', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    sizes = [10000 + int(5000 * (1 + syn.hash_uniform(7, args.clouds)[i])) for i in range(args.clouds)]
    raws = [(syn.forest_cloud(3000 + i, n).astype(np.float64) * (45.0, 45.0, 25.0)).astype(np.float32)
            for i, n in enumerate(sizes)]
    cfg = A.AugmentConfig.from_training_params(2, 1, 180.0, True, 'cylindrical')
    params = A.draw_params(sizes, cfg, torch.Generator().manual_seed(1))
    res = {'clouds': args.clouds, 'points': int(sum(sizes))}

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

    res['device_call'] = timed(lambda: A.augment_clouds(raws, cfg, seed=5, params=params), args.repeats, args.warmup)
    res['host_chain_and_upload'] = timed(
        lambda: [t.cuda() for t in A.augment_clouds_host(raws, cfg, seed=5, params=params)], args.host_repeats, 1)
    # the launch alone
    pts = torch.cat([torch.from_numpy(r) for r in raws]).cuda()
    ncfg = A.native_config(cfg, params, True)
    rows = params.rows()
    _, counts, _ = ops.augment_clouds(pts, sizes, rows, ncfg, 5)
    kept = int(counts.sum().item())
    passes = sum(n * (2 + int(b)) for n, b in zip(sizes, params.block))
    nbytes = 12 * passes + 12 * kept
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(20):
            ops.augment_clouds(pts, sizes, rows, ncfg, 5)
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) / 20)
    ms = statistics.median(per)
    gbs = nbytes / (ms * 1e-3) / 1e9
    res['launch'] = {'median_ms': round(ms, 4), 'min_ms': round(min(per), 4), 'max_ms': round(max(per), 4),
                     'algorithmic_bytes': nbytes, 'GBps': round(gbs, 1), 'frac_of_8TBps': round(gbs / HBM_PEAK_GBS, 4),
                     'how': '20 back-to-back launches (with their table uploads) between two HIP events'}
    res['speedup_call'] = round(res['host_chain_and_upload']['median_ms'] / res['device_call']['median_ms'], 1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
