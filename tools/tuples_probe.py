"""Time the tuple lists of a whole training set by three routes, at N = 20 000 and 60 000 positions.

A synthetic trajectory at UTM magnitudes: laps of a noisy closed curve about 20 km long, 10 000 scans 2 m apart per lap, so
that a scan has some tens of positives at 15 m and a few hundred non-negatives at 60 m (the README's CS-Wild-Places
thresholds).

  device   `tuples.radius_lists(p, None, 15, 60, exclude_self=True)` on host positions: the upload, the count launch, the
           cumsum, the read of the totals and the fill launch.  Also the two launches alone on device positions between two
           HIP events, against the pairs tested (N^2 per launch) -- a pair rate, not a share of peak.
  host     `tuples.radius_lists_host`: the same expression in numpy, chunked over rows.
  sklearn  the reference's way: `KDTree(p)`, `query_radius` at both thresholds, and the per-anchor loop of
           `np.setdiff1d(ind_pos[i], [i])` / `np.sort(ind_non_neg[i])`.

Wall clock with a device synchronisation on both sides, median / min / max of `--repeats` calls after `--warmup`.  The two
CPU routes take seconds to minutes a call, so they run `--host-repeats` times without warm-up and the first of those calls
is the one whose lists are compared; all three routes' lists are compared entry for entry.  One JSON line per N.  Run it
under `timeout`."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hotformerloc_amd import ops, radius_lists, radius_lists_host      # noqa: E402

POS_THRESH, NEG_THRESH = 15.0, 60.0


def trajectory(n, seed=0):
    rng = np.random.RandomState(seed)
    s = np.arange(n) / 10000.0 * 2.0 * np.pi                             # one lap per 10 000 scans
    xy = np.stack([3000.0 * np.sin(s) + 750.0 * np.sin(3.0 * s), 2000.0 * np.cos(s) + 600.0 * np.sin(2.0 * s)], 1)
    return np.array([5.0e5, 6.9e6]) + xy + rng.normal(0.0, 4.0, xy.shape)


def sklearn_route(p):
    from sklearn.neighbors import KDTree
    tree = KDTree(p)
    ind_pos = tree.query_radius(p, r=POS_THRESH)
    ind_non_neg = tree.query_radius(p, r=NEG_THRESH)
    pos = [np.setdiff1d(ind_pos[i], [i]) for i in range(len(p))]
    nn = [np.sort(ind_non_neg[i]) for i in range(len(p))]
    return pos, nn


def timed(fn, repeats, warmup, keep=None):
    ms = []
    for i in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if keep is not None and i == 0:
            keep.append(out)
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {'median_ms': round(statistics.median(ms), 3), 'min_ms': round(min(ms), 3), 'max_ms': round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[20000, 60000])
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--host-repeats', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tuples_probe needs a GPU: nothing is timed without one')
    for n in args.sizes:
        p = trajectory(n)
        dev = [x.cpu().numpy() for x in radius_lists(p, None, POS_THRESH, NEG_THRESH, exclude_self=True)]
        kept = []
        host_time = timed(lambda: radius_lists_host(p, None, POS_THRESH, NEG_THRESH, exclude_self=True), args.host_repeats, 0,
                          kept)
        sklearn_time = timed(lambda: sklearn_route(p), args.host_repeats, 0, kept)
        host, (pos, nn) = kept
        assert all(np.array_equal(a, b) for a, b in zip(dev, host))
        assert np.array_equal(np.concatenate(pos), host[1]) and np.array_equal(np.concatenate(nn), host[3])
        res = {'positions': n, 'mean_positives': round(host[1].size / n, 1), 'mean_non_negatives': round(host[3].size / n, 1)}
        res['device_call'] = timed(lambda: radius_lists(p, None, POS_THRESH, NEG_THRESH, exclude_self=True), args.repeats,
                                   args.warmup)
        res['host_numpy'], res['sklearn_kdtree_and_loop'] = host_time, sklearn_time
        # the two launches alone
        dp = torch.from_numpy(p).cuda()
        off_a, idx_a, off_b, idx_b = ops.radius_lists(dp, dp, POS_THRESH, NEG_THRESH, True)
        lib = ops._native.load()
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        stream = ops._stream()
        count_ms, fill_ms = [], []
        counts = torch.empty((n, 2), dtype=torch.int32, device='cuda')
        for _ in range(args.warmup + args.repeats):
            torch.cuda.synchronize()
            e0.record()
            for _ in range(5):
                lib.hfl_radius_lists(counts.data_ptr(), None, None, None, None, dp.data_ptr(), n, dp.data_ptr(), n, POS_THRESH,
                                     NEG_THRESH, 1, stream)
            e1.record()
            for _ in range(5):
                lib.hfl_radius_lists(None, idx_a.data_ptr(), idx_b.data_ptr(), off_a.data_ptr(), off_b.data_ptr(),
                                     dp.data_ptr(), n, dp.data_ptr(), n, POS_THRESH, NEG_THRESH, 1, stream)
            e2.record()
            torch.cuda.synchronize()
            count_ms.append(e0.elapsed_time(e1) / 5)
            fill_ms.append(e1.elapsed_time(e2) / 5)
        for name, per in (('count_launch', count_ms[args.warmup:]), ('fill_launch', fill_ms[args.warmup:])):
            ms = statistics.median(per)
            res[name] = {'median_ms': round(ms, 4), 'min_ms': round(min(per), 4), 'max_ms': round(max(per), 4),
                         'pairs': n * n, 'Gpairs_per_s': round(n * n / (ms * 1e-3) / 1e9, 1),
                         'how': '5 back-to-back launches between two HIP events'}
        res['speedup_vs_host'] = round(res['host_numpy']['median_ms'] / res['device_call']['median_ms'], 1)
        res['speedup_vs_sklearn'] = round(res['sklearn_kdtree_and_loop']['median_ms'] / res['device_call']['median_ms'], 1)
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
