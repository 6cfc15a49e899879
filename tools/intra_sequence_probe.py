"""Causal (prefix-limited) flat-L2 search of one run against itself: the triangular streamed search, the unrestricted
streamed search at the same size, and the dense masked float64 route, same descriptors, same process.

    python tools/intra_sequence_probe.py                 Q = N = 20 000, D = 256: a long Wild-Places run
    python tools/intra_sequence_probe.py --n 4096        a smaller run (the dense leg holds several (N, N) float64 matrices)

Prints one JSON line.  The run is one scan per second, `causal_limits(t, 600)`: scan i sees scans [0, i - 599).  Per leg:
warm-up, then REPEATS runs each between two HIP events on the launch stream, median (min..max) ms; inputs, limits and the
index are made outside the timed region.  Legs: `FlatL2Index.search(k=25, limits=)` refined and its kernel launches alone
(`refine=False`, k = 32), the same two without limits (`hfl_flat_l2_topk` over the whole square), and the dense route: the
(N, N) float64 distance matrix, columns >= limits[i] set to +inf, a stable argsort.  `prefix_over_full_kernel` is the ratio
of the two kernel legs (the triangle holds about half the tiles of the square); peak memory = growth of
`torch.cuda.max_memory_allocated()` across one call of the leg."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                                        # noqa: E402
from hotformerloc_amd import retrieval             # noqa: E402

TIME_THRESH = 600.0


def timed(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4),
            'peak_MiB': round(peak / 2.0 ** 20, 1)}


def dense_masked_topk(db, limits, k):
    """(N, N) float64 distances, the columns a scan may not see at +inf, stable argsort: (d2, idx) with +inf / -1 past the
    prefix"""
    x = db.double()
    sq = (x * x).sum(1)
    d2 = sq[:, None] + sq[None, :] - 2.0 * (x @ x.t())
    d2.masked_fill_(torch.arange(x.shape[0], device=x.device)[None, :] >= limits[:, None], float('inf'))
    order = torch.argsort(d2, dim=1, stable=True)[:, :k]
    got = d2.gather(1, order)
    return got, torch.where(torch.isinf(got), torch.full_like(order, -1), order)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=20000)
    ap.add_argument('--dim', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-dense', action='store_true', help='skip the dense float64 leg')
    args = ap.parse_args()
    n, d = args.n, args.dim
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(1)
    db = torch.nn.functional.normalize(torch.rand((n, d), device=dev, generator=gen) - 0.5, dim=1)
    limits = retrieval.causal_limits(1.6e9 + torch.arange(n, device=dev, dtype=torch.float64), TIME_THRESH)
    index = retrieval.FlatL2Index(db)
    out = {'shape': {'Q': n, 'N': n, 'D': d}, 'time_thresh': TIME_THRESH, 'repeats': args.repeats, 'warmup': args.warmup,
           'pairs_inside_limits_frac': round(float(limits.double().sum().item()) / (float(n) * n), 4)}
    out['prefix_search_refined'] = timed(lambda: index.search(db, k=25, limits=limits), args.repeats, args.warmup)
    out['prefix_kernel_only_k32'] = timed(lambda: index.search(db, k=32, refine=False, limits=limits), args.repeats,
                                          args.warmup)
    out['full_search_refined'] = timed(lambda: index.search(db, k=25), args.repeats, args.warmup)
    out['full_kernel_only_k32'] = timed(lambda: index.search(db, k=32, refine=False), args.repeats, args.warmup)
    out['prefix_over_full_kernel'] = round(out['prefix_kernel_only_k32']['median_ms'] /
                                           out['full_kernel_only_k32']['median_ms'], 3)
    if not args.no_dense:
        out['dense_masked_f64'] = timed(lambda: dense_masked_topk(db, limits, 25), args.repeats, args.warmup)
        _, want = dense_masked_topk(db, limits, 25)
        _, got = index.search(db, k=25, limits=limits)
        out['indices_equal'] = bool(torch.equal(want, got))
        out['dense_over_prefix'] = round(out['dense_masked_f64']['median_ms'] / out['prefix_search_refined']['median_ms'], 2)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
