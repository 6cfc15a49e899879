"""Streamed flat-L2 search against the dense f64 search on the same descriptors, same process.

    python tools/retrieval_probe.py --shape small      (Q, N, D) = (400, 400, 256), the golden size
    python tools/retrieval_probe.py --shape large      (Q, N, D) = (4096, 32768, 256), an evaluation-sized pair

One shape per process (chain the two with `&&`, each under its own `timeout`); prints one JSON line.  Per leg: warm-up, then
REPEATS runs each between two HIP events on the launch stream, median (min..max) ms; inputs and the index are made outside
the timed region.  Legs: `FlatL2Index.search(k=25, refine=True)`, the kernel launches alone (`refine=False`, k = 32: what the
refined search runs), `retrieval.flat_l2_topk(k=25)`.  `kernel_frac_of_fp32_matrix_peak` = 2 Q N D FLOP over the kernel leg's
median against 157.3 TF; peak memory = growth of `torch.cuda.max_memory_allocated()` across one call of the leg."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                                        # noqa: E402
from hotformerloc_amd import retrieval             # noqa: E402

FP32_MATRIX_PEAK_TF = 157.3
SHAPES = {'small': (400, 400, 256), 'large': (4096, 32768, 256)}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', required=True, choices=sorted(SHAPES))
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    q_rows, n, d = SHAPES[args.shape]
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(1)
    db = torch.nn.functional.normalize(torch.rand((n, d), device=dev, generator=gen) - 0.5, dim=1)
    q = torch.nn.functional.normalize(torch.rand((q_rows, d), device=dev, generator=gen) - 0.5, dim=1)
    index = retrieval.FlatL2Index(db)
    out = {'shape': {'Q': q_rows, 'N': n, 'D': d}, 'repeats': args.repeats, 'warmup': args.warmup}
    out['index_search_refined'] = timed(lambda: index.search(q, k=25), args.repeats, args.warmup)
    out['kernel_only_k32'] = timed(lambda: index.search(q, k=32, refine=False), args.repeats, args.warmup)
    out['dense_flat_l2_topk'] = timed(lambda: retrieval.flat_l2_topk(db, q, 25), args.repeats, args.warmup)
    _, want = retrieval.flat_l2_topk(db, q, 25)
    _, got = index.search(q, k=25)
    out['indices_equal'] = bool(torch.equal(want, got))
    out['dense_over_streamed'] = round(out['dense_flat_l2_topk']['median_ms'] / out['index_search_refined']['median_ms'], 2)
    tf = 2.0 * q_rows * n * d / (out['kernel_only_k32']['median_ms'] * 1e-3) / 1e12
    out['kernel_TF'] = round(tf, 2)
    out['kernel_frac_of_fp32_matrix_peak'] = round(tf / FP32_MATRIX_PEAK_TF, 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
