"""Cost and accuracy of the training loss at the shipped recipe's size: B = 2048 embeddings of D = 256, 4 positives per query,
tau1 = 0.01 (`hotformerloc_amd.synthetic`-seeded unit rows in groups of 5, the case of tests/test_gpu_loss_euclid.py).
A call is `loss, stats = loss_fn(emb, pos, neg); loss.backward()`: forward, the stats' host reads, backward to d emb.

    (a) cosine      TruncatedSmoothAP(similarity='cosine'): E E^T and dE = (dS + dS^T) E as dense torch ops
    (b) euclidean   TruncatedSmoothAP(similarity='euclidean') on hfl_pairwise_dist / hfl_pairwise_dist_bwd
    (c) cdist       the same class with the affinity taken from -torch.cdist(E, E) and torch autograd (the reference's own
                    route, loss_utils.py:55-60), feeding the same hfl_smoothap_rows kernel

The three routes alternate call by call inside one process, so they meet the same machine state.  Wall clock around a call with
a device synchronisation on both sides, median (min..max) of STEPS calls per route after WARMUP; for (b) also each kernel alone,
20 back-to-back launches between two HIP events, with its arithmetic (one subtract and one fused multiply-add per (i, j, k):
B^2 D / 2 of them forward, on and above the diagonal, B^2 D backward) against the 157.3 TFLOP/s fp32 vector peak.  Accuracy: each
route's loss and gradient against the float64 restatement of tests/loss_cases.py.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np                                                              # noqa: E402
import torch                                                                    # noqa: E402
import loss_cases as lc                                                         # noqa: E402
from hotformerloc_amd import losses, ops                                        # noqa: E402

FP32_PEAK_TFLOPS = 157.3
CASE = (21, 2048, 256, 5, 17, 4)


def cdist_affinity(emb):
    x = emb.float().unsqueeze(0)
    return -torch.cdist(x, x, p=2).squeeze(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--no-accuracy', action='store_true', help='skip the float64 yardstick (about 2 s of CPU)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('loss_probe needs a GPU: a CPU run says nothing about these times')
    seed, batch, dim, group, drop, ppq = CASE
    e, pos, neg = lc.make_case(seed, batch, dim, group, drop)
    pos, neg = torch.from_numpy(pos).cuda(), torch.from_numpy(neg).cuda()
    native_affinity = losses.euclidean_affinity
    routes = {'cosine': (losses.TruncatedSmoothAP(lc.TAU1, 'cosine', ppq), native_affinity),
              'euclidean': (losses.TruncatedSmoothAP(lc.TAU1, 'euclidean', ppq), native_affinity),
              'cdist': (losses.TruncatedSmoothAP(lc.TAU1, 'euclidean', ppq), cdist_affinity)}

    def call(name):
        loss_fn, affinity = routes[name]
        losses.euclidean_affinity = affinity
        try:
            emb = torch.from_numpy(e).cuda().requires_grad_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss, _ = loss_fn(emb, pos, neg)
            loss.backward()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, loss.item(), emb.grad
        finally:
            losses.euclidean_affinity = native_affinity

    ms = {name: [] for name in routes}
    last = {}
    for k in range(args.warmup + args.steps):
        for name in routes:
            t, loss, grad = call(name)
            if k >= args.warmup:
                ms[name].append(t)
            last[name] = (loss, grad)
    out = {'batch': batch, 'dim': dim, 'positives_per_query': ppq, 'steps': args.steps, 'warmup': args.warmup, 'call_ms': {}}
    for name, v in ms.items():
        out['call_ms'][name] = {'median': round(statistics.median(v), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)}
    med = {name: statistics.median(v) for name, v in ms.items()}
    out['euclidean_minus_cdist_ms'] = round(med['euclidean'] - med['cdist'], 3)
    out['euclidean_minus_cosine_ms'] = round(med['euclidean'] - med['cosine'], 3)

    emb = torch.from_numpy(e).cuda()
    gd = torch.from_numpy(np.random.RandomState(0).standard_normal((batch, batch)).astype(np.float32)).cuda()
    dist = ops.pairwise_dist(emb)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kernels = {'hfl_pairwise_dist': (lambda: ops.pairwise_dist(emb), batch * batch * dim / 2),
               'hfl_pairwise_dist_bwd': (lambda: ops.pairwise_dist_bwd(gd, dist, emb), batch * batch * dim)}
    out['kernel'] = {}
    for name, (fn, pairs) in kernels.items():
        for _ in range(3):
            fn()
        e0.record()
        for _ in range(20):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / 20 * 1e3
        tflops = 3 * pairs / (us * 1e-6) / 1e12                  # a subtract and an FMA: 3 flop per (i, j, k)
        out['kernel'][name] = {'us': round(us, 1), 'TFLOPs': round(tflops, 2),
                               'frac_of_fp32_vector_peak': round(tflops / FP32_PEAK_TFLOPS, 4),
                               'how': '20 back-to-back launches between two HIP events'}
    if not args.no_accuracy:
        _, _, _, want, gref, _ = lc.yardstick(*CASE)
        cos_ref = torch.from_numpy(e).double().requires_grad_()
        from oracle import loss_ref
        cos_want, _ = loss_ref.truncated_smooth_ap(cos_ref, pos.cpu(), neg.cpu(), lc.TAU1, ppq)
        cos_want.backward()
        refs = {'cosine': (cos_want.item(), cos_ref.grad.numpy()), 'euclidean': (want, gref), 'cdist': (want, gref)}
        out['vs_float64'] = {}
        for name, (loss, grad) in last.items():
            w, g = refs[name]
            out['vs_float64'][name] = {'loss_err': float('%.3g' % abs(loss - w)),
                                       'grad_err_over_max': float('%.3g' % (np.abs(grad.cpu().numpy() - g).max() / np.abs(g).max()))}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
