"""GEMM mode x6 training on hand-written kernels: (1) hfl_wgrad_f32 against the fp32 library's dy^T x (+ column sum) on the
weight-gradient shapes of the training step, with the error of each against fp64; (2) one BASELINE config-3 forward + backward
(CS-Wild-Places, B = 64) in three setups: x6 with the hand-written route, x6 with set_train_x6(False) (fp32 library GEMMs),
and x3.

    python tools/train_x6_probe.py [--steps 3] [--warmup 2] [--no-step]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hotformerloc_amd import build_batch_octree, load_config, model_factory, ops  # noqa: E402
from hotformerloc_amd import synthetic as syn  # noqa: E402
from hotformerloc_amd.model import set_gemm_mode, set_train_x6  # noqa: E402


def timeit(fn, n=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3          # us


def wgrad_table():
    print('%-10s %7s %5s %5s | %-34s | %-34s' % ('layer', 'M', 'N', 'K', 'hfl_wgrad_f32 (dW + db)', 'dy.t() @ x + dy.sum(0)'))
    for m, n, k, tag in [(68167, 768, 256, 'qkv d4'), (68167, 256, 256, 'proj d4'), (68167, 1024, 256, 'fc1 d4'),
                         (68167, 256, 1024, 'fc2 d4'), (118096, 384, 128, 'qkv d5'), (118096, 512, 128, 'fc1 d5'),
                         (118096, 128, 512, 'fc2 d5'), (300000, 1024, 256, 'fc1 d4 cs'), (300000, 256, 1024, 'fc2 d4 cs'),
                         (14276, 1024, 256, 'fc1 d3')]:
        dy = torch.randn(m, n, device='cuda')
        x = torch.randn(m, k, device='cuda')
        ref = dy.double().t() @ x.double()
        dw, _ = ops.wgrad_f32(dy, x, with_bias=True)
        err = ((dw.double() - ref).norm() / ref.norm()).item()
        e32 = ((torch.mm(dy.t(), x).double() - ref).norm() / ref.norm()).item()
        t6 = timeit(lambda: ops.wgrad_f32(dy, x, with_bias=True))
        t32 = timeit(lambda: (torch.mm(dy.t(), x), dy.sum(0)))
        fl = 2.0 * m * n * k
        print('%-10s %7d %5d %5d | %8.1f us %5.1f TF/s err %.1e | %8.1f us %5.1f TF/s err %.1e'
              % (tag, m, n, k, t6, fl / t6 / 1e6, err, t32, fl / t32 / 1e6, e32))


def step_table(steps, warmup):
    params, depth = load_config('cs-wild-places')
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'init')
    model = model.cuda().train()
    clouds = []
    for i in range(64):
        clouds += syn.make_clouds(3, 1, 4096, 'cartesian', kind='forest' if i % 2 == 0 else 'ball', n_points_max=32768,
                                  first_index=i)
    octree = build_batch_octree(clouds, depth, 2, 'cuda')
    proj = torch.from_numpy(syn.hash_uniform(99, 64 * params.output_dim).reshape(64, params.output_dim)
                            .astype(np.float32)).cuda()

    def step():
        model.zero_grad(set_to_none=True)
        y = model({'octree': octree})['global']
        (y * proj).sum().backward()

    for label, mode, route in (('x6, hand-written route', 'x6', True), ('x6, set_train_x6(False)', 'x6', False),
                               ('x3', 'x3', True)):
        set_gemm_mode(mode)
        set_train_x6(route)
        try:
            torch.manual_seed(0)
            for _ in range(warmup):
                step()
            torch.cuda.synchronize()
            times = []
            for _ in range(steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step()
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
        finally:
            set_train_x6(True)
            set_gemm_mode('x3')
        print('config-3 forward + backward, %-24s median %7.1f ms  (%s)' % (label, float(np.median(times)),
                                                                           ', '.join('%.1f' % t for t in times)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-step', action='store_true')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    wgrad_table()
    if not args.no_step:
        step_table(args.steps, args.warmup)


if __name__ == '__main__':
    main()
