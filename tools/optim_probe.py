"""Cost of the optimizer step (and the EMA update behind it) on the config-3 model (CS-Wild-Places: 726 fp32 tensors,
35 371 176 elements; synthetic weights and gradients, lr 8e-4, weight decay 1e-4 folded into the gradient: what the shipped
configs train with).  One leg per process (a leg that faults must not be followed by another on the same card: chain the legs
with `&&`, each under its own `timeout`); every leg prints one JSON line.

    python tools/optim_probe.py --leg adam              torch.optim.Adam at its default (foreach)
    python tools/optim_probe.py --leg adam_fused        torch.optim.Adam(fused=True)
    python tools/optim_probe.py --leg adam_ema          the first, followed by ModelEma.update
    python tools/optim_probe.py --leg adam_fused_ema    the second, followed by ModelEma.update
    python tools/optim_probe.py --leg fusedadam         FusedAdam without a teacher
    python tools/optim_probe.py --leg fusedadam_ema     FusedAdam with the teacher attached

A call is what follows the backward in a training step: `optimizer.step()` (then `model_ema.update(model)`).  Before every
call the gradients are set to the other of two sets of tensors, outside the timed region, so every call meets gradients at
new addresses as it does after `zero_grad()`.  Wall clock around a call with a device synchronisation on both sides, median
(min..max) of STEPS calls after WARMUP; for the FusedAdam legs also the launch alone, 20 back to back between two HIP events,
and its traffic (28 B per element, 36 B with the teacher) against the 8 TB/s HBM peak."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np                                                              # noqa: E402
import torch                                                                    # noqa: E402
from hotformerloc_amd import FusedAdam, load_config, model_factory, ops         # noqa: E402
from hotformerloc_amd import synthetic as syn                                   # noqa: E402
from hotformerloc_amd.ema import ModelEma                                       # noqa: E402

HBM_PEAK_GBS = 8000.0
LR, WEIGHT_DECAY = 8e-4, 1e-4
LEGS = ['adam', 'adam_fused', 'adam_ema', 'adam_fused_ema', 'fusedadam', 'fusedadam_ema']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--leg', required=True, choices=LEGS)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    params, _ = load_config('cs-wild-places')
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'init')
    model = model.to(dev).train()
    plist = list(model.parameters())
    grad_sets = [[torch.from_numpy((1e-2 * syn.hash_uniform(1000 * s + i, p.numel())).astype(np.float32)).reshape(p.shape).to(dev)
                  for i, p in enumerate(plist)] for s in range(2)]
    with_ema = args.leg.endswith('_ema')
    ema = ModelEma(model) if with_ema else None
    if args.leg.startswith('fusedadam'):
        optim = FusedAdam(plist, lr=LR, weight_decay=WEIGHT_DECAY)
        if with_ema:
            optim.attach_ema(ema, model)
    else:
        optim = torch.optim.Adam(plist, lr=LR, weight_decay=WEIGHT_DECAY, fused=True if 'fused' in args.leg else None)

    def call():
        optim.step()
        if with_ema and not args.leg.startswith('fusedadam'):
            ema.update(model)

    ms = []
    for k in range(args.warmup + args.steps):
        for p, g in zip(plist, grad_sets[k % 2]):
            p.grad = g
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if k >= args.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    out = {'leg': args.leg, 'steps': args.steps, 'warmup': args.warmup, 'tensors': len(plist),
           'elements': sum(p.numel() for p in plist),
           'call': {'median_ms': round(statistics.median(ms), 3), 'min_ms': round(min(ms), 3), 'max_ms': round(max(ms), 3)}}
    if args.leg.startswith('fusedadam'):
        table = optim._plan.table
        w = 1.0 - ema.decay if with_ema else 0.0
        slots = [ops.adam_slot(LR, 0.9, 0.999, 1e-8, WEIGHT_DECAY, False, args.warmup + args.steps + 1)]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(3):
            ops.adam_step(table, slots, w)
        e0.record()
        for _ in range(20):
            ops.adam_step(table, slots, w)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / 20 * 1e3
        per_element = 36 if with_ema else 28
        gbs = per_element * out['elements'] / (us * 1e-6) / 1e9
        out['launch'] = {'us': round(us, 1), 'chunks': table.n_chunks, 'launches': len(table.launches),
                         'bytes_moved': per_element * out['elements'], 'GBps': round(gbs, 1),
                         'frac_of_8TBps': round(gbs / HBM_PEAK_GBS, 4), 'how': '20 back-to-back launches between two HIP events'}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
