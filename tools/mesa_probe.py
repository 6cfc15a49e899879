"""Cost of MESA self-distillation on the BASELINE config-3 workload (CS-Wild-Places, B = 64, one minibatch, AdamW: the settings
of `bench.py --config cs-wild-places --train --multistaged`).  One leg per process (a leg that faults must not be followed by
another on the same card: chain the legs with `&&`, each under its own `timeout`); every leg prints one JSON line.

    python tools/mesa_probe.py --leg plain     (i)   the step without a teacher, REPEATS times: the run-to-run spread
    python tools/mesa_probe.py --leg ema       (ii)  model_ema given, mesa = 0; and ModelEma.update / the launch alone
    python tools/mesa_probe.py --leg mesa      (iii) mesa = 1; teacher forward with and without re-packing, kdloss alone
    python tools/mesa_probe.py --leg user      (iv)  (ii) and (iii) composed from library pieces: copy.deepcopy +
                                                     torch._foreach_lerp_ + the reference's torch formula of kdloss

All times: wall clock around a step with a device synchronisation on both sides, after warm-up; median (min..max) ms."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

os.environ.setdefault('TENSILE_STREAMK_DATA_PARALLEL', '0')        # as bench.py --train
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                                                                    # noqa: E402
from hotformerloc_amd import build_batch_octree, load_config, model_factory, ops   # noqa: E402
from hotformerloc_amd import synthetic as syn                                   # noqa: E402
from hotformerloc_amd.ema import ModelEma                                       # noqa: E402
from hotformerloc_amd.losses import TruncatedSmoothAP, kdloss                  # noqa: E402
from hotformerloc_amd.training import OverlappedGradReducer, multistaged_training_step   # noqa: E402

HBM_PEAK_GBS = 8000.0
BATCH = 64


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {'median_ms': round(statistics.median(ms), 3), 'min_ms': round(min(ms), 3), 'max_ms': round(max(ms), 3)}


def kd_torch(y, teacher):
    """models/losses/loss.py:138-147"""
    p = torch.nn.functional.log_softmax(y / 3, dim=1)
    q = torch.nn.functional.softmax(teacher / 3, dim=1)
    return 50.0 * torch.nn.functional.kl_div(p, q, reduction='batchmean')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--leg', required=True, choices=['plain', 'ema', 'mesa', 'user'])
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    params, depth = load_config('cs-wild-places')
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'init')
    model = model.to(dev).train()
    torch.manual_seed(0)
    clouds = []
    for i in range(BATCH):
        clouds += syn.make_clouds(3, 1, 4096, params.coordinates, kind='forest' if i % 2 == 0 else 'ball',
                                  n_points_max=32768, first_index=i)
    octree = build_batch_octree(clouds, depth, 2, dev, construct_neigh=True)
    batch = {'octree': octree}
    lab = torch.arange(BATCH) // 4
    pos = ((lab[:, None] == lab[None, :]) & ~torch.eye(BATCH, dtype=torch.bool)).to(dev)
    neg = (lab[:, None] != lab[None, :]).to(dev)
    loss_fn = TruncatedSmoothAP(tau1=0.01, positives_per_query=4)
    optim = torch.optim.AdamW(model.parameters(), lr=1e-5)
    reducer = OverlappedGradReducer(model.parameters())

    def step(loss=loss_fn, **kw):
        octree.drop_forward_caches()
        return multistaged_training_step(model, [batch], pos, neg, loss, optim, n_total=BATCH, reducer=reducer, **kw)

    out = {'leg': args.leg, 'steps': args.steps, 'warmup': args.warmup}
    if args.leg == 'plain':
        runs = [timed(step, args.steps, args.warmup if r == 0 else 1) for r in range(args.repeats)]
        meds = [r['median_ms'] for r in runs]
        out.update(step_plain=runs, median_of_medians_ms=statistics.median(meds), spread_ms=round(max(meds) - min(meds), 3))
    elif args.leg == 'ema':
        ema = ModelEma(model)
        out['step_ema_mesa0'] = timed(lambda: step(model_ema=ema, mesa=0.0), args.steps, args.warmup)
        out['ema_update_call'] = timed(lambda: ema.update(model), 20, 3)          # state dicts + stamp + launch + version bump
        table, n = ema._launch[1], ema._launch[2]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        w = 1.0 - ema.decay
        for _ in range(3):
            ops.ema_update(table, n, w)
        e0.record()
        for _ in range(20):
            ops.ema_update(table, n, w)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / 20 * 1e3
        elements = int(table[:, 2].sum())
        gbs = 12.0 * elements / (us * 1e-6) / 1e9
        out['ema_launch'] = {'us': round(us, 1), 'chunks': n, 'elements': elements, 'bytes_moved': 12 * elements,
                             'GBps': round(gbs, 1), 'frac_of_8TBps': round(gbs / HBM_PEAK_GBS, 4),
                             'how': '20 back-to-back launches between two HIP events'}
    elif args.leg == 'mesa':
        ema = ModelEma(model)
        out['step_mesa1'] = timed(lambda: step(model_ema=ema, mesa=1.0), args.steps, args.warmup)
        out['stats'] = {k: v for k, v in step(model_ema=ema, mesa=1.0).items() if k in ('loss', 'mesa_kd')}

        def teacher(update):
            if update:
                ema.update(model)
            octree.drop_forward_caches()
            with torch.no_grad():
                return ema.module(batch)['global']
        out['teacher_forward_packs_cached'] = timed(lambda: teacher(False), args.steps, 2)
        out['teacher_forward_after_update'] = timed(lambda: teacher(True), args.steps, 2)     # includes the update call
        y = torch.nn.functional.normalize(torch.randn(BATCH, 256, device=dev), dim=1)
        t = torch.nn.functional.normalize(y + 0.05 * torch.randn_like(y), dim=1)

        def kd(fn):
            ys = y.clone().requires_grad_()
            fn(ys, t).backward()
        out['kdloss_fwd_bwd'] = timed(lambda: kd(kdloss), 20, 3)
        out['kd_torch_formula_fwd_bwd'] = timed(lambda: kd(kd_torch), 20, 3)
    else:
        teacher = copy.deepcopy(model).eval().requires_grad_(False)
        tp, mp = list(teacher.parameters()), list(model.parameters())

        def lerp():
            with torch.no_grad():
                torch._foreach_lerp_(tp, mp, 1.0 - 0.9998)

        def user_ema():
            step()
            lerp()

        def user_mesa():
            octree.drop_forward_caches()
            with torch.no_grad():
                emb_ema = teacher(batch)['global']

            def loss(e, p, n):
                listwise, stats = loss_fn(e, p, n)
                return listwise + 1.0 * kd_torch(e, emb_ema), stats
            step(loss=loss)
            lerp()
        out['user_step_ema_mesa0'] = timed(user_ema, args.steps, args.warmup)
        out['user_step_mesa1'] = timed(user_mesa, args.steps, args.warmup)
        out['foreach_lerp_call'] = timed(lerp, 20, 3)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
