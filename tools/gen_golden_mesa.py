"""Build container only: golden vectors of the reference's MESA distillation loss (`models/losses/loss.py:138-147`, `kdloss`)
and of its stage-2 sum `TruncatedSmoothAP + mesa * kdloss` (`training/trainer.py:327-336`) -> tests/golden/mesa.npz.

Inputs are closed-form (`hotformerloc_amd.synthetic.kd_case`, `oracle.gen_golden_loss.make_case`), so the file pins only
seeds and outputs.  Per distillation case `<name>`:
  .cfg        seed, batch, dim, scale
  .loss64     kdloss on float64 inputs (the float32 rows, widened)
  .grad64     its gradient with respect to the student rows, float64
  .ref32_err  the reference's own float32 run against its float64 run ON THIS CASE: (relative loss error, gradient rel-L2)
  .ref32_max  the largest of both figures over the 8 seeds seed .. seed + 7 of this shape: a single case's fp32 error is
              partly luck (the KL of nearly equal rows is a small difference of nearly equal numbers), the bar of a test is
              taken from this maximum
and for the case `stage2`: `.loss` / `.grad` (float32, as loss_smoothap.npz stores them) of
TruncatedSmoothAP(tau1=0.01, positives_per_query=4) + 1.0 * kdloss on the `b64` inputs, plus `.loss_listwise`, `.loss_kd`,
`.grad_listwise_absmax`, `.grad_kd_absmax` for the negative control."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hotformerloc_amd import synthetic as syn    # noqa: E402

CASES = {'b8': (31, 8, 256, 1.0), 'b64': (41, 64, 256, 1.0), 'b257': (51, 257, 256, 1.0), 'b48_d128': (61, 48, 128, 1.0),
         'b64_x20': (71, 64, 256, 20.0)}
SEEDS_PER_SHAPE = 8


def stage2_teacher(e: np.ndarray) -> np.ndarray:
    t = e + 2.0 * (syn.hash_uniform(99, e.size).reshape(e.shape).astype(np.float32) - 0.5)
    return (t / np.linalg.norm(t, axis=1, keepdims=True)).astype(np.float32)


def import_reference():
    from oracle import ref_import
    ref_import.install()
    if not hasattr(np, 'NINF'):
        np.NINF = -np.inf          # the reference targets numpy 1.x; same value
    # models.losses.loss imports pytorch_metric_learning at module level and uses it only in losses this project does not
    # ship: empty stand-ins let the module import
    pml = types.ModuleType('pytorch_metric_learning')
    for sub in ('losses', 'reducers', 'distances'):
        m = types.ModuleType('pytorch_metric_learning.' + sub)
        setattr(pml, sub, m)
        sys.modules['pytorch_metric_learning.' + sub] = m
    sys.modules['pytorch_metric_learning.distances'].LpDistance = object
    sys.modules['pytorch_metric_learning'] = pml
    from models.losses.loss import kdloss
    from models.losses.truncated_smoothap import TruncatedSmoothAP
    return kdloss, TruncatedSmoothAP


def run(kdloss, y: np.ndarray, t: np.ndarray, dtype):
    ys = torch.from_numpy(y).to(dtype).requires_grad_()
    loss = kdloss(ys, torch.from_numpy(t).to(dtype))
    loss.backward()
    return loss.item(), ys.grad.numpy()


def main():
    kdloss, TruncatedSmoothAP = import_reference()
    out = {}
    for name, (seed, batch, dim, scale) in CASES.items():
        errs = []
        for s in range(seed, seed + SEEDS_PER_SHAPE):
            y, t = syn.kd_case(s, batch, dim, scale)
            l64, g64 = run(kdloss, y, t, torch.float64)
            l32, g32 = run(kdloss, y, t, torch.float32)
            errs.append((abs(l32 - l64) / abs(l64), np.linalg.norm(g32 - g64) / np.linalg.norm(g64)))
            if s == seed:
                out[name + '.cfg'] = np.array([seed, batch, dim, scale], dtype=np.float64)
                out[name + '.loss64'] = np.float64(l64)
                out[name + '.grad64'] = g64
                out[name + '.ref32_err'] = np.array(errs[0], dtype=np.float64)
        out[name + '.ref32_max'] = np.array(errs, dtype=np.float64).max(0)
        print(name, 'loss', out[name + '.loss64'], 'ref fp32 err (loss, grad)', out[name + '.ref32_err'], 'max over seeds',
              out[name + '.ref32_max'])
    from oracle.gen_golden_loss import make_case
    e, pos, neg = make_case(11, 64, 256, 4, 0)
    emb = torch.from_numpy(e).requires_grad_()
    listwise, _ = TruncatedSmoothAP(tau1=0.01, positives_per_query=4)(emb, torch.from_numpy(pos), torch.from_numpy(neg))
    kd = kdloss(emb, torch.from_numpy(stage2_teacher(e)))
    g_list = torch.autograd.grad(listwise, emb, retain_graph=True)[0]
    g_kd = torch.autograd.grad(kd, emb, retain_graph=True)[0]
    loss = listwise + 1.0 * kd
    loss.backward()
    out['stage2.loss'] = np.float32(loss.item())
    out['stage2.grad'] = emb.grad.numpy()
    out['stage2.loss_listwise'] = np.float32(listwise.item())
    out['stage2.loss_kd'] = np.float32(kd.item())
    out['stage2.grad_listwise_absmax'] = np.float32(g_list.abs().max().item())
    out['stage2.grad_kd_absmax'] = np.float32(g_kd.abs().max().item())
    print('stage2', loss.item(), listwise.item(), kd.item(), g_list.abs().max().item(), g_kd.abs().max().item())
    path = os.path.join(ROOT, 'tests', 'golden', 'mesa.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
