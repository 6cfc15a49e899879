"""Build-container only: golden vectors of the reference's TruncatedSmoothAP with `similarity='euclidean'`, the value every
shipped training config resolves to (`/root/reference/misc/utils.py:204`) -> tests/golden/loss_smoothap_euclid.npz, and the
loss settings `TrainingParams` resolves for the four shipped configs -> tests/golden/training_loss_settings.json.

The reference's own class runs in float64 (`torch.cdist` switches to |x|^2 + |y|^2 - 2 x.y above 25 rows, which in float32
costs up to 2e-5 of the largest gradient entry: stored per case as `.ref32_loss_gap` / `.ref32_grad_gap`, for the record).
Inputs are closed-form (`oracle.gen_golden_loss.make_case`), so the file only pins outputs."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import ref_import                       # noqa: E402
from oracle.gen_golden_loss import make_case        # noqa: E402
from loss_cases import CASES, GOLDEN_NAME, SETTINGS_NAME, TAU1, stats_vector        # noqa: E402

CONFIGS = {'wild-places': ('config/config_wild-places.txt', 'models/hotformerloc_wild-places_cfg.txt'),
           'oxford': ('config/config_oxford.txt', 'models/hotformerloc_oxford_cfg.txt'),
           'cs-campus3d': ('config/config_cs-campus3d.txt', 'models/hotformerloc_cs-campus3d_cfg.txt'),
           'cs-wild-places': ('config/config_cs-wild-places.txt', 'models/hotformerloc_cs-wild-places_cfg.txt')}


def run(cls, e, pos, neg, ppq, dtype):
    emb = torch.from_numpy(e).to(dtype).requires_grad_()
    loss, stats = cls(tau1=TAU1, similarity='euclidean', positives_per_query=ppq)(emb, torch.from_numpy(pos), torch.from_numpy(neg))
    loss.backward()
    return loss.item(), emb.grad.numpy().astype(np.float64), stats


def main():
    ref_import.install()
    if not hasattr(np, 'NINF'):
        np.NINF = -np.inf          # the reference targets numpy 1.x (truncated_smoothap.py:37); same value
    from models.losses.truncated_smoothap import TruncatedSmoothAP       # the reference itself
    out = {}
    for name, (seed, batch, dim, group, drop, ppq) in CASES.items():
        e, pos, neg = make_case(seed, batch, dim, group, drop)
        loss, grad, stats = run(TruncatedSmoothAP, e, pos, neg, ppq, torch.float64)
        loss32, grad32, _ = run(TruncatedSmoothAP, e, pos, neg, ppq, torch.float32)
        out[name + '.cfg'] = np.array([seed, batch, dim, group, drop, ppq])
        out[name + '.loss'] = np.float64(loss)
        out[name + '.grad'] = grad
        out[name + '.stats'] = np.array(stats_vector(stats), dtype=np.float64)
        out[name + '.ref32_loss_gap'] = np.float64(abs(loss32 - loss))
        out[name + '.ref32_grad_gap'] = np.float64(np.abs(grad32 - grad).max() / np.abs(grad).max())
        print(name, loss, stats, 'fp32 reference: loss gap %.2e, grad gap / max %.2e'
              % (out[name + '.ref32_loss_gap'], out[name + '.ref32_grad_gap']))
    np.savez_compressed(os.path.join(ROOT, 'tests', 'golden', GOLDEN_NAME), **out)

    from misc.utils import TrainingParams                                  # the reference itself

    class Resolved(TrainingParams):
        def _check_params(self):           # the data sets are not in the build container; nothing else is skipped
            pass

    settings = {}
    for name, (cfg, model_cfg) in CONFIGS.items():
        p = Resolved(os.path.join(ref_import.REFERENCE_ROOT, cfg), os.path.join(ref_import.REFERENCE_ROOT, model_cfg))
        settings[name] = {'loss': p.loss, 'tau1': p.tau1, 'positives_per_query': p.positives_per_query,
                          'similarity': p.similarity}
        print(name, settings[name])
    with open(os.path.join(ROOT, 'tests', 'golden', SETTINGS_NAME), 'w') as f:
        json.dump(settings, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
