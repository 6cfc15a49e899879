"""MESA self-distillation, the parts that need no GPU: the golden file of the reference's `kdloss` is self-consistent, the
layout of `ModelEma`'s state dict (the reference's `model_ema_state_dict` checkpoint entry), argument checks."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hotformerloc_amd import load_config, model_factory       # noqa: E402
from hotformerloc_amd import synthetic as syn                  # noqa: E402
from hotformerloc_amd._native import NativeLibraryError        # noqa: E402
from hotformerloc_amd.ema import ModelEma                      # noqa: E402
from hotformerloc_amd.losses import kdloss                     # noqa: E402
from hotformerloc_amd.training import multistaged_training_step    # noqa: E402

KD_CASES = ['b8', 'b64', 'b257', 'b48_d128', 'b64_x20']


def kd_fp64(y, t, T=3.0, weight=50.0):
    """`weight * KLDivLoss('batchmean')(log_softmax(y / T), softmax(t / T))` and its gradient with respect to y, restated in
    float64 numpy: loss = weight / B * sum_ij q_ij (log q_ij - log p_ij), gradient = weight / B * (p - q) / T."""
    y, t = y.astype(np.float64) / T, t.astype(np.float64) / T

    def log_softmax(x):
        x = x - x.max(1, keepdims=True)
        return x - np.log(np.exp(x).sum(1, keepdims=True))
    lp, lq = log_softmax(y), log_softmax(t)
    q = np.exp(lq)
    b = y.shape[0]
    return weight / b * (q * (lq - lp)).sum(), weight / b * (np.exp(lp) - q) / T


@pytest.mark.parametrize('case', KD_CASES)
def test_golden_is_the_stated_formula(golden_dir, case):
    g = np.load(os.path.join(golden_dir, 'mesa.npz'))
    seed, batch, dim, scale = g[case + '.cfg']
    y, t = syn.kd_case(int(seed), int(batch), int(dim), float(scale))
    loss, grad = kd_fp64(y, t)
    assert abs(loss - float(g[case + '.loss64'])) <= 1e-12 * abs(loss)
    want = g[case + '.grad64']
    assert want.dtype == np.float64 and want.shape == y.shape
    assert np.abs(grad - want).max() <= 1e-12 * np.abs(want).max()
    # the reference's own fp32 run is no better than these figures; a bar below them would ask more than the reference gives
    assert (g[case + '.ref32_max'] >= g[case + '.ref32_err']).all() and (g[case + '.ref32_max'] > 0).all()


def test_golden_stage2_is_listwise_plus_kd(golden_dir):
    from oracle import loss_ref
    from oracle.gen_golden_loss import make_case
    from tools.gen_golden_mesa import stage2_teacher
    g = np.load(os.path.join(golden_dir, 'mesa.npz'))
    e, pos, neg = make_case(11, 64, 256, 4, 0)
    emb = torch.from_numpy(e).requires_grad_()
    listwise, _ = loss_ref.truncated_smooth_ap(emb, torch.from_numpy(pos), torch.from_numpy(neg), 0.01, 4)
    listwise.backward()
    kd, kd_grad = kd_fp64(e, stage2_teacher(e))
    assert abs(float(g['stage2.loss']) - (listwise.item() + kd)) < 2e-6
    # the stored parts are the reference's fp32 results: its KD term carries its own fp32 error (b64 shape: ref32_max)
    assert abs(float(g['stage2.loss_kd']) - kd) <= 4 * g['b64.ref32_max'][0] * kd
    assert abs(float(g['stage2.loss_listwise']) - listwise.item()) < 2e-6
    want = g['stage2.grad']
    assert np.abs(emb.grad.numpy() + kd_grad - want).max() <= 2e-5 * np.abs(want).max() + 1e-7
    # the listwise loss of loss_smoothap.npz's b64 case: the same inputs
    assert abs(float(np.load(os.path.join(golden_dir, 'loss_smoothap.npz'))['b64.loss']) - float(g['stage2.loss_listwise'])) < 1e-7


def test_model_ema_state_dict_layout_and_round_trip():
    params, _ = load_config('cs-wild-places')
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'stress')
    model.train()
    ema = ModelEma(model, decay=0.9998)
    sd, msd = ema.state_dict(), model.state_dict()
    assert list(sd.keys()) == ['module.' + k for k in msd.keys()]
    assert len(sd) == 726 and sum(v.numel() for v in sd.values()) == 35371176
    assert all(torch.equal(sd['module.' + k], v) and sd['module.' + k].data_ptr() != v.data_ptr() for k, v in msd.items())
    assert not ema.module.training and model.training
    assert not any(p.requires_grad for p in ema.parameters()) and all(p.requires_grad for p in model.parameters())
    ema.train()
    assert not ema.module.training                      # the teacher stays in eval mode
    # what a checkpoint holds under `model_ema_state_dict` loads into a teacher made from another model
    other = model_factory(params)
    ema2 = ModelEma(other)
    res = ema2.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(v, sd[k]) for k, v in ema2.state_dict().items())
    with pytest.raises(ValueError):
        ModelEma(other, decay=1.5)


def test_model_ema_update_has_no_cpu_path():
    m = torch.nn.Linear(4, 4)
    ema = ModelEma(m, decay=0.5)
    with pytest.raises(NativeLibraryError):
        ema.update(m)
    bad = torch.nn.Linear(4, 5)
    with pytest.raises((KeyError, ValueError, NativeLibraryError)):
        ema.update(bad)


def test_kdloss_argument_checks():
    y = torch.zeros(4, 64, requires_grad=True)
    with pytest.raises(ValueError):
        kdloss(y, torch.zeros(4, 64, requires_grad=True))
    with pytest.raises(NativeLibraryError):
        kdloss(y, torch.zeros(4, 64))


def test_step_argument_checks():
    calls = []

    class Toy(torch.nn.Module):
        def forward(self, mb):
            calls.append(1)
            raise AssertionError('the step must refuse its arguments before it runs the model')

    eye = torch.eye(2, dtype=torch.bool)
    with pytest.raises(ValueError):
        multistaged_training_step(Toy(), [{}], eye, ~eye, lambda *a: None, mesa=1.0)
    with pytest.raises(ValueError):
        multistaged_training_step(Toy(), [{}], eye, ~eye, lambda *a: None, mesa=-1.0, model_ema=ModelEma(Toy()))
    assert not calls
