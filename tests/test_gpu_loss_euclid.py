"""GPU TruncatedSmoothAP with `similarity='euclidean'` (what the shipped training configs resolve to): the golden values of
the reference's own class in float64, the float64 restatement of tests/loss_cases.py at the training batch size, the
untouched cosine path, and one multi-staged training step with the loss `make_losses` builds."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import loss_cases as lc
from hotformerloc_amd.losses import TruncatedSmoothAP, euclidean_affinity, make_losses

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', sorted(lc.CASES))
def test_euclidean_loss_matches_reference_golden(golden_dir, case):
    """The bars of tests/test_gpu_loss.py:28-34."""
    g = lc.load_golden(golden_dir)
    seed, batch, dim, group, drop, ppq = [int(v) for v in g[case + '.cfg']]
    e, pos, neg = lc.make_case(seed, batch, dim, group, drop)
    emb = torch.from_numpy(e).cuda().requires_grad_()
    loss_fn = TruncatedSmoothAP(tau1=lc.TAU1, similarity='euclidean', positives_per_query=ppq)
    loss, stats = loss_fn(emb, torch.from_numpy(pos), torch.from_numpy(neg))
    loss.backward()
    gref = g[case + '.grad']
    print(case, 'loss err', abs(loss.item() - float(g[case + '.loss'])), 'grad err / max',
          np.abs(emb.grad.cpu().numpy() - gref).max() / np.abs(gref).max(),
          '(the reference in fp32: %.2e, %.2e)' % (float(g[case + '.ref32_loss_gap']), float(g[case + '.ref32_grad_gap'])))
    assert abs(loss.item() - float(g[case + '.loss'])) < 2e-6
    assert np.abs(emb.grad.cpu().numpy() - gref).max() <= 2e-5 * max(np.abs(gref).max(), 1e-6) + 1e-7
    got = [stats['positives_per_query'], stats['ap'], stats['avg_embedding_norm']]
    assert np.allclose(got, g[case + '.stats'][[0, 3, 4]], atol=2e-6)
    if drop == 0:          # rows without positives pick an arbitrary "best positive" in the reference
        assert np.allclose([stats['best_positive_ranking'], stats['recall'][1]], g[case + '.stats'][[1, 2]], atol=1e-6)


def test_euclidean_loss_at_training_batch_size_matches_float64():
    """batch_size = 2048, positives_per_query = 4, tau1 = 0.01; groups of 5 give exactly 4 positives per query, so the
    selected set cannot flip on a near tie.  The bars of tests/test_gpu_loss.py:48-54."""
    e, pos, neg, want, gref, wstats = lc.yardstick(21, 2048, 256, 5, 17, 4)
    emb = torch.from_numpy(e).cuda().requires_grad_()
    loss, stats = TruncatedSmoothAP(tau1=lc.TAU1, similarity='euclidean', positives_per_query=4)(
        emb, torch.from_numpy(pos), torch.from_numpy(neg))
    loss.backward()
    err = np.abs(emb.grad.cpu().numpy() - gref).max() / np.abs(gref).max()
    print('B=2048 euclidean loss', loss.item(), want, 'diff', abs(loss.item() - want), 'grad err / max', err,
          'ap diff', abs(stats['ap'] - wstats['ap']))
    assert abs(loss.item() - want) < 5e-6
    assert err <= 3e-4
    assert abs(stats['ap'] - wstats['ap']) < 5e-6


def test_euclidean_affinity_takes_an_arbitrary_gradient():
    """-dist and the gradient of sum(G * affinity) for a non-symmetric G, against float64 autograd through cdist."""
    e = lc.make_case(41, 70, 40, 5, 0)[0]
    g = torch.from_numpy(np.random.RandomState(3).standard_normal((70, 70)).astype(np.float32))
    x = torch.from_numpy(e).double().requires_grad_()
    want = -torch.cdist(x, x, compute_mode='donot_use_mm_for_euclid_dist')
    (want * g.double()).sum().backward()
    emb = torch.from_numpy(e).cuda().requires_grad_()
    aff = euclidean_affinity(emb)
    (aff * g.cuda()).sum().backward()
    u, d64, g64, xd = 2.0 ** -24, -want.detach(), g.double(), x.detach()
    assert ((aff.detach().cpu().double() + d64).abs() <= (40 / 2 + 2) * u * d64).all()          # tests/test_gpu_pairwise.py's bounds
    w = torch.where(d64 > 0, (g64 + g64.t()).abs() / torch.where(d64 > 0, d64, torch.ones_like(d64)), torch.zeros_like(d64))
    mag = (w[:, :, None] * (xd[:, None, :] - xd[None, :, :]).abs()).sum(1)
    assert ((emb.grad.cpu().double() - x.grad).abs() <= (70 + 40 / 2 + 8) * u * mag).all()


def test_cosine_path_still_reproduces_its_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'loss_smoothap.npz'))
    seed, batch, dim, group, drop, ppq = [int(v) for v in g['b64.cfg']]
    e, pos, neg = lc.make_case(seed, batch, dim, group, drop)
    emb = torch.from_numpy(e).cuda().requires_grad_()
    loss, stats = TruncatedSmoothAP(tau1=0.01, positives_per_query=ppq)(emb, torch.from_numpy(pos), torch.from_numpy(neg))
    loss.backward()
    assert abs(loss.item() - float(g['b64.loss'])) < 2e-6
    gref = g['b64.grad']
    assert np.abs(emb.grad.cpu().numpy() - gref).max() <= 2e-5 * max(np.abs(gref).max(), 1e-6) + 1e-7
    assert np.allclose([stats['positives_per_query'], stats['ap'], stats['avg_embedding_norm']], g['b64.stats'][[0, 3, 4]],
                       atol=2e-6)
    assert np.allclose([stats['best_positive_ranking'], stats['recall'][1]], g['b64.stats'][[1, 2]], atol=1e-6)


def test_multistaged_step_with_the_euclidean_loss_matches_direct_autograd():
    """Two minibatches of two clouds through the HIP encoder, the loss of `make_losses(similarity='euclidean')`, stage-3
    back-propagation, against direct autograd through both minibatches on the GPU (the set-up and bars of
    tests/test_gpu_loss.py::test_multistaged_step_on_the_encoder_matches_oracle_chain, leg (a))."""
    from hotformerloc_amd import build_batch_octree, load_config, model_factory
    from hotformerloc_amd import synthetic as syn
    from hotformerloc_amd.training import multistaged_training_step
    params, depth = load_config('wild-places')
    params.drop_path = 0.0
    clouds = [syn.cylindrical(syn.unit_ball_cloud(3100 + i, 700 + 100 * i)) for i in range(4)]
    parts = [clouds[:2], clouds[2:]]
    lab = torch.arange(4) // 2
    pos = (lab[:, None] == lab[None, :]) & ~torch.eye(4, dtype=torch.bool)
    neg = lab[:, None] != lab[None, :]
    loss_fn = make_losses(SimpleNamespace(loss='truncatedsmoothap', tau1=0.01, similarity='euclidean', positives_per_query=1))
    assert loss_fn.similarity == 'euclidean'

    def fresh():
        m = model_factory(params)
        syn.fill_synthetic_weights(m, 'stress')
        return m.cuda()

    model = fresh()
    mbs = [{'octree': build_batch_octree(p, depth, 2, 'cuda')} for p in parts]
    stats = multistaged_training_step(model, mbs, pos, neg, loss_fn)
    direct = fresh().train()
    emb = torch.cat([direct({'octree': build_batch_octree(p, depth, 2, 'cuda')})['global'] for p in parts], 0)
    loss, _ = loss_fn(emb, pos, neg)
    loss.backward()
    print('multistaged euclidean step: loss', stats['loss'], loss.item())
    assert abs(stats['loss'] - loss.item()) < 1e-5
    assert any(p.grad is not None and p.grad.abs().max().item() > 0 for p in model.parameters())
    for (n, p), q in zip(model.named_parameters(), direct.parameters()):
        d = (p.grad - q.grad).norm().item()
        assert d <= 2e-4 * max(q.grad.norm().item(), 1e-9) + 1e-9, (n, d, q.grad.norm().item())
