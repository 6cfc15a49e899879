"""Host side of the Euclidean TruncatedSmoothAP: the float64 restatement of `tests/loss_cases.py` against the golden
values of the reference's own class (`tools/gen_golden_loss_euclid.py`), the loss factory `make_losses`, and the loss
settings the reference resolves for its four shipped training configs."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import loss_cases as lc
from hotformerloc_amd import losses


@pytest.mark.parametrize('case', sorted(lc.CASES))
def test_restatement_matches_reference_golden(golden_dir, case):
    """The bars of tests/test_oracle_loss.py: loss 1e-6, gradient 1e-6 max(1, |g|max), stats 1e-6."""
    g = lc.load_golden(golden_dir)
    cfg = tuple(int(v) for v in g[case + '.cfg'])
    assert cfg == lc.CASES[case]
    _, _, _, loss, grad, stats = lc.yardstick(*cfg)
    gref = g[case + '.grad']
    print(case, 'loss diff', abs(loss - float(g[case + '.loss'])), 'grad diff', np.abs(grad - gref).max(), 'of', np.abs(gref).max())
    assert abs(loss - float(g[case + '.loss'])) < 1e-6
    assert np.abs(grad - gref).max() <= 1e-6 * max(1.0, np.abs(gref).max())
    assert np.allclose(lc.stats_vector(stats), g[case + '.stats'], atol=1e-6)


def test_golden_records_the_reference_fp32_gap(golden_dir):
    g = lc.load_golden(golden_dir)
    for case in lc.CASES:
        assert 0.0 <= float(g[case + '.ref32_loss_gap']) < 1e-5 and 0.0 < float(g[case + '.ref32_grad_gap']) < 1e-3


def test_large_batch_yardstick_is_the_restatement():
    """The memory-lean form used at B = 2048 is the same function (float64: equal up to summation order)."""
    e, pos, neg = lc.make_case(31, 70, 24, 5, 3)
    pos, neg = torch.from_numpy(pos), torch.from_numpy(neg)
    a = torch.from_numpy(e).double().requires_grad_()
    b = torch.from_numpy(e).double().requires_grad_()
    la, sa = lc.truncated_smooth_ap_euclid(a, pos, neg, lc.TAU1, 4)
    lb, sb = lc._big_yardstick(b, pos, neg, 4)
    la.backward()
    lb.backward()
    assert abs(la.item() - lb.item()) < 1e-12
    assert (a.grad - b.grad).abs().max().item() < 1e-10 * a.grad.abs().max().item()
    assert np.allclose(lc.stats_vector(sa), lc.stats_vector(sb), atol=1e-12)


def test_restatement_gives_coincident_rows_no_gradient_from_each_other():
    e = torch.tensor([[1., 0.], [1., 0.], [0., 2.]], dtype=torch.float64, requires_grad=True)
    d = lc.direct_dist(e)
    assert d[0, 1].item() == 0.0 and d.diagonal().abs().max().item() == 0.0
    d.sum().backward()
    assert torch.isfinite(e.grad).all()
    want = torch.tensor([[1., -2.], [1., -2.], [-2., 4.]], dtype=torch.float64) * (2.0 / 5.0 ** 0.5)
    assert torch.allclose(e.grad, want, atol=1e-12)


@pytest.mark.parametrize('similarity', ['euclidean', 'cosine'])
def test_make_losses_builds_truncated_smoothap(similarity):
    fn = losses.make_losses(SimpleNamespace(loss='truncatedsmoothap', tau1=0.02, similarity=similarity, positives_per_query=3))
    assert isinstance(fn, losses.TruncatedSmoothAP)
    assert (fn.tau1, fn.similarity, fn.positives_per_query) == (0.02, similarity, 3)


@pytest.mark.parametrize('name', ['batchhardtripletmarginloss', 'batchhardcontrastiveloss'])
def test_make_losses_names_the_losses_it_does_not_build(name):
    with pytest.raises(NotImplementedError, match=name):
        losses.make_losses(SimpleNamespace(loss=name, margin=0.4, pos_margin=0.2, neg_margin=0.65, similarity='euclidean'))


def test_make_losses_rejects_unknown_names():
    with pytest.raises(NotImplementedError, match='Unknown loss: focal'):
        losses.make_losses(SimpleNamespace(loss='focal', tau1=0.01, similarity='euclidean', positives_per_query=4))


def test_unknown_similarity_is_rejected_in_the_reference_wording():
    with pytest.raises(NotImplementedError, match='Incorrect similarity measure: manhattan'):
        losses.TruncatedSmoothAP(similarity='manhattan')
    with pytest.raises(NotImplementedError, match='Incorrect similarity measure: manhattan'):
        losses.make_losses(SimpleNamespace(loss='truncatedsmoothap', tau1=0.01, similarity='manhattan', positives_per_query=4))
    assert losses.TruncatedSmoothAP().similarity == 'cosine'                 # the constructor default stays the reference's


def test_every_shipped_config_trains_with_the_euclidean_loss(golden_dir):
    with open(os.path.join(golden_dir, lc.SETTINGS_NAME)) as f:
        settings = json.load(f)
    assert sorted(settings) == ['cs-campus3d', 'cs-wild-places', 'oxford', 'wild-places']
    for name, s in settings.items():
        assert s['similarity'] == 'euclidean', name
        fn = losses.make_losses(SimpleNamespace(**s))
        assert (fn.tau1, fn.similarity, fn.positives_per_query) == (s['tau1'], 'euclidean', s['positives_per_query']), name


def test_euclidean_loss_has_no_cpu_fallback():
    from hotformerloc_amd._native import NativeLibraryError
    with pytest.raises(NativeLibraryError):
        losses.TruncatedSmoothAP(similarity='euclidean')(torch.zeros(4, 8), torch.zeros(4, 4, dtype=torch.bool),
                                                         torch.zeros(4, 4, dtype=torch.bool))
    with pytest.raises(NativeLibraryError):
        losses.euclidean_affinity(torch.zeros(4, 8))
