"""GPU batch-hard triplet and contrastive losses (`hfl_batch_hard_mine`, `hfl_batch_hard_terms`, `hfl_batch_hard_grad`):
the mining against the first extrema of `ops.pairwise_dist`, bit for bit; both classes against the float64 restatement of
tests/batch_hard_cases.py at the bars tests/test_gpu_loss_euclid.py uses for the same arithmetic; the gradient against the
fp32 numpy twin, which follows the kernels operation for operation, so the comparison is for EQUALITY; and one multi-staged
training step with each class."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import batch_hard_cases as bc
from hotformerloc_amd import losses, ops

pytestmark = pytest.mark.gpu

ALL_CASES = sorted(bc.CASES) + sorted(bc.EMPTY_CASES)
_TWINS = {}


def _twin32(case, kind):
    """the fp32 numpy twin on a case, computed once: (loss, grad, stats, details)"""
    if (case, kind) not in _TWINS:
        e, pos, neg = bc.inputs(case)
        m, pm, nm = bc.margins(case)
        if kind == 'triplet':
            _TWINS[(case, kind)] = losses.batch_hard_triplet_host(e, pos, neg, m, details=True)
        else:
            _TWINS[(case, kind)] = losses.batch_hard_contrastive_host(e, pos, neg, pm, nm, details=True)
    return _TWINS[(case, kind)]


def _device_inputs(case):
    e, pos, neg = bc.inputs(case)
    return torch.from_numpy(e.copy()).cuda(), torch.from_numpy(pos.copy()).cuda(), torch.from_numpy(neg.copy()).cuda()


@pytest.mark.parametrize('case', ALL_CASES)
def test_mining_equals_the_first_extrema_of_pairwise_dist(case):
    """Indices equal numpy's first arg-max / arg-min over `ops.pairwise_dist(emb)` with the masks applied, on every row; the
    distances, and d_pn through the terms kernel, are that matrix's entries bit for bit."""
    emb, pos, neg = _device_inputs(case)
    e, pos_h, neg_h = bc.inputs(case)
    b = e.shape[0]
    dm = ops.pairwise_dist(emb).cpu().numpy()
    p, d_ap, n, d_an = ops.batch_hard_mine(emb, pos.view(torch.uint8), neg.view(torch.uint8))
    stats, scale, d_pn, flags = ops.batch_hard_terms(emb, p, d_ap, n, d_an, ops.BATCH_HARD_TRIPLET, bc.margins(case)[0])
    p, d_ap, n, d_an, d_pn, flags = (t.cpu().numpy() for t in (p, d_ap, n, d_an, d_pn, flags))
    rows = np.arange(b)
    want_p = np.where(pos_h.any(1), np.argmax(np.where(pos_h, dm, -1), axis=1), -1)
    want_n = np.where(neg_h.any(1), np.argmin(np.where(neg_h, dm, np.inf), axis=1), -1)
    assert p.dtype == np.int32 and np.array_equal(p, want_p) and np.array_equal(n, want_n)
    assert np.array_equal(d_ap, np.where(want_p >= 0, dm[rows, want_p], 0).astype(np.float32))
    assert np.array_equal(d_an, np.where(want_n >= 0, dm[rows, want_n], 0).astype(np.float32))
    kept = (want_p >= 0) & (want_n >= 0)
    assert np.array_equal(flags & 1, kept.astype(np.int32))
    assert np.array_equal(d_pn, np.where(kept, dm[want_p, want_n], 0).astype(np.float32))
    assert stats[0].item() == kept.sum()
    # the public miner: the kept rows, compacted
    a, pa, na, dap, dan = losses.batch_hard_mine(emb, pos, neg)
    assert a.dtype == pa.dtype == na.dtype == torch.int64
    assert np.array_equal(a.cpu().numpy(), rows[kept]) and np.array_equal(pa.cpu().numpy(), want_p[kept])
    assert np.array_equal(na.cpu().numpy(), want_n[kept])
    assert np.array_equal(dap.cpu().numpy(), d_ap[kept]) and np.array_equal(dan.cpu().numpy(), d_an[kept])
    if case == 'dup24':
        assert n[12] == 0 and p[18] == 19 and d_ap[18] == 0.0 and d_an[7] == 0.0


def _loss_fn(case, kind):
    m, pm, nm = bc.margins(case)
    if kind == 'triplet':
        return losses.BatchHardTripletLossWithMasks(m)
    return losses.BatchHardContrastiveLossWithMasks(pm, nm)


def _check_stats(kind, got, want, tol):
    floats, counts = bc.stat_keys(kind)
    assert sorted(got) == sorted(floats + counts)
    for key in counts:
        assert got[key] == want[key], (key, got[key], want[key])
    for key in floats:
        assert (math.isnan(got[key]) and math.isnan(want[key])) or abs(got[key] - want[key]) <= tol, (key, got[key], want[key])


@pytest.mark.parametrize('kind', ['triplet', 'contrastive'])
@pytest.mark.parametrize('case', ALL_CASES)
def test_loss_classes_match_float64_and_the_fp32_twin(case, kind):
    """Against the float64 yardstick: loss and float stats within 2e-6, counts equal, gradient within 2e-5 max|g_ref| + 1e-7.
    Against the fp32 twin: the gradient is EQUAL (the chains are identical: the distances' fmaf chain, correctly rounded
    sqrt and division, one fmaf per addend in ascending anchor order).  Two runs give the same bits, and an upstream
    gradient of 3 gives three times the gradient."""
    emb_h, pos, neg = _device_inputs(case)
    fn = _loss_fn(case, kind)
    want_loss, want_grad, want_stats, _ = bc.yardstick(case, kind)
    runs = []
    for factor in (1.0, 1.0, 3.0):
        emb = emb_h.clone().requires_grad_()
        loss, stats = fn(emb, pos, neg)
        assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
        (loss if factor == 1.0 else factor * loss).backward()
        runs.append((loss.item(), emb.grad.cpu().numpy(), stats))
    loss, grad, stats = runs[0]
    err = np.abs(grad - want_grad).max()
    print(case, kind, 'loss', loss, 'diff', abs(loss - want_loss), 'grad err', err, 'of', np.abs(want_grad).max(), stats)
    assert abs(loss - want_loss) <= 2e-6
    _check_stats(kind, stats, want_stats, 2e-6)
    assert err <= 2e-5 * np.abs(want_grad).max() + 1e-7
    twin_loss, twin_grad, twin_stats, _ = _twin32(case, kind)
    assert np.array_equal(grad, twin_grad)
    assert abs(twin_loss - stats['loss']) <= 1e-12
    _check_stats(kind, stats, twin_stats, 1e-12)
    assert runs[1][0] == loss and np.array_equal(runs[1][1], grad)
    _check_stats(kind, runs[1][2], stats, 0.0)
    assert np.array_equal(runs[2][1], grad * np.float32(3.0))
    if case in bc.EMPTY_CASES:
        assert loss == 0.0 and not grad.any() and math.isnan(stats['max_pos_pair_dist'])


def test_operands_are_checked_not_converted():
    emb, pos, neg = _device_inputs('b8_g2')
    pos8, neg8 = pos.view(torch.uint8), neg.view(torch.uint8)
    with pytest.raises(TypeError):
        ops.batch_hard_mine(emb, pos, neg8)                                # bool mask
    with pytest.raises(TypeError):
        ops.batch_hard_mine(emb.double(), pos8, neg8)
    with pytest.raises(ValueError):
        ops.batch_hard_mine(emb, pos8[:, :4], neg8)
    with pytest.raises(ValueError):
        ops.batch_hard_mine(emb, pos8.t(), neg8)                           # not contiguous
    p, d_ap, n, d_an = ops.batch_hard_mine(emb, pos8, neg8)
    with pytest.raises(TypeError):
        ops.batch_hard_terms(emb, p.long(), d_ap, n, d_an, ops.BATCH_HARD_TRIPLET, 0.4)
    with pytest.raises(ValueError):
        ops.batch_hard_terms(emb, p, d_ap, n, d_an, 2, 0.4)
    with pytest.raises(ValueError):
        ops.batch_hard_terms(emb, p[:4], d_ap, n, d_an, ops.BATCH_HARD_TRIPLET, 0.4)


def test_both_classes_pass_through_the_multistaged_step():
    """`make_loss_fn` builds each class from a config's names, and an instance drops into `multistaged_training_step`: two
    minibatches of two clouds through the HIP encoder (the set-up of tests/test_gpu_loss_euclid.py), finite parameter
    gradients, the statistics of the reference.  The margins are large so that every term is active."""
    from hotformerloc_amd import build_batch_octree, load_config, model_factory
    from hotformerloc_amd import synthetic as syn
    from hotformerloc_amd.training import multistaged_training_step, should_expand_batch
    params, depth = load_config('wild-places')
    params.drop_path = 0.0
    clouds = [syn.cylindrical(syn.unit_ball_cloud(3100 + i, 700 + 100 * i)) for i in range(4)]
    parts = [clouds[:2], clouds[2:]]
    lab = torch.arange(4) // 2
    pos = (lab[:, None] == lab[None, :]) & ~torch.eye(4, dtype=torch.bool)
    neg = lab[:, None] != lab[None, :]
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'stress')
    model = model.cuda()
    mbs = [{'octree': build_batch_octree(p, depth, 2, 'cuda')} for p in parts]
    for cfg in (SimpleNamespace(loss='batchhardtripletmarginloss', margin=1e3),
                SimpleNamespace(loss='batchhardcontrastiveloss', pos_margin=-1e3, neg_margin=1e3)):
        loss_fn = losses.make_loss_fn(cfg)
        model.zero_grad(set_to_none=True)
        stats = multistaged_training_step(model, mbs, pos, neg, loss_fn)
        print(cfg.loss, stats)
        assert math.isfinite(stats['loss']) and stats['loss'] > 0
        grads = [p.grad for p in model.parameters() if p.grad is not None]
        assert grads and all(torch.isfinite(g).all().item() for g in grads)
        assert any(g.abs().max().item() > 0 for g in grads)
        if cfg.loss == 'batchhardtripletmarginloss':
            assert stats['num_triplets'] == 4 and stats['num_non_zero_triplets'] == 4
            assert not should_expand_batch(stats, 0.5)
        else:
            assert stats['num_pairs'] == 8 and stats['pos_pairs_above_threshold'] == 4 and stats['neg_pairs_above_threshold'] == 4
