"""MESA self-distillation on the GPU: the distillation loss (`hfl_kd_rows`) against the reference's golden values, the
one-launch weight average (`hfl_ema_update`), the teacher's weight packs after an update, and the multi-staged step with a
teacher."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hotformerloc_amd import build_batch_octree, load_config, model_factory     # noqa: E402
from hotformerloc_amd import model as hmodel                                      # noqa: E402
from hotformerloc_amd import ops                                                  # noqa: E402
from hotformerloc_amd import synthetic as syn                                     # noqa: E402
from hotformerloc_amd.ema import ModelEma                                         # noqa: E402
from hotformerloc_amd.losses import TruncatedSmoothAP, kdloss                    # noqa: E402
from hotformerloc_amd.training import multistaged_training_step                   # noqa: E402
from oracle.gen_golden_loss import make_case                                      # noqa: E402

pytestmark = pytest.mark.gpu

KD_CASES = ['b8', 'b64', 'b257', 'b48_d128', 'b64_x20']
BAR_FACTOR = 4.0          # times the reference's largest fp32 error over 8 seeds of the shape (tests/golden/mesa.npz)


def _kd_gpu(y, t, **kw):
    ys = torch.from_numpy(y).cuda().requires_grad_()
    loss = kdloss(ys, torch.from_numpy(t).cuda(), **kw)
    loss.backward()
    return loss.detach(), ys.grad


def _kd_torch64(y, t, T=3.0):
    """the reference's formula (`models/losses/loss.py:138-147`) on float64 device tensors"""
    p = torch.log_softmax(y.double() / T, dim=1)
    q = torch.softmax(t.double() / T, dim=1)
    return 50.0 * torch.nn.functional.kl_div(p, q, reduction='batchmean')


# ------------------------------------------------------------------------------------------- 1. kdloss
@pytest.mark.parametrize('case', KD_CASES)
def test_kdloss_matches_reference_golden(golden_dir, case):
    """Loss and gradient against the reference's float64 values; bar = 4 x the largest error of the reference's own fp32
    run over 8 seeds of the shape (the kernel sums in another order than torch: a small multiple of the rounding error of
    a cancelling sum, nothing more).  Measured on MI355X, error / bar: loss 0.000 - 0.005, gradient 0.002 - 0.038 over the
    five cases (DESIGN.md section 6b "MESA"): 26x of headroom at the worst.

    Negative controls.  T = 1 misses both bars by far more than 100x in every case.  Student and teacher SWAPPED misses
    the gradient bar by more than 100x in every case (the gradient changes sign), but the LOSS bar only where the rows
    differ grossly (`b64_x20`): KL(q || p) and KL(p || q) agree to second order in the difference of nearly equal rows,
    and in float64 the swapped loss of the four unit-norm cases lies 2e-4 of the loss away, 0.02 to 0.07 of the bar.  No
    implementation can fail that, so the swapped loss is asserted for `b64_x20` alone."""
    g = np.load(os.path.join(golden_dir, 'mesa.npz'))
    seed, batch, dim, scale = g[case + '.cfg']
    y, t = syn.kd_case(int(seed), int(batch), int(dim), float(scale))
    want_l, want_g = float(g[case + '.loss64']), g[case + '.grad64']
    bar_l, bar_g = BAR_FACTOR * g[case + '.ref32_max']

    def errors(loss, grad):
        return (abs(loss.item() - want_l) / abs(want_l),
                np.linalg.norm(grad.cpu().numpy().astype(np.float64) - want_g) / np.linalg.norm(want_g))

    loss, grad = _kd_gpu(y, t)
    el, eg = errors(loss, grad)
    print('kdloss %s: loss %.9g (fp64 %.9g) rel err %.3g = %.3f of the bar %.3g; grad rel-L2 %.3g = %.3f of the bar %.3g'
          % (case, loss.item(), want_l, el, el / bar_l, bar_l, eg, eg / bar_g, bar_g))
    assert el <= bar_l and eg <= bar_g
    again_l, again_g = _kd_gpu(y, t)
    assert torch.equal(loss, again_l) and torch.equal(grad, again_g), 'two calls on the same input must agree bit for bit'
    # negative controls
    e1l, e1g = errors(*_kd_gpu(y, t, T=1.0))
    esl, esg = errors(*_kd_gpu(t, y))
    print('  controls: T=1 misses by %.3g x (loss) %.3g x (grad); swapped by %.3g x (loss) %.3g x (grad)'
          % (e1l / bar_l, e1g / bar_g, esl / bar_l, esg / bar_g))
    assert e1l >= 100 * bar_l and e1g >= 100 * bar_g
    assert esg >= 100 * bar_g
    if case == 'b64_x20':
        assert esl >= 100 * bar_l


def test_kdloss_rejects_unsupported_shapes():
    from hotformerloc_amd._native import NativeLibraryError
    for d in (32, 100, 1088):
        with pytest.raises(NativeLibraryError):
            kdloss(torch.zeros(4, d, device='cuda'), torch.zeros(4, d, device='cuda'))
    with pytest.raises(ValueError):
        kdloss(torch.zeros(4, 64, device='cuda'), torch.zeros(5, 64, device='cuda'))
    # D = 1024 (16 elements per lane) and identical rows: zero loss, zero gradient
    y = torch.randn(3, 1024, device='cuda', requires_grad=True)
    loss = kdloss(y, y.detach().clone())
    loss.backward()
    assert abs(loss.item()) < 1e-6 and y.grad.abs().max().item() < 1e-7


def test_stage2_listwise_plus_kd_matches_reference_golden(golden_dir):
    """TruncatedSmoothAP + 1.0 * kdloss on the GPU against the reference's stage-2 sum, at the bars
    `test_gpu_loss.py::test_loss_matches_reference_golden` holds for the listwise loss alone; the listwise loss alone (a
    step that drops the distillation term) must fail both."""
    from tools.gen_golden_mesa import stage2_teacher
    g = np.load(os.path.join(golden_dir, 'mesa.npz'))
    e, pos, neg = make_case(11, 64, 256, 4, 0)
    teacher = torch.from_numpy(stage2_teacher(e)).cuda()
    loss_fn = TruncatedSmoothAP(tau1=0.01, positives_per_query=4)
    gref = g['stage2.grad']
    bar_l, bar_g = 2e-6, 2e-5 * max(np.abs(gref).max(), 1e-6) + 1e-7

    emb = torch.from_numpy(e).cuda().requires_grad_()
    listwise, _ = loss_fn(emb, torch.from_numpy(pos), torch.from_numpy(neg))
    loss = listwise + 1.0 * kdloss(emb, teacher)
    loss.backward()
    el, eg = abs(loss.item() - float(g['stage2.loss'])), np.abs(emb.grad.cpu().numpy() - gref).max()
    print('stage 2: loss %.9g (reference %.9g) err %.3g, bar %.3g; grad max err %.3g, bar %.3g'
          % (loss.item(), float(g['stage2.loss']), el, bar_l, eg, bar_g))
    assert el < bar_l and eg <= bar_g
    # control: without the distillation term
    emb = torch.from_numpy(e).cuda().requires_grad_()
    listwise, _ = loss_fn(emb, torch.from_numpy(pos), torch.from_numpy(neg))
    listwise.backward()
    cl, cg = abs(listwise.item() - float(g['stage2.loss'])), np.abs(emb.grad.cpu().numpy() - gref).max()
    print('  control (listwise alone): loss err %.3g = %.0f x bar, grad err %.3g = %.1f x bar' % (cl, cl / bar_l, cg, cg / bar_g))
    assert cl > bar_l and cg > bar_g


# ------------------------------------------------------------------------------------------- 2. hfl_ema_update
def _ema_check(ema, src, w, steps_bound=1):
    """run the launch on clones of `ema`; per element at most steps_bound * 2^-23 * max(|ema|, |src|) from the float64 formula:
    one rounding of the difference, one of the fused multiply-add (w <= 1/2), each at most half an ulp of a quantity no
    larger than the operands"""
    want = [e.double() + w * (s.double() - e.double()) for e, s in zip(ema, src)]
    old = [e.double().abs() for e in ema]
    before = [s.clone() for s in src]
    table, n = ops.ema_table(ema, src)
    ops.ema_update(table, n, w)
    torch.cuda.synchronize()
    worst = 0.0
    for e, s, b, x, o in zip(ema, src, before, want, old):
        assert torch.equal(s, b), 'the source must not be written'
        bound = steps_bound * 2.0 ** -23 * torch.maximum(o, s.double().abs())
        ratio = ((e.double() - x).abs() / bound.clamp_min(1e-300)).max().item() if e.numel() else 0.0
        worst = max(worst, ratio)
    return worst


def _shipped_model():
    params, depth = load_config('cs-wild-places')
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'stress')
    return model.cuda(), params, depth


def _perturb(model, rel, seed):
    gen = torch.Generator(device='cuda').manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(rel * p.abs().mean().clamp_min(1e-3) * torch.randn(p.shape, device=p.device, generator=gen))


def test_ema_update_on_the_shipped_model():
    model, _, _ = _shipped_model()
    ema = ModelEma(model, decay=0.9998)
    _perturb(model, 0.1, 1)
    e = [v for v in ema.module.state_dict().values()]
    s = [v for v in model.state_dict().values()]
    assert len(e) == 726 and all(v.dtype == torch.float32 for v in e)
    want = [a.double() + (1.0 - 0.9998) * (b.double() - a.double()) for a, b in zip(e, s)]
    old = [a.double().abs() for a in e]
    versions = [p._version for p in ema.module.parameters()]
    ema.update(model)
    torch.cuda.synchronize()
    worst = 0.0
    for a, b, x, o in zip(e, s, want, old):
        bound = 2.0 ** -23 * torch.maximum(o, b.double().abs()).clamp_min(1e-300)
        worst = max(worst, ((a.double() - x).abs() / bound).max().item())
    print('ema update, 726 tensors: worst error / bound', worst)
    assert worst <= 1.0
    assert all(p._version > v for p, v in zip(ema.module.parameters(), versions)), 'cached weight packs key on _version'
    table = ema._launch[1]
    assert int(table[:, 2].sum()) == 35371176 and int(table[:, 2].max()) <= ops.EMA_CHUNK
    # 20 consecutive updates with fresh perturbations: 20 x the single-step bound
    ref = [a.double().clone() for a in e]
    for step in range(20):
        _perturb(model, 0.05, 100 + step)
        ref = [r + (1.0 - 0.9998) * (b.double() - r) for r, b in zip(ref, s)]
        ema.update(model)
    torch.cuda.synchronize()
    worst = 0.0
    for a, b, r in zip(e, s, ref):
        bound = 20 * 2.0 ** -23 * torch.maximum(r.abs(), b.double().abs()).clamp_min(1e-300)
        worst = max(worst, ((a.double() - r).abs() / bound).max().item())
    print('20 ema updates: worst error / (20 x bound)', worst)
    assert worst <= 1.0
    assert ema._launch[1] is table, 'the pointer table is rebuilt only when a data_ptr changes'


@pytest.mark.parametrize('w', [0.5, 1.0 - 0.9998])
def test_ema_update_tails_and_unaligned_views(w):
    gen = torch.Generator(device='cuda').manual_seed(5)
    ema, src, guards = [], [], []
    for n in (1, 3, 5, 63, 1025, 4 * ops.EMA_CHUNK + 7):
        for off_e, off_s in ((0, 0), (1, 0), (0, 3), (2, 2)):          # element offsets: 4-byte aligned, mostly not 16-byte
            be = torch.randn(n + 8, device='cuda', generator=gen)
            bs = torch.randn(n + 8, device='cuda', generator=gen)
            ema.append(be[off_e:off_e + n])
            src.append(bs[off_s:off_s + n])
            guards.append((be, be.clone(), off_e, n))
    assert any(t.data_ptr() % 16 for t in ema) and any(t.data_ptr() % 16 for t in src)
    worst = _ema_check(ema, src, w)
    print('tails / unaligned views, w = %g: worst error / bound' % w, worst)
    assert worst <= 1.0
    for buf, old, off, n in guards:                                     # nothing outside a view is touched
        assert torch.equal(buf[:off], old[:off]) and torch.equal(buf[off + n:], old[off + n:])


def test_ema_copies_what_it_cannot_average():
    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(5, 3)
            self.register_buffer('steps', torch.tensor([7, 11], dtype=torch.int64))

    toy = Toy().cuda()
    ema = ModelEma(toy, decay=0.75)
    with torch.no_grad():
        toy.steps += 100
        toy.lin.weight += 1.0
    old = ema.module.lin.weight.clone()
    ema.update(toy)
    assert torch.equal(ema.module.steps, toy.steps) and ema.module.steps.dtype == torch.int64
    assert torch.allclose(ema.module.lin.weight, old + 0.25 * (toy.lin.weight - old), rtol=0, atol=1e-6)
    # after model.to(...)-style reallocation the table follows the new pointers
    with torch.no_grad():
        toy.lin.weight.data = toy.lin.weight.data.clone() + 1.0
    old = ema.module.lin.weight.clone()
    ema.update(toy)
    assert torch.allclose(ema.module.lin.weight, old + 0.25 * (toy.lin.weight - old), rtol=0, atol=1e-6)


# ------------------------------------------------------------------------------------------- 3. stale weight packs
@pytest.mark.parametrize('mode', ['x3', 'x6'])
def test_teacher_encodes_with_its_updated_weights(mode):
    """Every hand-written GEMM caches a packed copy of its weight per parameter version.  After `update` the teacher must
    encode with the NEW weights: its descriptors equal those of a fresh model loaded with its state dict, bit for bit when
    the inference path is repeatable (measured here on two fresh models; on MI355X it is, in both modes).

    The fresh models are frozen (`requires_grad_(False)`) as the teacher is: in mode x6 the attention-pooling head runs
    `torch.matmul(batched rows, parameter)`, and torch picks its folded or its batched GEMM by the parameter's
    `requires_grad` flag, also under `no_grad`.  A frozen and an unfrozen model with equal weights differ there by 3e-7
    rel-L2 (measured), which has nothing to do with weight packs; stale packs show as the 0.47 of `moved`."""
    hmodel.set_gemm_mode(mode)
    model, params, depth = _shipped_model()
    clouds = syn.make_clouds(9, 4, 3000, params.coordinates)

    def encode(m):
        with torch.no_grad():
            return m({'octree': build_batch_octree(clouds, depth, 2, 'cuda')})['global']

    ema = ModelEma(model, decay=0.5)
    before = encode(ema.module)
    _perturb(model, 0.1, 3)
    ema.update(model)
    after = encode(ema.module)

    def fresh():
        m = model_factory(params).cuda().eval().requires_grad_(False)
        m.load_state_dict(ema.module.state_dict())
        return m

    want, want2 = encode(fresh()), encode(fresh())
    moved = ((after - before).norm() / before.norm()).item()
    floor = ((want - want2).norm() / want.norm()).item()
    err = ((after - want).norm() / want.norm()).item()
    print('stale packs (%s): teacher moved %.3g rel-L2; fresh vs fresh %.3g; teacher vs fresh %.3g' % (mode, moved, floor, err))
    assert moved > 1e-3, 'the update must change the descriptors, or this test proves nothing'
    if floor == 0.0:
        assert torch.equal(after, want)
    else:
        assert err <= 2 * floor


# ------------------------------------------------------------------------------------------- 4. the step
@pytest.fixture(scope='module')
def rccl_world1():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    assert not dist.is_initialized()
    dist.init_process_group('nccl', world_size=1, rank=0, init_method='tcp://127.0.0.1:%d' % port)
    try:
        yield dist.group.WORLD
    finally:
        dist.destroy_process_group()


class _StepSetup:
    def __init__(self):
        self.params, self.depth = load_config('wild-places')
        self.params.drop_path = 0.0
        clouds = [syn.cylindrical(syn.unit_ball_cloud(3100 + i, 700 + 100 * i)) for i in range(4)]
        self.parts = [clouds[:2], clouds[2:]]
        lab = torch.arange(4) // 2
        self.pos = (lab[:, None] == lab[None, :]) & ~torch.eye(4, dtype=torch.bool)
        self.neg = lab[:, None] != lab[None, :]
        self.loss_fn = TruncatedSmoothAP(tau1=0.01, positives_per_query=1)

    def student(self):
        m = model_factory(self.params)
        syn.fill_synthetic_weights(m, 'stress')
        return m.cuda()

    def teacher(self, decay=0.9998):
        """an average that has drifted from the student: same weights plus 5 % noise"""
        m = self.student()
        _perturb(m, 0.05, 17)
        return ModelEma(m, decay=decay)

    def batches(self):
        return [{'octree': build_batch_octree(p, self.depth, 2, 'cuda')} for p in self.parts]


def _grads(model):
    return {k: (None if p.grad is None else p.grad.clone()) for k, p in model.named_parameters()}


def _assert_same_grads(a, b, exact):
    for k in a:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is None:
            continue
        if exact and not k.endswith('rpe_table'):
            assert torch.equal(a[k], b[k]), (k, (a[k] - b[k]).abs().max().item())
        elif exact:
            # the table gradient is flushed with float atomics (one per workgroup): run-to-run order noise of the step as
            # it was before this feature (tests/test_gpu_configs.py::test_rccl_multistaged_step_equals_no_group_step)
            assert torch.allclose(a[k], b[k], rtol=1e-4, atol=1e-6 * max(a[k].abs().max().item(), 1e-30)), k
        else:
            d = (a[k] - b[k]).norm().item()
            assert d <= 2e-4 * max(b[k].norm().item(), 1e-9) + 1e-9, (k, d, b[k].norm().item())


def _chain(su, ema, mesa):
    """the step composed by hand from the existing pieces, the distillation term as the reference's torch formula in float64"""
    model = su.student().train()
    mbs = su.batches()
    with torch.no_grad():
        with hmodel.training_numerics():
            emb = torch.cat([model(mb)['global'] for mb in mbs], 0)
        emb_ema = torch.cat([ema.module(mb)['global'] for mb in mbs], 0)
    emb = emb.detach().requires_grad_()
    listwise, _ = su.loss_fn(emb, su.pos, su.neg)
    kd = _kd_torch64(emb, emb_ema)
    (listwise.double() + mesa * kd).backward()
    i = 0
    for mb in mbs:
        y = model(mb)['global']
        y.backward(gradient=emb.grad[i:i + y.shape[0]])
        i += y.shape[0]
    return model, listwise.item(), kd.item(), emb.grad


@pytest.mark.parametrize('mesa', [1.0, 1000.0])
def test_step_with_distillation_matches_hand_composed_chain(mesa, rccl_world1):
    """(a) loss and parameter gradients of the step with a teacher against the chain composed by hand; mesa = 1 checks the
    plumbing and the ordering (the distillation part of the gradient is ~1e-3 of the listwise part), mesa = 1000 the term
    itself.  Bar: 2e-4 rel-L2 per parameter, the one `test_gpu_loss.py::test_multistaged_step_on_the_encoder_matches_oracle_chain`
    holds between two GPU chains (tighter than 2e-3).  (c) the same numbers with the collectives forced at world size 1."""
    su = _StepSetup()
    ema = su.teacher()
    ema_w0 = {k: v.clone() for k, v in ema.state_dict().items()}
    want_model, want_listwise, want_kd, emb_grad = _chain(su, ema, mesa)
    want = _grads(want_model)

    model = su.student()
    stats = multistaged_training_step(model, su.batches(), su.pos, su.neg, su.loss_fn, model_ema=ema, mesa=mesa)
    torch.cuda.synchronize()
    got = _grads(model)
    print('step mesa=%g: listwise %.9g (chain %.9g), kd %.9g (chain fp64 %.9g)' % (mesa, stats['loss'], want_listwise,
                                                                                 stats['mesa_kd'], want_kd))
    assert abs(stats['loss'] - want_listwise) < 1e-5, 'stats["loss"] is the listwise loss alone, as in the reference'
    assert want_kd > 1e-4 and abs(stats['mesa_kd'] - want_kd) <= 4 * 1.6e-3 * want_kd      # b8's ref32_max x 4
    _assert_same_grads(got, want, exact=False)
    # the teacher received its update after the backward: ema + w * (model - ema), the student's weights unchanged (no optimizer)
    msd = model.state_dict()
    for k, v in ema.state_dict().items():
        x = ema_w0[k].double() + (1.0 - 0.9998) * (msd[k[len('module.'):]].double() - ema_w0[k].double())
        src = msd[k[len('module.'):]].double().abs()
        assert ((v.double() - x).abs() <= 2.0 ** -23 * torch.maximum(ema_w0[k].double().abs(), src) + 1e-300).all(), k
    # (c) forced collectives, a teacher with the same (pre-update) weights
    ema_c = su.teacher()
    model_c = su.student()
    stats_c = multistaged_training_step(model_c, su.batches(), su.pos, su.neg, su.loss_fn, model_ema=ema_c, mesa=mesa,
                                        n_total=4, group=rccl_world1, force_collectives=True)
    torch.cuda.synchronize()
    assert stats_c['loss'] == stats['loss'] and stats_c['mesa_kd'] == stats['mesa_kd']
    _assert_same_grads(_grads(model_c), got, exact=True)


def test_step_with_teacher_but_mesa_zero_is_the_plain_step():
    """(b) `model_ema` given, mesa = 0: statistics and gradients of the step without a teacher (bit for bit, except the one
    gradient the backward accumulates with float atomics), the teacher's forward never runs, the average moves."""
    su = _StepSetup()
    plain = su.student()
    stats0 = multistaged_training_step(plain, su.batches(), su.pos, su.neg, su.loss_fn)
    model = su.student()
    ema = su.teacher()
    before = {k: v.clone() for k, v in ema.state_dict().items()}
    calls = []
    hook = ema.module.register_forward_hook(lambda *a: calls.append(1))
    stats = multistaged_training_step(model, su.batches(), su.pos, su.neg, su.loss_fn, model_ema=ema, mesa=0.0)
    hook.remove()
    torch.cuda.synchronize()
    assert stats == stats0 and 'mesa_kd' not in stats
    _assert_same_grads(_grads(model), _grads(plain), exact=True)
    assert not calls
    assert any(not torch.equal(v, before[k]) for k, v in ema.state_dict().items())


def test_validation_phase_leaves_the_teacher_alone():
    """(d)"""
    su = _StepSetup()
    model = su.student()
    ema = su.teacher()
    before = {k: v.clone() for k, v in ema.state_dict().items()}
    calls = []
    hook = ema.module.register_forward_hook(lambda *a: calls.append(1))
    stats = multistaged_training_step(model, su.batches(), su.pos, su.neg, su.loss_fn, phase='val', model_ema=ema, mesa=1.0)
    hook.remove()
    plain = multistaged_training_step(su.student(), su.batches(), su.pos, su.neg, su.loss_fn, phase='val')
    assert stats == plain and not calls
    assert all(torch.equal(v, before[k]) for k, v in ema.state_dict().items())
