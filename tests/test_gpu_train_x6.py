"""GEMM mode x6 under autograd: the matched-precision training path on hand-written kernels.

Kernels: hfl_wgrad_f32 (dW = dy^T x and db on the fp32 matrix cores), the GELU-forward / GELU-backward epilogues of
hfl_linear_x6.  Autograd: LinearFn, MlpFn, LnMlpResidualFn with the X6 family against fp64 autograd next to torch's fp32 autograd.  Model:
no library GEMM in the block Linears, parameter gradients against the CPU oracle next to the fp32 library route
(set_train_x6(False)), the multi-staged step, config 3 at full size.  Reference arithmetic: fp32 torch.nn.Linear under
autograd (training/trainer.py:344-362)."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from hotformerloc_amd import autograd as ag
from hotformerloc_amd import build_batch_octree, load_config, model_factory, ops
from hotformerloc_amd import model as M
from hotformerloc_amd import synthetic as syn
from hotformerloc_amd.model import set_gemm_mode, set_train_x6

DEV = 'cuda'
# (dW rows N, dW columns K) of the block Linears at C = 128 and C = 256: qkv, proj, fc1, fc2
WGRAD_SHAPES = [(384, 128), (128, 128), (512, 128), (128, 512), (768, 256), (256, 256), (1024, 256), (256, 1024)]
GRAD_TOL = 1e-3


def _rel(a, ref) -> float:
    return ((a.double() - ref).norm() / ref.norm().clamp_min(1e-300)).item()


@pytest.mark.parametrize('m', [1, 31, 4097, 300000])
def test_wgrad_f32_against_fp64(m):
    """hfl_wgrad_f32 against fp64 and next to torch's fp32 dy^T x on the GPU: dW rel-L2 <= max(1.5x the library's, 1e-6)
    (the absolute floor: how the library splits a long row contraction is its own business), db within 1e-6, and two calls
    give the same bits (fixed reduction order)."""
    g = torch.Generator(device=DEV).manual_seed(17 + m)
    for n, k in WGRAD_SHAPES:
        dy = torch.randn(m, n, device=DEV, generator=g) * 0.7
        x = torch.randn(m, k, device=DEV, generator=g) * 1.3 + 0.2
        dw, db = ops.wgrad_f32(dy, x, with_bias=True)
        ref = dy.double().t() @ x.double()
        refb = dy.double().sum(0)
        e = _rel(dw, ref)
        e32 = _rel(dy.t() @ x, ref)
        eb = _rel(db, refb)
        print('M %d N %d K %d: wgrad_f32 %.2e  fp32 library %.2e  db %.2e' % (m, n, k, e, e32, eb))
        assert e <= max(1.5 * e32, 1e-6), (m, n, k, e, e32)
        assert eb <= 1e-6, (m, n, k, eb)
        dw2, db2 = ops.wgrad_f32(dy, x, with_bias=True)
        assert torch.equal(dw, dw2) and torch.equal(db, db2), (m, n, k)
        dw3, none = ops.wgrad_f32(dy, x)
        assert none is None and torch.equal(dw, dw3), (m, n, k)


def test_wgrad_f32_rejects_unsupported_shapes():
    from hotformerloc_amd._native import NativeLibraryError
    with pytest.raises(NativeLibraryError):
        ops.wgrad_f32(torch.zeros(8, 96, device=DEV), torch.zeros(8, 128, device=DEV))


def _gelu_grad64(v):
    return 0.5 * (1.0 + torch.erf(v / 2 ** 0.5)) + v * torch.exp(-0.5 * v * v) / (2 * np.pi) ** 0.5


def test_linear_x6_gelu_epilogues():
    """hfl_linear_x6_gelu_fwd: its pre-activation is bitwise linear_x6(x, w3, bias), its output bitwise linear_x6(...,
    gelu=True).  hfl_linear_x6_gelu_bwd: (dy W) * gelu'(pre) within 1e-6 rel-L2 of fp64 (the GELU epilogue's bar in
    test_linear_x6_is_as_accurate_as_the_fp32_library_gemm)."""
    g = torch.Generator(device=DEV).manual_seed(5)
    for m, c, h in ((5000, 128, 512), (3001, 256, 1024), (77, 256, 256)):
        x = torch.randn(m, c, device=DEV, generator=g)
        w1 = torch.randn(h, c, device=DEV, generator=g) * 0.08
        b1 = torch.randn(h, device=DEV, generator=g) * 0.1
        w13 = ops.x6_pack(w1)
        out, pre = ops.linear_x6_gelu_fwd(x, w13, b1)
        assert torch.equal(pre, ops.linear_x6(x, w13, bias=b1)), (m, c, h)
        assert torch.equal(out, ops.linear_x6(x, w13, bias=b1, gelu=True)), (m, c, h)
        # fc2 (c, h): its input gradient times gelu'(pre), W2^T packed
        w2 = torch.randn(c, h, device=DEV, generator=g) * 0.05
        dy = torch.randn(m, c, device=DEV, generator=g)
        got = ops.linear_x6_gelu_bwd(dy, ops.x6_pack(w2.t().contiguous()), pre)
        ref = (dy.double() @ w2.double()) * _gelu_grad64(pre.double())
        e = _rel(got, ref)
        print('gelu_bwd M %d C %d H %d: %.2e' % (m, c, h, e))
        assert e <= 1e-6, (m, c, h, e)


def _grads(fn, tensors, dout):
    ts = [t.detach().clone().requires_grad_(t.requires_grad) for t in tensors]
    y = fn(*ts)
    y.backward(dout)
    return y.detach(), [t.grad for t in ts]


def test_linear_x6_fn_against_fp64_autograd():
    """ag.linear_x6 (LinearFn, X6 family: forward / dx on hfl_linear_x6, dW / db on hfl_wgrad_f32): every gradient's rel-L2 error against fp64
    autograd at most 1.5x torch fp32 autograd's on the same data (with the 1e-6 floor of the wgrad test)."""
    g = torch.Generator(device=DEV).manual_seed(8)
    for m, k, n in ((20000, 256, 768), (4097, 128, 512), (300, 1024, 256)):
        x = (torch.randn(m, k, device=DEV, generator=g) * 1.1).requires_grad_()
        w = (torch.randn(n, k, device=DEV, generator=g) * 0.05).requires_grad_()
        b = (torch.randn(n, device=DEV, generator=g) * 0.1).requires_grad_()
        dout = torch.randn(m, n, device=DEV, generator=g)
        y6, g6 = _grads(ag.linear_x6, (x, w, b), dout)
        y32, g32 = _grads(F.linear, (x, w, b), dout)
        y64, g64 = _grads(F.linear, (x.double(), w.double(), b.double()), dout.double())
        assert _rel(y6, y64) <= max(1.5 * _rel(y32, y64), 1e-6)
        for name, a, l, r in zip(('x', 'W', 'b'), g6, g32, g64):
            e, e32 = _rel(a, r), _rel(l, r)
            print('linear_x6 M %d K %d N %d d%s: %.2e  fp32 autograd %.2e' % (m, k, n, name, e, e32))
            assert e <= max(1.5 * e32, 1e-6), (m, k, n, name, e, e32)
    # the weight images these Functions multiply by live in the one store of model._W3_CACHE: the transposed x6 planes
    # (dx = dy W) and the padded per-tap blocks of the live-tap convolution, both orientations
    _check_image_cache(lambda t: ag._w6_cached(t, True), lambda t: ops.x6_pack(t.detach().t().contiguous()), (256, 128))
    lin = torch.nn.Linear(128, 256).to(DEV)
    assert M._w6(lin) is ag._w6_cached(lin.weight, False)             # one image for inference and training
    for transposed in (True, False):
        def want(t, transposed=transposed):
            blocks = t.detach().transpose(1, 2) if transposed else t.detach()
            pad = blocks.new_zeros(27, 128 - blocks.shape[1], blocks.shape[2])
            return ops.x6_pack(torch.cat([blocks, pad], 1).reshape(27 * 128, -1).contiguous())
        _check_image_cache(lambda t, transposed=transposed: ag._tap_blocks(t, transposed, 128), want, (27, 64, 64))


def _check_image_cache(get, want, shape):
    """cached on the second call; rebuilt, with no new entry, after an in-place update and after `.data` moved to new
    storage (same version, new data_ptr: what module.to(device) does); gone from the store with the parameter"""
    import gc
    before = len(M._W3_CACHE)
    p = torch.nn.Parameter(torch.randn(*shape, device=DEV) * 0.05)
    a = get(p)
    assert torch.equal(a, want(p)) and get(p) is a and len(M._W3_CACHE) == before + 1
    with torch.no_grad():
        p.add_(1.0)
    b = get(p)
    assert b is not a and torch.equal(b, want(p)) and len(M._W3_CACHE) == before + 1
    version = p._version
    p.data = p.data.clone() + 1
    c = get(p)
    assert p._version == version and c is not b and torch.equal(c, want(p)) and len(M._W3_CACHE) == before + 1
    del p, a, b, c
    gc.collect()
    assert len(M._W3_CACHE) == before


def _mlp_branch_ref(x, gamma, beta, w1, b1, w2, b2, s):
    y = F.linear(F.gelu(F.linear(F.layer_norm(x, (x.shape[1],), gamma, beta, 1e-5), w1, b1)), w2, b2)
    return x + (y if s is None else y * s.unsqueeze(1))


@pytest.mark.parametrize('scaled', [False, True])
def test_mlp_x6_functions_against_fp64_autograd(scaled):
    """ag.ln_mlp_residual_x6 (x + s * fc2(gelu(fc1(LN(x)))), s = the stochastic-depth row factor) and ag.mlp_x6 against fp64
    autograd: x, W and b gradients within 1.5x torch fp32 autograd's error (1e-6 floor)."""
    g = torch.Generator(device=DEV).manual_seed(12 + scaled)
    for m, c in ((12000, 128), (5000, 256)):
        h = 4 * c
        x = torch.randn(m, c, device=DEV, generator=g) * 0.8 + 0.1
        gamma = 1.0 + 0.1 * torch.randn(c, device=DEV, generator=g)
        beta = 0.1 * torch.randn(c, device=DEV, generator=g)
        w1 = torch.randn(h, c, device=DEV, generator=g) * c ** -0.5
        b1 = torch.randn(h, device=DEV, generator=g) * 0.1
        w2 = torch.randn(c, h, device=DEV, generator=g) * h ** -0.5
        b2 = torch.randn(c, device=DEV, generator=g) * 0.1
        s = (torch.rand(m, device=DEV, generator=g) < 0.5).float() * 2.0 if scaled else None
        dout = torch.randn(m, c, device=DEV, generator=g)
        for t in (x, gamma, beta, w1, b1, w2, b2):
            t.requires_grad_()
        names = ('x', 'gamma', 'beta', 'W1', 'b1', 'W2', 'b2')

        def f6(x, gamma, beta, w1, b1, w2, b2):
            return ag.ln_mlp_residual_x6(x, gamma, beta, 1e-5, w1, b1, w2, b2, s)

        def fref(x, gamma, beta, w1, b1, w2, b2):
            return _mlp_branch_ref(x, gamma, beta, w1, b1, w2, b2, None if s is None else s.to(x.dtype))

        args = (x, gamma, beta, w1, b1, w2, b2)
        y6, g6 = _grads(f6, args, dout)
        y32, g32 = _grads(fref, args, dout)
        y64, g64 = _grads(fref, [t.double() for t in args], dout.double())
        assert _rel(y6, y64) <= max(1.5 * _rel(y32, y64), 1e-6)
        for name, a, l, r in zip(names, g6, g32, g64):
            e, e32 = _rel(a, r), _rel(l, r)
            print('ln_mlp_residual_x6 M %d C %d scaled %s d%s: %.2e  fp32 autograd %.2e' % (m, c, scaled, name, e, e32))
            if name != 'gamma' and name != 'beta':
                assert e <= max(1.5 * e32, 1e-6), (m, c, name, e, e32)
            else:                       # LayerNorm's parameters: the same HIP LayerNorm backward as the x3 path
                assert e <= 1e-5, (m, c, name, e, e32)
        if scaled:
            continue
        # ag.mlp_x6: fc2(gelu(fc1(h))) alone (no LayerNorm, no residual)
        margs = (x, w1, b1, w2, b2)
        y6, g6 = _grads(ag.mlp_x6, margs, dout)
        mref = lambda x, w1, b1, w2, b2: F.linear(F.gelu(F.linear(x, w1, b1)), w2, b2)     # noqa: E731
        y32, g32 = _grads(mref, margs, dout)
        y64, g64 = _grads(mref, [t.double() for t in margs], dout.double())
        assert _rel(y6, y64) <= max(1.5 * _rel(y32, y64), 1e-6)
        for name, a, l, r in zip(('x', 'W1', 'b1', 'W2', 'b2'), g6, g32, g64):
            e, e32 = _rel(a, r), _rel(l, r)
            print('mlp_x6 M %d C %d d%s: %.2e  fp32 autograd %.2e' % (m, c, name, e, e32))
            assert e <= max(1.5 * e32, 1e-6), (m, c, name, e, e32)


def _block_linear_weights(model):
    """id(weight) -> name of every block Linear the x6 route must take.  The one SplitLinear it leaves alone is the first layer
    of ADaPE's MLP (9 input features: no shape for the hand-written kernels; stays on F.linear by design)."""
    from hotformerloc_amd.model import FeatureMixerLayer, SplitLinear
    ids = {}
    for name, mod in model.named_modules():
        if isinstance(mod, SplitLinear):
            if not ag.linear_x6_ok(mod.in_features, mod.out_features):
                assert 'adape' in name and mod.in_features == 9, name
                continue
            ids[id(mod.weight)] = name
        elif isinstance(mod, FeatureMixerLayer):
            ids[id(mod.mix[1].weight)] = name + '.fc1'
            ids[id(mod.mix[3].weight)] = name + '.fc2'
    return ids


@pytest.mark.parametrize('cfg', ['wild-places', 'cs-wild-places'])
def test_no_library_gemm_in_the_block_linears(monkeypatch, cfg):
    """x6 training: forward + backward without F.linear (hipBLASLt) on any SplitLinear (attention qkv / proj of the octree
    and relay-token blocks, MLP fc1 / fc2) or Mixer fc1 / fc2.  The library route (set_train_x6(False)) does use them -- the
    recorder sees what it should."""
    params, depth = load_config(cfg)
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'stress')
    model = model.cuda().train()
    clouds = syn.make_clouds(31, 2, 1500, params.coordinates)
    octree = build_batch_octree(clouds, depth, 2, DEV)
    block = _block_linear_weights(model)
    seen = []
    real_linear = F.linear

    def recording_linear(x, weight, bias=None):
        seen.append(id(weight))
        return real_linear(x, weight, bias)

    monkeypatch.setattr(torch.nn.functional, 'linear', recording_linear)
    found = {}
    set_gemm_mode('x6')
    try:
        for route in (True, False):
            set_train_x6(route)
            seen.clear()
            torch.manual_seed(0)
            y = model({'octree': octree})['global']
            y.square().sum().backward()
            found[route] = sorted({block[i] for i in seen if i in block})
    finally:
        set_train_x6(True)
        set_gemm_mode('x3')
    print(cfg, 'library route: %d block Linears on F.linear' % len(found[False]))
    assert not found[True], found[True][:8]
    assert len(found[False]) > 10


_ORACLE = {}


@pytest.mark.parametrize('cfg,sizes', [('cs-wild-places', [2000, 1400]), ('wild-places', [1300, 800, 1000])])
def test_x6_training_gradients_match_oracle(cfg, sizes):
    """The workloads of test_forward_backward_matches_oracle_autograd in GEMM mode x6 (drop_path = 0): forward within 1e-3,
    every parameter gradient within GRAD_TOL rel-L2 of autograd through the CPU oracle, and per parameter kind the worst
    error at most 2x that of the fp32 library route (set_train_x6(False)) on the same model."""
    from oracle import hotformer_ref
    from oracle.testing import oracle_octree, synthetic_state_dict
    params, depth = load_config(cfg)
    clouds = [syn.forest_cloud(1400 + i, n) if i % 2 else syn.unit_ball_cloud(1400 + i, n) for i, n in enumerate(sizes)]
    if params.coordinates == 'cylindrical':
        clouds = [syn.cylindrical(c) for c in clouds]
    proj = torch.from_numpy(syn.hash_uniform(4242, len(sizes) * 256).reshape(len(sizes), 256).astype(np.float32))
    key = (cfg, tuple(sizes))
    if key not in _ORACLE:
        sd = {k: v.clone().requires_grad_() for k, v in synthetic_state_dict(params, 'stress').items()}
        y_ref = hotformer_ref.forward_with_grad(sd, params, oracle_octree(clouds, depth))
        (y_ref * proj).sum().backward()
        _ORACLE[key] = (y_ref.detach(), {k: v.grad for k, v in sd.items()})
    y_ref, grads_ref = _ORACLE[key]
    params.drop_path = 0.0
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'stress')
    model = model.cuda().train()
    octree = build_batch_octree(clouds, depth, 2, DEV)
    worst, rels = {}, {}
    set_gemm_mode('x6')
    try:
        for route in (True, False):
            set_train_x6(route)
            model.zero_grad(set_to_none=True)
            y = model({'octree': octree})['global']
            (y * proj.cuda()).sum().backward()
            rel = np.linalg.norm(y.detach().cpu().numpy() - y_ref.numpy(), axis=1) / np.linalg.norm(y_ref.numpy(), axis=1)
            rels[route] = float(rel.max())
            w = worst.setdefault(route, {})
            for name, p in model.named_parameters():
                gref = grads_ref[name]
                assert p.grad is not None, name
                err = (p.grad.cpu() - gref).norm().item() / max(gref.norm().item(), 1e-12)
                kind = name.split('.')[-1] if 'rpe_table' not in name else 'rpe_table'
                w[kind] = max(w.get(kind, 0.0), err)
                if route:
                    assert err < GRAD_TOL or gref.norm().item() < 1e-9, (name, err, gref.norm().item())
    finally:
        set_train_x6(True)
        set_gemm_mode('x3')
    print(cfg, 'forward rel: x6 route %.2e, library route %.2e' % (rels[True], rels[False]))
    for kind in sorted(worst[True]):
        print('  %-12s worst grad rel-L2: x6 route %.2e  library route %.2e' % (kind, worst[True][kind], worst[False][kind]))
    assert rels[True] <= 1e-3, rels
    bad = {k: (v, worst[False][k]) for k, v in worst[True].items() if v > 2.0 * worst[False][k]}
    assert not bad, bad


def test_multistaged_step_in_x6_matches_direct_autograd_and_oracle_chain():
    """test_multistaged_step_on_the_encoder_matches_oracle_chain in GEMM mode x6: stage 1 (training_numerics, no autograd)
    runs the same launches as stage 3's recomputation, so the step agrees with direct autograd within 2e-4 and with the CPU
    oracle chain within 1e-3."""
    from hotformerloc_amd.losses import TruncatedSmoothAP
    from hotformerloc_amd.training import multistaged_training_step
    from oracle import hotformer_ref, loss_ref
    from oracle.testing import oracle_octree, synthetic_state_dict
    params, depth = load_config('wild-places')
    params.drop_path = 0.0
    clouds = [syn.cylindrical(syn.unit_ball_cloud(3100 + i, 700 + 100 * i)) for i in range(4)]
    parts = [clouds[:2], clouds[2:]]
    lab = torch.arange(4) // 2
    pos = (lab[:, None] == lab[None, :]) & ~torch.eye(4, dtype=torch.bool)
    neg = lab[:, None] != lab[None, :]
    loss_fn = TruncatedSmoothAP(tau1=0.01, positives_per_query=1)

    def fresh():
        m = model_factory(params)
        syn.fill_synthetic_weights(m, 'stress')
        return m.cuda()

    set_gemm_mode('x6')
    try:
        model = fresh()
        mbs = [{'octree': build_batch_octree(p, depth, 2, DEV)} for p in parts]
        stats = multistaged_training_step(model, mbs, pos, neg, loss_fn)
        direct = fresh().train()
        emb = torch.cat([direct({'octree': build_batch_octree(p, depth, 2, DEV)})['global'] for p in parts], 0)
        loss, _ = loss_fn(emb, pos, neg)
        loss.backward()
    finally:
        set_train_x6(True)
        set_gemm_mode('x3')
    assert abs(stats['loss'] - loss.item()) < 1e-5
    for (n, p), q in zip(model.named_parameters(), direct.parameters()):
        d = (p.grad - q.grad).norm().item()
        assert d <= 2e-4 * max(q.grad.norm().item(), 1e-9) + 1e-9, (n, d, q.grad.norm().item())
    sd = {k: v.clone().requires_grad_() for k, v in synthetic_state_dict(params, 'stress').items()}
    emb_ref = torch.cat([hotformer_ref.forward_with_grad(sd, params, oracle_octree(p, depth)) for p in parts], 0)
    want, _ = loss_ref.truncated_smooth_ap(emb_ref, pos, neg, 0.01, 1)
    want.backward()
    assert abs(stats['loss'] - want.item()) < 1e-4
    worst = 0.0
    for n, p in model.named_parameters():
        gref = sd[n].grad
        err = (p.grad.cpu() - gref).norm().item() / max(gref.norm().item(), 1e-12)
        worst = max(worst, err if gref.norm().item() > 1e-9 else 0.0)
        assert err < 1e-3 or gref.norm().item() < 1e-9, (n, err, gref.norm().item())
    print('x6 multistaged step: loss', stats['loss'], want.item(), 'worst param-grad rel-L2 vs oracle', worst)


@pytest.mark.timeout(900)
def test_cs_wild_places_b64_x6_train_forward_backward():
    """BASELINE config 3 at full size (64 clouds of 4096..32768 points, the config's stochastic depth and grad_checkpoint)
    in GEMM mode x6 under autograd: finite descriptors and gradients, no parameter with an all-zero gradient."""
    params, depth = load_config('cs-wild-places')
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'init')
    model = model.cuda().train()
    clouds = []
    for i in range(64):
        clouds += syn.make_clouds(3, 1, 4096, 'cartesian', kind='forest' if i % 2 == 0 else 'ball', n_points_max=32768,
                                  first_index=i)
    octree = build_batch_octree(clouds, depth, 2, DEV)
    proj = torch.from_numpy(syn.hash_uniform(7, 64 * 256).reshape(64, 256).astype(np.float32)).cuda()
    set_gemm_mode('x6')
    try:
        torch.manual_seed(0)
        y = model({'octree': octree})['global']
        assert y.shape == (64, 256) and torch.isfinite(y).all()
        (y * proj).sum().backward()
        torch.cuda.synchronize()
    finally:
        set_train_x6(True)
        set_gemm_mode('x3')
    n_zero = []
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        assert torch.isfinite(p.grad).all(), name
        if p.grad.abs().max().item() == 0.0:
            n_zero.append(name)
    assert not n_zero, 'parameters with an all-zero gradient: %s' % n_zero[:8]
