"""The FeatureMixerLayers of the pooling head plus row_proj as ONE launch (hfl_mixer_chain_x3, csrc/mixer_chain.hip) and the
rest of the head with the normalisation (hfl_descriptor_tail, csrc/attn_pool.hip) against the launches they replace, against
float64, and inside the model."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from hotformerloc_amd import _native, build_batch_octree, load_config, model_factory, ops
from hotformerloc_amd import synthetic as syn

DEV = 'cuda'
C = 256
EPS = 1e-5
ROWS = 32           # rows per workgroup of the shipped launch (MC_ROWS); 64 was the other candidate
M_CASES = (1, 17, ROWS - 1, ROWS + 1, 63, 65, 300, 8192)


def _layers(n, seed=41):
    """n DISTINCT random layers (the scales of test_ln_mlp_fused_mixer_shape_hidden_equals_channels): a wrong layer order or
    pack stride cannot cancel."""
    g = torch.Generator().manual_seed(seed)
    return [dict(w1=torch.randn(C, C, generator=g) * 0.06, w2=torch.randn(C, C, generator=g) * 0.06,
                 b1=torch.randn(C, generator=g) * 0.1, b2=torch.randn(C, generator=g) * 0.1,
                 gamma=1 + 0.1 * torch.randn(C, generator=g), beta=0.1 * torch.randn(C, generator=g)) for _ in range(n)]


def _mlp_ref(x, p):
    h = torch.nn.functional.layer_norm(x, (C,), p['gamma'].double(), p['beta'].double(), EPS)
    h = torch.nn.functional.gelu(h @ p['w1'].double().t() + p['b1'].double())
    return x + h @ p['w2'].double().t() + p['b2'].double()


_DEVICE_LAYERS, _CASES = {}, {}


def _on_device(n):
    if n not in _DEVICE_LAYERS:
        d = [{k: v.to(DEV) for k, v in p.items()} for p in _layers(n)]
        _DEVICE_LAYERS[n] = (d, ops.mixer_chain_pack([p['w1'] for p in d], [p['w2'] for p in d]),
                             [ops.mlp_fused_pack(p['w1'], p['w2']) for p in d])
    return _DEVICE_LAYERS[n]


def _chain(x, n, row_w=None, want_x=True):
    d, pack, _ = _on_device(n)
    return ops.mixer_chain(x, pack, [p['gamma'] for p in d], [p['beta'] for p in d], [p['b1'] for p in d],
                           [p['b2'] for p in d], EPS, row_w=row_w, want_x=want_x)


def _case(m, n):
    """x, the chain (twice), the loop of hfl_ln_mlp_fused_h launches and the chained float64 reference: once per (M, L)."""
    if (m, n) not in _CASES:
        x = torch.randn(m, C, generator=torch.Generator().manual_seed(1000 * n + m)) * 2
        xd = x.to(DEV)
        d, _, packs = _on_device(n)
        got, got2 = _chain(xd, n)[0], _chain(xd, n)[0]
        loop = xd
        for p, pack in zip(d, packs):
            loop = ops.ln_mlp_fused(loop, p['gamma'], p['beta'], EPS, pack, p['b1'], p['b2'])
        ref = x.double()
        for p in _layers(n):
            ref = _mlp_ref(ref, p)
        _CASES[(m, n)] = dict(x=xd, chain=got.cpu(), chain2=got2.cpu(), loop=loop.cpu(), ref=ref)
    return _CASES[(m, n)]


@pytest.mark.parametrize('n_layers', [1, 4])
@pytest.mark.parametrize('m', M_CASES)
def test_chain_matches_the_launches_it_replaces_and_float64(m, n_layers):
    """One row, partial 16-row tiles, one row less and one more than a workgroup's (both candidates), several workgroups, the
    bench's 8192 rows; 1 and 4 distinct layers.  Relative L2 against float64 of the chain at most 1.5 x that of the loop of
    launches on the same input (the yardstick is the existing path; the margin covers another f32 summation order and nothing
    else -- a lost rounding point is a ratio of 100 or more); two calls bitwise equal; per layer (L = 1) the bars of
    test_ln_mlp_fused_mixer_shape_hidden_equals_channels."""
    c = _case(m, n_layers)
    chain, loop, ref = c['chain'].double(), c['loop'].double(), c['ref']
    assert torch.isfinite(chain).all()
    e_chain = ((chain - ref).norm() / ref.norm()).item()
    e_loop = ((loop - ref).norm() / ref.norm()).item()
    diff = (chain - loop).abs().max().item()
    print('mixer chain M = %d, L = %d: rel L2 vs float64: chain %.3e, launches %.3e; max|chain - launches| %.3e (max|ref| %.3e)'
          % (m, n_layers, e_chain, e_loop, diff, ref.abs().max().item()))
    assert torch.equal(c['chain'], c['chain2'])
    assert e_chain <= 1.5 * e_loop, (e_chain, e_loop)
    if n_layers == 1:
        assert e_chain < 1e-5, e_chain
        assert diff <= 2e-5 * ref.abs().max().item(), diff


@pytest.mark.parametrize('d', [1, 4, 8])
def test_row_proj_epilogue(d):
    """u = x_final Wr^T against float64 of the chain's own x_final (the 2e-5 max|want| bar of
    test_mixer_tail_matches_the_two_linears), rows past the last whole workgroup included; with and without out_x the same
    u bit for bit."""
    c = _case(300, 4)
    wr = (torch.randn(d, C, generator=torch.Generator().manual_seed(7 + d)) * 0.1).to(DEV)
    x_out, u = _chain(c['x'], 4, row_w=wr)
    _, u_only = _chain(c['x'], 4, row_w=wr, want_x=False)
    assert torch.equal(x_out.cpu(), c['chain'])
    assert tuple(u.shape) == (300, d) and torch.equal(u, u_only)
    want = c['chain'].double() @ wr.cpu().double().t()
    assert (u.cpu().double() - want).abs().max().item() < 2e-5 * want.abs().max().item()


def _tail_ref(u_src, wc, bc, wr, br):
    """the reference order of test_mixer_tail_matches_the_two_linears in float64, from the token matrix x"""
    y = torch.nn.functional.linear(u_src.double().permute(0, 2, 1), wc.double(), bc.double()).permute(0, 2, 1)
    return torch.nn.functional.linear(y, wr.double(), br.double()).flatten(1)


@pytest.mark.parametrize('b,k,ko,d', [(5, 256, 64, 4), (3, 128, 32, 8), (1, 77, 19, 1)])
def test_descriptor_tail_matches_the_two_linears_and_normalize(b, k, ko, d):
    g = torch.Generator().manual_seed(3 + k)
    c = 64
    x = torch.randn(b, k, c, generator=g)
    wc, bc = torch.randn(ko, k, generator=g) * 0.1, torch.randn(ko, generator=g)
    wr, br = torch.randn(d, c, generator=g) * 0.1, torch.randn(d, generator=g)
    want = _tail_ref(x, wc, bc, wr, br)
    u = (x.double() @ wr.double().t()).float().to(DEV)                      # row_proj without its bias
    args = (u, wc.to(DEV), bc.to(DEV), wr.to(DEV), br.to(DEV))
    got = ops.descriptor_tail(*args, False).cpu().double()
    assert got.shape == want.shape
    assert (got - want).abs().max().item() < 2e-5 * want.abs().max().item()
    wantn = torch.nn.functional.normalize(want, dim=1)
    gotn = ops.descriptor_tail(*args, True)
    assert (gotn.cpu().double() - wantn).abs().max().item() < 2e-5 * wantn.abs().max().item()
    assert torch.equal(gotn, ops.descriptor_tail(*args, True))


def test_descriptor_tail_of_a_zero_row_is_zero():
    """u = 0 and zero biases: the norm is 0, the row is divided by 1e-12 like F.normalize -- zeros, no NaN."""
    b, k, ko, d, c = 2, 40, 10, 4, 64
    g = torch.Generator().manual_seed(9)
    wc, wr = (torch.randn(ko, k, generator=g) * 0.1).to(DEV), (torch.randn(d, c, generator=g) * 0.1).to(DEV)
    u = torch.zeros(b, k, d, device=DEV)
    u[1] = torch.randn(k, d, generator=g).to(DEV)
    got = ops.descriptor_tail(u, wc, torch.zeros(ko, device=DEV), wr, torch.zeros(d, device=DEV), True).cpu()
    assert torch.isfinite(got).all() and torch.equal(got[0], torch.zeros(ko * d))
    assert abs(got[1].double().norm().item() - 1) < 1e-6


def test_refusals_launch_nothing():
    """C = 128, hidden = 512, L = 0 and 5, D = 9, non-contiguous x, null pointers: HFL_EINVAL, and the outputs keep what they
    held."""
    lib = _native.load()
    assert ops.mixer_chain_ok(256, 256, 1, 0) and ops.mixer_chain_ok(256, 256, 4, 8)
    for bad in ((128, 128, 4, 4), (256, 512, 4, 4), (256, 256, 0, 4), (256, 256, 5, 4), (256, 256, 4, 9), (256, 256, 4, -1)):
        assert not ops.mixer_chain_ok(*bad), bad
    d, pack, _ = _on_device(4)
    x = torch.randn(40, C, device=DEV)

    def vecs(n=4, width=C):
        return [[torch.zeros(width, device=DEV) for _ in range(n)] for _ in range(4)]

    einval = 'HFL_EINVAL'
    with pytest.raises(_native.NativeLibraryError, match=einval):                              # C = 128
        ops.mixer_chain(torch.randn(40, 128, device=DEV), pack, *vecs(4, 128), EPS)
    with pytest.raises(_native.NativeLibraryError, match=einval):                              # hidden = 512
        g, b, _, b2 = vecs()
        ops.mixer_chain(x, pack, g, b, [torch.zeros(512, device=DEV) for _ in range(4)], b2, EPS)
    for n in (0, 5):                                                                           # L = 0, 5
        with pytest.raises(_native.NativeLibraryError, match=einval):
            ops.mixer_chain(x, pack, *vecs(n), EPS)
    with pytest.raises(_native.NativeLibraryError, match=einval):                              # D = 9
        ops.mixer_chain(x, pack, *vecs(), EPS, row_w=torch.zeros(9, C, device=DEV))
    with pytest.raises(_native.NativeLibraryError, match=einval):                              # rows with a stride
        ops.mixer_chain(torch.randn(40, 2 * C, device=DEV)[:, :C], pack, *vecs(), EPS)

    # the entry point itself: layer counts, D, null pointers
    out = torch.full((40, C), 7.0, device=DEV)
    u = torch.full((40, 8), 7.0, device=DEV)
    tabs = [_native.ptr_array([t.data_ptr() for t in v]) for v in vecs()]
    wr = torch.zeros(8, C, device=DEV)

    def call(out_x=out.data_ptr(), out_u=u.data_ptr(), xp=x.data_ptr(), pk=pack.data_ptr(), t=tabs, row_w=wr.data_ptr(), m=40,
             layers=4, out_d=8):
        return lib.hfl_mixer_chain_x3(out_x, out_u, xp, pk, t[0], t[1], t[2], t[3], EPS, row_w, m, layers, out_d, ops._stream())

    for kw in (dict(layers=0), dict(layers=5), dict(out_d=9), dict(out_d=-1), dict(xp=None), dict(pk=None), dict(row_w=None),
               dict(out_u=None), dict(out_x=None, out_u=None, out_d=0), dict(m=-1), dict(t=[None] + tabs[1:]),
               dict(t=tabs[:3] + [_native.ptr_array([0] * 4)])):
        assert call(**kw) == _native.HFL_EINVAL, kw
    nul = _native.ptr_array([0] * 4)
    assert lib.hfl_mixer_chain_pack(pack.data_ptr(), nul, nul, 4, ops._stream()) == _native.HFL_EINVAL
    assert lib.hfl_mixer_chain_pack_bytes(0) == 0 and lib.hfl_mixer_chain_pack_bytes(5) == 0
    assert lib.hfl_descriptor_tail(None, u.data_ptr(), wr.data_ptr(), wr.data_ptr(), wr.data_ptr(), wr.data_ptr(), 1, 40, C, 10,
                                   8, 1, ops._stream()) == _native.HFL_EINVAL
    assert lib.hfl_descriptor_tail(out.data_ptr(), u.data_ptr(), wr.data_ptr(), wr.data_ptr(), wr.data_ptr(), wr.data_ptr(), 1,
                                   40, C, 10, 9, 1, ops._stream()) == _native.HFL_EINVAL
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (u == 7.0).all()
    assert call(m=0) == 0                                                                      # no rows: nothing to do
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (u == 7.0).all()


_MODEL = {}


def _model_and_octree():
    """The Wild-Places model (stress weights) and a batch octree of three small clouds, built once."""
    if not _MODEL:
        params, depth = load_config('wild-places')
        model = model_factory(params)
        syn.fill_synthetic_weights(model, 'stress')
        clouds = [c[:n] for c, n in zip(syn.make_clouds(23, 3, 2000, params.coordinates), (800, 1400, 2000))]
        _MODEL['m'] = (model.cuda().eval(), build_batch_octree(clouds, depth, 2, 'cuda'))
    return _MODEL['m']


def _descriptors(chain, normalize, counts):
    from hotformerloc_amd import model as M
    model, octree = _model_and_octree()
    lib = _native.load()
    entries = {n: getattr(lib, n) for n in ('hfl_mixer_chain_x3', 'hfl_descriptor_tail', 'hfl_mixer_tail')}

    def counted(name):
        def f(*a):
            counts[name] = counts.get(name, 0) + 1
            return entries[name](*a)
        return f

    keep = model.normalize_embeddings
    M._MIXER_CHAIN, model.normalize_embeddings = chain, normalize
    for n in entries:
        setattr(lib, n, counted(n))
    try:
        with torch.no_grad():
            return model({'octree': octree})['global'].cpu()
    finally:
        M._MIXER_CHAIN, model.normalize_embeddings = True, keep
        for n, f in entries.items():
            setattr(lib, n, f)


@pytest.mark.parametrize('normalize', [True, False])
def test_model_descriptors_with_the_chain_match_the_launches(normalize):
    """Wild-Places forward of three small clouds in GEMM mode x3: the head as two launches against a launch per layer,
    hfl_mixer_tail and F.normalize -- relative L2 of the descriptors <= 1e-5 per cloud (the bar of
    tests/test_gpu_relay_block_fused.py's seam), with and without normalize_embeddings.  The new entries run with the switch on
    (once each) and never with it off."""
    on_calls, off_calls = {}, {}
    on = _descriptors(True, normalize, on_calls)
    off = _descriptors(False, normalize, off_calls)
    assert on_calls.get('hfl_mixer_chain_x3') == 1 and on_calls.get('hfl_descriptor_tail') == 1, on_calls
    assert 'hfl_mixer_tail' not in on_calls
    assert 'hfl_mixer_chain_x3' not in off_calls and 'hfl_descriptor_tail' not in off_calls, off_calls
    assert off_calls.get('hfl_mixer_tail') == 1
    rel = (on.double() - off.double()).norm(dim=1) / off.double().norm(dim=1)
    print('mixer chain on / off, normalize %s: descriptors rel L2 per cloud:' % normalize, rel.tolist())
    assert torch.isfinite(on).all() and rel.max().item() <= 1e-5, rel
    if normalize:
        assert (on.double().norm(dim=1) - 1).abs().max().item() < 1e-6


def test_gemm_mode_x6_does_not_take_the_chain():
    from hotformerloc_amd import model as M
    calls = {}
    mode = M._GEMM_MODE
    M.set_gemm_mode('x6')
    try:
        out = _descriptors(True, True, calls)
    finally:
        M.set_gemm_mode(mode)
    assert torch.isfinite(out).all()
    assert 'hfl_mixer_chain_x3' not in calls and 'hfl_descriptor_tail' not in calls, calls
