"""The split-precision and fp16-operand kernels across input magnitudes ("numeric range contract").

Most assertions are tolerance-free: a kernel that is pure floating-point arithmetic commutes with powers of two bit for bit, so a
flush, a hidden constant, an fp16 intermediate or a per-tensor scale shows as a changed bit.  The rest are per-element bounds
derived from the operand formats (tests/range_cases.py; proven on the CPU in tests/test_range_host.py) or measured against torch's
own fp32 operator on the same inputs on the same device."""

import ctypes
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hotformerloc_amd import _native, ops

import range_cases as rc
from attention_cases import DEV, pack_qkv_f16, plans, relay_ref, sequence_table, windows_ref


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _split2_halves(a2, c):
    """split2 (rows, 2c) bf16 -> (hi, lo) bf16 (rows, c)."""
    v = a2.view(a2.shape[0], c // 32, 2, 32)
    return v[:, :, 0].reshape(-1, c), v[:, :, 1].reshape(-1, c)


def _unsplit2(a2, c):
    hi, lo = _split2_halves(a2.cpu(), c)
    return hi.double() + lo.double()


def _u16(t):
    return t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


# ------------------------------------------------------------------------------------------------------------ 2. splits
@pytest.mark.parametrize('rows,c', rc.SPLIT_SHAPES)
def test_splits_per_element_over_the_exponent_range(rows, c):
    """split2 (with and without row_scale), split3, split2_weight and the LayerNorm producers, element by element over
    +-m 2^e, e in [-100, 100]: hi bit-equal to the host model of round-to-nearest-even, |hi + lo - v| <= 2^-17 |v|, lo bit-equal
    to the model too, the same pairs in the split2 and the [hi | hi | lo] layout."""
    v = rc.split_values(rows, c, 100 + rc.SPLIT_SHAPES.index((rows, c)))
    d = v.to(DEV)

    def check_pairs(hi, lo, value, what):
        mh, ml = rc.split_bf16(value.numpy())
        assert np.array_equal(_u16(hi), rc.bf16_rne_bits(value.numpy())), what
        err = (hi.cpu().double() + lo.cpu().double() - value.double()).abs().numpy()
        assert (err <= rc.e_bf(value.numpy())).all(), (what, float((err / np.maximum(rc.e_bf(value.numpy()), 1e-300)).max()))
        assert np.array_equal(_u16(lo), rc.bf16_rne_bits(ml)), what

    s2 = ops.split2(d)
    hi, lo = _split2_halves(s2, c)
    check_pairs(hi, lo, v, 'split2')
    a3 = ops.split3(d)
    assert _same(a3[:, :c], hi) and _same(a3[:, c:2 * c], hi) and _same(a3[:, 2 * c:], lo)
    scale = rc.row_scales(rows, 9 + rows)
    hs, ls = _split2_halves(ops.split2(d, scale.to(DEV)), c)
    check_pairs(hs, ls, v * scale[:, None], 'split2 row_scale')
    hw, lw = _split2_halves(ops.split2_weight(d), c)
    check_pairs(hw, lw, v, 'split2_weight')
    if c >= 128:                                          # the LayerNorm kernels: gamma carries the exponent sweep
        x = rc.real_values((rows, c), 300 + rows)
        gamma = rc.shrink_exponents(rc.split_values(1, c, 77)[0])          # 2^-90 .. 2^90: times |LN| < 2^4 stays below 2^100
        beta = torch.zeros(c)
        beta[::3] = rc.shrink_exponents(rc.split_values(1, c, 78)[0])[::3]
        y = ops.layer_norm(x.to(DEV), gamma.to(DEV), beta.to(DEV)).cpu()
        mag = y.abs()[y != 0]
        # the lo half of the smallest value is still a normal number: 2^-116 2^-9 > 2^-126
        assert torch.isfinite(y).all() and float(mag.min()) >= 2.0 ** -116 and float(mag.max()) <= rc.RANGE_HI
        h2, l2 = _split2_halves(ops.layer_norm_split2(x.to(DEV), gamma.to(DEV), beta.to(DEV)), c)
        check_pairs(h2, l2, y, 'layer_norm_split2')
        a3 = ops.layer_norm_split3(x.to(DEV), gamma.to(DEV), beta.to(DEV))
        assert _same(a3[:, :c], h2) and _same(a3[:, c:2 * c], h2) and _same(a3[:, 2 * c:], l2)


@pytest.mark.parametrize('k', [32, 96, 256])
def test_x6_planes_sum_exactly_over_the_exponent_range(k):
    """x6_pack over 2^-100 .. 2^100: h + m + l == w exactly, each plane bit-equal to the host model."""
    w = rc.split_values(128, k, 600 + k)
    w3 = ops.x6_pack(w.to(DEV)).cpu()
    kp = (k + 63) // 64 * 64
    assert tuple(w3.shape) == (3, 128, kp) and (w3[:, :, k:] == 0).all()
    w3 = w3[:, :, :k]
    assert torch.equal(w3[0].double() + w3[1].double() + w3[2].double(), w.double())
    for plane, model in zip(w3, rc.split3_bf16(w.numpy())):
        assert np.array_equal(_u16(plane), rc.bf16_rne_bits(model))


# ------------------------------------------------------------------------------------------------------------ 3. equivariance
def _x3_forms(x, w, b, r):
    """linear_x3: plain, bias, bias + residual, bias + residual aliasing the output."""
    x2, w2 = ops.split2(x.to(DEV)), ops.split2_weight(w.to(DEV))
    bd, rd = b.to(DEV), r.to(DEV)
    buf = rd.clone()
    ops.linear_x3(x2, w2, bias=bd, residual=buf, out=buf)
    return [ops.linear_x3(x2, w2), ops.linear_x3(x2, w2, bias=bd), ops.linear_x3(x2, w2, bias=bd, residual=rd), buf]


def _x6_forms(x, w, b, r, sc):
    """linear_x6: plain, bias + residual, bias + row_scale + residual, residual aliasing the output."""
    xd, w6 = x.to(DEV), ops.x6_pack(w.to(DEV))
    bd, rd, sd = b.to(DEV), r.to(DEV), sc.to(DEV)
    buf = rd.clone()
    ops.linear_x6(xd, w6, bias=bd, residual=buf, out=buf)
    return [ops.linear_x6(xd, w6), ops.linear_x6(xd, w6, bias=bd, residual=rd),
            ops.linear_x6(xd, w6, bias=bd, residual=rd, row_scale=sd), buf]


def _equivariance(forms, x, w, b, r, tag):
    """out(2^a x, 2^b w, 2^(a+b) bias, 2^(a+b) residual) == 2^(a+b) out(x, w, bias, residual), and the per-column variant
    x[:, k] 2^(a_k), w[:, k] 2^(-a_k) == out: both bit for bit."""
    base = forms(x, w, b, r)
    for t in base:
        assert torch.isfinite(t).all(), tag
    for a, bb in itertools.product(rc.SCALES_A, rc.SCALES_B):
        got = forms(rc.pow2(x, a), rc.pow2(w, bb), rc.pow2(b, a + bb), rc.pow2(r, a + bb))
        for i, (g, t) in enumerate(zip(got, base)):
            assert _same(g, rc.pow2(t, a + bb)), (tag, 'form', i, a, bb)
    ak = rc.column_exponents(x.shape[1], 7 + x.shape[1])
    got = forms(torch.ldexp(x, ak), torch.ldexp(w, -ak), b, r)
    for i, (g, t) in enumerate(zip(got, base)):
        assert _same(g, t), (tag, 'per-column, form', i)


@pytest.mark.parametrize('k,n', rc.GEMM_KN)
def test_linear_x3_is_power_of_two_equivariant(k, n):
    for m in rc.GEMM_M:
        x, w, b, r = rc.gemm_case(m, k, n, 1000 + m + k + n)
        _equivariance(_x3_forms, x, w, b, r, ('x3', m, k, n))


@pytest.mark.parametrize('mt', rc.X6_TILES)
def test_linear_x6_is_power_of_two_equivariant_at_every_tile(mt):
    lib = _native.load()
    lib.hfl_internal_set_x6_mt.argtypes = [ctypes.c_int]
    try:
        lib.hfl_internal_set_x6_mt(mt)
        for (k, n), m in itertools.product(rc.GEMM_KN, rc.GEMM_M):
            x, w, b, r = rc.gemm_case(m, k, n, 1000 + m + k + n)
            sc = rc.row_scales(m, 5 + m)                                   # row_scale is left unscaled
            _equivariance(lambda *t: _x6_forms(*t, sc), x, w, b, r, ('x6', mt, m, k, n))
    finally:
        lib.hfl_internal_set_x6_mt(0)


@pytest.mark.parametrize('cin,cout', rc.GROUP_KN)
def test_grouped_linears_are_power_of_two_equivariant(cin, cout):
    """linear_x3_grouped, linear_x3_grouped_gather and linear_x6_grouped_gather over ragged tiles with a weight block each."""
    npad = max(cout, 128)
    nb = len(rc.GROUP_SIZES)
    tiles, edges = rc.grouped_tiles(rc.GROUP_SIZES, npad)
    tiles_t = torch.tensor(tiles, dtype=torch.int32, device=DEV)
    rows = edges[-1]
    x = rc.real_values((rows, cin), 3000 + cin)
    w = rc.real_values((nb * cout, cin), 3001 + cin, 0.25).view(nb, cout, cin)
    n_src = 97
    source = rc.real_values((n_src, cin), 3002 + cin)
    src = torch.from_numpy(np.random.RandomState(cin).randint(0, n_src, size=rows).astype(np.int32)).to(DEV)

    def padded(wt):
        wp = torch.cat([wt, wt.new_zeros(nb, npad - cout, cin)], 1) if npad > cout else wt
        return wp.reshape(nb * npad, cin).contiguous().to(DEV)

    def forms(xs, ws, ss):
        w2, w6 = ops.split2(padded(ws)), ops.x6_pack(padded(ws))
        return [ops.linear_x3_grouped(ops.split2(xs.to(DEV)), w2, tiles_t, cout),
                ops.linear_x3_grouped_gather(ops.split2(ss.to(DEV)), src, w2, tiles_t, cout),
                ops.linear_x6_grouped_gather(ss.to(DEV), src, w6, tiles_t, cout)]

    base = forms(x, w, source)
    assert all(torch.isfinite(t).all() for t in base)
    for a, bb in itertools.product(rc.SCALES_A, rc.SCALES_B):
        got = forms(rc.pow2(x, a), rc.pow2(w, bb), rc.pow2(source, a))
        for i, (g, t) in enumerate(zip(got, base)):
            assert _same(g, rc.pow2(t, a + bb)), (cin, cout, 'form', i, a, bb)
    ak = rc.column_exponents(cin, 7 + cin)
    got = forms(torch.ldexp(x, ak), torch.ldexp(w, -ak), torch.ldexp(source, ak))
    for i, (g, t) in enumerate(zip(got, base)):
        assert _same(g, t), (cin, cout, 'per-column, form', i)


@pytest.mark.parametrize('n,k', rc.WGRAD_NK)
def test_wgrad_is_power_of_two_equivariant(n, k):
    """wgrad_x3 and wgrad_f32: dW(2^a dy, 2^b x) == 2^(a+b) dW, db == 2^a db; rows scaled by 2^(a_m) / 2^(-a_m) leave dW alone
    (the contraction runs over the rows there)."""
    def forms(dy, x):
        dyd, xd = dy.to(DEV), x.to(DEV)
        dw3, db3 = ops.wgrad_x3(ops.split2(dyd), ops.split2(xd), with_bias=True)
        dwf, dbf = ops.wgrad_f32(dyd, xd, with_bias=True)
        return [dw3, dwf], [db3, dbf]

    for m in rc.WGRAD_M:
        dy, x = rc.real_values((m, n), 2000 + m + n), rc.real_values((m, k), 2001 + m + k)
        dws, dbs = forms(dy, x)
        assert all(torch.isfinite(t).all() for t in dws + dbs)
        for a, bb in itertools.product(rc.SCALES_A, rc.SCALES_B):
            gw, gb = forms(rc.pow2(dy, a), rc.pow2(x, bb))
            for i in range(2):
                assert _same(gw[i], rc.pow2(dws[i], a + bb)), (m, n, k, 'dW', i, a, bb)
                assert _same(gb[i], rc.pow2(dbs[i], a)), (m, n, k, 'db', i, a, bb)
        am = rc.column_exponents(m, 11 + m)
        gw, _ = forms(torch.ldexp(dy, am[:, None]), torch.ldexp(x, -am[:, None]))
        for i in range(2):
            assert _same(gw[i], dws[i]), (m, n, k, 'per-row dW', i)


# ------------------------------------------------------------------------------------------------------------ 4. per element
def _ratio(y, ref, mag):
    return float(((y.cpu().double() - ref).abs() / mag).max())


@pytest.mark.parametrize('k,n', rc.GEMM_KN)
def test_linear_error_per_element_against_float64(k, n):
    """|y - ref| <= c sum_k |x_k w_k| for EVERY element.  x3: c = 2^-15 (two operands at 2^-17 each give 2^-16, the dropped
    lo x lo term is below 2^-32, fp32 accumulation at most 1.5e-7 for K <= 1024, a factor 2 covers the rest).  x6:
    c = max(2 c_lib, 2^-22) with c_lib the largest such ratio of torch's fp32 linear on the same device and inputs."""
    for m, a in itertools.product(rc.GEMM_M, rc.ERR_SCALES):
        x, w, _, _ = rc.gemm_case(m, k, n, 1000 + m + k + n)
        x, w = rc.pow2(x, a), rc.pow2(w, a)
        ref = x.double() @ w.double().t()
        mag = x.double().abs() @ w.double().abs().t()
        assert torch.isfinite(ref).all() and rc.in_range(mag)
        xd, wd = x.to(DEV), w.to(DEV)
        c3 = _ratio(ops.linear_x3(ops.split2(xd), ops.split2_weight(wd)), ref, mag)
        c6 = _ratio(ops.linear_x6(xd, ops.x6_pack(wd)), ref, mag)
        c_lib = _ratio(torch.nn.functional.linear(xd, wd), ref, mag)
        print('per-element ratio M %d K %d N %d 2^%d: x3 %.3g  x6 %.3g  fp32 library %.3g' % (m, k, n, a, c3, c6, c_lib))
        assert c3 <= rc.C_X3, (m, k, n, a, c3)
        assert c6 <= max(2 * c_lib, rc.C_X6_FLOOR), (m, k, n, a, c6, c_lib)


@pytest.mark.parametrize('n,k', rc.WGRAD_NK)
def test_wgrad_error_per_element_against_float64(n, k):
    """The same bounds for dW = dy^T x, the sum running over the rows: wgrad_x3 at 2^-15, wgrad_f32 at max(2 c_lib, 2^-22)."""
    for m, a in itertools.product(rc.WGRAD_M, rc.ERR_SCALES):
        dy, x = rc.pow2(rc.real_values((m, n), 2000 + m + n), a), rc.pow2(rc.real_values((m, k), 2001 + m + k), a)
        ref = dy.double().t() @ x.double()
        mag = dy.double().abs().t() @ x.double().abs()
        dyd, xd = dy.to(DEV), x.to(DEV)
        c3 = _ratio(ops.wgrad_x3(ops.split2(dyd), ops.split2(xd))[0], ref, mag)
        cf = _ratio(ops.wgrad_f32(dyd, xd)[0], ref, mag)
        c_lib = _ratio(dyd.t() @ xd, ref, mag)
        print('per-element ratio wgrad m %d N %d K %d 2^%d: x3 %.3g  f32 %.3g  fp32 library %.3g' % (m, n, k, a, c3, cf, c_lib))
        assert c3 <= rc.C_X3, (m, n, k, a, c3)
        assert cf <= max(2 * c_lib, rc.C_X6_FLOOR), (m, n, k, a, cf, c_lib)


GELU_C = 128


def _gelu_rows(values):
    """The values as rows of 128 channels, zero padded: (x (rows, 128), number of real values)."""
    n = values.numel()
    rows = -(-n // GELU_C)
    x = torch.zeros(rows * GELU_C)
    x[:n] = values
    return x.view(rows, GELU_C), n


def _gelu_checks(g, v, bound, what):
    """g (float64, flat) against gelu64(v) under `bound`, and the properties no rounding may break."""
    ref = rc.gelu64(v)
    err = (g - ref).abs()
    worst = int((err / bound).argmax())
    print('gelu %s: worst err / bound %.3g at v = %r' % (what, float(err[worst] / bound[worst]), float(v[worst])))
    assert (err <= bound).all(), (what, float(v[worst]), float(err[worst]), float(bound[worst]))
    assert ((g == 0) | (torch.sign(g) == torch.sign(v.double()))).all(), what
    assert float(g.min()) >= -0.17, what
    tail = v <= -6
    assert (g[tail].abs() <= v[tail].double().abs() * 2e-7).all(), what


def test_gelu_epilogues_pointwise():
    """GELU and GELU' of every fused epilogue, value by value: a sweep pushed through an identity weight with zero bias, so the
    epilogue sees the value exactly.  |g - gelu64(v)| <= 2 max(E_lib(v), 0.5 |v| 1.5e-7 + 2^-24) [+ 2^-16 |gelu64(v)| for a
    split2 output], E_lib the error of torch's fp32 gelu at v on this device; the derivative likewise with the erf error
    entering Phi(v) directly (range_cases.gelu_grad_format_bound)."""
    eye = torch.eye(GELU_C, device=DEV)
    w2, w6 = ops.split2_weight(eye), ops.x6_pack(eye)
    zero = torch.zeros(GELU_C, device=DEV)
    sweep = rc.gelu_sweep()
    both = torch.cat([sweep, rc.gelu_random()])

    def lib_errors(v):
        vd = v.to(DEV).requires_grad_()
        y = torch.nn.functional.gelu(vd)
        y.sum().backward()
        return (y.detach().cpu().double() - rc.gelu64(v)).abs(), (vd.grad.cpu().double() - rc.gelu_grad64(v)).abs()

    for family, values in (('x3', sweep), ('x6', both)):
        x, n = _gelu_rows(values)
        xd = x.to(DEV)
        e_lib, e_lib_grad = lib_errors(values)
        fwd_bound = 2 * torch.maximum(e_lib, rc.gelu_format_bound(values))
        bwd_bound = 2 * torch.maximum(e_lib_grad, rc.gelu_grad_format_bound(values))
        ones = torch.ones_like(xd)
        if family == 'x3':
            x2 = ops.split2(xd)
            split_bound = fwd_bound + 2.0 ** -16 * rc.gelu64(values).abs()
            g = _unsplit2(ops.linear_x3(x2, w2, bias=zero, gelu_split_out=True), GELU_C).reshape(-1)[:n]
            _gelu_checks(g, values, split_bound, 'linear_x3(gelu_split_out)')
            out, pre = ops.linear_x3_gelu_fwd(x2, w2, zero)
            assert _same(pre.cpu().reshape(-1)[:n] + 0.0, values + 0.0)            # the epilogue saw the value exactly
            _gelu_checks(_unsplit2(out, GELU_C).reshape(-1)[:n], values, split_bound, 'linear_x3_gelu_fwd')
            d = _unsplit2(ops.linear_x3_gelu_bwd(ops.split2(ones), w2, xd), GELU_C).reshape(-1)[:n]
            grad_bound = bwd_bound + 2.0 ** -16 * rc.gelu_grad64(values).abs()
            what = 'linear_x3_gelu_bwd'
        else:
            g = ops.linear_x6(xd, w6, bias=zero, gelu=True).cpu().double().reshape(-1)[:n]
            _gelu_checks(g, values, fwd_bound, 'linear_x6(gelu)')
            out, pre = ops.linear_x6_gelu_fwd(xd, w6, zero)
            assert _same(pre.cpu().reshape(-1)[:n] + 0.0, values + 0.0)
            _gelu_checks(out.cpu().double().reshape(-1)[:n], values, fwd_bound, 'linear_x6_gelu_fwd')
            d = ops.linear_x6_gelu_bwd(ones, w6, xd).cpu().double().reshape(-1)[:n]
            grad_bound = bwd_bound
            what = 'linear_x6_gelu_bwd'
        err = (d - rc.gelu_grad64(values)).abs()
        worst = int((err / grad_bound).argmax())
        print("gelu' %s: worst err / bound %.3g at v = %r" % (what, float(err[worst] / grad_bound[worst]), float(values[worst])))
        assert (err <= grad_bound).all(), (what, float(values[worst]), float(err[worst]), float(grad_bound[worst]))
        assert float(d.min()) >= -0.13 and float(d.max()) <= 1.13, what


# ------------------------------------------------------------------------------------------------------------ 5. LayerNorm
def _ln_yardstick(x, gamma, beta):
    """(float64 LayerNorm, per-row bound 2 E_torch + 2^-22 max |ln64|) with E_torch the largest error of torch's fp32
    layer_norm on this device in that row."""
    ref = rc.ln64(x, gamma, beta)
    lib = torch.nn.functional.layer_norm(x.to(DEV), (x.shape[1],), gamma.to(DEV), beta.to(DEV), rc.LN_EPS).cpu().double()
    e_torch = (lib - ref).abs().amax(1, keepdim=True)
    return ref, 2 * e_torch + rc.LN_FLOOR * ref.abs().amax(1, keepdim=True), e_torch


def _ln_report(what, err, bound, kinds):
    ratio = (err / bound).amax(1)
    worst = {}
    for r, kind in enumerate(kinds):
        worst[kind] = max(worst.get(kind, 0.0), float(ratio[r]))
    print('layer norm %s: worst err / bound per row kind %s' % (what, {k: '%.3g' % v for k, v in sorted(worst.items())}))
    bad = [(r, kinds[r], float(ratio[r])) for r in range(len(kinds)) if ratio[r] > 1]
    assert not bad, (what, bad[:8])


def _ulp_apart(a, b):
    """Largest distance in units of the last place between two fp32 tensors of equal sign pattern."""
    ia, ib = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    return int((ia - ib).abs().max())


@pytest.mark.parametrize('rows,c', rc.LN_SHAPES)
def test_layer_norm_family_on_hard_rows(rows, c):
    """layer_norm, add_layer_norm, layer_norm_relu, layer_norm_split2 on rows with a large mean, rows scaled by 2^+-30, constant
    rows and a row with one dominant element: per element within 2 E_torch + 2^-22 max |ln64| of float64 LayerNorm of the same
    fp32 input; constant rows give beta to 1 ulp."""
    x, kinds = rc.ln_rows(rows, c, 40 + rc.LN_SHAPES.index((rows, c)))
    gamma, beta = rc.ln_params(c, 50 + rc.LN_SHAPES.index((rows, c)))
    ref, bound, _ = _ln_yardstick(x, gamma, beta)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    const = [r for r, kind in enumerate(kinds) if kind == 'const']
    y = ops.layer_norm(xd, gd, bd, rc.LN_EPS).cpu()
    assert torch.isfinite(y).all()
    _ln_report('layer_norm', (y.double() - ref).abs(), bound, kinds)
    assert _ulp_apart(y[const], beta.expand(len(const), c)) <= 1
    # add_layer_norm: x = u + v with an exact fp32 sum, so the reference input is the same
    u = (x.view(torch.int32) & ~0xFFF).view(torch.float32)               # the upper 12 significand bits, and the rest
    v = x - u
    assert torch.equal(u + v, x) and (v != 0).any()
    xo, h = ops.add_layer_norm(u.to(DEV), v.to(DEV), gd, bd, rc.LN_EPS)
    assert _same(xo.cpu(), x)
    _ln_report('add_layer_norm', (h.cpu().double() - ref).abs(), bound, kinds)
    assert _ulp_apart(h.cpu()[const], beta.expand(len(const), c)) <= 1
    yr = ops.layer_norm_relu(xd, gd, bd, rc.LN_EPS).cpu()
    _ln_report('layer_norm_relu', (yr.double() - ref.clamp(min=0)).abs(), bound, kinds)
    s2 = _unsplit2(ops.layer_norm_split2(xd, gd, bd, rc.LN_EPS), c)
    _ln_report('layer_norm_split2', (s2 - ref).abs(), bound + 2.0 ** -17 * ref.abs(), kinds)
    sr = _unsplit2(ops.layer_norm_relu(xd, gd, bd, rc.LN_EPS, split2=True), c)
    _ln_report('layer_norm_relu split2', (sr - ref.clamp(min=0)).abs(), bound + 2.0 ** -17 * ref.abs(), kinds)


@pytest.mark.parametrize('rows,c', rc.LN_SHAPES)
def test_layer_norm_backward_on_hard_rows(rows, c):
    """layer_norm_bwd against float64 autograd with torch's fp32 autograd on the device as the yardstick: dx per row within
    2 E_torch + 2^-22 max |dx64|, dgamma / dbeta per channel within 2 E_torch (torch's largest error over that vector, as a row
    is the unit of the forward yardstick) + 2^-22 of the sum of the magnitudes added into the channel."""
    i = rc.LN_SHAPES.index((rows, c))
    x, kinds = rc.ln_rows(rows, c, 40 + i)
    gamma, beta = rc.ln_params(c, 50 + i)
    dy = rc.real_values((rows, c), 60 + i)

    def autograd(dtype, device):
        xr, gr, br = (t.to(device=device, dtype=dtype).requires_grad_() for t in (x, gamma, beta))
        torch.nn.functional.layer_norm(xr, (c,), gr, br, rc.LN_EPS).backward(dy.to(device=device, dtype=dtype))
        return [t.grad.cpu().double() for t in (xr, gr, br)]

    want = autograd(torch.float64, 'cpu')
    lib = autograd(torch.float32, DEV)
    assert all(torch.isfinite(t).all() for t in want)
    dx, dg, db = (t.cpu().double() for t in ops.layer_norm_bwd(dy.to(DEV), x.to(DEV), gamma.to(DEV), rc.LN_EPS))
    e_torch = (lib[0] - want[0]).abs().amax(1, keepdim=True)
    _ln_report('layer_norm_bwd dx', (dx - want[0]).abs(), 2 * e_torch + rc.LN_FLOOR * want[0].abs().amax(1, keepdim=True), kinds)
    xhat = (rc.ln64(x, torch.ones(c), torch.zeros(c))).abs()
    for name, got, w, l, mag in (('dgamma', dg, want[1], lib[1], (dy.double().abs() * xhat).sum(0)),
                                 ('dbeta', db, want[2], lib[2], dy.double().abs().sum(0))):
        bound = 2 * (l - w).abs().max() + rc.LN_FLOOR * mag                 # E_torch: its largest error over the vector
        ratio = (got - w).abs() / bound
        print('layer norm bwd %s: worst err / bound %.3g' % (name, float(ratio.max())))
        assert (ratio <= 1).all(), (name, float(ratio.max()))


@pytest.mark.parametrize('rows,c', rc.LN_SHAPES)
def test_fused_layer_norm_prologues_on_hard_rows(rows, c):
    """The LayerNorm prologues of ln_qkv_fused and ln_mlp_fused on the same rows.  ln_qkv_fused with a block-identity weight
    and zero bias hands LN(x) to the fp16 (hi, lo) image: within the LayerNorm yardstick + e_bf (the split2 operand of the
    product) + e_h (the image) of float64, and close to its documented composition layer_norm_split2 -> linear_x3_qkv.
    ln_mlp_fused against float64 of x + fc2(gelu(fc1(LN(x)))) with the LayerNorm yardstick carried through both products,
    and against its composition layer_norm_split2 -> linear_x3(gelu) -> linear_x3(residual)."""
    i = rc.LN_SHAPES.index((rows, c))
    x, kinds = rc.ln_rows(rows, c, 40 + i)
    gamma, beta = rc.ln_params(c, 50 + i)
    ref, ln_bound, _ = _ln_yardstick(x, gamma, beta)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    H = c // 16
    w = rc.block_identity_qkv(c).to(DEV)
    zero3 = torch.zeros(3 * c, device=DEV)

    def image(buf):
        hi, lo = rc.decode_f16_image(buf, rows, H)
        return torch.from_numpy(hi.astype(np.float64) + lo.astype(np.float64)).reshape(rows, 3, c)

    fused = image(ops.ln_qkv_fused(xd, gd, bd, rc.LN_EPS, ops.qkv_fused_pack(w), zero3, 0.5))
    two = image(ops.linear_x3_qkv(ops.layer_norm_split2(xd, gd, bd, rc.LN_EPS), ops.split2_weight(w), zero3, 0.5))
    for part, factor in ((0, 0.5), (1, 1.0), (2, 1.0)):
        target = ref * factor
        fmt = torch.from_numpy(rc.e_bf(target.numpy()) + rc.e_h(target.numpy()))
        _ln_report('ln_qkv_fused part %d' % part, (fused[:, part] - target).abs(), ln_bound * factor + fmt, kinds)
        _ln_report('layer_norm_split2 + linear_x3_qkv part %d' % part, (two[:, part] - target).abs(), ln_bound * factor + fmt, kinds)
    # ln_mlp_fused
    hid = 4 * c
    w1, w2 = rc.real_values((hid, c), 70 + i, 0.05), rc.real_values((c, hid), 71 + i, 0.05)
    b1, b2 = rc.real_values((hid,), 72 + i, 0.1), rc.real_values((c,), 73 + i, 0.1)
    pre = ref @ w1.double().t() + b1.double()
    g = rc.gelu64(pre)
    want = x.double() + g @ w2.double().t() + b2.double()
    assert torch.isfinite(want).all()
    # error carried through: LayerNorm yardstick -> fc1 (x3: 2^-15 of the magnitudes) -> gelu (slope <= 1.13, its own error,
    # the split2 of its result) -> fc2 (x3) -> the fp32 sums with bias and residual
    e_pre = rc.C_X3 * (ref.abs() @ w1.double().abs().t() + b1.double().abs()) + ln_bound * w1.double().abs().sum(1)
    e_g = 1.13 * e_pre + 2 * rc.gelu_format_bound(pre) + 2.0 ** -16 * g.abs()
    e_out = rc.C_X3 * (g.abs() @ w2.double().abs().t()) + e_g @ w2.double().abs().t() + \
        2.0 ** -22 * (x.double().abs() + want.abs() + b2.double().abs())
    w1d, w2d, b1d, b2d = w1.to(DEV), w2.to(DEV), b1.to(DEV), b2.to(DEV)
    got = ops.ln_mlp_fused(xd, gd, bd, rc.LN_EPS, ops.mlp_fused_pack(w1d, w2d), b1d, b2d)
    assert torch.isfinite(got).all()
    _ln_report('ln_mlp_fused', (got.cpu().double() - want).abs(), e_out, kinds)
    h2 = ops.layer_norm_split2(xd, gd, bd, rc.LN_EPS)
    unf = ops.linear_x3(ops.linear_x3(h2, ops.split2_weight(w1d), bias=b1d, gelu_split_out=True), ops.split2_weight(w2d),
                        bias=b2d, residual=xd)
    _ln_report('layer_norm_split2 + linear_x3 + linear_x3', (unf.cpu().double() - want).abs(), e_out, kinds)


# ------------------------------------------------------------------------------------------------------------ 6a. operand image
@pytest.mark.parametrize('s', rc.F16_SCALES)
def test_fp16_operand_image_per_element(s):
    """linear_x3_qkv and ln_qkv_fused with a block-identity weight: q, k, v are the input times (q_scale, 1, 1).  Decoded as
    fp16 (rows, 3, H, 2, 16): hi == RTZ_fp16(v) bit for bit and |hi + lo - v| <= e_h(v) = max(2^-20 |v|, 2^-24), from 2^-20
    (deep in the fixed-point regime) to 2^15 (the largest value just below 65504)."""
    rows, c = rc.IMAGE_ROWS, rc.IMAGE_C
    H = c // 16
    v = rc.pow2(rc.image_values(rows, c, 500), s)
    w = rc.block_identity_qkv(c).to(DEV)
    zero3 = torch.zeros(3 * c, device=DEV)
    q_scale = 0.25 * rc.LOG2E
    x2 = ops.split2(v.to(DEV))
    hi2, lo2 = _split2_halves(x2.cpu(), c)
    seen = (hi2.float() + lo2.float())                                    # what the product hands the epilogue: hi + lo in fp32
    assert ((seen.double() - v.double()).abs().numpy() <= rc.e_bf(v.numpy())).all()
    want = torch.stack([seen * np.float32(q_scale), seen, seen], 1).numpy().reshape(rows, 3, H, 16)
    assert float(np.abs(want).max()) < rc.F16_MAX
    hi, lo = rc.decode_f16_image(ops.linear_x3_qkv(x2, ops.split2_weight(w), zero3, q_scale), rows, H)
    model_hi, _ = rc.split_fp16(want)
    assert np.array_equal(hi.view(np.uint16), model_hi.view(np.uint16)), s
    err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - want.astype(np.float64))
    print('fp16 image 2^%d: worst err / e_h %.3g, lo subnormal in %.0f %% of the elements'
          % (s, float((err / rc.e_h(want)).max()), 100 * float((np.abs(lo.astype(np.float64)) < 2.0 ** -14).mean())))
    assert (err <= rc.e_h(want)).all(), s
    # ln_qkv_fused: gamma = 2^(s - 2) on a unit-variance input makes LN(x) span the same scale (|LN(x)| < 7 stays below 65504 at
    # s = 15); its value is not known bit for bit, so the halves are checked for the shape of a truncation (lo below one
    # spacing of hi, of the same sign) and the pair against e_h on top of the LayerNorm yardstick
    x = rc.real_values((rows, c), 510)
    gamma, beta = torch.full((c,), 2.0 ** (s - 2)), torch.zeros(c)
    buf = ops.ln_qkv_fused(x.to(DEV), gamma.to(DEV), beta.to(DEV), rc.LN_EPS, ops.qkv_fused_pack(w), zero3, q_scale)
    hi, lo = rc.decode_f16_image(buf, rows, H)
    total = hi.astype(np.float64) + lo.astype(np.float64)
    assert np.isfinite(total).all() and float(np.abs(total).max()) < rc.F16_MAX
    assert (np.abs(lo.astype(np.float64)) < np.maximum(np.abs(hi.astype(np.float64)) * 2.0 ** -10, 2.0 ** -24) + 1e-300).all()
    assert (np.sign(lo.astype(np.float64)) * np.sign(hi.astype(np.float64)) >= 0).all()       # both halves truncate toward zero
    ref = rc.ln64(x, gamma, beta)
    target = torch.stack([ref * q_scale, ref, ref], 1).numpy().reshape(rows, 3, H, 16)
    lib = torch.nn.functional.layer_norm(x.to(DEV), (c,), gamma.to(DEV), beta.to(DEV), rc.LN_EPS).cpu().double()
    ln_bound = (2 * (lib - ref).abs().amax(1) + rc.LN_FLOOR * ref.abs().amax(1)).numpy().reshape(rows, 1, 1, 1)
    ln_bound = ln_bound * np.array([q_scale, 1.0, 1.0]).reshape(1, 3, 1, 1)
    bound = ln_bound +rc.e_bf(target) + rc.e_h(target) + 2.0 ** -23 * np.abs(target)           # the fp32 product with q_scale
    assert (np.abs(total - target) <= bound).all(), (s, float((np.abs(total - target) / bound).max()))


# ------------------------------------------------------------------------------------------------------------ 6b. attention
def _attention_case(K, G, depth):
    """Clouds, plans and unit-scale operands of one family (H = 2, dilation 1, with an RPE table)."""
    H, dil = rc.ATT_H, 1
    oplan, plan = plans(K, dil)
    nt, W = plan.n_tokens[depth], plan.n_windows[depth]
    g = torch.Generator().manual_seed(5000 + K + depth)
    C = H * 16
    bnd = int(0.8 * K * dil ** 0.5)
    return dict(K=K, G=G, depth=depth, H=H, C=C, oplan=oplan, plan=plan, nt=nt, W=W, real=-(-nt // K),
                tok=torch.randn(nt, 3 * C, generator=g), rt=torch.randn(W, 3 * C, generator=g),
                table=torch.randn(3 * (2 * bnd + 1), H, generator=g) * 0.5)


def _scaled(t, C, sq, sk, sv):
    out = t.clone()
    out[:, :C] = rc.pow2(t[:, :C], sq)
    out[:, C:2 * C] = rc.pow2(t[:, C:2 * C], sk)
    out[:, 2 * C:] = rc.pow2(t[:, 2 * C:], sv)
    return out


def _run_window(case, x, f16):
    c = case
    src = pack_qkv_f16(x, c['H'], 0.25 * rc.LOG2E) if f16 else x
    return ops.window_attention(src.to(DEV), c['plan'].meta[c['depth']], c['table'].to(DEV), c['nt'], c['W'], c['K'], 1, c['G'],
                                c['H'], 3, rt_row0=c['nt'], depth=c['depth'], qkv_f16=f16).cpu()


def _dev_rows(case, got):
    """The rows a launch owns: the tokens, and the relay rows of the windows that hold a token."""
    c = case
    return torch.cat([got[:c['nt']], got[c['nt']:c['nt'] + c['real']]]) if c['G'] else got[:c['nt']]


def _ref_rows(case, tok, rt):
    """float64 reference of the same rows."""
    c = case
    want, want_tok = windows_ref(c['oplan'], tok.double(), rt.double(), c['table'].double(), c['depth'], c['K'], c['G'], 1, c['H'])
    return torch.cat([want_tok, want[:c['real'], 0]]) if c['G'] else want_tok


@pytest.mark.parametrize('K,G,depth', rc.ATT_FAMILIES)
def test_window_attention_across_operand_scales(K, G, depth):
    """fp32 operands: |o - ref| <= 2^-20 v_max per element at every scale, and bitwise equivariant in the scale of v.
    fp16 (hi, lo) operands: |o - ref| <= 2 E32 + e_h(v_max) + 2 d_s v_max with d_s = 16 (q_max e_h(k_max) + k_max e_h(q_max))
    (q as the kernel holds it, softmax scale and log2 e folded in) and E32 the fp32-operand kernel's own largest error on the
    same input.  (s_q, s_k) = (2^4, 2^-4) and its mirror leave the logits unchanged mathematically -- and the float64 reference
    bit for bit up to the power of two in v, so it is computed once."""
    case = _attention_case(K, G, depth)
    C, H = case['C'], case['H']
    assert ops.window_attention_f16_ok(case['nt'] + case['W'], K, 1, G, H, depth)
    ref_unit = _ref_rows(case, case['tok'], case['rt'])
    assert torch.isfinite(ref_unit).all()
    unit = {}
    for (sq, sk), sv in itertools.product(rc.ATT_SQK, (0,) + tuple(s for s in rc.ATT_SV if s != 0)):
        x = torch.cat([_scaled(case['tok'], C, sq, sk, sv), _scaled(case['rt'], C, sq, sk, sv)])
        ref = rc.pow2(ref_unit, sv)
        v_max = float(x[:, 2 * C:].abs().max())
        q_max = float(x[:, :C].abs().max()) * 0.25 * rc.LOG2E
        k_max = float(x[:, C:2 * C].abs().max())
        o32 = _dev_rows(case, _run_window(case, x, False))
        assert torch.isfinite(o32).all()
        e32 = float((o32.double() - ref).abs().max())
        o16 = _dev_rows(case, _run_window(case, x, True))
        e16 = float((o16.double() - ref).abs().max())
        bound16 = 2 * e32 + float(rc.e_h(v_max)) + 2 * rc.logit_bound(q_max, k_max) * v_max
        print('window K %d G %d  s_q 2^%d s_k 2^%d s_v 2^%d: f32 %.3g (bound %.3g)  f16 %.3g (bound %.3g)'
              % (K, G, sq, sk, sv, e32, rc.ATT_F32_BOUND * v_max, e16, bound16))
        assert e32 <= rc.ATT_F32_BOUND * v_max, (sq, sk, sv, e32, v_max)
        assert torch.isfinite(o16).all() and e16 <= bound16, (sq, sk, sv, e16, bound16)
        if sv == 0:
            unit[(sq, sk)] = o32
        else:
            assert _same(o32, rc.pow2(unit[(sq, sk)], sv)), (sq, sk, sv)             # bitwise equivariance in s_v



def test_relay_attention_f16_across_operand_scales():
    """relay_attention_f16 under the same bound, E32 from relay_attention (fp32 operands) on the same input; that kernel is
    itself held to 2^-20 v_max per element."""
    H, n_rows = rc.ATT_H, 600
    lengths = [1, 15, 16, 17, 63, 64, 65, 0, 250]
    C, B = H * 16, len(lengths)
    seq_rows, seq_off, orphans = sequence_table(lengths, n_rows, 77 + H)
    g = torch.Generator().manual_seed(5100)
    base = torch.randn(n_rows, 3 * C, generator=g)
    rows_d, off_d, orph_d = (torch.from_numpy(t).to(DEV) for t in (seq_rows, seq_off, orphans))
    used = torch.from_numpy(seq_rows.astype(np.int64))
    for (sq, sk), sv in itertools.product(rc.ATT_SQK, rc.ATT_SV):
        x = _scaled(base, C, sq, sk, sv)
        ref = relay_ref(x.double(), seq_rows, seq_off, H)[used]
        assert torch.isfinite(ref).all()
        v_max = float(x[used][:, 2 * C:].abs().max())
        q_max = float(x[used][:, :C].abs().max()) * 0.25 * rc.LOG2E
        k_max = float(x[used][:, C:2 * C].abs().max())
        o32 = ops.relay_attention(x.to(DEV), rows_d, off_d, B, H, max(lengths)).cpu()[used]
        e32 = float((o32.double() - ref).abs().max())
        o16 = ops.relay_attention_f16(pack_qkv_f16(x, H, 0.25 * rc.LOG2E).to(DEV), rows_d, off_d, B, H, max(lengths), orph_d)
        val = _unsplit2(o16, C)[used]
        e16 = float((val - ref).abs().max())
        bound16 = 2 * e32 + float(rc.e_h(v_max)) + 2 * rc.logit_bound(q_max, k_max) * v_max + 2.0 ** -17 * v_max
        print('relay s_q 2^%d s_k 2^%d s_v 2^%d: f32 %.3g (bound %.3g)  f16 %.3g (bound %.3g)'
              % (sq, sk, sv, e32, rc.ATT_F32_BOUND * v_max, e16, bound16))
        assert e32 <= rc.ATT_F32_BOUND * v_max, (sq, sk, sv, e32)
        assert torch.isfinite(val).all() and e16 <= bound16, (sq, sk, sv, e16, bound16)


# ------------------------------------------------------------------------------------------------------------ 7. non-finite
POISON = (float('nan'), float('inf'))


def _poison_check(clean, got, ref, what):
    """Every element the float64 reference makes non-finite is non-finite; every other one is bit-equal to the clean run."""
    bad = ~torch.isfinite(ref)
    assert bad.any() and not bad.all(), what
    assert not torch.isfinite(got[bad]).any(), (what, 'a non-finite value vanished')
    assert torch.equal(_bits(got)[~bad], _bits(clean)[~bad]), (what, 'a clean element changed')


@pytest.mark.parametrize('poison', POISON, ids=['nan', 'inf'])
def test_non_finite_inputs_do_not_vanish_in_the_linears_and_layer_norm(poison):
    for m, (k, n) in ((127, (96, 384)), (129, (32, 128))):
        x, w, b, r = rc.gemm_case(m, k, n, 1000 + m + k + n)
        xp = x.clone()
        xp[m // 2, k - 5] = poison
        ref = xp.double() @ w.double().t() + b.double() + r.double()
        wd, bd, rd = w.to(DEV), b.to(DEV), r.to(DEV)
        w2, w6 = ops.split2_weight(wd), ops.x6_pack(wd)
        run3 = lambda t: ops.linear_x3(ops.split2(t.to(DEV)), w2, bias=bd, residual=rd).cpu()
        run6 = lambda t: ops.linear_x6(t.to(DEV), w6, bias=bd, residual=rd).cpu()
        _poison_check(run3(x), run3(xp), ref, ('linear_x3', m, k, n))
        _poison_check(run6(x), run6(xp), ref, ('linear_x6', m, k, n))
    for i, (rows, c) in enumerate(rc.LN_SHAPES):
        x, _ = rc.ln_rows(rows, c, 40 + i)
        gamma, beta = rc.ln_params(c, 50 + i)
        xp = x.clone()
        xp[rows // 2, c - 3] = poison
        gd, bd = gamma.to(DEV), beta.to(DEV)
        ref = rc.ln64(xp, gamma, beta)
        run = lambda t: ops.layer_norm(t.to(DEV), gd, bd, rc.LN_EPS).cpu()
        _poison_check(run(x), run(xp), ref, ('layer_norm', rows, c))
        hid = 4 * c
        w1, w2 = rc.real_values((hid, c), 70 + i, 0.05).to(DEV), rc.real_values((c, hid), 71 + i, 0.05).to(DEV)
        b1, b2 = rc.real_values((hid,), 72 + i, 0.1).to(DEV), rc.real_values((c,), 73 + i, 0.1).to(DEV)
        pack = ops.mlp_fused_pack(w1, w2)
        runm = lambda t: ops.ln_mlp_fused(t.to(DEV), gd, bd, rc.LN_EPS, pack, b1, b2).cpu()
        # x + fc2(gelu(fc1(LN(x)))): non-finite exactly in the rows where LN(x) is
        _poison_check(runm(x), runm(xp), ref[:, :1] + x.double(), ('ln_mlp_fused', rows, c))


@pytest.mark.parametrize('poison', POISON, ids=['nan', 'inf'])
@pytest.mark.parametrize('K,G,depth', rc.ATT_FAMILIES)
def test_non_finite_inputs_do_not_vanish_in_window_attention(K, G, depth, poison):
    """One poisoned q element (its query row, that head), then one poisoned v element (every query of its window, that head),
    through both operand forms of window_attention."""
    case = _attention_case(K, G, depth)
    C = case['C']
    x = torch.cat([case['tok'], case['rt']])
    clean = {f16: _dev_rows(case, _run_window(case, x, f16)) for f16 in (False, True)}
    for column in (3, 2 * C + 16 + 5):                                    # q of head 0, v of head 1
        tok = case['tok'].clone()
        tok[case['nt'] // 2, column] = poison
        ref = _ref_rows(case, tok, case['rt'])
        xp = torch.cat([tok, case['rt']])
        for f16 in (False, True):
            got = _dev_rows(case, _run_window(case, xp, f16))
            _poison_check(clean[f16], got, ref, ('window_attention', K, G, 'f16' if f16 else 'f32', column))
