"""CPU proofs under tests/test_gpu_dynamic_range.py: the numpy models of the bf16 (RNE) and fp16 (RTZ) operand splits meet the
bounds the device tests hold the kernels to, those bounds are not slack, every input / product / K-sum of the device tests stays
inside [2^-100, 2^100] (no fp32 underflow or overflow can excuse a device mismatch), the GELU sweep is exact in a bf16 pair, and
the float64 references are finite wherever a device test demands a finite result."""

import itertools

import numpy as np
import torch

import range_cases as rc


def _all_split_values():
    for i, (rows, c) in enumerate(rc.SPLIT_SHAPES):
        yield rc.split_values(rows, c, 100 + i).numpy()


def test_split_inputs_cover_the_exponent_sweep_inside_the_range():
    seen = set()
    for v in _all_split_values():
        assert rc.in_range(torch.from_numpy(v))
        assert (v != 0).all()
        e = np.floor(np.log2(np.abs(v.astype(np.float64)))).astype(np.int64)
        seen |= set(e.ravel().tolist())
        # every value carries a full 24-bit significand (top bit of m set, the low bits random): some low bit is set somewhere
        assert (v.view(np.uint32) & 0xFF).any()
    want = {e if e < 0 else e - 1 for e in rc.SPLIT_EXPONENTS}
    assert want <= seen, sorted(want - seen)


def test_bf16_model_is_round_to_nearest_even_and_meets_e_bf():
    """The model against torch's own fp32 -> bf16 conversion (an independent implementation of RNE), the pair against
    e_bf = 2^-17 |v|, the triple exact; and the bound is not slack: some value uses more than a quarter of it."""
    worst = 0.0
    for v in _all_split_values():
        t = torch.from_numpy(v)
        assert np.array_equal(rc.bf16_rne_bits(v), t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
        hi, lo = rc.split_bf16(v)
        err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - v.astype(np.float64))
        assert (err <= rc.e_bf(v)).all()
        worst = max(worst, float((err / rc.e_bf(v)).max()))
        assert (np.abs(lo) <= np.abs(hi) * 2.0 ** -8).all()
        h, m, l = rc.split3_bf16(v)
        assert np.array_equal(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64), v.astype(np.float64))
    assert worst > 0.25, worst
    # ties go to the even neighbour, both ways
    ties = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8)], dtype=np.float32)
    assert rc.bf16_value(rc.bf16_rne_bits(ties)).tolist() == [1.0, 1.0 + 2.0 ** -6, -1.0]


def _image_at(s):
    return np.ldexp(rc.image_values(rc.IMAGE_ROWS, rc.IMAGE_C, 500).numpy().astype(np.float64), s).astype(np.float32)


def test_fp16_model_rounds_toward_zero_and_meets_e_h():
    """hi never exceeds |v| and is within one fp16 spacing of it; the pair meets e_h = max(2^-20 |v|, 2^-24) at every scale of
    the operand-image test, and touches the 2^-24 floor where lo is subnormal: a floor of 2^-14 would be 1000 times slack."""
    floor_use = 0.0
    rel_use = 0.0
    for s in rc.F16_SCALES:
        v = _image_at(s)
        assert float(np.abs(v).max()) < rc.F16_MAX
        hi, lo = rc.split_fp16(v)
        h64, v64 = hi.astype(np.float64), v.astype(np.float64)
        assert np.isfinite(h64).all()
        assert (np.abs(h64) <= np.abs(v64)).all() and (np.sign(h64) * np.sign(v64) >= 0).all()
        spacing = np.maximum(np.exp2(np.floor(np.log2(np.maximum(np.abs(v64), 2.0 ** -14))) - 10), 2.0 ** -24)
        assert (np.abs(v64 - h64) < spacing).all()
        err = np.abs(h64 + lo.astype(np.float64) - v64)
        bound = rc.e_h(v)
        assert (err <= bound).all(), s
        small = bound == rc.E_H_FLOOR
        if small.any():
            floor_use = max(floor_use, float((err[small] / rc.E_H_FLOOR).max()))
        if (~small).any():
            rel_use = max(rel_use, float((err[~small] / bound[~small]).max()))
    assert rc.e_h(0.0) == 2.0 ** -24 and rc.e_h(1.0) == 2.0 ** -20
    assert floor_use > 0.5, floor_use                     # the fixed-point regime really costs up to one quantum
    assert rel_use > 0.25, rel_use
    # the exact boundary cases of the format
    edge = np.array([65503.9, 2.0 ** -24, 2.0 ** -25, -2.0 ** -14 - 2.0 ** -26, 1.0 + 2.0 ** -11 + 2.0 ** -23], dtype=np.float32)
    hi, lo = rc.split_fp16(edge)
    assert hi.astype(np.float64).tolist() == [65472.0, 2.0 ** -24, 0.0, -2.0 ** -14, 1.0]
    assert lo.astype(np.float64).tolist()[2:] == [0.0, 0.0, 2.0 ** -11]


def _check_products(x, w, e_total):
    """Smallest product and largest sum of magnitudes of x @ w^T, times 2^e_total."""
    ax, aw = x.double().abs(), w.double().abs()
    lo = float(ax.min() * aw.min()) * 2.0 ** e_total
    hi = float((ax @ aw.t()).max()) * 2.0 ** e_total
    assert rc.RANGE_LO <= lo * 2.0 ** -18 and hi <= rc.RANGE_HI, (lo, hi, e_total)     # 2^-18: the lo x hi plane products


def test_gemm_inputs_products_and_sums_stay_in_range():
    for (k, n), m in itertools.product(rc.GEMM_KN, rc.GEMM_M):
        x, w, b, r = rc.gemm_case(m, k, n, 1000 + m + k + n)
        for t in (x, w, b, r):
            assert float(t.abs().min()) >= rc.MAG_LO and float(t.abs().max()) <= rc.MAG_HI
        for a, bb in itertools.product(rc.SCALES_A, rc.SCALES_B):
            assert rc.in_range(rc.pow2(x, a)) and rc.in_range(rc.pow2(w, bb))
            assert rc.in_range(rc.pow2(b, a + bb)) and rc.in_range(rc.pow2(r, a + bb))
            _check_products(x, w, a + bb)
        ak = rc.column_exponents(k, 7 + k)
        assert int(ak.abs().max()) <= rc.COLUMN_SHIFT and len(set(ak.tolist())) > 8
        assert rc.in_range(torch.ldexp(x, ak)) and rc.in_range(torch.ldexp(w, -ak))
        for a in rc.ERR_SCALES:
            _check_products(x, w, 2 * a)
    for (n, k), m in itertools.product(rc.WGRAD_NK, rc.WGRAD_M):
        dy, x = rc.real_values((m, n), 2000 + m + n), rc.real_values((m, k), 2001 + m + k)
        for a, bb in itertools.product(rc.SCALES_A, rc.SCALES_B):
            _check_products(dy.t(), x.t(), a + bb)
            assert float(dy.double().abs().sum(0).max()) * 2.0 ** a <= rc.RANGE_HI
    for cin, cout in rc.GROUP_KN:
        rows = sum(rc.GROUP_SIZES)
        x = rc.real_values((rows, cin), 3000 + cin)
        w = rc.real_values((len(rc.GROUP_SIZES) * cout, cin), 3001 + cin, 0.25)
        for a, bb in itertools.product(rc.SCALES_A, rc.SCALES_B):
            _check_products(x, w, a + bb)


def test_gelu_sweep_is_exact_in_a_bf16_pair():
    v = rc.gelu_sweep().numpy()
    assert v.size == 2 * (1 << 15) - 1 + 6
    hi, lo = rc.split_bf16(v)
    assert np.array_equal((hi + lo).view(np.uint32)[v != 0], v.view(np.uint32)[v != 0])       # fp32 add of the halves: exact
    assert np.array_equal(hi.astype(np.float64) + lo.astype(np.float64), v.astype(np.float64))
    # 16 significant bits: the significand's low 8 bits are zero
    assert not (v.view(np.uint32) & 0xFF).any()
    assert {0.0, 2.0 ** -20, 300.0, -300.0, 255.9921875} <= set(v.tolist()) and np.signbit(v[v == 0]).any()
    r = rc.gelu_random().numpy()
    assert np.abs(r).max() <= 12.0 and (r.view(np.uint32) & 0xFF).any()
    h, m, l = rc.split3_bf16(r)
    assert np.array_equal(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64), r.astype(np.float64))
    g = rc.gelu64(torch.from_numpy(np.concatenate([v, r])))
    d = rc.gelu_grad64(torch.from_numpy(np.concatenate([v, r])))
    assert torch.isfinite(g).all() and torch.isfinite(d).all() and float(g.min()) > -0.17 and float(d.min()) > -0.13


def test_layer_norm_rows_and_references_are_finite():
    for i, (rows, c) in enumerate(rc.LN_SHAPES):
        x, kinds = rc.ln_rows(rows, c, 40 + i)
        assert set(kinds) == {'mean0', 'mean8', 'mean14', 'up30', 'down30', 'const', 'unit', 'outlier'}
        assert torch.isfinite(x).all() and rc.in_range(x)
        assert rc.in_range((x.double() ** 2).sum(1))                      # the variance sums
        gamma, beta = rc.ln_params(c, 50 + i)
        y = rc.ln64(x, gamma, beta)
        assert torch.isfinite(y).all()
        for r, kind in enumerate(kinds):
            if kind == 'const':
                assert float(x[r].min()) == float(x[r].max())
                assert torch.equal(y[r], beta.double())                   # variance 0: eps decides, the output is beta
            if kind == 'outlier':
                top = x[r].abs().topk(2).values
                assert float(top[0] / top[1]) > 2.0 ** 17
        # every partial sum of a constant row is exact in fp32 whatever the order: C * value has few significant bits
        for cst in rc.LN_CONSTANTS:
            assert float(np.float32(cst)) == cst and float(np.float32(cst * 7)) == cst * 7


def test_attention_scales_keep_the_fp16_operands_in_range():
    """The clouds' qkv rows times the scales of the attention test: q (with the softmax scale and log2 e folded in), k and v
    below 65504, and the float64 reference finite (its rows are what the device rows must match)."""
    g = torch.Generator().manual_seed(4000)
    qkv = torch.randn(2000, 3 * rc.ATT_H * 16, generator=g)
    top = float(qkv.abs().max())
    for sq, sk in rc.ATT_SQK:
        assert top * 2.0 ** sq * 0.25 * rc.LOG2E < rc.F16_MAX and top * 2.0 ** sk < rc.F16_MAX
        assert sq + sk == 0                                               # the logits do not change
    for sv in rc.ATT_SV:
        assert top * 2.0 ** sv < rc.F16_MAX
    assert rc.logit_bound(1.0, 1.0) == 16 * 2 * 2.0 ** -20
    assert rc.logit_bound(2.0 ** -20, 1.0) == 16 * (2.0 ** -20 * 2.0 ** -20 + 2.0 ** -24)     # the floor of the small operand
