"""`hfl_smoothap_rows` and `hfl_kd_rows` (csrc/loss.hip) element by element against float64, through their checked wrappers
`ops.smoothap_rows` / `ops.kd_rows`.  Cases, references and the yardstick are tests/loss_kernel_cases.py, proven on the CPU by
tests/test_loss_kernel_host.py.

Bars ("Numeric range contract"): per row `2 E32 + 2^-22 scale`, E32 the largest error over the row of the same
formula in float32 torch on the device, `scale` 1 for an AP, sum_j sum_z |d AP / d e_jz| / tau for a row of d AP / d S,
sum_j q_j (|log q_j| + |log p_j|) for a KL and max_j (p_j + q_j) / T for a row of d KL / d y; E32 alone for the close-rows cases
of the distillation kernel.  Every test prints its worst use of the bars before it asserts; DESIGN.md section 6b has the table."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import loss_kernel_cases as lk                                         # noqa: E402
from hotformerloc_amd import _native, losses, ops                      # noqa: E402
from hotformerloc_amd._native import NativeLibraryError                # noqa: E402
from oracle.gen_golden_loss import make_case                           # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')


def _dev(case):
    return lk.SmoothAPCase(*(t.to(DEV) for t in case[:4]), case.tau)


# ================================================================================================ SmoothAP
def _smoothap(case):
    """one launch into NaN-filled outputs: every entry written and finite, a second launch gives the same bits"""
    B = case.S.shape[0]
    ap = torch.full((B,), NAN, dtype=torch.float32, device=DEV)
    dap = torch.full((B, B), NAN, dtype=torch.float32, device=DEV)
    out = ops.smoothap_rows(case.S, case.pos, case.neg, case.idx, case.tau, out=(ap, dap))
    assert out[0] is ap and out[1] is dap
    assert bool(torch.isfinite(ap).all()) and bool(torch.isfinite(dap).all()), 'an entry was not written, or is not finite'
    ap2, dap2 = ops.smoothap_rows(case.S, case.pos, case.neg, case.idx, case.tau)
    assert torch.equal(ap, ap2) and torch.equal(dap, dap2), 'two calls on the same input must agree bit for bit'
    assert 0.0 <= ap.min().item() and ap.max().item() <= 1.0
    return ap, dap


def _smoothap_bars(sub):
    r64 = lk.smoothap_ref(*sub)
    r32 = lk.smoothap_ref(*sub, dtype=torch.float32)
    bar_ap = lk.row_bars((r32.ap.double() - r64.ap).abs(), torch.ones_like(r64.ap))
    bar_g = lk.row_bars((r32.grad.double() - r64.grad).abs().amax(1), r64.scale)
    return r64, bar_ap, bar_g


def _smoothap_check(label, case, rows=None):
    """kernel on the whole batch; float64 on `rows` of it (all rows by default).  Returns the worst uses of the bars."""
    ap, dap = _smoothap(case)
    sub = case if rows is None else lk.SmoothAPCase(*(t[rows.to(DEV)] for t in case[:4]), case.tau)
    got_ap, got_g = (ap, dap) if rows is None else (ap[rows.to(DEV)], dap[rows.to(DEV)])
    r64, bar_ap, bar_g = _smoothap_bars(sub)
    use = (lk.bar_use((got_ap.double() - r64.ap).abs(), bar_ap),
           lk.bar_use((got_g.double() - r64.grad).abs().amax(1), bar_g),
           lk.bar_use(got_g.double().sum(1).abs(), bar_g))
    print('smoothap %-28s worst use of the bar: ap %.3f  dap_ds %.3f  row sum %.3f   (bars: ap %.2e..%.2e, dap_ds %.2e..%.2e)'
          % (label, use[0], use[1], use[2], bar_ap.min(), bar_ap.max(), bar_g.min(), bar_g.max()))
    return use, ap, dap


@pytest.mark.parametrize('B', lk.SIZES_B)
def test_smoothap_sizes(B):
    """Below, at and above the wavefront and the workgroup (idle waves in `block_sum`, one and several elements per thread),
    P up to more than B - 1.  Measured on MI355X, worst use of the bars over the ten sizes: ap 0.33, dap_ds 0.92 (B = 64,
    P = 1; a row with one or two live terms), row sum 0.54.  Before the derivative was formed as
    a^2 e^x the gradient missed by 11441 x at B = 63."""
    worst = [max(_smoothap_check('B=%d P=%d' % (B, P), _dev(lk.smoothap_random(B, P)))[0]) for P in lk.SIZES_P]
    assert max(worst) <= 1.0


@pytest.mark.parametrize('tau', lk.TAUS)
def test_smoothap_temperatures(tau):
    use, _, _ = _smoothap_check('tau=%g' % tau, _dev(lk.smoothap_random(257, 4, tau)))
    assert max(use) <= 1.0


def test_smoothap_mask_families():
    cpu = lk.smoothap_families()
    case = _dev(cpu)
    use, ap, dap = _smoothap_check('mask families', case)
    R = lk.FAMILY_ROWS
    assert ap[R['no_neg']].item() == 1.0 and not dap[R['no_neg']].any(), 'no negatives: AP exactly 1, gradient row exactly 0'
    assert ap[R['no_pos']].item() == 0.0 and not dap[R['no_pos']].any(), 'no valid slot: AP 0 and a zero gradient row'
    # per family row, against float64 (the batch-wide figure above hides which family is the worst)
    r64, bar_ap, bar_g = _smoothap_bars(case)
    for name, q in R.items():
        ua = lk.bar_use((ap[q:q + 1].double() - r64.ap[q:q + 1]).abs(), bar_ap[q:q + 1])
        ug = lk.bar_use((dap[q:q + 1].double() - r64.grad[q:q + 1]).abs().amax(1), bar_g[q:q + 1])
        print('   row %-12s ap %.9g (float64 %.9g)  use: ap %.3f dap_ds %.3f' % (name, ap[q], r64.ap[q], ua, ug))
    # one workgroup owns a row: the rest of the batch must not matter
    for name, q in R.items():
        ap1, dap1 = _smoothap(_dev(lk.alone(cpu, q)))
        assert torch.equal(ap1[q], ap[q]) and torch.equal(dap1[q], dap[q]), name
        ap1[q] = 0.0
        dap1[q] = 0.0
        assert not ap1.any() and not dap1.any(), 'an emptied row has AP 0 and a zero gradient row'
    assert max(use) <= 1.0


def test_smoothap_clamped_exponents():
    case, _ = lk.smoothap_clamp()
    use, _, _ = _smoothap_check('clamp tau=2^-6 |S|<=1.6e4', _dev(case))
    assert max(use) <= 1.0


def test_smoothap_equal_similarities():
    case, _ = lk.smoothap_ties()
    use, _, _ = _smoothap_check('100 ties', _dev(case))
    assert max(use) <= 1.0


@pytest.mark.parametrize('B,P', lk.LDS_SIZES)
def test_smoothap_lds_edges(B, P):
    """9 B bytes of dynamic LDS: 49149 (below 48 KiB, no attribute call), 49158 and 65538 (the hipFuncSetAttribute branch),
    153594 (the largest accepted size).  64 hash-chosen rows against float64, every row written and finite."""
    case = lk.smoothap_lds(B, P, device=DEV)
    use, _, _ = _smoothap_check('LDS %d bytes (B=%d P=%d)' % (9 * B, B, P), case, rows=lk.sample_rows(B))
    assert max(use) <= 1.0


def test_smoothap_capacity_refusal():
    """B = 17067 needs 153603 bytes: refused with HFL_ECAPACITY before any launch.  Every buffer has its full size."""
    B = lk.CAPACITY + 1
    S = torch.zeros((B, B), dtype=torch.float32, device=DEV)
    pos = torch.zeros((B, B), dtype=torch.uint8, device=DEV)
    neg = torch.zeros((B, B), dtype=torch.uint8, device=DEV)
    idx = torch.zeros((B, 1), dtype=torch.int64, device=DEV)
    ap = torch.full((B,), NAN, dtype=torch.float32, device=DEV)
    dap = torch.full((B, B), NAN, dtype=torch.float32, device=DEV)
    with pytest.raises(NativeLibraryError, match='HFL_ECAPACITY'):
        ops.smoothap_rows(S, pos, neg, idx, lk.TAU, out=(ap, dap))
    torch.cuda.synchronize()
    assert bool(torch.isnan(ap).all()) and bool(torch.isnan(dap).all()), 'nothing may be launched'


def _miss(wrong, r64, bar_ap, bar_g, rows=slice(None)):
    """by how many bars a wrong float64 formula misses: (ap, gradient), the worst row"""
    ea, eg = (wrong.ap - r64.ap).abs()[rows], (wrong.grad - r64.grad).abs().amax(1)[rows]
    ba, bg = bar_ap[rows], bar_g[rows]
    return float((ea / ba).max()), float((eg[bg > 0] / bg[bg > 0]).max())


def test_smoothap_negative_controls():
    """Wrong formulas on the float64 side only (no broken kernel is built): each misses the bars of its case by 10 x or more,
    so the cases can see these mistakes."""
    case = _dev(lk.smoothap_random(257, 4))
    r64, bar_ap, bar_g = _smoothap_bars(case)
    for variant in ('keep_self', 'neg_in_rp'):
        ma, mg = _miss(lk.smoothap_ref(*case, variant=variant), r64, bar_ap, bar_g)
        print('control %-10s misses the bars by %.3g x (ap) %.3g x (dap_ds)' % (variant, ma, mg))
        assert ma >= 10 and mg >= 10
    case = _dev(lk.smoothap_families())
    r64, bar_ap, bar_g = _smoothap_bars(case)
    few = [lk.FAMILY_ROWS[n] for n in lk.FEW_ROWS]
    wrong = lk.smoothap_ref(*case, variant='over_p')
    for q in few:
        ma, mg = _miss(wrong, r64, bar_ap, bar_g, slice(q, q + 1))
        print('control over_p   row %d misses the bars by %.3g x (ap) %.3g x (dap_ds)' % (q, ma, mg))
        assert ma >= 10 and mg >= 10


def test_smoothap_wrapper_refusals():
    """every argument error raises before any launch: the NaN-filled outputs stay NaN"""
    B, P = 8, 2
    c = _dev(lk.smoothap_random(B, P))
    ap = torch.full((B,), NAN, dtype=torch.float32, device=DEV)
    dap = torch.full((B, B), NAN, dtype=torch.float32, device=DEV)
    wide = torch.zeros((B, 2 * B), dtype=torch.float32, device=DEV)
    wide_u8 = torch.zeros((B, 2 * B), dtype=torch.uint8, device=DEV)
    wide_idx = torch.zeros((B, 2 * P), dtype=torch.int64, device=DEV)
    bad = [
        (TypeError, dict(sim=c.S.double())),
        (TypeError, dict(sim=c.S.half())),
        (ValueError, dict(sim=c.S[:, :B - 1].contiguous())),
        (ValueError, dict(sim=c.S.reshape(B, B, 1))),
        (ValueError, dict(sim=c.S.flatten())),
        (ValueError, dict(sim=wide[:, ::2])),                        # (B, B), not contiguous
        (ValueError, dict(sim=c.S.t())),
        (TypeError, dict(pos_u8=c.pos.bool())),
        (TypeError, dict(neg_u8=c.neg.to(torch.int8))),
        (ValueError, dict(pos_u8=c.pos[:B - 1].contiguous())),       # a mask of another shape
        (ValueError, dict(neg_u8=torch.zeros((B, B + 1), dtype=torch.uint8, device=DEV))),
        (ValueError, dict(pos_u8=wide_u8[:, ::2])),
        (ValueError, dict(neg_u8=wide_u8[:, ::2])),
        (TypeError, dict(idx=c.idx.int())),
        (ValueError, dict(idx=c.idx[:, :0])),                        # P = 0
        (ValueError, dict(idx=c.idx[:B - 1].contiguous())),
        (ValueError, dict(idx=c.idx[:, 0].contiguous())),
        (ValueError, dict(idx=wide_idx[:, ::2])),
        (ValueError, dict(idx=c.idx.cpu())),                         # operands on different devices
        (ValueError, dict(pos_u8=c.pos.cpu())),
        (ValueError, dict(tau=0.0)),
        (ValueError, dict(tau=-0.01)),
        (ValueError, dict(tau=NAN)),
        (ValueError, dict(out=(ap[:B - 1], dap))),
        (ValueError, dict(out=(ap, dap.double()))),
    ]
    for exc, change in bad:
        kw = dict(sim=c.S, pos_u8=c.pos, neg_u8=c.neg, idx=c.idx, tau=c.tau, out=(ap, dap))
        kw.update(change)
        with pytest.raises(exc):
            ops.smoothap_rows(**kw)
    with pytest.raises(NativeLibraryError):                          # no CPU fallback
        ops.smoothap_rows(c.S.cpu(), c.pos.cpu(), c.neg.cpu(), c.idx.cpu(), c.tau)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ap).all()) and bool(torch.isnan(dap).all())
    got = ops.smoothap_rows(c.S, c.pos, c.neg, c.idx, c.tau, out=(ap, dap))      # and the valid call goes through
    assert got[0] is ap and bool(torch.isfinite(ap).all()) and bool(torch.isfinite(dap).all())


class _RowsThroughTheCAbi(torch.autograd.Function):
    """`losses._SmoothAPRows` as it was before `ops.smoothap_rows` existed: raw pointers to the C ABI"""
    @staticmethod
    def forward(ctx, sim, pos_u8, neg_u8, idx, tau):
        b = sim.shape[0]
        ap = torch.empty(b, dtype=torch.float32, device=sim.device)
        dap = torch.empty((b, b), dtype=torch.float32, device=sim.device)
        _native.check(_native.load().hfl_smoothap_rows(ap.data_ptr(), dap.data_ptr(), sim.data_ptr(), pos_u8.data_ptr(),
                                                       neg_u8.data_ptr(), idx.data_ptr(), b, idx.shape[1], float(tau),
                                                       ops._stream()), 'hfl_smoothap_rows')
        ctx.save_for_backward(dap)
        return ap

    @staticmethod
    def backward(ctx, grad_ap):
        (dap,) = ctx.saved_tensors
        return dap * grad_ap[:, None], None, None, None, None


def test_module_through_the_wrapper_is_bitwise_the_module_before(golden_dir, monkeypatch):
    g = np.load(os.path.join(golden_dir, 'loss_smoothap.npz'))
    seed, batch, dim, group, drop, ppq = [int(v) for v in g['b48_few_pos.cfg']]
    e, pos, neg = make_case(seed, batch, dim, group, drop)

    def run():
        emb = torch.from_numpy(e).to(DEV).requires_grad_()
        loss, _ = losses.TruncatedSmoothAP(tau1=0.01, positives_per_query=ppq)(emb, torch.from_numpy(pos), torch.from_numpy(neg))
        loss.backward()
        return loss.detach(), emb.grad

    new1, new2 = run(), run()
    monkeypatch.setattr(losses, '_SmoothAPRows', _RowsThroughTheCAbi)
    old = run()
    for a, b in ((new1, new2), (new1, old)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert abs(new1[0].item() - float(g['b48_few_pos.loss'])) < 2e-6


# ================================================================================================ KD
def _kd(y, t, T):
    kl, g = ops.kd_rows(y, t, T)
    kl2, g2 = ops.kd_rows(y, t, T)
    assert torch.equal(kl, kl2) and torch.equal(g, g2), 'two calls on the same input must agree bit for bit'
    assert bool(torch.isfinite(kl).all()) and bool(torch.isfinite(g).all())
    return kl, g


def _kd_bars(y, t, T, close=False):
    r64, r32 = lk.kd_ref(y, t, T), lk.kd_ref(y, t, T, torch.float32)
    bar_kl = lk.row_bars((r32.kl.double() - r64.kl).abs(), r64.kl_scale, close)
    bar_g = lk.row_bars((r32.grad.double() - r64.grad).abs().amax(1), r64.grad_scale, close)
    # The sum of a gradient row is (sum_j p_j - sum_j q_j) / T: D terms whose magnitudes add up to 2 / T, each normalised
    # with a reciprocal that is itself rounded (2^-24 of the whole sum).  The bar of ONE entry, 2^-22 max_j (p_j + q_j) / T,
    # is about 3 / D of that and below what one rounding of 1 / Z leaves; so the sum has the bar of
    # the convention applied to the sum itself.  The close rows keep the entry's bar: there every entry is q_j expm1(.)
    # and the sum inherits errors in proportion to |p_j - q_j| only.
    bar_sum = bar_g if close else lk.row_bars(r32.grad.double().sum(1).abs(), r64.sum_scale)
    return r64, bar_kl, bar_g, bar_sum


def _kd_check(label, y, t, T, close=False, reference_rows=None):
    """kernel on (y, t); float64 and the bars on `reference_rows` (another pair with the same exact result) or on (y, t)"""
    y, t = y.to(DEV), t.to(DEV)
    kl, g = _kd(y, t, T)
    ry, rt = (y, t) if reference_rows is None else (v.to(DEV) for v in reference_rows)
    r64, bar_kl, bar_g, bar_sum = _kd_bars(ry, rt, T, close)
    use = (lk.bar_use((kl.double() - r64.kl).abs(), bar_kl),
           lk.bar_use((g.double() - r64.grad).abs().amax(1), bar_g),
           lk.bar_use(g.double().sum(1).abs(), bar_sum),
           lk.bar_use((-kl.double()).clamp(min=0), bar_kl))
    print('kd %-34s worst use of the bar: kl %.3f  dkl_dy %.3f  row sum %.3f (%.3f of an entry\'s bar)  -kl %.3f   '
          '(bars: kl %.2e..%.2e, dkl_dy %.2e..%.2e)'
          % (label, use[0], use[1], use[2], lk.bar_use(g.double().sum(1).abs(), bar_g), use[3], bar_kl.min(), bar_kl.max(),
             bar_g.min(), bar_g.max()))
    return use, kl, g


@pytest.mark.parametrize('dim', lk.KD_DIMS)
def test_kd_every_width(dim):
    worst = [max(_kd_check('D=%d B=%d' % (dim, b), *lk.kd_width(b, dim), lk.KD_T)[0]) for b in lk.KD_BATCHES]
    assert max(worst) <= 1.0


@pytest.mark.parametrize('T', lk.KD_TEMPERATURES)
def test_kd_temperatures(T):
    use, _, _ = _kd_check('D=256 B=5 T=%g' % T, *lk.kd_width(5, 256), T)
    assert max(use) <= 1.0


@pytest.mark.parametrize('noise,dim', lk.KD_CLOSE)
def test_kd_close_rows(noise, dim):
    """the regime the expm1 / log1p formulation exists for: the bar is the float32 reference's own error, not twice it"""
    use, _, _ = _kd_check('close %g D=%d' % (noise, dim), *lk.kd_close(noise, dim), lk.KD_T, close=True)
    assert max(use) <= 1.0


@pytest.mark.parametrize('dim', [64, 256, 1024])
def test_kd_identical_rows_are_exactly_zero(dim):
    y, _ = lk.kd_width(5, dim)
    kl, g = _kd(y.to(DEV), y.clone().to(DEV), lk.KD_T)
    assert not kl.any() and not g.any(), 'every term of the kernel is an exact zero'


@pytest.mark.parametrize('scale', [20.0, 200.0])
def test_kd_gross_rows(scale):
    use, _, _ = _kd_check('gross scale=%g' % scale, *lk.kd_width(5, 256, scale), lk.KD_T)
    assert max(use) <= 1.0


def test_kd_underflowing_exponentials():
    d, scale, T = lk.KD_UNDERFLOW
    use, _, _ = _kd_check('underflow D=%d scale=%g T=%g' % (d, scale, T), *lk.kd_width(5, d, scale), T)
    assert max(use) <= 1.0


@pytest.mark.parametrize('dim', [256, 1024])
def test_kd_mixed_rows(dim):
    use, _, _ = _kd_check('mixed D=%d' % dim, *lk.kd_mixed(dim), lk.KD_T)
    assert max(use) <= 1.0


@pytest.mark.parametrize('dim', [64, 1024])
def test_kd_peaked_against_flat(dim):
    peaked, flat = lk.kd_peaked(dim)
    a, _, _ = _kd_check('peaked student D=%d' % dim, peaked, flat, lk.KD_T)           # Zp / Zq - 1 <= -0.5: logf(1 + x)
    b, _, _ = _kd_check('peaked teacher D=%d' % dim, flat, peaked, lk.KD_T)
    assert max(a) <= 1.0 and max(b) <= 1.0


def test_kd_shifted_rows():
    """a constant added to a row changes nothing: the shifted rows are held to the float64 values and bars of the unshifted"""
    (y, t), (ys, ts) = lk.kd_shifted()
    plain, kl0, g0 = _kd_check('unshifted', y, t, lk.KD_T)
    shifted, kl1, g1 = _kd_check('shifted +1e4 / -3000', ys, ts, lk.KD_T, reference_rows=(y, t))
    print('   shifted == unshifted bit for bit:', torch.equal(kl0, kl1) and torch.equal(g0, g1))
    assert max(plain) <= 1.0 and max(shifted) <= 1.0


@pytest.mark.parametrize('dim', [256, 1024])
def test_kd_rows_do_not_depend_on_their_batch(dim):
    y, t = (v.to(DEV) for v in lk.kd_width(5, dim))
    kl, g = _kd(y, t, lk.KD_T)
    for r in range(5):
        kl1, g1 = _kd(y[r:r + 1].contiguous(), t[r:r + 1].contiguous(), lk.KD_T)
        assert torch.equal(kl1[0], kl[r]) and torch.equal(g1[0], g[r])


def test_kd_negative_controls():
    """float64 side only.  T = 1 misses both bars; student and teacher swapped misses the gradient bar everywhere and the KL
    bar where the rows differ grossly -- KL(q || p) and KL(p || q) agree to second order between nearly equal rows (the
    finding of tests/test_gpu_mesa.py), so no implementation could fail that control on unit-norm rows."""
    for label, scale in (('unit', 1.0), ('x20', 20.0)):
        y, t = (v.to(DEV) for v in lk.kd_width(5, 256, scale))
        r64, bar_kl, bar_g, _ = _kd_bars(y, t, lk.KD_T)
        t1, sw = lk.kd_ref(y, t, 1.0), lk.kd_ref(t, y, lk.KD_T)
        miss = [float(((w.kl - r64.kl).abs() / bar_kl).max()) for w in (t1, sw)]
        miss += [float(((w.grad - r64.grad).abs().amax(1) / bar_g).max()) for w in (t1, sw)]
        print('kd controls (%s): T=1 misses by %.3g x (kl) %.3g x (dkl_dy); swapped by %.3g x (kl) %.3g x (dkl_dy)'
              % (label, miss[0], miss[2], miss[1], miss[3]))
        assert miss[0] >= 10 and miss[2] >= 10 and miss[3] >= 10
        if scale == 20.0:
            assert miss[1] >= 10
