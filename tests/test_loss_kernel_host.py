"""The references and cases of tests/loss_kernel_cases.py, proven on the CPU: the float64 references reproduce the golden
values of the reference's own loss classes, every case has the property it is named for, and the float32 yardstick exists
(finite, non-zero) on every case -- so that tests/test_gpu_loss_kernels.py cannot pass or fail for the wrong reason."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import loss_kernel_cases as lk                              # noqa: E402
from hotformerloc_amd import synthetic as syn               # noqa: E402
from oracle import loss_ref                                 # noqa: E402
from oracle.gen_golden_loss import make_case                # noqa: E402


# ------------------------------------------------------------------------------------------------ the references
def _loss_through_ref(emb, pos, neg, tau, ppq):
    """loss and d loss / d emb of the cosine TruncatedSmoothAP, the ranking rows through `smoothap_ref`: top-k, the mean over
    the valid rows and dE = (dS + dS^T) E are the module's own dense steps, restated here in float64."""
    e = emb.double()
    S = e @ e.t()
    idx = lk.top_positives(S, pos, ppq)
    r = lk.smoothap_ref(S, pos, neg, idx, tau)
    valid = torch.gather(pos, 1, idx).sum(1) > 0
    loss = 1.0 - r.ap[valid].mean()
    dS = -r.grad * (valid.double() / valid.sum())[:, None]
    return loss.item(), (dS + dS.t()) @ e


@pytest.mark.parametrize('case', ['b64', 'b48_few_pos', 'b96_p2'])
def test_smoothap_ref64_reproduces_the_reference_golden(golden_dir, case):
    g = np.load(os.path.join(golden_dir, 'loss_smoothap.npz'))
    seed, batch, dim, group, drop, ppq = [int(v) for v in g[case + '.cfg']]
    e, pos, neg = make_case(seed, batch, dim, group, drop)
    loss, grad = _loss_through_ref(torch.from_numpy(e), torch.from_numpy(pos), torch.from_numpy(neg), 0.01, ppq)
    gref = g[case + '.grad']
    print(case, 'loss', loss, float(g[case + '.loss']), 'grad err', np.abs(grad.numpy() - gref).max(), 'of', np.abs(gref).max())
    assert abs(loss - float(g[case + '.loss'])) < 1e-6
    assert np.abs(grad.numpy() - gref).max() <= 1e-6 * max(1.0, np.abs(gref).max())


@pytest.mark.parametrize('seed,batch,dim,ppq', [(3, 24, 16, 4), (4, 37, 8, 2)])
def test_smoothap_ref64_equals_the_loss_oracle(seed, batch, dim, ppq):
    """float64 on both sides, the oracle through its own autograd graph: 1e-10.  The references take the temperature as the
    float32 number the kernel receives, so the oracle is given that number."""
    e = torch.from_numpy(lk.uniform(seed, batch, dim))
    e = e / e.norm(dim=1, keepdim=True)
    pos = torch.from_numpy(lk.uniform(seed + 10, batch, batch) < -0.6)
    neg = torch.from_numpy(lk.uniform(seed + 20, batch, batch) < 0.2) & ~pos
    pos[1], pos[2, 3:] = False, False                       # a row without positives, a row with fewer than P
    ref = e.clone().requires_grad_()
    want, _ = loss_ref.truncated_smooth_ap(ref, pos, neg, lk.f32(0.01), ppq)
    want.backward()
    loss, grad = _loss_through_ref(e, pos, neg, 0.01, ppq)
    assert abs(loss - want.item()) <= 1e-10
    assert (grad - ref.grad).abs().max().item() <= 1e-10 * max(1.0, ref.grad.abs().max().item())


@pytest.mark.parametrize('case', ['b8', 'b64', 'b257', 'b48_d128', 'b64_x20'])
def test_kd_ref64_reproduces_the_reference_golden(golden_dir, case):
    g = np.load(os.path.join(golden_dir, 'mesa.npz'))
    seed, batch, dim, scale = g[case + '.cfg']
    y, t = (torch.from_numpy(v) for v in syn.kd_case(int(seed), int(batch), int(dim), float(scale)))
    kl, grad = lk.kd_ref64(y, t, 3.0)
    loss = 50.0 * kl.sum().item() / int(batch)              # loss.py:141-147: weight 50, reduction 'batchmean'
    want_l, want_g = float(g[case + '.loss64']), g[case + '.grad64']
    assert abs(loss - want_l) <= 1e-12 * abs(want_l)
    assert np.abs(50.0 / int(batch) * grad.numpy() - want_g).max() <= 1e-12 * np.abs(want_g).max()


# ------------------------------------------------------------------------------------------------ SmoothAP cases
def _exponents(case, q, slot=0):
    """e = -(s_z - s_p) / tau of row q, the subtraction in float32 as the kernel does it, and in float64"""
    S, p = case.S, int(case.idx[q, slot])
    e32 = -(S[q] - S[q, p]).double() / lk.f32(case.tau)
    e64 = -(S[q].double() - S[q, p].double()) / lk.f32(case.tau)
    return e32, e64


def _yardstick_exists(case):
    r64 = lk.smoothap_ref(*case)
    r32 = lk.smoothap_ref(*case, dtype=torch.float32)
    e_ap = (r32.ap.double() - r64.ap).abs().max().item()
    e_g = (r32.grad.double() - r64.grad).abs().max().item()
    assert np.isfinite(e_ap) and np.isfinite(e_g) and torch.isfinite(r64.scale).all()
    assert torch.isfinite(r64.ap).all() and torch.isfinite(r64.grad).all()
    return e_ap, e_g, r64


@pytest.mark.parametrize('B', lk.SIZES_B)
def test_size_cases(B):
    for P in lk.SIZES_P:
        case = lk.smoothap_random(B, P)
        assert case.S.shape == (B, B) and case.idx.shape == (B, P) and case.idx.dtype == torch.int64
        assert case.S.abs().max() < 1
        if B > 3:
            assert not (case.pos & case.neg).any() and not case.pos.diagonal().any() and not case.neg.diagonal().any()
        else:                      # dense masks: some row has a valid slot, and from B = 2 on a gradient
            r = lk.smoothap_ref(*case)
            assert (r.ap > 0).any() and (B == 1 or (r.scale > 0).any())
        if P > B:
            assert (case.idx[:, B:] == -1).all()
        if B >= 255:
            assert 0.07 < case.pos.float().mean() < 0.13 and 0.55 < case.neg.float().mean() < 0.65
            valid = torch.gather(case.pos, 1, case.idx.clamp(0, B - 1)) != 0
            assert valid.all(1).any() and (B < 1000 or valid.all())
            # idx is the true top-P: no unselected positive is more similar than the last selected one
            sp = case.S.double().masked_fill(case.pos == 0, float('-inf'))
            kth = sp.gather(1, case.idx[:, -1:].clamp(0, B - 1))
            assert ((sp > kth).sum(1) <= P - 1).all()
        e_ap, e_g, r64 = _yardstick_exists(case)
        if B >= 63:
            assert e_ap > 0 and e_g > 0 and (r64.scale > 0).any()


@pytest.mark.parametrize('tau', lk.TAUS)
def test_temperature_cases(tau):
    case = lk.smoothap_random(257, 4, tau)
    e_ap, e_g, r64 = _yardstick_exists(case)
    assert e_ap > 0 and e_g > 0
    e32, _ = _exponents(case, 0)
    assert ((e32.abs() > lk.CLAMP).any()) == (tau == 0.01)          # |s_z - s_p| < 2: only tau = 0.01 reaches the clamp


def test_mask_family_rows():
    case = lk.smoothap_families()
    B, P, R = lk.FAMILY_B, lk.FAMILY_P, lk.FAMILY_ROWS
    S, pos, neg, idx = case.S, case.pos.bool(), case.neg.bool(), case.idx
    e_ap, e_g, r64 = _yardstick_exists(case)
    assert e_ap > 0 and e_g > 0

    def valid(q):
        return [0 <= int(z) < B and bool(pos[q, int(z)]) for z in idx[q]]

    assert not pos[R['no_pos']].any() and valid(R['no_pos']) == [False] * P
    assert r64.ap[R['no_pos']] == 0 and (r64.grad[R['no_pos']] == 0).all()
    for name in lk.FEW_ROWS:
        q = R[name]
        assert pos[q].sum() == 2 and valid(q) == [True, True, False, False] and neg[q].any()
        assert S[q, idx[q, 0]] >= S[q, idx[q, 1]]
        if name == 'few_nonpos':
            assert all(0 <= int(z) < B and not pos[q, int(z)] for z in idx[q, 2:])
        elif name == 'few_wrap':       # the low 32 bits are the index of a positive
            assert idx[q, 2:].tolist() == [2 ** 32 + int(idx[q, 0])] * 2 and pos[q, int(idx[q, 2]) & 0xFFFFFFFF]
        else:
            assert idx[q, 2:].tolist() == [lk.FEW_SPARE[name]] * 2
        assert 0 < r64.ap[q] < 1 and r64.scale[q] > 0
    q = R['no_neg']
    assert not neg[q].any() and all(valid(q)) and r64.ap[q] == 1.0 and (r64.grad[q] == 0).all()
    q = R['all_pos']
    assert pos[q].all() and neg[q].any() and all(valid(q))
    q = R['both']
    both = (pos[q] & neg[q]).nonzero().flatten().tolist()
    assert len(both) == 1 and both[0] not in idx[q].tolist() and all(valid(q))
    assert 0 < S[q, idx[q, P - 1]] - S[q, both[0]] < 0.0031
    q = R['diag']
    assert pos[q, q] and int(idx[q, 0]) == q and all(valid(q))
    q = R['dup']
    assert int(idx[q, 0]) == int(idx[q, 1]) and len(set(idx[q].tolist())) == P - 1 and all(valid(q))
    # the other rows are ordinary ones
    rest = [q for q in range(B) if q not in R.values()]
    assert not (pos[rest] & neg[rest]).any() and not pos[rest, rest].any()
    # a row alone in its batch is the same row
    one = lk.alone(case, R['dup'])
    others = [q for q in range(B) if q != R['dup']]
    assert torch.equal(one.S[R['dup']], S[R['dup']]) and torch.equal(one.idx[R['dup']], idx[R['dup']])
    assert not one.S[others].any() and not one.pos[others].any() and not one.neg[others].any() and (one.idx[others] == -1).all()


def test_clamp_rows():
    case, special = lk.smoothap_clamp()
    assert case.tau == 2.0 ** -6 and case.idx.shape == (lk.CLAMP_B, 2)
    assert 1.5e4 < case.S.abs().max() < 1.6e4
    want = {50.0, -50.0, 200.0, -200.0, 1e6, -1e6}
    seen_pos, seen_neg = set(), set()
    for q in range(lk.CLAMP_B):
        e32, e64 = _exponents(case, q)
        assert torch.equal(e32, e64), 's_z - s_p of the first slot is exact in float32'
        e = e32[special[q]].tolist()
        assert want <= set(e)
        for sign in (1.0, -1.0):
            near = sorted(sign * v for v in e if 49.99 < sign * v < 50.01)
            assert len(near) == 3 and near[0] < 50.0 < near[2] and near[1] == 50.0
            assert all(abs(abs(v) / 50.0 - 1.0) <= 1.05 * 2.0 ** -20 for v in near)
        rest = [z for z in range(lk.CLAMP_B) if z not in special[q]]
        assert e32[rest].abs().max() < 8 and (e32[rest].abs() > 0.1).any()
        for z, v in zip(special[q], e):
            assert bool(case.pos[q, z]) != bool(case.neg[q, z])
            (seen_pos if case.pos[q, z] else seen_neg).add(v)
        assert case.pos[q, case.idx[q]].all()
    assert seen_pos == seen_neg == set(lk.clamp_exponents()) and len(seen_pos) == 10         # every exponent as a positive and as a negative
    e_ap, e_g, r64 = _yardstick_exists(case)
    assert e_ap > 0 and e_g > 0


def test_tie_row():
    case, cols = lk.smoothap_ties()
    q = lk.TIE_ROW
    assert len(cols) == lk.TIE_COUNT
    for j in range(lk.FAMILY_P):
        p = int(case.idx[q, j])
        assert case.pos[q, p] and (case.S[q, cols] == case.S[q, p]).all()
    assert case.pos[q, cols].sum() == 30 and case.neg[q, cols].sum() == 50
    a = 1.0 / (1.0 + torch.exp(-(case.S[q, cols] - case.S[q, int(case.idx[q, 0])]) / 0.01))
    assert (a == 0.5).all()
    e_ap, e_g, _ = _yardstick_exists(case)
    assert e_ap > 0 and e_g > 0


def test_lds_sizes_and_row_subsets():
    assert [9 * b for b, _ in lk.LDS_SIZES] == [49149, 49158, 65538, 153594]
    assert 9 * lk.CAPACITY <= 150 * 1024 < 9 * (lk.CAPACITY + 1) and lk.LDS_SIZES[-1][0] == lk.CAPACITY
    # a subset of rows built alone equals those rows of the whole batch (checked where the whole batch is cheap on the host)
    full = lk.smoothap_lds(1111, 2)
    rows = lk.sample_rows(1111)
    assert rows.numel() == 64 and rows[0] == 0 and rows[-1] == 1110 and rows.unique().numel() == 64
    part = lk.smoothap_lds(1111, 2, rows=rows)
    for a, b in zip(full[:4], part[:4]):
        assert torch.equal(a[rows], b)
    assert 0.07 < full.pos.float().mean() < 0.13 and 0.55 < full.neg.float().mean() < 0.65
    assert not (full.pos & full.neg).any() and not full.pos.diagonal().any() and not full.neg.diagonal().any()
    for B, P in lk.LDS_SIZES:
        rows = lk.sample_rows(B, 8)
        part = lk.smoothap_lds(B, P, rows=rows)
        assert part.S.shape == (8, B) and part.idx.shape == (8, P)
        assert (torch.gather(part.pos, 1, part.idx) != 0).all()
        r64 = lk.smoothap_ref(*part)
        r32 = lk.smoothap_ref(*part, dtype=torch.float32)
        assert torch.isfinite(r64.grad).all() and (r64.scale > 0).all()
        assert (r32.ap.double() - r64.ap).abs().max() > 0 and (r32.grad.double() - r64.grad).abs().max() > 0


# ------------------------------------------------------------------------------------------------ KD cases
def _kd_yardstick_exists(y, t, T):
    r64, r32 = lk.kd_ref(y, t, T), lk.kd_ref(y, t, T, torch.float32)
    assert torch.isfinite(r64.kl).all() and torch.isfinite(r64.grad).all()
    assert torch.isfinite(r32.kl).all() and torch.isfinite(r32.grad).all()
    e_kl, e_g = (r32.kl.double() - r64.kl).abs().max().item(), (r32.grad.double() - r64.grad).abs().max().item()
    assert e_kl > 0 and e_g > 0
    assert (r64.kl > 0).all() and (r64.grad.sum(1).abs() <= 1e-14 / lk.f32(T)).all()
    return r64


def _kernel_view(y, t, T):
    """the quantities the kernel branches on, in float32 as it forms them: delta = b - a, exp(b), x = Zp / Zq - 1, and
    u = log(q / p) from float64"""
    T = np.float32(T)
    a = (y - y.amax(1, keepdim=True)) / T
    b = (t - t.amax(1, keepdim=True)) / T
    r64 = lk.kd_ref(y, t, T)
    p, q = torch.softmax(y.double() / float(T), 1), torch.softmax(t.double() / float(T), 1)
    x = a.double().exp().sum(1) / b.double().exp().sum(1) - 1.0
    return b - a, torch.exp(b), x, torch.log(q) - torch.log(p), r64


def test_kd_width_and_temperature_cases():
    assert lk.KD_DIMS == tuple(64 * k for k in range(1, 17))
    for d in lk.KD_DIMS:
        for b in lk.KD_BATCHES:
            y, t = lk.kd_width(b, d)
            assert y.shape == (b, d) and y.dtype == torch.float32 and not torch.equal(y, t)
        _kd_yardstick_exists(y, t, lk.KD_T)
    for T in lk.KD_TEMPERATURES:
        _kd_yardstick_exists(*lk.kd_width(5, 256), T)


@pytest.mark.parametrize('noise,dim', lk.KD_CLOSE)
def test_kd_close_cases(noise, dim):
    y, t = lk.kd_close(noise, dim)
    d = (t - y).abs()
    assert 0.5 * noise < d.max() <= 1.01 * noise and (d > 0).float().mean() > 0.9
    delta, _, x, u, r64 = _kernel_view(y, t, lk.KD_T)
    assert delta.abs().max() < 1 and u.abs().max() < 1 and x.abs().max() < 0.5        # the expm1 / log1p regime throughout
    _kd_yardstick_exists(y, t, lk.KD_T)


def test_kd_gross_and_underflow_cases():
    for scale in (20.0, 200.0):
        y, t = lk.kd_width(5, 256, scale)
        delta, _, _, _, _ = _kernel_view(y, t, lk.KD_T)
        assert (delta.abs() >= 1).any() == (scale == 200.0)
        _kd_yardstick_exists(y, t, lk.KD_T)
    d, scale, T = lk.KD_UNDERFLOW
    y, t = lk.kd_width(5, d, scale)
    delta, eb, _, _, _ = _kernel_view(y, t, T)
    assert (eb == 0).any(1).all(), 'exp(b) underflows to 0 in float32 in every row'
    assert (delta.abs() >= 1).any() and (delta.abs() < 1).any()
    _kd_yardstick_exists(y, t, T)


@pytest.mark.parametrize('dim', [256, 1024])
def test_kd_mixed_cases(dim):
    y, t = lk.kd_mixed(dim)
    assert ((t - y).abs() > 14.9).sum(1).tolist() == [3] * y.shape[0]
    delta, _, _, u, _ = _kernel_view(y, t, lk.KD_T)
    for r in range(y.shape[0]):
        assert (delta[r].abs() < 1).any() and (delta[r].abs() >= 1).any(), 'both sides of |delta| = 1 in one row'
        assert (u[r].abs() < 1).any() and (u[r].abs() >= 1).any(), 'both sides of |u| = 1 in one row'
        small = int((delta[r].abs() < 1).sum())
        assert small == 1 if r % 2 == 0 else small == dim - 3
    _kd_yardstick_exists(y, t, lk.KD_T)


@pytest.mark.parametrize('dim', [64, 1024])
def test_kd_peaked_cases(dim):
    peaked, flat = lk.kd_peaked(dim)
    _, _, x, _, _ = _kernel_view(peaked, flat, lk.KD_T)
    assert (x <= -0.5).all(), 'peaked student, flat teacher: Zp / Zq - 1 <= -0.5 in float64'
    _, _, x, _, _ = _kernel_view(flat, peaked, lk.KD_T)
    assert (x >= 0.5 * dim).all()
    _kd_yardstick_exists(peaked, flat, lk.KD_T)
    _kd_yardstick_exists(flat, peaked, lk.KD_T)


def test_kd_shifted_case():
    (y, t), (ys, ts) = lk.kd_shifted()
    for v in (y, t, ys, ts):
        assert torch.equal(v.double() * 256, (v.double() * 256).round())
    assert torch.equal(ys.double() - y.double(), torch.full_like(y, lk.KD_SHIFTS[0]).double())
    assert torch.equal(ts.double() - t.double(), torch.full_like(t, lk.KD_SHIFTS[1]).double())
    a, b = lk.kd_ref(y, t, lk.KD_T), lk.kd_ref(ys, ts, lk.KD_T)
    assert (a.kl - b.kl).abs().max() <= 1e-12 and (a.grad - b.grad).abs().max() <= 1e-12
    _kd_yardstick_exists(y, t, lk.KD_T)


def test_bar_helpers():
    err, bar = torch.tensor([0.0, 1.0, 3.0]), torch.tensor([0.0, 2.0, 4.0])
    assert lk.bar_use(err, bar) == 0.75
    with pytest.raises(AssertionError):
        lk.bar_use(torch.tensor([1e-30]), torch.tensor([0.0]))
    assert lk.bar_use(torch.zeros(2), torch.zeros(2)) == 0.0
    assert torch.equal(lk.row_bars(torch.tensor([1.0]), torch.tensor([4.0])), torch.tensor([2.0 + 4.0 * 2.0 ** -22]))
    assert torch.equal(lk.row_bars(torch.tensor([1.0]), torch.tensor([4.0]), close=True), torch.tensor([1.0]))
