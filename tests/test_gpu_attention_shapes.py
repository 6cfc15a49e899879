"""Window and relay attention at every shape the launchers accept, not only the four shipped configs: patch_size K in
{16, 32, 48, 64} with and without the relay token, dilation 1 / 2 / 3, 1 / 2 / 6 / 16 heads, octree depths 5..2 -- against a
float64 restatement of the reference's materialised windows (`oracle.hotformer_ref`) and torch autograd over it.

Small K makes the reference's RPE clamp live at depths <= 5 (pos_bnd = int(0.8 K sqrt(D)) is 12 for K = 16 and 25 for K = 32,
below the largest coordinate difference 2^depth - 1 at depth 4 resp. 5): the clamped forward kernels, the three-table RPE form of
the fp16 kernel and the edge-row fold of the matrix-core table gradient then see coordinates that the shipped K = 48 / 64 never
produce below depth 6.  `test_the_small_patch_sizes_make_the_clamp_live` proves that from the oracle alone.

Which kernel instance every family reaches is listed in DESIGN.md ("shape coverage of the attention kernels")."""

import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hotformerloc_amd import _native, build_batch_octree, model_factory, ops
from hotformerloc_amd import autograd as ag
from hotformerloc_amd import synthetic as syn
from hotformerloc_amd.params import CONFIG_DIR, ModelParams
from oracle import hotformer_ref
from oracle.testing import oracle_octree, synthetic_state_dict

from attention_cases import (DEV, ODEPTH, SIZES, octrees, pack_qkv_f16, window_plans, clouds as _clouds,
                             mask_pos as _mask_pos, oracle_plan as _oracle_plan, plan_args as _plan_args, plans as _plans,
                             relay_ref as _relay_ref, sequence_table as _sequence_table, windows_ref as _windows_ref)

HFL_EINVAL, HFL_ECAPACITY = -1, -2
LOG2E = 1.4426950408889634


def _clamp_is_live(oplan, depth, G, dil, K):
    """Some same-cloud pair of tokens inside one window is further apart than pos_bnd on some axis (oracle data only)."""
    bnd = int(0.8 * K * dil ** 0.5)
    mask, pos = _mask_pos(oplan, depth, 0, dil)          # (relay tokens carry no position)
    return bool(((pos.abs().amax(-1) > bnd) & (mask == 0)).any())


def _heads_per_wg(H):
    return 4 if H % 4 == 0 else 2 if H % 2 == 0 else 1


def _v5_promise(K, G, H, depth, bnd, rows):
    """What `v5_geometry` (csrc/attention.hip) promises for a problem with an RPE table, restated: the expanded-table form
    and whether the fp16 kernel takes the launch."""
    T = K // 16 + G
    if not (1 <= T <= 5 and (G == 0 and T <= 4 or G == 1 and T >= 2)) or not 1 <= depth <= 7:
        return 0, False
    LP, NP, W = T * 16, (T + 1) // 2, 2 * ((1 << depth) - 1) + 1
    form = 1 if depth <= 4 and (1 << depth) - 1 <= bnd else 2
    ts = (W + W * W + 3) & ~3 if form == 1 else (3 * W + 3) & ~3
    lds_of = lambda hpw: 2 * LP * 28 + hpw * ts * 4 + hpw * (2 * NP * 16) * 64
    hpw = _heads_per_wg(H)
    if lds_of(hpw) > 72 * 1024 and hpw == 4:
        hpw = 2
    ok = (lds_of(hpw) <= 72 * 1024 and hpw * 64 >= LP and not (form == 2 and hpw * ts * 4 + 12 * W >= 65536)
          and rows * 3 * H * 16 * 4 < 1 << 32)
    return form, ok


FAMILIES = ((5, 0, 1), (5, 0, 2), (5, 0, 3), (5, 1, 1), (4, 1, 1), (3, 1, 1), (2, 1, 1))        # (depth, G, dilation)
# what must hold before the GPU comparisons of the small patch sizes mean anything: (K, depth, G, dilation) with a live clamp
LIVE_CLAMP = ((16, 5, 0, 1), (16, 4, 0, 1), (16, 4, 1, 1), (16, 5, 1, 1), (16, 5, 0, 2), (32, 5, 0, 1), (32, 5, 1, 1))


def check_live_clamp():
    """CPU only (also run by hand without a GPU): the chosen clouds make the reference's RPE clamp live where the tests
    below say so, and nowhere at the shipped patch sizes."""
    for K, depth, G, dil in LIVE_CLAMP:
        assert _clamp_is_live(_oracle_plan(K, dil), depth, G, dil, K), (K, depth, G, dil)
    for K in (48, 64):
        for depth, G, dil in FAMILIES:
            assert not _clamp_is_live(_oracle_plan(K, dil), depth, G, dil, K), (K, depth, G, dil)


def test_the_small_patch_sizes_make_the_clamp_live():
    check_live_clamp()


def _split_value(o, rows, C, mode):
    """fp32 value of a split-precision output: mode 1 = [hi | hi | lo] planes, mode 2 = split2 blocks of 32 channels."""
    o = o.float().cpu()
    if mode == 1:
        assert torch.equal(o[:, :C], o[:, C:2 * C])
        return o[:, :C] + o[:, 2 * C:]
    v = o.view(rows, C // 32, 2, 32)
    return (v[:, :, 0] + v[:, :, 1]).reshape(rows, C)


@pytest.mark.parametrize('K,H', [(K, H) for K in (16, 32, 48, 64) for H in (2, 6, 16)] + [(64, 1)])
def test_window_attention_forward_every_family(K, H):
    """Forward kernels (v2 plain and clamped, v4, v5 in its three RPE forms) against the float64 oracle: 2e-5 for fp32
    operands, 3e-5 for the fp16 (hi, lo) operands, 3e-5 / 4e-5 for the reconstructed split output of the two.
    H = 1 (K = 64 with the relay token: 80 window slots against one wave of 64 threads) goes to v2 and has no fp16 form."""
    C = H * 16
    B = len(SIZES)
    g = torch.Generator().manual_seed(1000 + 17 * K + H)
    families = FAMILIES if H > 1 else tuple(f for f in FAMILIES if f[1] == 1)
    for depth, G, dil in families:
        oplan, plan = _plans(K, dil)
        nt, W = plan.n_tokens[depth], plan.n_windows[depth]
        assert nt == int(oplan.nnum_t[depth]) and W == int(oplan.nnum_a[depth]) // K
        real = -(-nt // K)                                     # windows that hold at least one token
        bnd = int(0.8 * K * dil ** 0.5)
        qkv_tok = torch.randn(nt, 3 * C, generator=g)
        qkv_rt = torch.randn(W, 3 * C, generator=g)
        table = torch.randn(3 * (2 * bnd + 1), H, generator=g) * 0.5
        want, want_tok = _windows_ref(oplan, qkv_tok.double(), qkv_rt.double(), table.double(), depth, K, G, dil, H)
        want0, want0_tok = _windows_ref(oplan, qkv_tok.double(), qkv_rt.double(), None, depth, K, G, dil, H)
        x = torch.cat([qkv_tok, qkv_rt]).to(DEV)
        rows_all = nt + W
        tag = (K, H, depth, G, dil)

        def run(tbl, dd, src=x, **kw):
            return ops.window_attention(src, plan.meta[depth], None if tbl is None else tbl, nt, W, K, dil, G, H, B,
                                        rt_row0=nt, depth=dd, **kw)

        def compare(got, ref_w, ref_tok, tol, what):
            err = (got[:nt].double() - ref_tok).abs().max().item()
            print('fwd', tag, what, 'tokens %.3g' % err)
            assert err < tol, (tag, what, err)
            if G:
                err = (got[nt:nt + real].double() - ref_w[:real, 0]).abs().max().item()
                print('fwd', tag, what, 'relay rows %.3g' % err)
                assert err < tol, (tag, what, 'relay rows', err)
                assert torch.isfinite(got).all(), (tag, what)
            else:
                assert torch.isfinite(got[:nt]).all(), (tag, what)

        tdev = table.to(DEV)
        for dd in (0, depth):                                  # depth given: the launcher may drop the clamp / take v4
            compare(run(tdev, dd).cpu(), want, want_tok, 2e-5, 'f32 depth=%d' % dd)
            compare(run(None, dd).cpu(), want0, want0_tok, 2e-5, 'f32 no table depth=%d' % dd)
        if C % 32 == 0:
            for mode in (1, 2):
                got = _split_value(run(tdev, depth, out_split=mode), rows_all, C, mode)
                compare(got, want, want_tok, 3e-5, 'f32 split %d' % mode)
        # fp16 (hi, lo) operands: the predicate answers what v5_geometry promises
        form, promised = _v5_promise(K, G, H, depth, bnd, rows_all)
        ok = ops.window_attention_f16_ok(rows_all, K, dil, G, H, depth)
        assert ok == promised, (tag, ok, promised)
        if H == 1:
            assert not ok                                      # one wave cannot own 80 window slots
        elif K in (16, 32, 48) and H == 16:
            assert ok, tag
        elif K == 64 and G == 1:
            assert ok, tag                                     # 5 tiles: the tables and image blocks of 4 (2) heads fit 72 KB
        if ok:
            assert form == (1 if depth <= 4 and (1 << depth) - 1 <= bnd else 2)
            packed = pack_qkv_f16(torch.cat([qkv_tok, qkv_rt]), H, 0.25 * LOG2E).to(DEV)
            compare(run(tdev, depth, src=packed, qkv_f16=True).cpu(), want, want_tok, 3e-5, 'f16 form %d' % form)
            compare(run(None, depth, src=packed, qkv_f16=True).cpu(), want0, want0_tok, 3e-5, 'f16 no table')
            for mode in (1, 2):
                got = _split_value(run(tdev, depth, src=packed, qkv_f16=True, out_split=mode), rows_all, C, mode)
                compare(got, want, want_tok, 4e-5, 'f16 split %d' % mode)


# ------------------------------------------------------------------------------------------------------------ backward
def _loss_weights(g, nt, W, C, real, G):
    wt = torch.randn(nt, C, generator=g)
    wr = torch.randn(W, C, generator=g)
    wd = torch.cat([wt, wr])
    if G:
        wd[nt + real:] = 0                                     # padding windows: their relay rows are not outputs
    else:
        wd[nt:] = 0
    return wt, wr, wd


def _backward_reference(oplan, qkv_tok, qkv_rt, table, wt, wr, depth, K, G, dil, H, real):
    """float64 autograd over the oracle's formulation: (dqkv token rows, dqkv relay rows, dtable)."""
    a = qkv_tok.double().requires_grad_()
    r = qkv_rt.double().requires_grad_()
    t = table.double().requires_grad_()
    o, o_tok = _windows_ref(oplan, a, r, t, depth, K, G, dil, H)
    loss = (o_tok * wt.double()).sum()
    if G:
        loss = loss + (o[:real, 0] * wr[:real].double()).sum()
    loss.backward()
    return a.grad, (r.grad if G else None), t.grad


def _hip_backward(plan, x, table, wd, depth, K, G, dil, H, B, nt, W):
    qd = x.detach().clone().requires_grad_()
    td = table.detach().clone().requires_grad_()
    od = ag.window_attention(qd, td, plan.meta[depth], n_tokens=nt, n_windows=W, patch_size=K, dilation=dil, n_relay=G,
                             n_heads=H, batch_size=B, rt_row0=nt, depth=depth)
    (od * wd).sum().backward()
    return qd.grad, td.grad


BWD_CASES = [(K, H, depth, G, dil) for K in (16, 32) for H in (2, 16)
             for depth, G, dil in ((5, 0, 1), (5, 0, 2), (4, 1, 1), (2, 1, 1), (5, 1, 1))] + \
            [(64, 6, 4, 1, 1), (64, 6, 5, 1, 1)]


@pytest.mark.parametrize('K,H,depth,G,dil', BWD_CASES)
def test_window_attention_backward_every_family(K, H, depth, G, dil):
    """dQKV (3e-5 max(scale, 1)) and the table gradient (1e-4 max(tscale, 1)) of the second-generation backward against float64
    autograd; both bitwise reproducible; the split2 form bitwise `ops.split2` of the fp32 gradient; the matrix-core table
    gradient against the scatter-add form (2e-5).  Where the clamp is live (K = 16 at depths 4 and 5, K = 32 at depth 5) the
    edge rows t = 0 and t = nrpe - 1 of the reference gradient are checked to be non-zero first: the fold of the clamped
    diagonals cannot pass on zeros.  RT = 2 needs three 16-row tiles (LR >= 64): of the live-clamp shapes only K = 32 with the
    relay token at depth 5 reaches it; K = 16 / 32 without it take the scatter-add at depth 5."""
    C, B = H * 16, len(SIZES)
    oplan, plan = _plans(K, dil)
    g = torch.Generator().manual_seed(2000 + 31 * K + 7 * H + 3 * depth + G + dil)
    nt, W = plan.n_tokens[depth], plan.n_windows[depth]
    real = -(-nt // K)
    bnd = int(0.8 * K * dil ** 0.5)
    nrpe = 2 * bnd + 1
    qkv_tok = torch.randn(nt, 3 * C, generator=g)
    qkv_rt = torch.randn(W, 3 * C, generator=g)
    table = torch.randn(3 * nrpe, H, generator=g) * 0.5
    wt, wr, wd = _loss_weights(g, nt, W, C, real, G)
    g_tok, g_rt, g_tab = _backward_reference(oplan, qkv_tok, qkv_rt, table, wt, wr, depth, K, G, dil, H, real)
    tag = (K, H, depth, G, dil)
    live = _clamp_is_live(oplan, depth, G, dil, K)
    assert live == ((K, depth, G, dil) in LIVE_CLAMP), tag
    if live:
        edges = g_tab.view(3, nrpe, H)
        assert edges[:, 0].abs().max().item() > 0 and edges[:, nrpe - 1].abs().max().item() > 0, tag
    x = torch.cat([qkv_tok, qkv_rt]).to(DEV)
    tdev, wdev = table.to(DEV), wd.to(DEV)
    desc = ag._desc(nt, W, K, dil, G, H, B, nt, depth)
    assert int(_native.load().hfl_window_attention_bwd_workspace(ctypes.byref(desc))) > 0      # the second-generation kernel
    gq, gt = _hip_backward(plan, x, tdev, wdev, depth, K, G, dil, H, B, nt, W)
    rows_ok = nt + real if G else nt                           # rows of padding windows are never written
    scale, tscale = g_tok.abs().max().item(), g_tab.abs().max().item()
    err = (gq[:nt].cpu().double() - g_tok).abs().max().item()
    terr = (gt.cpu().double() - g_tab).abs().max().item()
    print('bwd', tag, 'dqkv %.3g of scale %.3g, dtable %.3g of tscale %.3g' % (err, scale, terr, tscale))
    assert err < 3e-5 * max(scale, 1), (tag, err, scale)
    if G:
        err = (gq[nt:nt + real].cpu().double() - g_rt[:real]).abs().max().item()
        print('bwd', tag, 'relay rows %.3g' % err)
        assert err < 3e-5 * max(scale, 1), (tag, 'relay rows', err, scale)
    assert terr < 1e-4 * max(tscale, 1), (tag, terr, tscale)
    if live:
        e = (gt.cpu().double() - g_tab).view(3, nrpe, H)[:, [0, nrpe - 1]].abs().max().item()
        print('bwd', tag, 'edge rows %.3g' % e)
    # reproducible: partial tables per grid column, fixed-order sum
    gq2, gt2 = _hip_backward(plan, x, tdev, wdev, depth, K, G, dil, H, B, nt, W)
    assert torch.equal(gt2, gt), tag
    assert torch.equal(gq2[:rows_ok], gq[:rows_ok]), tag
    # the split2 form of dqkv
    dsp = torch.zeros((x.shape[0], 6 * C), dtype=torch.bfloat16, device=DEV)
    dtab = torch.zeros_like(tdev)
    ag._window_attention_bwd(dsp, dtab, x, wdev, plan.meta[depth], tdev, desc, split=True)
    assert torch.equal(dsp[:rows_ok].view(torch.int16), ops.split2(gq[:rows_ok].contiguous()).view(torch.int16)), tag
    assert torch.equal(dtab, gt), tag
    # the scatter-add table gradient
    lib = _native.load()
    try:
        assert lib.hfl_set_variant(b'window_bwd_rt', 0) == 0
        dq0 = torch.zeros((x.shape[0], 3 * C), device=DEV)
        dt0 = torch.zeros_like(tdev)
        ag._window_attention_bwd(dq0, dt0, x, wdev, plan.meta[depth], tdev, desc)
    finally:
        lib.hfl_set_variant(b'window_bwd_rt', -1)
    e0 = (dt0 - gt).abs().max().item()
    print('bwd', tag, 'matrix-core vs scatter-add dtable %.3g' % e0)
    assert e0 < 2e-5 * max(tscale, 1), (tag, e0)
    assert (dq0[:rows_ok] - gq[:rows_ok]).abs().max().item() < 2e-5 * max(scale, 1), tag


def test_window_attention_backward_first_generation_kernel():
    """K = 64, dilation 12: pos_bnd = 177, the table has 3 * 355 = 1065 > 1023 rows, so `launch_window_bwd` takes the
    first-generation kernel (float atomics on the table gradient: agreement within the tolerance, no bitwise promise)."""
    K, H, depth, G, dil = 64, 8, 5, 0, 12
    C, B = H * 16, len(SIZES)
    oplan, plan = _plans(K, dil)
    g = torch.Generator().manual_seed(2999)
    nt, W = plan.n_tokens[depth], plan.n_windows[depth]
    real = -(-nt // K)
    bnd = int(0.8 * K * dil ** 0.5)
    assert bnd == 177 and 3 * (2 * bnd + 1) > 1023
    qkv_tok = torch.randn(nt, 3 * C, generator=g)
    qkv_rt = torch.randn(W, 3 * C, generator=g)
    table = torch.randn(3 * (2 * bnd + 1), H, generator=g) * 0.5
    wt, wr, wd = _loss_weights(g, nt, W, C, real, G)
    g_tok, _, g_tab = _backward_reference(oplan, qkv_tok, qkv_rt, table, wt, wr, depth, K, G, dil, H, real)
    assert g_tab.abs().max().item() > 0
    desc = ag._desc(nt, W, K, dil, G, H, B, nt, depth)
    assert int(_native.load().hfl_window_attention_bwd_workspace(ctypes.byref(desc))) == 0     # no second-generation launch
    x = torch.cat([qkv_tok, qkv_rt]).to(DEV)
    # the forward of this shape first
    want, want_tok = _windows_ref(oplan, qkv_tok.double(), qkv_rt.double(), table.double(), depth, K, G, dil, H)
    got = ops.window_attention(x, plan.meta[depth], table.to(DEV), nt, W, K, dil, G, H, B, rt_row0=nt, depth=depth).cpu()
    assert (got[:nt].double() - want_tok).abs().max().item() < 2e-5
    gq, gt = _hip_backward(plan, x, table.to(DEV), wd.to(DEV), depth, K, G, dil, H, B, nt, W)
    scale, tscale = g_tok.abs().max().item(), g_tab.abs().max().item()
    err = (gq[:nt].cpu().double() - g_tok).abs().max().item()
    terr = (gt.cpu().double() - g_tab).abs().max().item()
    print('bwd first generation dqkv %.3g of scale %.3g, dtable %.3g of tscale %.3g' % (err, scale, terr, tscale))
    assert err < 3e-5 * max(scale, 1), (err, scale)
    assert terr < 1e-4 * max(tscale, 1), (terr, tscale)


def _reject_desc(**over):
    f = dict(n_tokens=64, rt_row0=64, n_windows=4, patch_size=16, dilation=1, n_relay=0, n_heads=2, pos_bnd=12, batch_size=1,
             scale=0.25, depth=5)
    f.update(over)
    return _native.WindowAttnDesc(**f)


@pytest.mark.parametrize('what,over,fwd', [('odd heads (backward)', dict(n_heads=3), False),
                                           ('one head (backward)', dict(n_heads=1), False),
                                           ('patch_size 40', dict(patch_size=40, pos_bnd=32), True),
                                           ('patch_size 80', dict(patch_size=80, pos_bnd=64), True),
                                           ('patch_size 0', dict(patch_size=0, pos_bnd=0), True),
                                           ('patch_size 0 with relay', dict(patch_size=0, pos_bnd=0, n_relay=1), True),
                                           ('n_relay 2', dict(n_relay=2), True),
                                           ('relay with dilation', dict(n_relay=1, dilation=2), True),
                                           ('17 heads', dict(n_heads=17), True)])
def test_window_attention_rejects_what_it_has_no_kernel_for(what, over, fwd):
    """HFL_EINVAL on the host, before any launch: the output buffers keep their contents."""
    lib = _native.load()
    d = _reject_desc(**over)
    H = max(d.n_heads, 1)
    rows = 128
    qkv = torch.zeros(rows, 3 * H * 16, device=DEV)
    dout = torch.zeros(rows, H * 16, device=DEV)
    meta = torch.zeros(rows, 2, dtype=torch.int32, device=DEV)
    table = torch.zeros(3 * (2 * d.pos_bnd + 1), H, device=DEV)
    out = torch.full((rows, 3 * H * 16), 7.0, device=DEV)
    dtab = torch.full_like(table, 7.0)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    args = (out.data_ptr(), dtab.data_ptr(), qkv.data_ptr(), dout.data_ptr(), meta.data_ptr(), table.data_ptr(), ctypes.byref(d))
    assert lib.hfl_window_attention_bwd(*args, ops._stream()) == HFL_EINVAL, what
    assert lib.hfl_window_attention_bwd_det(*args, ws.data_ptr(), ops._stream()) == HFL_EINVAL, what
    assert lib.hfl_window_attention_bwd_split2(*args, ws.data_ptr(), ops._stream()) == HFL_EINVAL, what
    with pytest.raises(_native.NativeLibraryError):
        ag._window_attention_bwd(out, dtab, qkv, dout, meta, table, d)
    if fwd:
        for flags in (0, 1, 2, 0x100):
            assert lib.hfl_window_attention_fwd_ex(out.data_ptr(), qkv.data_ptr(), None, meta.data_ptr(), table.data_ptr(),
                                                   ctypes.byref(d), flags, ops._stream()) == HFL_EINVAL, (what, flags)
        assert lib.hfl_window_attention_fwd(out.data_ptr(), qkv.data_ptr(), meta.data_ptr(), table.data_ptr(), ctypes.byref(d),
                                            ops._stream()) == HFL_EINVAL, what
        assert not lib.hfl_window_attention_f16_ok(ctypes.byref(d), rows), what        # the predicate refuses what the launcher does
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((dtab == 7.0).all()), what


# ------------------------------------------------------------------------------------------------------------ relay attention
RELAY_LENGTHS = [1, 15, 16, 17, 63, 64, 65, 0, 250]           # the <= 64 fast path, the 16-row tile edges, an empty cloud


@pytest.mark.parametrize('lengths,n_rows', [(RELAY_LENGTHS, 600), ([611], 640)], ids=['ragged', 'one-of-611'])
@pytest.mark.parametrize('H', [16, 2])
def test_relay_attention_by_sequence_length(lengths, n_rows, H):
    """Forward (2e-5), fp16-operand forward with and without the <= 64 fast path (3e-5 max), HIP backward (3e-5 max(scale, 1))
    against per-cloud dense attention in float64; orphan rows exactly 0.  611 rows is the LDS limit of the backward."""
    C, B = H * 16, len(lengths)
    seq_rows, seq_off, orphans = _sequence_table(lengths, n_rows, 77 + H)
    g = torch.Generator().manual_seed(3000 + H + n_rows)
    qkv = torch.randn(n_rows, 3 * C, generator=g)
    wgt = torch.randn(n_rows, C, generator=g)
    a = qkv.double().requires_grad_()
    want = _relay_ref(a, seq_rows, seq_off, H)
    (want * wgt.double()).sum().backward()
    want = want.detach()
    rows_d, off_d, orph_d = (torch.from_numpy(t).to(DEV) for t in (seq_rows, seq_off, orphans))
    max_len = max(lengths)
    x = qkv.to(DEV)
    got = ops.relay_attention(x, rows_d, off_d, B, H, max_len).cpu()
    err = (got.double() - want).abs().max().item()
    print('relay', lengths[-1], H, 'fwd %.3g' % err)
    assert err < 2e-5, err
    assert torch.all(got[torch.from_numpy(orphans.astype(np.int64))] == 0)
    bound = 3e-5 * max(want.abs().max().item(), 1.0)
    packed = pack_qkv_f16(qkv, H, 0.25 * LOG2E).to(DEV)
    lib = _native.load()
    for fast in (1, 0):
        try:
            assert lib.hfl_set_variant(b'relay_fast', fast) == 0
            o2 = ops.relay_attention_f16(packed, rows_d, off_d, B, H, max_len, orph_d)
        finally:
            lib.hfl_set_variant(b'relay_fast', 1)
        val = _split_value(o2, n_rows, C, 2)
        err = (val.double() - want).abs().max().item()
        print('relay', lengths[-1], H, 'f16 fast=%d %.3g (bound %.3g)' % (fast, err, bound))
        assert err < bound, (fast, err, bound)
        assert torch.all(val[torch.from_numpy(orphans.astype(np.int64))] == 0)
    xd = x.clone().requires_grad_()
    out = ag.RelayAttentionFn.apply(xd, rows_d, off_d, B, H, max_len)
    (out * wgt.to(DEV)).sum().backward()
    scale = a.grad.abs().max().item()
    err = (xd.grad.cpu().double() - a.grad).abs().max().item()
    print('relay', lengths[-1], H, 'bwd %.3g of scale %.3g' % (err, scale))
    assert err < 3e-5 * max(scale, 1.0), (err, scale)
    assert torch.all(xd.grad.cpu()[torch.from_numpy(orphans.astype(np.int64))] == 0)


def test_relay_attention_backward_capacity_and_the_torch_fallback(monkeypatch):
    """612 rows do not fit the LDS of `hfl_relay_attention_bwd`: HFL_ECAPACITY without a launch, and `RTAttention` takes the
    differentiable torch form there (its linear layers replaced by the identity: the attention core alone, held to the
    bounds of the HIP kernels)."""
    from hotformerloc_amd import model as hmodel
    H, lengths, n_rows = 2, [612, 40], 700
    C, B = H * 16, len(lengths)
    seq_rows, seq_off, orphans = _sequence_table(lengths, n_rows, 91)
    g = torch.Generator().manual_seed(3100)
    qkv = torch.randn(n_rows, 3 * C, generator=g)
    wgt = torch.randn(n_rows, C, generator=g)
    rows_d, off_d = torch.from_numpy(seq_rows).to(DEV), torch.from_numpy(seq_off).to(DEV)
    x = qkv.to(DEV)
    dq = torch.full_like(x, 7.0)
    rc = _native.load().hfl_relay_attention_bwd(dq.data_ptr(), x.data_ptr(), wgt.to(DEV).data_ptr(), rows_d.data_ptr(),
                                                off_d.data_ptr(), B, H, 0.25, 612, ops._stream())
    assert rc == HFL_ECAPACITY
    torch.cuda.synchronize()
    assert bool((dq == 7.0).all())
    idx = np.full((B, max(lengths)), -1, dtype=np.int64)
    for b in range(B):
        idx[b, :lengths[b]] = seq_rows[seq_off[b]:seq_off[b + 1]]
    pad = torch.from_numpy(idx).to(DEV)
    plan = types.SimpleNamespace(B=B, seq_rows=rows_d, seq_off=off_d, max_seq_len=612, relay_pad_index=lambda: (pad, pad >= 0))

    def no_hip_backward(*a, **k):
        raise AssertionError('the HIP relay backward must not be launched beyond 611 rows')
    monkeypatch.setattr(ag, 'relay_attention', no_hip_backward)
    taken = []
    torch_form = ag.relay_attention_torch
    monkeypatch.setattr(ag, 'relay_attention_torch', lambda *a, **k: (taken.append(1), torch_form(*a, **k))[1])
    mod = hmodel.RTAttention(C, H)
    mod.qkv, mod.proj = torch.nn.Identity(), torch.nn.Identity()
    xd = x.clone().requires_grad_()
    out = mod(xd, plan)
    (out * wgt.to(DEV)).sum().backward()
    assert taken == [1]
    a = qkv.double().requires_grad_()
    want = _relay_ref(a, seq_rows, seq_off, H)
    (want * wgt.double()).sum().backward()
    assert (out.detach().cpu().double() - want.detach()).abs().max().item() < 2e-5
    scale = a.grad.abs().max().item()
    assert (xd.grad.cpu().double() - a.grad).abs().max().item() < 3e-5 * max(scale, 1.0)
    assert torch.all(out.detach().cpu()[torch.from_numpy(orphans.astype(np.int64))] == 0)


# ------------------------------------------------------------------------------------------------------------ model level
REL_TOL = 1e-3           # descriptors: relative L2 (tests/test_gpu_model.py)
GRAD_TOL = 1e-3          # parameter gradients: relative L2 per tensor (tests/test_gpu_model.py)
_MODEL_ORACLE = {}


def _params_with(tmp_path, **over):
    src = open(os.path.join(CONFIG_DIR, 'wild_places.ini')).read()
    for k, v in over.items():
        pat = re.compile(r'^%s\s*=.*$' % re.escape(k), flags=re.M)
        line = '%s = %s' % (k, v)
        src = pat.sub(line, src) if pat.search(src) else src.rstrip('\n') + '\n' + line + '\n'
    path = tmp_path / 'wild_places_shapes.ini'
    path.write_text(src)
    return ModelParams(str(path))


@pytest.mark.parametrize('over', [dict(patch_size=32), dict(patch_size=16, dilation=2)], ids=['K32', 'K16-D2'])
def test_model_at_the_default_and_the_smallest_patch_size(tmp_path, over):
    """The Wild-Places model with patch_size 32 (the value `ModelParams` falls back to) and with 16 / dilation 2: eval
    descriptors on the x3 and x6 GEMMs and the parameter gradients of one training step against the CPU oracle, to the bounds
    of tests/test_gpu_model.py.  Neither one-launch attention kernel takes these K: the model runs on the separate launches."""
    from hotformerloc_amd.model import set_gemm_mode, set_train_split, set_train_x3
    params = _params_with(tmp_path, **over)
    K, D = params.patch_size, params.dilation
    assert (K, D) == (over['patch_size'], over.get('dilation', 4))
    clouds = [syn.cylindrical(syn.unit_ball_cloud(2300, 1500)), syn.cylindrical(syn.forest_cloud(2301, 1000))]
    proj = torch.from_numpy(syn.hash_uniform(4243, len(clouds) * 256).reshape(len(clouds), 256).astype(np.float32))
    key = (K, D)
    if key not in _MODEL_ORACLE:
        sd = {k: v.clone().requires_grad_() for k, v in synthetic_state_dict(params, 'stress').items()}
        y_ref = hotformer_ref.forward_with_grad(sd, params, oracle_octree(clouds, ODEPTH))
        (y_ref * proj).sum().backward()
        _MODEL_ORACLE[key] = (y_ref.detach().numpy(), {k: v.grad for k, v in sd.items()})
    y_ref, grads_ref = _MODEL_ORACLE[key]
    octree = build_batch_octree(clouds, ODEPTH, 2, DEV)
    # the predicates of the one-launch kernels
    nne = octree.nnum_nempty.tolist()
    heads, chans = list(params.num_heads), list(params.channels)
    for depth, dil, G in ((5, 1, 0), (5, D, 0), (4, 1, 1), (3, 1, 1), (2, 1, 1)):
        nt = int(nne[depth])
        W = -(-nt // (K * D)) * D
        if G == 0:
            assert not ops.attn_fused_ok(nt, W, K, dil, 0, heads[0], depth, chans[0], True), (K, depth, dil)
        else:
            assert not ops.attn_ws_ok(nt, W, K, heads[1], depth, chans[1]), (K, depth)
    rel = {}
    for mode in ('x3', 'x6'):
        set_gemm_mode(mode)
        try:
            model = model_factory(params)
            syn.fill_synthetic_weights(model, 'stress')
            model = model.cuda().eval()
            with torch.inference_mode():
                y = model({'octree': octree})['global'].cpu().numpy()
        finally:
            set_gemm_mode('x3')
        assert np.isfinite(y).all()
        rel[mode] = float((np.linalg.norm(y.astype(np.float64) - y_ref, axis=1) / np.linalg.norm(y_ref, axis=1)).max())
    print('model', key, 'descriptor rel-L2', rel)
    assert max(rel.values()) <= REL_TOL, rel
    # one training step (drop_path off: its draws are replayed in tests/test_gpu_train_drop_path.py)
    params.drop_path = 0.0
    model = model_factory(params)
    syn.fill_synthetic_weights(model, 'stress')
    model = model.cuda().train()
    set_train_x3(True)
    set_train_split(False)
    y = model({'octree': build_batch_octree(clouds, ODEPTH, 2, DEV)})['global']
    (y * proj.cuda()).sum().backward()
    yn = y.detach().cpu().numpy()
    r = float((np.linalg.norm(yn.astype(np.float64) - y_ref, axis=1) / np.linalg.norm(y_ref, axis=1)).max())
    assert r <= REL_TOL, r
    worst = {}
    for name, p in model.named_parameters():
        gref = grads_ref[name]
        assert p.grad is not None, name
        err = (p.grad.cpu() - gref).norm().item() / max(gref.norm().item(), 1e-12)
        kind = name.split('.')[-1] if 'rpe_table' not in name else 'rpe_table'
        worst[kind] = max(worst.get(kind, 0.0), err)
        assert err < GRAD_TOL or gref.norm().item() < 1e-9, (name, err, gref.norm().item())
    print('model', key, 'train forward rel', r, 'worst grad rel-L2 per kind', worst)
