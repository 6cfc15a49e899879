"""The octree convolution kernels (csrc/dwconv.hip, csrc/tapconv.hip, the gather pair of csrc/window_misc.hip) element by
element at every launch shape, through `ops` / `hotformerloc_amd.dwconv` and therefore the C ABI.  Cases, float64 references
and the bound are tests/octree_conv_cases.py, proven on the CPU by tests/test_octree_conv_cases_host.py; DESIGN.md ("shape
coverage of the octree convolution kernels") names the kernel instantiation every family below reaches.

Integer data must EQUAL the float64 reference (`torch.equal`); real data holds to `(T + 2) u S` per element.  The only literal
tolerance is the one `test_cpe_fused_and_gather` already uses for the fused LayerNorm output (atol 2e-5, rtol 1e-5).

'edges' tables need `edges_min_rows(K)` rows, so the row counts below that are smaller than that (1, rpb - 1, ...) run on
'sparse' tables only; every (C, K) gets one 'edges' case of `edges_min_rows(K) + rpb + 1` rows besides."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import octree_conv_cases as oc                                          # noqa: E402
from hotformerloc_amd import _native, ops                               # noqa: E402
from hotformerloc_amd import autograd as ag                             # noqa: E402
from hotformerloc_amd import dwconv as hdw                              # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
INF, NAN = float('inf'), float('nan')
IDX = (torch.int32, torch.int64)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _rpb(C):
    """rows per workgroup of the vec4 kernels (row_geom of csrc/dwconv.hip); 16 stands in for the scalar kernels"""
    return max(1, min(16, 256 // (C // 4))) if C % 4 == 0 and C <= 1024 else 16


def _d(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def _exact(got, ref64, what):
    assert torch.equal(ref64.float().double(), ref64), 'the reference itself is not exact in fp32: ' + str(what)
    assert torch.equal(got.cpu(), ref64.float()), what


def _within(got, ref64, S, T, what):
    err = (got.cpu().double() - ref64).abs()
    bar = oc.bound(T, S).expand_as(err)
    use = float((err / bar.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print('%s: worst use of (T+2)uS %.3f' % (what, use))
    assert bool((err <= bar).all()), (what, use)


def _tables(n, K, extra_src=0):
    """[(label, live)] for n rows"""
    return ['sparse'] + (['edges'] if n >= oc.edges_min_rows(K) and not extra_src else [])


def _row_counts(counts, K, rpb):
    """the issue's row counts, plus the smallest one that holds an 'edges' table"""
    return sorted({n for n in counts if n >= 1} | {oc.edges_min_rows(K) + rpb + 1})


# ==================================================================================== hfl_dwconv_forward_backward
FWD = [(C, K) for C in (4, 8, 12, 32, 96, 256, 512, 768, 1024) for K in (1, 8, 27)] + [(1028, 27), (64, 28), (7, 27)]


def _fwd_check(C, K, n, live, dtype, seed, what):
    table = oc.make_table(n, n, K, live, seed, dtype)
    data, w, g, _ = oc.int_operands(table, n, C, seed + 1)
    dev_t = table.to(DEV)
    _exact(ops.dwconv_forward_backward(*_d(data, w), dev_t), oc.dwconv_ref(data, w, table)[0], ('int', what))
    rdata, rw, rg = oc.real_operands(table, n, C, seed + 2)
    _within(ops.dwconv_forward_backward(*_d(rdata, rw), dev_t), *oc.dwconv_ref(rdata, rw, table), ('real', what))
    # the data gradient: the same kernel over hfl_inverse_neigh of the (square) table == the transpose of the reference
    inv = ops.inverse_neigh(dev_t)
    assert inv.dtype == dtype and torch.equal(inv.cpu(), oc.inverse_ref(table, n)), ('inverse', what)
    _exact(ops.dwconv_forward_backward(*_d(g, w), inv), oc.dwconv_transpose_ref(g, w, table, n)[0], ('int transpose', what))
    _within(ops.dwconv_forward_backward(*_d(rg, rw), inv), *oc.dwconv_transpose_ref(rg, rw, table, n), ('real transpose', what))


@pytest.mark.parametrize('C,K', FWD)
def test_dwconv_forward_backward_widths_taps_and_row_counts(C, K):
    rpb = _rpb(C)
    for dtype in IDX:
        for n in _row_counts((1, rpb - 1, rpb, rpb + 1, 8 * rpb + 1), K, rpb):
            for live in _tables(n, K):
                _fwd_check(C, K, n, live, dtype, 100 + n, (C, K, n, live, dtype))
            # a non-square sparse table (forward only: more source than output rows)
            table = oc.make_table(n, n + 5, K, 'sparse', 7 + n, dtype)
            data, w, _, _ = oc.int_operands(table, n + 5, C, n)
            _exact(ops.dwconv_forward_backward(*_d(data, w, table)), oc.dwconv_ref(data, w, table)[0], ('non-square', C, K, n))


@pytest.mark.parametrize('C', (4, 8, 12, 32, 96, 256, 512, 768, 1024))
def test_dwconv_forward_second_trip_of_the_persistent_loop(C):
    """more row groups than the grid can hold (at most 8 workgroups per CU): every workgroup takes a second trip"""
    n = _cus() * 8 * _rpb(C) + 1
    assert n * C * 4 <= 8.5e6
    _fwd_check(C, 27, n, 'edges', torch.int32, 31, (C, 27, n, 'second trip'))


# ==================================================================================== hfl_dwconv_weight_backward
def _slabs(n, C, K):
    """partial slabs per element, from the workspace the C API asks for (one (K, C) f32 slab per workgroup)"""
    return int(_native.load().hfl_dwconv_weight_backward_workspace(n, C, K)) // (K * C * 4)


@pytest.mark.parametrize('C,K', FWD)
def test_dwconv_weight_backward_widths_taps_and_row_counts(C, K):
    rpb = _rpb(C)
    for n in _row_counts((1, 7, 8, 9, 8 * rpb - 1, 8 * rpb + 1, 4099), K, rpb):
        assert _slabs(n, C, K) == oc.wgrad_slabs(n, C, K, _cus())
        for dtype in IDX:
            for live in _tables(n, K):
                n_src = n + 3 if live == 'sparse' else n
                table = oc.make_table(n, n_src, K, live, 200 + n, dtype)
                dead_col = live == 'sparse' and K > 1
                if dead_col:
                    table[:, K - 1] = -1                                 # a tap column that is dead everywhere
                what = (C, K, n, live, dtype)
                data, _, g, _ = oc.int_operands(table, n_src, C, n, lim=1, rows_sum=True)
                got = ops.dwconv_weight_backward(*_d(g, data, table))
                _exact(got, oc.wgrad_ref(g, data, table)[0], ('int', what))
                assert torch.equal(got, ops.dwconv_weight_backward(*_d(g, data, table))), ('two calls', what)
                if dead_col:
                    assert torch.equal(got[K - 1].cpu(), torch.zeros(1, C)), ('dead column', what)
                if dtype == torch.int32 or n == 4099:
                    rdata, _, rg = oc.real_operands(table, n_src, C, n + 1)
                    ref, S, rows = oc.wgrad_ref(rg, rdata, table)
                    _within(ops.dwconv_weight_backward(*_d(rg, rdata, table)), ref, S, rows + _slabs(n, C, K), ('real', what))
    if K == 1:                                                           # K = 1: the only column dead
        table = torch.full((9, 1), -1, dtype=torch.int32)
        data, _, g, _ = oc.int_operands(table, 9, C, 1, lim=1, rows_sum=True)
        assert torch.equal(ops.dwconv_weight_backward(*_d(g, data, table)).cpu(), torch.zeros(1, 1, C))


# ==================================================================================== CPE: hfl_cpe_forward[_save], hfl_dwconv_add
CPE = [(C, K) for C in (32, 64, 128, 256) for K in (1, 8, 26, 27)]


@pytest.mark.parametrize('C,K', CPE)
def test_cpe_and_dwconv_add_row_counts_tables_and_residual(C, K):
    RPB = 1024 // C
    for n in _row_counts((1, RPB - 1, RPB, RPB + 1, 7 * RPB, 8 * RPB + 1, 64 * RPB + 3), K, RPB):
        for live in _tables(n, K):
            table = oc.make_table(n, n, K, live, 300 + n)
            dev_t = table.to(DEV)
            dead = torch.from_numpy(oc.zero_live_rows(table))
            what = (C, K, n, live)
            # ---- integer data
            x, w, add, _ = oc.int_operands(table, n, C, n)
            gamma, beta = oc.norm_params(C, n + 1)
            conv64 = oc.dwconv_ref(x, w, table)[0]
            _exact(ops.dwconv_add(*_d(x, w), dev_t), conv64, ('dwconv_add int', what))
            _exact(ops.dwconv_add(*_d(x, w), dev_t, add=add.to(DEV)), oc.dwconv_ref(x, w, table, add=add)[0], ('dwconv_add + add', what))
            for residual in (False, True):
                conv = torch.full((n, C), NAN, device=DEV)
                out = ops.cpe_forward(*_d(x, w, gamma, beta), dev_t, residual, conv_out=conv)
                _exact(conv, conv64, ('conv_out int', what, residual))
                assert torch.equal(out, ops.cpe_forward(*_d(x, w, gamma, beta), dev_t, residual)), ('save == no save', what)
                want = (beta + x[dead]) if residual else beta.expand(int(dead.sum()), C)      # fp32: beta, or fl(x + beta)
                assert torch.equal(out.cpu()[dead], want), ('zero-live rows', what, residual)
            # ---- real data
            x, w, add = oc.real_operands(table, n, C, n + 2)
            _within(ops.dwconv_add(*_d(x, w), dev_t, add=add.to(DEV)), *oc.dwconv_ref(x, w, table, add=add), ('dwconv_add real', what))
            for residual in (False, True):
                ref, conv64, S, T = oc.cpe_ref(x, w, gamma, beta, table, residual)
                conv = torch.full((n, C), NAN, device=DEV)
                out = ops.cpe_forward(*_d(x, w, gamma, beta), dev_t, residual, conv_out=conv)
                _within(conv, conv64, S, T, ('conv_out real', what, residual))
                assert torch.allclose(out.cpu().double(), ref, atol=2e-5, rtol=1e-5), ('out', what, residual)
                assert torch.equal(out, ops.cpe_forward(*_d(x, w, gamma, beta), dev_t, residual)), ('save == no save', what)


@pytest.mark.parametrize('C', (32, 64, 128, 256))
def test_cpe_second_trip_of_the_persistent_loop(C):
    """more row groups than the grid can hold (at most 8 workgroups per CU, dealt to the XCDs in eighths)"""
    K, n = 27, _cus() * 8 * (1024 // C) + 1
    assert n * C * 4 <= 8.5e6
    table = oc.make_table(n, n, K, 'edges', 33)
    dead = torch.from_numpy(oc.zero_live_rows(table))
    x, w, add, _ = oc.int_operands(table, n, C, 34)
    gamma, beta = oc.norm_params(C, 35)
    conv = torch.full((n, C), NAN, device=DEV)
    out = ops.cpe_forward(*_d(x, w, gamma, beta, table), True, conv_out=conv)
    _exact(conv, oc.dwconv_ref(x, w, table)[0], ('conv_out', C))
    assert torch.equal(out.cpu()[dead], beta + x[dead])
    _exact(ops.dwconv_add(*_d(x, w, table), add=add.to(DEV)), oc.dwconv_ref(x, w, table, add=add)[0], ('dwconv_add', C))
    x, w, _ = oc.real_operands(table, n, C, 36)
    ref, conv64, S, T = oc.cpe_ref(x, w, gamma, beta, table, True)
    out = ops.cpe_forward(*_d(x, w, gamma, beta, table), True, conv_out=conv)
    _within(conv, conv64, S, T, ('conv_out real', C))
    assert torch.allclose(out.cpu().double(), ref, atol=2e-5, rtol=1e-5)


@pytest.mark.parametrize('C,K', CPE)
def test_dwconv_add_over_the_inverse_of_a_non_square_table(C, K):
    """the data gradient of a convolution whose source and destination rows differ: dwconv_add over ops.inverse_table"""
    for n_dst, n_src, live in ((70, 201, 'sparse'), (201, 70, 'sparse'), (70, 201, 'dense')):
        table = oc.make_table(n_dst, n_src, K, live, 41)
        inv = ops.inverse_table(torch.empty((n_src, K), dtype=torch.int32, device=DEV), table.to(DEV))
        assert torch.equal(inv.cpu(), oc.inverse_ref(table, n_src))
        _, w, g, _ = oc.int_operands(table, n_src, C, 42)
        _exact(ops.dwconv_add(*_d(g, w), inv), oc.dwconv_transpose_ref(g, w, table, n_src)[0], (C, K, n_dst, n_src, live))
        _, rw, rg = oc.real_operands(table, n_src, C, 43)
        _within(ops.dwconv_add(*_d(rg, rw), inv), *oc.dwconv_transpose_ref(rg, rw, table, n_src), ('real', C, K, n_dst, n_src))


def test_cpe_entry_points_refuse_what_they_list():
    """other widths, K = 28 and out == data come back as HFL_EINVAL and leave `out` as it was"""
    lib = _native.load()
    s = ops._stream()
    for C, K in ((96, 27), (512, 27), (16, 8), (128, 28), (32, 28)):
        n = 40
        table = oc.make_table(n, n, K, 'sparse', 5).to(DEV)
        x, w = torch.randn(n, C, device=DEV), torch.randn(K, 1, C, device=DEV)
        gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
        out = torch.full((n, C), 7.0, device=DEV)
        conv = torch.full((n, C), 7.0, device=DEV)
        p = [t.data_ptr() for t in (out, conv, x, w, gamma, beta, table)]
        assert lib.hfl_cpe_forward_save(*p, n, C, K, 1e-5, 1, s) == _native.HFL_EINVAL, (C, K)
        assert lib.hfl_cpe_forward(p[0], *p[2:], n, C, K, 1e-5, 1, s) == _native.HFL_EINVAL, (C, K)
        assert lib.hfl_dwconv_add(p[0], p[2], p[3], p[6], None, n, C, K, s) == _native.HFL_EINVAL, (C, K)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and bool((conv == 7.0).all()), (C, K)
        with pytest.raises(_native.NativeLibraryError, match='HFL_EINVAL'):
            ops.cpe_forward(x, w, gamma, beta, table, True)
    n, C, K = 40, 64, 27
    table = oc.make_table(n, n, K, 'sparse', 5).to(DEV)
    x, w = torch.full((n, C), 7.0, device=DEV), torch.randn(K, 1, C, device=DEV)
    assert lib.hfl_dwconv_add(x.data_ptr(), x.data_ptr(), w.data_ptr(), table.data_ptr(), None, n, C, K, s) == _native.HFL_EINVAL
    assert lib.hfl_dwconv_add(None, x.data_ptr(), w.data_ptr(), table.data_ptr(), None, n, C, K, s) == _native.HFL_EINVAL
    torch.cuda.synchronize()
    assert bool((x == 7.0).all())


# ==================================================================================== hfl_slot_sum, hfl_slot_sum_norm
@pytest.mark.parametrize('C', (4, 12, 32, 64, 96, 128, 256, 1024))
@pytest.mark.parametrize('K', (1, 8, 27, 32))
def test_slot_sum_widths_and_slot_counts(C, K):
    rpb = _rpb(C)
    n = oc.edges_min_rows(K) + 8 * rpb + 1
    slot = oc.make_table(n, n + 9, K, 'edges', 400 + K)
    dead = torch.from_numpy(oc.zero_live_rows(slot))
    assert int(dead.sum()) >= oc.DEAD_RUN + 1
    part, w, _, _ = oc.int_operands(slot, n + 9, C, K)
    bias = w[0, 0]
    rpart, rw, _ = oc.real_operands(slot, n + 9, C, K + 1)
    dev_s = slot.to(DEV)
    for b, rb in ((None, None), (bias, rw[0, 0])):
        got = ops.slot_sum(part.to(DEV), dev_s, None if b is None else b.to(DEV))
        _exact(got, oc.slot_sum_ref(part, slot, b)[0], ('int', C, K, b is not None))
        want = torch.zeros(C) if b is None else b
        assert torch.equal(got.cpu()[dead], want.expand(int(dead.sum()), C)), ('all-dead rows', C, K)
        _within(ops.slot_sum(rpart.to(DEV), dev_s, None if rb is None else rb.to(DEV)), *oc.slot_sum_ref(rpart, slot, rb),
                ('real', C, K, rb is not None))
    if C in (32, 64, 128, 256):
        gamma, beta = _d(*oc.norm_params(C, K))
        beta[0] = -0.5                                                   # a negative beta: relu(beta) differs from beta
        for p, b in ((part, None), (part, bias), (rpart, None), (rpart, rw[0, 0])):
            p, b = _d(p, b)
            plain = ops.slot_sum(p, dev_s, b)
            for relu in (False, True):
                got = ops.slot_sum_norm(p, dev_s, b, gamma, beta, relu=relu)
                two = ops.layer_norm_relu(plain, gamma, beta) if relu else ops.layer_norm(plain, gamma, beta)
                assert torch.equal(got, two), ('fused norm == slot_sum + LayerNorm', C, K, relu)
                if b is None:
                    want = torch.relu(beta) if relu else beta
                    assert torch.equal(got[dead.to(DEV)], want.expand(int(dead.sum()), C)), ('zero-live rows', C, K, relu)


@pytest.mark.parametrize('C', (64, 96))
def test_slot_sum_second_trip_of_the_persistent_loop(C):
    """C = 64: slot_sum_kernel<16, ., 8>, C = 96: the generic <0, 0, 8>"""
    K, n = 32, _cus() * 8 * _rpb(C) + 1
    slot = oc.make_table(n, n + 9, K, 'edges', 37)
    part, w, _, _ = oc.int_operands(slot, n + 9, C, 38)
    _exact(ops.slot_sum(*_d(part, slot, w[0, 0])), oc.slot_sum_ref(part, slot, w[0, 0])[0], C)
    if C == 64:
        gamma, beta = _d(*oc.norm_params(C, 39))
        assert torch.equal(ops.slot_sum_norm(*_d(part, slot), None, gamma, beta),
                           ops.layer_norm(ops.slot_sum(*_d(part, slot)), gamma, beta))


# ==================================================================================== gather pair and inverse tables
@pytest.mark.parametrize('C', (3, 4, 64, 130))
@pytest.mark.parametrize('K', (8, 27))
def test_octree_gather_its_transpose_and_the_inverse_tables(C, K):
    n_dst, n_src = 300, 431
    table = oc.make_table(n_dst, n_src, K, 'sparse', 50 + K)
    dev_t = table.to(DEV)
    x = torch.randn(n_src, C, generator=torch.Generator().manual_seed(C))
    assert torch.equal(ops.octree_gather(x.to(DEV), dev_t).cpu(), oc.gather_ref(x, table))
    inv = ops.inverse_table(torch.empty((n_src, K), dtype=torch.int32, device=DEV), dev_t)
    assert torch.equal(inv.cpu(), oc.inverse_ref(table, n_src))
    # backward over the inverse table, integer data: the exact transpose
    xi = oc.int_operands(table, n_src, C, 3)[0].to(DEV).requires_grad_(True)
    dcol = torch.randint(-3, 4, (n_dst, K * C), generator=torch.Generator().manual_seed(K)).float()
    col = ag.octree_gather(xi, dev_t)
    assert torch.equal(col.detach().cpu(), oc.gather_ref(xi.detach().cpu(), table))
    col.backward(dcol.to(DEV))
    _exact(xi.grad, oc.gather_transpose_ref(dcol, table, n_src), ('gather_bwd', C, K))
    for dtype in IDX:                                                    # hfl_inverse_neigh: square tables, both index types
        for live in ('sparse', 'edges', 'dense'):
            sq = oc.make_table(n_dst, n_dst, K, live, 60 + K, dtype)
            got = ops.inverse_neigh(sq.to(DEV))
            assert got.dtype == dtype and torch.equal(got.cpu(), oc.inverse_ref(sq, n_dst)), (K, live, dtype)


# ==================================================================================== hfl_tap_wgrad[_gather]
def _tap_case(taps, cin, cout, kind, seed):
    counts = oc.TAP_COUNTS[taps]
    edges, chunks, off = oc.tap_tables(counts)
    P = int(edges[-1])
    gen = torch.Generator().manual_seed(seed)
    n_g, n_d = P // 3 + 5, P + 11                                       # g rows are shared between pairs, dpart rows are not
    if kind == 'int':
        g_src = torch.randint(-1, 2, (n_g, cin), generator=gen).float()
        d_src = torch.randint(-1, 2, (n_d, cout), generator=gen).float()
    else:
        g_src, d_src = torch.randn(n_g, cin, generator=gen), torch.randn(n_d, cout, generator=gen)
    g_rows = torch.randint(0, n_g, (P,), generator=gen, dtype=torch.int32)
    d_rows = torch.randperm(n_d, generator=gen)[:P].to(torch.int32)
    return counts, edges, chunks.to(DEV), off.to(DEV), g_src, d_src, g_rows, d_rows


def _tap_forms(taps, chunks, off, g_src, d_src, g_rows, d_rows):
    """the four instantiations of tap_wgrad_kernel<GATHER_G, GATHER_D>"""
    g_src, d_src, g_rows, d_rows = _d(g_src, d_src, g_rows, d_rows)
    g, d = g_src[g_rows.long()].contiguous(), d_src[d_rows.long()].contiguous()
    return [ops.tap_wgrad(g, d, chunks, off, taps),
            ops.tap_wgrad(g_src, d, chunks, off, taps, g_rows=g_rows),
            ops.tap_wgrad(g, d_src, chunks, off, taps, d_rows=d_rows),
            ops.tap_wgrad(g_src, d_src, chunks, off, taps, g_rows=g_rows, d_rows=d_rows)]


@pytest.mark.parametrize('cin,cout', [(64, 64), (64, 192), (192, 64), (128, 128)])
@pytest.mark.parametrize('taps', (8, 27))
def test_tap_wgrad_chunk_and_tile_edges(taps, cin, cout):
    for kind in ('int', 'real'):
        counts, edges, chunks, off, g_src, d_src, g_rows, d_rows = _tap_case(taps, cin, cout, kind, taps + cin)
        ref, S = oc.tap_wgrad_ref(g_src[g_rows.long()], d_src[d_rows.long()], edges)
        forms = _tap_forms(taps, chunks, off, g_src, d_src, g_rows, d_rows)
        for i, got in enumerate(forms):
            if kind == 'int':
                _exact(got, ref, ('int', taps, cin, cout, i))
            else:
                _within(got, ref, S, oc.tap_terms(counts), ('real', taps, cin, cout, i))
            assert torch.equal(got, forms[0]), ('the gather forms agree bit for bit', taps, cin, cout, i)
            for k, c in enumerate(counts):
                if c == 0:
                    assert torch.equal(got[k].cpu(), torch.zeros(cin, cout)), ('a tap without pairs', k)


# ==================================================================================== non-finite containment
def _same_class(got, ref64, what):
    """where the float64 reference of the poisoned problem is an inf or a NaN, the kernel's element is the same inf or a NaN;
    everywhere else it equals the reference (integer data)"""
    got = got.cpu().double()
    nan = torch.isnan(ref64)
    assert torch.equal(torch.isnan(got), nan), ('NaN where the element\'s own sum has none, or none where it has one', what)
    assert torch.equal(got[~nan], ref64[~nan]), what
    return int((~torch.isfinite(ref64)).sum())


def _poisoned(n, K, C, seed, dtype=torch.int32, lim=3, rows_sum=False):
    """a sparse square table in which exactly one live (row, tap) pair reads source row 0, and integer operands whose row 0
    holds one inf and one NaN"""
    table, h, k = oc.single_reader(oc.make_table(n, n, K, 'sparse', seed, dtype))
    data, w, g, _ = oc.int_operands(table, n, C, seed + 1, lim=lim, rows_sum=rows_sum)
    w[w == 0] = 1.0                                                      # (0 * inf is a NaN in the reference too; keep the inf an inf)
    g[g == 0] = 1.0
    bad = data.clone()
    bad[0, 1], bad[0, C - 2] = INF, NAN
    return table, h, k, data, bad, w, g


@pytest.mark.parametrize('C,K,dtype', [(32, 27, torch.int32), (256, 27, torch.int64), (1024, 8, torch.int32), (7, 27, torch.int32)])
def test_non_finite_values_stay_in_their_own_sums_dwconv_forward(C, K, dtype):
    table, h, k, data, bad, w, _ = _poisoned(150, K, C, 70, dtype)
    ref = oc.dwconv_ref(bad, w, table)[0]
    assert _same_class(ops.dwconv_forward_backward(*_d(bad, w, table)), ref, (C, K)) == 2
    clean = oc.dwconv_ref(data, w, table)[0]
    keep = torch.ones_like(ref, dtype=torch.bool)
    keep[h, 1] = keep[h, C - 2] = False
    assert torch.equal(ref[keep], clean[keep]) and not torch.isfinite(ref[~keep]).any()


@pytest.mark.parametrize('C', (32, 64, 128, 256))
def test_non_finite_values_stay_in_their_own_sums_cpe(C):
    """both gather paths of cpe_fwd_kernel (C >= 128: ballot path, whose loop repeats the row's last live tap past n_live)"""
    for seed in (71, 72, 73):
        n, K = 150, 27
        table, h, k, x, bad, w, add = _poisoned(n, K, C, seed)
        gamma, beta = oc.norm_params(C, 3)
        ref = oc.dwconv_ref(bad, w, table)[0]
        assert _same_class(ops.dwconv_add(*_d(bad, w, table)), ref, ('dwconv_add', C, seed)) == 2
        conv = torch.full((n, C), NAN, device=DEV)
        out = ops.cpe_forward(*_d(bad, w, gamma, beta, table), False, conv_out=conv)
        assert _same_class(conv, ref, ('conv_out', C, seed)) == 2
        clean = ops.cpe_forward(*_d(x, w, gamma, beta, table), False)
        rows = torch.arange(n, device=DEV) != h
        assert torch.equal(out[rows], clean[rows]), ('rows that do not read the poisoned row', C, seed)
        assert not bool(torch.isfinite(out[h]).any()), ('the LayerNorm of the row that does', C, seed)
    # the poisoned row as the LAST live tap of a row whose live count is no multiple of the gather batch (9)
    table = oc.make_table(n, n, K, 'sparse', 74)
    table[table == 0] = -1                                               # (no column holds row 0 now: reviving one entry keeps it injective)
    n_live = (table >= 0).sum(1)
    r = int(((n_live >= 2) & (n_live % 9 != 0)).nonzero()[0])
    last = int((table[r] >= 0).nonzero()[-1])
    table[r, last] = 0
    assert oc.is_injective(table) and int((table == 0).sum()) == 1
    ref = oc.dwconv_ref(bad, w, table)[0]
    assert bool(torch.isinf(ref[r, 1])) and bool(torch.isnan(ref[r, C - 2]))
    conv = torch.full((n, C), NAN, device=DEV)
    ops.cpe_forward(*_d(bad, w, gamma, beta, table), False, conv_out=conv)
    assert _same_class(conv, ref, ('conv_out, last live tap of ten', C)) == 2
    assert _same_class(ops.dwconv_add(*_d(bad, w, table)), ref, ('dwconv_add, last live tap of ten', C)) == 2


@pytest.mark.parametrize('C', (12, 64, 256))
def test_non_finite_values_stay_in_their_own_sums_slot_sum(C):
    slot, h, k, part, bad, w, _ = _poisoned(150, 32, C, 75)
    for bias in (None, w[0, 0]):
        ref = oc.slot_sum_ref(bad, slot, bias)[0]
        assert _same_class(ops.slot_sum(*_d(bad, slot, bias)), ref, (C, bias is not None)) == 2


@pytest.mark.parametrize('C,K,dtype', [(32, 27, torch.int32), (96, 27, torch.int64), (1024, 8, torch.int32), (7, 27, torch.int32)])
def test_non_finite_values_stay_in_their_own_sums_dwconv_weight_backward(C, K, dtype):
    """the kernel reads source row 0 for every dead tap and drops it by a select: the poison sits in row 0"""
    table, h, k, data, bad, _, g = _poisoned(300, K, C, 76, dtype, lim=1, rows_sum=True)
    ref = oc.wgrad_ref(g, bad, table)[0]
    assert _same_class(ops.dwconv_weight_backward(*_d(g, bad, table)), ref, (C, K)) == 2
    assert not torch.isfinite(ref[k, 0, 1]) and not torch.isfinite(ref[k, 0, C - 2])


@pytest.mark.parametrize('cin,cout', [(64, 64), (192, 64), (64, 192)])
def test_non_finite_values_stay_in_their_own_sums_tap_wgrad(cin, cout):
    """one inf and one NaN in the dpart row of the LAST pair of a chunk whose length is no multiple of 64 (17 and 65 pairs):
    the kernel clamps the pairs past the chunk's end to that pair.  Column j of dW[k] holds the pair's g[i] * dpart[j] for every
    i, so the whole column is an inf of the sign of g[i] (a NaN where g[i] = 0) or NaN in the reference; a kernel that multiplies
    the clamped row by a zeroed A operand makes the inf column NaN."""
    taps = 27
    counts, edges, chunks, off, g_src, d_src, g_rows, d_rows = _tap_case(taps, cin, cout, 'int', 77)
    hit = 0
    for k in (4, 7):                                                    # taps of 17 and 65 pairs
        assert counts[k] in (17, 65)
        last = int(d_rows[int(edges[k + 1]) - 1])
        bad = d_src.clone()
        bad[last, 2], bad[last, cout - 3] = INF, NAN
        ref, _ = oc.tap_wgrad_ref(g_src[g_rows.long()], bad[d_rows.long()], edges)
        assert int((~torch.isfinite(ref)).sum()) == 2 * cin and bool(torch.isinf(ref[k, :, 2]).any())
        for i, got in enumerate(_tap_forms(taps, chunks, off, g_src, bad, g_rows, d_rows)):
            hit += _same_class(got, ref, (cin, cout, k, i))
    assert hit == 2 * 4 * 2 * cin


# ==================================================================================== the drop-in Function
@pytest.mark.parametrize('C', (12, 96, 768))
@pytest.mark.parametrize('dtype', IDX)
def test_octree_dwconv_function_matches_float64_autograd(C, dtype):
    """hotformerloc_amd.dwconv.octree_dwconv (three kernels and the inverse-table cache) against float64 autograd of
    out[h] = sum_k w[k] data[t[h, k]]; integer data, so exactly.  The second round edits the table in place: the cached
    inverse must be rebuilt."""
    K = 27
    n = oc.edges_min_rows(K) + 40
    table = oc.make_table(n, n, K, 'edges', 80, dtype)
    dev_t = table.to(DEV)
    data, w, proj, _ = oc.int_operands(table, n, C, 81, lim=1, rows_sum=True)
    for rnd in range(2):
        if rnd == 1:
            dev_t[3:n:2, 5:20] = -1                                      # in place: same tensor, new version
            table = dev_t.cpu()
            assert oc.is_injective(table)
        x = data.clone().to(DEV).requires_grad_(True)
        wt = w.clone().to(DEV).requires_grad_(True)
        y = hdw.octree_dwconv(x, wt, dev_t)
        y.backward(proj.to(DEV))
        x64 = data.double().requires_grad_(True)
        w64 = w.double().requires_grad_(True)
        idx, live = table.long().clamp_min(0), (table >= 0).unsqueeze(-1)
        y64 = (x64[idx] * live * w64.reshape(1, K, C)).sum(1)
        y64.backward(proj.double())
        _exact(y.detach(), y64.detach(), ('out', C, dtype, rnd))
        _exact(x.grad, x64.grad, ('d data', C, dtype, rnd))
        _exact(wt.grad, w64.grad, ('d weights', C, dtype, rnd))
