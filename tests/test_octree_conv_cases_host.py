"""The generators and float64 references of tests/octree_conv_cases.py, proven on the CPU so that the GPU tests built on them
(tests/test_gpu_octree_conv_shapes.py) are not vacuous: the 'edges' tables hold every promised row, every column is injective,
the integer operands stay exact in fp32, the references agree with the oracle's OctreeDWConv and torch autograd on a real
octree, and a sequential fp32 evaluation of every real-data sum fits the `(T + 2) u S` bound the kernels are held to."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import octree_conv_cases as oc                                          # noqa: E402

KS = (1, 8, 26, 27, 28, 32)


@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
def test_edges_tables_hold_every_promised_row(K, dtype):
    n = oc.edges_min_rows(K) + 37
    t = oc.make_table(n, n + 11, K, 'edges', 3, dtype)
    assert t.dtype == dtype and tuple(t.shape) == (n, K)
    oc.check_edges(t, K)
    n_live = (t >= 0).sum(1)[:len(oc.edge_counts(K))].tolist()
    for c in oc.EDGE_COUNTS:
        assert (c in n_live) == (c <= K)
    assert K in n_live and int(oc.zero_live_rows(t).sum()) >= oc.DEAD_RUN + 1
    assert int(t.max()) < n + 11 and int(t.min()) == -1
    with pytest.raises(ValueError):                                     # a table that cannot hold them is refused
        oc.make_table(oc.edges_min_rows(K) - 1, n, K, 'edges', 3)


@pytest.mark.parametrize('live', ['dense', 'sparse', 'edges'])
@pytest.mark.parametrize('shape', [(40, 40), (40, 97), (300, 300)])
def test_every_column_is_injective(live, shape):
    for K in (1, 8, 27):
        t = oc.make_table(shape[0], shape[1], K, live, 5)
        assert oc.is_injective(t)
        frac = float((t >= 0).double().mean())
        assert frac == 1.0 if live == 'dense' else frac < 0.6
    t = oc.make_table(97, 40, 8, 'sparse', 5)                            # more output than source rows
    assert oc.is_injective(t) and int(t.max()) < 40
    assert not oc.is_injective(torch.tensor([[0, 1], [0, -1]]))
    t1, h, k = oc.single_reader(oc.make_table(300, 300, 27, 'sparse', 5))
    assert int(t1[h, k]) == 0 and int((t1 == 0).sum()) == 1 and int((t1[h] >= 0).sum()) > 1


def test_int_operands_stay_exact():
    """the worst |sum| the table allows is below 2^24, and the helper refuses operands that would pass it"""
    for K in KS:
        n = 4099
        t = oc.make_table(n, n, K, 'edges', 1)
        data, weight, grad, b = oc.int_operands(t, n, 12, 2, lim=3)
        assert b == 9 * K + 3 and float(data.abs().max()) == 3 and data.dtype == torch.float32
        assert torch.equal(data, data.round()) and torch.equal(weight, weight.round()) and torch.equal(grad, grad.round())
        *_, b1 = oc.int_operands(t, n, 12, 2, lim=1, rows_sum=True)
        assert b1 == max(K + 1, int((t >= 0).sum(0).max())) < 2 ** 24
        out, S, _ = oc.dwconv_ref(data, weight, t)
        assert float(S.max()) + 3 <= b and torch.equal(out.float().double(), out)
    with pytest.raises(AssertionError):
        oc.int_operands(oc.make_table(8, 8, 27, 'dense', 1), 8, 4, 2, lim=1000)
    for counts in oc.TAP_COUNTS.values():
        assert max(counts) < 2 ** 24                                     # |g|, |dpart| <= 1: a tap's sum is at most its pairs


def _golden_octree(golden_dir, i):
    from oracle.ocnn_ref import Octree, Points
    d = np.load(os.path.join(golden_dir, 'ocnn', 'test_%03d.npz' % i))
    o = Octree(int(d['depth']), int(d['full_depth']))
    o.build_octree(Points(torch.from_numpy(d['points']), torch.from_numpy(d['normals'])))
    o.construct_all_neigh()
    return o


@pytest.mark.parametrize('nempty', [True, False])
def test_references_agree_with_the_oracle_and_autograd(golden_dir, nempty):
    from oracle.ocnn_ref.nn import OctreeDWConv
    o = _golden_octree(golden_dir, 4)
    depth, C = 4, 6
    table = o.get_neigh(depth, '333', 1, nempty)
    n = int(o.nnum_nempty[depth] if nempty else o.nnum[depth])
    assert table.shape == (n, 27) and oc.is_injective(table)
    g = torch.Generator().manual_seed(7)
    conv = OctreeDWConv(C, [3], nempty=nempty).double()
    x = torch.randn(n, C, generator=g, dtype=torch.float64, requires_grad=True)
    proj = torch.randn(n, C, generator=g, dtype=torch.float64)
    y = conv(x, o, depth)
    y.backward(proj)
    out, S, T = oc.dwconv_ref(x.detach(), conv.weights.detach(), table)
    assert torch.allclose(out, y.detach(), rtol=0, atol=1e-13)
    assert torch.equal(T.flatten(), (table >= 0).sum(1)) and bool((S >= out.abs() - 1e-13).all())
    gw, _, rows = oc.wgrad_ref(proj, x.detach(), table)
    assert torch.allclose(gw, conv.weights.grad, rtol=0, atol=1e-12)
    assert torch.equal(rows.flatten(), (table >= 0).sum(0))
    dx, _, _ = oc.dwconv_transpose_ref(proj, conv.weights.detach(), table, n)
    assert torch.allclose(dx, x.grad, rtol=0, atol=1e-13)
    # the data gradient is the forward over the inverse table (libs/dwconv/dwconv/nn.py:36-38)
    inv = oc.inverse_ref(table, n)
    assert torch.allclose(oc.dwconv_ref(proj, conv.weights.detach(), inv)[0], dx, rtol=0, atol=1e-13)
    assert torch.equal(oc.inverse_ref(inv, n), table)                   # a square injective table: an involution
    # octree2col and its transpose
    from oracle.ocnn_ref.nn import octree_gather
    assert torch.equal(oc.gather_ref(x.detach(), table), octree_gather(x.detach(), table).flatten(1))
    dcol = torch.randn(n, 27 * C, generator=g, dtype=torch.float64)
    x2 = x.detach().clone().requires_grad_(True)
    (octree_gather(x2, table).flatten(1) * dcol).sum().backward()
    assert torch.allclose(oc.gather_transpose_ref(dcol, table, n), x2.grad, rtol=0, atol=1e-13)


def test_inverse_of_a_non_square_table():
    t = oc.make_table(50, 131, 8, 'sparse', 9)
    inv = oc.inverse_ref(t, 131)
    assert tuple(inv.shape) == (131, 8) and inv.dtype == t.dtype
    h, k = (t >= 0).nonzero(as_tuple=True)
    assert torch.equal(inv[t[h, k].long(), k], h.to(inv.dtype)) and int((inv >= 0).sum()) == h.numel()


def test_layer_norm_reference_is_beta_on_a_zero_live_row():
    K, C = 27, 32
    n = oc.edges_min_rows(K)
    t = oc.make_table(n, n, K, 'edges', 4)
    x, w, _ = oc.real_operands(t, n, C, 5)
    gamma, beta = oc.norm_params(C, 6)
    out, conv, _, T = oc.cpe_ref(x, w, gamma, beta, t, residual=False)
    dead = torch.from_numpy(oc.zero_live_rows(t))
    assert int(dead.sum()) == oc.DEAD_RUN + 1 and bool((T.flatten()[dead] == 0).all())
    assert torch.equal(conv[dead], torch.zeros_like(conv[dead]))
    assert torch.equal(out[dead], beta.double().expand_as(out[dead]))
    out_r = oc.cpe_ref(x, w, gamma, beta, t, residual=True)[0]
    assert torch.equal(out_r[dead], beta.double() + x.double()[dead])
    ln = torch.nn.functional.layer_norm(conv, (C,), gamma.double(), beta.double(), 1e-5)
    assert torch.allclose(out, ln, rtol=0, atol=1e-12)


def test_slot_sum_reference():
    t = oc.make_table(60, 200, 32, 'edges', 8)
    part, _, _ = oc.real_operands(t, 200, 8, 9)
    bias = torch.randn(8)
    out, S, T = oc.slot_sum_ref(part, t, bias)
    want = torch.stack([part.double()[t[h][t[h] >= 0].long()].sum(0) for h in range(60)]) + bias.double()
    assert torch.allclose(out, want, rtol=0, atol=1e-13) and bool((S >= out.abs() - 1e-13).all())
    assert torch.equal(oc.slot_sum_ref(part, t)[0][torch.from_numpy(oc.zero_live_rows(t))], torch.zeros(oc.DEAD_RUN + 1, 8).double())


def test_tap_tables_follow_the_documented_layout():
    for taps, counts in oc.TAP_COUNTS.items():
        assert len(counts) == taps and counts[0] == 0 and counts[-1] == 0
        assert any(counts[i - 1] == 2048 and counts[i] == 0 and counts[i + 1] == 2048 for i in range(1, taps - 1))
        edges, chunks, off = oc.tap_tables(counts)
        assert chunks.dtype == torch.int32 and off.dtype == torch.int32 and off.numel() == taps + 1
        c = chunks.numpy()
        for k in range(taps):
            mine = c[off[k]:off[k + 1]]
            assert (mine[:, 0] == k).all() and (mine[:, 2] - mine[:, 1]).sum() == counts[k]
            if counts[k]:
                assert mine[0, 1] == edges[k] and mine[-1, 2] == edges[k + 1] and (mine[1:, 1] == mine[:-1, 2]).all()
    assert set(oc.TAP_COUNTS[27]) == set(oc.TAP_PAIR_COUNTS)
    lens = {int(b - a) for _, a, b in oc.tap_tables(oc.TAP_COUNTS[27])[1].numpy()}
    assert {1, 15, 16, 17, 63, 64, 65, 2047, 2048}.issubset(lens)          # the wave and group edges of the kernel's chunk loop


def _fits(got32, ref, S, T):
    err = (got32.double() - ref).abs()
    return bool((err <= oc.bound(T, S)).all())


@pytest.mark.parametrize('live', ['edges', 'sparse'])
def test_sequential_fp32_sums_fit_the_bound(live):
    """a correct fp32 kernel fits `(T + 2) u S`: the same sums, evaluated term by term in fp32 with torch on the CPU"""
    K, C, n = 27, 12, 120
    t = oc.make_table(n, n, K, live, 11)
    data, w, grad = oc.real_operands(t, n, C, 12)
    idx, lv = t.long().clamp_min(0), (t >= 0)
    terms = torch.stack([torch.where(lv[:, k:k + 1], data[idx[:, k]] * w[k], torch.zeros(n, C)) for k in range(K)])
    ref, S, T = oc.dwconv_ref(data, w, t)
    assert _fits(oc.seq32(terms), ref, S, T)
    ref, S, T = oc.dwconv_ref(data, w, t, add=grad)                      # dwconv_add
    assert _fits(oc.seq32(terms) + grad, ref, S, T)
    ref, S, T = oc.slot_sum_ref(data, t, w[0, 0])                        # slot sum with a bias
    ones = torch.stack([torch.where(lv[:, k:k + 1], data[idx[:, k]], torch.zeros(n, C)) for k in range(K)])
    assert _fits(oc.seq32(ones) + w[0, 0], ref, S, T)
    # the transpose (the data gradient through the inverse table)
    inv = oc.inverse_ref(t, n)
    ii, il = inv.long().clamp_min(0), (inv >= 0)
    terms = torch.stack([torch.where(il[:, k:k + 1], grad[ii[:, k]] * w[k], torch.zeros(n, C)) for k in range(K)])
    ref, S, T = oc.dwconv_transpose_ref(grad, w, t, n)
    assert _fits(oc.seq32(terms), ref, S, T)
    # depth-wise weight gradient: rows in order; T = live rows + slabs, the slabs only widen it
    ref, S, rows = oc.wgrad_ref(grad, data, t)
    terms = torch.stack([torch.where(lv[h].reshape(K, 1, 1), (data[idx[h]] * grad[h]).reshape(K, 1, C), torch.zeros(K, 1, C))
                         for h in range(n)])
    assert _fits(oc.seq32(terms), ref, S, rows + oc.wgrad_slabs(n, C, K, 256))
    assert oc.wgrad_slabs(n, C, K, 256) == 8 and oc.wgrad_slabs(4099, 1028, 27, 256) == 0 and oc.wgrad_slabs(10 ** 6, 4, 27, 256) == 768


def test_sequential_fp32_tap_wgrad_fits_the_bound():
    counts = oc.TAP_COUNTS[8]
    edges, _, _ = oc.tap_tables(counts)
    g = torch.Generator().manual_seed(13)
    a, b = torch.randn(int(edges[-1]), 4, generator=g), torch.randn(int(edges[-1]), 3, generator=g)
    ref, S = oc.tap_wgrad_ref(a, b, edges)
    got = torch.zeros(8, 4, 3)
    prod = a[:, :, None] * b[:, None, :]
    for k in range(8):
        if counts[k]:
            got[k] = prod[edges[k]:edges[k + 1]].cumsum(0)[-1]           # (cumsum in fp32 runs in storage order)
    assert _fits(got, ref, S, oc.tap_terms(counts))
    assert torch.equal(ref[0], torch.zeros(4, 3).double()) and torch.equal(ref[2], torch.zeros(4, 3).double())
    # non-finite values propagate through the reference as IEEE arithmetic has them
    b[int(edges[5]) - 1, 0], b[int(edges[5]) - 1, 1] = float('inf'), float('nan')
    bad, _ = oc.tap_wgrad_ref(a, b, edges)
    assert bool(torch.isinf(bad[4, :, 0]).all()) and bool(torch.isnan(bad[4, :, 1]).all())
    keep = torch.ones_like(bad, dtype=torch.bool)
    keep[4, :, :2] = False
    assert torch.equal(bad[keep], ref[keep])
