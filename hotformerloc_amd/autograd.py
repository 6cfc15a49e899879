"""Autograd glue of the training path: `torch.autograd.Function`s whose forward AND backward are
HIP kernels (window attention, octree-conv gather, relay-token init; the depth-wise conv lives in
`hotformerloc_amd.dwconv`), plus differentiable torch formulations of the two tiny ragged ops
whose backward kernels are not written yet (relay-token attention, attentional pooling).

The reference gets all of this from PyTorch autograd over its materialised masks
(`models/octformer_backbone.py:59-93`) and from `libs/dwconv/dwconv/nn.py:17-43`."""

import ctypes
import weakref
from typing import Callable, NamedTuple

import torch

from . import _native, ops
from ._native import WindowAttnDesc, check
from .weight_cache import derived


def _desc(n_tokens, n_windows, patch_size, dilation, n_relay, n_heads, batch_size, rt_row0, depth):
    return WindowAttnDesc(n_tokens=n_tokens, rt_row0=rt_row0, n_windows=n_windows,
                          patch_size=patch_size, dilation=dilation, n_relay=n_relay, n_heads=n_heads,
                          pos_bnd=int(0.8 * patch_size * dilation ** 0.5), batch_size=batch_size,
                          scale=16 ** -0.5, depth=depth)


def _window_attention_bwd(dqkv, dtable, qkv, dout, tok_meta, table, desc, split=False):
    """hfl_window_attention_bwd with the reproducible table gradient when the launch has one (partial tables in a workspace,
    fixed-order sum), the float-atomic form otherwise (tables too large for the second-generation kernel).  split: dqkv is the
    (rows, 2 * 3C) bf16 split2 operand of the GEMMs behind it (hfl_window_attention_bwd_split2)."""
    lib = _native.load()
    tp = None if table is None else table.data_ptr()
    dp = None if dtable is None else dtable.data_ptr()
    nbytes = int(lib.hfl_window_attention_bwd_workspace(ctypes.byref(desc))) if dtable is not None else 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=qkv.device) if nbytes > 0 else None
    if split:
        assert dqkv.dtype == torch.bfloat16 and dqkv.shape[1] == 2 * qkv.shape[1]
        check(lib.hfl_window_attention_bwd_split2(dqkv.data_ptr(), dp, qkv.data_ptr(), dout.data_ptr(), tok_meta.data_ptr(), tp,
                                                  ctypes.byref(desc), None if ws is None else ws.data_ptr(), ops._stream()),
              'hfl_window_attention_bwd_split2')
    elif ws is not None:
        check(lib.hfl_window_attention_bwd_det(dqkv.data_ptr(), dp, qkv.data_ptr(), dout.data_ptr(), tok_meta.data_ptr(), tp,
                                               ctypes.byref(desc), ws.data_ptr(), ops._stream()), 'hfl_window_attention_bwd_det')
    else:
        check(lib.hfl_window_attention_bwd(dqkv.data_ptr(), dp, qkv.data_ptr(), dout.data_ptr(), tok_meta.data_ptr(), tp,
                                           ctypes.byref(desc), ops._stream()), 'hfl_window_attention_bwd')


class WindowAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, rpe_table, tok_meta, cfg):
        qkv = qkv.contiguous()
        out = ops.window_attention(qkv, tok_meta, rpe_table, **cfg)
        ctx.save_for_backward(qkv, rpe_table if rpe_table is not None else qkv.new_empty(0), tok_meta)
        ctx.cfg = cfg
        ctx.has_table = rpe_table is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, table, tok_meta = ctx.saved_tensors
        cfg = ctx.cfg
        dout = dout.contiguous()
        dqkv = torch.empty_like(qkv)
        dtable = torch.zeros_like(table) if ctx.has_table else None
        d = _desc(cfg['n_tokens'], cfg['n_windows'], cfg['patch_size'], cfg['dilation'], cfg['n_relay'],
                  cfg['n_heads'], cfg['batch_size'], cfg.get('rt_row0', 0), cfg.get('depth', 0))
        _window_attention_bwd(dqkv, dtable, qkv, dout, tok_meta, table if ctx.has_table else None, d)
        return dqkv, dtable, None, None


def window_attention(qkv, rpe_table, tok_meta, **cfg):
    return WindowAttentionFn.apply(qkv, rpe_table, tok_meta, cfg)


_INV_CACHE = {}


def _inverse_table(neigh, n_src):
    key = (id(neigh), n_src)
    hit = _INV_CACHE.get(key)
    if hit is not None and hit[0]() is neigh:
        return hit[1]
    inv = torch.empty((n_src, neigh.shape[1]), dtype=torch.int32, device=neigh.device)
    check(_native.load().hfl_inverse_table(inv.data_ptr(), n_src, neigh.data_ptr(), neigh.shape[0],
                                           neigh.shape[1], ops._stream()), 'hfl_inverse_table')
    if hit is None:                       # evicted when the gather table dies (a new octree every training batch)
        weakref.finalize(neigh, _INV_CACHE.pop, key, None)
    _INV_CACHE[key] = (weakref.ref(neigh), inv)
    return inv


class OctreeGatherFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, data, neigh):
        ctx.save_for_backward(neigh)
        ctx.n_src, ctx.c = data.shape
        return ops.octree_gather(data, neigh)

    @staticmethod
    def backward(ctx, dcol):
        (neigh,) = ctx.saved_tensors
        inv = _inverse_table(neigh, ctx.n_src)
        dcol = dcol.contiguous()
        ddata = torch.empty((ctx.n_src, ctx.c), dtype=torch.float32, device=dcol.device)
        check(_native.load().hfl_octree_gather_bwd(ddata.data_ptr(), dcol.data_ptr(), inv.data_ptr(),
                                                   ctx.n_src, neigh.shape[1], ctx.c, ops._stream()),
              'hfl_octree_gather_bwd')
        return ddata, None


def octree_gather(data, neigh):
    return OctreeGatherFn.apply(data, neigh)


class TallMmFn(torch.autograd.Function):
    """y = col @ w [+ bias] for a dense-gather octree convolution (model.OctreeConv's fallback: the first stem convolution,
    3 input channels, and the 32 -> 64 stride-2 one -- `ocnn.nn.OctreeConv`'s octree2col + mm, models/layers/octformer_layers.py:
    89-95) with the weight gradient as a split-K product.  Autograd's dW = col^T dy is a (27 Cin, Cout) = (81, 32) or (256, 64)
    output contracted over 0.66-0.87 M rows: the BLAS library runs it on the three to eight workgroups its output tiles give
    (5.5 and 4.6 ms of the 160 ms config-3 step, tools/train_ops_profile.py).  Here the rows are cut into chunks that one
    batched GEMM contracts side by side and a small sum over the chunks finishes (fp32, fixed order)."""

    CHUNK = 4096

    @staticmethod
    def forward(ctx, col, w, bias):
        ctx.save_for_backward(col, w)
        ctx.has_bias = bias is not None
        return torch.addmm(bias, col, w) if bias is not None else torch.mm(col, w)

    @staticmethod
    def backward(ctx, dy):
        col, w = ctx.saved_tensors
        dy = dy.contiguous()
        dcol = dy.mm(w.t()) if ctx.needs_input_grad[0] else None
        dw = None
        if ctx.needs_input_grad[1]:
            n, rows = col.shape[0], TallMmFn.CHUNK
            s = n // rows
            if s >= 2:
                n0 = s * rows
                dw = torch.bmm(col[:n0].view(s, rows, -1).transpose(1, 2), dy[:n0].view(s, rows, -1)).sum(0)
                if n0 < n:
                    dw = dw.addmm_(col[n0:].t(), dy[n0:])
            else:
                dw = col.t().mm(dy)
        db = dy.sum(0) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        return dcol, dw, db


def tall_mm(col, w, bias=None):
    return TallMmFn.apply(col, w, bias)


class LiveTapConvFn(torch.autograd.Function):
    """Octree convolution over its LIVE (row, tap) pairs (model.OctreeConv._forward_live_taps) with its gradients in the
    same form: the output gradient is gathered pair-major, every tap is two small GEMMs (dg_k = dpart_k W_k^T,
    dW_k = g_k^T dpart_k) on its contiguous slice, and the input gradient is the fixed-order slot sum over the pairs that
    read each input row.  Replaces autograd over the dense (N, 27 Cin) gather + GEMM (94 % zeros at depth 6)."""

    @staticmethod
    def forward(ctx, data, weights, octree, depth, kernel, stride):
        src, slot, edges = octree.sparse_taps(depth, kernel, stride)
        kdim, cin, cout = weights.shape
        x6 = _x6_taps_ok(cin, cout) and edges[-1] > 0 and data.dtype == torch.float32
        if x6:
            # one grouped launch at fp32-grade products (hfl_linear_x6_grouped_gather): the tile loader reads the pairs' input
            # rows itself, so the (pairs, Cin) matrix is neither written here nor kept for the backward (it is re-gathered there)
            npad = max(cout, 128)
            part = ops.linear_x6_grouped_gather(data, src, _tap_blocks(weights, True, npad),
                                                octree.tap_tiles(depth, kernel, stride, npad), cout)
            ctx.save_for_backward(data, weights)
        else:
            g = ops.octree_gather(data, src)
            part = torch.empty((g.shape[0], cout), dtype=torch.float32, device=data.device)
            for k in range(kdim):
                if edges[k + 1] > edges[k]:
                    torch.mm(g[edges[k]:edges[k + 1]], weights[k], out=part[edges[k]:edges[k + 1]])
            ctx.save_for_backward(g, weights)
        ctx.octree, ctx.key, ctx.n_src, ctx.x6 = octree, (depth, kernel, stride), data.shape[0], x6
        return ops.slot_sum(part, slot) if _slot_sum_ok(part, slot) else ops.dwconv_forward_backward(part, _unit_taps(kdim, cout, data.device), slot)

    @staticmethod
    def backward(ctx, dout):
        g, weights = ctx.saved_tensors
        src, _, edges = ctx.octree.sparse_taps(*ctx.key)
        rowof, inv_slot, chunks, tap_off = ctx.octree.sparse_taps_bwd(*ctx.key)
        kdim, cin, cout = weights.shape
        dout = dout.contiguous()
        if ctx.x6 and cin % 64 == 0 and cout % 64 == 0:
            # neither pair-major copy exists: the weight-gradient kernel and the grouped GEMM below read the layer input
            # (the saved tensor) and the output gradient through the pair tables
            dw = ops.tap_wgrad(g, dout, chunks, tap_off, kdim, g_rows=src, d_rows=rowof)
            dpart = None
        else:
            if ctx.x6:
                g = ops.octree_gather(g, src)
            dpart = ops.octree_gather(dout, rowof)
        if dpart is None:
            pass
        elif cin % 64 == 0 and cout % 64 == 0:
            dw = ops.tap_wgrad(g, dpart, chunks, tap_off, kdim)       # long contractions into small matrices: own kernel
        else:
            dw = torch.zeros_like(weights)
            for k in range(kdim):
                if edges[k + 1] > edges[k]:
                    torch.mm(g[edges[k]:edges[k + 1]].t(), dpart[edges[k]:edges[k + 1]], out=dw[k])
        ddata = None
        if ctx.needs_input_grad[0]:
            if ctx.x6:
                npad = max(cin, 128)
                dg = ops.linear_x6_grouped_gather(dout, rowof, _tap_blocks(weights, False, npad),
                                                  ctx.octree.tap_tiles(*ctx.key, npad), cin)
            else:
                dg = torch.empty_like(g)
                for k in range(kdim):
                    a, b = edges[k], edges[k + 1]
                    if b > a:
                        torch.mm(dpart[a:b], weights[k].t(), out=dg[a:b])
            ddata = (ops.slot_sum(dg, inv_slot) if _slot_sum_ok(dg, inv_slot)
                     else ops.dwconv_forward_backward(dg, _unit_taps(kdim, cin, dg.device), inv_slot))
        return ddata, dw, None, None, None, None


def _slot_sum_ok(part, slot) -> bool:
    return part.shape[1] % 4 == 0 and part.shape[1] <= 1024 and slot.shape[1] <= 27 and slot.dtype == torch.int32


# The training path's live-tap convolutions run as ONE grouped launch at fp32-grade products (hfl_linear_x6_grouped_gather;
# its error is below the fp32 library GEMM's, so the gradient bar is untouched) where the channel widths allow, else as the
# fp32 per-tap GEMMs.  (The grouped split-precision launch bought 0.6 % of the config-3 step, but the deepest gradient of the
# loss chain -- first stem convolution, amplified by the 1/tau = 100 of the listwise loss -- moved from 8.5e-4 to 2.2e-3 of
# the oracle chain with it; that path has since been removed.)
def _x6_taps_ok(cin, cout) -> bool:
    return cin % 32 == 0 and cout % 32 == 0 and (cout % 128 == 0 or cout == 64) and (cin % 128 == 0 or cin == 64)


def _tap_blocks(weights, transposed: bool, npad: int, pack=ops.x6_pack, kind='taps6'):
    """The three bf16 planes (`ops.x6_pack`; or another `pack` / `kind`: model.OctreeConv's split2 form) of the per-tap
    weight blocks of an octree convolution, every block padded to `npad` rows: transposed = W[k]^T (Cout x Cin) for the
    forward product, else W[k] (Cin x Cout) for the input gradient; rebuilt when the optimizer updates the parameter."""
    def build():
        w = weights.detach()
        blocks = w.transpose(1, 2) if transposed else w                   # (kdim, rows, K)
        kdim, rows, kk = blocks.shape
        if npad > rows:
            blocks = torch.cat([blocks, blocks.new_zeros(kdim, npad - rows, kk)], 1)
        return pack(blocks.reshape(kdim * npad, kk).contiguous())
    return derived((kind, transposed, npad), (weights,), build)


_UNIT_TAPS = {}


def _unit_taps(kdim, channels, device):
    key = (kdim, channels, device.type, device.index)
    if key not in _UNIT_TAPS:
        _UNIT_TAPS[key] = torch.ones((kdim, 1, channels), dtype=torch.float32, device=device)
    return _UNIT_TAPS[key]


def live_tap_conv(data, weights, octree, depth, kernel, stride):
    return LiveTapConvFn.apply(data, weights, octree, depth, kernel, stride)


class RelayTokenInitFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, tok_meta, n_windows, patch_size):
        ctx.save_for_backward(tok_meta)
        ctx.shape = x.shape
        ctx.n_windows, ctx.patch_size = n_windows, patch_size
        return ops.relay_token_init(x, tok_meta, n_windows, patch_size)

    @staticmethod
    def backward(ctx, drt):
        (tok_meta,) = ctx.saved_tensors
        n, c = ctx.shape
        drt = drt.contiguous()
        dx = torch.empty((n, c), dtype=torch.float32, device=drt.device)
        check(_native.load().hfl_relay_token_init_bwd(dx.data_ptr(), drt.data_ptr(), tok_meta.data_ptr(),
                                                      n, ctx.n_windows, ctx.patch_size, c, ops._stream()),
              'hfl_relay_token_init_bwd')
        return dx, None, None, None


def relay_token_init(x, tok_meta, n_windows, patch_size):
    return RelayTokenInitFn.apply(x, tok_meta, n_windows, patch_size)


class RelayAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, seq_rows, seq_off, batch, n_heads, max_seq_len):
        qkv = qkv.contiguous()
        ctx.save_for_backward(qkv, seq_rows, seq_off)
        ctx.cfg = (batch, n_heads, max_seq_len)
        return ops.relay_attention(qkv, seq_rows, seq_off, batch, n_heads, max_seq_len)

    @staticmethod
    def backward(ctx, dout):
        qkv, seq_rows, seq_off = ctx.saved_tensors
        batch, n_heads, max_seq_len = ctx.cfg
        dqkv = torch.zeros_like(qkv)
        check(_native.load().hfl_relay_attention_bwd(
            dqkv.data_ptr(), qkv.data_ptr(), dout.contiguous().data_ptr(), seq_rows.data_ptr(),
            seq_off.data_ptr(), batch, n_heads, 16 ** -0.5, max_seq_len, ops._stream()),
            'hfl_relay_attention_bwd')
        return dqkv, None, None, None, None, None


def relay_attention(qkv, plan, n_heads: int):
    """Ragged relay-token attention, HIP forward and backward."""
    return RelayAttentionFn.apply(qkv, plan.seq_rows, plan.seq_off, plan.B, n_heads, plan.max_seq_len)


# ------------------------------------------------ differentiable torch forms (GPU, tiny ops)
def relay_attention_torch(qkv, plan, n_heads: int):
    """Ragged relay-token attention as padded dense math (training path only): rows of cloud b
    are gathered to (B, Rmax, ...), masked softmax over the real entries, scattered back."""
    B, C = plan.B, n_heads * 16
    idx, valid = plan.relay_pad_index()                       # (B, Rmax) row ids / bool
    x = qkv[idx.clamp(min=0)]                                 # (B, R, 3C)
    q, k, v = x.reshape(B, -1, 3, n_heads, 16).permute(2, 0, 3, 1, 4)
    s = torch.matmul(q, k.transpose(-2, -1)) * (16 ** -0.5)
    s = s.masked_fill(~valid[:, None, None, :], float('-inf'))
    s = s.masked_fill(~valid.any(1)[:, None, None, None], 0.0)     # clouds without relay tokens
    o = torch.matmul(torch.softmax(s, dim=-1), v).transpose(1, 2).reshape(B, -1, C)
    out = qkv.new_zeros((qkv.shape[0], C))
    return out.index_put((idx[valid],), o[valid])


class PadRowsFn(torch.autograd.Function):
    """(B, nmax, C) zero-padded per-cloud copy of ragged rows (hfl_pad_rows); the gradient is the same rows read back -- every
    input row has exactly one padded position -- where autograd over cat + index_select scatters with `index_add_` (2 ms of the
    config-3 step)."""

    @staticmethod
    def forward(ctx, x, row_off, batch, nmax, live):
        ctx.save_for_backward(live)
        return ops.pad_rows(x, row_off, batch, nmax)

    @staticmethod
    def backward(ctx, dxp):
        (live,) = ctx.saved_tensors
        return dxp.reshape(-1, dxp.shape[-1]).index_select(0, live), None, None, None, None


class PoolScoresFn(torch.autograd.Function):
    """scale * query xp^T of the attentional pooling, (k, C) x (B, nmax, C) -> (B, k, nmax).  The query gradient is contracted
    cloud by cloud (one batched product + a fixed-order sum over the clouds): autograd's single (k, B nmax) x (B nmax, C)
    product runs on the handful of workgroups its (k, C) output gives (1.2 ms)."""

    @staticmethod
    def forward(ctx, query, xp, scale):
        ctx.save_for_backward(query, xp)
        ctx.scale = scale
        return torch.matmul(query.unsqueeze(0), xp.transpose(1, 2)) * scale

    @staticmethod
    def backward(ctx, ds):
        query, xp = ctx.saved_tensors
        ds = ds * ctx.scale
        dq = torch.bmm(ds, xp).sum(0) if ctx.needs_input_grad[0] else None
        dxp = torch.matmul(ds.transpose(1, 2), query) if ctx.needs_input_grad[1] else None
        return dq, dxp, None


def attentional_pooling_torch(x, query, plan, depth: int, scale: float):
    """learned-query pooling over each cloud's tokens (training path): padded dense math."""
    idx = plan.pad_index[depth]
    B = plan.B
    valid = (idx != x.shape[0]).view(B, -1)
    if x.is_cuda and x.dtype == torch.float32 and x.shape[1] % 4 == 0:
        live = plan.__dict__.setdefault('_pad_live', {}).get(depth)
        if live is None:                       # padded position of every row (clouds are contiguous row ranges); no host sync
            off = plan.cloud_off[depth]
            rows = torch.arange(x.shape[0], device=x.device)
            cloud = torch.searchsorted(off[1:].contiguous(), rows, right=True)
            live = plan.__dict__['_pad_live'][depth] = rows + cloud * valid.shape[1] - off[cloud]
        xp = PadRowsFn.apply(x, plan.cloud_off[depth], B, valid.shape[1], live)
        s = PoolScoresFn.apply(query, xp, scale)
    else:
        xp = torch.cat([x, x.new_zeros(1, x.shape[1])], 0).index_select(0, idx).view(B, -1, x.shape[1])
        s = torch.matmul(query.unsqueeze(0), xp.transpose(1, 2)) * scale          # (B, k, Nmax)
    s = s.masked_fill(~valid[:, None, :], float('-inf'))
    return torch.matmul(torch.softmax(s, dim=-1), xp)


# ------------------------------------------------ split-precision Linear with HIP/hipBLASLt backward
def _weight_image(kind, pack, weight, transposed: bool):
    """`pack` of a Linear weight, or of its transpose for dx = dy W: one `weight_cache` entry per (kind, orientation),
    rebuilt when the optimizer updates the parameter (a checkpointed block's recomputation finds it), released with it."""
    return derived((kind, transposed), (weight,),
                   lambda: pack(weight.detach().t().contiguous() if transposed else weight.detach()))


def _w3_cached(weight, transposed: bool):
    return _weight_image('split3', ops.split_weight, weight, transposed)


class LinearSplitFn(torch.autograd.Function):
    """y = x W^T + b with every product evaluated as the 3-term bf16 split (fp32 accumulate): forward
    `hfl_gemm_bf16`, dx = dy W through the same entry point on the transposed weight split, dW = dy^T x
    through `hfl_gemm_bf16_tn` on row-stacked splits.  Same accuracy class as the inference path
    (4e-6 per GEMM) at ~2x the fp32 hipBLASLt rate."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        shape = x.shape
        x2 = x.reshape(-1, shape[-1])
        ctx.save_for_backward(x2, weight)
        ctx.has_bias = bias is not None
        ctx.shape = shape
        y = ops.gemm_bf16(ops.split3(x2), _w3_cached(weight, False), bias=bias)
        return y.view(*shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, weight = ctx.saved_tensors
        dy2 = dy.reshape(-1, weight.shape[0]).contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = ops.gemm_bf16(ops.split3(dy2), _w3_cached(weight, True)).view(ctx.shape)
        if ctx.needs_input_grad[1]:
            dw = ops.gemm_bf16_tn(ops.stack3(dy2, 'hhl'), ops.stack3(x2, 'hlh'))
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = dy2.sum(0)
        return dx, dw, db


def linear_split(x, weight, bias=None):
    return LinearSplitFn.apply(x, weight, bias)


# ------------------------------------------------ Linear / MLP on the hand-written GEMMs, one set of Functions for two families:
# X3 = split precision (csrc/gemm_x3.hip: three-term bf16 split, fp32 accumulation, 4e-6 per GEMM; operands are "split2" rows,
# same bytes as the f32 rows), X6 = matched precision of GEMM mode x6 (csrc/gemm_x6.hip: three bf16 planes per operand, six
# plane products, fp32 accumulation -- fp32 grade; operands are the f32 rows themselves)
def _w2_cached(weight, transposed: bool):
    """split2 layout of a Linear weight (or of its transpose, for dx = dy W).  model._w2 shares the entry and builds it with
    `ops.split2_weight` (torch arithmetic): the two builders are bit-identical (torch.equal over every Linear weight, both
    orientations, of the wild-places and cs-wild-places models, default and synthetic weights: 746 of 746 on an MI355X)."""
    return _weight_image('x3', ops.split2, weight, transposed)


def _w6_cached(weight, transposed: bool):
    """The three bf16 planes (`ops.x6_pack`) of a Linear weight, or of its transpose for dx = dy W."""
    return _weight_image('x6', ops.x6_pack, weight, transposed)


def linear_x3_ok(in_features: int, out_features: int) -> bool:
    """Shapes the hand-written GEMM takes in both directions (forward: K % 32, N % 128; dx: N % 32, K % 128)."""
    return in_features % 128 == 0 and out_features % 128 == 0


def linear_x6_ok(in_features: int, out_features: int) -> bool:
    """Shapes `hfl_linear_x6` takes in both directions (forward and dx = dy W) and `hfl_wgrad_f32` takes for dW."""
    return (in_features % 128 == 0 and out_features % 128 == 0 and ops.linear_x6_ok(in_features, out_features)
            and ops.linear_x6_ok(out_features, in_features))


def _scaled_rows(t, row_scale=None):
    return t if row_scale is None else t * row_scale.unsqueeze(1)


class GemmFamily(NamedTuple):
    """The seven operations a training Function is written in; the Functions never ask which family they were given."""
    operand: Callable       # (f32 rows, row_scale or None) -> GEMM operand of the rows [times their per-row factor]
    ln_operand: Callable    # (f32 rows, gamma, beta, eps) -> GEMM operand of LayerNorm(rows)
    weight: Callable        # (weight, transposed) -> cached weight image
    linear: Callable        # (operand, weight image, bias=, residual=, row_scale=) -> f32 rows
    gelu_fwd: Callable      # (operand, weight image, bias) -> (operand of gelu(pre-activation), f32 pre-activation)
    gelu_bwd: Callable      # (operand of dy, image of W^T, pre-activation) -> operand of (dy W) * gelu'(pre-activation)
    wgrad: Callable         # (operand of dy, operand of x, with_bias=) -> (dW, db), fixed reduction order


X3 = GemmFamily(ops.split2, ops.layer_norm_split2, _w2_cached, ops.linear_x3, ops.linear_x3_gelu_fwd,
                ops.linear_x3_gelu_bwd, ops.wgrad_x3)
X6 = GemmFamily(_scaled_rows, ops.layer_norm, _w6_cached, ops.linear_x6, ops.linear_x6_gelu_fwd,
                ops.linear_x6_gelu_bwd, ops.wgrad_f32)


def _wgrad(fam: GemmFamily, dy, x, need_w: bool, need_b: bool):
    """(dW, db) through `hfl_wgrad_x3` / `hfl_wgrad_f32`, or (None, None) without a launch when neither is wanted (frozen
    layers)."""
    if not (need_w or need_b):
        return None, None
    dw, db = fam.wgrad(dy, x, with_bias=need_b)
    return (dw if need_w else None), db


class LinearFn(torch.autograd.Function):
    """y = x W^T + b on the hand-written kernels: forward and dx = dy W on `hfl_linear_x3` / `hfl_linear_x6`, dW = dy^T x
    and db on `hfl_wgrad_x3` / `hfl_wgrad_f32` (fp32 MFMA).  What is kept for the backward is the GEMM operand of x (X3: its
    split2 form, same bytes as x; X6: x itself).  The X6 forward is the x6 inference launch, with or without autograd.
    Zero rows: zeros out, zero gradients, no launch."""

    @staticmethod
    def forward(ctx, fam, x, weight, bias):
        shape = x.shape
        x2 = x.reshape(-1, shape[-1]).contiguous()
        ctx.fam, ctx.has_bias, ctx.shape = fam, bias is not None, shape
        if x2.shape[0] == 0:
            ctx.save_for_backward(None, weight)
            return x.new_zeros(*shape[:-1], weight.shape[0])
        xs = fam.operand(x2, None)
        ctx.save_for_backward(xs, weight)
        return fam.linear(xs, fam.weight(weight, False), bias=bias).view(*shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, dy):
        xs, weight = ctx.saved_tensors
        fam = ctx.fam
        if xs is None:
            return (None, torch.zeros(ctx.shape, device=dy.device), torch.zeros_like(weight),
                    torch.zeros(weight.shape[0], device=dy.device) if ctx.has_bias else None)
        dys = fam.operand(dy.reshape(-1, weight.shape[0]).contiguous(), None)
        need = ctx.needs_input_grad                    # (fam, x, weight, bias)
        dx = fam.linear(dys, fam.weight(weight, True)).view(ctx.shape) if need[1] else None
        dw, db = _wgrad(fam, dys, xs, need[2], ctx.has_bias and need[3])
        return None, dx, dw, db


def linear_x3(x, weight, bias=None):
    return LinearFn.apply(X3, x, weight, bias)


def linear_x6(x, weight, bias=None):
    return LinearFn.apply(X6, x, weight, bias)


class MlpFn(torch.autograd.Function):
    """fc2(gelu(fc1(h))) of a transformer block (models/layers/octformer_layers.py:53-59) with no element-wise pass of its
    own: fc1 writes the operand of gelu(.) and the pre-activation in one launch (hfl_linear_x3_gelu_fwd /
    hfl_linear_x6_gelu_fwd), the backward's dx GEMM of fc2 multiplies by gelu'(pre-activation) in its epilogue and writes the
    operand of fc1's gradient GEMMs directly.  The X6 forward is bitwise the x6 inference MLP (MLP.forward)."""

    @staticmethod
    def forward(ctx, fam, h, w1, b1, w2, b2):
        shape = h.shape
        hs = fam.operand(h.reshape(-1, shape[-1]).contiguous(), None)
        gs, pre = fam.gelu_fwd(hs, fam.weight(w1, False), b1)
        ctx.save_for_backward(hs, gs, pre, w1, w2)
        ctx.fam, ctx.shape = fam, shape
        return fam.linear(gs, fam.weight(w2, False), bias=b2).view(*shape[:-1], w2.shape[0])

    @staticmethod
    def backward(ctx, dout):
        hs, gs, pre, w1, w2 = ctx.saved_tensors
        fam = ctx.fam
        dys = fam.operand(dout.reshape(-1, w2.shape[0]).contiguous(), None)
        dps = fam.gelu_bwd(dys, fam.weight(w2, True), pre)
        need = ctx.needs_input_grad                    # (fam, h, w1, b1, w2, b2)
        dw2, db2 = _wgrad(fam, dys, gs, need[4], need[5])
        dh = fam.linear(dps, fam.weight(w1, True)).view(ctx.shape) if need[1] else None
        dw1, db1 = _wgrad(fam, dps, hs, need[2], need[3])
        return None, dh, dw1, db1, dw2, db2


def mlp_x3(h, w1, b1, w2, b2):
    return MlpFn.apply(X3, h, w1, b1, w2, b2)


def mlp_x6(h, w1, b1, w2, b2):
    return MlpFn.apply(X6, h, w1, b1, w2, b2)


class LnMlpResidualFn(torch.autograd.Function):
    """x + s * fc2(gelu(fc1(LN(x)))): the whole pre-norm MLP branch of a transformer block (models/octformer_backbone.py:
    275-278; s = the per-row stochastic-depth factor of OctreeDropPath or None) as three launches forward (LN -> operand,
    fc1 + GELU, fc2 + bias + scale + residual) and seven backward; no element-wise pass: LayerNorm writes the GEMM operand,
    the residual add rides in fc2's epilogue, the skip path's gradient joins inside the LayerNorm backward kernel."""

    @staticmethod
    def forward(ctx, fam, x, gamma, beta, eps, w1, b1, w2, b2, row_scale):
        shape = x.shape
        x2 = x.reshape(-1, shape[-1]).contiguous()
        hs = fam.ln_operand(x2, gamma, beta, eps)
        gs, pre = fam.gelu_fwd(hs, fam.weight(w1, False), b1)
        ctx.save_for_backward(x2, gamma, hs, gs, pre, w1, w2, row_scale if row_scale is not None else x2.new_empty(0))
        ctx.fam, ctx.shape, ctx.eps, ctx.scaled = fam, shape, eps, row_scale is not None
        return fam.linear(gs, fam.weight(w2, False), bias=b2, residual=x2, row_scale=row_scale).view(shape)

    @staticmethod
    def backward(ctx, dout):
        x2, gamma, hs, gs, pre, w1, w2, row_scale = ctx.saved_tensors
        fam = ctx.fam
        dout2 = dout.reshape(-1, w2.shape[0]).contiguous()
        dys = fam.operand(dout2, row_scale if ctx.scaled else None)
        dps = fam.gelu_bwd(dys, fam.weight(w2, True), pre)
        need = ctx.needs_input_grad                    # (fam, x, gamma, beta, eps, w1, b1, w2, b2, row_scale)
        dw2, db2 = _wgrad(fam, dys, gs, need[7], need[8])
        dw1, db1 = _wgrad(fam, dps, hs, need[5], need[6])
        if not (need[1] or need[2] or need[3]):
            return None, None, None, None, None, dw1, db1, dw2, db2, None
        dh = fam.linear(dps, fam.weight(w1, True))
        dx, dg, dbeta = ops.layer_norm_bwd(dh, x2, gamma, ctx.eps, dres=dout2)
        return (None, dx.view(ctx.shape), dg if need[2] else None, dbeta if need[3] else None, None, dw1, db1, dw2, db2,
                None)


def ln_mlp_residual_x3(x, gamma, beta, eps, w1, b1, w2, b2, row_scale=None):
    return LnMlpResidualFn.apply(X3, x, gamma, beta, eps, w1, b1, w2, b2, row_scale)


def ln_mlp_residual_x6(x, gamma, beta, eps, w1, b1, w2, b2, row_scale=None):
    return LnMlpResidualFn.apply(X6, x, gamma, beta, eps, w1, b1, w2, b2, row_scale)


class LnAttnResidualX3Fn(torch.autograd.Function):
    """x + proj(window_attention(qkv(LN(x)))): the pre-norm attention branch of a transformer block
    (models/octformer_backbone.py:59-93,275-278; layer scale and stochastic depth off) without element-wise passes:
    LayerNorm writes the qkv GEMM's operand, the attention kernel writes the proj GEMM's operand, the residual add rides in
    proj's epilogue, and in the backward the skip gradient joins inside the LayerNorm backward kernel."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, wqkv, bqkv, rpe_table, tok_meta, cfg, wp, bp, row_scale):
        shape = x.shape
        x2 = x.reshape(-1, shape[-1]).contiguous()
        hs = ops.layer_norm_split2(x2, gamma, beta, eps)
        qkv = ops.linear_x3(hs, _w2_cached(wqkv, False), bias=bqkv)
        os_ = ops.window_attention(qkv, tok_meta, rpe_table, out_split=2, **cfg)
        ctx.save_for_backward(x2, gamma, hs, qkv, os_, rpe_table if rpe_table is not None else x2.new_empty(0), tok_meta,
                              wqkv, wp, row_scale if row_scale is not None else x2.new_empty(0))
        ctx.shape, ctx.eps, ctx.cfg, ctx.has_table, ctx.has_qkv_bias = shape, eps, cfg, rpe_table is not None, bqkv is not None
        ctx.scaled = row_scale is not None
        return ops.linear_x3(os_, _w2_cached(wp, False), bias=bp, residual=x2, row_scale=row_scale).view(shape)

    @staticmethod
    def backward(ctx, dout):
        x2, gamma, hs, qkv, os_, table, tok_meta, wqkv, wp, row_scale = ctx.saved_tensors
        cfg = ctx.cfg
        dout2 = dout.reshape(-1, wp.shape[0]).contiguous()
        dys = ops.split2(dout2, row_scale if ctx.scaled else None)
        need = ctx.needs_input_grad    # (x, gamma, beta, eps, wqkv, bqkv, rpe_table, tok_meta, cfg, wp, bp, row_scale)
        do = ops.linear_x3(dys, _w2_cached(wp, True))
        dwp, dbp = _wgrad(X3, dys, os_, need[9], need[10])
        dtable = torch.zeros_like(table) if ctx.has_table else None
        d = _desc(cfg['n_tokens'], cfg['n_windows'], cfg['patch_size'], cfg['dilation'], cfg['n_relay'],
                  cfg['n_heads'], cfg['batch_size'], cfg.get('rt_row0', 0), cfg.get('depth', 0))
        # the attention backward writes dqkv as the split2 operand of the two GEMMs below (no f32 gradient, no split pass)
        dqs = torch.empty((qkv.shape[0], 2 * qkv.shape[1]), dtype=torch.bfloat16, device=qkv.device)
        _window_attention_bwd(dqs, dtable, qkv, do, tok_meta, table if ctx.has_table else None, d, split=True)
        if cfg['n_relay']:
            # relay rows of pure-padding windows are in no window: the kernel leaves them unwritten, the GEMMs below read them
            live = cfg.get('rt_row0', 0) + -(-cfg['n_tokens'] // cfg['patch_size'])
            if live < dqs.shape[0]:
                dqs[live:].zero_()
        dh = ops.linear_x3(dqs, _w2_cached(wqkv, True))
        dwqkv, dbqkv = _wgrad(X3, dqs, hs, need[4], ctx.has_qkv_bias and need[5])
        dx, dg, dbeta = ops.layer_norm_bwd(dh, x2, gamma, ctx.eps, dres=dout2)
        return (dx.view(ctx.shape), dg if need[1] else None, dbeta if need[2] else None, None, dwqkv, dbqkv,
                dtable if need[6] else None, None, None, dwp, dbp, None)


def ln_attn_residual_x3(x, gamma, beta, eps, wqkv, bqkv, rpe_table, tok_meta, cfg, wp, bp, row_scale=None):
    return LnAttnResidualX3Fn.apply(x, gamma, beta, eps, wqkv, bqkv, rpe_table, tok_meta, cfg, wp, bp, row_scale)


# ------------------------------------------------ conditional position encoding, training forward as one launch
class CpeFn(torch.autograd.Function):
    """[x +] LayerNorm(dwconv(x)) (CPE.forward and its callers' residual: models/layers/octformer_layers.py:138-142,
    models/octformer_backbone.py:258) with the inference path's fused launch as the forward -- it additionally writes the
    convolution's output, which is all the backward needs besides x: LayerNorm backward (hfl_layer_norm_bwd), the data
    gradient of the convolution through the inverse neighbour table and its weight gradient (libs/dwconv/dwconv/nn.py:31-43),
    and the skip connection's gradient added to the data gradient.  Replaces three launches (dwconv, LayerNorm, add) and two
    saved tensors' worth of passes in every block's forward."""

    @staticmethod
    def forward(ctx, x, weights, gamma, beta, neigh, residual, eps):
        x = x.contiguous()
        conv = torch.empty_like(x)
        out = ops.cpe_forward(x, weights, gamma, beta, neigh, residual, eps, conv_out=conv)
        ctx.save_for_backward(x, conv, weights, gamma, neigh)
        ctx.residual, ctx.eps = bool(residual), eps
        return out

    @staticmethod
    def backward(ctx, dout):
        from .dwconv import _inverse_of
        x, conv, weights, gamma, neigh = ctx.saved_tensors
        need = ctx.needs_input_grad                    # (x, weights, gamma, beta, neigh, residual, eps)
        dout = dout.contiguous()
        dconv, dg, dbeta = ops.layer_norm_bwd(dout, conv, gamma, ctx.eps)
        dx = None
        if need[0] and x.shape[1] in (32, 64, 128, 256) and neigh.dtype == torch.int32:
            # the same gather as the forward, over the inverse table, the skip gradient added in its epilogue
            dx = ops.dwconv_add(dconv, weights, _inverse_of(neigh), dout if ctx.residual else None)
        elif need[0]:
            dx = ops.dwconv_forward_backward(dconv, weights.contiguous(), _inverse_of(neigh))
            if ctx.residual:
                dx += dout
        dw = ops.dwconv_weight_backward(dconv, x, neigh) if need[1] else None
        return dx, dw, (dg if need[2] else None), (dbeta if need[3] else None), None, None, None


def cpe(x, weights, gamma, beta, neigh, residual: bool, eps: float):
    return CpeFn.apply(x, weights, gamma, beta, neigh, residual, eps)


class CpeBufferFn(torch.autograd.Function):
    """new = [ tokens + LayerNorm(dwconv(tokens)) | relay rows ] of a pyramid level's [tokens | relay rows] buffer: what
    `torch.cat([cpe(buf[:nt]), relay], 0)` computes at the head of every HOTFormer block (models/hotformerloc_backbone.py:
    197-205), with the CPE launch writing the token rows of the new buffer itself.  The backward writes the token rows' gradient
    straight into the buffer's gradient: autograd over the slices and the concatenation made two zero-filled full-size
    gradients, two copies and an add per block (1.5 ms of the config-3 step) besides the concatenation's copy."""

    @staticmethod
    def forward(ctx, buf, relay, weights, gamma, beta, neigh, nt, eps):
        buf = buf.contiguous()
        new = torch.empty_like(buf)
        conv = torch.empty((nt, buf.shape[1]), dtype=torch.float32, device=buf.device)
        ops.cpe_forward(buf[:nt], weights, gamma, beta, neigh, True, eps, out=new[:nt], conv_out=conv)
        new[nt:].copy_(buf[nt:] if relay is None else relay)
        ctx.save_for_backward(buf, conv, weights, gamma, neigh)
        ctx.nt, ctx.eps, ctx.has_relay = nt, eps, relay is not None
        return new

    @staticmethod
    def backward(ctx, dnew):
        from .dwconv import _inverse_of
        buf, conv, weights, gamma, neigh = ctx.saved_tensors
        need = ctx.needs_input_grad                    # (buf, relay, weights, gamma, beta, neigh, nt, eps)
        nt = ctx.nt
        dnew = dnew.contiguous()
        dtok = dnew[:nt]
        dconv, dg, dbeta = ops.layer_norm_bwd(dtok, conv, gamma, ctx.eps)
        dbuf = None
        if need[0]:
            dbuf = torch.empty_like(buf)
            ops.dwconv_add(dconv, weights, _inverse_of(neigh), dtok, out=dbuf[:nt])
            if ctx.has_relay:
                dbuf[nt:].zero_()                       # the buffer's old relay rows were replaced
            else:
                dbuf[nt:].copy_(dnew[nt:])
        drelay = dnew[nt:] if (ctx.has_relay and need[1]) else None
        dw = ops.dwconv_weight_backward(dconv, buf[:nt], neigh) if need[2] else None
        return dbuf, drelay, dw, (dg if need[3] else None), (dbeta if need[4] else None), None, None, None


def cpe_buffer(buf, relay, weights, gamma, beta, neigh, nt: int, eps: float):
    return CpeBufferFn.apply(buf, relay, weights, gamma, beta, neigh, nt, eps)


# ------------------------------------------------ LayerNorm with HIP forward and backward
class LayerNormFn(torch.autograd.Function):
    """LayerNorm over the channel axis: `hfl_layer_norm` forward (keeps only its input), `hfl_layer_norm_bwd` backward.
    Replaces F.layer_norm + native_layer_norm_backward on the training path (14 % of the config-3 step in torch)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        ctx.save_for_backward(x, weight)
        ctx.eps = eps
        return ops.layer_norm(x, weight, bias, eps)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dx, dg, db = ops.layer_norm_bwd(dy, x, weight, ctx.eps)
        return dx, dg, db, None


def layer_norm(x, weight, bias, eps: float = 1e-5):
    return LayerNormFn.apply(x, weight, bias, eps)
