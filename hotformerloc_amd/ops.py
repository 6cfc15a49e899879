"""Torch-facing wrappers over the C-ABI: tensors in, tensors out, current stream.

PyTorch is plumbing here (device memory + streams): every function hands raw
device pointers to libhotformerloc_hip.so on `torch.cuda.current_stream()` and
never synchronises.  Inputs must live on the GPU -- there is no CPU path.
"""

import ctypes
import weakref

import numpy as np
import torch

from . import _native
from ._native import WindowAttnDesc, check


# torch.cuda.current_stream() / current_device() cost ~8 us / ~1 us of Python per call (device-index normalisation, lazy-init
# checks) and every launch wrapper needs both: 3.4 ms of a 9.9 ms host issue budget per forward.  The raw C hooks are the ones
# torch's own compiled-kernel launchers use.
_RAW_STREAM = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_RAW_DEVICE = getattr(torch._C, '_cuda_getDevice', None)


def _current_device() -> int:
    return _RAW_DEVICE() if _RAW_DEVICE is not None else torch.cuda.current_device()


def _stream():
    if _RAW_STREAM is not None and _RAW_DEVICE is not None:
        return ctypes.c_void_p(_RAW_STREAM(_RAW_DEVICE()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class KernelTimer:
    """Optional per-launch HIP-event timing on the launch stream (bench.py roofline leg).
    `with KernelTimer() as t: ...; t.summary()` -> {kernel: (launches, ms, algorithmic bytes, flops, moved bytes)};
    "algorithmic" = SURVEY.md section 8(d)'s per-unit figure, "moved" = what this implementation actually
    reads + writes when that differs (e.g. the duplicated bf16 `hi` plane of a split output)."""
    active = None

    def __init__(self, only=None):
        self.records = []
        self.only = None if only is None else frozenset(only)     # time just these kernels (cheap: 2 events each)

    def __enter__(self):
        KernelTimer.active = self
        return self

    def __exit__(self, *exc):
        KernelTimer.active = None

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1, nbytes, flops, moved in self.records:
            n, ms, b, f, mv = out.get(name, (0, 0.0, 0, 0, 0))
            out[name] = (n + 1, ms + e0.elapsed_time(e1), b + nbytes, f + flops, mv + moved)
        return out

    def by_size(self, name):
        """Launches of one kernel grouped by their algorithmic byte count: [(bytes per launch, launches, total ms)],
        largest first (a step's window-attention launches span 9 MB .. 280 MB: the small ones are latency-bound)."""
        torch.cuda.synchronize()
        groups = {}
        for n, e0, e1, nbytes, flops, moved in self.records:
            if n == name:
                c, ms = groups.get(nbytes, (0, 0.0))
                groups[nbytes] = (c + 1, ms + e0.elapsed_time(e1))
        return [(b, c, ms) for b, (c, ms) in sorted(groups.items(), reverse=True)]


class _timed:
    def __init__(self, name, nbytes, flops=0, moved=None):
        self.t = KernelTimer.active
        if self.t is not None and self.t.only is not None and name not in self.t.only:
            self.t = None
        if self.t is not None:
            self.name, self.nbytes, self.flops = name, int(nbytes), int(flops)
            self.moved = int(nbytes if moved is None else moved)

    def __enter__(self):
        if self.t is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if self.t is not None:
            self.e1.record()
            self.t.records.append((self.name, self.e0, self.e1, self.nbytes, self.flops, self.moved))


def _dev(*tensors):
    """Every operand on the GPU, and on the CURRENT device: launches go to `torch.cuda.current_stream()` and the
    library's hipBLASLt state is per (device, stream), so a tensor of another GPU would be read through the wrong
    context.  Use `with torch.cuda.device(t.device):` around the model for a second GPU in one process."""
    cur = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise _native.NativeLibraryError(
                'hotformerloc_amd ops need GPU tensors (got %s); there is no CPU fallback' % t.device)
        if cur is None:
            cur = _current_device()
        if t.device.index != cur:
            raise _native.NativeLibraryError(
                'tensor on %s but the current device is cuda:%d; wrap the call in torch.cuda.device(...)'
                % (t.device, cur))


def _f32c(t):
    if t.dtype != torch.float32:
        raise TypeError('float32 expected, got %s' % t.dtype)
    return t.contiguous()


def _idx(neigh):
    if neigh.dtype == torch.int64:
        return neigh.contiguous(), 1
    if neigh.dtype == torch.int32:
        return neigh.contiguous(), 0
    raise TypeError('neighbour table must be int32 or int64, got %s' % neigh.dtype)


# ------------------------------------------------------------------ dwconv.core API
def dwconv_forward_backward(data: torch.Tensor, weight: torch.Tensor, neigh: torch.Tensor):
    """libs/dwconv/csrc/dwconv.h:13 -- data (N,C), weight (K,1,C), neigh (M,K) -> (M,C)."""
    _dev(data, weight, neigh)
    data, weight = _f32c(data), _f32c(weight)
    neigh, i64 = _idx(neigh)
    m, k = neigh.shape
    c = data.shape[1]
    out = torch.empty((m, c), dtype=torch.float32, device=data.device)
    check(_native.load().hfl_dwconv_forward_backward(
        out.data_ptr(), data.data_ptr(), weight.data_ptr(), neigh.data_ptr(), i64, m, c, k,
        _stream()), 'hfl_dwconv_forward_backward')
    return out


def dwconv_add(data: torch.Tensor, weight: torch.Tensor, neigh: torch.Tensor, add=None, out=None):
    """dwconv(data, weight, neigh) [+ add] through the CPE kernel's gather (hfl_dwconv_add): int32 table, C in {32, 64, 128,
    256}; the data gradient of CPE (neigh = the inverse table, add = the skip connection's gradient).  `out`: a preallocated
    contiguous (m, C) f32 view to write to (not `data`: the kernel gathers)."""
    _dev(data, weight, neigh, add, out)
    data, weight = _f32c(data), _f32c(weight)
    assert neigh.dtype == torch.int32 and neigh.is_contiguous()
    m, k = neigh.shape
    c = data.shape[1]
    if out is None:
        out = torch.empty((m, c), dtype=torch.float32, device=data.device)
    else:
        assert tuple(out.shape) == (m, c) and out.is_contiguous() and out.dtype == torch.float32
        assert out.data_ptr() != data.data_ptr()
    if add is not None:
        add = _f32c(add)
        assert tuple(add.shape) == (m, c)
    check(_native.load().hfl_dwconv_add(out.data_ptr(), data.data_ptr(), weight.data_ptr(), neigh.data_ptr(),
                                        None if add is None else add.data_ptr(), m, c, k, _stream()), 'hfl_dwconv_add')
    return out


def slot_sum(part: torch.Tensor, slot: torch.Tensor, bias=None):
    """out[h] = sum of part[slot[h, k]] over the row's live slots [+ bias] (hfl_slot_sum): the per-row sum of the partial
    products of a live-tap octree convolution.  part (P, C) f32, slot (n_out, K) int32 (-1 = none)."""
    _dev(part, slot, bias)
    part = _f32c(part)
    assert slot.dtype == torch.int32 and slot.is_contiguous() and slot.dim() == 2
    n, k = slot.shape
    c = part.shape[1]
    out = torch.empty((n, c), dtype=torch.float32, device=part.device)
    check(_native.load().hfl_slot_sum(out.data_ptr(), part.data_ptr(), slot.data_ptr(),
                                      None if bias is None else _f32c(bias).data_ptr(), n, c, k, _stream()), 'hfl_slot_sum')
    return out


_SLOT_NORM_CHANNELS = (32, 64, 128, 256)


def slot_sum_norm(part: torch.Tensor, slot: torch.Tensor, bias, weight, norm_bias, eps: float = 1e-5, relu: bool = False,
                  split2: bool = False):
    """[relu](LN(slot_sum(part, slot, bias))) in the slot sum's own pass (hfl_slot_sum_norm): fp32 rows, or -- `split2` -- the
    bf16 split2 operand (rows, 2C) of the next convolution's GEMM.  C in _SLOT_NORM_CHANNELS; bit for bit `slot_sum` followed
    by `layer_norm` / `layer_norm_relu`."""
    _dev(part, slot, bias, weight, norm_bias)
    part = _f32c(part)
    assert slot.dtype == torch.int32 and slot.is_contiguous() and slot.dim() == 2
    n, k = slot.shape
    c = part.shape[1]
    if split2:
        out = torch.empty((n, 2 * c), dtype=torch.bfloat16, device=part.device)
    else:
        out = torch.empty((n, c), dtype=torch.float32, device=part.device)
    check(_native.load().hfl_slot_sum_norm(None if split2 else out.data_ptr(), out.data_ptr() if split2 else None,
                                           part.data_ptr(), slot.data_ptr(), None if bias is None else _f32c(bias).data_ptr(),
                                           _f32c(weight).data_ptr(), _f32c(norm_bias).data_ptr(), n, c, k, float(eps),
                                           int(bool(relu)), _stream()), 'hfl_slot_sum_norm')
    return out


def dwconv_weight_backward(grad: torch.Tensor, data: torch.Tensor, neigh: torch.Tensor):
    """libs/dwconv/csrc/dwconv.h:14 -- -> (K,1,C)."""
    _dev(grad, data, neigh)
    grad, data = _f32c(grad), _f32c(data)
    neigh, i64 = _idx(neigh)
    n, k = neigh.shape
    c = data.shape[1]
    lib = _native.load()
    ws = torch.empty(int(lib.hfl_dwconv_weight_backward_workspace(n, c, k)), dtype=torch.uint8,
                     device=data.device)
    out = torch.empty((k, 1, c), dtype=torch.float32, device=data.device)
    check(lib.hfl_dwconv_weight_backward(out.data_ptr(), grad.data_ptr(), data.data_ptr(),
                                         neigh.data_ptr(), i64, n, c, k, ws.data_ptr(), _stream()),
          'hfl_dwconv_weight_backward')
    return out


def inverse_neigh(neigh: torch.Tensor):
    """libs/dwconv/csrc/dwconv.h:15."""
    _dev(neigh)
    neigh, i64 = _idx(neigh)
    out = torch.empty_like(neigh)
    check(_native.load().hfl_inverse_neigh(out.data_ptr(), neigh.data_ptr(), i64, neigh.shape[0],
                                           neigh.shape[1], _stream()), 'hfl_inverse_neigh')
    return out


def cpe_forward(x, weight, gamma, beta, neigh, residual: bool, eps: float = 1e-5, out=None, conv_out=None):
    """out = [x +] LayerNorm(dwconv(x, weight, neigh)) * gamma + beta (fused).  `out` may be a
    preallocated contiguous (n, C) view (e.g. the token rows of a larger buffer); `conv_out` (n, C) f32, optional:
    receives dwconv(x) (the training forward keeps it for the LayerNorm backward: hfl_cpe_forward_save)."""
    _dev(x, weight, gamma, beta, neigh, conv_out)
    x = _f32c(x)
    assert neigh.dtype == torch.int32 and neigh.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    else:
        assert out.shape == x.shape and out.is_contiguous() and out.dtype == torch.float32
        assert out.data_ptr() != x.data_ptr(), 'CPE gathers neighbours: cannot run in place'
    n, c = x.shape
    # algorithmic bytes: read x once, write out once, read the int32 neighbour rows
    with _timed('hfl_cpe_forward', n * c * 8 + n * neigh.shape[1] * 4, 2 * neigh.shape[1] * n * c):
        if conv_out is not None:
            assert conv_out.shape == x.shape and conv_out.is_contiguous() and conv_out.dtype == torch.float32
            check(_native.load().hfl_cpe_forward_save(
                out.data_ptr(), conv_out.data_ptr(), x.data_ptr(), _f32c(weight).data_ptr(), _f32c(gamma).data_ptr(),
                _f32c(beta).data_ptr(), neigh.data_ptr(), n, c, neigh.shape[1],
                float(eps), int(bool(residual)), _stream()), 'hfl_cpe_forward_save')
            return out
        check(_native.load().hfl_cpe_forward(
            out.data_ptr(), x.data_ptr(), _f32c(weight).data_ptr(), _f32c(gamma).data_ptr(),
            _f32c(beta).data_ptr(), neigh.data_ptr(), n, c, neigh.shape[1],
            float(eps), int(bool(residual)), _stream()), 'hfl_cpe_forward')
    return out


# ---------------------------------------------------------------------- layer norm
_LN_CHANNELS = (16, 32, 64, 128, 256, 512, 1024)


def layer_norm(x, weight, bias, eps: float = 1e-5):
    """LayerNorm over the last axis of a (..., C) fp32 tensor (HIP kernel, one pass)."""
    _dev(x, weight, bias)
    c = x.shape[-1]
    xc = _f32c(x)
    out = torch.empty_like(xc)                  # not a view: autograd Functions return it as it is
    with _timed('hfl_layer_norm', xc.numel() * 8):
        check(_native.load().hfl_layer_norm(out.data_ptr(), xc.data_ptr(), weight.data_ptr(),
                                            bias.data_ptr(), xc.numel() // c, c, float(eps), _stream()),
              'hfl_layer_norm')
    return out


def layer_norm_bwd(dy, x, weight, eps: float = 1e-5, dres=None):
    """(dx, dgamma, dbeta) of LayerNorm over the last axis (hfl_layer_norm_bwd; statistics recomputed from x); with
    `dres` the gradient of a skip connection around the normalised branch is added to dx in the same pass."""
    _dev(dy, x, weight, dres)
    c = x.shape[-1]
    x2, dy2 = _f32c(x).view(-1, c), _f32c(dy).view(-1, c)
    lib = _native.load()
    nb = int(lib.hfl_layer_norm_bwd_blocks(x2.shape[0], c))
    if nb <= 0:
        raise _native.NativeLibraryError('hfl_layer_norm_bwd: unsupported channel count %d' % c)
    dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    part = torch.empty((2, nb, c), dtype=torch.float32, device=x.device)
    check(lib.hfl_layer_norm_bwd_add(dx.data_ptr(), part[0].data_ptr(), part[1].data_ptr(), dy2.data_ptr(), x2.data_ptr(),
                                     _f32c(weight).data_ptr(), None if dres is None else _f32c(dres).data_ptr(),
                                     x2.shape[0], c, float(eps), _stream()), 'hfl_layer_norm_bwd')
    dgb = torch.empty((2, c), dtype=torch.float32, device=x.device)
    check(lib.hfl_layer_norm_bwd_finalize(dgb[0].data_ptr(), dgb[1].data_ptr(), part[0].data_ptr(), part[1].data_ptr(),
                                          nb, c, _stream()), 'hfl_layer_norm_bwd_finalize')
    return dx, dgb[0], dgb[1]


def add_layer_norm(x, y, weight, bias, eps: float = 1e-5, add_bias=None, inplace: bool = False):
    """(x + y [+ add_bias], LN(x + y [+ add_bias])) in one pass over the rows."""
    _dev(x, y, weight, bias, add_bias)
    c = x.shape[-1]
    x2, y2 = _f32c(x).view(-1, c), _f32c(y).view(-1, c)
    xo = x2 if inplace else torch.empty_like(x2)
    h = torch.empty_like(x2)
    with _timed('hfl_add_layer_norm', x2.numel() * 16):
        check(_native.load().hfl_add_layer_norm(
            xo.data_ptr(), h.data_ptr(), x2.data_ptr(), y2.data_ptr(),
            None if add_bias is None else add_bias.data_ptr(), weight.data_ptr(), bias.data_ptr(),
            x2.shape[0], c, float(eps), _stream()), 'hfl_add_layer_norm')
    return xo.view(x.shape), h.view(x.shape)


# ------------------------------------------------------- split-precision Linear path
def _a3(rows, c, device):
    return torch.empty((rows, 3 * c), dtype=torch.bfloat16, device=device)


def layer_norm_split3(x, weight, bias, eps: float = 1e-5):
    """A3 = [hi | hi | lo] bf16 of LN(x): the A operand of `split_mm` (header section 9)."""
    _dev(x, weight, bias)
    c = x.shape[-1]
    x2 = _f32c(x).view(-1, c)
    out = _a3(x2.shape[0], c, x.device)
    with _timed('hfl_layer_norm_split3', x2.numel() * 10):
        check(_native.load().hfl_layer_norm_split3(out.data_ptr(), x2.data_ptr(), weight.data_ptr(),
                                                   bias.data_ptr(), x2.shape[0], c, float(eps),
                                                   _stream()), 'hfl_layer_norm_split3')
    return out


def add_layer_norm_split3(x, y, weight, bias, eps: float = 1e-5, add_bias=None):
    """(x + y [+ add_bias] as fp32, split3(LN(that)))."""
    _dev(x, y, weight, bias, add_bias)
    c = x.shape[-1]
    x2, y2 = _f32c(x).view(-1, c), _f32c(y).view(-1, c)
    xo = torch.empty_like(x2)
    h = _a3(x2.shape[0], c, x.device)
    with _timed('hfl_add_layer_norm_split3', x2.numel() * 18):
        check(_native.load().hfl_add_layer_norm_split3(
            xo.data_ptr(), h.data_ptr(), x2.data_ptr(), y2.data_ptr(),
            None if add_bias is None else add_bias.data_ptr(), weight.data_ptr(), bias.data_ptr(),
            x2.shape[0], c, float(eps), _stream()), 'hfl_add_layer_norm_split3')
    return xo.view(x.shape), h


def add_bias(x, y, bias=None):
    """x + y + bias (fp32), one pass."""
    _dev(x, y, bias)
    c = x.shape[-1]
    x2, y2 = _f32c(x).view(-1, c), _f32c(y).view(-1, c)
    out = torch.empty_like(x2)
    with _timed('hfl_add_bias', x2.numel() * 12):
        check(_native.load().hfl_add_bias(out.data_ptr(), x2.data_ptr(), y2.data_ptr(),
                                          None if bias is None else bias.data_ptr(), x2.shape[0], c,
                                          _stream()), 'hfl_add_bias')
    return out.view(x.shape)


def bias_gelu_split3(x, bias=None):
    """split3(gelu(x + bias)) with the exact (erf) GELU."""
    _dev(x, bias)
    c = x.shape[-1]
    x2 = _f32c(x).view(-1, c)
    out = _a3(x2.shape[0], c, x.device)
    with _timed('hfl_bias_gelu_split3', x2.numel() * 10):
        check(_native.load().hfl_bias_gelu_split3(out.data_ptr(), x2.data_ptr(),
                                                  None if bias is None else bias.data_ptr(),
                                                  x2.shape[0], c, _stream()), 'hfl_bias_gelu_split3')
    return out


def split3(x):
    _dev(x)
    c = x.shape[-1]
    x2 = _f32c(x).view(-1, c)
    out = _a3(x2.shape[0], c, x.device)
    check(_native.load().hfl_split3(out.data_ptr(), x2.data_ptr(), x2.shape[0], c, _stream()),
          'hfl_split3')
    return out


def split_weight(w: torch.Tensor) -> torch.Tensor:
    """(N, K) fp32 Linear weight -> W3 = [w_hi | w_lo | w_hi] bf16 (N, 3K)."""
    w = w.detach().float()
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    return torch.cat([hi, lo, hi], dim=1).contiguous()


def split_mm(a3: torch.Tensor, w3: torch.Tensor) -> torch.Tensor:
    """fp32 (rows, N) = A3 @ W3^T: one hipBLASLt bf16 GEMM, fp32 accumulate and output,
    computing x_hi w_hi + x_hi w_lo + x_lo w_hi."""
    return torch.mm(a3, w3.t(), out_dtype=torch.float32)


def gemm_bf16(a3: torch.Tensor, w3: torch.Tensor, bias=None, residual=None, out=None) -> torch.Tensor:
    """fp32 (rows, N) = A3 @ W3^T [+ bias] [+ residual] in one hipBLASLt launch (hfl_gemm_bf16): the
    Linear + bias + residual add of a transformer block without a pass over the residual stream."""
    _dev(a3, w3, bias, residual)
    assert a3.dtype == torch.bfloat16 and w3.dtype == torch.bfloat16 and a3.is_contiguous() and w3.is_contiguous()
    m, k = a3.shape
    n = w3.shape[0]
    assert w3.shape[1] == k
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=a3.device)
    else:
        assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (m, n)
    if residual is not None:
        residual = _f32c(residual)
        assert tuple(residual.shape) == (m, n)
    check(_native.load().hfl_gemm_bf16(out.data_ptr(), a3.data_ptr(), w3.data_ptr(),
                                       None if bias is None else _f32c(bias).data_ptr(),
                                       None if residual is None else residual.data_ptr(), m, n, k, _stream()),
          'hfl_gemm_bf16')
    return out


# ------------------------------------------- hand-written split-precision Linear (csrc/gemm_x3.hip)
def split2(x, row_scale=None):
    """fp32 (rows, C) [* row_scale (rows)] -> split2 bf16 (rows, 2C): per 32-channel block [32 x hi | 32 x lo]
    (hfl_split2 / hfl_split2_rows)."""
    _dev(x, row_scale)
    c = x.shape[-1]
    x2 = _f32c(x).view(-1, c)
    out = torch.empty((x2.shape[0], 2 * c), dtype=torch.bfloat16, device=x.device)
    check(_native.load().hfl_split2_rows(out.data_ptr(), x2.data_ptr(),
                                         None if row_scale is None else _f32c(row_scale).data_ptr(), x2.shape[0], c,
                                         _stream()), 'hfl_split2')
    return out


def layer_norm_split2(x, weight, bias, eps: float = 1e-5):
    """split2(LN(x)): the operand of `linear_x3` (hfl_layer_norm_split2)."""
    _dev(x, weight, bias)
    c = x.shape[-1]
    x2 = _f32c(x).view(-1, c)
    out = torch.empty((x2.shape[0], 2 * c), dtype=torch.bfloat16, device=x.device)
    with _timed('hfl_layer_norm_split2', x2.numel() * 8):
        check(_native.load().hfl_layer_norm_split2(out.data_ptr(), x2.data_ptr(), weight.data_ptr(),
                                                   bias.data_ptr(), x2.shape[0], c, float(eps),
                                                   _stream()), 'hfl_layer_norm_split2')
    return out


def layer_norm_relu(x, weight, bias, eps: float = 1e-5, split2: bool = False):
    """relu(LN(x)) in one pass (hfl_layer_norm_relu): fp32 rows, or -- `split2` -- the bf16 split2 operand (rows, 2C) of the
    next convolution's GEMM."""
    _dev(x, weight, bias)
    c = x.shape[-1]
    x2 = _f32c(x).view(-1, c)
    if split2:
        out = torch.empty((x2.shape[0], 2 * c), dtype=torch.bfloat16, device=x.device)
    else:
        out = torch.empty_like(x2)
    if x2.shape[0] == 0:
        return out
    with _timed('hfl_layer_norm_relu', x2.numel() * 8):
        check(_native.load().hfl_layer_norm_relu(None if split2 else out.data_ptr(), out.data_ptr() if split2 else None,
                                                 x2.data_ptr(), weight.data_ptr(), bias.data_ptr(), x2.shape[0], c,
                                                 float(eps), _stream()), 'hfl_layer_norm_relu')
    return out


def split2_weight(w: torch.Tensor) -> torch.Tensor:
    """(N, K) fp32 Linear weight -> split2 bf16 (N, 2K) (host-side layout, once per parameter)."""
    w = w.detach().float()
    n, k = w.shape
    assert k % 32 == 0
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    return torch.stack([hi.view(n, k // 32, 32), lo.view(n, k // 32, 32)], dim=2).reshape(n, 2 * k).contiguous()


def linear_x3(x2: torch.Tensor, w2: torch.Tensor, bias=None, residual=None, gelu_split_out: bool = False,
              out=None, row_scale=None) -> torch.Tensor:
    """y = x W^T [+ bias] [+ residual] (fp32), or with gelu_split_out the split2 bf16 operand of the next Linear,
    split2(gelu(x W^T + bias)); x2 / w2 are split2 operands (hfl_linear_x3)."""
    _dev(x2, w2, bias, *(residual if isinstance(residual, (list, tuple)) else (residual,)))
    assert x2.dtype == torch.bfloat16 and w2.dtype == torch.bfloat16 and x2.is_contiguous() and w2.is_contiguous()
    m, k2 = x2.shape
    n = w2.shape[0]
    assert w2.shape[1] == k2 and k2 % 64 == 0
    k = k2 // 2
    if gelu_split_out:
        assert residual is None
        if out is None:
            out = torch.empty((m, 2 * n), dtype=torch.bfloat16, device=x2.device)
    else:
        if out is None:
            out = torch.empty((m, n), dtype=torch.float32, device=x2.device)
        if isinstance(residual, (list, tuple)):       # the residual rows in several arrays (hfl_linear_x3_seg)
            assert row_scale is None
            seg, rows = row_segments(residual)
            assert rows == m and residual[0].shape[1] == n
            with _timed('hfl_linear_x3', m * k * 4 + m * n * 8, 2 * m * k * n):
                check(_native.load().hfl_linear_x3_seg(out.data_ptr(), x2.data_ptr(), w2.data_ptr(),
                                                       None if bias is None else _f32c(bias).data_ptr(), ctypes.byref(seg),
                                                       m, k, n, _stream()), 'hfl_linear_x3_seg')
            return out
        if residual is not None:
            residual = _f32c(residual)
            assert tuple(residual.shape) == (m, n)
    # algorithmic bytes: x once (4 B/elt), out once (4 B/elt either form), residual once; 2 M K N flop (fp32-equivalent)
    with _timed('hfl_linear_x3', m * k * 4 + m * n * (8 if residual is not None else 4), 2 * m * k * n):
        if row_scale is not None:          # (acc + bias) * row_scale[m] + residual: stochastic depth of a fused branch
            assert not gelu_split_out and tuple(row_scale.shape) == (m,)
            check(_native.load().hfl_linear_x3_rows(out.data_ptr(), x2.data_ptr(), w2.data_ptr(),
                                                    None if bias is None else _f32c(bias).data_ptr(),
                                                    None if residual is None else residual.data_ptr(),
                                                    _f32c(row_scale).data_ptr(), m, k, n, _stream()), 'hfl_linear_x3_rows')
            return out
        check(_native.load().hfl_linear_x3(out.data_ptr(), x2.data_ptr(), w2.data_ptr(),
                                           None if bias is None else _f32c(bias).data_ptr(),
                                           None if residual is None else residual.data_ptr(), m, k, n,
                                           int(bool(gelu_split_out)), _stream()), 'hfl_linear_x3')
    return out


def x6_pack(w: torch.Tensor) -> torch.Tensor:
    """(N, K) fp32 Linear weight -> its three bf16 planes (3, N, Kp) for `linear_x6` (hfl_linear_x6_pack, once per parameter;
    Kp = K rounded up to a multiple of 64, zero-padded)."""
    _dev(w)
    wc = _f32c(w.detach())
    n, k = wc.shape
    assert k % 32 == 0 and n % 128 == 0
    w3 = torch.empty((3, n, (k + 63) // 64 * 64), dtype=torch.bfloat16, device=w.device)
    check(_native.load().hfl_linear_x6_pack(w3.data_ptr(), wc.data_ptr(), n, k, _stream()), 'hfl_linear_x6_pack')
    return w3


def linear_x6_ok(in_features: int, out_features: int) -> bool:
    return in_features % 32 == 0 and out_features % 128 == 0 and 2 * (in_features + 32) * out_features < 2 ** 31


def linear_x6(x: torch.Tensor, w3: torch.Tensor, bias=None, residual=None, gelu: bool = False, out=None,
              row_scale=None) -> torch.Tensor:
    """y = x W^T [+ bias] [gelu] [* row_scale] [+ residual], fp32 in and out, fp32-grade products (hfl_linear_x6: three
    bf16 planes per operand, six plane products with fp32 accumulation).  x (M, K) f32, w3 = x6_pack(W)."""
    _dev(x, w3, bias, residual, row_scale)
    assert w3.dtype == torch.bfloat16 and w3.is_contiguous() and w3.dim() == 3 and w3.shape[0] == 3
    xc = _f32c(x)
    m, k = xc.shape
    n = w3.shape[1]
    assert w3.shape[2] == (k + 63) // 64 * 64
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=x.device)
    else:
        assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (m, n)
    if residual is not None:
        residual = _f32c(residual)
        assert tuple(residual.shape) == (m, n)
    if row_scale is not None:
        row_scale = _f32c(row_scale)
        assert tuple(row_scale.shape) == (m,)
    with _timed('hfl_linear_x6', m * k * 4 + m * n * (8 if residual is not None else 4), 2 * m * k * n):
        check(_native.load().hfl_linear_x6(out.data_ptr(), xc.data_ptr(), w3.data_ptr(),
                                           None if bias is None else _f32c(bias).data_ptr(),
                                           None if residual is None else residual.data_ptr(),
                                           None if row_scale is None else row_scale.data_ptr(), m, k, n, int(bool(gelu)),
                                           _stream()), 'hfl_linear_x6')
    return out


def linear_x6_gelu_fwd(x: torch.Tensor, w3: torch.Tensor, bias):
    """(gelu(x W^T + b), x W^T + b) in one launch (hfl_linear_x6_gelu_fwd): the training forward of fc1 at matched precision.
    The first is bitwise `linear_x6(x, w3, bias, gelu=True)`, the second bitwise `linear_x6(x, w3, bias)`."""
    _dev(x, w3, bias)
    assert w3.dtype == torch.bfloat16 and w3.is_contiguous() and w3.dim() == 3 and w3.shape[0] == 3
    xc = _f32c(x)
    m, k = xc.shape
    n = w3.shape[1]
    assert w3.shape[2] == (k + 63) // 64 * 64
    out = torch.empty((m, n), dtype=torch.float32, device=x.device)
    pre = torch.empty((m, n), dtype=torch.float32, device=x.device)
    with _timed('hfl_linear_x6', m * k * 4 + m * n * 8, 2 * m * k * n):
        check(_native.load().hfl_linear_x6_gelu_fwd(out.data_ptr(), pre.data_ptr(), xc.data_ptr(), w3.data_ptr(),
                                                    None if bias is None else _f32c(bias).data_ptr(), m, k, n, _stream()),
              'hfl_linear_x6_gelu_fwd')
    return out, pre


def linear_x6_gelu_bwd(dy: torch.Tensor, wt3: torch.Tensor, preact: torch.Tensor) -> torch.Tensor:
    """(dy W) * gelu'(preact) (hfl_linear_x6_gelu_bwd): wt3 = x6_pack(W^T), preact (rows, wt3.shape[1]) f32."""
    _dev(dy, wt3, preact)
    assert wt3.dtype == torch.bfloat16 and wt3.is_contiguous() and wt3.dim() == 3 and wt3.shape[0] == 3
    dyc, pre = _f32c(dy), _f32c(preact)
    m, k = dyc.shape
    n = wt3.shape[1]
    assert wt3.shape[2] == (k + 63) // 64 * 64 and tuple(pre.shape) == (m, n)
    out = torch.empty((m, n), dtype=torch.float32, device=dy.device)
    with _timed('hfl_linear_x6', m * k * 4 + m * n * 8, 2 * m * k * n):
        check(_native.load().hfl_linear_x6_gelu_bwd(out.data_ptr(), dyc.data_ptr(), wt3.data_ptr(), pre.data_ptr(), m, k, n,
                                                    _stream()), 'hfl_linear_x6_gelu_bwd')
    return out


def linear_x6_grouped_gather(x: torch.Tensor, src: torch.Tensor, w3: torch.Tensor, tiles: torch.Tensor,
                             out_features: int) -> torch.Tensor:
    """The per-tap products of an octree convolution over its live (row, tap) pairs at matched precision: row m of the
    operand is x[src[m]] (x (n_src, Cin) f32), tiles (n_tiles, 3) int32 as `linear_x3_grouped`, w3 = x6_pack of the stacked
    per-tap weight blocks (each padded to a multiple of 128 rows); returns (len(src), out_features) f32."""
    _dev(x, src, w3, tiles)
    xc = _f32c(x)
    assert src.dtype == torch.int32 and src.is_contiguous() and tiles.dtype == torch.int32 and tiles.is_contiguous()
    assert w3.dtype == torch.bfloat16 and w3.is_contiguous() and w3.dim() == 3 and w3.shape[0] == 3
    k = xc.shape[1]
    assert w3.shape[2] == (k + 63) // 64 * 64
    m = src.shape[0]
    out = torch.empty((m, out_features), dtype=torch.float32, device=x.device)
    with _timed('hfl_linear_x6', m * k * 4 + m * out_features * 4, 2 * m * k * out_features):
        check(_native.load().hfl_linear_x6_grouped_gather(out.data_ptr(), xc.data_ptr(), src.data_ptr(), w3.data_ptr(),
                                                          w3.shape[1], tiles.data_ptr(), tiles.shape[0], m, k, out_features,
                                                          _stream()), 'hfl_linear_x6_grouped_gather')
    return out


def linear_x3_gelu_fwd(x2: torch.Tensor, w2: torch.Tensor, bias):
    """(split2(gelu(x W^T + b)), x W^T + b as f32) in one launch (hfl_linear_x3_gelu_fwd): training forward of fc1."""
    _dev(x2, w2, bias)
    assert x2.dtype == torch.bfloat16 and w2.dtype == torch.bfloat16 and x2.is_contiguous() and w2.is_contiguous()
    m, k2 = x2.shape
    n = w2.shape[0]
    assert w2.shape[1] == k2
    out = torch.empty((m, 2 * n), dtype=torch.bfloat16, device=x2.device)
    pre = torch.empty((m, n), dtype=torch.float32, device=x2.device)
    with _timed('hfl_linear_x3', m * (k2 // 2) * 4 + m * n * 8, 2 * m * (k2 // 2) * n):
        check(_native.load().hfl_linear_x3_gelu_fwd(out.data_ptr(), pre.data_ptr(), x2.data_ptr(), w2.data_ptr(),
                                                    None if bias is None else _f32c(bias).data_ptr(), m, k2 // 2, n,
                                                    _stream()), 'hfl_linear_x3_gelu_fwd')
    return out, pre


def linear_x3_gelu_bwd(dy2: torch.Tensor, wt2: torch.Tensor, preact: torch.Tensor):
    """split2((dy W) * gelu'(preact)) (hfl_linear_x3_gelu_bwd): wt2 = split2 of W^T, preact (rows, wt2.shape[0]) f32."""
    _dev(dy2, wt2, preact)
    assert dy2.dtype == torch.bfloat16 and wt2.dtype == torch.bfloat16 and dy2.is_contiguous() and wt2.is_contiguous()
    m, k2 = dy2.shape
    n = wt2.shape[0]
    assert wt2.shape[1] == k2 and tuple(preact.shape) == (m, n) and preact.is_contiguous()
    out = torch.empty((m, 2 * n), dtype=torch.bfloat16, device=dy2.device)
    with _timed('hfl_linear_x3', m * (k2 // 2) * 4 + m * n * 8, 2 * m * (k2 // 2) * n):
        check(_native.load().hfl_linear_x3_gelu_bwd(out.data_ptr(), dy2.data_ptr(), wt2.data_ptr(), preact.data_ptr(),
                                                    m, k2 // 2, n, _stream()), 'hfl_linear_x3_gelu_bwd')
    return out


def linear_x3_grouped(x2: torch.Tensor, w2: torch.Tensor, tiles: torch.Tensor, out_features: int) -> torch.Tensor:
    """One launch of the split-precision GEMM over row tiles with different weight blocks (hfl_linear_x3_grouped):
    x2 (rows, 2K) split2, w2 (blocks * Npad, 2K) split2, tiles (n, 3) int32 {first row, rows, first weight row};
    returns (rows, out_features) f32."""
    _dev(x2, w2, tiles)
    assert x2.dtype == torch.bfloat16 and w2.dtype == torch.bfloat16 and x2.is_contiguous() and w2.is_contiguous()
    assert tiles.dtype == torch.int32 and tiles.is_contiguous() and tiles.shape[1] == 3 and w2.shape[1] == x2.shape[1]
    m, k = x2.shape[0], x2.shape[1] // 2
    out = torch.empty((m, out_features), dtype=torch.float32, device=x2.device)
    with _timed('hfl_linear_x3', m * k * 4 + m * out_features * 4, 2 * m * k * out_features):
        check(_native.load().hfl_linear_x3_grouped(out.data_ptr(), x2.data_ptr(), w2.data_ptr(), tiles.data_ptr(),
                                                   tiles.shape[0], m, k, out_features, _stream()), 'hfl_linear_x3_grouped')
    return out


def linear_x3_grouped_gather(x2: torch.Tensor, src: torch.Tensor, w2: torch.Tensor, tiles: torch.Tensor,
                             out_features: int) -> torch.Tensor:
    """`linear_x3_grouped` over the rows x2[src[m]] without materialising them (hfl_linear_x3_grouped_gather): x2 (N, 2K) split2
    input rows of an octree convolution, src (P) or (P, 1) int32 the input row of every live pair; returns (P, out_features)."""
    _dev(x2, src, w2, tiles)
    assert x2.dtype == torch.bfloat16 and w2.dtype == torch.bfloat16 and x2.is_contiguous() and w2.is_contiguous()
    assert tiles.dtype == torch.int32 and tiles.is_contiguous() and tiles.shape[1] == 3 and w2.shape[1] == x2.shape[1]
    assert src.dtype == torch.int32 and src.is_contiguous()
    m, k = src.numel(), x2.shape[1] // 2
    out = torch.empty((m, out_features), dtype=torch.float32, device=x2.device)
    with _timed('hfl_linear_x3', m * k * 4 + m * out_features * 4, 2 * m * k * out_features):
        check(_native.load().hfl_linear_x3_grouped_gather(out.data_ptr(), x2.data_ptr(), src.data_ptr(), x2.shape[0],
                                                          w2.data_ptr(), tiles.data_ptr(), tiles.shape[0], m, k, out_features,
                                                          _stream()), 'hfl_linear_x3_grouped_gather')
    return out


def mlp_fused_ok(channels: int) -> bool:
    """Channel widths `ln_mlp_fused` takes (hfl_mlp_fused_pack_bytes > 0)."""
    return int(_native.load().hfl_mlp_fused_pack_bytes(int(channels))) > 0


def mlp_fused_shape_ok(channels: int, hidden: int) -> bool:
    return int(_native.load().hfl_mlp_fused_pack_bytes_h(int(channels), int(hidden))) > 0


def mlp_fused_pack(w1: torch.Tensor, w2: torch.Tensor) -> torch.Tensor:
    """Weight image of `ln_mlp_fused` from the fp32 Linear weights fc1 (H, C) and fc2 (C, H) (hfl_mlp_fused_pack_h): the
    (hi, lo) bf16 split of both, cut into the 32-hidden-feature stages the kernel streams through LDS.  Once per parameter.
    H = 4C (C = 128, 256: transformer blocks) or H = C = 256 (Mixer layers)."""
    _dev(w1, w2)
    w1, w2 = _f32c(w1.detach()), _f32c(w2.detach())
    h, c = w1.shape
    assert tuple(w2.shape) == (c, h)
    lib = _native.load()
    n = int(lib.hfl_mlp_fused_pack_bytes_h(c, h))
    if n <= 0:
        raise _native.NativeLibraryError('hfl_mlp_fused_pack: unsupported shape C = %d, hidden = %d' % (c, h))
    pack = torch.empty(n, dtype=torch.uint8, device=w1.device)
    check(lib.hfl_mlp_fused_pack_h(pack.data_ptr(), w1.data_ptr(), w2.data_ptr(), c, h, _stream()), 'hfl_mlp_fused_pack_h')
    return pack


def ln_mlp_fused(x, gamma, beta, eps: float, pack, b1, b2, out=None):
    """out = x + fc2(gelu(fc1(LN(x)) + b1)) + b2 in ONE launch (hfl_ln_mlp_fused_h); `pack` from `mlp_fused_pack`; the hidden
    width is the length of b1."""
    _dev(x, gamma, beta, pack, b1, b2)
    x = _f32c(x)
    m, c = x.shape
    h = b1.numel()
    if out is None:
        out = torch.empty_like(x)
    else:
        assert out.shape == x.shape and out.dtype == torch.float32 and out.is_contiguous()
    assert out.data_ptr() != x.data_ptr(), 'the residual rows are re-read: cannot run in place'
    # algorithmic bytes: read x, write out (the LayerNorm input doubles as the residual); 2 * 2 * M * C * H flop
    lib = _native.load()
    assert pack.numel() == int(lib.hfl_mlp_fused_pack_bytes_h(c, h)), 'pack does not belong to this (C, hidden)'
    ws_bytes = int(lib.hfl_ln_mlp_fused_workspace_h(m, c, h))   # partial sums of the rows left over after the last whole round
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes > 0 else None
    with _timed('hfl_ln_mlp_fused', m * c * 8, 4 * m * c * h):
        check(lib.hfl_ln_mlp_fused_h(out.data_ptr(), x.data_ptr(), _f32c(gamma).data_ptr(), _f32c(beta).data_ptr(),
                                     float(eps), pack.data_ptr(), _f32c(b1).data_ptr(), _f32c(b2).data_ptr(), m, c, h,
                                     ws.data_ptr() if ws is not None else None, ws_bytes, _stream()), 'hfl_ln_mlp_fused_h')
    return out


class BlockCall:
    """One transformer block of the inference path through the native call hfl_block_forward_x3 (CPE -> [relay rows] -> LN1 ->
    qkv -> window attention -> proj + residual -> LN2 -> fc1 + GELU -> fc2 + residual); `weights` = a filled
    `_native.BlockWeights` (model._native_block_forms), `keep_alive` the tensors its pointers refer to.
    The same block in two phases (hfl_block_io.phase, named in `_native`): `run(PHASE_TOKENS)` issues what reads token rows
    only (CPE, their LN1 and qkv projection) -- the caller may do that while the relay-token self-attention of the iteration is
    still running on another stream -- `run(PHASE_REST, relay)` the rest, on whatever stream is current at that call;
    `run(PHASE_WHOLE, relay)` = both.  `run(PHASE_RELAY_QKV, relay)` / `block_attention_multi([...])` / `run(PHASE_TAIL)` split
    PHASE_REST around the window attention, so that the attention of several blocks goes out as one launch.  Which
    attention launches the call uses is `weights.fuse_attention` (FUSE_ATTN_NO_RELAY, FUSE_ATTN_WS)."""

    def __init__(self, weights, keep_alive, x_in, neigh, tok_meta, n_tokens: int, desc: WindowAttnDesc):
        _dev(x_in, neigh, tok_meta)
        rows, c = x_in.shape
        self.lib = _native.load()
        self.weights, self.keep, self.desc = weights, (keep_alive, x_in, neigh, tok_meta), desc
        self.out = torch.empty((rows, c), dtype=torch.float32, device=x_in.device)
        self.arena = torch.empty(int(self.lib.hfl_block_forward_x3_arena(rows, c)), dtype=torch.uint8, device=x_in.device)
        self.io = _native.BlockIO(x_in=x_in.data_ptr(), relay=None, out=self.out.data_ptr(), arena=self.arena.data_ptr(),
                                  neigh=neigh.data_ptr(), tok_meta=tok_meta.data_ptr(), n_rows=rows, n_tokens=n_tokens,
                                  phase=_native.PHASE_WHOLE)

    def run(self, phase: int, relay=None):
        if relay is not None:           # (stays set for the later phases of the call: PHASE_TAIL's proj reads the relay rows)
            _dev(relay)
            assert relay.dtype == torch.float32 and relay.is_contiguous()
            self.keep = self.keep + (relay,)
            self.io.relay = relay.data_ptr()
        self.io.phase = phase
        check(self.lib.hfl_block_forward_x3(ctypes.byref(self.weights), ctypes.byref(self.io), ctypes.byref(self.desc),
                                            _stream()), 'hfl_block_forward_x3')
        return self.out


def block_attention_multi(calls):
    """The window attention of several blocks that have run `BlockCall.run(PHASE_TOKENS)` and `.run(PHASE_RELAY_QKV, relay)`, as
    one launch when their attention shapes agree (hfl_block_attention_x3_multi); `.run(PHASE_TAIL)` of each block follows."""
    n = len(calls)
    assert 1 <= n <= 4
    lib = _native.load()
    ws = _native.ptr_array([ctypes.addressof(c.weights) for c in calls])
    ios = _native.ptr_array([ctypes.addressof(c.io) for c in calls])
    ds = _native.ptr_array([ctypes.addressof(c.desc) for c in calls])
    check(lib.hfl_block_attention_x3_multi(n, ws, ios, ds, _stream()), 'hfl_block_attention_x3_multi')


def row_segments(parts):
    """hfl_row_segments of the row-wise concatenation of `parts` (1..4 contiguous f32 (rows_i, C) tensors): (struct, rows)."""
    assert 1 <= len(parts) <= 4
    _dev(*parts)
    seg = _native.RowSegments()
    seg.n = len(parts)
    r = 0
    for i, t in enumerate(parts):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape[1] == parts[0].shape[1]
        seg.ptr[i], seg.row0[i] = t.data_ptr(), r
        r += t.shape[0]
    return seg, r


def relay_block_pack(w_qkv, w_proj, w_fc1, w_fc2) -> torch.Tensor:
    """Weight image of the one-launch relay-token block (hfl_relay_block_pack) from the fp32 Linear weights qkv (3C, C), proj
    (C, C), fc1 (4C, C), fc2 (C, 4C), C = 256: the bf16 (hi, lo) split of `split2_weight`, cut into the 16-feature x 32-k MFMA
    fragments a wave loads whole.  Once per parameter set."""
    _dev(w_qkv, w_proj, w_fc1, w_fc2)
    ws = [_f32c(w.detach()) for w in (w_qkv, w_proj, w_fc1, w_fc2)]
    c = ws[1].shape[0]
    assert [tuple(w.shape) for w in ws] == [(3 * c, c), (c, c), (4 * c, c), (c, 4 * c)]
    lib = _native.load()
    n = int(lib.hfl_relay_block_pack_bytes(c))
    if n <= 0:
        raise _native.NativeLibraryError('hfl_relay_block_pack: unsupported channel count %d' % c)
    pack = torch.empty(n, dtype=torch.uint8, device=ws[0].device)
    check(lib.hfl_relay_block_pack(pack.data_ptr(), *(w.data_ptr() for w in ws), c, _stream()), 'hfl_relay_block_pack')
    return pack


def _relay_block_io(rt, seq_rows, seq_off, batch, max_seq_len, orphan_rows):
    """(hfl_relay_block_io with a fresh `out`, out, what the struct points to) for the relay-token block calls."""
    seg = None
    if isinstance(rt, (list, tuple)):
        seg, rows = row_segments(rt)
        c, dev, x_ptr = rt[0].shape[1], rt[0].device, None
    else:
        _dev(rt)
        (rows, c), dev, x_ptr = rt.shape, rt.device, rt.data_ptr()
    _dev(seq_rows, seq_off, orphan_rows)
    out = torch.empty((rows, c), dtype=torch.float32, device=dev)
    io = _native.RelayBlockIO(x_in=x_ptr, x_segments=None if seg is None else ctypes.addressof(seg),
                              out=out.data_ptr(), arena=None, seq_rows=seq_rows.data_ptr(),
                              seq_off=seq_off.data_ptr(), n_rows=rows, batch=batch, max_seq_len=max_seq_len,
                              orphan_rows=None if orphan_rows is None or orphan_rows.numel() == 0 else orphan_rows.data_ptr(),
                              n_orphans=0 if orphan_rows is None else orphan_rows.numel())
    return io, out, (seg, rt)


def relay_block_fused_x3(weights, keep_alive, rt, seq_rows, seq_off, batch: int, max_seq_len: int, orphan_rows=None):
    """The relay-token transformer block (RTSA) of the inference path as ONE launch (hfl_relay_block_fused_x3, no arena), or
    None when hfl_relay_block_fused_ok refuses the problem (it takes C = 256, 16 heads, weights.relay_pack, at most 64 relay
    tokens per cloud).  rt as in `relay_block_forward_x3`."""
    lib = _native.load()
    io, out, _keep = _relay_block_io(rt, seq_rows, seq_off, batch, max_seq_len, orphan_rows)
    if not lib.hfl_relay_block_fused_ok(ctypes.byref(weights), ctypes.byref(io)):
        return None
    check(lib.hfl_relay_block_fused_x3(ctypes.byref(weights), ctypes.byref(io), _stream()), 'hfl_relay_block_fused_x3')
    return out


def relay_block_forward_x3(weights, keep_alive, rt, seq_rows, seq_off, batch: int, max_seq_len: int, orphan_rows=None,
                           fused: bool = True):
    """The relay-token transformer block (RTSA) of the inference path in ONE native call.  rt: the (rows, C) relay rows, or a
    list of up to four tensors whose row-wise concatenation they are (the pyramid levels' relay rows where the levels left
    them: needs weights.qkv_pack).  With `fused`, the one launch of `relay_block_fused_x3` where it applies; otherwise the five
    launches of hfl_relay_block_forward_x3."""
    if fused:
        out = relay_block_fused_x3(weights, keep_alive, rt, seq_rows, seq_off, batch, max_seq_len, orphan_rows)
        if out is not None:
            return out
    lib = _native.load()
    io, out, _keep = _relay_block_io(rt, seq_rows, seq_off, batch, max_seq_len, orphan_rows)
    arena = torch.empty(int(lib.hfl_relay_block_forward_x3_arena(io.n_rows, out.shape[1])), dtype=torch.uint8, device=out.device)
    io.arena = arena.data_ptr()
    check(lib.hfl_relay_block_forward_x3(ctypes.byref(weights), ctypes.byref(io), _stream()), 'hfl_relay_block_forward_x3')
    return out


def wgrad_x3(dy2: torch.Tensor, x2: torch.Tensor, with_bias: bool = False):
    """(dW, db) of y = x W^T + b from split2 operands: dW (N, K) = dy^T x, db (N) = dy summed over rows (hfl_wgrad_x3;
    fixed reduction order)."""
    _dev(dy2, x2)
    assert dy2.dtype == torch.bfloat16 and x2.dtype == torch.bfloat16 and dy2.is_contiguous() and x2.is_contiguous()
    m = dy2.shape[0]
    n, k = dy2.shape[1] // 2, x2.shape[1] // 2
    assert x2.shape[0] == m and m > 0
    lib = _native.load()
    nbytes = int(lib.hfl_wgrad_x3_workspace(m, n, k))
    if nbytes <= 0:
        raise _native.NativeLibraryError('hfl_wgrad_x3: unsupported shape (%d, %d, %d)' % (m, n, k))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dy2.device)
    dw = torch.empty((n, k), dtype=torch.float32, device=dy2.device)
    db = torch.empty(n, dtype=torch.float32, device=dy2.device) if with_bias else None
    with _timed('hfl_wgrad_x3', m * (n + k) * 4, 2 * m * n * k):
        check(lib.hfl_wgrad_x3(dw.data_ptr(), None if db is None else db.data_ptr(), dy2.data_ptr(), x2.data_ptr(),
                               m, n, k, ws.data_ptr(), _stream()), 'hfl_wgrad_x3')
    return dw, db


def wgrad_f32(dy: torch.Tensor, x: torch.Tensor, with_bias: bool = False):
    """(dW, db) of y = x W^T + b from f32 rows on the fp32 matrix cores: dW (N, K) = dy^T x, db (N) = dy summed over rows
    (hfl_wgrad_f32; fixed reduction order, bitwise reproducible).  dy (M, N), x (M, K), N and K multiples of 128."""
    _dev(dy, x)
    dyc, xc = _f32c(dy), _f32c(x)
    m, n = dyc.shape
    k = xc.shape[1]
    assert xc.shape[0] == m
    dw = torch.empty((n, k), dtype=torch.float32, device=dy.device)
    db = torch.empty(n, dtype=torch.float32, device=dy.device) if with_bias else None
    if m == 0:
        dw.zero_()
        if db is not None:
            db.zero_()
        return dw, db
    lib = _native.load()
    nbytes = int(lib.hfl_wgrad_f32_workspace(m, n, k))
    if nbytes <= 0:
        raise _native.NativeLibraryError('hfl_wgrad_f32: unsupported shape (%d, %d, %d)' % (m, n, k))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dy.device)
    with _timed('hfl_wgrad_f32', m * (n + k) * 4, 2 * m * n * k):
        check(lib.hfl_wgrad_f32(dw.data_ptr(), None if db is None else db.data_ptr(), dyc.data_ptr(), xc.data_ptr(),
                                m, n, k, ws.data_ptr(), _stream()), 'hfl_wgrad_f32')
    return dw, db


def linear_x3_qkv(x2: torch.Tensor, w2: torch.Tensor, bias, q_scale: float, out=None) -> torch.Tensor:
    """qkv projection into the fp16 (hi, lo) operand layout of the v5 window-attention kernel (hfl_linear_x3_qkv):
    returns an opaque (rows, 3C) float32-sized buffer for `window_attention(..., qkv_f16=True)`."""
    _dev(x2, w2, bias)
    assert x2.dtype == torch.bfloat16 and w2.dtype == torch.bfloat16 and x2.is_contiguous() and w2.is_contiguous()
    m, k2 = x2.shape
    n = w2.shape[0]
    assert w2.shape[1] == k2 and n % 3 == 0
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=x2.device)
    else:
        assert tuple(out.shape) == (m, n) and out.dtype == torch.float32 and out.is_contiguous()
    with _timed('hfl_linear_x3', m * (k2 // 2) * 4 + m * n * 4, 2 * m * (k2 // 2) * n):
        check(_native.load().hfl_linear_x3_qkv(out.data_ptr(), x2.data_ptr(), w2.data_ptr(),
                                               None if bias is None else _f32c(bias).data_ptr(), m, k2 // 2, n,
                                               float(q_scale), _stream()), 'hfl_linear_x3_qkv')
    return out


def qkv_fused_pack(w_qkv: torch.Tensor) -> torch.Tensor:
    """Weight image of `ln_qkv_fused` from the fp32 qkv weight (3C, C) (hfl_qkv_fused_pack).  Once per parameter."""
    _dev(w_qkv)
    w = _f32c(w_qkv.detach())
    c = w.shape[1]
    assert tuple(w.shape) == (3 * c, c)
    lib = _native.load()
    n = int(lib.hfl_qkv_fused_pack_bytes(c))
    if n <= 0:
        raise _native.NativeLibraryError('hfl_qkv_fused_pack: unsupported channel count %d' % c)
    pack = torch.empty(n, dtype=torch.uint8, device=w.device)
    check(lib.hfl_qkv_fused_pack(pack.data_ptr(), w.data_ptr(), c, _stream()), 'hfl_qkv_fused_pack')
    return pack


def ln_qkv_fused(x, gamma, beta, eps: float, pack, bias, q_scale: float, out=None):
    """LayerNorm + qkv projection into the fp16 (hi, lo) operand layout of the window kernel in ONE launch
    (hfl_ln_qkv_fused = layer_norm_split2 + linear_x3_qkv): an opaque (rows, 3C) float32-sized buffer."""
    _dev(gamma, beta, pack, bias)
    if isinstance(x, (list, tuple)):                  # the rows in several arrays (hfl_ln_qkv_fused_seg)
        seg, m = row_segments(x)
        c = x[0].shape[1]
        if out is None:
            out = torch.empty((m, 3 * c), dtype=torch.float32, device=x[0].device)
        with _timed('hfl_ln_qkv_fused', m * c * 16, 6 * m * c * c):
            check(_native.load().hfl_ln_qkv_fused_seg(out.data_ptr(), ctypes.byref(seg), _f32c(gamma).data_ptr(),
                                                      _f32c(beta).data_ptr(), float(eps), pack.data_ptr(), _f32c(bias).data_ptr(),
                                                      float(q_scale), m, c, _stream()), 'hfl_ln_qkv_fused_seg')
        return out
    _dev(x)
    x = _f32c(x)
    m, c = x.shape
    if out is None:
        out = torch.empty((m, 3 * c), dtype=torch.float32, device=x.device)
    # algorithmic bytes: read x, write the operand rows; 2 M C 3C flop
    with _timed('hfl_ln_qkv_fused', m * c * 16, 6 * m * c * c):
        check(_native.load().hfl_ln_qkv_fused(out.data_ptr(), x.data_ptr(), _f32c(gamma).data_ptr(), _f32c(beta).data_ptr(),
                                              float(eps), pack.data_ptr(), _f32c(bias).data_ptr(), float(q_scale), m, c,
                                              _stream()), 'hfl_ln_qkv_fused')
    return out


def attn_fused_ok(n_tokens: int, n_windows: int, patch_size: int, dilation: int, n_relay: int, n_heads: int, depth: int,
                  channels: int, has_rpe: bool) -> bool:
    """Whether `attn_fused` (LayerNorm -> qkv -> window attention in one launch) takes this configuration."""
    desc = WindowAttnDesc(n_tokens=n_tokens, rt_row0=n_tokens, n_windows=n_windows, patch_size=patch_size, dilation=dilation,
                          n_relay=n_relay, n_heads=n_heads, pos_bnd=int(0.8 * patch_size * dilation ** 0.5),
                          batch_size=1, scale=16 ** -0.5, depth=depth)
    return bool(_native.load().hfl_attn_fused_ok(ctypes.byref(desc), int(channels), 1 if has_rpe else 0))


def attn_fused(x, gamma, beta, eps: float, qkv_pack, qkv_bias, q_scale: float, tok_meta, rpe_table, n_tokens: int,
               n_windows: int, patch_size: int, dilation: int, n_heads: int, batch_size: int, depth: int, out=None):
    """split2(window_attention(qkv(LayerNorm(x)))) in ONE launch (hfl_attn_fused_fwd): x (n_tokens, C) f32 -> (n_tokens, 2C)
    bf16, the operand of the proj GEMM -- bitwise what `ln_qkv_fused` + `window_attention(..., out_split=2, qkv_f16=True)` give."""
    _dev(x, gamma, beta, qkv_pack, qkv_bias, tok_meta, rpe_table)
    x = _f32c(x)
    c = x.shape[1]
    assert x.shape[0] >= n_tokens
    if out is None:
        out = torch.empty((x.shape[0], 2 * c), dtype=torch.bfloat16, device=x.device)
    desc = WindowAttnDesc(n_tokens=n_tokens, rt_row0=n_tokens, n_windows=n_windows, patch_size=patch_size, dilation=dilation,
                          n_relay=0, n_heads=n_heads, pos_bnd=int(0.8 * patch_size * dilation ** 0.5),
                          batch_size=batch_size, scale=16 ** -0.5, depth=depth)
    table_ptr, expanded = None, None
    if rpe_table is not None:
        expanded = rpe_expand(rpe_table, n_heads, desc.pos_bnd, depth, True)
        assert expanded is not None
        desc.rpe_expanded = expanded.data_ptr()
        rpe_table = _f32c(rpe_table)
        table_ptr = rpe_table.data_ptr()
    # algorithmic bytes: read x, write the split2 output (8 B per (row, channel)) + 8 B of metadata per token
    real_windows = -(-n_tokens // patch_size)
    with _timed('hfl_attn_fused_fwd', n_tokens * c * 8 + n_tokens * 8,
                6 * n_tokens * c * c + 4 * patch_size * patch_size * c * real_windows):
        check(_native.load().hfl_attn_fused_fwd(out.data_ptr(), x.data_ptr(), _f32c(gamma).data_ptr(), _f32c(beta).data_ptr(),
                                                float(eps), qkv_pack.data_ptr(), _f32c(qkv_bias).data_ptr(), float(q_scale),
                                                tok_meta.data_ptr(), table_ptr, ctypes.byref(desc), _stream()),
              'hfl_attn_fused_fwd')
    return out


def attn_ws_ok(n_tokens: int, n_windows: int, patch_size: int, n_heads: int, depth: int, channels: int) -> bool:
    """Whether `attn_ws` takes this relay-token block configuration."""
    desc = WindowAttnDesc(n_tokens=n_tokens, rt_row0=n_tokens, n_windows=n_windows, patch_size=patch_size, dilation=1,
                          n_relay=1, n_heads=n_heads, pos_bnd=int(0.8 * patch_size), batch_size=1, scale=16 ** -0.5, depth=depth)
    return bool(_native.load().hfl_attn_ws_ok(ctypes.byref(desc), int(channels)))


def attn_ws(x, gamma, beta, eps: float, qkv_pack, qkv_bias, q_scale: float, relay_qkv, tok_meta, rpe_table, n_tokens: int,
            n_windows: int, patch_size: int, n_heads: int, batch_size: int, depth: int, out=None):
    """split2(window_attention(qkv(LayerNorm(x)), relay q / k / v)) of a relay-token block in ONE launch (hfl_attn_ws_fwd):
    x (n_tokens, C) f32 token rows, relay_qkv (n_windows, 3C) the relay rows' fp16 (hi, lo) operand rows (`ln_qkv_fused` over
    them) -> (n_tokens + n_windows, 2C) bf16, the operand of the proj GEMM (relay rows at n_tokens + window)."""
    _dev(x, gamma, beta, qkv_pack, qkv_bias, relay_qkv, tok_meta, rpe_table)
    x = _f32c(x)
    c = x.shape[1]
    assert x.shape[0] >= n_tokens and relay_qkv.is_contiguous() and relay_qkv.shape[0] >= n_windows
    if out is None:
        out = torch.zeros((n_tokens + n_windows, 2 * c), dtype=torch.bfloat16, device=x.device)
    bnd = int(0.8 * patch_size)
    desc = WindowAttnDesc(n_tokens=n_tokens, rt_row0=n_tokens, n_windows=n_windows, patch_size=patch_size, dilation=1,
                          n_relay=1, n_heads=n_heads, pos_bnd=bnd, batch_size=batch_size, scale=16 ** -0.5, depth=depth)
    tables = None
    if rpe_table is not None:
        tables = rpe_expand(rpe_table, n_heads, bnd, depth, 2)
        assert tables is not None
    with _timed('hfl_attn_ws_fwd', n_tokens * c * 8 + n_tokens * 8 + n_windows * c * 16,
                6 * n_tokens * c * c + 4 * (patch_size + 1) ** 2 * c * n_windows):
        check(_native.load().hfl_attn_ws_fwd(out.data_ptr(), x.data_ptr(), _f32c(gamma).data_ptr(), _f32c(beta).data_ptr(),
                                             float(eps), qkv_pack.data_ptr(), _f32c(qkv_bias).data_ptr(), float(q_scale),
                                             relay_qkv.data_ptr(), tok_meta.data_ptr(),
                                             None if tables is None else tables.data_ptr(), ctypes.byref(desc), _stream()),
              'hfl_attn_ws_fwd')
    return out


def window_attention_f16_ok(n_rows: int, patch_size: int, dilation: int, n_relay: int, n_heads: int, depth: int) -> bool:
    """Whether the window kernel takes the fp16 (hi, lo) qkv layout for this launch (else: fp32 qkv)."""
    desc = WindowAttnDesc(n_tokens=n_rows, rt_row0=0, n_windows=1, patch_size=patch_size, dilation=dilation,
                          n_relay=n_relay, n_heads=n_heads, pos_bnd=int(0.8 * patch_size * dilation ** 0.5),
                          batch_size=1, scale=16 ** -0.5, depth=depth)
    return bool(_native.load().hfl_window_attention_f16_ok(ctypes.byref(desc), int(n_rows)))


def stack3(x: torch.Tensor, order: str) -> torch.Tensor:
    """(M, C) fp32 -> (3M, C) bf16 planes stacked along the rows: 'hhl' = [hi; hi; lo], 'hlh' = [hi; lo; hi]
    (operands of `gemm_bf16_tn`, the contraction runs over the rows)."""
    x = _f32c(x)
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return torch.cat([hi, hi, lo] if order == 'hhl' else [hi, lo, hi], 0)


def gemm_bf16_tn(a_stack: torch.Tensor, b_stack: torch.Tensor) -> torch.Tensor:
    """fp32 (N, K) = a_stack^T @ b_stack over the stacked rows (hfl_gemm_bf16_tn): dW = dy^T x."""
    _dev(a_stack, b_stack)
    assert a_stack.dtype == torch.bfloat16 and b_stack.dtype == torch.bfloat16
    assert a_stack.is_contiguous() and b_stack.is_contiguous() and a_stack.shape[0] == b_stack.shape[0]
    r, n = a_stack.shape
    k = b_stack.shape[1]
    out = torch.empty((n, k), dtype=torch.float32, device=a_stack.device)
    check(_native.load().hfl_gemm_bf16_tn(out.data_ptr(), a_stack.data_ptr(), b_stack.data_ptr(), r, n, k,
                                          _stream()), 'hfl_gemm_bf16_tn')
    return out


# ------------------------------------------------------------------------- gather
def octree_gather(data, neigh):
    """(N,C),(M,K) int32 -> (M, K*C): ocnn octree2col with zero fill."""
    _dev(data, neigh)
    data = _f32c(data)
    assert neigh.dtype == torch.int32 and neigh.is_contiguous()
    m, k = neigh.shape
    c = data.shape[1]
    out = torch.empty((m, k * c), dtype=torch.float32, device=data.device)
    with _timed('hfl_octree_gather', data.numel() * 4 + m * k * c * 4 + m * k * 4):
        check(_native.load().hfl_octree_gather(out.data_ptr(), data.data_ptr(), neigh.data_ptr(), m, k,
                                               c, _stream()), 'hfl_octree_gather')
    return out


def inverse_table(inverse: torch.Tensor, table: torch.Tensor):
    """inverse (n_src, K) int32 of a gather table (n_dst, K) int32: inverse[table[m, k], k] = m, -1 elsewhere
    (hfl_inverse_table)."""
    _dev(inverse, table)
    assert table.dtype == torch.int32 and inverse.dtype == torch.int32 and table.is_contiguous() and inverse.is_contiguous()
    check(_native.load().hfl_inverse_table(inverse.data_ptr(), inverse.shape[0], table.data_ptr(), table.shape[0],
                                           table.shape[1], _stream()), 'hfl_inverse_table')
    return inverse


def tap_wgrad(g: torch.Tensor, dpart: torch.Tensor, chunks: torch.Tensor, tap_chunk_off: torch.Tensor, taps: int,
              g_rows=None, d_rows=None):
    """dW (taps, Cin, Cout) of a live-tap octree convolution: dW[k] = g_k^T dpart_k over the pairs of tap k
    (hfl_tap_wgrad; `chunks` / `tap_chunk_off` from Octree.sparse_taps_bwd).  g_rows / d_rows (P,) int32: pair p reads row
    g_rows[p] of g / d_rows[p] of dpart (hfl_tap_wgrad_gather) instead of row p of a pair-major copy."""
    _dev(g, dpart, chunks, tap_chunk_off, g_rows, d_rows)
    g, dpart = _f32c(g), _f32c(dpart)
    cin, cout = g.shape[1], dpart.shape[1]
    n_chunks = chunks.shape[0]
    for t in (g_rows, d_rows):
        assert t is None or (t.dtype == torch.int32 and t.is_contiguous())
    pairs = (g_rows if g_rows is not None else g).shape[0]
    dw = torch.empty((taps, cin, cout), dtype=torch.float32, device=g.device)
    ws = torch.empty((max(n_chunks, 1), cin, cout), dtype=torch.float32, device=g.device)
    with _timed('hfl_tap_wgrad', pairs * (cin + cout) * 4, 2 * pairs * cin * cout):
        check(_native.load().hfl_tap_wgrad_gather(dw.data_ptr(), g.data_ptr(), None if g_rows is None else g_rows.data_ptr(),
                                                  dpart.data_ptr(), None if d_rows is None else d_rows.data_ptr(),
                                                  chunks.data_ptr(), n_chunks, tap_chunk_off.data_ptr(), taps, cin, cout,
                                                  ws.data_ptr(), _stream()), 'hfl_tap_wgrad_gather')
    return dw


def tap_lists(table: torch.Tensor, edges_out: torch.Tensor = None):
    """Live-tap lists of a (rows, taps) int32 table (hfl_tap_lists): (src capacity rows*taps, slot (rows, taps),
    edges (taps+1) int32 on the device).  No host synchronisation; the caller narrows `src` once it knows
    edges[-1]."""
    _dev(table)
    assert table.dtype == torch.int32 and table.is_contiguous() and table.dim() == 2
    rows, taps = table.shape
    lib = _native.load()
    dev = table.device
    src = torch.empty(max(rows * taps, 1), dtype=torch.int32, device=dev)
    slot = torch.empty((rows, taps), dtype=torch.int32, device=dev)
    edges = torch.empty(taps + 1, dtype=torch.int32, device=dev) if edges_out is None else edges_out
    assert edges.dtype == torch.int32 and edges.numel() == taps + 1 and edges.is_contiguous()
    ws = torch.empty(int(lib.hfl_tap_lists_workspace(rows, taps)), dtype=torch.uint8, device=dev)
    check(lib.hfl_tap_lists(src.data_ptr(), slot.data_ptr(), edges.data_ptr(), table.data_ptr(), rows, taps,
                            ws.data_ptr(), _stream()), 'hfl_tap_lists')
    return src, slot, edges


def tap_lists_multi(tables, edges_outs):
    """`tap_lists` for up to 16 tables in three launches in all (hfl_tap_lists_multi): [(src, slot, edges)] per table."""
    import ctypes
    lib = _native.load()
    n = len(tables)
    assert 1 <= n <= 16 and len(edges_outs) == n
    _dev(*tables)
    dev = tables[0].device
    out, ws = [], []
    for t, e in zip(tables, edges_outs):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.dim() == 2
        rows, taps = t.shape
        assert e.dtype == torch.int32 and e.numel() == taps + 1 and e.is_contiguous()
        out.append((torch.empty(max(rows * taps, 1), dtype=torch.int32, device=dev),
                    torch.empty((rows, taps), dtype=torch.int32, device=dev), e))
        ws.append(torch.empty(int(lib.hfl_tap_lists_workspace(rows, taps)), dtype=torch.uint8, device=dev))
    ptr = lambda xs: (ctypes.c_void_p * n)(*[x.data_ptr() for x in xs])            # noqa: E731
    rows = (ctypes.c_int64 * n)(*[t.shape[0] for t in tables])
    taps = (ctypes.c_int32 * n)(*[t.shape[1] for t in tables])
    check(lib.hfl_tap_lists_multi(n, ptr([o[0] for o in out]), ptr([o[1] for o in out]), ptr([o[2] for o in out]),
                                  ptr(tables), rows, taps, ptr(ws), _stream()), 'hfl_tap_lists_multi')
    return out


def tap_tiles(edges_dev: torch.Tensor, n_tiles: int, taps: int, w_rows: int, tile_rows: int = 128):
    """(n_tiles, 3) int32 row-tile table of `linear_x3_grouped` from the device-side tap edges (hfl_tap_tiles)."""
    _dev(edges_dev)
    assert edges_dev.dtype == torch.int32 and edges_dev.numel() == taps + 1
    tiles = torch.empty((n_tiles, 3), dtype=torch.int32, device=edges_dev.device)
    if n_tiles > 0:
        check(_native.load().hfl_tap_tiles(tiles.data_ptr(), edges_dev.data_ptr(), taps, tile_rows, w_rows, _stream()),
              'hfl_tap_tiles')
    return tiles


def pad_index(row_off: torch.Tensor, batch: int, nmax: int):
    """(batch * nmax) int64 gather index of a ragged per-cloud row stream, sentinel = row_off[batch] (hfl_pad_index)."""
    _dev(row_off)
    assert row_off.dtype == torch.int64 and row_off.numel() == batch + 1
    out = torch.empty(batch * nmax, dtype=torch.int64, device=row_off.device)
    check(_native.load().hfl_pad_index(out.data_ptr(), row_off.data_ptr(), batch, nmax, _stream()), 'hfl_pad_index')
    return out


def pad_rows(x: torch.Tensor, row_off: torch.Tensor, batch: int, nmax: int):
    """(batch, nmax, C) zero-padded per-cloud copy of the ragged rows x (N, C) (hfl_pad_rows)."""
    _dev(x, row_off)
    x = _f32c(x)
    assert row_off.dtype == torch.int64 and row_off.numel() == batch + 1 and x.shape[1] % 4 == 0
    out = torch.empty((batch, nmax, x.shape[1]), dtype=torch.float32, device=x.device)
    check(_native.load().hfl_pad_rows(out.data_ptr(), x.data_ptr(), row_off.data_ptr(), batch, nmax, x.shape[1], _stream()),
          'hfl_pad_rows')
    return out


def mixer_tail(x: torch.Tensor, channel_w, channel_b, row_w, row_b):
    """(B, k_out * out_d) = flatten(row_proj(channel_proj(x^T)^T)) of the Mixer aggregator in one launch (hfl_mixer_tail);
    x (B, K, C), channel_w (k_out, K), row_w (out_d, C)."""
    _dev(x, channel_w, channel_b, row_w, row_b)
    x = _f32c(x)
    b, k, c = x.shape
    ko, d = channel_w.shape[0], row_w.shape[0]
    assert tuple(channel_w.shape) == (ko, k) and tuple(row_w.shape) == (d, c)
    out = torch.empty((b, ko * d), dtype=torch.float32, device=x.device)
    check(_native.load().hfl_mixer_tail(out.data_ptr(), x.data_ptr(), _f32c(channel_w).data_ptr(), _f32c(channel_b).data_ptr(),
                                        _f32c(row_w).data_ptr(), _f32c(row_b).data_ptr(), b, k, c, ko, d, _stream()),
          'hfl_mixer_tail')
    return out


def mixer_chain_ok(channels: int, hidden: int, layers: int, out_d: int) -> bool:
    return bool(_native.load().hfl_mixer_chain_ok(int(channels), int(hidden), int(layers), int(out_d)))


def mixer_chain_pack(w1s, w2s) -> torch.Tensor:
    """Weight image of `mixer_chain` (hfl_mixer_chain_pack) from the fp32 weights fc1 (C, C) and fc2 (C, C) of every layer, in
    layer order: bf16 (hi, lo) MFMA fragments.  Once per parameter set."""
    w1s, w2s = [_f32c(w.detach()) for w in w1s], [_f32c(w.detach()) for w in w2s]
    _dev(*w1s, *w2s)
    lib = _native.load()
    layers = len(w1s)
    ok = len(w2s) == layers and all(tuple(w.shape) == (256, 256) for w in w1s + w2s)
    n = int(lib.hfl_mixer_chain_pack_bytes(layers)) if ok else 0
    if n <= 0:
        raise _native.NativeLibraryError('hfl_mixer_chain_pack: unsupported layer count or shape')
    pack = torch.empty(n, dtype=torch.uint8, device=w1s[0].device)
    check(lib.hfl_mixer_chain_pack(pack.data_ptr(), _native.ptr_array([w.data_ptr() for w in w1s]),
                                   _native.ptr_array([w.data_ptr() for w in w2s]), layers, _stream()), 'hfl_mixer_chain_pack')
    return pack


def mixer_chain(x, pack, gammas, betas, b1s, b2s, eps: float, row_w=None, want_x: bool = True):
    """L FeatureMixerLayers x = x + fc2(gelu(fc1(LN(x)))) on the rows of x (M, 256), then u = x @ row_w^T (row_w (D, 256), D <= 8,
    optional), in ONE launch (hfl_mixer_chain_x3); `pack` from `mixer_chain_pack`, the other lists hold one tensor per layer.
    Returns (x after the last layer or None, u (M, D) or None): each is written only when asked for.  A problem the launch
    does not take (hfl_mixer_chain_ok, or rows that are not contiguous) raises with the library's HFL_EINVAL: nothing runs."""
    vecs = [list(gammas), list(betas), list(b1s), list(b2s)]
    _dev(x, pack, row_w, *[v for vs in vecs for v in vs])
    layers = len(vecs[0])
    lib = _native.load()
    if x.dtype != torch.float32:
        raise TypeError('float32 expected, got %s' % x.dtype)
    hidden = vecs[2][0].numel() if layers > 0 else 0
    d = 0 if row_w is None else int(row_w.shape[0])
    fits = (x.dim() == 2 and x.is_contiguous() and all(len(v) == layers for v in vecs[1:])
            and lib.hfl_mixer_chain_ok(x.shape[-1], hidden, layers, d)
            and all(v.numel() == x.shape[1] for vs in vecs for v in vs)
            and (row_w is None or row_w.shape[1] == x.shape[1]) and (row_w is not None or want_x))
    if not fits:
        check(_native.HFL_EINVAL, 'hfl_mixer_chain_x3')
    assert pack.numel() == int(lib.hfl_mixer_chain_pack_bytes(layers)), 'pack does not belong to this layer count'
    m, c = x.shape
    vecs = [[_f32c(v) for v in vs] for vs in vecs]
    row_w = None if row_w is None else _f32c(row_w)
    out_x = torch.empty_like(x) if want_x else None
    out_u = torch.empty((m, d), dtype=torch.float32, device=x.device) if d > 0 else None
    # algorithmic bytes: read x, write what was asked for; 2 GEMMs of 2 M C C flop per layer
    with _timed('hfl_mixer_chain_x3', m * c * (8 if want_x else 4) + m * d * 4, layers * 4 * m * c * c + 2 * m * c * d):
        check(lib.hfl_mixer_chain_x3(None if out_x is None else out_x.data_ptr(), None if out_u is None else out_u.data_ptr(),
                                     x.data_ptr(), pack.data_ptr(), *[_native.ptr_array([v.data_ptr() for v in vs]) for vs in vecs],
                                     float(eps), None if row_w is None else row_w.data_ptr(), m, layers, d, _stream()),
              'hfl_mixer_chain_x3')
    return out_x, out_u


def descriptor_tail(u: torch.Tensor, channel_w, channel_b, row_w, row_b, normalize: bool):
    """(B, k_out * D) descriptors from u (B, K, D) = row_proj without its bias (`mixer_chain`): channel_proj over the token axis,
    both biases, the flatten, and with `normalize` F.normalize(., dim=1), in one launch (hfl_descriptor_tail); channel_w
    (k_out, K), row_w (D, C)."""
    _dev(u, channel_w, channel_b, row_w, row_b)
    u = _f32c(u)
    b, k, d = u.shape
    ko, c = channel_w.shape[0], row_w.shape[1]
    assert tuple(channel_w.shape) == (ko, k) and tuple(row_w.shape) == (d, c)
    out = torch.empty((b, ko * d), dtype=torch.float32, device=u.device)
    with _timed('hfl_descriptor_tail', u.numel() * 4 + out.numel() * 4 + ko * k * 4, 2 * b * ko * k * d):
        check(_native.load().hfl_descriptor_tail(out.data_ptr(), u.data_ptr(), _f32c(channel_w).data_ptr(),
                                                 _f32c(channel_b).data_ptr(), _f32c(row_w).data_ptr(), _f32c(row_b).data_ptr(),
                                                 b, k, c, ko, d, 1 if normalize else 0, _stream()), 'hfl_descriptor_tail')
    return out


def attn_pool_ok(channels: int) -> bool:
    return bool(_native.load().hfl_attn_pool_ok(int(channels)))


def attn_pool(x: torch.Tensor, row_off: torch.Tensor, query: torch.Tensor, batch: int, scale: float, out=None):
    """(batch, k, C) = per cloud softmax(scale * query x^T) x over the cloud's rows of the ragged x (N, C)
    (hfl_attn_pool: salsa.py:25-55).  `out`: a (batch, k, C) view, possibly a slice of a wider token matrix along dim 1."""
    _dev(x, row_off, query)
    x, query = _f32c(x), _f32c(query)
    assert row_off.dtype == torch.int64 and row_off.numel() == batch + 1 and query.shape[1] == x.shape[1]
    k, c = query.shape
    if out is None:
        out = torch.empty((batch, k, c), dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.shape == (batch, k, c) and out.stride(2) == 1 and out.stride(1) == c
    lib = _native.load()
    nb = lib.hfl_attn_pool_workspace(batch, k, c, x.shape[0])
    ws = torch.empty(max(int(nb), 16), dtype=torch.uint8, device=x.device)
    with _timed('hfl_attn_pool', x.numel() * 4 + out.numel() * 4, 4 * x.shape[0] * k * c):
        check(lib.hfl_attn_pool(out.data_ptr(), out.stride(0), x.data_ptr(), row_off.data_ptr(), query.data_ptr(), batch, k, c,
                                x.shape[0], float(scale), ws.data_ptr(), int(nb), _stream()), 'hfl_attn_pool')
    return out


# ---------------------------------------------------------------------- attention
_RPE2_CACHE = {}        # (id(table), depth) -> (weakref to table, version, expanded table)


def rpe_expand(rpe_table, n_heads: int, pos_bnd: int, depth: int, f16: bool = False):
    """Expanded relative-position table of the window kernels (hfl_window_rpe_expand) for the fp32-qkv kernel or, with
    `f16`, for the fp16 (hi, lo) one (the two take different forms at depth 5+), cached per (table, depth, consumer) and
    rebuilt when the table is modified in place.  None when the consumer has no expanded form for this depth."""
    lib = _native.load()
    n = lib.hfl_window_rpe_expand_size(n_heads, pos_bnd, depth, int(f16))
    if n <= 0:
        return None
    key = (id(rpe_table), depth, int(f16))            # (f16 = 2: the fused attention kernels' three 1-D tables at every depth)
    hit = _RPE2_CACHE.get(key)
    # data_ptr / device: `module.to(...)` swaps `.data` without bumping the version counter
    if (hit is not None and hit[0]() is rpe_table and hit[1] == rpe_table._version and hit[3] == rpe_table.data_ptr()
            and hit[2].device == rpe_table.device):
        return hit[2]
    out = torch.empty(n, dtype=torch.float32, device=rpe_table.device)
    src = _f32c(rpe_table.detach())
    check(lib.hfl_window_rpe_expand(out.data_ptr(), src.data_ptr(), n_heads, pos_bnd, depth, int(f16), _stream()),
          'hfl_window_rpe_expand')
    if len(_RPE2_CACHE) > 512:
        _RPE2_CACHE.clear()
    _RPE2_CACHE[key] = (weakref.ref(rpe_table), rpe_table._version, out, rpe_table.data_ptr())
    return out


def window_attention(qkv, tok_meta, rpe_table, n_tokens: int, n_windows: int, patch_size: int,
                     dilation: int, n_relay: int, n_heads: int, batch_size: int, rt_row0: int = 0,
                     depth: int = 0, qkv_bias=None, out_split: bool = False, qkv_f16: bool = False):
    """qkv (rows, 3*H*16) -> out (rows, H*16) fp32, or with out_split the bf16 [hi|hi|lo]
    (rows, 3*H*16) operand of the projection GEMM; qkv_bias is added to q,k,v on load.  qkv_f16: `qkv` is the
    fp16 (hi, lo) operand buffer of `linear_x3_qkv` (bias and softmax scale already folded in).
    See hfl_window_attention_fwd(_ex)."""
    _dev(qkv, tok_meta, rpe_table, qkv_bias)
    qkv = _f32c(qkv)
    rows = qkv.shape[0]
    c = n_heads * 16
    assert qkv.shape[1] == 3 * c
    out_split = int(out_split)          # 0: fp32 out; 1: bf16 [hi|hi|lo] (rows, 3c); 2: bf16 split2 (rows, 2c)
    if out_split:
        width = 3 * c if out_split == 1 else 2 * c
        # rows the kernel does not own (none today) must not hold NaN bit patterns
        out = torch.zeros((rows, width), dtype=torch.bfloat16, device=qkv.device) if rows > n_tokens + \
            (n_windows if n_relay else 0) else torch.empty((rows, width), dtype=torch.bfloat16, device=qkv.device)
    else:
        out = torch.empty((rows, c), dtype=torch.float32, device=qkv.device)
    desc = WindowAttnDesc(n_tokens=n_tokens, rt_row0=rt_row0, n_windows=n_windows,
                          patch_size=patch_size, dilation=dilation, n_relay=n_relay,
                          n_heads=n_heads, pos_bnd=int(0.8 * patch_size * dilation ** 0.5),
                          batch_size=batch_size, scale=16 ** -0.5, depth=depth)
    table_ptr = None
    if rpe_table is not None:
        assert tuple(rpe_table.shape) == (3 * (2 * desc.pos_bnd + 1), n_heads)
        expanded = rpe_expand(rpe_table, n_heads, desc.pos_bnd, depth, qkv_f16)   # keeps the tensor alive below
        if expanded is not None:
            desc.rpe_expanded = expanded.data_ptr()
        rpe_table = _f32c(rpe_table)
        table_ptr = rpe_table.data_ptr()
    used = n_tokens + (n_windows if n_relay else 0)          # rows the kernel touches
    seq = patch_size + n_relay
    real_windows = -(-n_tokens // patch_size)
    # algorithmic work: read q,k,v + write out = 16 B per (row, channel); QK^T + PV = 4 L^2 C per
    # window.  Moved: the bf16 [hi|hi|lo] output is 6 B instead of 4 B per channel, plus 8 B of metadata per token
    with _timed('hfl_window_attention_fwd', used * c * 16, 4 * seq * seq * c * real_windows,
                moved=used * c * (18 if out_split == 1 else 16) + n_tokens * 8):
        check(_native.load().hfl_window_attention_fwd_ex(
            out.data_ptr(), qkv.data_ptr(), None if qkv_bias is None else _f32c(qkv_bias).data_ptr(),
            tok_meta.data_ptr(), table_ptr, ctypes.byref(desc), out_split | (0x100 if qkv_f16 else 0), _stream()),
            'hfl_window_attention_fwd')
    return out


def window_attention_multi(problems, out_split: int = 2):
    """Several window-attention problems on fp16 (hi, lo) qkv operands as ONE launch when their shapes agree
    (hfl_window_attention_fwd_multi), else one launch each.  `problems`: list of dicts with the arguments of
    `window_attention` (qkv, tok_meta, rpe_table, n_tokens, n_windows, patch_size, dilation, n_relay, n_heads, batch_size,
    rt_row0, depth).  Returns the list of outputs (split2 bf16 rows for out_split 2, fp32 rows for 0)."""
    assert 1 <= len(problems) <= 4 and out_split in (0, 2)
    lib = _native.load()
    outs, descs, keep = [], [], []
    for pr in problems:
        qkv = _f32c(pr['qkv'])
        _dev(qkv, pr['tok_meta'], pr['rpe_table'])
        rows, c = qkv.shape[0], pr['n_heads'] * 16
        assert qkv.shape[1] == 3 * c
        out = (torch.zeros((rows, 2 * c), dtype=torch.bfloat16, device=qkv.device) if out_split == 2
               else torch.zeros((rows, c), dtype=torch.float32, device=qkv.device))
        bnd = int(0.8 * pr['patch_size'] * pr['dilation'] ** 0.5)
        desc = WindowAttnDesc(n_tokens=pr['n_tokens'], rt_row0=pr.get('rt_row0', 0), n_windows=pr['n_windows'],
                              patch_size=pr['patch_size'], dilation=pr['dilation'], n_relay=pr['n_relay'],
                              n_heads=pr['n_heads'], pos_bnd=bnd, batch_size=pr['batch_size'], scale=16 ** -0.5,
                              depth=pr['depth'])
        table = pr['rpe_table']
        if table is not None:
            expanded = rpe_expand(table, pr['n_heads'], bnd, pr['depth'], True)
            desc.rpe_expanded = None if expanded is None else expanded.data_ptr()
            table = _f32c(table)
            keep.append((expanded, table))
        outs.append(out)
        descs.append(desc)
        keep.append(qkv)
        pr['_ptrs'] = (out.data_ptr(), qkv.data_ptr(), pr['tok_meta'].data_ptr(), None if table is None else table.data_ptr())
    arr = lambda i: _native.ptr_array([pr['_ptrs'][i] for pr in problems])
    check(lib.hfl_window_attention_fwd_multi(len(problems), arr(0), arr(1), arr(2), arr(3),
                                             _native.ptr_array([ctypes.addressof(d) for d in descs]),
                                             out_split | 0x100, _stream()), 'hfl_window_attention_fwd_multi')
    return outs


def relay_attention_f16(qkv_f16, seq_rows, seq_off, batch: int, n_heads: int, max_seq_len: int, orphan_rows=None):
    """Ragged relay-token self-attention on the fp16 (hi, lo) operand rows of `ln_qkv_fused` (q pre-scaled by 16^-0.5 log2 e)
    -> (rows, 2C) bf16 split2, the operand of attention.proj; rows of no sequence (`orphan_rows`) come out zero
    (hfl_relay_attention_f16_fwd)."""
    _dev(qkv_f16, seq_rows, seq_off, orphan_rows)
    rows, c3 = qkv_f16.shape
    c = c3 // 3
    assert qkv_f16.dtype == torch.float32 and qkv_f16.is_contiguous() and c == n_heads * 16
    out = torch.empty((rows, 2 * c), dtype=torch.bfloat16, device=qkv_f16.device)
    n_orph = 0 if orphan_rows is None else orphan_rows.numel()
    check(_native.load().hfl_relay_attention_f16_fwd(out.data_ptr(), qkv_f16.data_ptr(), seq_rows.data_ptr(), seq_off.data_ptr(),
                                                     batch, n_heads, max_seq_len,
                                                     orphan_rows.data_ptr() if n_orph else None, n_orph, _stream()),
          'hfl_relay_attention_f16_fwd')
    return out


def relay_attention(qkv, seq_rows, seq_off, batch: int, n_heads: int, max_seq_len: int):
    """Ragged per-cloud attention over relay-token rows; rows in no sequence -> 0."""
    _dev(qkv, seq_rows, seq_off)
    qkv = _f32c(qkv)
    c = n_heads * 16
    out = torch.zeros((qkv.shape[0], c), dtype=torch.float32, device=qkv.device)
    with _timed('hfl_relay_attention_fwd', qkv.shape[0] * c * 16):
        check(_native.load().hfl_relay_attention_fwd(out.data_ptr(), qkv.data_ptr(),
                                                     seq_rows.data_ptr(), seq_off.data_ptr(), batch,
                                                     n_heads, 16 ** -0.5, int(max_seq_len), _stream()),
              'hfl_relay_attention_fwd')
    return out


def relay_token_init(x, tok_meta, n_windows: int, patch_size: int):
    _dev(x, tok_meta)
    x = _f32c(x)
    rt = torch.empty((n_windows, x.shape[1]), dtype=torch.float32, device=x.device)
    check(_native.load().hfl_relay_token_init(rt.data_ptr(), x.data_ptr(), tok_meta.data_ptr(),
                                              x.shape[0], n_windows, patch_size, x.shape[1],
                                              _stream()), 'hfl_relay_token_init')
    return rt


def window_stats(tok_meta, n_tokens: int, n_windows: int, patch_size: int, depth: int):
    _dev(tok_meta)
    stats = torch.empty((n_windows, 9), dtype=torch.float32, device=tok_meta.device)
    check(_native.load().hfl_window_stats(stats.data_ptr(), tok_meta.data_ptr(), n_tokens, n_windows,
                                          patch_size, depth, _stream()), 'hfl_window_stats')
    return stats


def segment_softmax_(scores, row_off, batch: int, scale: float):
    """In place: softmax over each cloud's rows, per query column."""
    _dev(scores, row_off)
    assert scores.dtype == torch.float32 and scores.is_contiguous() and row_off.dtype == torch.int64
    check(_native.load().hfl_segment_softmax(scores.data_ptr(), row_off.data_ptr(), batch,
                                             scores.shape[1], float(scale), _stream()),
          'hfl_segment_softmax')
    return scores


# --------------------------------------------------------------------------- octree
def token_meta(nkeys, depth: int):
    _dev(nkeys)
    assert nkeys.dtype == torch.int64
    meta = torch.empty((nkeys.shape[0], 2), dtype=torch.int32, device=nkeys.device)
    check(_native.load().hfl_token_meta(meta.data_ptr(), nkeys.data_ptr(), nkeys.shape[0], depth,
                                        _stream()), 'hfl_token_meta')
    return meta


def octree_neigh(neigh_parent, nidx, children, nkeys, depth: int, full_depth: int):
    _dev(nidx, children, nkeys)
    nne = nkeys.shape[0]
    out = torch.empty((nne, 27), dtype=torch.int32, device=nkeys.device)
    check(_native.load().hfl_octree_neigh(
        out.data_ptr(), None if neigh_parent is None else neigh_parent.data_ptr(), nidx.data_ptr(),
        children.data_ptr(), nkeys.data_ptr(), nne, depth, full_depth, _stream()), 'hfl_octree_neigh')
    return out


# --------------------------------------------------------------------------- MESA: weight EMA and distillation rows
EMA_CHUNK = 8192          # HFL_EMA_CHUNK of include/hotformerloc_hip.h


def ema_table(ema_tensors, src_tensors):
    """Device table of `hfl_ema_chunk` entries for `ema_update`: every (ema, src) pair of fp32 tensors cut into chunks of at
    most EMA_CHUNK elements.  Returns (table, n_chunks); the table holds raw pointers, so it is valid only while every
    tensor keeps its `data_ptr()` (the caller revalidates).  A tensor that appears twice (tied weights) is taken once."""
    ema_tensors, src_tensors = list(ema_tensors), list(src_tensors)
    if len(ema_tensors) != len(src_tensors):
        raise ValueError('ema_table: %d ema tensors, %d source tensors' % (len(ema_tensors), len(src_tensors)))
    _dev(*ema_tensors, *src_tensors)
    rows, seen = [], set()
    for e, s in zip(ema_tensors, src_tensors):
        if e.dtype != torch.float32 or s.dtype != torch.float32:
            raise TypeError('ema_update takes float32 tensors, got %s and %s' % (e.dtype, s.dtype))
        if e.shape != s.shape:
            raise ValueError('ema_update: shapes %s and %s differ' % (tuple(e.shape), tuple(s.shape)))
        if not (e.is_contiguous() and s.is_contiguous()):
            raise ValueError('ema_update needs contiguous tensors')
        n = e.numel()
        if n == 0 or e.data_ptr() in seen:
            continue
        seen.add(e.data_ptr())
        off = np.arange(0, n, EMA_CHUNK, dtype=np.int64)
        chunk = np.empty((off.shape[0], 3), dtype=np.int64)
        chunk[:, 0] = e.data_ptr() + 4 * off
        chunk[:, 1] = s.data_ptr() + 4 * off
        chunk[:, 2] = np.minimum(n - off, EMA_CHUNK)
        rows.append(chunk)
    if not rows:
        return None, 0
    table = np.concatenate(rows, 0)
    return torch.from_numpy(table).to(ema_tensors[0].device), int(table.shape[0])


def ema_update(table, n_chunks: int, w: float):
    """ema <- ema + w * (src - ema) over every chunk of an `ema_table`, one launch."""
    if n_chunks == 0:
        return
    _dev(table)
    assert table.dtype == torch.int64 and table.is_contiguous() and tuple(table.shape) == (n_chunks, 3)
    check(_native.load().hfl_ema_update(table.data_ptr(), n_chunks, float(w), _stream()), 'hfl_ema_update')


ADAM_CHUNK = 8192         # HFL_ADAM_CHUNK
ADAM_MAX_SLOTS = 16       # HFL_ADAM_MAX_SLOTS


def adam_slot(lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, decoupled: bool, step: int):
    """The fields of one `hfl_adam_slot` as Python floats (doubles), in the structure's order; ctypes rounds each once to
    float.  The formulas are torch's `_single_tensor_adam` with its Python scalars: the bias corrections from the integer
    step count, `step_size = lr / bias_correction1`, `bias_correction2 ** 0.5`."""
    if step < 1:
        raise ValueError('adam_slot: the step count starts at 1, got %r' % (step,))
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    decay = 1 - lr * weight_decay if decoupled else weight_decay
    return (lr / bias_correction1, bias_correction2 ** 0.5, 1 - beta1, beta2, 1 - beta2, eps, decay, int(bool(decoupled)))


def adam_chunk_rows(numels, param_ptrs, grad_ptrs, exp_avg_ptrs, exp_avg_sq_ptrs, ema_ptrs, slots):
    """Host half of `adam_table`, on plain integers (no device needed): tensor i has numels[i] fp32 elements at the given
    addresses, 0 = null (grad: the parameter takes no step this time; ema: it has no average).  Every tensor is cut at
    multiples of ADAM_CHUNK elements; a tensor with neither gradient nor average, or without elements, emits nothing.
    Returns (rows, owner, launches): rows (n, 6) int64 in the layout of `hfl_adam_chunk` (five addresses, then
    count | slot % ADAM_MAX_SLOTS << 32), owner (n,) the index of each row's tensor, launches a list of (first row, rows,
    first slot): rows are ordered so that every run of ADAM_MAX_SLOTS consecutive slots is one contiguous launch."""
    rows, owner = [], []
    for i, n in enumerate(numels):
        if n == 0 or (not grad_ptrs[i] and not ema_ptrs[i]):
            continue
        slot = int(slots[i]) if grad_ptrs[i] else 0
        if slot < 0:
            raise ValueError('adam_chunk_rows: negative slot %d' % slot)
        off = np.arange(0, n, ADAM_CHUNK, dtype=np.int64)
        chunk = np.empty((off.shape[0], 7), dtype=np.int64)
        for col, base in enumerate((param_ptrs[i], grad_ptrs[i], exp_avg_ptrs[i], exp_avg_sq_ptrs[i], ema_ptrs[i])):
            chunk[:, col] = base + 4 * off if base and (col in (0, 4) or grad_ptrs[i]) else 0
        chunk[:, 5] = np.minimum(n - off, ADAM_CHUNK) | ((slot % ADAM_MAX_SLOTS) << 32)
        chunk[:, 6] = slot // ADAM_MAX_SLOTS
        rows.append(chunk)
        owner.append(np.full(off.shape[0], i, dtype=np.int64))
    if not rows:
        return np.empty((0, 6), dtype=np.int64), np.empty((0,), dtype=np.int64), []
    rows, owner = np.concatenate(rows, 0), np.concatenate(owner, 0)
    order = np.argsort(rows[:, 6], kind='stable')
    rows, owner = rows[order], owner[order]
    launches = []
    for group in np.unique(rows[:, 6]):
        idx = np.nonzero(rows[:, 6] == group)[0]
        launches.append((int(idx[0]), int(idx.shape[0]), int(group) * ADAM_MAX_SLOTS))
    return np.ascontiguousarray(rows[:, :6]), owner, launches


class AdamTable:
    """Device table of `adam_table` with what the host needs to refresh its gradient column."""
    __slots__ = ('table', 'n_chunks', 'launches', 'grad_rows', 'grad_owner', 'grad_offset')


def _adam_operands(params, grads, exp_avgs, exp_avg_sqs, emas):
    lists = [list(params), list(grads), list(exp_avgs), list(exp_avg_sqs), list(emas)]
    if len({len(x) for x in lists}) != 1:
        raise ValueError('adam_table: lists of %s entries' % '/'.join(str(len(x)) for x in lists))
    _dev(*(t for col in lists for t in col))
    for row in zip(*lists):
        p = row[0]
        for t in row:
            if t is None:
                continue
            if t.is_sparse:
                raise TypeError('adam_step takes dense tensors (sparse gradients are not supported)')
            if t.dtype != torch.float32:
                raise TypeError('adam_step takes float32 tensors, got %s' % t.dtype)
            if t.shape != p.shape:
                raise ValueError('adam_step: shapes %s and %s differ' % (tuple(t.shape), tuple(p.shape)))
            if not t.is_contiguous():
                raise ValueError('adam_step needs contiguous tensors')
        if row[1] is not None and (row[2] is None or row[3] is None):
            raise ValueError('adam_step: a parameter with a gradient needs exp_avg and exp_avg_sq')
    return lists


def adam_table(params, grads, exp_avgs, exp_avg_sqs, emas, slots) -> AdamTable:
    """Device table of `hfl_adam_chunk` entries for `adam_step`.  Six lists of one length: fp32 contiguous device tensors of
    the parameter's shape, `grads[i]` / `emas[i]` None where the parameter takes no step / has no average (the moments may
    then be None too), `slots[i]` the index of parameter i's hyper-parameters in the list `adam_step` receives.  Empty tensors
    are skipped.  The table holds raw pointers: it is valid only while every tensor keeps its `data_ptr()` (the caller
    revalidates; moved gradients alone are followed by `adam_refresh_grads`)."""
    params, grads, exp_avgs, exp_avg_sqs, emas = _adam_operands(params, grads, exp_avgs, exp_avg_sqs, emas)

    def ptrs(col):
        return [0 if t is None else t.data_ptr() for t in col]
    gp = ptrs(grads)
    rows, owner, launches = adam_chunk_rows([p.numel() for p in params], ptrs(params), gp, ptrs(exp_avgs), ptrs(exp_avg_sqs),
                                            ptrs(emas), slots)
    t = AdamTable()
    t.n_chunks, t.launches = int(rows.shape[0]), launches
    t.table = torch.from_numpy(rows).to(params[0].device) if t.n_chunks else None
    t.grad_rows = np.nonzero(rows[:, 1])[0]
    t.grad_owner = owner[t.grad_rows]
    t.grad_offset = rows[t.grad_rows, 1] - np.asarray(gp, dtype=np.int64)[t.grad_owner]
    if t.n_chunks and t.grad_rows.shape[0] != t.n_chunks:
        t.grad_rows = torch.from_numpy(t.grad_rows).to(params[0].device)
    else:
        t.grad_rows = None                                     # every row has a gradient: the column is written whole
    return t


def adam_refresh_grads(t: AdamTable, grads):
    """Rewrite the gradient column of `t` for gradient tensors at new addresses: the same parameters have gradients as when
    the table was built (the caller checks), of the same shapes; nothing else of the table changes."""
    grads = list(grads)
    _dev(*grads)
    for g in grads:
        if g is None:
            continue
        if g.is_sparse:
            raise TypeError('adam_step takes dense tensors (sparse gradients are not supported)')
        if g.dtype != torch.float32:
            raise TypeError('adam_step takes float32 tensors, got %s' % g.dtype)
        if not g.is_contiguous():
            raise ValueError('adam_step needs contiguous tensors')
    if t.n_chunks == 0 or t.grad_owner.shape[0] == 0:
        return
    base = np.asarray([0 if g is None else g.data_ptr() for g in grads], dtype=np.int64)[t.grad_owner]
    if (base == 0).any():
        raise ValueError('adam_refresh_grads: a parameter of the table lost its gradient; build a new table')
    col = torch.from_numpy(base + t.grad_offset).to(t.table.device)
    if t.grad_rows is None:
        t.table[:, 1] = col
    else:
        t.table[t.grad_rows, 1] = col


def adam_step(t: AdamTable, slots, w: float = 0.0):
    """One Adam / AdamW step (and EMA line, weight `w`) over every chunk of an `adam_table`: one launch per run of
    ADAM_MAX_SLOTS slots, i.e. one launch unless the parameters sit at more than ADAM_MAX_SLOTS distinct (group, step count)
    combinations.  `slots`: a list of `adam_slot(...)` tuples, indexed by the table's slot numbers."""
    if t.n_chunks == 0:
        return
    _dev(t.table)
    assert t.table.dtype == torch.int64 and t.table.is_contiguous() and tuple(t.table.shape) == (t.n_chunks, 6)
    lib, stream = _native.load(), _stream()
    for first, n, slot0 in t.launches:
        part = slots[slot0:slot0 + ADAM_MAX_SLOTS]
        arr = (_native.AdamSlot * max(len(part), 1))(*[_native.AdamSlot(*s) for s in part])
        check(lib.hfl_adam_step(t.table.data_ptr() + 48 * first, n, ctypes.addressof(arr) if part else None, len(part),
                                float(w), stream), 'hfl_adam_step')


def kd_rows(y: torch.Tensor, t: torch.Tensor, temperature: float):
    """Per row: KL(softmax(t / T) || softmax(y / T)) and its derivative (p - q) / T with respect to y.  y, t: (B, D) fp32,
    D a multiple of 64 up to 1024.  Returns (kl (B,), dkl_dy (B, D))."""
    _dev(y, t)
    if y.dim() != 2 or y.shape != t.shape:
        raise ValueError('kd_rows: (B, D) student and teacher rows of one shape expected, got %s and %s'
                         % (tuple(y.shape), tuple(t.shape)))
    y, t = _f32c(y), _f32c(t)
    b, d = y.shape
    kl = torch.empty(b, dtype=torch.float32, device=y.device)
    dkl = torch.empty((b, d), dtype=torch.float32, device=y.device)
    if b == 0:
        return kl, dkl
    check(_native.load().hfl_kd_rows(kl.data_ptr(), dkl.data_ptr(), y.data_ptr(), t.data_ptr(), b, d, float(temperature),
                                     _stream()), 'hfl_kd_rows')
    return kl, dkl


def smoothap_rows(sim: torch.Tensor, pos_u8: torch.Tensor, neg_u8: torch.Tensor, idx: torch.Tensor, tau: float, out=None):
    """Per query row q of the (B, B) similarity matrix: the smoothed AP over the selected positives idx[q, :] and its
    derivative with respect to the row (`hfl_smoothap_rows`).  sim: (B, B) fp32, contiguous; pos_u8, neg_u8: (B, B) uint8
    masks (non-zero = set), contiguous; idx: (B, P >= 1) int64, contiguous; a slot counts iff 0 <= idx < B and it points at a
    positive, a row without such a slot gets AP 0 and a zero gradient row.  B <= 17066 (the row, its gradient and the masks sit
    in LDS).  Nothing is converted or copied: an operand of another dtype, shape or layout is an error.  `out`: an
    (ap (B,), dap_ds (B, B)) pair of contiguous fp32 tensors to write into.  Returns (ap (B,), dap_ds (B, B))."""
    operands = (('sim', sim), ('pos_u8', pos_u8), ('neg_u8', neg_u8), ('idx', idx))
    for name, t in operands[1:]:
        if t.device != sim.device:
            raise ValueError('smoothap_rows: %s on %s, sim on %s' % (name, t.device, sim.device))
    _dev(sim, pos_u8, neg_u8, idx)
    if sim.dtype != torch.float32:
        raise TypeError('smoothap_rows: float32 sim expected, got %s' % sim.dtype)
    if sim.dim() != 2 or sim.shape[0] != sim.shape[1] or sim.shape[0] < 1:
        raise ValueError('smoothap_rows: a (B, B) similarity matrix with B >= 1 expected, got %s' % (tuple(sim.shape),))
    b = sim.shape[0]
    for name, t in operands[1:3]:
        if t.dtype != torch.uint8:
            raise TypeError('smoothap_rows: uint8 %s expected, got %s' % (name, t.dtype))
        if tuple(t.shape) != (b, b):
            raise ValueError('smoothap_rows: (%d, %d) %s expected, got %s' % (b, b, name, tuple(t.shape)))
    if idx.dtype != torch.int64:
        raise TypeError('smoothap_rows: int64 idx expected, got %s' % idx.dtype)
    if idx.dim() != 2 or idx.shape[0] != b or idx.shape[1] < 1:
        raise ValueError('smoothap_rows: (%d, P >= 1) idx expected, got %s' % (b, tuple(idx.shape)))
    for name, t in operands:
        if not t.is_contiguous():
            raise ValueError('smoothap_rows: %s must be contiguous (strides %s)' % (name, tuple(t.stride())))
    tau = float(tau)
    if not tau > 0.0:
        raise ValueError('smoothap_rows: tau > 0 expected, got %r' % (tau,))
    if out is None:
        ap = torch.empty(b, dtype=torch.float32, device=sim.device)
        dap = torch.empty((b, b), dtype=torch.float32, device=sim.device)
    else:
        ap, dap = out
        for name, t, shape in (('out[0]', ap, (b,)), ('out[1]', dap, (b, b))):
            if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != sim.device:
                raise ValueError('smoothap_rows: %s must be a contiguous float32 %s tensor on %s' % (name, shape, sim.device))
    check(_native.load().hfl_smoothap_rows(ap.data_ptr(), dap.data_ptr(), sim.data_ptr(), pos_u8.data_ptr(), neg_u8.data_ptr(),
                                           idx.data_ptr(), b, idx.shape[1], tau, _stream()), 'hfl_smoothap_rows')
    return ap, dap


def pairwise_dist(emb: torch.Tensor):
    """dist[i, j] = ||emb[i] - emb[j]||, summed over the differences themselves (`hfl_pairwise_dist`).  emb: (B, D) fp32,
    any B >= 1 and D >= 1.  Returns (B, B) fp32: bitwise symmetric, exactly 0 on the diagonal and between equal rows."""
    _dev(emb)
    if emb.dim() != 2 or emb.shape[0] < 1 or emb.shape[1] < 1:
        raise ValueError('pairwise_dist: a (B, D) matrix with B >= 1 and D >= 1 expected, got %s' % (tuple(emb.shape),))
    emb = _f32c(emb)
    b, d = emb.shape
    dist = torch.empty((b, b), dtype=torch.float32, device=emb.device)
    check(_native.load().hfl_pairwise_dist(dist.data_ptr(), emb.data_ptr(), b, d, _stream()), 'hfl_pairwise_dist')
    return dist


def pairwise_dist_bwd(grad_dist: torch.Tensor, dist: torch.Tensor, emb: torch.Tensor):
    """Gradient of sum(grad_dist * pairwise_dist(emb)) with respect to emb (`hfl_pairwise_dist_bwd`): row i is
    sum_j (grad_dist[i, j] + grad_dist[j, i]) (emb[i] - emb[j]) / dist[i, j], pairs at distance 0 contributing nothing.
    grad_dist: any (B, B) fp32 matrix; dist: `pairwise_dist(emb)`; emb: (B, D) fp32.  Returns (B, D) fp32."""
    _dev(grad_dist, dist, emb)
    if emb.dim() != 2 or emb.shape[0] < 1 or emb.shape[1] < 1:
        raise ValueError('pairwise_dist_bwd: a (B, D) matrix with B >= 1 and D >= 1 expected, got %s' % (tuple(emb.shape),))
    b, d = emb.shape
    if tuple(grad_dist.shape) != (b, b) or tuple(dist.shape) != (b, b):
        raise ValueError('pairwise_dist_bwd: (%d, %d) grad_dist and dist expected for %d rows, got %s and %s'
                         % (b, b, b, tuple(grad_dist.shape), tuple(dist.shape)))
    grad_dist, dist, emb = _f32c(grad_dist), _f32c(dist), _f32c(emb)
    d_emb = torch.empty((b, d), dtype=torch.float32, device=emb.device)
    check(_native.load().hfl_pairwise_dist_bwd(d_emb.data_ptr(), grad_dist.data_ptr(), dist.data_ptr(), emb.data_ptr(), b, d,
                                               _stream()), 'hfl_pairwise_dist_bwd')
    return d_emb


BATCH_HARD_TRIPLET, BATCH_HARD_CONTRASTIVE = 0, 1          # the mode argument of hfl_batch_hard_terms / hfl_batch_hard_grad


def _batch_hard_rows(who, emb):
    _dev(emb)
    if emb.dim() != 2 or emb.shape[0] < 1 or emb.shape[1] < 1:
        raise ValueError('%s: a (B, D) matrix with B >= 1 and D >= 1 expected, got %s' % (who, tuple(emb.shape)))
    return _f32c(emb)


def _batch_hard_vectors(who, emb, vectors):
    """(B,) contiguous vectors of the given dtypes on emb's device; nothing is converted."""
    b = emb.shape[0]
    for name, t, dtype in vectors:
        if t.device != emb.device:
            raise ValueError('%s: %s on %s, emb on %s' % (who, name, t.device, emb.device))
        if t.dtype != dtype:
            raise TypeError('%s: %s %s expected, got %s' % (who, dtype, name, t.dtype))
        if tuple(t.shape) != (b,) or not t.is_contiguous():
            raise ValueError('%s: a contiguous (%d,) %s expected, got %s' % (who, b, name, tuple(t.shape)))


def batch_hard_mine(emb: torch.Tensor, pos_u8: torch.Tensor, neg_u8: torch.Tensor):
    """Hardest positive and hardest negative of every row (`hfl_batch_hard_mine`): p[a] = the first arg-max of
    `pairwise_dist(emb)[a]` over the columns with pos_u8[a] != 0, n[a] = the first arg-min over those with neg_u8[a] != 0, and
    the two distances, bit for bit the entries of that matrix, which is never formed.  emb: (B, D) fp32, any B >= 1 and
    D >= 1; pos_u8, neg_u8: (B, B) uint8, contiguous (an operand of another dtype, shape or layout is an error).
    Returns (p (B,) int32, d_ap (B,) fp32, n (B,) int32, d_an (B,) fp32); index -1 and distance 0 where a row has none."""
    emb = _batch_hard_rows('batch_hard_mine', emb)
    b, d = emb.shape
    for name, t in (('pos_u8', pos_u8), ('neg_u8', neg_u8)):
        if t.device != emb.device:
            raise ValueError('batch_hard_mine: %s on %s, emb on %s' % (name, t.device, emb.device))
        if t.dtype != torch.uint8:
            raise TypeError('batch_hard_mine: uint8 %s expected, got %s' % (name, t.dtype))
        if tuple(t.shape) != (b, b):
            raise ValueError('batch_hard_mine: (%d, %d) %s expected, got %s' % (b, b, name, tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError('batch_hard_mine: %s must be contiguous (strides %s)' % (name, tuple(t.stride())))
    lib = _native.load()
    work = torch.empty(int(lib.hfl_batch_hard_mine_workspace(b)), dtype=torch.uint8, device=emb.device)
    idx = torch.empty((2, b), dtype=torch.int32, device=emb.device)
    dist = torch.empty((2, b), dtype=torch.float32, device=emb.device)
    check(lib.hfl_batch_hard_mine(idx[0].data_ptr(), dist[0].data_ptr(), idx[1].data_ptr(), dist[1].data_ptr(), work.data_ptr(),
                                  emb.data_ptr(), pos_u8.data_ptr(), neg_u8.data_ptr(), b, d, _stream()), 'hfl_batch_hard_mine')
    return idx[0], dist[0], idx[1], dist[1]


def batch_hard_terms(emb: torch.Tensor, p: torch.Tensor, d_ap: torch.Tensor, n: torch.Tensor, d_an: torch.Tensor, mode: int,
                     margin0: float, margin1: float = 0.0):
    """Loss terms of mined triples, one entry point for both losses (`hfl_batch_hard_terms`).  emb: (B, D) fp32; p, n: (B,) int32 and d_ap, d_an:
    (B,) fp32 as `batch_hard_mine` returns them.  mode BATCH_HARD_TRIPLET: margin0 is the margin; BATCH_HARD_CONTRASTIVE:
    margin0, margin1 are pos_margin, neg_margin.  Returns (stats (16,) float64, scale (4,) fp32, d_pn (B,) fp32,
    flags (B,) int32) on the device, laid out as include/hotformerloc_hip.h says; scale[2] is the loss."""
    emb = _batch_hard_rows('batch_hard_terms', emb)
    _batch_hard_vectors('batch_hard_terms', emb, (('p', p, torch.int32), ('d_ap', d_ap, torch.float32),
                                                  ('n', n, torch.int32), ('d_an', d_an, torch.float32)))
    if mode not in (BATCH_HARD_TRIPLET, BATCH_HARD_CONTRASTIVE):
        raise ValueError('batch_hard_terms: mode 0 (triplet) or 1 (contrastive) expected, got %r' % (mode,))
    b, d = emb.shape
    stats = torch.empty(16, dtype=torch.float64, device=emb.device)
    scale = torch.empty(4, dtype=torch.float32, device=emb.device)
    d_pn = torch.empty(b, dtype=torch.float32, device=emb.device)
    flags = torch.empty(b, dtype=torch.int32, device=emb.device)
    lib = _native.load()
    work = torch.empty(int(lib.hfl_batch_hard_terms_workspace(b)) // 8, dtype=torch.float64, device=emb.device)
    check(lib.hfl_batch_hard_terms(stats.data_ptr(), scale.data_ptr(), d_pn.data_ptr(), flags.data_ptr(), work.data_ptr(),
                                   emb.data_ptr(), p.data_ptr(), d_ap.data_ptr(), n.data_ptr(), d_an.data_ptr(), b, d,
                                   int(mode), float(margin0), float(margin1), _stream()), 'hfl_batch_hard_terms')
    return stats, scale, d_pn, flags


def batch_hard_grad(emb: torch.Tensor, p: torch.Tensor, n: torch.Tensor, d_ap: torch.Tensor, d_an: torch.Tensor,
                    d_pn: torch.Tensor, flags: torch.Tensor, scale: torch.Tensor, mode: int):
    """Gradient of the loss of `batch_hard_terms` (same mode) with respect to emb for unit upstream gradient
    (`hfl_batch_hard_grad`), from what `batch_hard_mine` and `batch_hard_terms` returned.  Returns (B, D) fp32."""
    emb = _batch_hard_rows('batch_hard_grad', emb)
    _batch_hard_vectors('batch_hard_grad', emb, (('p', p, torch.int32), ('n', n, torch.int32), ('d_ap', d_ap, torch.float32),
                                                 ('d_an', d_an, torch.float32), ('d_pn', d_pn, torch.float32),
                                                 ('flags', flags, torch.int32)))
    if scale.device != emb.device or scale.dtype != torch.float32 or tuple(scale.shape) != (4,) or not scale.is_contiguous():
        raise ValueError('batch_hard_grad: scale must be the contiguous (4,) float32 vector of batch_hard_terms')
    if mode not in (BATCH_HARD_TRIPLET, BATCH_HARD_CONTRASTIVE):
        raise ValueError('batch_hard_grad: mode 0 (triplet) or 1 (contrastive) expected, got %r' % (mode,))
    b, d = emb.shape
    d_emb = torch.empty((b, d), dtype=torch.float32, device=emb.device)
    check(_native.load().hfl_batch_hard_grad(d_emb.data_ptr(), emb.data_ptr(), p.data_ptr(), n.data_ptr(), d_ap.data_ptr(),
                                             d_an.data_ptr(), d_pn.data_ptr(), flags.data_ptr(), scale.data_ptr(), b, d, int(mode),
                                             _stream()), 'hfl_batch_hard_grad')
    return d_emb


BATCH_MASKS_LDS_ENTRIES = 4096        # HFL_BATCH_MASKS_LDS_ENTRIES: entries of each list a workgroup stages in LDS


def batch_masks(labels: torch.Tensor, pos_off: torch.Tensor, pos_idx: torch.Tensor, nn_off: torch.Tensor, nn_idx: torch.Tensor,
                n_elems: int, return_counts: bool = False, out=None):
    """`hfl_batch_masks`: pos[i, j] = labels[j] in positives[labels[i]], neg[i, j] = labels[j] not in non_negatives[labels[i]].
    labels (B,) int64 on the GPU with every value in [0, n_elems) (the caller checks); the two CSRs as (n_elems + 1,) int64
    offsets and int32 ids, each id tensor with at least one element of storage.  `out`: a pair of contiguous (B, B) bool or
    uint8 tensors to write into.  Returns (pos (B, B) bool, neg (B, B) bool, counts (B, 2) int32 or None)."""
    _dev(labels, pos_off, pos_idx, nn_off, nn_idx)
    if labels.dtype != torch.int64 or labels.dim() != 1 or labels.shape[0] < 1 or not labels.is_contiguous():
        raise TypeError('batch_masks: a contiguous (B,) int64 label tensor with B >= 1 expected')
    n_elems = int(n_elems)
    for off, idx in ((pos_off, pos_idx), (nn_off, nn_idx)):
        if off.dtype != torch.int64 or idx.dtype != torch.int32 or not off.is_contiguous() or not idx.is_contiguous() \
                or off.dim() != 1 or idx.dim() != 1 or off.shape[0] != n_elems + 1 or idx.shape[0] < 1:
            raise TypeError('batch_masks: CSR of %d lists as (%d,) int64 offsets and non-empty int32 ids expected'
                            % (n_elems, n_elems + 1))
    b = labels.shape[0]
    if out is None:
        pos = torch.empty((b, b), dtype=torch.bool, device=labels.device)
        neg = torch.empty((b, b), dtype=torch.bool, device=labels.device)
    else:
        pos, neg = out
        _dev(pos, neg)
        for m in (pos, neg):
            if m.dtype not in (torch.bool, torch.uint8) or tuple(m.shape) != (b, b) or not m.is_contiguous():
                raise TypeError('batch_masks: out is a pair of contiguous (%d, %d) bool or uint8 tensors' % (b, b))
    counts = torch.empty((b, 2), dtype=torch.int32, device=labels.device) if return_counts else None
    check(_native.load().hfl_batch_masks(pos.data_ptr(), neg.data_ptr(), counts.data_ptr() if return_counts else None,
                                         labels.data_ptr(), b, pos_off.data_ptr(), pos_idx.data_ptr(), nn_off.data_ptr(),
                                         nn_idx.data_ptr(), n_elems, _stream()), 'hfl_batch_masks')
    return pos, neg, counts


RADIUS_ROWS = 8                        # HFL_RADIUS_ROWS: query rows (one wave each) of a workgroup
RADIUS_TILE = 2048                     # HFL_RADIUS_TILE: database positions of the LDS tile those rows share


def _radius_check(queries: torch.Tensor, database: torch.Tensor):
    _dev(queries, database)
    for x in (queries, database):
        if x.dtype != torch.float64 or x.dim() != 2 or x.shape[1] != 2 or x.shape[0] < 1 or not x.is_contiguous():
            raise TypeError('radius_lists: contiguous (rows >= 1, 2) float64 positions expected')
    if database.shape[0] >= 2 ** 31:
        raise ValueError('radius_lists: %d database positions, ids must fit int32' % database.shape[0])


def radius_counts(queries: torch.Tensor, database: torch.Tensor, r_a: float, r_b: float, exclude_self: bool = False):
    """The count pass of `hfl_radius_lists`: (Q, 2) int32, per query the number of database positions with
    dx*dx + dy*dy <= r_a*r_a and <= r_b*r_b in float64 (`exclude_self`: without j == i in the first column)."""
    _radius_check(queries, database)
    counts = torch.empty((queries.shape[0], 2), dtype=torch.int32, device=queries.device)
    check(_native.load().hfl_radius_lists(counts.data_ptr(), None, None, None, None, queries.data_ptr(), queries.shape[0],
                                          database.data_ptr(), database.shape[0], float(r_a), float(r_b), int(exclude_self),
                                          _stream()), 'hfl_radius_lists (count)')
    return counts


def radius_lists(queries: torch.Tensor, database: torch.Tensor, r_a: float, r_b: float, exclude_self: bool = False,
                 want_b: bool = True):
    """Both passes of `hfl_radius_lists` around one `torch.cumsum`: (off_a, idx_a, off_b, idx_b), (Q + 1,) int64 offsets and
    int32 ids ascending within every list (`want_b=False`: the second family is None, None and is not written).  A family
    without any entry keeps one element of storage (a (1,) id tensor holding 0, as `TupleIndex` pads its own): kernels take
    no null pointer; `off[-1]` is the number of entries.  One device-to-host read (the totals) between the passes."""
    counts = radius_counts(queries, database, r_a, r_b, exclude_self)
    n_q = queries.shape[0]
    off = torch.zeros((2, n_q + 1), dtype=torch.int64, device=queries.device)
    off[:, 1:] = torch.cumsum(counts.t(), dim=1)
    total_a, total_b = (int(v) for v in off[:, -1].tolist())
    ids = lambda total: (torch.empty(total, dtype=torch.int32, device=queries.device) if total      # noqa: E731
                         else torch.zeros(1, dtype=torch.int32, device=queries.device))
    idx_a, idx_b = ids(total_a), ids(total_b) if want_b else None
    off_a, off_b = off[0], off[1]
    if total_a > 0 or (want_b and total_b > 0):
        check(_native.load().hfl_radius_lists(None, idx_a.data_ptr(), idx_b.data_ptr() if want_b else None, off_a.data_ptr(),
                                              off_b.data_ptr() if want_b else None, queries.data_ptr(), n_q,
                                              database.data_ptr(), database.shape[0], float(r_a), float(r_b),
                                              int(exclude_self), _stream()), 'hfl_radius_lists (fill)')
    return (off_a, idx_a, off_b, idx_b) if want_b else (off_a, idx_a, None, None)


OVERLAP_ROWS = 512                     # HFL_OVERLAP_ROWS: query rows of a workgroup of hfl_nn_dist (two per thread)
OVERLAP_TILE = 2048                    # HFL_OVERLAP_TILE: target points of the LDS tile those rows share
OVERLAP_MAX_TAUS = 8                   # HFL_OVERLAP_MAX_TAUS: thresholds of one hfl_pair_stats launch


def _points_check(what: str, points: torch.Tensor):
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3 or not points.is_contiguous():
        raise TypeError('%s: contiguous (P, 3) float32 points expected' % what)


def _vector_check(what: str, t: torch.Tensor, dtype, n=None, kind: str = 'vector'):
    if t.dtype != dtype or t.dim() != 1 or not t.is_contiguous() or (n is not None and t.shape[0] != n):
        raise TypeError('%s: contiguous (%s,) %s %s expected'
                        % (what, 'n' if n is None else n, str(dtype).replace('torch.', ''), kind))


def _offsets_check(what: str, offsets: torch.Tensor):
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.shape[0] < 2 or not offsets.is_contiguous():
        raise TypeError('%s: contiguous (B + 1,) int64 cloud offsets with B >= 1 expected' % what)


def _ragged_check(what: str, points: torch.Tensor, offsets: torch.Tensor) -> int:
    """a ragged batch (of clouds, or of the clouds of pairs) on the current device -> its number of clouds"""
    _dev(points, offsets)
    _points_check(what, points)
    _offsets_check(what, offsets)
    return int(offsets.shape[0]) - 1


def _some(t: torch.Tensor):
    """`t`, or one zero row of its kind where it has none: kernels take no null pointer (the row is never read)."""
    return t if t.shape[0] else torch.zeros((1,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)


def overlap_tiles(lengths):
    """The tile table of `hfl_nn_dist` from the query clouds' lengths on the host: (n_tiles, 2) int64 numpy rows of (pair,
    first query row), OVERLAP_ROWS rows of one pair per workgroup, pairs in order; an empty cloud has no tile."""
    return pair_tiles(lengths)[0]


def pair_tiles(lengths, rows=OVERLAP_ROWS):
    """`overlap_tiles` and, beside it, the (P + 1,) int64 offsets of every pair's rows in that table; `rows` rows of one pair
    per workgroup."""
    lengths = np.asarray(lengths, dtype=np.int64)
    tile_off = np.zeros(lengths.shape[0] + 1, np.int64)
    np.cumsum(-(-lengths // rows), out=tile_off[1:])
    pair = np.repeat(np.arange(lengths.shape[0], dtype=np.int64), np.diff(tile_off))
    start = np.cumsum(lengths) - lengths
    row = start[pair] + (np.arange(pair.shape[0], dtype=np.int64) - tile_off[pair]) * rows
    return np.stack([pair, row], 1), tile_off


def _pair_batch_check(what: str, queries: torch.Tensor, q_offsets: torch.Tensor, targets: torch.Tensor, t_offsets: torch.Tensor,
                      tiles: torch.Tensor, sides=('query', 'target'), rows_check=_points_check) -> int:
    """What every launch of the pair scan takes: two ragged batches of the same P pairs and the (n_tiles, 2) int64 tile
    table, on the current device -> P.  The order of the checks: the device of all five, the query side's rows and
    offsets, the target side's, the number of pairs, the tile table; what a caller checks besides comes after."""
    _dev(queries, q_offsets, targets, t_offsets, tiles)
    for rows, offsets in ((queries, q_offsets), (targets, t_offsets)):
        rows_check(what, rows)
        _offsets_check(what, offsets)
    pairs = int(q_offsets.shape[0]) - 1
    if int(t_offsets.shape[0]) - 1 != pairs:
        raise ValueError('%s: the %s batch and the %s batch differ in their number of pairs' % ((what,) + tuple(sides)))
    if tiles.dtype != torch.int64 or tiles.dim() != 2 or tiles.shape[1] != 2 or not tiles.is_contiguous():
        raise TypeError('%s: contiguous (n_tiles, 2) int64 tile table expected' % what)
    return pairs


def transform_points(points: torch.Tensor, offsets: torch.Tensor, transforms: torch.Tensor):
    """`hfl_transform_points`: points (N, 3) fp32, offsets (P + 1,) int64 with offsets[0] = 0 and offsets[P] = N (the caller
    checks) and transforms (P, 12) fp32, a row-major (R | t) per pair, all on the GPU -> R_p x + t_p for every row."""
    pairs = _ragged_check('transform_points', points, offsets)
    _dev(transforms)
    if transforms.dtype != torch.float32 or tuple(transforms.shape) != (pairs, 12) or not transforms.is_contiguous():
        raise TypeError('transform_points: contiguous (%d, 12) float32 transforms expected' % pairs)
    out = torch.empty_like(points)
    if points.shape[0]:
        check(_native.load().hfl_transform_points(out.data_ptr(), points.data_ptr(), offsets.data_ptr(), transforms.data_ptr(),
                                                  pairs, int(points.shape[0]), _stream()), 'hfl_transform_points')
    return out


def nn_dist(queries: torch.Tensor, q_offsets: torch.Tensor, targets: torch.Tensor, t_offsets: torch.Tensor,
            tiles: torch.Tensor):
    """`hfl_nn_dist`: two ragged batches of the same P pairs and the (n_tiles, 2) int64 device copy of `overlap_tiles` ->
    (dist (Nq,) fp32, idx (Nq,) int32): every query's distance to the nearest point of its pair's target cloud and that
    point's index within the cloud, +inf and -1 where the cloud is empty.  Rows the table does not cover stay unwritten."""
    pairs = _pair_batch_check('nn_dist', queries, q_offsets, targets, t_offsets, tiles)
    n_q = int(queries.shape[0])
    dist = torch.empty(n_q, dtype=torch.float32, device=queries.device)
    idx = torch.empty(n_q, dtype=torch.int32, device=queries.device)
    if n_q and tiles.shape[0]:
        check(_native.load().hfl_nn_dist(dist.data_ptr(), idx.data_ptr(), queries.data_ptr(), q_offsets.data_ptr(), n_q,
                                         _some(targets).data_ptr(), t_offsets.data_ptr(), int(targets.shape[0]),
                                         tiles.data_ptr(), int(tiles.shape[0]), pairs, _stream()), 'hfl_nn_dist')
    return dist, idx


def pair_stats(dist: torch.Tensor, offsets: torch.Tensor, taus=()):
    """`hfl_pair_stats`: dist (N,) fp32 and offsets (P + 1,) int64 on the GPU, up to OVERLAP_MAX_TAUS thresholds ->
    (sums (P, 2) float64: the sum of a pair's distances and of their squares, counts (P, K + 1) int64: the distances
    <= taus[k] compared in fp32, and in the last column the +inf ones, which are in no other figure)."""
    _dev(dist, offsets)
    _vector_check('pair_stats', dist, torch.float32, kind='distances')
    _offsets_check('pair_stats', offsets)
    taus = [float(t) for t in taus]
    if len(taus) > OVERLAP_MAX_TAUS:
        raise ValueError('pair_stats: at most %d thresholds in one launch, got %d' % (OVERLAP_MAX_TAUS, len(taus)))
    pairs = int(offsets.shape[0]) - 1
    sums = torch.empty((pairs, 2), dtype=torch.float64, device=dist.device)
    counts = torch.empty((pairs, len(taus) + 1), dtype=torch.int64, device=dist.device)
    host_taus = (ctypes.c_float * OVERLAP_MAX_TAUS)(*taus)
    check(_native.load().hfl_pair_stats(sums.data_ptr(), counts.data_ptr(), _some(dist).data_ptr(), offsets.data_ptr(),
                                        int(dist.shape[0]), pairs, host_taus, len(taus), _stream()), 'hfl_pair_stats')
    return sums, counts


ICP_SUMS = 17                          # HFL_ICP_SUMS: n, Sp (3), Sq (3), Spq (9), sum d^2
ICP_PLANE_SUMS = 29                    # HFL_ICP_PLANE_SUMS: n, sum d^2, g (6), the upper triangle of A row-major (21)


def _icp_state_check(what: str, state: torch.Tensor, istate: torch.Tensor, pairs: int):
    _dev(state, istate)
    if state.dtype != torch.float64 or tuple(state.shape) != (pairs, 16) or not state.is_contiguous():
        raise TypeError('%s: contiguous (%d, 16) float64 state expected' % (what, pairs))
    if istate.dtype != torch.int32 or tuple(istate.shape) != (pairs, 2) or not istate.is_contiguous():
        raise TypeError('%s: contiguous (%d, 2) int32 iterations / status expected' % (what, pairs))


def _partials_check(what: str, partials: torch.Tensor, rows: int, n_sums: int):
    """the per-workgroup sums an evaluation writes and `icp_solve` reads: at least `rows` rows of `n_sums`"""
    _dev(partials)
    if partials.dtype != torch.float64 or partials.dim() != 2 or partials.shape[0] < rows or \
            partials.shape[1] != n_sums or not partials.is_contiguous():
        raise TypeError('%s: contiguous (>= %d, %d) float64 partials expected' % (what, rows, n_sums))


def icp_correspond(source: torch.Tensor, s_offsets: torch.Tensor, targets: torch.Tensor, t_offsets: torch.Tensor,
                   tiles: torch.Tensor, state: torch.Tensor, istate: torch.Tensor, max_dist: float, partials=None,
                   want_rows: bool = False, target_normals: torch.Tensor = None, source_normals: torch.Tensor = None,
                   epsilon: float = 1e-3):
    """`hfl_icp_correspond`: one evaluation of every RUNNING pair.  source / targets: two ragged batches of the same P pairs;
    tiles: the device copy of `overlap_tiles` of the source lengths; state (P, 16) float64 and istate (P, 2) int32 as the
    header lays them out.  -> (partials (n_tiles, ICP_SUMS) float64, dist, idx): `partials` is written in place where one is
    given (the iteration loop allocates once), dist (Ns,) fp32 and idx (Ns,) int32 are None unless `want_rows`.  Rows of
    pairs that are not RUNNING stay unwritten.  With `target_normals` ((Nt, 3) fp32, the rows of `targets`) it is
    `hfl_icp_correspond_plane` and the partials have ICP_PLANE_SUMS columns; with `source_normals` ((Ns, 3) fp32, the rows
    of `source`) as well it is `hfl_icp_correspond_generalized` with the covariance `epsilon` in (0, 1]."""
    plane = target_normals is not None
    generalized = source_normals is not None
    if generalized and not plane:
        raise ValueError('icp_correspond: source_normals go with target_normals')
    n_sums = ICP_PLANE_SUMS if plane else ICP_SUMS
    what = 'icp_correspond_generalized' if generalized else 'icp_correspond_plane' if plane else 'icp_correspond'
    name = 'hfl_' + what
    pairs = _pair_batch_check(what, source, s_offsets, targets, t_offsets, tiles, ('source', 'target'))
    if plane:
        _dev(target_normals)
        _points_check(what, target_normals)
        if target_normals.shape[0] != targets.shape[0]:
            raise ValueError('%s: %d target normals for %d target points' % (what, target_normals.shape[0], targets.shape[0]))
    if generalized:
        _dev(source_normals)
        _points_check(what, source_normals)
        if source_normals.shape[0] != source.shape[0]:
            raise ValueError('%s: %d source normals for %d source points' % (what, source_normals.shape[0], source.shape[0]))
        if not 0.0 < float(epsilon) <= 1.0:
            raise ValueError('%s: epsilon must lie in (0, 1], got %r' % (what, epsilon))
    _icp_state_check(what, state, istate, pairs)
    n_s, n_tiles = int(source.shape[0]), int(tiles.shape[0])
    if partials is None:
        partials = torch.empty((max(n_tiles, 1), n_sums), dtype=torch.float64, device=source.device)
    _partials_check(what, partials, n_tiles, n_sums)
    dist = torch.empty(n_s, dtype=torch.float32, device=source.device) if want_rows else None
    idx = torch.empty(n_s, dtype=torch.int32, device=source.device) if want_rows else None
    if n_tiles:
        normals = (_some(target_normals).data_ptr(),) if plane else ()          # the one argument the plane entry point adds
        s_normals = (source_normals.data_ptr(),) if generalized else ()         # and the two of the generalized one
        eps = (float(epsilon),) if generalized else ()
        check(getattr(_native.load(), name)(
            partials.data_ptr(), dist.data_ptr() if want_rows else None, idx.data_ptr() if want_rows else None,
            source.data_ptr(), *s_normals, s_offsets.data_ptr(), n_s, _some(targets).data_ptr(), *normals, t_offsets.data_ptr(),
            int(targets.shape[0]), tiles.data_ptr(), n_tiles, state.data_ptr(), istate.data_ptr(), float(max_dist), *eps, pairs,
            _stream()), name)
    return partials, dist, idx


def icp_solve(state: torch.Tensor, istate: torch.Tensor, partials: torch.Tensor, tile_offsets: torch.Tensor, n_tiles: int,
              s_offsets: torch.Tensor, min_correspondences: int, relative_fitness: float, relative_rmse: float, is_last: bool,
              want_sums: bool = False, plane: bool = False):
    """`hfl_icp_solve`: the stop rules and the rigid update of every RUNNING pair, in place in state / istate.  partials: at
    least `n_tiles` rows; tile_offsets (P + 1,) int64: the rows of every pair; s_offsets: the source offsets (the
    denominator of the fitness).  -> sums (P, ICP_SUMS) float64 with `want_sums` (a pair that is not RUNNING keeps zeros),
    else None.  `plane`: `hfl_icp_solve_plane` on partials of ICP_PLANE_SUMS columns."""
    n_sums = ICP_PLANE_SUMS if plane else ICP_SUMS
    name = 'hfl_icp_solve_plane' if plane else 'hfl_icp_solve'
    _offsets_check('icp_solve', tile_offsets)
    _offsets_check('icp_solve', s_offsets)
    pairs = int(s_offsets.shape[0]) - 1
    _icp_state_check('icp_solve', state, istate, pairs)
    _dev(partials, tile_offsets, s_offsets)
    if tile_offsets.shape[0] != pairs + 1:
        raise TypeError('icp_solve: (%d,) tile offsets expected' % (pairs + 1))
    _partials_check('icp_solve', partials, max(int(n_tiles), 1), n_sums)
    sums = torch.zeros((pairs, n_sums), dtype=torch.float64, device=state.device) if want_sums else None
    check(getattr(_native.load(), name)(state.data_ptr(), istate.data_ptr(), sums.data_ptr() if want_sums else None,
                                        partials.data_ptr(), tile_offsets.data_ptr(), int(n_tiles), s_offsets.data_ptr(), pairs,
                                        int(min_correspondences), float(relative_fitness), float(relative_rmse),
                                        int(bool(is_last)), _stream()), name)
    return sums


RANSAC_ROWS = 512                      # HFL_RANSAC_ROWS: hypotheses of a workgroup of hfl_ransac_score (two per thread)
RANSAC_TILE = 1024                     # HFL_RANSAC_TILE: correspondences of a workgroup of hfl_ransac_score / hfl_ransac_sums
RANSAC_NO_HYPOTHESIS = 5               # HFL_RANSAC_NO_HYPOTHESIS: a pair's status beside those of the ICP


def ransac_tiles(lengths):
    """The tile table of `hfl_ransac_score` and `hfl_ransac_sums` from the pairs' numbers of correspondences on the host:
    `pair_tiles` with RANSAC_TILE correspondences of one pair per workgroup -- ((n_tiles, 2) int64 numpy rows of (pair, first
    correspondence), pairs in order, none for a pair without correspondences; the (P + 1,) int64 offsets of every pair's
    rows in it)."""
    return pair_tiles(lengths, RANSAC_TILE)


def _ransac_corr_check(what: str, corr: torch.Tensor, c_offsets: torch.Tensor) -> int:
    """the gathered correspondences of P pairs on the current device -> P"""
    _dev(corr, c_offsets)
    if corr.dtype != torch.float32 or corr.dim() != 2 or corr.shape[1] != 6 or not corr.is_contiguous():
        raise TypeError('%s: contiguous (C, 6) float32 point pairs expected' % what)
    _offsets_check(what, c_offsets)
    return int(c_offsets.shape[0]) - 1


def _ransac_poses_check(what: str, poses: torch.Tensor, pairs: int) -> int:
    _dev(poses)
    if poses.dtype != torch.float32 or poses.dim() != 3 or poses.shape[0] != pairs or poses.shape[1] < 1 or \
            poses.shape[2] != 12 or not poses.is_contiguous() or poses.data_ptr() % 16:
        raise TypeError('%s: contiguous, 16-byte aligned (%d, H >= 1, 12) float32 poses expected' % (what, pairs))
    return int(poses.shape[1])


def _ransac_tiles_check(what: str, tiles: torch.Tensor):
    _dev(tiles)
    if tiles.dtype != torch.int64 or tiles.dim() != 2 or tiles.shape[1] != 2 or not tiles.is_contiguous():
        raise TypeError('%s: contiguous (n_tiles, 2) int64 tile table expected' % what)


def ransac_hypotheses(corr: torch.Tensor, c_offsets: torch.Tensor, hypotheses: int, seed: int, rho2: float):
    """`hfl_ransac_hypotheses`: corr (C, 6) fp32 rows (source point, target point) of P pairs under c_offsets (P + 1,) int64,
    all on the GPU -> (poses (P, H, 12) fp32, valid (P, H) uint8, draws (P, H, 3) int32); an invalid hypothesis has a pose of
    NaNs.  `rho2`: the squared edge-length ratio as a float64, 0 for no check."""
    pairs = _ransac_corr_check('ransac_hypotheses', corr, c_offsets)
    n_hyp = int(hypotheses)
    if n_hyp < 1 or not float(rho2) >= 0.0 or not 0 <= int(seed) < 2 ** 64:
        raise ValueError('ransac_hypotheses: hypotheses >= 1, rho2 >= 0 and a seed of 64 bits expected')
    poses = torch.empty((pairs, n_hyp, 12), dtype=torch.float32, device=corr.device)
    valid = torch.empty((pairs, n_hyp), dtype=torch.uint8, device=corr.device)
    draws = torch.empty((pairs, n_hyp, 3), dtype=torch.int32, device=corr.device)
    check(_native.load().hfl_ransac_hypotheses(poses.data_ptr(), valid.data_ptr(), draws.data_ptr(), _some(corr).data_ptr(),
                                               c_offsets.data_ptr(), int(corr.shape[0]), pairs, n_hyp, int(seed), float(rho2),
                                               _stream()), 'hfl_ransac_hypotheses')
    return poses, valid, draws


def ransac_score(corr: torch.Tensor, c_offsets: torch.Tensor, tiles: torch.Tensor, poses: torch.Tensor, valid: torch.Tensor,
                 d2_max: float):
    """`hfl_ransac_score`: the correspondences as above, the device copy of `ransac_tiles`, poses (P, H, 12) fp32 and valid
    (P, H) uint8 -> counts (P, H) int32: the correspondences with d2 <= d2_max (fp32) under each pose, -1 where valid is 0."""
    pairs = _ransac_corr_check('ransac_score', corr, c_offsets)
    _ransac_tiles_check('ransac_score', tiles)
    n_hyp = _ransac_poses_check('ransac_score', poses, pairs)
    _dev(valid)
    if valid.dtype != torch.uint8 or tuple(valid.shape) != (pairs, n_hyp) or not valid.is_contiguous():
        raise TypeError('ransac_score: contiguous (%d, %d) uint8 flags expected' % (pairs, n_hyp))
    counts = torch.empty((pairs, n_hyp), dtype=torch.int32, device=corr.device)
    check(_native.load().hfl_ransac_score(counts.data_ptr(), valid.data_ptr(), poses.data_ptr(), _some(corr).data_ptr(),
                                          c_offsets.data_ptr(), int(corr.shape[0]), _some(tiles).data_ptr(),
                                          int(tiles.shape[0]), pairs, n_hyp, float(d2_max), _stream()), 'hfl_ransac_score')
    return counts


def ransac_select(counts: torch.Tensor, poses: torch.Tensor):
    """`hfl_ransac_select`: counts (P, H) int32 and poses (P, H, 12) fp32 -> (state (P, 16) float64, istate (P, 2) int32,
    chosen (P, 3) int32): the pose of the largest count (the lowest h of equal ones) as the state `icp_solve` takes, RUNNING
    at iteration 0, and (h, its count, the number of counts >= 0); a pair whose counts are all -1 gets the identity,
    RANSAC_NO_HYPOTHESIS and (-1, -1, 0)."""
    _dev(counts)
    if counts.dtype != torch.int32 or counts.dim() != 2 or counts.shape[0] < 1 or not counts.is_contiguous():
        raise TypeError('ransac_select: contiguous (P >= 1, H) int32 counts expected')
    pairs = int(counts.shape[0])
    n_hyp = _ransac_poses_check('ransac_select', poses, pairs)
    if int(counts.shape[1]) != n_hyp:
        raise TypeError('ransac_select: %d counts for %d poses per pair' % (int(counts.shape[1]), n_hyp))
    state = torch.empty((pairs, 16), dtype=torch.float64, device=counts.device)
    istate = torch.empty((pairs, 2), dtype=torch.int32, device=counts.device)
    chosen = torch.empty((pairs, 3), dtype=torch.int32, device=counts.device)
    check(_native.load().hfl_ransac_select(state.data_ptr(), istate.data_ptr(), chosen.data_ptr(), counts.data_ptr(),
                                           poses.data_ptr(), pairs, n_hyp, _stream()), 'hfl_ransac_select')
    return state, istate, chosen


def ransac_sums(corr: torch.Tensor, c_offsets: torch.Tensor, tiles: torch.Tensor, state: torch.Tensor, istate: torch.Tensor,
                d2_max: float, partials=None):
    """`hfl_ransac_sums`: one evaluation of every RUNNING pair on its fixed correspondences -> partials (n_tiles, ICP_SUMS)
    float64, written in place where one is given: what `icp_solve` takes with the tile offsets of `ransac_tiles` and
    `c_offsets` as the source offsets."""
    pairs = _ransac_corr_check('ransac_sums', corr, c_offsets)
    _ransac_tiles_check('ransac_sums', tiles)
    _icp_state_check('ransac_sums', state, istate, pairs)
    n_tiles = int(tiles.shape[0])
    if partials is None:
        partials = torch.empty((max(n_tiles, 1), ICP_SUMS), dtype=torch.float64, device=corr.device)
    _partials_check('ransac_sums', partials, n_tiles, ICP_SUMS)
    if n_tiles:
        check(_native.load().hfl_ransac_sums(partials.data_ptr(), corr.data_ptr(), c_offsets.data_ptr(), int(corr.shape[0]),
                                             tiles.data_ptr(), n_tiles, state.data_ptr(), istate.data_ptr(), pairs,
                                             float(d2_max), _stream()), 'hfl_ransac_sums')
    return partials


SPECTRAL_ROWS = 512                    # HFL_SPECTRAL_ROWS: rows (correspondences) of a workgroup of hfl_spectral_matvec (two per thread)
SPECTRAL_TILE = 1024                   # HFL_SPECTRAL_TILE: columns of the LDS tile those rows share
SPECTRAL_SUMS = 3                      # HFL_SPECTRAL_SUMS: sum v w, sum v^2, sum w^2


def spectral_tiles(lengths):
    """The tile table of `hfl_spectral_matvec` from the pairs' numbers of correspondences on the host: `pair_tiles` with
    SPECTRAL_ROWS rows of one pair per workgroup -- ((n_tiles, 2) int64 numpy rows of (pair, first row), the (P + 1,) int64
    offsets of every pair's rows in it)."""
    return pair_tiles(lengths, SPECTRAL_ROWS)


def _spectral_check(what: str, corr: torch.Tensor, c_offsets: torch.Tensor, tile_offsets: torch.Tensor, w, partials,
                    n_tiles: int) -> int:
    pairs = _ransac_corr_check(what, corr, c_offsets)
    _dev(tile_offsets)
    _offsets_check(what, tile_offsets)
    if int(tile_offsets.shape[0]) != pairs + 1:
        raise TypeError('%s: (%d,) tile offsets expected' % (what, pairs + 1))
    if w is not None:
        _dev(w)
        _vector_check(what, w, torch.float32, int(corr.shape[0]), 'products')
        _partials_check(what, partials, n_tiles, SPECTRAL_SUMS)
    return pairs


def spectral_matvec(corr: torch.Tensor, c_offsets: torch.Tensor, tiles: torch.Tensor, tile_offsets: torch.Tensor,
                    inv_sigma2: float, w_in=None, partials_in=None, w_out=None, partials_out=None):
    """`hfl_spectral_matvec`: one step of the power iteration on the length-consistency matrix of every pair's
    correspondences (corr (C, 6) fp32 under c_offsets, as `ransac_score` takes them; tiles and tile_offsets: the device
    copies of `spectral_tiles`).  `w_in` (C,) fp32 and `partials_in` (n_tiles, SPECTRAL_SUMS) float64 are the previous step's
    results, which this step normalises as it loads them; without them it is the first step, v = 1.  -> (w (C,) fp32,
    partials (n_tiles, SPECTRAL_SUMS) float64), written in place where `w_out` / `partials_out` are given (not the inputs)."""
    what = 'spectral_matvec'
    _ransac_tiles_check(what, tiles)
    n_tiles, n_corr = int(tiles.shape[0]), int(corr.shape[0]) if corr.dim() else 0
    if (w_in is None) != (partials_in is None):
        raise TypeError('%s: w_in and partials_in come together' % what)
    pairs = _spectral_check(what, corr, c_offsets, tile_offsets, w_in, partials_in, n_tiles)
    if not (float(inv_sigma2) > 0.0 and np.isfinite(np.float32(inv_sigma2))):
        raise ValueError('%s: a finite inv_sigma2 > 0 expected' % what)
    if w_out is None:
        w_out = torch.zeros(n_corr, dtype=torch.float32, device=corr.device)
    if partials_out is None:
        partials_out = torch.zeros((max(n_tiles, 1), SPECTRAL_SUMS), dtype=torch.float64, device=corr.device)
    _spectral_check(what, corr, c_offsets, tile_offsets, w_out, partials_out, n_tiles)
    if w_in is not None and n_tiles and (w_in.data_ptr() == w_out.data_ptr() or partials_in.data_ptr() == partials_out.data_ptr()):
        raise ValueError('%s: a step cannot write where it reads' % what)
    if n_tiles:
        check(_native.load().hfl_spectral_matvec(
            w_out.data_ptr(), partials_out.data_ptr(), corr.data_ptr(), c_offsets.data_ptr(), n_corr, tiles.data_ptr(), n_tiles,
            tile_offsets.data_ptr(), None if w_in is None else w_in.data_ptr(),
            None if partials_in is None else partials_in.data_ptr(), pairs, float(inv_sigma2), _stream()), 'hfl_spectral_matvec')
    return w_out, partials_out


def spectral_finish(w: torch.Tensor, partials: torch.Tensor, n_tiles: int, tile_offsets: torch.Tensor, corr: torch.Tensor,
                    c_offsets: torch.Tensor, n_source: torch.Tensor):
    """`hfl_spectral_finish` on the last step's (w, partials): -> (eigenvalue (P,) float64, score (P,) float64 = eigenvalue /
    max(n_source, 1), weights (C,) fp32 = w / fp32(sqrt(sum w^2)) per pair); eigenvalue 0 and weights 0 where sum w^2 is 0.
    n_source: (P,) int64, every pair's number of source points."""
    what = 'spectral_finish'
    pairs = _spectral_check(what, corr, c_offsets, tile_offsets, w, partials, int(n_tiles))
    _dev(n_source)
    _vector_check(what, n_source, torch.int64, pairs, 'source sizes')
    eigenvalue = torch.empty(pairs, dtype=torch.float64, device=corr.device)
    score = torch.empty(pairs, dtype=torch.float64, device=corr.device)
    weights = torch.empty(int(corr.shape[0]), dtype=torch.float32, device=corr.device)
    check(_native.load().hfl_spectral_finish(eigenvalue.data_ptr(), score.data_ptr(), _some(weights).data_ptr(),
                                             _some(w).data_ptr(), partials.data_ptr(), int(n_tiles), tile_offsets.data_ptr(),
                                             c_offsets.data_ptr(), int(corr.shape[0]), n_source.data_ptr(), pairs, _stream()),
          'hfl_spectral_finish')
    return eigenvalue, score, weights


CONSENSUS_ROWS = 512                   # HFL_CONSENSUS_ROWS: rows (correspondences) of a workgroup of hfl_consensus_graph (two per thread)
CONSENSUS_TILE = 1024                  # HFL_CONSENSUS_TILE: columns of the LDS tile those rows share
CONSENSUS_MAX_CORRESPONDENCES = 16384  # HFL_CONSENSUS_MAX_CORRESPONDENCES: of one pair
CONSENSUS_MAX_SIZE = 64                # HFL_CONSENSUS_MAX_SIZE: the largest consensus set, the seed included


def consensus_tiles(lengths):
    """The tile table of `hfl_consensus_graph` from the pairs' numbers of correspondences on the host: `pair_tiles` with
    CONSENSUS_ROWS rows of one pair per workgroup."""
    return pair_tiles(lengths, CONSENSUS_ROWS)


def consensus_words(lengths):
    """Where every pair's bit matrix lies, from the pairs' numbers of correspondences on the host: ((P + 1,) int64 numpy word
    offsets, the last one the total; (P,) int64 words of a row, 4 ceil(C / 128))."""
    lengths = np.asarray(lengths, dtype=np.int64)
    row_words = 4 * (-(-lengths // 128))
    word_off = np.zeros(lengths.shape[0] + 1, np.int64)
    np.cumsum(lengths * row_words, out=word_off[1:])
    return word_off, row_words


def _consensus_graph_check(what: str, bits: torch.Tensor, word_offsets: torch.Tensor, pairs: int):
    _dev(bits, word_offsets)
    _vector_check(what, bits, torch.int32, None, 'bit matrices')
    _vector_check(what, word_offsets, torch.int64, pairs + 1, 'word offsets')
    if bits.data_ptr() % 16:
        raise TypeError('%s: 16-byte aligned bit matrices expected' % what)


def consensus_graph(corr: torch.Tensor, c_offsets: torch.Tensor, tiles: torch.Tensor, word_offsets: torch.Tensor, n_words: int,
                    distance: float):
    """`hfl_consensus_graph`: the compatibility graph of every pair's correspondences (corr (C, 6) fp32 under c_offsets, as
    `ransac_score` takes them; tiles: the device copy of `consensus_tiles`; word_offsets (P + 1,) int64: the device copy of
    `consensus_words`, n_words its last entry) -> (bits (n_words,) int32: every pair's row-major bit matrix, degree (C,)
    int32)."""
    what = 'consensus_graph'
    pairs = _ransac_corr_check(what, corr, c_offsets)
    _ransac_tiles_check(what, tiles)
    if not (float(distance) > 0.0 and np.isfinite(np.float32(distance)) and np.float32(distance) > 0.0):
        raise ValueError('%s: a distance that is a finite float32 > 0 expected' % what)
    bits = torch.empty(max(int(n_words), 4), dtype=torch.int32, device=corr.device)
    _consensus_graph_check(what, bits, word_offsets, pairs)
    degree = torch.zeros(int(corr.shape[0]), dtype=torch.int32, device=corr.device)
    if int(tiles.shape[0]):
        check(_native.load().hfl_consensus_graph(bits.data_ptr(), degree.data_ptr(), corr.data_ptr(), c_offsets.data_ptr(),
                                                 int(corr.shape[0]), tiles.data_ptr(), int(tiles.shape[0]),
                                                 word_offsets.data_ptr(), int(n_words), pairs, float(distance), _stream()),
              'hfl_consensus_graph')
    return bits, degree


def consensus_poses(corr: torch.Tensor, c_offsets: torch.Tensor, bits: torch.Tensor, word_offsets: torch.Tensor, n_words: int,
                    seeds: torch.Tensor, consensus_size: int):
    """`hfl_consensus_poses`: seeds (P, S) int32, a row of the pair or -1, against the graph `consensus_graph` wrote -> (poses
    (P, S, 12) fp32, valid (P, S) uint8, members (P, S, consensus_size) int32 padded with -1, support (P, S) int32); an
    unused slot or an invalid set has a pose of NaNs, no members and support 0."""
    what = 'consensus_poses'
    pairs = _ransac_corr_check(what, corr, c_offsets)
    _consensus_graph_check(what, bits, word_offsets, pairs)
    _dev(seeds)
    k1 = int(consensus_size)
    if seeds.dtype != torch.int32 or seeds.dim() != 2 or seeds.shape[0] != pairs or seeds.shape[1] < 1 or \
            not seeds.is_contiguous():
        raise TypeError('%s: contiguous (%d, S >= 1) int32 seeds expected' % (what, pairs))
    if not 3 <= k1 <= CONSENSUS_MAX_SIZE or not 0 <= int(n_words) <= int(bits.shape[0]):
        raise ValueError('%s: consensus_size in 3 .. %d and n_words within the bit matrices expected'
                         % (what, CONSENSUS_MAX_SIZE))
    n_seeds = int(seeds.shape[1])
    poses = torch.empty((pairs, n_seeds, 12), dtype=torch.float32, device=corr.device)
    valid = torch.empty((pairs, n_seeds), dtype=torch.uint8, device=corr.device)
    members = torch.empty((pairs, n_seeds, k1), dtype=torch.int32, device=corr.device)
    support = torch.empty((pairs, n_seeds), dtype=torch.int32, device=corr.device)
    check(_native.load().hfl_consensus_poses(poses.data_ptr(), valid.data_ptr(), members.data_ptr(), support.data_ptr(),
                                             seeds.data_ptr(), bits.data_ptr(), word_offsets.data_ptr(), int(n_words),
                                             _some(corr).data_ptr(), c_offsets.data_ptr(), int(corr.shape[0]), pairs, n_seeds,
                                             k1, _stream()), 'hfl_consensus_poses')
    return poses, valid, members, support


VOXEL_MAX_CLOUDS = 32767           # HFL_VOXEL_MAX_CLOUDS
VOXEL_MAX_CELLS = 65535                # HFL_VOXEL_MAX_CELLS: a cloud may span this many cells along an axis
VOXEL_MAX_POINTS = 2147483646          # HFL_VOXEL_MAX_POINTS


def voxel_keys(points: torch.Tensor, offsets: torch.Tensor, voxel_size: float):
    """`hfl_voxel_keys`: points (P, 3) fp32 and offsets (B + 1,) int64 on the GPU, every cloud non-empty and offsets[B] == P
    (the caller checks) -> (keys (P,) int64 = cloud << 48 | ix << 32 | iy << 16 | iz, flags (B,) int32: 1 where a cloud
    spans 65 536 or more cells along an axis)."""
    batch = _ragged_check('voxel_keys', points, offsets)
    n = int(points.shape[0])
    if n < batch:
        raise ValueError('voxel_keys: %d points for %d non-empty clouds' % (n, batch))
    keys = torch.empty(n, dtype=torch.int64, device=points.device)
    flags = torch.empty(batch, dtype=torch.int32, device=points.device)
    bounds = torch.empty((batch, 6), dtype=torch.int32, device=points.device)
    check(_native.load().hfl_voxel_keys(keys.data_ptr(), flags.data_ptr(), bounds.data_ptr(), points.data_ptr(),
                                        offsets.data_ptr(), batch, n, float(voxel_size), _stream()), 'hfl_voxel_keys')
    return keys, flags


def voxel_reduce(sorted_keys: torch.Tensor, perm: torch.Tensor, points: torch.Tensor, batch: int,
                 return_counts: bool = False, return_keys: bool = False):
    """`hfl_voxel_reduce`: the ascending keys of `voxel_keys`, the stable sort's permutation and the points -> (out (P, 3)
    fp32 whose first M rows are the cell means in key order, out_offsets (B + 1,) int64 on the GPU with cloud b at rows
    [out_offsets[b], out_offsets[b + 1]) and out_offsets[B] = M, cell_counts (P,) int32 or None, out_keys (P,) int64 or
    None).  Nothing is read back."""
    _dev(sorted_keys, perm, points)
    n = int(points.shape[0])
    for t in (sorted_keys, perm):
        _vector_check('voxel_reduce', t, torch.int64, n, 'keys and permutation')
    _points_check('voxel_reduce', points)
    lib = _native.load()
    nbytes = int(lib.hfl_voxel_reduce_workspace(n))
    if nbytes <= 0:
        raise ValueError('voxel_reduce: 1..%d points expected, got %d' % (VOXEL_MAX_POINTS, n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=points.device)
    out = torch.empty_like(points)
    out_off = torch.empty(int(batch) + 1, dtype=torch.int64, device=points.device)
    counts = torch.empty(n, dtype=torch.int32, device=points.device) if return_counts else None
    okeys = torch.empty(n, dtype=torch.int64, device=points.device) if return_keys else None
    check(lib.hfl_voxel_reduce(out.data_ptr(), out_off.data_ptr(), counts.data_ptr() if return_counts else None,
                               okeys.data_ptr() if return_keys else None, sorted_keys.data_ptr(), perm.data_ptr(),
                               points.data_ptr(), n, int(batch), ws.data_ptr(), nbytes, _stream()), 'hfl_voxel_reduce')
    return out, out_off, counts, okeys


def submap_normalise(points: torch.Tensor, offsets: torch.Tensor):
    """`hfl_submap_normalise`: points (P, 3) fp32 and offsets (B + 1,) int64 on the GPU (offsets[B] <= P) -> (out (P, 3) with
    cloud b's kept rows from row offsets[b] on, counts (B,) int32, flags (B,) int32: 1 where the mean radius is not > 0)."""
    batch = _ragged_check('submap_normalise', points, offsets)
    out = torch.empty_like(points)
    counts = torch.empty(batch, dtype=torch.int32, device=points.device)
    flags = torch.empty(batch, dtype=torch.int32, device=points.device)
    check(_native.load().hfl_submap_normalise(out.data_ptr(), counts.data_ptr(), flags.data_ptr(), points.data_ptr(),
                                              offsets.data_ptr(), batch, _stream()), 'hfl_submap_normalise')
    return out, counts, flags


def submap_normalise_rows(points: torch.Tensor, offsets: torch.Tensor, raw: torch.Tensor, raw_offsets: torch.Tensor,
                          row_index: torch.Tensor, row_offsets: torch.Tensor):
    """`hfl_submap_normalise_rows`: the centroid and scale of cloud b of `points` / `offsets` (as `submap_normalise` computes
    them) applied to raw rows raw_offsets[b] + row_index[j], j in [row_offsets[b], row_offsets[b + 1]) -> (rows (R, 3) fp32,
    keep (R,) int32: 1 where every |q'| <= 1).  All tensors on the GPU; the index and offset tensors int64."""
    batch = _ragged_check('submap_normalise_rows', points, offsets)
    if _ragged_check('submap_normalise_rows', raw, raw_offsets) != batch:
        raise ValueError('submap_normalise_rows: the raw batch and the downsampled batch differ in size')
    _dev(row_index, row_offsets)
    _vector_check('submap_normalise_rows', row_index, torch.int64, kind='row_index')
    _vector_check('submap_normalise_rows', row_offsets, torch.int64, batch + 1, 'row_offsets')
    rows = int(row_index.shape[0])
    out = torch.empty((rows, 3), dtype=torch.float32, device=points.device)
    keep = torch.empty(rows, dtype=torch.int32, device=points.device)
    if rows:
        check(_native.load().hfl_submap_normalise_rows(out.data_ptr(), keep.data_ptr(), points.data_ptr(), offsets.data_ptr(),
                                                       raw.data_ptr(), raw_offsets.data_ptr(), row_index.data_ptr(),
                                                       row_offsets.data_ptr(), batch, _stream()), 'hfl_submap_normalise_rows')
    return out, keep


def voxel_gather_rows(points: torch.Tensor, index: torch.Tensor):
    """`hfl_voxel_gather_rows`: points (P, 3) fp32 and index (R,) int64 on the GPU -> points[index] (R, 3); an index outside
    [0, P) gives a zero row."""
    _dev(points, index)
    _points_check('voxel_gather_rows', points)
    _vector_check('voxel_gather_rows', index, torch.int64, kind='index')
    out = torch.empty((int(index.shape[0]), 3), dtype=torch.float32, device=points.device)
    if index.shape[0]:
        check(_native.load().hfl_voxel_gather_rows(out.data_ptr(), points.data_ptr(), int(points.shape[0]), index.data_ptr(),
                                                   int(index.shape[0]), _stream()), 'hfl_voxel_gather_rows')
    return out


def voxel_bounds(points: torch.Tensor, offsets: torch.Tensor):
    """`hfl_voxel_bounds`: -> bounds (B, 6) int32 on the GPU, the ordered-integer images of every cloud's minimum and maximum
    that `voxel_occupancy` takes; `decode_voxel_bounds` turns a host copy into floats."""
    batch = _ragged_check('voxel_bounds', points, offsets)
    n = int(points.shape[0])
    if n < batch:
        raise ValueError('voxel_bounds: %d points for %d non-empty clouds' % (n, batch))
    bounds = torch.empty((batch, 6), dtype=torch.int32, device=points.device)
    check(_native.load().hfl_voxel_bounds(bounds.data_ptr(), points.data_ptr(), offsets.data_ptr(), batch, n, _stream()),
          'hfl_voxel_bounds')
    return bounds


def decode_voxel_bounds(bounds):
    """a host copy of `voxel_bounds` -> (B, 6) float32 numpy: min x, y, z, max x, y, z"""
    e = np.ascontiguousarray(bounds).view(np.uint32).reshape(-1, 6).copy()
    e[:, :3] = ~e[:, :3]
    return np.where(e & 0x80000000, e & 0x7FFFFFFF, ~e).astype(np.uint32).view(np.float32)


VOXEL_CANDIDATE_DTYPE = [('cloud', '<i4'), ('nx', '<i4'), ('ny', '<i4'), ('nz', '<i4'), ('voxel', '<f8'), ('word_offset', '<i8')]
VOXEL_OCC_MAX_CANDIDATES = 65535       # HFL_VOXEL_OCC_MAX_CANDIDATES
VOXEL_OCC_MAX_WORDS = 67108863         # HFL_VOXEL_OCC_MAX_WORDS


def voxel_occupancy(points: torch.Tensor, offsets: torch.Tensor, bounds: torch.Tensor, candidates, bitmap_words: int,
                    max_cloud_points: int):
    """`hfl_voxel_occupancy`: `candidates` is a host numpy array of `VOXEL_CANDIDATE_DTYPE` (hfl_voxel_candidate) whose
    bitmaps take `bitmap_words` words together -> counts (n_cand,) int32 on the GPU.  Nothing is read back."""
    batch = _ragged_check('voxel_occupancy', points, offsets)
    _dev(bounds)
    if bounds.dtype != torch.int32 or tuple(bounds.shape) != (batch, 6) or not bounds.is_contiguous():
        raise TypeError('voxel_occupancy: (B, 6) int32 bounds expected')
    table = np.ascontiguousarray(candidates, dtype=np.dtype(VOXEL_CANDIDATE_DTYPE))
    n_cand = int(table.shape[0])
    lib = _native.load()
    nbytes = int(lib.hfl_voxel_occupancy_workspace(n_cand, int(bitmap_words)))
    if table.ndim != 1 or nbytes <= 0:
        raise ValueError('voxel_occupancy: 1..%d candidates and 1..%d bitmap words expected, got %d and %d'
                         % (VOXEL_OCC_MAX_CANDIDATES, VOXEL_OCC_MAX_WORDS, n_cand, bitmap_words))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=points.device)
    counts = torch.empty(n_cand, dtype=torch.int32, device=points.device)
    check(lib.hfl_voxel_occupancy(counts.data_ptr(), table.ctypes.data, n_cand, int(bitmap_words), bounds.data_ptr(),
                                  points.data_ptr(), offsets.data_ptr(), batch, int(points.shape[0]), int(max_cloud_points),
                                  ws.data_ptr(), nbytes, _stream()), 'hfl_voxel_occupancy')
    counts._hfl_candidates = table      # the host table outlives the asynchronous copy: it goes when the counts go
    return counts


CLOTH_MAX_PARTICLES = 10240            # HFL_CLOTH_MAX_PARTICLES: width * height of one cloth
CLOTH_DESC_DTYPE = [('ox', '<f4'), ('oy', '<f4'), ('u0', '<f4'), ('width', '<i4'), ('height', '<i4'), ('reserved', '<i4'),
                    ('cell_offset', '<i8')]                                          # hfl_cloth_desc


class _DescTable:
    """One descriptor per cloud on both sides: `host` (a numpy array of the subclass's `DTYPE`, what the library checks
    before a launch) and `device` (the same bytes, what the kernels read); `batch` clouds and `cells` cells in all, as the
    subclass counts and bounds them (`_checked_cells`)."""
    DTYPE = STRUCT = None

    def __init__(self, descs, device):
        self.host = np.ascontiguousarray(descs, dtype=np.dtype(self.DTYPE))
        if self.host.ndim != 1 or self.host.shape[0] < 1:
            raise ValueError('%s: one %s per cloud expected' % (type(self).__name__, self.STRUCT))
        self.batch = int(self.host.shape[0])
        self.cells = self._checked_cells(self.host)
        self.device = torch.from_numpy(self.host.view(np.uint8).copy()).to(device)


class ClothTable(_DescTable):
    """`hfl_cloth_desc` per cloud; `cells` particles in all, cloud b's at `host['cell_offset'][b]`."""
    DTYPE, STRUCT = CLOTH_DESC_DTYPE, 'hfl_cloth_desc'

    @staticmethod
    def _checked_cells(h):
        return int((h['width'].astype(np.int64) * h['height']).sum())


def _cloth_check(what: str, table: ClothTable, points=None, offsets=None):
    _dev(table.device)
    if points is not None and _ragged_check(what, points, offsets) != table.batch:
        raise ValueError('%s: %d clouds but %d cloths' % (what, int(offsets.shape[0]) - 1, table.batch))
    if table.cells < 1:
        raise ValueError('%s: the cloths hold no particle' % what)


def cloth_raster(points: torch.Tensor, offsets: torch.Tensor, table: ClothTable, resolution: float):
    """`hfl_cloth_raster`: points (P, 3) fp32 and offsets (B + 1,) int64 on the GPU -> terrain (cells,) fp32: every particle's
    t, rastered or filled.  Nothing is read back."""
    _cloth_check('cloth_raster', table, points, offsets)
    terrain = torch.empty(table.cells, dtype=torch.float32, device=points.device)
    keys = torch.empty(table.cells, dtype=torch.int64, device=points.device)
    check(_native.load().hfl_cloth_raster(terrain.data_ptr(), keys.data_ptr(), table.host.ctypes.data, table.device.data_ptr(),
                                          table.batch, table.cells, points.data_ptr(), offsets.data_ptr(),
                                          int(points.shape[0]), float(resolution), _stream()), 'hfl_cloth_raster')
    return terrain


def cloth_simulate(terrain: torch.Tensor, table: ClothTable, f_one: float, f_two: float, gravity_step: float,
                   velocity_keep: float, iterations: int, slope_smooth: bool):
    """`hfl_cloth_simulate`: terrain (cells,) fp32 -> (heights (cells,) fp32, movable (cells,) uint8, steps_run (B,) int32),
    one workgroup per cloud.  The four factors are passed as the fp32 values the host route uses."""
    _cloth_check('cloth_simulate', table)
    _dev(terrain)
    _vector_check('cloth_simulate', terrain, torch.float32, table.cells, 'terrain')
    heights = torch.empty_like(terrain)
    movable = torch.empty(table.cells, dtype=torch.uint8, device=terrain.device)
    steps = torch.empty(table.batch, dtype=torch.int32, device=terrain.device)
    check(_native.load().hfl_cloth_simulate(heights.data_ptr(), movable.data_ptr(), steps.data_ptr(), terrain.data_ptr(),
                                            table.host.ctypes.data, table.device.data_ptr(), table.batch, table.cells,
                                            float(f_one), float(f_two), float(gravity_step), float(velocity_keep),
                                            int(iterations), int(bool(slope_smooth)), _stream()), 'hfl_cloth_simulate')
    return heights, movable, steps


def cloth_classify(points: torch.Tensor, offsets: torch.Tensor, heights: torch.Tensor, table: ClothTable, resolution: float,
                   threshold: float):
    """`hfl_cloth_classify`: -> keep (P,) uint8 on the GPU, 0 where a point lies within `threshold` of the cloth (ground)."""
    _cloth_check('cloth_classify', table, points, offsets)
    _dev(heights)
    _vector_check('cloth_classify', heights, torch.float32, table.cells, 'heights')
    keep = torch.empty(int(points.shape[0]), dtype=torch.uint8, device=points.device)
    check(_native.load().hfl_cloth_classify(keep.data_ptr(), heights.data_ptr(), table.host.ctypes.data,
                                            table.device.data_ptr(), table.batch, table.cells, points.data_ptr(),
                                            offsets.data_ptr(), int(points.shape[0]), float(resolution), float(threshold),
                                            _stream()), 'hfl_cloth_classify')
    return keep


KNN_MAX_NEIGHBOURS = 32                # HFL_KNN_MAX_NEIGHBOURS
KNN_MAX_CELLS = 268435455              # HFL_KNN_MAX_CELLS: cells of all grids of one call
KNN_PHASE_STARTS, KNN_PHASE_QUERY, KNN_PHASE_FALLBACK, KNN_PHASE_ALL = 1, 2, 4, 7      # HFL_KNN_PHASE_*
KNN_GRID_DTYPE = [('ox', '<f4'), ('oy', '<f4'), ('oz', '<f4'), ('cell', '<f4'), ('mx', '<f4'), ('my', '<f4'), ('mz', '<f4'),
                  ('k', '<i4'), ('nx', '<i4'), ('ny', '<i4'), ('nz', '<i4'), ('reserved', '<i4'),
                  ('cell_base', '<i8')]                                              # hfl_knn_grid


class KnnGridTable(_DescTable):
    """`hfl_knn_grid` per cloud; `cells` cells in all (1..KNN_MAX_CELLS), cloud b's from `host['cell_base'][b]` on."""
    DTYPE, STRUCT = KNN_GRID_DTYPE, 'hfl_knn_grid'

    @staticmethod
    def _checked_cells(h):
        cells = int((h['nx'].astype(np.int64) * h['ny'] * h['nz']).sum())
        if cells < 1 or cells > KNN_MAX_CELLS:
            raise ValueError('KnnGridTable: 1..%d cells expected, got %d' % (KNN_MAX_CELLS, cells))
        return cells


def cloud_nonfinite(points: torch.Tensor, offsets: torch.Tensor):
    """`hfl_cloud_nonfinite`: -> flags (B,) int32 on the GPU, 1 where a cloud holds a coordinate that is not finite."""
    batch = _ragged_check('cloud_nonfinite', points, offsets)
    flags = torch.empty(batch, dtype=torch.int32, device=points.device)
    check(_native.load().hfl_cloud_nonfinite(flags.data_ptr(), points.data_ptr(), offsets.data_ptr(), batch,
                                             int(points.shape[0]), _stream()), 'hfl_cloud_nonfinite')
    return flags


def _knn_check(what: str, table: KnnGridTable, points: torch.Tensor, offsets: torch.Tensor):
    _dev(table.device)
    if _ragged_check(what, points, offsets) != table.batch:
        raise ValueError('%s: %d clouds but %d grids' % (what, int(offsets.shape[0]) - 1, table.batch))


def knn_cell_keys(points: torch.Tensor, offsets: torch.Tensor, table: KnnGridTable):
    """`hfl_knn_cell_keys`: points (P, 3) fp32 and offsets (B + 1,) int64 on the GPU -> keys (P,) int64, every point's cell
    on its cloud's grid, counted through the batch.  Nothing is read back."""
    _knn_check('knn_cell_keys', table, points, offsets)
    keys = torch.empty(int(points.shape[0]), dtype=torch.int64, device=points.device)
    check(_native.load().hfl_knn_cell_keys(keys.data_ptr(), table.host.ctypes.data, table.device.data_ptr(), table.batch,
                                           table.cells, points.data_ptr(), offsets.data_ptr(), int(points.shape[0]),
                                           _stream()), 'hfl_knn_cell_keys')
    return keys


class KnnWorkspace:
    """what `hfl_knn_mean_dist` keeps between its launches: the cell-start table, the list of pending points, its counter"""

    def __init__(self, n_points: int, cells: int, device):
        self.starts = torch.empty(cells + 1, dtype=torch.int32, device=device)
        self.pending = torch.empty(n_points, dtype=torch.int32, device=device)
        self.counter = torch.zeros(1, dtype=torch.int32, device=device)


def _knn_sorted_check(what: str, table: KnnGridTable, sorted_points: torch.Tensor, offsets: torch.Tensor,
                      workspace: KnnWorkspace, label: str, *vectors):
    """What every call on a sorted batch checks before it launches: `_knn_check`, the (P,) int64 `vectors` (`label` names
    them in the message), and a workspace made for this batch (a fresh one for None).  -> (P, the workspace)"""
    _knn_check(what, table, sorted_points, offsets)
    _dev(*vectors)
    n = int(sorted_points.shape[0])
    for t in vectors:
        _vector_check(what, t, torch.int64, n, label)
    ws = workspace if workspace is not None else KnnWorkspace(n, table.cells, sorted_points.device)
    if tuple(ws.starts.shape) != (table.cells + 1,) or tuple(ws.pending.shape) != (n,):
        raise ValueError('%s: the workspace was made for another batch' % what)
    _dev(ws.starts, ws.pending, ws.counter)
    return n, ws


def knn_mean_dist(sorted_points: torch.Tensor, sorted_keys: torch.Tensor, perm: torch.Tensor, offsets: torch.Tensor,
                  table: KnnGridTable, phases: int = KNN_PHASE_ALL, workspace: KnnWorkspace = None, out: torch.Tensor = None):
    """`hfl_knn_mean_dist`: the ascending keys of `knn_cell_keys`, the sort's permutation and `points[perm]` -> (avg (P,)
    fp32 in INPUT order: the mean distance to the k nearest points of the own cloud, pending (1,) int32 on the GPU: how many
    points the whole-cloud scan had to finish).  `phases` runs single launches on a `workspace` and an `out` kept from an
    earlier call.  Nothing is read back."""
    n, ws = _knn_sorted_check('knn_mean_dist', table, sorted_points, offsets, workspace, 'keys and permutation', sorted_keys,
                              perm)
    avg = out if out is not None else torch.empty(n, dtype=torch.float32, device=sorted_points.device)
    _vector_check('knn_mean_dist', avg, torch.float32, n, 'output')
    _dev(avg)
    check(_native.load().hfl_knn_mean_dist(avg.data_ptr(), ws.pending.data_ptr(), ws.counter.data_ptr(), ws.starts.data_ptr(),
                                           sorted_points.data_ptr(), sorted_keys.data_ptr(), perm.data_ptr(),
                                           table.host.ctypes.data, table.device.data_ptr(), table.batch, table.cells,
                                           offsets.data_ptr(), n, int(phases), _stream()), 'hfl_knn_mean_dist')
    return avg, ws.counter


def _radius2(what: str, radius2) -> float:
    """R2 of a radius or hybrid search as the float the C-ABI takes: a squared distance or +inf, as fp32 holds it"""
    r2 = float(np.float32(radius2))
    if not r2 >= 0.0:
        raise ValueError('%s: radius2 must be a squared distance >= 0 (+inf allowed), got %r' % (what, radius2))
    return r2


def knn_normals(sorted_points: torch.Tensor, sorted_keys: torch.Tensor, perm: torch.Tensor, offsets: torch.Tensor,
                table: KnnGridTable, viewpoints: torch.Tensor = None, phases: int = KNN_PHASE_ALL,
                workspace: KnnWorkspace = None, radius2=None, radius_only: bool = False):
    """`hfl_knn_normals`: the arguments of `knn_mean_dist` -> (normals (P, 3) fp32, curvature (P,) fp32, counts (P,) int32,
    all in INPUT order, pending (1,) int32 on the GPU).  `viewpoints`: (B, 3) float64 on the GPU, one per cloud, or None for
    the upward rule.  With `radius2` (R2 as fp32 holds it) `hfl_knn_normals_radius`: r2 = min(k-th smallest, R2), or, with
    `radius_only`, r2 = R2 and the table's k unread.  Nothing is read back."""
    if radius_only and radius2 is None:
        raise ValueError('knn_normals: radius_only needs radius2')
    n, ws = _knn_sorted_check('knn_normals', table, sorted_points, offsets, workspace, 'keys and permutation', sorted_keys,
                              perm)
    if viewpoints is not None:
        _dev(viewpoints)
        if viewpoints.dtype != torch.float64 or tuple(viewpoints.shape) != (table.batch, 3) or not viewpoints.is_contiguous():
            raise TypeError('knn_normals: contiguous (%d, 3) float64 viewpoints expected' % table.batch)
    normals = torch.empty((n, 3), dtype=torch.float32, device=sorted_points.device)
    curvature = torch.empty(n, dtype=torch.float32, device=sorted_points.device)
    counts = torch.empty(n, dtype=torch.int32, device=sorted_points.device)
    args = (normals.data_ptr(), curvature.data_ptr(), counts.data_ptr(), ws.pending.data_ptr(), ws.counter.data_ptr(),
            ws.starts.data_ptr(), sorted_points.data_ptr(), sorted_keys.data_ptr(), perm.data_ptr(), table.host.ctypes.data,
            table.device.data_ptr(), table.batch, table.cells, offsets.data_ptr(), n,
            viewpoints.data_ptr() if viewpoints is not None else None)
    if radius2 is None:
        check(_native.load().hfl_knn_normals(*args, int(phases), _stream()), 'hfl_knn_normals')
    else:
        check(_native.load().hfl_knn_normals_radius(*args, _radius2('knn_normals', radius2), int(bool(radius_only)),
                                                    int(phases), _stream()), 'hfl_knn_normals_radius')
    return normals, curvature, counts, ws.counter


def knn_radius_count(sorted_points: torch.Tensor, sorted_keys: torch.Tensor, perm: torch.Tensor, offsets: torch.Tensor,
                     table: KnnGridTable, radius2, phases: int = KNN_PHASE_ALL, workspace: KnnWorkspace = None):
    """`hfl_knn_radius_count`: the arguments of `knn_mean_dist` and R2 -> (counts (P,) int32 in INPUT order: the points of
    the own cloud with d2 <= R2, the point itself included; pending (1,) int32 on the GPU).  Nothing is read back."""
    n, ws = _knn_sorted_check('knn_radius_count', table, sorted_points, offsets, workspace, 'keys and permutation',
                              sorted_keys, perm)
    counts = torch.empty(n, dtype=torch.int32, device=sorted_points.device)
    check(_native.load().hfl_knn_radius_count(counts.data_ptr(), ws.pending.data_ptr(), ws.counter.data_ptr(),
                                              ws.starts.data_ptr(), sorted_points.data_ptr(), sorted_keys.data_ptr(),
                                              perm.data_ptr(), table.host.ctypes.data, table.device.data_ptr(), table.batch,
                                              table.cells, offsets.data_ptr(), n, _radius2('knn_radius_count', radius2),
                                              int(phases), _stream()), 'hfl_knn_radius_count')
    return counts, ws.counter


def iss_saliency(sorted_points: torch.Tensor, sorted_keys: torch.Tensor, perm: torch.Tensor, offsets: torch.Tensor,
                 table: KnnGridTable, radius2, gamma_21: float, gamma_32: float, min_neighbors: int,
                 phases: int = KNN_PHASE_ALL, workspace: KnnWorkspace = None):
    """`hfl_iss_saliency`: the arguments of `knn_mean_dist`, R2 of the salient radius and the three thresholds -> (saliency
    (P,) fp32 and counts (P,) int32 in INPUT order, the same saliency by SORTED position for `iss_select`, pending (1,)
    int32 on the GPU).  Nothing is read back."""
    n, ws = _knn_sorted_check('iss_saliency', table, sorted_points, offsets, workspace, 'keys and permutation', sorted_keys,
                              perm)
    saliency, sorted_saliency = (torch.empty(n, dtype=torch.float32, device=sorted_points.device) for _ in range(2))
    counts = torch.empty(n, dtype=torch.int32, device=sorted_points.device)
    check(_native.load().hfl_iss_saliency(saliency.data_ptr(), sorted_saliency.data_ptr(), counts.data_ptr(),
                                          ws.pending.data_ptr(), ws.counter.data_ptr(), ws.starts.data_ptr(),
                                          sorted_points.data_ptr(), sorted_keys.data_ptr(), perm.data_ptr(),
                                          table.host.ctypes.data, table.device.data_ptr(), table.batch, table.cells,
                                          offsets.data_ptr(), n, _radius2('iss_saliency', radius2), float(gamma_21),
                                          float(gamma_32), int(min_neighbors), int(phases), _stream()), 'hfl_iss_saliency')
    return saliency, counts, sorted_saliency, ws.counter


def iss_select(sorted_points: torch.Tensor, sorted_keys: torch.Tensor, perm: torch.Tensor, sorted_saliency: torch.Tensor,
               offsets: torch.Tensor, table: KnnGridTable, radius2, min_neighbors: int, phases: int = KNN_PHASE_ALL,
               workspace: KnnWorkspace = None):
    """`hfl_iss_select`: the arguments of `knn_mean_dist`, the (P,) fp32 saliency by SORTED position (`saliency[perm]`), R2
    of the non-maximum radius -> (mask (P,) uint8 in INPUT order, pending (1,) int32 on the GPU).  A `workspace` that an
    earlier call on this batch filled spares the cell-start table (`phases` without `KNN_PHASE_STARTS`).  Nothing is read
    back."""
    n, ws = _knn_sorted_check('iss_select', table, sorted_points, offsets, workspace, 'keys and permutation', sorted_keys, perm)
    _dev(sorted_saliency)
    _vector_check('iss_select', sorted_saliency, torch.float32, n, 'saliency')
    mask = torch.empty(n, dtype=torch.uint8, device=sorted_points.device)
    check(_native.load().hfl_iss_select(mask.data_ptr(), ws.pending.data_ptr(), ws.counter.data_ptr(), ws.starts.data_ptr(),
                                        sorted_points.data_ptr(), sorted_keys.data_ptr(), perm.data_ptr(),
                                        sorted_saliency.data_ptr(), table.host.ctypes.data, table.device.data_ptr(),
                                        table.batch, table.cells, offsets.data_ptr(), n, _radius2('iss_select', radius2),
                                        int(min_neighbors), int(phases), _stream()), 'hfl_iss_select')
    return mask, ws.counter


def count_mask(counts: torch.Tensor, nb_points: int):
    """`hfl_count_mask`: counts (P,) int32 on the GPU -> keep (P,) uint8, 1 where counts > nb_points."""
    _dev(counts)
    n = int(counts.shape[0])
    _vector_check('count_mask', counts, torch.int32, n, 'counts')
    keep = torch.empty(n, dtype=torch.uint8, device=counts.device)
    check(_native.load().hfl_count_mask(keep.data_ptr(), counts.data_ptr(), n, int(nb_points), _stream()), 'hfl_count_mask')
    return keep


FPFH_DIM = 33                          # three groups of 11 bins
FEATURE_ROWS = OVERLAP_ROWS            # HFL_FEATURE_ROWS: query rows of a workgroup of hfl_feature_nn, as `feature_tiles` needs
FEATURE_MAX_DIM = 64                   # HFL_FEATURE_MAX_DIM


class FpfhWorkspace(KnnWorkspace):
    """what the three hfl_fpfh_* calls hand to each other, all by SORTED position: the workspace of the search, every
    point's r2 and whether the 3 x 3 x 3 block proves it, the integer histograms and the pair counts"""

    def __init__(self, n_points: int, cells: int, device):
        super().__init__(n_points, cells, device)
        self.r2 = torch.empty(n_points, dtype=torch.float32, device=device)
        self.proven = torch.empty(n_points, dtype=torch.uint8, device=device)
        self.hist = torch.empty((n_points, FPFH_DIM), dtype=torch.int32, device=device)
        self.pairs = torch.empty(n_points, dtype=torch.int32, device=device)


def _fpfh_check(what: str, ws: FpfhWorkspace, table: KnnGridTable, sorted_points: torch.Tensor, offsets: torch.Tensor,
                sorted_keys: torch.Tensor) -> int:
    n, _ = _knn_sorted_check(what, table, sorted_points, offsets, ws, 'keys', sorted_keys)
    _dev(ws.r2, ws.proven, ws.hist, ws.pairs)
    return n


def fpfh_radius(ws: FpfhWorkspace, sorted_points: torch.Tensor, sorted_keys: torch.Tensor, offsets: torch.Tensor,
                table: KnnGridTable, radius2=None, radius_only: bool = False):
    """`hfl_fpfh_radius`: the sorted batch of `knn_mean_dist` -> ws.r2, ws.proven and the pending list filled; returns the
    (1,) int32 counter of points the whole-cloud scan finished.  With `radius2` (R2 as fp32 holds it)
    `hfl_fpfh_radius_capped`: r2 = min(k-th smallest, R2), or, with `radius_only`, r2 = R2 and no scan.  Nothing is read
    back."""
    if radius_only and radius2 is None:
        raise ValueError('fpfh_radius: radius_only needs radius2')
    n = _fpfh_check('fpfh_radius', ws, table, sorted_points, offsets, sorted_keys)
    args = (ws.r2.data_ptr(), ws.proven.data_ptr(), ws.pending.data_ptr(), ws.counter.data_ptr(), ws.starts.data_ptr(),
            sorted_points.data_ptr(), sorted_keys.data_ptr(), table.host.ctypes.data, table.device.data_ptr(), table.batch,
            table.cells, offsets.data_ptr(), n)
    if radius2 is None:
        check(_native.load().hfl_fpfh_radius(*args, _stream()), 'hfl_fpfh_radius')
    else:
        check(_native.load().hfl_fpfh_radius_capped(*args, _radius2('fpfh_radius', radius2), int(bool(radius_only)),
                                                    _stream()), 'hfl_fpfh_radius_capped')
    return ws.counter


def fpfh_spfh(ws: FpfhWorkspace, sorted_points: torch.Tensor, sorted_normals: torch.Tensor, sorted_keys: torch.Tensor,
              offsets: torch.Tensor, table: KnnGridTable, theta_table: np.ndarray):
    """`hfl_fpfh_spfh` after `fpfh_radius` on the same workspace: sorted_normals (P, 3) fp32 = normals[perm] and the (10, 2)
    float64 numpy table of (cos e_k, sin e_k) -> (ws.hist (P, 33) int32, ws.pairs (P,) int32), by SORTED position."""
    n = _fpfh_check('fpfh_spfh', ws, table, sorted_points, offsets, sorted_keys)
    _dev(sorted_normals)
    _points_check('fpfh_spfh', sorted_normals)
    if int(sorted_normals.shape[0]) != n:
        raise TypeError('fpfh_spfh: %d normals for %d points' % (int(sorted_normals.shape[0]), n))
    if not isinstance(theta_table, np.ndarray) or theta_table.dtype != np.float64 or theta_table.shape != (10, 2) or \
            not theta_table.flags['C_CONTIGUOUS']:
        raise TypeError('fpfh_spfh: contiguous (10, 2) float64 numpy table of the theta edges expected')
    check(_native.load().hfl_fpfh_spfh(ws.hist.data_ptr(), ws.pairs.data_ptr(), ws.r2.data_ptr(), ws.proven.data_ptr(),
                                       ws.pending.data_ptr(), ws.counter.data_ptr(), ws.starts.data_ptr(),
                                       sorted_points.data_ptr(), sorted_normals.data_ptr(), sorted_keys.data_ptr(),
                                       table.host.ctypes.data, table.device.data_ptr(), table.batch, table.cells,
                                       offsets.data_ptr(), n, theta_table.ctypes.data, _stream()), 'hfl_fpfh_spfh')
    return ws.hist, ws.pairs


def fpfh_combine(ws: FpfhWorkspace, sorted_points: torch.Tensor, sorted_keys: torch.Tensor, perm: torch.Tensor,
                 offsets: torch.Tensor, table: KnnGridTable, out: torch.Tensor = None):
    """`hfl_fpfh_combine` after `fpfh_spfh` on the same workspace -> fpfh (P, 33) fp32 in INPUT order."""
    n = _fpfh_check('fpfh_combine', ws, table, sorted_points, offsets, sorted_keys)
    _dev(perm)
    _vector_check('fpfh_combine', perm, torch.int64, n, 'permutation')
    fpfh = out if out is not None else torch.empty((n, FPFH_DIM), dtype=torch.float32, device=sorted_points.device)
    _dev(fpfh)
    if fpfh.dtype != torch.float32 or tuple(fpfh.shape) != (n, FPFH_DIM) or not fpfh.is_contiguous():
        raise TypeError('fpfh_combine: contiguous (%d, %d) float32 output expected' % (n, FPFH_DIM))
    check(_native.load().hfl_fpfh_combine(fpfh.data_ptr(), ws.hist.data_ptr(), ws.pairs.data_ptr(), ws.r2.data_ptr(),
                                          ws.proven.data_ptr(), ws.pending.data_ptr(), ws.counter.data_ptr(),
                                          ws.starts.data_ptr(), sorted_points.data_ptr(), sorted_keys.data_ptr(),
                                          perm.data_ptr(), table.host.ctypes.data, table.device.data_ptr(), table.batch,
                                          table.cells, offsets.data_ptr(), n, _stream()), 'hfl_fpfh_combine')
    return fpfh


# the tile table of `hfl_feature_nn` from the query lengths of the pairs on the host; right while FEATURE_ROWS is OVERLAP_ROWS,
# which csrc/pair_scan.h asserts of the header's two defines
feature_tiles = overlap_tiles


def _feature_rows_check(what: str, rows: torch.Tensor):
    if rows.dtype != torch.float32 or rows.dim() != 2 or not rows.is_contiguous():
        raise TypeError('%s: contiguous (N, D) float32 rows expected' % what)


def feature_nn(queries: torch.Tensor, q_offsets: torch.Tensor, targets: torch.Tensor, t_offsets: torch.Tensor,
               tiles: torch.Tensor):
    """`hfl_feature_nn`: two ragged batches of (N, D) fp32 feature rows of the same P pairs, 1 <= D <= FEATURE_MAX_DIM, and
    the (n_tiles, 2) int64 device copy of `feature_tiles` -> (dist2 (Nq,) fp32, idx (Nq,) int32): every query row's smallest
    squared distance to a target row of its pair and that row's index within the pair, +inf and -1 where the pair has no
    target.  Rows the table does not cover stay unwritten."""
    pairs = _pair_batch_check('feature_nn', queries, q_offsets, targets, t_offsets, tiles, rows_check=_feature_rows_check)
    dim = int(queries.shape[1])
    if int(targets.shape[1]) != dim or not 1 <= dim <= FEATURE_MAX_DIM:
        raise ValueError('feature_nn: both sides need the same D in 1..%d, got %d and %d'
                         % (FEATURE_MAX_DIM, dim, int(targets.shape[1])))
    n_q = int(queries.shape[0])
    dist2 = torch.empty(n_q, dtype=torch.float32, device=queries.device)
    idx = torch.empty(n_q, dtype=torch.int32, device=queries.device)
    if n_q and tiles.shape[0]:
        check(_native.load().hfl_feature_nn(dist2.data_ptr(), idx.data_ptr(), queries.data_ptr(), q_offsets.data_ptr(), n_q,
                                            _some(targets).data_ptr(), t_offsets.data_ptr(), int(targets.shape[0]), dim,
                                            tiles.data_ptr(), int(tiles.shape[0]), pairs, _stream()), 'hfl_feature_nn')
    return dist2, idx


def outlier_threshold(avg: torch.Tensor, offsets: torch.Tensor, std_ratio: float):
    """`hfl_outlier_threshold`: avg (P,) fp32 and offsets (B + 1,) int64 on the GPU -> stats (B, 4) float64: mean, std,
    mean + std_ratio std and the number of valid rows (avg > 0) of every cloud."""
    _dev(avg, offsets)
    _vector_check('outlier_threshold', avg, torch.float32, kind='distances')
    _offsets_check('outlier_threshold', offsets)
    batch = int(offsets.shape[0]) - 1
    stats = torch.empty((batch, 4), dtype=torch.float64, device=avg.device)
    check(_native.load().hfl_outlier_threshold(stats.data_ptr(), _some(avg).data_ptr(), offsets.data_ptr(), batch,
                                               int(avg.shape[0]), float(std_ratio), _stream()), 'hfl_outlier_threshold')
    return stats


def outlier_mask(avg: torch.Tensor, offsets: torch.Tensor, stats: torch.Tensor):
    """`hfl_outlier_mask`: -> keep (P,) uint8 on the GPU, 1 where avg > 0 and below the cloud's threshold (stats[:, 2])."""
    _dev(avg, offsets, stats)
    _vector_check('outlier_mask', avg, torch.float32, kind='distances')
    if avg.shape[0] < 1:
        raise TypeError('outlier_mask: non-empty distances expected')
    _offsets_check('outlier_mask', offsets)
    batch = int(offsets.shape[0]) - 1
    if stats.dtype != torch.float64 or tuple(stats.shape) != (batch, 4) or not stats.is_contiguous():
        raise TypeError('outlier_mask: contiguous (%d, 4) float64 stats expected' % batch)
    keep = torch.empty(int(avg.shape[0]), dtype=torch.uint8, device=avg.device)
    check(_native.load().hfl_outlier_mask(keep.data_ptr(), avg.data_ptr(), stats.data_ptr(), offsets.data_ptr(), batch,
                                          int(avg.shape[0]), _stream()), 'hfl_outlier_mask')
    return keep


def radius_mask(points: torch.Tensor, radius_max: float):
    """`hfl_radius_mask`: points (P, 3) fp32 on the GPU, P >= 1 -> keep (P,) uint8, 1 where sqrt(x x + y y) <= radius_max in
    float64."""
    _dev(points)
    _points_check('radius_mask', points)
    keep = torch.empty(int(points.shape[0]), dtype=torch.uint8, device=points.device)
    check(_native.load().hfl_radius_mask(keep.data_ptr(), points.data_ptr(), int(points.shape[0]), float(radius_max),
                                         _stream()), 'hfl_radius_mask')
    return keep


def _flat_l2_check(what: str, x: torch.Tensor):
    if x.dim() != 2:
        raise ValueError('%s: a (rows, D) matrix expected, got %s' % (what, tuple(x.shape)))
    d = x.shape[1]
    if d % 4 != 0 or d < 4 or d > 1024:
        raise ValueError('%s: D must be a multiple of 4 in 4..1024, got %d' % (what, d))


def row_sq_norms(x: torch.Tensor):
    """Squared L2 norm of every row of x (n, D) fp32, one fmaf chain per row (`hfl_row_sq_norms`)."""
    _dev(x)
    _flat_l2_check('row_sq_norms', x)
    x = _f32c(x)
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    if x.shape[0] > 0:
        check(_native.load().hfl_row_sq_norms(out.data_ptr(), x.data_ptr(), x.shape[0], x.shape[1], _stream()), 'hfl_row_sq_norms')
    return out


def _flat_l2_operands(name: str, queries, database, k, database_sq_norms):
    """The argument rules both searches share -> (queries, database, database_sq_norms, k) ready for the library."""
    _dev(queries, database, database_sq_norms)
    _flat_l2_check(name + ' queries', queries)
    _flat_l2_check(name + ' database', database)
    if queries.shape[1] != database.shape[1]:
        raise ValueError('%s: queries have D = %d, the database D = %d' % (name, queries.shape[1], database.shape[1]))
    k = int(k)
    if k < 1 or k > 32:
        raise ValueError('%s: 1 <= k <= 32 expected, got %d' % (name, k))
    n_rows = database.shape[0]
    if n_rows < 1:
        raise ValueError('%s: the database is empty' % name)
    queries, database = _f32c(queries), _f32c(database)
    if database_sq_norms is not None:
        database_sq_norms = _f32c(database_sq_norms)
        if tuple(database_sq_norms.shape) != (n_rows,):
            raise ValueError('%s: %d database norms expected, got %s' % (name, n_rows, tuple(database_sq_norms.shape)))
    return queries, database, database_sq_norms, k


def _flat_l2_workspace(name: str, lib, q_rows, n_rows, d, k, device):
    ws_bytes = lib.hfl_flat_l2_topk_workspace(q_rows, n_rows, d, k)
    if ws_bytes < 0:
        raise ValueError('%s: unsupported shape Q = %d, N = %d, D = %d, k = %d' % (name, q_rows, n_rows, d, k))
    return torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=device), ws_bytes


def flat_l2_topk(queries: torch.Tensor, database: torch.Tensor, k: int, database_sq_norms: torch.Tensor = None):
    """The min(k, N) nearest database rows of every query by squared L2 distance, nearest first, equal distances by lower
    index, without a (Q, N) matrix (`hfl_flat_l2_topk`).  queries (Q, D), database (N, D) fp32, D a multiple of 4 in 4..1024,
    1 <= k <= 32; database_sq_norms: `row_sq_norms(database)` to reuse it.  Returns (dist (Q, kc) fp32, idx (Q, kc) int32)."""
    queries, database, database_sq_norms, k = _flat_l2_operands('flat_l2_topk', queries, database, k, database_sq_norms)
    q_rows, n_rows, d = queries.shape[0], database.shape[0], queries.shape[1]
    kc = min(k, n_rows)
    dist = torch.empty((q_rows, kc), dtype=torch.float32, device=queries.device)
    idx = torch.empty((q_rows, kc), dtype=torch.int32, device=queries.device)
    if q_rows == 0:
        return dist, idx
    lib = _native.load()
    ws, ws_bytes = _flat_l2_workspace('flat_l2_topk', lib, q_rows, n_rows, d, k, queries.device)
    check(lib.hfl_flat_l2_topk(dist.data_ptr(), idx.data_ptr(), queries.data_ptr(), database.data_ptr(),
                               None if database_sq_norms is None else database_sq_norms.data_ptr(), q_rows, n_rows, d, k,
                               ws.data_ptr(), ws_bytes, _stream()), 'hfl_flat_l2_topk')
    return dist, idx


def flat_l2_topk_prefix(queries: torch.Tensor, database: torch.Tensor, limits, k: int,
                        database_sq_norms: torch.Tensor = None):
    """`flat_l2_topk` with a prefix per query (`hfl_flat_l2_topk_prefix`): query q sees database rows [0, limits[q]) only.
    `limits`: (Q,) integers, a tensor on either device or a numpy array, every value in [0, N], else ValueError (one host
    read).  Returns (dist (Q, k) fp32, idx (Q, k) int32) whatever N: row q holds what `flat_l2_topk(queries[q:q + 1],
    database[:limits[q]], k)` returns, bit for bit, then distance +inf and index -1 in the slots past min(k, limits[q])."""
    name = 'flat_l2_topk_prefix'
    queries, database, database_sq_norms, k = _flat_l2_operands(name, queries, database, k, database_sq_norms)
    q_rows, n_rows, d = queries.shape[0], database.shape[0], queries.shape[1]
    if not isinstance(limits, torch.Tensor):
        limits = np.asarray(limits)
        if limits.dtype.kind not in 'iu':
            raise ValueError('%s: integer limits expected, got %s' % (name, limits.dtype))
        limits = torch.from_numpy(np.ascontiguousarray(limits, dtype=np.int64))
    if limits.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
        raise ValueError('%s: integer limits expected, got %s' % (name, limits.dtype))
    if tuple(limits.shape) != (q_rows,):
        raise ValueError('%s: (%d,) limits expected, one per query, got %s' % (name, q_rows, tuple(limits.shape)))
    limits = limits.to(queries.device)
    if q_rows > 0 and bool(((limits < 0) | (limits > n_rows)).any().item()):
        raise ValueError('%s: limits outside [0, %d]' % (name, n_rows))
    limits = limits.to(torch.int32).contiguous()
    dist = torch.empty((q_rows, k), dtype=torch.float32, device=queries.device)
    idx = torch.empty((q_rows, k), dtype=torch.int32, device=queries.device)
    if q_rows == 0:
        return dist, idx
    lib = _native.load()
    ws, ws_bytes = _flat_l2_workspace(name, lib, q_rows, n_rows, d, k, queries.device)
    check(lib.hfl_flat_l2_topk_prefix(dist.data_ptr(), idx.data_ptr(), queries.data_ptr(), database.data_ptr(),
                                      None if database_sq_norms is None else database_sq_norms.data_ptr(),
                                      limits.data_ptr(), q_rows, n_rows, d, k, ws.data_ptr(), ws_bytes, _stream()),
          'hfl_flat_l2_topk_prefix')
    return dist, idx


def augment_clouds(points, sizes, table_rows, config, seed: int, cloud_base: int = 0, selection_keys=None,
                   return_index: bool = False):
    """`hfl_augment_clouds` on a concatenated batch: points (P, 3) fp32 on the GPU, `sizes` the clouds' point counts (host
    integers), `table_rows` the (B, 12) uint32 host table of `hfl_augment_cloud` rows, `config` a `_native.AugmentConfig`,
    `selection_keys` an optional (P,) int32 device tensor holding uint32 bit patterns.  Returns (out (P, 3), counts (B,)
    int32, index (P,) int32 or None): the kept points of cloud b start at its input offset."""
    _dev(points, selection_keys)
    if points.dtype != torch.float32 or not points.is_contiguous() or points.dim() != 2 or points.shape[1] != 3:
        raise TypeError('augment_clouds takes a contiguous (P, 3) float32 tensor')
    off_host = np.ascontiguousarray(np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]), dtype=np.int64)
    rows = np.ascontiguousarray(table_rows, dtype=np.uint32)
    batch = len(off_host) - 1
    if rows.shape != (batch, 12) or int(off_host[-1]) != points.shape[0]:
        raise ValueError('augment_clouds: %d clouds of %d points, table %r, points %r'
                         % (batch, int(off_host[-1]), rows.shape, tuple(points.shape)))
    if selection_keys is not None and (selection_keys.dtype != torch.int32 or selection_keys.numel() != points.shape[0]
                                       or not selection_keys.is_contiguous()):
        raise TypeError('augment_clouds: selection keys are one contiguous int32 word per point')
    off = torch.from_numpy(off_host).to(points.device, non_blocking=True)
    table = torch.from_numpy(rows.view(np.int32)).to(points.device, non_blocking=True)
    out = torch.empty_like(points)
    counts = torch.empty(batch, dtype=torch.int32, device=points.device)
    index = torch.empty(points.shape[0], dtype=torch.int32, device=points.device) if return_index else None
    check(_native.load().hfl_augment_clouds(
        out.data_ptr(), counts.data_ptr(), index.data_ptr() if return_index else None, points.data_ptr(), off.data_ptr(),
        off_host.ctypes.data, batch, table.data_ptr(), rows.ctypes.data, ctypes.byref(config), int(seed) & (2 ** 64 - 1),
        int(cloud_base), selection_keys.data_ptr() if selection_keys is not None else None, _stream()), 'hfl_augment_clouds')
    return out, counts, index
