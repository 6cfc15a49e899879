"""HOTFormerLoc on MI355X: module tree with the reference's parameter names, forward
re-designed around the HIP kernels.

Drop-in contract: `model_factory(ModelParams)` returns a
`torch.nn.Module` whose `forward({'octree': O}) -> {'global': (B, output_dim)}` and whose
`state_dict()` keys/shapes equal the reference's (Appendix D), so reference checkpoints load
with `load_state_dict`.  Reference files followed: `models/hotformerloc.py`,
`models/hotformerloc_backbone.py`, `models/octformer_backbone.py`,
`models/layers/{octformer_layers,pooling,pooling_wrapper,salsa}.py`.

What is different from the reference (same function, different dataflow):
  * tokens are never padded, permuted into windows or concatenated with relay tokens in
    HBM: per-token ops (LayerNorm, Linear, MLP -- hipBLASLt fp32 through PyTorch-ROCm) run
    on the octree-ordered (N_t, C) stream, windows exist only as index arithmetic inside
    the attention kernel (`ops.window_attention`);
  * in the pyramid stage every depth keeps ONE buffer [tokens | relay tokens] so the
    token and relay-token rows share each GEMM launch;
  * relay-token self-attention is ragged per cloud (`ops.relay_attention`), no
    concat/pad/split, no host sync;
  * CPE = depth-wise octree conv + LayerNorm + residual is one kernel (`ops.cpe_forward`).
Only the options the shipped configs use are implemented; anything else raises.
"""

import contextlib
import functools
import os
from typing import Dict, List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

from . import autograd as ag
from . import dwconv as hdw
from . import ops
from ._native import (BlockWeights, RelayBlockWeights, WindowAttnDesc, FUSE_ATTN_NO_RELAY, FUSE_ATTN_WS, PHASE_WHOLE,
                      PHASE_TOKENS, PHASE_REST, PHASE_RELAY_QKV, PHASE_TAIL)
from .plan import WindowPlan
from .weight_cache import _STORE as _W3_CACHE, derived     # the one store of weight images


_FORCE_TRAIN_PATH = False


def _grad_path(x=None) -> bool:
    """True when autograd must see the op (training / fine-tuning): route through the
    autograd Functions instead of the fused inference kernels."""
    return torch.is_grad_enabled() or _FORCE_TRAIN_PATH


@contextlib.contextmanager
def training_numerics():
    """Run the training-path kernels even with autograd off.  Stage 1 of the multi-staged step
    (`training/trainer.py:305-317`) must produce the SAME descriptors as stage 3 recomputes with autograd --
    the loss gradient is taken at the stage-1 values, and tau1 = 0.01 amplifies any difference 100x."""
    global _FORCE_TRAIN_PATH
    old, _FORCE_TRAIN_PATH = _FORCE_TRAIN_PATH, True
    try:
        yield
    finally:
        _FORCE_TRAIN_PATH = old


def _ln(x, m: nn.LayerNorm):
    """LayerNorm over channels: HIP kernel in inference, torch (autograd) when grads are needed."""
    if x.is_cuda and not _grad_path(x) and x.shape[-1] in ops._LN_CHANNELS:
        return ops.layer_norm(x, m.weight, m.bias, m.eps)
    if x.is_cuda and x.numel() > 0 and x.shape[-1] in ops._LN_CHANNELS and x.dtype == torch.float32:
        return ag.layer_norm(x, m.weight, m.bias, m.eps)            # HIP forward + backward
    return F.layer_norm(x, m.normalized_shape, m.weight, m.bias, m.eps)


def _add_ln(x, y, m: nn.LayerNorm):
    """(x + y, LN(x + y)): one fused pass in inference."""
    if x.is_cuda and not _grad_path(x) and x.shape[-1] in ops._LN_CHANNELS:
        return ops.add_layer_norm(x, y, m.weight, m.bias, m.eps)
    x = x + y
    return x, _ln(x, m)


# ---- Linear layers: 'fp32' = hipBLASLt fp32 GEMM; 'bf16x3' = one bf16 GEMM over K-concatenated
# (hi|hi|lo) x (hi|lo|hi) operands with fp32 accumulation/output (include/hotformerloc_hip.h section 9).
# 'x3' = the same split arithmetic on the hand-written kernel (csrc/gemm_x3.hip: pre-split "split2" operands, bias /
# GELU / residual / re-split fused into the epilogue) for the Linear layers of the transformer blocks.
# 'x6' = MATCHED PRECISION: fp32-grade products on the hand-written kernel csrc/gemm_x6.hip (three bf16 planes per operand,
# six plane products, fp32 accumulation: as accurate as an fp32 GEMM), fp32 LayerNorm / softmax / GELU, window attention
# on the fp32 matrix cores -- the reference's own arithmetic (models/layers/octformer_layers.py:53-59,
# models/octformer_backbone.py:52-93) without a library GEMM in the transformer blocks.
_GEMM_MODE = os.environ.get('HFL_GEMM', 'x3')   # product switch (set_gemm_mode): x3 | x6 | fp32 | bf16x3
_SIDE_STREAM_MAX_ROWS = 32768                    # pyramid depths up to this many rows run on side streams

# Schedule and fusion seams: module attributes (no environment read) switched only by the tests and bench.py, each to compare a
# fused launch or a schedule with the plain form it replaces.
_PYRAMID_STREAMS = True        # pyramid depths on separate HIP streams (set_pyramid_streams)
_SERIAL_STREAMS = False        # ... their launches in the same order on one stream (set_pyramid_streams('serial'))
# training-path Linear layers on split-bf16 GEMMs (autograd.LinearSplitFn).  Off by default: parity-tested, but
# at 191 ms/step (B=32, Wild-Places) still slower than the fp32 hipBLASLt route (145 ms) because the operand
# splits of the backward are torch element-wise passes; needs fused split kernels to pay off.
_TRAIN_SPLIT = False
# training-path Linear layers on the hand-written split GEMMs (autograd.LinearFn with the X3 family: forward + dx on
# hfl_linear_x3, dW / db on hfl_wgrad_x3)
_TRAIN_X3 = True
# GEMM mode 'x6' training-path Linear layers on the hand-written fp32-grade kernels (autograd.LinearFn / MlpFn /
# LnMlpResidualFn with the X6 family: forward and dx on hfl_linear_x6, dW / db on hfl_wgrad_f32); off = the fp32 library
# GEMMs (F.linear)
_TRAIN_X6 = True
_TRAIN_MLP = True              # fused fc1 -> GELU -> fc2 autograd Function
_SPARSE_CONV = True            # large 3x3x3 convs over live taps only
_EARLY_PHASE = True            # token-row half of a block issued before / beside RTSA
# LN1 -> qkv -> window attention of a relay-token block's token rows as one launch (csrc/attn_ws.hip) from this many token rows
_ATTN_WS = True
_ATTN_WS_MIN_ROWS = 40000
_ATTN_WS_EARLY = False         # keep the early-phase schedule beside it
_MERGED_ATTN = True            # window attention of an iteration's levels as one launch
# Inference blocks as one native call (hfl_block_forward_x3, hfl_relay_block_forward_x3); False: the same launches issued one
# by one through the Python wrappers.  The flag says WHO issues a block's launches, not which kernels run.
_NATIVE_BLOCK = True
# The relay-token block as ONE launch (hfl_relay_block_fused_x3, csrc/relay_block.hip) where hfl_relay_block_fused_ok takes the
# shape (C = 256, 16 heads, at most 64 relay tokens per cloud); False: its five launches everywhere (routes: _native_route).
_RELAY_FUSED = True
# The LayerNorm [+ ReLU] behind an octree convolution inside the convolution's last launch (hfl_slot_sum_norm) on the inference
# live-tap routes; False: slot sum and norm as two launches everywhere.
_CONV_NORM_FUSED = True
# Every FeatureMixerLayer of the Mixer aggregator plus row_proj as ONE launch (hfl_mixer_chain_x3, csrc/mixer_chain.hip) and the
# rest of the head -- channel_proj, biases, flatten, the descriptor's L2 normalisation -- as a second (hfl_descriptor_tail), where
# hfl_mixer_chain_ok takes the shapes (C = hidden = 256, at most 4 layers, out_d <= 8); False: a launch (+ its reduce) per
# layer, hfl_mixer_tail and F.normalize, as before.
_MIXER_CHAIN = True
_Q_PRESCALE = 16 ** -0.5 * 1.4426950408889634    # folded into q for the fp16-MFMA attention kernels: head dim 16's scale x log2 e


def set_train_split(enabled: bool):
    """Route the training-path Linear layers through the split-bf16 GEMMs (experimental, see _TRAIN_SPLIT)."""
    global _TRAIN_SPLIT
    _TRAIN_SPLIT = bool(enabled)


def set_train_x3(enabled: bool):
    """Training-path Linear layers through `autograd.linear_x3` (default on in GEMM mode 'x3')."""
    global _TRAIN_X3
    _TRAIN_X3 = bool(enabled)


def set_train_x6(enabled: bool):
    """Training-path Linear layers of GEMM mode 'x6' through `autograd.linear_x6` and the MLP Functions (default on);
    False: torch's fp32 Linear (hipBLASLt) as before."""
    global _TRAIN_X6
    _TRAIN_X6 = bool(enabled)


def set_pyramid_streams(enabled):
    """Run the pyramid depths of one H-OSA iteration on separate HIP streams (inference path).  'serial': the launches of
    that schedule, in its order, all on the current stream (bench.py's roofline leg: a kernel's events then bracket the
    kernel alone)."""
    global _PYRAMID_STREAMS, _SERIAL_STREAMS
    _SERIAL_STREAMS = enabled == 'serial'
    _PYRAMID_STREAMS = bool(enabled)


def set_gemm_mode(mode: str):
    global _GEMM_MODE
    assert mode in ('fp32', 'bf16x3', 'x3', 'x6')
    _GEMM_MODE = mode


def get_gemm_mode() -> str:
    return _GEMM_MODE


def _split_path(x) -> bool:
    # (channel widths that are not a multiple of the GEMM tile, e.g. 192 in per-level-width configs: fp32 library path)
    return _GEMM_MODE in ('bf16x3', 'x3') and x.is_cuda and not _grad_path() and x.shape[-1] % 128 == 0


def _w2(lin: nn.Linear):
    """split2 layout of a Linear weight for `ops.linear_x3`: the entry of `autograd._w2_cached(w, False)`, built here with
    torch arithmetic (bit-identical to the kernel's, see there; also runs on CPU tensors)."""
    return ag._weight_image('x3', ops.split2_weight, lin.weight, False)


def _w6(lin: nn.Linear):
    """The three bf16 planes of a Linear weight for `ops.linear_x6` (one image for inference and training)."""
    return ag._w6_cached(lin.weight, False)


def _x6_lin_ok(lin: nn.Linear) -> bool:
    return ops.linear_x6_ok(lin.in_features, lin.out_features)


def _x6_path(x, *linears) -> bool:
    """Matched-precision inference path: GEMM mode 'x6', no autograd, fp32 rows on the GPU, every Linear a shape the kernel
    takes (in_features % 32 == 0, out_features % 128 == 0)."""
    return (_GEMM_MODE == 'x6' and x.is_cuda and not _grad_path() and x.dtype == torch.float32 and x.numel() > 0
            and all(_x6_lin_ok(l) for l in linears))


def _x3_train(x, *linears) -> bool:
    """Split-precision training Functions apply: GEMM mode 'x3', fp32 rows on the GPU, every Linear a shape the hand-written
    kernels take in both directions.  `_grad_path()` is not asked here but by the callers that need it: a block in train mode
    with live stochastic depth takes the fused residual branches also without autograd."""
    return (_GEMM_MODE == 'x3' and _TRAIN_X3 and x.is_cuda and x.dtype == torch.float32 and x.numel() > 0
            and all(ag.linear_x3_ok(l.in_features, l.out_features) for l in linears))


def _x6_train(x, *linears) -> bool:
    """Matched-precision training path: GEMM mode 'x6' under autograd (or `training_numerics`), fp32 rows on the GPU, every
    Linear a shape the hand-written kernels take in both directions."""
    return (_GEMM_MODE == 'x6' and _TRAIN_X6 and x.is_cuda and _grad_path() and x.dtype == torch.float32 and x.numel() > 0
            and all(ag.linear_x6_ok(l.in_features, l.out_features) for l in linears))


def _block_tail_x6(x, attn_out, proj: nn.Linear, norm2: nn.LayerNorm, mlp: 'MLP'):
    """x + proj(attn_out) -> x + fc2(gelu(fc1(LN2(x)))) with fp32-grade products: bias + residual ride in the proj / fc2
    launches, bias + GELU in fc1's (four launches: proj, LayerNorm, fc1, fc2)."""
    x = ops.linear_x6(attn_out, _w6(proj), bias=proj.bias, residual=x)
    h = ops.layer_norm(x, norm2.weight, norm2.bias, norm2.eps)
    g = ops.linear_x6(h, _w6(mlp.fc1), bias=mlp.fc1.bias, gelu=True)
    return ops.linear_x6(g, _w6(mlp.fc2), bias=mlp.fc2.bias, residual=x)


# LN2 -> fc1 -> GELU -> fc2 -> residual as ONE launch (csrc/mlp_fused.hip) from this many rows on.  (Rounds 3-4: 24 576 -- below
# that the three-launch form is as fast ALONE.  In the step the coarse pyramid levels' chains are launch-bound: with them on the
# fused launches too -- hidden / feature dimension split over the chip -- three alternating runs gave 2952-2975 clouds/s against
# 2914-2947, profiles/r05_g_ab.log.)
_MLP_FUSED_MIN_ROWS = 1000


def _mlp_pack(mlp: 'MLP', rows: int):
    """Weight image of the fused MLP launch for this block, or None when the launch does not apply (channel width, row count,
    missing biases).  Cached per (fc1, fc2) parameter pair like `_w2`."""
    f1, f2 = mlp.fc1, mlp.fc2
    c = f1.in_features
    if not (rows >= _MLP_FUSED_MIN_ROWS and c in (128, 256) and f1.out_features == 4 * c
            and f2.in_features == 4 * c and f2.out_features == c and f1.bias is not None and f2.bias is not None):
        return None
    w1, w2 = f1.weight, f2.weight
    return derived('mlp', (w1, w2), lambda: ops.mlp_fused_pack(w1, w2))


# LN1 -> qkv of the token rows as ONE launch (csrc/qkv_fused.hip) from 24 576 rows on (C = 128, 118 096 rows: 71 vs 96 us for
# LayerNorm + qkv GEMM; C = 256, 65 536 rows: 95 vs 114-122 us).  Round 3 skipped C = 256 shapes whose last round of 32 768 rows
# was less than half full (66 775 rows, 2.04 rounds: three passes, 153 vs 127 us); since the left-over rows are computed with
# the output features split over the workgroups (round 4) that shape takes 101 us and the restriction is gone.
_QKV_FUSED_MIN_ROWS = 1000


def _qkv_pack(att: 'OctreeAttention', rows: int):
    """Weight image of the fused LN1 -> qkv launch for this block, or None when the launch does not apply / does not pay."""
    lin = att.qkv
    c = lin.in_features
    if not (rows >= _QKV_FUSED_MIN_ROWS and c in (128, 256) and lin.out_features == 3 * c and lin.bias is not None):
        return None
    w = lin.weight
    return derived('qkvpack', (w,), lambda: ops.qkv_fused_pack(w))


def _relay_pack(att: 'RTAttention', mlp: 'MLP'):
    """Weight image of the one-launch relay-token block (csrc/relay_block.hip), or None when the launch does not apply
    (C = 256 with 16 heads, every bias present).  Cached per parameter set like `_mlp_pack`."""
    lins = (att.qkv, att.proj, mlp.fc1, mlp.fc2)
    c = att.dim
    if not (c == 256 and att.num_heads == 16 and mlp.fc1.out_features == 4 * c and all(l.bias is not None for l in lins)):
        return None
    ws = tuple(l.weight for l in lins)
    return derived('relaypack', ws, lambda: ops.relay_block_pack(*ws))


def _block_tail_x3(x, attn_out2, attn: 'OctreeAttention', norm2: nn.LayerNorm, mlp: 'MLP', fused_any_rows: bool = False):
    """proj (+bias +residual) -> LN2 -> fc1 (+bias, GELU, re-split) -> fc2 (+bias +residual): the proj launch of the
    hand-written GEMM, then the MLP branch as one fused launch (hidden activation in registers) or, for small row counts,
    as LayerNorm + two GEMM launches (the M x 4C hidden activation crosses HBM once each way as 4 B per element)."""
    x = ops.linear_x3(attn_out2, _w2(attn.proj), bias=attn.proj.bias, residual=x)
    pack = _mlp_pack(mlp, _MLP_FUSED_MIN_ROWS if fused_any_rows else x.shape[0])
    if pack is not None:
        return ops.ln_mlp_fused(x, norm2.weight, norm2.bias, norm2.eps, pack, mlp.fc1.bias, mlp.fc2.bias)
    h2 = ops.layer_norm_split2(x, norm2.weight, norm2.bias, norm2.eps)
    g2 = ops.linear_x3(h2, _w2(mlp.fc1), bias=mlp.fc1.bias, gelu_split_out=True)
    return ops.linear_x3(g2, _w2(mlp.fc2), bias=mlp.fc2.bias, residual=x)


def _w3(lin: nn.Linear):
    return ag._w3_cached(lin.weight, False)


class SplitLinear(nn.Linear):
    """`nn.Linear` whose training-path products use the split-bf16 GEMMs (autograd.LinearSplitFn) when the
    GEMM mode is 'bf16x3'; parameters, names and the fp32 fallback are those of nn.Linear."""

    def forward(self, x):
        if _grad_path() and _x3_train(x, self):
            return ag.linear_x3(x, self.weight, self.bias)       # hand-written split GEMM, forward and dx
        if (_GEMM_MODE == 'bf16x3' and _TRAIN_SPLIT and x.is_cuda and _grad_path()
                and self.in_features % 8 == 0 and self.out_features % 8 == 0 and x.numel() > 0):
            return ag.linear_split(x, self.weight, self.bias)
        if _x6_train(x, self):
            return ag.linear_x6(x, self.weight, self.bias)       # fp32-grade forward and dx, fp32-MFMA dW
        if _x6_path(x, self):
            y = ops.linear_x6(x.reshape(-1, self.in_features), _w6(self), bias=self.bias)
            return y.view(*x.shape[:-1], self.out_features)
        return F.linear(x, self.weight, self.bias)


def _block_tail_split(x, attn_out3, attn: 'OctreeAttention', norm2: nn.LayerNorm, mlp: 'MLP'):
    """proj -> +residual -> LN2 -> fc1 -> GELU -> fc2 -> +residual: bias + residual in the proj / fc2 GEMM launches, fc1's
    bias in the GELU pass that follows its GEMM."""
    if _GEMM_MODE == 'x3':
        return _block_tail_x3(x, attn_out3, attn, norm2, mlp)
    # bias + residual ride in the GEMM launch (hfl_gemm_bf16): no pass over the residual stream
    x = ops.gemm_bf16(attn_out3, _w3(attn.proj), bias=attn.proj.bias, residual=x)
    h3 = ops.layer_norm_split3(x, norm2.weight, norm2.bias, norm2.eps)
    g3 = ops.bias_gelu_split3(ops.split_mm(h3, _w3(mlp.fc1)), mlp.fc1.bias)
    return ops.gemm_bf16(g3, _w3(mlp.fc2), bias=mlp.fc2.bias, residual=x)


# Activation checkpointing policy.  `grad_checkpoint = True` in the reference's configs buys memory with a second forward of
# every block (written for 24-80 GB devices).  'always': as the reference; 'never': keep the activations; 'auto' (default):
# keep them when they fit comfortably -- an MI355X has 288 GB and the largest shipped training shape (CS-Wild-Places, 64
# clouds) keeps ~40 GB -- and checkpoint like the reference otherwise: a stage keeps its blocks' activations when their
# estimated size is below _CHECKPOINT_FREE_FRACTION of the memory that is free when the stage starts.
# The results are the same either way (the recomputation repeats the same launches on the same inputs).
_CHECKPOINT_POLICY = os.environ.get('HFL_CHECKPOINT', 'auto')
_CHECKPOINT_FREE_FRACTION = float(os.environ.get('HFL_CHECKPOINT_FREE_FRACTION', '0.5'))
# what one transformer block keeps per (row, channel) for its backward: MLP branch x 4 + LN split 4 + GELU split 16 +
# pre-activation 16, attention branch x 4 + LN split 4 + qkv 12 + attention split 4, CPE input and norm ~16 (measured:
# 40.7 GiB against 38 GiB by this count on the config-3 workload)
_BLOCK_BYTES_PER_ROW_CHANNEL = 80


def set_checkpoint_policy(policy: str):
    """'always' | 'never' | 'auto' (see above); returns the previous policy."""
    global _CHECKPOINT_POLICY
    assert policy in ('always', 'never', 'auto')
    prev, _CHECKPOINT_POLICY = _CHECKPOINT_POLICY, policy
    return prev


def _free_memory(device) -> int:
    free, _ = torch.cuda.mem_get_info(device)
    # (what the caching allocator holds but has not handed out is free for this purpose)
    return free + torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)


def _use_checkpoint(stage, row_channels: int = 0, n_blocks: int = 1, device=None) -> bool:
    """The reference checkpoints every transformer block `if self.grad_checkpoint and self.training`
    (models/octformer_backbone.py:415-416, models/hotformerloc_backbone.py:596-618); here additionally subject to the policy
    above, decided once per forward and stage (all blocks of a stage go the same way): `row_channels` = sum over the stage's
    levels of rows x channels, `n_blocks` = blocks per level."""
    if not (bool(stage.grad_checkpoint) and stage.training and torch.is_grad_enabled()):
        return False
    if _CHECKPOINT_POLICY == 'always':
        return True
    if _CHECKPOINT_POLICY == 'never':
        return False
    if device is None or device.type != 'cuda' or row_channels <= 0:
        return True
    need = row_channels * n_blocks * _BLOCK_BYTES_PER_ROW_CHANNEL
    return need > _CHECKPOINT_FREE_FRACTION * _free_memory(device)


def _checkpoint_block(blk, *args):
    """`checkpoint(blk, *args, use_reentrant=False)` with the block's stochastic-depth factors captured in the closure: the
    recomputation in the backward must see the draws of ITS forward, also when another forward has re-armed the model in
    between (forward A, forward B, backward A).  The reference's checkpoint gets this from the preserved RNG state
    (octformer_backbone.py:415-416); here the draws are tensors handed out by `arm_drop_paths`."""
    mods = blk.__dict__.get('_drop_path_mods')
    if mods is None:
        mods = blk.__dict__['_drop_path_mods'] = [m for m in blk.modules() if isinstance(m, OctreeDropPath)]
    snap = [(m, m._factors) for m in mods]

    def run(*a):
        # the saved draws are visible during the block call only: the recomputation in the backward must not leave the previous
        # step's factors armed on the modules (a submodule called on its own afterwards draws fresh ones)
        prev = [(m, m._factors, m._calls) for m, _ in snap]
        for m, f in snap:
            m._factors, m._calls = f, 0
        try:
            return blk(*a)
        finally:
            for m, f, c in prev:
                m._factors, m._calls = f, c
    return checkpoint(run, *args, use_reentrant=False)


def disarm_drop_paths(model: nn.Module):
    """End of a model forward: the pooled draws belong to that forward only.  A submodule called on its own afterwards
    (backbone alone, tests) draws fresh factors instead of silently reusing the last forward's."""
    cache = model.__dict__.get('_drop_path_cache')
    if cache is not None:
        for m in cache['mods']:
            m._factors = None


def _require_layernorm(conv_norm: str):
    if conv_norm.lower() != 'layernorm':
        raise NotImplementedError("conv_norm=%r: every shipped config uses 'layernorm'" % conv_norm)


def arm_drop_paths(model: nn.Module, batch_size: int, device, dtype=torch.float32):
    """Draw the per-cloud stochastic-depth factors of every active `OctreeDropPath` of `model` for one forward in three
    launches (rand, floor, div over an (instances x 2, B) matrix) and hand each instance its two rows.  Same distribution as
    the reference's per-call draws (models/layers/octformer_layers.py:213-289: independent Bernoulli(keep) per call and
    cloud).  The draws do not follow the reference's RNG stream; tests/test_gpu_train_drop_path.py replaces this function to
    replay the draws recorded from the reference (tests/golden/train_*.npz) and so checks stochastic depth against it."""
    cache = model.__dict__.get('_drop_path_cache')
    if cache is None:
        cache = model.__dict__['_drop_path_cache'] = {'mods': [m for m in model.modules() if isinstance(m, OctreeDropPath)]}
    mods = [m for m in cache['mods'] if m.drop_prob > 0.0]
    sig = (tuple((m.drop_prob, m.scale_by_keep) for m in mods), str(device), dtype)
    if cache.get('sig') != sig:
        keep = [1.0 - m.drop_prob for m in mods for _ in range(2)]
        div = [(1.0 - m.drop_prob) if (m.scale_by_keep and m.drop_prob < 1.0) else 1.0 for m in mods for _ in range(2)]
        cache['sig'] = sig
        cache['keep'] = torch.tensor(keep, dtype=dtype).reshape(-1, 1).to(device)
        cache['div'] = torch.tensor(div, dtype=dtype).reshape(-1, 1).to(device)
    if not mods:
        return
    f = torch.floor(torch.rand(2 * len(mods), batch_size, dtype=dtype, device=device) + cache['keep']) / cache['div']
    for i, m in enumerate(mods):
        m._factors = f[2 * i:2 * i + 2]
        m._calls = 0


class OctreeDropPath(nn.Module):
    """Per-cloud stochastic depth (models/layers/octformer_layers.py:213-289): in training every
    cloud keeps (scaled by 1/keep) or drops a residual branch; identity in eval.  `bid` gives the
    cloud of every row (relay rows carry their window owner, padding rows the last cloud)."""

    def __init__(self, drop_prob: float = 0.0, scale_by_keep: bool = True):
        super().__init__()
        self.drop_prob = float(drop_prob)
        self.scale_by_keep = scale_by_keep

    # Every block calls its drop path twice per forward (attention branch, MLP branch).  Inside a model forward the draws of
    # ALL instances are made at once (`arm_drop_paths`: one rand + floor + div for the whole network instead of four tiny
    # launches per call, ~570 launches per CS-Wild-Places training step); `_factors` holds this instance's two rows (2, B).
    # A recomputation under gradient checkpointing calls the same two branches again and so reads the same rows.
    _factors = None
    _calls = 0

    def _draw(self, batch_size: int, dtype, device):
        """(B,) per-cloud factor of one call: 0 or 1 / keep.  Armed factors that do not fit the call are an error: drawing
        fresh ones instead would silently give the two calls of a recomputation different draws."""
        f = self._factors
        if f is not None:
            if f.dim() != 2 or f.shape[1] != batch_size or f.device != device or f.dtype != dtype:
                raise RuntimeError('OctreeDropPath: armed factors %s %s on %s do not match a call with batch %d, %s on %s'
                                   % (tuple(f.shape), f.dtype, f.device, batch_size, dtype, device))
            r = f[self._calls % f.shape[0]]
            self._calls += 1
            return r
        keep = 1.0 - self.drop_prob
        rnd = torch.floor(torch.rand(batch_size, dtype=dtype, device=device) + keep)
        if keep > 0.0 and self.scale_by_keep:
            rnd = rnd / keep
        return rnd

    def forward(self, data, bid, batch_size: int):
        if self.drop_prob <= 0.0 or not self.training:
            return data
        return data * self._draw(batch_size, data.dtype, data.device)[bid].unsqueeze(1)

    def row_scale(self, bid, batch_size: int, like):
        """The same draw as forward() as a per-row factor (rows,) for the fused residual branches; None when inactive."""
        if self.drop_prob <= 0.0 or not self.training:
            return None
        return self._draw(batch_size, like.dtype, like.device)[bid].reshape(-1).contiguous()

    def extra_repr(self):
        return 'drop_prob={:.4f}'.format(self.drop_prob)


# --------------------------------------------------------------------------- convs
class _NormTail:
    """The caller's LayerNorm [+ ReLU] [+ split2 hand-over], offered to an OctreeConv for its last launch; the convolution
    sets `done` where its route took it (the x3 / x6 live-tap routes), and the caller runs the norm itself where not."""
    __slots__ = ('norm', 'relu', 'split2', 'done')

    def __init__(self, norm: nn.LayerNorm, relu: bool, split2: bool = False):
        self.norm, self.relu, self.split2, self.done = norm, relu, split2, False


class OctreeConv(nn.Module):
    """`ocnn.nn.OctreeConv` (nempty=True): parameter `weights` (kdim, Cin, Cout) [+ `bias`].
    gather through the neighbour / child table (HIP) then one fp32 GEMM."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: List[int] = [3],
                 stride: int = 1, nempty: bool = True, use_bias: bool = False):
        super().__init__()
        if not nempty:
            raise NotImplementedError('nempty=False octree conv is off the HOTFormerLoc path')
        ks = list(kernel_size) * 3 if len(kernel_size) == 1 else list(kernel_size)
        self.kernel = ''.join(str(k) for k in ks)
        self.kdim = ks[0] * ks[1] * ks[2]
        self.in_channels, self.out_channels, self.stride = in_channels, out_channels, stride
        self.weights = nn.Parameter(torch.empty(self.kdim, in_channels, out_channels))
        self.bias = nn.Parameter(torch.zeros(out_channels)) if use_bias else None
        nn.init.xavier_uniform_(self.weights)

    def takes_split2(self) -> bool:
        """Inference: does forward() run the grouped split-precision GEMM over the live taps, i.e. can it take the split2
        form of its input (rows, 2 Cin) bf16 instead of fp32 rows?"""
        return (_SPARSE_CONV and (self.kernel, self.stride) in (('333', 1), ('222', 2)) and self.in_channels >= 32
                and _GEMM_MODE == 'x3' and self.in_channels % 32 == 0
                and (self.out_channels % 128 == 0 or self.out_channels == 64) and not _grad_path())

    def forward(self, data: torch.Tensor, octree, depth: int, tail: Optional[_NormTail] = None):
        if data.dtype == torch.bfloat16:                 # split2 rows from the previous layer's fused norm + ReLU
            assert self.takes_split2() and data.shape[1] == 2 * self.in_channels
            return self._forward_live_taps(data, octree, depth, tail)
        if (_SPARSE_CONV and (self.kernel, self.stride) in (('333', 1), ('222', 2)) and self.in_channels >= 32
                and data.is_cuda):
            if not _grad_path(data):
                return self._forward_live_taps(data, octree, depth, tail)
            if self.in_channels % 64 == 0 and self.out_channels % 64 == 0:      # tile shape of hfl_tap_wgrad
                out = ag.live_tap_conv(data, self.weights, octree, depth, self.kernel, self.stride)
                return out if self.bias is None else out + self.bias
        neigh = octree.get_neigh(depth, self.kernel, self.stride, nempty=True)
        col = ag.octree_gather(data, neigh) if _grad_path(data) else ops.octree_gather(data, neigh)
        w = self.weights.reshape(self.kdim * self.in_channels, self.out_channels)
        if torch.is_grad_enabled() and (col.requires_grad or self.weights.requires_grad):
            return ag.tall_mm(col, w, self.bias)          # (weight gradient contracted over the rows as a split-K product)
        if self.bias is not None:
            return torch.addmm(self.bias, col, w)
        return torch.mm(col, w)


    def _forward_live_taps(self, data, octree, depth, tail=None):
        """3x3x3 (stride 1) or 2x2x2 (stride 2) conv over the LIVE taps only.  The dense form gathers (N, 27*Cin) -- 80 % zeros on surface-like
        clouds (5.6 live taps of 27 at depth 5, 4 at depth 6) -- and multiplies all of it.  Here: gather one row
        per live (row, tap) pair in tap-major order, one GEMM per tap on its contiguous slice (W[k] is (Cin, Cout)),
        then every output row sums its own partial products through the slot table (the depth-wise conv kernel
        with unit weights: no atomics, fixed summation order)."""
        src, slot, edges = octree.sparse_taps(depth, self.kernel, self.stride)
        if (_GEMM_MODE == 'x3' and self.in_channels % 32 == 0
                and (self.out_channels % 128 == 0 or self.out_channels == 64) and edges[-1] > 0):
            # ONE launch of the split-precision GEMM over all taps: the pairs are gathered from the split2 form of the input
            # (a split2 row is Cin 4-byte cells, so the same gather kernel moves it), row tiles never straddle a tap and
            # carry the offset of their tap's weight block
            npad = max(self.out_channels, 128)
            d2 = data if data.dtype == torch.bfloat16 else ops.split2(data)
            if d2.shape[0] * self.in_channels * 4 < (1 << 32):
                # the GEMM's tile loader fetches the pairs' input rows itself: no (pairs, Cin) matrix in memory
                part = ops.linear_x3_grouped_gather(d2, src, ag._tap_blocks(self.weights, True, npad, ops.split2, 'taps2'),
                                                    octree.tap_tiles(depth, self.kernel, self.stride, npad), self.out_channels)
            else:
                gs = ops.octree_gather(d2.view(torch.float32), src).view(torch.bfloat16)
                part = ops.linear_x3_grouped(gs, ag._tap_blocks(self.weights, True, npad, ops.split2, 'taps2'),
                                             octree.tap_tiles(depth, self.kernel, self.stride, npad), self.out_channels)
            return self._slot_sum(part, slot, tail)
        if (_GEMM_MODE == 'x6' and not _grad_path() and data.dtype == torch.float32 and edges[-1] > 0
                and self.in_channels % 32 == 0 and (self.out_channels % 128 == 0 or self.out_channels == 64)):
            # matched precision: the same grouped launch on hfl_linear_x6 (fp32-grade products; the tile loader gathers the pairs'
            # input rows from the f32 rows themselves)
            npad = max(self.out_channels, 128)
            part = ops.linear_x6_grouped_gather(data, src, ag._tap_blocks(self.weights, True, npad),
                                                octree.tap_tiles(depth, self.kernel, self.stride, npad), self.out_channels)
            return self._slot_sum(part, slot, tail)
        g = ops.octree_gather(data, src)                                  # (P, Cin)
        part = torch.empty((g.shape[0], self.out_channels), dtype=torch.float32, device=data.device)
        w = self.weights
        for k in range(self.kdim):
            if edges[k + 1] > edges[k]:
                torch.mm(g[edges[k]:edges[k + 1]], w[k], out=part[edges[k]:edges[k + 1]])
        return self._slot_sum(part, slot)

    def _slot_sum(self, part, slot, tail=None):
        """every output row adds the partial products of its own live taps (+ the bias) in one pass (hfl_slot_sum); with the
        caller's norm `tail` in the same pass where the kernel takes the width (hfl_slot_sum_norm)"""
        if (tail is not None and _CONV_NORM_FUSED and part.shape[1] in ops._SLOT_NORM_CHANNELS and slot.shape[1] <= 32
                and slot.dtype == torch.int32 and slot.shape[0] > 0):
            tail.done = True
            return ops.slot_sum_norm(part, slot, self.bias, tail.norm.weight, tail.norm.bias, tail.norm.eps, relu=tail.relu,
                                     split2=tail.split2)
        if part.shape[1] % 4 == 0 and part.shape[1] <= 1024 and slot.shape[1] <= 27 and slot.dtype == torch.int32:
            return ops.slot_sum(part, slot, self.bias)
        out = ops.dwconv_forward_backward(part, self._unit(part.device), slot)
        return out if self.bias is None else out + self.bias

    def _unit(self, device):
        ones = self.__dict__.get('_unit_taps')
        if ones is None or ones.device != device:
            ones = torch.ones((self.kdim, 1, self.out_channels), dtype=torch.float32, device=device)
            self.__dict__['_unit_taps'] = ones
        return ones


class OctreeDWConvParams(nn.Module):
    """Holder of the depth-wise conv parameter `weights` (27, 1, C) (reference
    `dwconv.OctreeDWConv`, libs/dwconv/dwconv/nn.py:49-63); the op itself is fused into CPE."""

    def __init__(self, channels: int):
        super().__init__()
        self.weights = nn.Parameter(torch.empty(27, 1, channels))
        nn.init.xavier_uniform_(self.weights)


class OctreeConvNormRelu(nn.Module):
    """models/layers/octformer_layers.py:80-98"""

    def __init__(self, in_channels, out_channels, kernel_size=[3], stride=1, conv_norm='layernorm'):
        super().__init__()
        _require_layernorm(conv_norm)
        self.conv = OctreeConv(in_channels, out_channels, kernel_size, stride, nempty=True)
        self.norm = nn.LayerNorm(out_channels)

    def forward(self, data, octree, depth, split2_out: bool = False):
        """`split2_out` (inference): return the split2 operand of the next convolution's GEMM instead of fp32 rows."""
        tail = _NormTail(self.norm, True, split2_out)
        y = self.conv(data, octree, depth, tail)
        if tail.done:
            return y
        if y.is_cuda and not _grad_path(y) and y.shape[-1] in ops._LN_CHANNELS:
            return ops.layer_norm_relu(y, self.norm.weight, self.norm.bias, self.norm.eps, split2=split2_out)
        y = F.relu_(_ln(y, self.norm))
        # (a width the fused norm + ReLU kernel is not instantiated for, e.g. 192 of dim = 384: the split as its own pass)
        return ops.split2(y) if split2_out else y


class PatchEmbed(nn.Module):
    """models/octformer_backbone.py:424-461"""

    def __init__(self, in_channels=3, dim=96, num_down=2, conv_norm='layernorm', downsample_input_embeddings=True):
        super().__init__()
        self.num_stages = num_down
        self.downsample_input_embeddings = downsample_input_embeddings
        if not downsample_input_embeddings:            # num_down 3x3x3 convolutions at the input depth (:449-452)
            self.convs = nn.ModuleList([OctreeConvNormRelu(in_channels if i == 0 else dim, dim, [3], 1, conv_norm)
                                        for i in range(num_down)])
            return
        ch = [int(dim * 2 ** i) for i in range(-num_down, 1)]
        self.convs = nn.ModuleList([OctreeConvNormRelu(in_channels if i == 0 else ch[i], ch[i], [3], 1,
                                                       conv_norm) for i in range(num_down)])
        self.downsamples = nn.ModuleList([OctreeConvNormRelu(ch[i], ch[i + 1], [2], 2, conv_norm)
                                          for i in range(num_down)])
        self.proj = OctreeConvNormRelu(ch[-1], dim, [3], 1, conv_norm)

    def forward(self, data, octree, depth):
        if not self.downsample_input_embeddings:
            for i in range(self.num_stages):
                data = self.convs[i](data, octree, depth)
            return data
        # (inference: a layer whose successor runs the grouped split-precision GEMM hands it the split2 rows directly --
        # norm + ReLU + split in one pass instead of three)
        seq = []
        for i in range(self.num_stages):
            seq += [(self.convs[i], depth - i), (self.downsamples[i], depth - i)]
        seq.append((self.proj, depth - self.num_stages))
        fast = data.is_cuda and not _grad_path(data)
        for n, (m, d) in enumerate(seq):
            nxt = seq[n + 1][0].conv if n + 1 < len(seq) else None
            data = m(data, octree, d, split2_out=bool(fast and nxt is not None and nxt.takes_split2()))
        return data


class Downsample(nn.Module):
    """models/octformer_backbone.py:464-477"""

    def __init__(self, in_channels, out_channels, conv_norm='layernorm'):
        super().__init__()
        _require_layernorm(conv_norm)
        self.conv = OctreeConv(in_channels, out_channels, [2], stride=2, nempty=True, use_bias=True)
        self.norm = nn.LayerNorm(out_channels)

    def forward(self, data, octree, depth):
        tail = _NormTail(self.norm, False)
        y = self.conv(data, octree, depth, tail)
        return y if tail.done else _ln(y, self.norm)


# ---------------------------------------------------------------- transformer parts
class MLP(nn.Module):
    """models/layers/octformer_layers.py:38-59"""

    def __init__(self, in_features, hidden_features=None, out_features=None):
        super().__init__()
        self.fc1 = SplitLinear(in_features, hidden_features or in_features)
        self.fc2 = SplitLinear(hidden_features or in_features, out_features or in_features)

    def forward(self, x):
        f1, f2 = self.fc1, self.fc2
        if f1.bias is not None and f2.bias is not None:
            # the training family of these two Linears, or none (_TRAIN_MLP gates the x3 fused Functions only)
            fused = (ag.mlp_x3 if _TRAIN_MLP and _grad_path() and _x3_train(x, f1, f2)
                     else ag.mlp_x6 if _x6_train(x, f1, f2) else None)
            if fused is not None:
                return fused(x, f1.weight, f1.bias, f2.weight, f2.bias)      # GELU and its gradient inside the GEMMs
        if _x6_path(x, f1, f2) and x.dim() == 2:
            return ops.linear_x6(ops.linear_x6(x, _w6(f1), bias=f1.bias, gelu=True), _w6(f2), bias=f2.bias)
        return self.fc2(F.gelu(self.fc1(x)))


def _mlp_branch(x, norm: nn.LayerNorm, mlp: 'MLP', row_scale=None):
    """x + mlp(LN(x)) on the training path: one fused autograd Function when the shapes allow (LayerNorm writes the GEMM
    operand, GELU and the residual ride in the GEMM epilogues, the skip gradient joins inside the LayerNorm backward)."""
    f1, f2 = mlp.fc1, mlp.fc2
    if x.shape[-1] in ops._LN_CHANNELS and f1.bias is not None and f2.bias is not None:
        # the training family of these two Linears, or none (_TRAIN_MLP gates the x3 fused Functions only)
        fused = (ag.ln_mlp_residual_x3 if _TRAIN_MLP and _x3_train(x, f1, f2)
                 else ag.ln_mlp_residual_x6 if x.dim() == 2 and _x6_train(x, f1, f2) else None)
        if fused is not None:
            return fused(x, norm.weight, norm.bias, norm.eps, f1.weight, f1.bias, f2.weight, f2.bias, row_scale)
    y = mlp(_ln(x, norm))
    return x + (y if row_scale is None else y * row_scale.unsqueeze(1))


class CPE(nn.Module):
    """models/layers/octformer_layers.py:122-142.  xcpe=False: depth-wise octree conv + LayerNorm (one fused kernel in
    inference); xcpe=True (PointTransformerV3's xCPE): full octree conv with bias + Linear + LayerNorm."""

    def __init__(self, dim, conv_norm='layernorm', xcpe=False):
        super().__init__()
        _require_layernorm(conv_norm)
        self.xcpe = xcpe
        if xcpe:
            self.conv = OctreeConv(dim, dim, [3], 1, nempty=True, use_bias=True)
            self.linear = nn.Linear(dim, dim)
        else:
            self.conv = OctreeDWConvParams(dim)
            self.linear = nn.Identity()
        self.norm = nn.LayerNorm(dim)

    def forward(self, data, plan: WindowPlan, depth: int, residual: bool, out=None):
        if self.xcpe:
            y = _ln(self.linear(self.conv(data, plan.octree, depth)), self.norm)
            y = data + y if residual else y
            if out is not None:
                out.copy_(y)
                return out
            return y
        if (_grad_path(data) and data.shape[1] in (32, 64, 128, 256) and data.is_cuda
                and data.dtype == torch.float32 and out is None):
            # training: the fused launch as the forward (it also writes the convolution's output for the backward)
            return ag.cpe(data, self.conv.weights, self.norm.weight, self.norm.bias, plan.neigh(depth), residual,
                          self.norm.eps)
        if _grad_path(data) or data.shape[1] not in (32, 64, 128, 256):
            # dwconv (HIP fwd/bwd, libs/dwconv semantics) -> LayerNorm -> residual (also the inference path of channel
            # widths the fused kernel is not instantiated for, e.g. 192 in per-level-width configurations)
            y = _ln(hdw.octree_dwconv(data, self.conv.weights, plan.neigh(depth)), self.norm)
            y = data + y if residual else y
            if out is not None:
                out.copy_(y)
                return out
            return y
        return ops.cpe_forward(data, self.conv.weights, self.norm.weight, self.norm.bias,
                               plan.neigh(depth), residual, self.norm.eps, out=out)


class RPE(nn.Module):
    """models/layers/octformer_layers.py:144-174: only the table; the gather happens in
    registers inside the attention kernel."""

    def __init__(self, patch_size, num_heads, dilation=1):
        super().__init__()
        self.pos_bnd = int(0.8 * patch_size * dilation ** 0.5)
        self.rpe_num = 2 * self.pos_bnd + 1
        self.rpe_table = nn.Parameter(torch.zeros(3 * self.rpe_num, num_heads))
        nn.init.trunc_normal_(self.rpe_table, std=0.02)


class OctreeAttention(nn.Module):
    """models/octformer_backbone.py:24-106"""

    def __init__(self, dim, patch_size, num_heads, dilation=1, rt_per_window=0, use_rpe=True):
        super().__init__()
        if dim // num_heads != 16:
            raise NotImplementedError('head dim must be 16 (all shipped configs)')
        self.dim, self.patch_size, self.num_heads = dim, patch_size, num_heads
        self.dilation, self.rt_per_window = dilation, rt_per_window
        self.qkv = SplitLinear(dim, dim * 3)
        self.proj = SplitLinear(dim, dim)
        self.rpe = RPE(patch_size, num_heads, dilation) if use_rpe else None

    def _cfg(self, plan: WindowPlan, depth: int) -> dict:
        """The window-attention problem of this module at one depth, as the keyword arguments of the attention ops."""
        nt = plan.n_tokens[depth]
        return dict(n_tokens=nt, n_windows=plan.n_windows[depth], patch_size=self.patch_size,
                    dilation=self.dilation, n_relay=self.rt_per_window, n_heads=self.num_heads,
                    batch_size=plan.B, rt_row0=nt, depth=depth)

    def core(self, qkv, plan: WindowPlan, depth: int, qkv_bias=None, out_split=False, qkv_f16=False):
        cfg = self._cfg(plan, depth)
        table = None if self.rpe is None else self.rpe.rpe_table
        if _grad_path(qkv):
            return ag.window_attention(qkv, table, plan.meta[depth], **cfg)
        return ops.window_attention(qkv, plan.meta[depth], table, qkv_bias=qkv_bias,
                                    out_split=out_split, qkv_f16=qkv_f16, **cfg)

    def forward(self, x, plan: WindowPlan, depth: int):
        """x: (N_t [+ W], C) token rows [followed by the relay-token rows]."""
        return self.proj(self.core(self.qkv(x), plan, depth))

    def residual_branch(self, x, norm1: nn.LayerNorm, plan: WindowPlan, depth: int, row_scale=None):
        """x + attention(LN(x)) on the training path: one fused autograd Function when the shapes allow."""
        C = self.dim
        if _TRAIN_MLP and _x3_train(x, self.qkv, self.proj) and C in ops._LN_CHANNELS and self.proj.bias is not None:
            table = None if self.rpe is None else self.rpe.rpe_table
            return ag.ln_attn_residual_x3(x, norm1.weight, norm1.bias, norm1.eps, self.qkv.weight, self.qkv.bias, table,
                                          plan.meta[depth], self._cfg(plan, depth), self.proj.weight, self.proj.bias, row_scale)
        y = self.forward(_ln(x, norm1), plan, depth)
        return x + (y if row_scale is None else y * row_scale.unsqueeze(1))

    def forward_split(self, x, norm1: nn.LayerNorm, plan: WindowPlan, depth: int):
        """LN1 -> qkv -> attention, split-precision path; returns the bf16 operand of `proj`."""
        if _GEMM_MODE == 'x3':         # qkv bias folded into the GEMM epilogue, attention writes split2 rows
            f16 = _attn_f16_ok(x.shape[0], self, depth)
            nt = plan.n_tokens[depth]
            qpack = _qkv_pack(self, nt) if (f16 and x.dtype == torch.float32 and x.is_contiguous()) else None
            if qpack is not None:
                # as hfl_block_forward_x3 does it: LN1 -> qkv of the token rows in one launch, the relay rows through
                # LayerNorm + the qkv GEMM
                qkv = torch.empty((x.shape[0], 3 * x.shape[1]), dtype=torch.float32, device=x.device)
                ops.ln_qkv_fused(x[:nt], norm1.weight, norm1.bias, norm1.eps, qpack, self.qkv.bias, _Q_PRESCALE, out=qkv[:nt])
                if x.shape[0] > nt:          # the relay rows: the same launch, output features split over the workgroups
                    ops.ln_qkv_fused(x[nt:], norm1.weight, norm1.bias, norm1.eps, qpack, self.qkv.bias, _Q_PRESCALE, out=qkv[nt:])
                return self.core(qkv, plan, depth, out_split=2, qkv_f16=True)
            a2 = ops.layer_norm_split2(x, norm1.weight, norm1.bias, norm1.eps)
            if f16:
                # the projection writes q, k, v as fp16 (hi, lo) MFMA operands (q pre-scaled): fp16-MFMA window kernel
                qkv = ops.linear_x3_qkv(a2, _w2(self.qkv), self.qkv.bias, _Q_PRESCALE)
                return self.core(qkv, plan, depth, out_split=2, qkv_f16=True)
            qkv = ops.linear_x3(a2, _w2(self.qkv), bias=self.qkv.bias)
            return self.core(qkv, plan, depth, out_split=2)
        a3 = ops.layer_norm_split3(x, norm1.weight, norm1.bias, norm1.eps)
        return self.core(ops.split_mm(a3, _w3(self.qkv)), plan, depth, qkv_bias=self.qkv.bias,
                         out_split=True)


def _drops(block) -> bool:
    """Stochastic depth is live (train mode, non-zero probability): the fused inference paths do not apply it."""
    return block.training and block.drop_path.drop_prob > 0.0


def _fused_inference(block, x) -> bool:
    """Eligibility for the hand-written inference path, first layer: the fused split-precision kernels apply to this block on
    these rows (they know neither layer scale nor stochastic depth)."""
    return _split_path(x) and not block.use_layer_scale and not _drops(block)


def _native_rows(block, x) -> bool:
    """... second layer: the block's 'x3' launches can go out on the raw pointers of these rows, from a native call or as one
    launch (no kernel timer: it brackets launches issued from Python).  What one site adds stands there with its reason."""
    return (_fused_inference(block, x) and _GEMM_MODE == 'x3' and ops.KernelTimer.active is None
            and x.dtype == torch.float32 and x.is_contiguous())


def _init_layer_scale(block, dim, layer_scale):
    """`gamma1` / `gamma2`: learnable channel-wise multipliers of the attention / MLP branches when `layer_scale` is a
    number (models/octformer_backbone.py:214-229), the constant 1 otherwise (not parameters then, as in the reference)."""
    block.use_layer_scale = layer_scale is not None and type(layer_scale) in (int, float)
    if block.use_layer_scale:
        block.gamma1 = nn.Parameter(layer_scale * torch.ones(dim))
        block.gamma2 = nn.Parameter(layer_scale * torch.ones(dim))
    else:
        block.gamma1 = block.gamma2 = 1


_f16_ok = functools.lru_cache(maxsize=4096)(lambda *key: ops.window_attention_f16_ok(*key))


def _attn_f16_ok(rows, att, depth) -> bool:
    return _f16_ok(rows, att.patch_size, att.dilation, att.rt_per_window, att.num_heads, depth)


def _native_block_static(block, device):
    """(BlockWeights, tensors it points to) of a block, or None when the block's parameters do not qualify for the native
    call; cached (`weight_cache.derived`) and revalidated by the (version, pointer) stamp of every parameter (a few
    microseconds instead of rebuilding a 20-field ctypes structure per block and forward: the host runs only just ahead of
    the GPU)."""
    att, mlp, cpe = block.attention, block.mlp, block.cpe
    table = None if att.rpe is None else att.rpe.rpe_table
    plist = (cpe.conv.weights, cpe.norm.weight, cpe.norm.bias, block.norm1.weight, block.norm1.bias, block.norm2.weight,
             block.norm2.bias, att.qkv.bias, att.proj.bias, mlp.fc1.bias, mlp.fc2.bias, att.qkv.weight, att.proj.weight,
             mlp.fc1.weight, mlp.fc2.weight, table)

    def build():
        # the native call reads raw pointers: every parameter must be what the Python wrappers would have checked (fp32,
        # contiguous, on this device), the biases must exist and the three LayerNorms must share one eps
        ok = (all(p is not None for p in plist[:-1]) and block.norm1.eps == block.norm2.eps == cpe.norm.eps
              and all(p is None or (p.dtype == torch.float32 and p.is_contiguous() and p.device == device) for p in plist))
        if not ok:
            return None
        keep = [_w2(att.qkv), _w2(att.proj), None, None]
        w = BlockWeights(channels=att.dim, eps=block.norm1.eps, q_scale=_Q_PRESCALE,
                         cpe_weight=cpe.conv.weights.data_ptr(), cpe_gamma=cpe.norm.weight.data_ptr(),
                         cpe_beta=cpe.norm.bias.data_ptr(), norm1_gamma=block.norm1.weight.data_ptr(),
                         norm1_beta=block.norm1.bias.data_ptr(), norm2_gamma=block.norm2.weight.data_ptr(),
                         norm2_beta=block.norm2.bias.data_ptr(), qkv_w=keep[0].data_ptr(), proj_w=keep[1].data_ptr(),
                         fc1_w=None, fc2_w=None, mlp_pack=None, qkv_b=att.qkv.bias.data_ptr(),
                         proj_b=att.proj.bias.data_ptr(), fc1_b=mlp.fc1.bias.data_ptr(), fc2_b=mlp.fc2.bias.data_ptr(),
                         rpe_table=None if table is None else table.data_ptr())
        return w, keep
    return derived('native-block', plist, build)


def _native_block_forms(block, x_in, plan: WindowPlan, depth: int):
    """DECIDE: whether the block's inference forward on these rows is a native call (else None: the Python sequence of the same
    kernels runs) and which forms its launches take: (the block's BlockWeights with the forms written in, the cached weight
    images they point to, the expanded RPE table).  Allocates nothing but those cached images."""
    # (xCPE is a full convolution + Linear: not in the native call)
    if not (_NATIVE_BLOCK and _native_rows(block, x_in) and not block.cpe.xcpe):
        return None
    att, mlp, nt, rows = block.attention, block.mlp, plan.n_tokens[depth], x_in.shape[0]
    static = _native_block_static(block, x_in.device) if _attn_f16_ok(rows, att, depth) else None
    if static is None:
        return None
    w, keep = static
    table = None if att.rpe is None else att.rpe.rpe_table
    bnd = int(0.8 * att.patch_size * att.dilation ** 0.5)
    expanded = None if table is None else ops.rpe_expand(table, att.num_heads, bnd, depth, True)
    if table is not None and expanded is None:
        return None
    qpack = _qkv_pack(att, nt)
    w.qkv_pack = None if qpack is None else qpack.data_ptr()
    w.fuse_attention, tables3 = FUSE_ATTN_NO_RELAY, None
    # a relay-token block of this shape takes the one-launch LN1 -> qkv -> window attention (csrc/attn_ws.hip)
    if (qpack is not None and _ATTN_WS and table is not None and rows > nt >= _ATTN_WS_MIN_ROWS and att.dilation == 1
            and att.rt_per_window == 1
            and ops.attn_ws_ok(nt, plan.n_windows[depth], att.patch_size, att.num_heads, depth, att.dim)):
        tables3 = ops.rpe_expand(table, att.num_heads, bnd, depth, 2)
        w.fuse_attention |= FUSE_ATTN_WS
    w.rpe_tables3 = None if tables3 is None else tables3.data_ptr()
    pack = _mlp_pack(mlp, rows)
    if pack is None and keep[2] is None:                # the operands of the three-launch form, on first use
        keep[2], keep[3] = _w2(mlp.fc1), _w2(mlp.fc2)
    w.mlp_pack = None if pack is None else pack.data_ptr()
    w.fc1_w, w.fc2_w = (keep[2].data_ptr(), keep[3].data_ptr()) if pack is None else (None, None)
    return w, (keep, expanded, pack, qpack, tables3), expanded


def _native_block_call(block, x_in, plan: WindowPlan, depth: int):
    """PREPARE: the native call for the block's inference forward (ops.BlockCall) from the decision above, or None when there is
    none.  Same kernels, same order, same results as the Python sequence; only the host work differs."""
    forms = _native_block_forms(block, x_in, plan, depth)
    if forms is None:
        return None
    (w, images, expanded), att, nt = forms, block.attention, plan.n_tokens[depth]
    desc = WindowAttnDesc(n_tokens=nt, rt_row0=nt, n_windows=plan.n_windows[depth], patch_size=att.patch_size,
                          dilation=att.dilation, n_relay=att.rt_per_window, n_heads=att.num_heads,
                          pos_bnd=int(0.8 * att.patch_size * att.dilation ** 0.5), batch_size=plan.B, scale=16 ** -0.5,
                          depth=depth, rpe_expanded=None if expanded is None else expanded.data_ptr())
    return ops.BlockCall(w, images, x_in, plan.neigh(depth), plan.meta[depth], nt, desc)


def _block_body(block, x, plan: WindowPlan, depth: int, with_relay: bool):
    """What OctFormerBlock and HOTFormerBlock do after their CPE heads: x + attention(LN1(x)), then x + mlp(LN2(x)), on the
    first path that applies (the order is the behaviour: the split path is tested before layer scale, and so on down).
    with_relay: x is the [tokens | relay rows] buffer of a HOTFormer level."""
    if _fused_inference(block, x):
        o3 = block.attention.forward_split(x, block.norm1, plan, depth)
        return _block_tail_split(x, o3, block.attention, block.norm2, block.mlp)
    if block.use_layer_scale:
        bid = plan.row_cloud(depth, with_relay=with_relay)
        x = x + block.drop_path(block.gamma1 * block.attention(_ln(x, block.norm1), plan, depth), bid, plan.B)
        return x + block.drop_path(block.gamma2 * block.mlp(_ln(x, block.norm2)), bid, plan.B)
    if block.training and block.drop_path.drop_prob > 0.0:        # stochastic depth: per-row factor inside the branches
        bid = plan.row_cloud(depth, with_relay=with_relay)
        x = block.attention.residual_branch(x, block.norm1, plan, depth, block.drop_path.row_scale(bid, plan.B, x))
        return _mlp_branch(x, block.norm2, block.mlp, block.drop_path.row_scale(bid, plan.B, x))
    if _grad_path(x):
        return _mlp_branch(block.attention.residual_branch(x, block.norm1, plan, depth), block.norm2, block.mlp)
    att = block.attention
    if _x6_path(x, att.qkv, att.proj, block.mlp.fc1, block.mlp.fc2) and x.shape[-1] in ops._LN_CHANNELS:
        o = att.core(att.qkv(_ln(x, block.norm1)), plan, depth)
        return _block_tail_x6(x, o, att.proj, block.norm2, block.mlp)
    x, h = _add_ln(x, block.attention(_ln(x, block.norm1), plan, depth), block.norm2)
    return x + block.mlp(h)


class OctFormerBlock(nn.Module):
    """models/octformer_backbone.py:182-299 (use_rt=False)"""

    def __init__(self, dim, num_heads, patch_size, dilation, disable_RPE=False, conv_norm='layernorm',
                 drop_path=0.0, layer_scale=None, xcpe=False):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.attention = OctreeAttention(dim, patch_size, num_heads, dilation, 0, not disable_RPE)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = MLP(dim, int(dim * 4.0), dim)
        self.drop_path = OctreeDropPath(drop_path)
        self.cpe = CPE(dim, conv_norm, xcpe)
        _init_layer_scale(self, dim, layer_scale)

    def forward(self, x, plan: WindowPlan, depth: int):
        call = _native_block_call(self, x, plan, depth)
        if call is not None:                        # the block as ONE native call (never on the training path)
            return call.run(PHASE_WHOLE)
        x = self.cpe(x, plan, depth, residual=True)
        return _block_body(self, x, plan, depth, with_relay=False)


class OctFormerStage(nn.Module):
    """models/octformer_backbone.py:363-421"""

    def __init__(self, dim, num_heads, patch_size, dilation, num_blocks, disable_RPE=False,
                 conv_norm='layernorm', drop_path=0.0, grad_checkpoint=False, layer_scale=None, xcpe=False):
        super().__init__()
        dp = drop_path if isinstance(drop_path, (list, tuple)) else [drop_path] * num_blocks
        self.grad_checkpoint = grad_checkpoint
        self.blocks = nn.ModuleList([
            OctFormerBlock(dim, num_heads, patch_size, 1 if i % 2 == 0 else dilation, disable_RPE,
                           conv_norm, dp[i], layer_scale, xcpe) for i in range(num_blocks)])

    def forward(self, x, plan, depth):
        ckpt = _use_checkpoint(self, x.shape[0] * x.shape[1], len(self.blocks), x.device)
        for blk in self.blocks:
            # activation checkpointing per block, non-reentrant, as octformer_backbone.py:415-416
            x = _checkpoint_block(blk, x, plan, depth) if ckpt else blk(x, plan, depth)
        return x


class HOTFormerBlock(nn.Module):
    """models/hotformerloc_backbone.py:130-236 (rt_propagation off): operates on the
    [tokens | relay tokens] buffer of one depth."""

    def __init__(self, dim, num_heads, patch_size, disable_RPE=False, conv_norm='layernorm',
                 drop_path=0.0, layer_scale=None, xcpe=False, rt_propagation=False, rt_propagation_scale=None, last=False):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.attention = OctreeAttention(dim, patch_size, num_heads, 1, 1, not disable_RPE)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = MLP(dim, int(dim * 4.0), dim)
        self.drop_path = OctreeDropPath(drop_path)
        self.cpe = CPE(dim, conv_norm, xcpe)
        _init_layer_scale(self, dim, layer_scale)
        # relay-token propagation (hotformerloc_backbone.py:183-193,224-235): the LAST block of a level adds every window's
        # relay token, times a scalar, to the local features of that window
        self.propagate = bool(last and rt_propagation)
        if self.propagate:
            self.upsampler = nn.Upsample(scale_factor=patch_size, mode='nearest')      # parameter-free; kept for the module tree
            self.rt_gamma_propagate = (nn.Parameter(torch.tensor(float(rt_propagation_scale)))
                                       if rt_propagation_scale is not None and type(rt_propagation_scale) in (int, float) else 1)

    def forward(self, buf, plan: WindowPlan, depth: int, relay=None):
        """buf: [tokens | relay rows] of this depth; `relay` (optional): this depth's relay rows as RTSA just produced
        them -- they replace buf's relay rows without a separate copy into buf first."""
        return self._tail(self._forward(buf, plan, depth, relay), plan, depth)

    def _tail(self, out, plan: WindowPlan, depth: int):
        if not self.propagate:
            return out
        # data + gamma * rt[window of the token], zero where the token's cloud is not the window's owner (rt_init_mask,
        # models/octree.py:143-145): a gather over the relay rows, differentiable torch ops (last block of a level only)
        nt = plan.n_tokens[depth]
        win, keep = plan.token_window(depth)
        tok = out[:nt] + self.rt_gamma_propagate * (out[nt:].index_select(0, win) * keep)
        return torch.cat([tok, out[nt:]], 0)

    def _forward(self, buf, plan: WindowPlan, depth: int, relay=None):
        nt = plan.n_tokens[depth]
        if _grad_path(buf):
            c = self.cpe
            if (not c.xcpe and buf.shape[1] in (32, 64, 128, 256) and buf.is_cuda
                    and buf.dtype == torch.float32 and nt > 0):
                # the CPE launch writes the token rows of the new [tokens | relay rows] buffer (no slices, no concatenation)
                buf = ag.cpe_buffer(buf, relay, c.conv.weights, c.norm.weight, c.norm.bias, plan.neigh(depth), nt, c.norm.eps)
            else:
                buf = torch.cat([self.cpe(buf[:nt], plan, depth, residual=True), buf[nt:] if relay is None else relay], 0)
        else:                                   # CPE writes straight into the new buffer's token rows
            call = _native_block_call(self, buf, plan, depth)
            if call is not None:                    # the block as ONE native call
                return call.run(PHASE_WHOLE, relay)
            new = torch.empty_like(buf)
            self.cpe(buf[:nt], plan, depth, residual=True, out=new[:nt])
            new[nt:].copy_(buf[nt:] if relay is None else relay)
            buf = new
        return _block_body(self, buf, plan, depth, with_relay=True)


class RTAttention(nn.Module):
    """models/hotformerloc_backbone.py:56-127"""

    def __init__(self, dim, num_heads):
        super().__init__()
        self.dim, self.num_heads = dim, num_heads
        self.qkv = SplitLinear(dim, dim * 3)
        self.proj = SplitLinear(dim, dim)

    def forward(self, rt, plan: WindowPlan):
        qkv = self.qkv(rt)
        if _grad_path(qkv):
            if plan.max_seq_len <= 611:             # LDS capacity of the HIP backward
                return self.proj(ag.relay_attention(qkv, plan, self.num_heads))
            return self.proj(ag.relay_attention_torch(qkv, plan, self.num_heads))
        out = ops.relay_attention(qkv, plan.seq_rows, plan.seq_off, plan.B, self.num_heads,
                                  plan.max_seq_len)
        return self.proj(out)


class RelayTokenTransformerBlock(nn.Module):
    """models/hotformerloc_backbone.py:239-302 on the concatenated (sum W_d, C) relay rows."""

    def __init__(self, dim, num_heads, drop_path=0.0, layer_scale=None):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.rt_attention = RTAttention(dim, num_heads)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = MLP(dim, int(dim * 4.0), dim)
        self.drop_path = OctreeDropPath(drop_path)
        _init_layer_scale(self, dim, layer_scale)                       # hotformerloc_backbone.py:260-272

    def _native_static(self, device, with_relay_pack: bool):
        """(RelayBlockWeights, tensors it points to) or None, cached and revalidated like _native_block_static.
        `with_relay_pack`: also the weight image of the one-launch block (built only for callers that can use it)."""
        att, mlp = self.rt_attention, self.mlp
        plist = (self.norm1.weight, self.norm1.bias, self.norm2.weight, self.norm2.bias, att.qkv.bias, att.proj.bias,
                 mlp.fc1.bias, mlp.fc2.bias, att.qkv.weight, att.proj.weight, mlp.fc1.weight, mlp.fc2.weight)

        def build():
            if not (all(p is not None and p.dtype == torch.float32 and p.is_contiguous() and p.device == device for p in plist)
                    and self.norm1.eps == self.norm2.eps and att.dim % 128 == 0 and att.num_heads * 16 == att.dim):
                return None
            # (the MLP branch as the fused launch with the hidden dimension split over the chip: 27 us against 48 us for the
            # three launches alone, and inside the step the relay tokens' fc2 -- K = 1024 over 28 workgroups -- took 120 us:
            # 2361 -> 2417 clouds/s, three alternating runs each)
            mpack = _mlp_pack(mlp, _MLP_FUSED_MIN_ROWS)
            # (LN1 -> qkv as one launch and the attention writing proj's operand: six launches -> three, see forward)
            qpack = _qkv_pack(att, _QKV_FUSED_MIN_ROWS)
            # (the whole block as one launch: csrc/relay_block.hip)
            rpack = _relay_pack(att, mlp) if with_relay_pack else None
            keep = (_w2(att.qkv), _w2(att.proj), _w2(mlp.fc1), _w2(mlp.fc2), mpack, qpack, rpack)
            w = RelayBlockWeights(channels=att.dim, n_heads=att.num_heads, eps=self.norm1.eps,
                                  mlp_pack=None if mpack is None else mpack.data_ptr(),
                                  qkv_pack=None if qpack is None else qpack.data_ptr(),
                                  relay_pack=None if rpack is None else rpack.data_ptr(),
                                  norm1_gamma=self.norm1.weight.data_ptr(), norm1_beta=self.norm1.bias.data_ptr(),
                                  norm2_gamma=self.norm2.weight.data_ptr(), norm2_beta=self.norm2.bias.data_ptr(),
                                  qkv_w=keep[0].data_ptr(), proj_w=keep[1].data_ptr(), fc1_w=keep[2].data_ptr(),
                                  fc2_w=keep[3].data_ptr(), qkv_b=att.qkv.bias.data_ptr(), proj_b=att.proj.bias.data_ptr(),
                                  fc1_b=mlp.fc1.bias.data_ptr(), fc2_b=mlp.fc2.bias.data_ptr())
            return w, keep
        return derived(('native-relay', with_relay_pack), plist, build)

    def _native_route(self, rows, plan):
        """The native and one-launch routes of the inference forward on the (n, C) relay rows, or on the list of tensors whose
        concatenation they are (hfl_relay_block_io.x_segments); None: the Python launch sequence of `forward` runs.
        With `_native_rows`, non-empty rows (the kernels take no empty launch) and qualifying parameters:
            _NATIVE_BLOCK on                                    ops.relay_block_forward_x3(..., fused=_RELAY_FUSED)
            _NATIVE_BLOCK off, one launch wanted and accepted   that single launch (the same one, whoever issues it)
            otherwise                                           None"""
        parts = rows if isinstance(rows, list) else (rows,)
        fused = _RELAY_FUSED and plan.max_seq_len <= 64  # wanted, and a batch it takes (hfl_relay_block_fused_ok's length rule)
        if not ((_NATIVE_BLOCK or fused) and all(p.shape[0] > 0 and _native_rows(self, p) for p in parts)):
            return None
        static = self._native_static(parts[0].device, fused)
        # (the row-segment table is read by the fused LN1 -> qkv launch and by proj's residual)
        if static is None or (parts is rows and not static[0].qkv_pack):
            return None
        args = (static[0], static[1], rows, plan.seq_rows, plan.seq_off, plan.B, plan.max_seq_len, plan.orphan_rows)
        if _NATIVE_BLOCK:
            return ops.relay_block_forward_x3(*args, fused=_RELAY_FUSED)
        return ops.relay_block_fused_x3(*args)              # None where hfl_relay_block_fused_ok refuses the problem

    def forward_parts(self, parts, plan):
        """forward(torch.cat(parts)), without the concatenation launch where the native call reads the rows in place (<= 4)"""
        out = self._native_route(list(parts), plan) if _NATIVE_BLOCK and len(parts) <= 4 else None
        return self(torch.cat(list(parts), 0), plan) if out is None else out

    def forward(self, rt, plan):
        att, out = self.rt_attention, self._native_route(rt, plan)
        if out is not None:
            return out
        # (the launch sequence below is made of the 'x3' kernels, which take no empty launch)
        if _fused_inference(self, rt) and _GEMM_MODE == 'x3' and rt.shape[0] > 0:
            # LN1 -> qkv as ONE launch (csrc/qkv_fused.hip, output features split over the chip for the ~2 k rows) and the
            # ragged attention reading its fp16 (hi, lo) rows and writing attention.proj's split2 operand itself
            # (hfl_relay_attention_f16_fwd): LayerNorm, qkv GEMM, memset, attention, split2 -> two launches.  The block is a
            # chain of tiny launches on the cycle every H-OSA iteration waits for.
            qpack = _qkv_pack(att, _QKV_FUSED_MIN_ROWS)
            if qpack is not None:
                qkv = ops.ln_qkv_fused(rt, self.norm1.weight, self.norm1.bias, self.norm1.eps, qpack, att.qkv.bias, _Q_PRESCALE)
                o2 = ops.relay_attention_f16(qkv, plan.seq_rows, plan.seq_off, plan.B, att.num_heads, plan.max_seq_len,
                                             plan.orphan_rows)
            else:
                a2 = ops.layer_norm_split2(rt, self.norm1.weight, self.norm1.bias, self.norm1.eps)
                qkv = ops.linear_x3(a2, _w2(att.qkv), bias=att.qkv.bias)
                o2 = ops.split2(ops.relay_attention(qkv, plan.seq_rows, plan.seq_off, plan.B, att.num_heads, plan.max_seq_len))
            return _block_tail_x3(rt, o2, att, self.norm2, self.mlp, fused_any_rows=True)
        if self.use_layer_scale or (self.training and self.drop_path.drop_prob > 0.0):
            bid = plan.relay_cloud()
            rt = rt + self.drop_path(self.gamma1 * self.rt_attention(_ln(rt, self.norm1), plan), bid, plan.B)
            return rt + self.drop_path(self.gamma2 * self.mlp(_ln(rt, self.norm2)), bid, plan.B)
        if _x6_path(rt, att.qkv, att.proj, self.mlp.fc1, self.mlp.fc2) and rt.shape[-1] in ops._LN_CHANNELS:
            o = ops.relay_attention(att.qkv(_ln(rt, self.norm1)), plan.seq_rows, plan.seq_off, plan.B, att.num_heads,
                                    plan.max_seq_len)
            return _block_tail_x6(rt, o, att.proj, self.norm2, self.mlp)
        rt, h = _add_ln(rt, self.rt_attention(_ln(rt, self.norm1), plan), self.norm2)
        return rt + self.mlp(h)


class RelayTokenInitialiser(nn.Module):
    """models/hotformerloc_backbone.py:305-363"""

    def __init__(self, dim, patch_size, conv_norm='layernorm', use_cpe=False, xcpe=False):
        super().__init__()
        self.patch_size = patch_size
        self.use_cpe = use_cpe
        if use_cpe:
            self.cpe = CPE(dim, conv_norm, xcpe)

    def forward(self, x, plan: WindowPlan, depth: int):
        if self.use_cpe:
            x = self.cpe(x, plan, depth, residual=False)
        if _grad_path(x):
            return ag.relay_token_init(x, plan.meta[depth], plan.n_windows[depth], self.patch_size)
        return ops.relay_token_init(x, plan.meta[depth], plan.n_windows[depth], self.patch_size)


class ADaPE(nn.Module):
    """models/layers/octformer_layers.py:177-210"""

    def __init__(self, dim, mode='cov'):
        super().__init__()
        self.mlp = MLP({'pos': 3, 'var': 6, 'cov': 9}[mode], dim, dim)

    def forward(self, plan: WindowPlan, depth: int):
        return self.mlp(plan.window_stats[depth])


class _PyramidLevels:
    """What a HOTFormerStage forward carries from H-OSA iteration to iteration, per pyramid level j (depth depths[j]): the token
    counts `nts`, the [tokens | relay] buffers `bufs[d]`, the relay rows as RTSA sees them `rts[d]` (each level's own rows or,
    with per-level widths, their projection to the widest level), whether the blocks are checkpointed, and which levels are
    `small`: the ones that run on side streams.  The early schedule adds its streams, calls and outputs (`_run_early`)."""

    def __init__(self, stage, plan: WindowPlan, depths, bufs, ckpt: bool):
        self.stage, self.plan, self.depths, self.bufs, self.ckpt = stage, plan, depths, bufs, ckpt
        self.proj = stage.use_projections
        self.nts = [plan.n_tokens[d] for d in depths]
        self.rts = {d: (stage.init_up_projections[j](bufs[d][nt:]) if self.proj else bufs[d][nt:])          # 585-591
                    for j, (d, nt) in enumerate(zip(depths, self.nts))}
        self.small = [j > 0 and bufs[d].shape[0] <= _SIDE_STREAM_MAX_ROWS for j, d in enumerate(depths)]

    def rtsa(self, i):
        """RTSA of iteration i over all levels' relay rows: (its rows, the fresh relay rows of every depth)"""
        blk, parts = self.stage.rtsa_blocks[i], [self.rts[d] for d in self.depths]
        rt_all = _checkpoint_block(blk, torch.cat(parts, 0), self.plan) if self.ckpt else blk.forward_parts(parts, self.plan)
        off, nw = self.plan.rt_offset, self.plan.n_windows                      # 596-601
        return rt_all, {d: rt_all[off[d]:off[d] + nw[d]] for d in self.depths}

    def relay_in(self, j, i, fresh_d):
        """a level's fresh relay rows at the level's own width (the down-projection of per-level-width configurations)"""
        return self.stage.down_projections[j][i](fresh_d) if self.proj else fresh_d

    def hand_over(self, j, i, out):
        """block i's output becomes level j's buffer, its relay rows (up-projected) what RTSA i + 1 reads"""
        d, relay = self.depths[j], out[self.nts[j]:]
        self.bufs[d], self.rts[d] = out, (self.stage.up_projections[j][i](relay) if self.proj else relay)

    def hosa(self, j, i, fresh_d):
        """down-projection -> H-OSA block -> up-projection of one level (610-630)"""
        blk, d, rin = self.stage.hosa_blocks[j][i], self.depths[j], self.relay_in(j, i, fresh_d)
        out = _checkpoint_block(blk, self.bufs[d], self.plan, d, rin) if self.ckpt else blk(self.bufs[d], self.plan, d, rin)
        self.hand_over(j, i, out)


class HOTFormerStage(nn.Module):
    """models/hotformerloc_backbone.py:366-635: one channel width for all pyramid levels (shipped configs), or one per level
    with linear projections between each level's width and the relay-token width (the widest level)."""

    def __init__(self, channels, num_heads, num_blocks, num_pyramid_levels, patch_size,
                 disable_RPE=False, ADaPE_mode=None, conv_norm='layernorm', drop_path=0.0, grad_checkpoint=False,
                 dilation=4, disable_rt=False, layer_scale=None, xcpe=False, rt_propagation=False,
                 rt_propagation_scale=None):
        super().__init__()
        self.grad_checkpoint = grad_checkpoint
        self.disable_rt = disable_rt
        channels, num_heads = list(channels), list(num_heads)
        self.use_projections = len(channels) != 1 and not disable_rt          # :384-400
        if len(channels) == 1:
            channels = channels * num_pyramid_levels
        if len(num_heads) == 1:
            num_heads = num_heads * num_pyramid_levels
        assert len(channels) == num_pyramid_levels, 'Invalid num channels specified'
        assert len(num_heads) == num_pyramid_levels, 'Invalid num heads specified'
        self.channels, self.num_heads = channels, num_heads
        Cm = self.max_rt_channels = max(channels)
        Hm = self.max_rt_num_heads = num_heads[channels.index(Cm)]
        self.num_pyramid_levels, self.num_blocks = num_pyramid_levels, num_blocks
        self.use_ADaPE = ADaPE_mode is not None
        dp = drop_path if isinstance(drop_path, (list, tuple)) else [drop_path] * num_blocks
        L = num_pyramid_levels
        if disable_rt:
            # ablation without relay tokens (hotformerloc_backbone.py:396-397,440-458,477): plain local-attention
            # blocks with the dilation re-enabled, no RTSA, no relay-token initialiser
            self.hosa_blocks = nn.ModuleList([
                nn.ModuleList([OctFormerBlock(channels[j], num_heads[j], patch_size, 1 if i % 2 == 0 else dilation,
                                              disable_RPE, conv_norm, dp[i], layer_scale, xcpe)
                               for i in range(num_blocks)]) for j in range(L)])
        else:
            self.hosa_blocks = nn.ModuleList([
                nn.ModuleList([HOTFormerBlock(channels[j], num_heads[j], patch_size, disable_RPE, conv_norm, dp[i],
                                              layer_scale, xcpe, rt_propagation, rt_propagation_scale,
                                              last=(i == num_blocks - 1))
                               for i in range(num_blocks)]) for j in range(L)])
            if self.use_projections:                                          # :406-408,461-475 (registration order)
                self.up_projections = nn.ModuleList([
                    nn.ModuleList([nn.Linear(channels[j], Cm) for _ in range(num_blocks)]) for j in range(L)])
                self.down_projections = nn.ModuleList([
                    nn.ModuleList([nn.Linear(Cm, channels[j]) for _ in range(num_blocks)]) for j in range(L)])
                self.init_up_projections = nn.ModuleList([nn.Linear(channels[j], Cm) for j in range(L)])
            self.rtsa_blocks = nn.ModuleList([RelayTokenTransformerBlock(Cm, Hm, dp[i], layer_scale)
                                              for i in range(num_blocks)])
            if self.use_projections:
                self.relay_tokeniser = nn.ModuleList([
                    RelayTokenInitialiser(channels[j], patch_size, conv_norm, use_cpe=not self.use_ADaPE, xcpe=xcpe)
                    for j in range(L)])
            else:
                self.relay_tokeniser = RelayTokenInitialiser(Cm, patch_size, conv_norm,
                                                             use_cpe=not self.use_ADaPE, xcpe=xcpe)
            if self.use_ADaPE:
                self.rt_adape = ADaPE(Cm, ADaPE_mode)
                if self.use_projections:
                    self.rt_adape_projections = nn.ModuleList([nn.Linear(Cm, channels[j]) for j in range(L)])
        self.downsamples = nn.ModuleList([Downsample(channels[j], channels[j + 1], conv_norm)
                                          for j in range(L - 1)])

    def _streams(self, device):
        """(side streams of the coarser levels, RTSA's stream), made on first use (`ema._DERIVED_STATE`: not part of a copy)"""
        made = self.__dict__.get('_stream_cache')
        if made is None:
            side = [torch.cuda.Stream(device=device) for _ in range(self.num_pyramid_levels - 1)]
            # high priority: RTSA is a chain of eight tiny launches that must slip in between the chip-filling kernels of the
            # token-row phase; at equal priority each of them queues behind a full round of workgroups
            made = self.__dict__['_stream_cache'] = (side, torch.cuda.Stream(device=device, priority=-1))
        return made

    def _forward_without_relay_tokens(self, data, plan: WindowPlan, depths):
        feats = {depths[0]: data}
        for j, d in enumerate(depths[:-1]):
            feats[d - 1] = self.downsamples[j](feats[d], plan.octree, d)
        ckpt = _use_checkpoint(self, sum(f.shape[0] * f.shape[1] for f in feats.values()), self.num_blocks, data.device)
        for i in range(self.num_blocks):
            for j, d in enumerate(depths):
                blk = self.hosa_blocks[j][i]
                feats[d] = _checkpoint_block(blk, feats[d], plan, d) if ckpt else blk(feats[d], plan, d)
        return feats, {d: None for d in depths}

    def forward(self, data, plan: WindowPlan, depth: int):
        depths = [depth - j for j in range(self.num_pyramid_levels)]
        if self.disable_rt:
            return self._forward_without_relay_tokens(data, plan, depths)
        feats = {depths[0]: data}
        bufs: Dict[int, torch.Tensor] = {}
        proj = self.use_projections
        for j, d in enumerate(depths):                                  # init_pyramid_feats, 540-572
            tokeniser = self.relay_tokeniser[j] if proj else self.relay_tokeniser
            rt = tokeniser(feats[d], plan, d)
            if self.use_ADaPE:
                pe = self.rt_adape(plan, d)
                rt = rt + (self.rt_adape_projections[j](pe) if proj else pe)
            bufs[d] = torch.cat([feats[d], rt], 0)
            if j < self.num_pyramid_levels - 1:
                feats[d - 1] = self.downsamples[j](feats[d], plan.octree, d)
        ckpt = _use_checkpoint(self, sum(b.shape[0] * b.shape[1] for b in bufs.values()), self.num_blocks, data.device)
        st = _PyramidLevels(self, plan, depths, bufs, ckpt)
        getattr(self, '_run_' + self._schedule(bufs[depths[0]], plan, depths[0], ckpt))(st)               # 593-633
        return {d: st.bufs[d][:nt] for d, nt in zip(depths, st.nts)}, st.rts

    def _schedule(self, buf, plan: WindowPlan, depth: int, ckpt: bool) -> str:
        """Which schedule the H-OSA iterations of this forward run on ('early' | 'forked' | 'sequential'; the same kernels on
        the same rows in each).  buf: the finest level's [tokens | relay] buffer, depth: its depth."""
        streams = _PYRAMID_STREAMS and not _grad_path(buf) and buf.is_cuda
        if _EARLY_PHASE and streams and not ckpt:
            # The finest level's LN1 -> qkv -> window attention is ONE launch there (csrc/attn_ws.hip) and needs the relay
            # rows: nothing but its CPE could run beside the relay-token block, and the persistent launch starves the coarse
            # levels' early phases.  RTSA first, then the levels side by side: +2-4 % on three boxes
            # (profiles/r05_w_ab_attn_ws_default.log); with the early phases kept the one-launch form gains nothing.
            if _ATTN_WS_EARLY or not self._finest_level_fuses_attention(buf, plan, depth):
                return 'early'
        return 'forked' if streams and not _SERIAL_STREAMS else 'sequential'

    def _finest_level_fuses_attention(self, buf, plan: WindowPlan, depth: int) -> bool:
        """The native call of the finest level's blocks takes the one-launch LN1 -> qkv -> window attention branch."""
        forms = _native_block_forms(self.hosa_blocks[0][0], buf, plan, depth)
        return forms is not None and bool(forms[0].fuse_attention & FUSE_ATTN_WS)

    def _run_sequential(self, st: _PyramidLevels):
        """RTSA, then the levels one after the other, all on the current stream."""
        for i in range(self.num_blocks):
            _, fresh = st.rtsa(i)
            for j, d in enumerate(st.depths):
                st.hosa(j, i, fresh[d])

    def _run_forked(self, st: _PyramidLevels):
        """RTSA, then the levels side by side: the three depths are independent inside an iteration (the reference runs them on
        three CUDA streams too, hotformerloc_backbone.py:604-633): the coarse depths' small GEMMs and kernels overlap the fine
        depth's.  Fork/join discipline: side streams wait for the main stream's event, the main stream waits for theirs.
        Only SMALL depths go to a side stream (_SIDE_STREAM_MAX_ROWS): they are the ones that cannot fill 256 CUs, and
        hipBLASLt's stream-K GEMMs (workgroups that wait on their peers' partial tiles) dead-lock when several chip-filling
        ones share the CUs."""
        main = torch.cuda.current_stream()
        side = self._streams(st.bufs[st.depths[0]].device)[0]
        forked = [j for j, small in enumerate(st.small) if small]
        for i in range(self.num_blocks):
            rt_all, fresh = st.rtsa(i)
            keep = [(st.bufs[st.depths[j]], rt_all) for j in forked]   # inputs allocated on the main stream live until the join
            for j in forked:
                side[j - 1].wait_stream(main)
                with torch.cuda.stream(side[j - 1]):
                    st.hosa(j, i, fresh[st.depths[j]])
            for j, d in enumerate(st.depths):
                if j not in forked:
                    st.hosa(j, i, fresh[d])
            for j in forked:
                main.wait_stream(side[j - 1])
            del keep

    def _run_early(self, st: _PyramidLevels):
        """RTSA of iteration i only feeds the relay rows: what a block does with its TOKEN rows before the window attention (CPE,
        LN1, qkv projection: a third of the block) does not wait for it.  Every level issues that part on its own stream first,
        RTSA runs beside it on a stream of its own, the rest of the block follows once both are done -- the ~120 us chain of
        eight tiny RTSA launches leaves the critical path.
        Who waits for whom.  A level's block i needs that level's block i - 1 (stream order) and, for its relay rows, RTSA i;
        RTSA i needs every level's block i - 1.  Nothing else: in particular the finest level's CPE / LN1 / qkv of iteration i
        do not wait for the coarse levels' MLP launches of iteration i - 1, which run (starved) beside and after the finest
        level's chip-filling fused MLP -- with a join of all streams at the end of every iteration (the schedule of rounds 2-3,
        since removed) the finest level's queue stood idle ~80 us per iteration there (kernel trace,
        profiles/r04_phases_iteration_timeline_join.log)."""
        st.main = main = torch.cuda.current_stream()
        side, st.rs = ([main] * len(st.small), main) if _SERIAL_STREAMS else self._streams(st.bufs[st.depths[0]].device)
        st.sts = [side[j - 1] if small else main for j, small in enumerate(st.small)]
        # issue order = critical path first (the host runs only just ahead of the GPU): finest level's token phase, RTSA, the rest
        st.order = sorted(range(len(st.small)), key=lambda j: -st.bufs[st.depths[j]].shape[0])
        done = None          # per-stream end-of-iteration events of the previous iteration
        first = (dict(st.bufs), dict(st.rts))    # the buffers the schedule started from (allocated on main, read by the others)
        for i in range(self.num_blocks):
            ev0 = main.record_event() if done is None else None         # first iteration: everybody joins the main stream
            st.calls, st.outs = {}, {}
            self._token_phase(st, i, st.order[0], ev0)
            for ev in ([ev0] if done is None else done):                # RTSA i, beside it: after every level's block i - 1
                st.rs.wait_event(ev)
            with torch.cuda.stream(st.rs):
                rt_all, fresh = st.rtsa(i)
                ev_rt = st.rs.record_event()
            for j in st.order[1:]:
                self._token_phase(st, i, j, ev0)
            old = (dict(st.bufs), dict(st.rts))        # buffers other streams still read stay alive until the join
            # The levels on SIDE streams (the small ones: 2 k and 14 k rows in the bench) send their window attention out as
            # ONE launch: their windows are one or two per workgroup, latency-bound launches of 14 and 21 us alone.  The
            # join is between those side streams only.  (Measured alternatives: all three levels in one launch joined
            # on the main stream -3.5 % of the step; the small levels back to back on one side stream -3 %.)
            # (blocks on the one-launch LN1 -> qkv -> attention path have no separate attention launch to merge)
            group = [j for j in st.order if st.small[j] and st.calls[st.depths[j]] is not None
                     and not st.calls[st.depths[j]].weights.fuse_attention & FUSE_ATTN_WS] if _MERGED_ATTN else []
            group = group if len(group) >= 2 else []
            self._relay_phase(st, i, fresh, ev_rt, group)
            if group:
                self._tails(st, i, group, self._merged_attention(st, group))
            done = self._hand_over(st, i)
            del old, fresh, rt_all, st.calls, st.outs

    def _token_phase(self, st, i, j, ev0):
        """level j's token-row half of block i (PHASE_TOKENS) on the level's stream"""
        d = st.depths[j]
        if ev0 is not None and st.sts[j] is not st.main:
            st.sts[j].wait_event(ev0)
        with torch.cuda.stream(st.sts[j]):
            call = st.calls[d] = _native_block_call(self.hosa_blocks[j][i], st.bufs[d], st.plan, d)
            if call is not None:
                call.run(PHASE_TOKENS)

    def _relay_phase(self, st, i, fresh, ev_rt, group):
        """after RTSA i: every level's relay rows in and the rest of its block (the `group`'s levels: up to the attention)"""
        for j in st.order:
            d, blk = st.depths[j], self.hosa_blocks[j][i]
            st.sts[j].wait_event(ev_rt)
            with torch.cuda.stream(st.sts[j]):
                rin = st.relay_in(j, i, fresh[d])
                if j in group:
                    st.calls[d].run(PHASE_RELAY_QKV, rin)                     # relay rows in, their LN1 / qkv
                elif st.calls[d] is not None:
                    st.outs[j] = blk._tail(st.calls[d].run(PHASE_REST, rin), st.plan, d)
                else:
                    st.outs[j] = blk(st.bufs[d], st.plan, d, rin)

    def _merged_attention(self, st, group):
        """the window attention of the group's levels as one launch on the first one's stream; the event after it"""
        lead = st.sts[group[0]]
        for j in group[1:]:
            lead.wait_event(st.sts[j].record_event())
        with torch.cuda.stream(lead):
            ops.block_attention_multi([st.calls[st.depths[j]] for j in group])
            return lead.record_event()

    def _tails(self, st, i, group, ev_att):
        """what follows the merged attention, every level on its own stream again"""
        for j in group:
            d = st.depths[j]
            if st.sts[j] is not st.sts[group[0]]:
                st.sts[j].wait_event(ev_att)
            with torch.cuda.stream(st.sts[j]):
                st.outs[j] = self.hosa_blocks[j][i]._tail(st.calls[d].run(PHASE_TAIL), st.plan, d)      # proj + MLP

    def _hand_over(self, st, i):
        """the outputs become iteration i + 1's inputs; the per-stream events it waits for (last: main joins instead)"""
        for j in st.order:
            with torch.cuda.stream(st.sts[j]):
                st.hand_over(j, i, st.outs[j])
        if i + 1 < self.num_blocks:
            return [s.record_event() for s in dict.fromkeys(st.sts)]
        for s in (s for s in st.sts if s is not st.main):
            st.main.wait_stream(s)


class HOTFormerBase(nn.Module):
    """models/hotformerloc_backbone.py:638-723"""

    def __init__(self, in_channels, channels, num_blocks, num_heads, num_pyramid_levels,
                 num_octf_levels, patch_size, dilation, stem_down, ADaPE_mode, disable_RPE, conv_norm,
                 drop_path=0.0, grad_checkpoint=False, disable_rt=False, layer_scale=None, xcpe=False,
                 rt_propagation=False, rt_propagation_scale=None, downsample_input_embeddings=True):
        super().__init__()
        self.downsample_input_embeddings = downsample_input_embeddings
        # stochastic depth per block (hotformerloc_backbone.py:669-700)
        drop_ratio = torch.linspace(0, drop_path, sum(num_blocks)).tolist()
        self.patch_size, self.dilation = patch_size, dilation
        self.num_pyramid_levels, self.num_octf_levels = num_pyramid_levels, num_octf_levels
        self.num_stages = num_octf_levels + num_pyramid_levels
        self.stem_down = stem_down
        self.ADaPE_mode = ADaPE_mode
        if num_heads is None:
            num_heads = [c // 16 for c in channels]
        self.patch_embed = PatchEmbed(in_channels, channels[0], stem_down, conv_norm, downsample_input_embeddings)
        self.octf_stage = nn.ModuleList([
            OctFormerStage(channels[i], num_heads[i], patch_size, dilation, num_blocks[i], disable_RPE,
                           conv_norm, drop_ratio[sum(num_blocks[:i]):sum(num_blocks[:i + 1])], grad_checkpoint,
                           layer_scale, xcpe)
            for i in range(num_octf_levels)])
        self.downsample = nn.ModuleList([Downsample(channels[i], channels[i + 1], conv_norm)
                                         for i in range(num_octf_levels)])
        self.hotf_stage = HOTFormerStage(list(channels[num_octf_levels:]),
                                         list(num_heads[num_octf_levels:]), num_blocks[-1],
                                         num_pyramid_levels, patch_size, disable_RPE, ADaPE_mode,
                                         conv_norm, drop_ratio[sum(num_blocks[:-1]):sum(num_blocks)],
                                         grad_checkpoint, dilation, disable_rt, layer_scale, xcpe, rt_propagation,
                                         rt_propagation_scale)

    def forward(self, data, octree, depth):
        # the plan depends on the octree only: built first, so that its host work hides the round trip of the tap counts
        # that `construct_all_neigh()` started (the stem convolutions below are the first to need them)
        top = depth - self.stem_down if self.downsample_input_embeddings else depth         # :707-708

        def make_plan():
            return WindowPlan.for_octree(octree, self.patch_size, self.dilation, max_depth=top,
                                         start_depth=top - self.num_stages + 1,
                                         num_pyramid_levels=self.num_pyramid_levels,
                                         num_octf_levels=self.num_octf_levels, adape_mode=self.ADaPE_mode)

        if not _grad_path() and data.is_cuda:
            # inference: the stem first (it only needs the tap lists, whose counts the host has to wait for anyway), THEN the
            # plan: its ~0.25 ms of host work runs while the GPU executes the stem's 0.7 ms instead of in front of it with
            # the GPU idle (kernel trace of a step's first millisecond, profiles/r04_phases_stem_head_end_of_round.log)
            data = self.patch_embed(data, octree, depth)
            plan = make_plan()
        else:
            plan = make_plan()
            data = self.patch_embed(data, octree, depth)
        depth = top
        for i in range(self.num_octf_levels):
            data = self.octf_stage[i](data, plan, depth)
            data = self.downsample[i](data, octree, depth)
            depth -= 1
        local, relay = self.hotf_stage(data, plan, depth)
        return local, relay, plan


class HOTFormer(nn.Module):
    """models/hotformerloc_backbone.py:726-849 (init: 817-843)"""

    def __init__(self, in_channels, channels, num_blocks, num_heads, num_pyramid_levels=3,
                 num_octf_levels=1, patch_size=32, dilation=4, drop_path=0.5, stem_down=2,
                 ADaPE_mode=None, disable_RPE=False, conv_norm='layernorm',
                 qkv_init=('trunc_normal', 0.02), grad_checkpoint=False, disable_rt=False, layer_scale=None,
                 xcpe=False, rt_size=1, rt_propagation=False, rt_propagation_scale=None,
                 downsample_input_embeddings=True):
        super().__init__()
        if rt_size != 1:
            # the reference's own model cannot run this option: RelayTokenInitialiser views the windows as (-1, K // G, C)
            # against a (windows, K) mask and raises (models/hotformerloc_backbone.py:354-357, "TODO: Make this work with
            # rt_size > 1"); tests/test_variants.py::test_ct_size_other_than_one_is_rejected_like_the_reference
            raise NotImplementedError('ct_size != 1: the reference model itself fails on it '
                                      '(models/hotformerloc_backbone.py:354-357)')
        self.backbone = HOTFormerBase(in_channels, list(channels), list(num_blocks),
                                      None if num_heads is None else list(num_heads),
                                      num_pyramid_levels, num_octf_levels, patch_size, dilation,
                                      stem_down, ADaPE_mode, disable_RPE, conv_norm, drop_path, grad_checkpoint,
                                      disable_rt, layer_scale, xcpe, rt_propagation, rt_propagation_scale,
                                      downsample_input_embeddings)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        if qkv_init[0] == 'trunc_normal':
            for name, m in self.named_modules():
                if 'qkv' in name and isinstance(m, nn.Linear):
                    nn.init.trunc_normal_(m.weight, std=qkv_init[1])

    def forward(self, data, octree, depth):
        return self.backbone(data, octree, depth)


# -------------------------------------------------------------------------- pooling
class AdaptivePooling(nn.Module):
    """models/layers/salsa.py:12-55: learned queries attend over one cloud's tokens."""

    def __init__(self, feature_dim, k_pooled_tokens):
        super().__init__()
        self.query = nn.Parameter(torch.randn(k_pooled_tokens, feature_dim))
        self.scale = feature_dim ** -0.5

    def forward(self, x, plan: WindowPlan, depth: int, out=None):
        """x (N_t, C) ragged over clouds -> (B, k, C) (`out`: where to, e.g. this level's slice of the token matrix)."""
        if _grad_path(x):
            return ag.attentional_pooling_torch(x, self.query, plan, depth, self.scale)
        if _GEMM_MODE == 'x3' and _split_path(x) and x.dtype == torch.float32 and ops.attn_pool_ok(x.shape[1]):
            # scores -> softmax over the cloud's rows -> weighted sum in one launch, nothing padded (csrc/attn_pool.hip; was GEMM
            # + segment softmax + two padding copies + batched GEMM)
            return ops.attn_pool(x, plan.cloud_off[depth], self.query, plan.B, self.scale, out=out)
        scores = torch.mm(x, self.query.t())                              # (N_t, k)
        ops.segment_softmax_(scores, plan.cloud_off[depth], plan.B, self.scale)
        nmax = plan.pad_index[depth].numel() // plan.B
        if scores.shape[1] % 4 == 0:                     # per-cloud zero-padded copies in one pass each (hfl_pad_rows)
            xp = ops.pad_rows(x, plan.cloud_off[depth], plan.B, nmax)
            pp = ops.pad_rows(scores, plan.cloud_off[depth], plan.B, nmax)
        else:
            idx = plan.pad_index[depth]
            zero = x.new_zeros(1, x.shape[1])
            xp = torch.cat([x, zero], 0).index_select(0, idx).view(plan.B, -1, x.shape[1])
            pp = torch.cat([scores, scores.new_zeros(1, scores.shape[1])], 0) \
                .index_select(0, idx).view(plan.B, -1, scores.shape[1])
        return torch.bmm(pp.transpose(1, 2), xp)


class FeatureMixerLayer(nn.Module):
    """models/layers/salsa.py:58-75"""

    def __init__(self, in_dim, mlp_ratio=1):
        super().__init__()
        self.mix = nn.Sequential(nn.LayerNorm(in_dim), nn.Linear(in_dim, int(in_dim * mlp_ratio)),
                                 nn.GELU(), nn.Linear(int(in_dim * mlp_ratio), in_dim))
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)

    def forward(self, x):
        return x + self.mix(x)


def _mixer_pack(fc1: nn.Linear, fc2: nn.Linear):
    """`ops.mlp_fused_pack` image of a Mixer layer's two Linears, cached per parameter pair like `_mlp_pack`."""
    w1, w2 = fc1.weight, fc2.weight
    return derived('mixer', (w1, w2), lambda: ops.mlp_fused_pack(w1, w2))


def _mixer_chain_pack(layers):
    """`ops.mixer_chain_pack` image of all FeatureMixerLayers' Linears, cached per parameter set like `_mixer_pack`."""
    w1s, w2s = [m.mix[1].weight for m in layers], [m.mix[3].weight for m in layers]
    return derived('mixerchain', (*w1s, *w2s), lambda: ops.mixer_chain_pack(w1s, w2s))


def _mixer_layer_fits(m) -> bool:
    ln, fc1, act, fc2 = m.mix
    return (isinstance(ln, nn.LayerNorm) and isinstance(act, nn.GELU) and fc1.in_features % 128 == 0
            and fc1.out_features % 128 == 0 and fc2.out_features % 128 == 0 and fc1.bias is not None and fc2.bias is not None)


class Mixer(nn.Module):
    """models/layers/salsa.py:78-111"""

    def __init__(self, k_input_tokens, k_output_tokens, in_d, mix_depth, mlp_ratio, out_d):
        super().__init__()
        self.mix = nn.Sequential(*[FeatureMixerLayer(in_d, mlp_ratio) for _ in range(mix_depth)])
        self.row_proj = nn.Linear(in_d, out_d)
        self.channel_proj = nn.Linear(k_input_tokens, k_output_tokens)

    def _tail_fits(self, x) -> bool:
        """the inference conditions of `ops.mixer_tail` (and of `ops.descriptor_tail`)"""
        return (_GEMM_MODE == 'x3' and x.is_cuda and not _grad_path() and x.dtype == torch.float32
                and x.shape[-1] % 4 == 0 and self.row_proj.out_features <= 8 and self.channel_proj.bias is not None
                and self.row_proj.bias is not None and x.shape[1] * self.row_proj.out_features <= 16000)

    def chain_shapes_ok(self) -> bool:
        """the part of the one-launch rule that depends on the module alone: hfl_mixer_chain_ok on its widths and depth, one
        LayerNorm eps for all layers"""
        if len(self.mix) == 0 or not all(_mixer_layer_fits(m) for m in self.mix):
            return False
        c, hidden = self.row_proj.in_features, self.mix[0].mix[1].out_features
        return (all(m.mix[1].in_features == c and m.mix[1].out_features == hidden and m.mix[3].out_features == c
                    and m.mix[0].eps == self.mix[0].mix[0].eps for m in self.mix)
                and ops.mixer_chain_ok(c, hidden, len(self.mix), self.row_proj.out_features))

    def forward(self, x, normalize=False):
        """(B, k_out * out_d) descriptors; `normalize`: L2-normalised rows (the wrapper's `normalize_embeddings`)"""
        if (_MIXER_CHAIN and _GEMM_MODE == 'x3' and _split_path(x) and x.dtype == torch.float32 and self._tail_fits(x)
                and ops.mlp_fused_shape_ok(x.shape[-1], self.mix[0].mix[1].out_features if len(self.mix) else 0)
                and (x.shape[1] + self.channel_proj.out_features + 1) * self.row_proj.out_features < 16384   # the tail's LDS
                and self.chain_shapes_ok()):
            # the aggregator as two launches: all layers + row_proj (csrc/mixer_chain.hip: the token matrix stays in LDS
            # between layers), then channel_proj, biases, flatten and the normalisation on the (B, K, out_d) result
            b, k, c = x.shape
            lns, fc1s, fc2s = ([m.mix[i] for m in self.mix] for i in (0, 1, 3))
            _, u = ops.mixer_chain(x.reshape(b * k, c).contiguous(), _mixer_chain_pack(self.mix), [l.weight for l in lns],
                                   [l.bias for l in lns], [f.bias for f in fc1s], [f.bias for f in fc2s], lns[0].eps,
                                   row_w=self.row_proj.weight, want_x=False)
            return ops.descriptor_tail(u.view(b, k, -1), self.channel_proj.weight, self.channel_proj.bias, self.row_proj.weight,
                                       self.row_proj.bias, normalize)
        x = self._forward_launches(x)
        return F.normalize(x, dim=1) if normalize else x

    def _forward_launches(self, x):
        if _split_path(x) and x.shape[-1] % 128 == 0 and all(_mixer_layer_fits(m) for m in self.mix):
            # inference: every FeatureMixerLayer as LayerNorm -> split2, fc1 + GELU, fc2 + residual on the hand-written split GEMM
            # (three launches instead of LayerNorm, addmm, GELU, addmm, add: the (B k, C) token matrix is 8 k rows, every one of
            # these launches is latency-bound and the host was issuing them into an idle GPU)
            b, k, c = x.shape
            x2 = x.reshape(b * k, c)
            for m in self.mix:
                ln, fc1, _, fc2 = m.mix
                if _GEMM_MODE == 'x3' and ops.mlp_fused_shape_ok(c, fc1.out_features):
                    # the whole layer as the block MLP's launch (hidden = C): one launch (+ the hidden split's reduce) for three
                    x2 = ops.ln_mlp_fused(x2.contiguous(), ln.weight, ln.bias, ln.eps, _mixer_pack(fc1, fc2), fc1.bias, fc2.bias)
                    continue
                h2 = ops.layer_norm_split2(x2, ln.weight, ln.bias, ln.eps)
                g2 = ops.linear_x3(h2, _w2(fc1), bias=fc1.bias, gelu_split_out=True)
                x2 = ops.linear_x3(g2, _w2(fc2), bias=fc2.bias, residual=x2)
            x = x2.view(b, k, c)
        elif (all(_mixer_layer_fits(m) for m in self.mix) and x.shape[-1] in ops._LN_CHANNELS
              and _x6_train(x, *[l for m in self.mix for l in (m.mix[1], m.mix[3])])):
            # matched-precision training: every FeatureMixerLayer as one autograd Function (LayerNorm, fc1 + GELU, fc2 + bias +
            # residual forward; weight gradients on hfl_wgrad_f32)
            b, k, c = x.shape
            x2 = x.reshape(b * k, c)
            for m in self.mix:
                ln, fc1, _, fc2 = m.mix
                x2 = ag.ln_mlp_residual_x6(x2, ln.weight, ln.bias, ln.eps, fc1.weight, fc1.bias, fc2.weight, fc2.bias)
            x = x2.view(b, k, c)
        elif all(_mixer_layer_fits(m) for m in self.mix) and _x6_path(x, *[l for m in self.mix for l in (m.mix[1], m.mix[3])]):
            # matched precision: LayerNorm, fc1 + bias + GELU, fc2 + bias + residual on hfl_linear_x6 (three launches per layer)
            b, k, c = x.shape
            x2 = x.reshape(b * k, c).contiguous()
            for m in self.mix:
                ln, fc1, _, fc2 = m.mix
                h = ops.layer_norm(x2, ln.weight, ln.bias, ln.eps)
                g = ops.linear_x6(h, _w6(fc1), bias=fc1.bias, gelu=True)
                x2 = ops.linear_x6(g, _w6(fc2), bias=fc2.bias, residual=x2)
            x = x2.view(b, k, c)
        else:
            x = self.mix(x)
        if self._tail_fits(x):
            # channel_proj, row_proj and the flatten as one small launch (row_proj first: the maps commute)
            return ops.mixer_tail(x, self.channel_proj.weight, self.channel_proj.bias, self.row_proj.weight, self.row_proj.bias)
        x = self.channel_proj(x.permute(0, 2, 1)).permute(0, 2, 1)
        return self.row_proj(x).flatten(1)


class PyramidAttnPoolWrapper(nn.Module):
    """models/layers/pooling.py:106-233 (aggregator='mixer')"""

    def __init__(self, feature_size, output_dim, channels, num_pyramid_levels, k_pooled_tokens,
                 mlp_ratio=1, mix_depth=4):
        super().__init__()
        channels = list(channels)
        self.use_projections = len(channels) != 1                               # pooling.py:123-129
        if len(channels) == 1:
            channels = channels * num_pyramid_levels
        assert len(channels) == num_pyramid_levels, 'Incorrect num channels'
        assert len(k_pooled_tokens) == num_pyramid_levels, \
            'k_pooled_tokens must be list of k for each pyramid level'
        self.k_pooled_tokens = list(k_pooled_tokens)
        total = sum(k_pooled_tokens)
        self.attpool = nn.ModuleList([AdaptivePooling(channels[j], k) for j, k in enumerate(k_pooled_tokens)])
        if self.use_projections:                                                # pooling.py:143-152
            self.local_projections = nn.ModuleList([nn.Linear(c, feature_size) if c != feature_size else nn.Identity()
                                                    for c in channels])
        k_out = total // 4
        out_d = output_dim // k_out
        assert k_out * out_d == output_dim, \
            f'Invalid k for k_pooled_tokens: {k_pooled_tokens}, not compatible with output dim {output_dim}'
        self.descriptor_extractor = Mixer(total, k_out, feature_size, mix_depth, mlp_ratio, out_d)

    def forward(self, local_feat_dict, plan: WindowPlan, depth=None, normalize=False):
        """`normalize`: the Mixer returns L2-normalised descriptors (one launch with its tail where that applies)"""
        feats = list(local_feat_dict.items())
        if (not self.use_projections and not _grad_path() and feats and feats[0][1].is_cuda
                and all(f.shape[1] == feats[0][1].shape[1] and f.dtype == torch.float32 for _, f in feats)):
            # every level writes its k_j tokens straight into the (B, sum k, C) token matrix: no torch.cat
            all_t = torch.empty((plan.B, sum(self.k_pooled_tokens), feats[0][1].shape[1]), dtype=torch.float32,
                                device=feats[0][1].device)
            off = 0
            for j, (d, f) in enumerate(feats):
                k = self.k_pooled_tokens[j]
                t = self.attpool[j](f, plan, d, out=all_t[:, off:off + k])
                if t.data_ptr() != all_t[:, off:off + k].data_ptr():
                    all_t[:, off:off + k].copy_(t)
                off += k
            return self.descriptor_extractor(all_t, normalize)
        toks = []
        for j, d in enumerate(local_feat_dict.keys()):
            t = self.attpool[j](local_feat_dict[d], plan, d)
            toks.append(self.local_projections[j](t) if self.use_projections else t)
        return self.descriptor_extractor(torch.cat(toks, 1), normalize)


class OctGeM(nn.Module):
    """models/layers/pooling.py:18-40: generalised-mean pooling of the finest pyramid level over each cloud's
    non-empty nodes (`ocnn.nn.OctreeGlobalPool(nempty=True)` = per-cloud mean)."""

    def __init__(self, input_dim, p=3, eps=1e-6):
        super().__init__()
        self.input_dim = self.output_dim = input_dim
        self.p = nn.Parameter(torch.ones(1) * p)
        self.eps = eps

    def forward(self, x, plan: WindowPlan, depth=None):
        if isinstance(x, dict):
            depth, x = max(x.items())
        temp = x.clamp(min=self.eps).pow(self.p)
        return _cloud_mean(temp, plan, depth).pow(1. / self.p)


class RelayTokenGeM(nn.Module):
    """models/layers/pooling.py:43-57 on a padded (B, N, C) tensor (every row counts, as in the reference)."""

    def __init__(self, input_dim, p=3, eps=1e-6):
        super().__init__()
        self.input_dim = self.output_dim = input_dim
        self.p = nn.Parameter(torch.ones(1) * p)
        self.eps = eps

    def forward(self, x):
        return x.clamp(min=self.eps).pow(self.p).mean(dim=1).pow(1. / self.p)


class GatingContext(nn.Module):
    """models/layers/netvlad.py:83-112"""

    def __init__(self, dim, add_batch_norm=True):
        super().__init__()
        self.dim, self.add_batch_norm = dim, add_batch_norm
        self.gating_weights = nn.Parameter(torch.randn(dim, dim) / dim ** 0.5)
        if add_batch_norm:
            self.gating_biases = None
            self.bn1 = nn.BatchNorm1d(dim)
        else:
            self.gating_biases = nn.Parameter(torch.randn(dim) / dim ** 0.5)
            self.bn1 = None

    def forward(self, x):
        gates = torch.matmul(x, self.gating_weights)
        gates = self.bn1(gates) if self.add_batch_norm else gates + self.gating_biases
        return x * torch.sigmoid(gates)


class PyramidOctGeMWrapper(nn.Module):
    """models/layers/pooling.py:60-103: GeM per pyramid level (own exponent each), concatenated, Linear + BatchNorm,
    optional context gating."""

    def __init__(self, input_dim, output_dim, num_pyramid_levels, channels, p=3, eps=1e-6, gating=False,
                 add_batch_norm=True):
        super().__init__()
        assert num_pyramid_levels > 0, 'Minimum 1 pyramid layer'
        if len(channels) == 1:                                                  # pooling.py:66-70
            concat_dim = input_dim * num_pyramid_levels
        else:
            assert len(channels) == num_pyramid_levels, 'Incorrect num channels'
            concat_dim = sum(channels)
        self.input_dim, self.output_dim, self.num_pyramid_levels = input_dim, output_dim, num_pyramid_levels
        self.p = nn.Parameter(torch.ones(num_pyramid_levels) * p)
        self.eps, self.gating = eps, gating
        self.linear_bn = nn.Sequential(nn.Linear(concat_dim, output_dim, bias=False),
                                       nn.BatchNorm1d(input_dim))
        if gating:
            self.context_gating = GatingContext(output_dim, add_batch_norm=add_batch_norm)

    def forward(self, local_feat_dict, plan: WindowPlan, depth=None):
        desc = []
        for j, d in enumerate(local_feat_dict.keys()):
            temp = local_feat_dict[d].clamp(min=self.eps).pow(self.p[j])
            desc.append(_cloud_mean(temp, plan, d).pow(1. / self.p[j]))
        g = self.linear_bn(torch.cat(desc, dim=-1))
        return self.context_gating(g) if self.gating else g


class AttnPoolWrapper(nn.Module):
    """models/layers/pooling.py:235-305: attentional pooling of every cloud's multi-scale relay tokens (fine to coarse,
    `relay_token_utils.py:12-40`) to k tokens, then the MLP mixer or LayerNorm + MLP + GeM."""

    def __init__(self, feature_size=256, output_dim=256, k_pooled_tokens=64, mlp_ratio=1, aggregator='mixer',
                 mix_depth=4):
        super().__init__()
        assert isinstance(k_pooled_tokens, int), 'Only 1 value allowed for k_pooled_tokens when using relay tokens'
        self.feature_size, self.output_dim, self.k_pooled_tokens = feature_size, output_dim, k_pooled_tokens
        self.aggregator = aggregator
        self.attpool = AdaptivePooling(feature_size, k_pooled_tokens)
        if aggregator.lower() == 'mixer':
            k_out = k_pooled_tokens // 4
            self.descriptor_extractor = Mixer(k_pooled_tokens, k_out, feature_size, mix_depth, mlp_ratio,
                                              output_dim // k_out)
        elif aggregator.lower() == 'gem':
            self.token_processor = nn.Sequential(nn.LayerNorm(feature_size),
                                                 MLP(feature_size, feature_size * mlp_ratio, output_dim))
            self.descriptor_extractor = RelayTokenGeM(input_dim=feature_size)
        else:
            raise NotImplementedError(f'No valid aggregator: {aggregator}')

    def forward(self, relay_token_dict, plan: WindowPlan, depth=None):
        rt_all = torch.cat([relay_token_dict[d] for d in plan.pyramid_depths], 0)      # rows as plan.rt_offset
        idx, valid = plan.relay_pad_index()                                            # (B, Rmax): cloud -> its rows
        x = rt_all[idx.clamp(min=0)] * valid.unsqueeze(-1).to(rt_all.dtype)            # zero padding rows
        # learned queries attend over the cloud's own tokens; padding keys get the reference's -1e3 additive mask
        scores = torch.matmul(self.attpool.query * self.attpool.scale, x.transpose(1, 2))          # (B, k, Rmax)
        scores = scores + (~valid).unsqueeze(1).to(scores.dtype) * -1e3
        tok = torch.matmul(torch.softmax(scores, dim=-1), x)                                      # (B, k, C)
        if self.aggregator.lower() != 'mixer':
            tok = tok + self.token_processor(tok)
        return self.descriptor_extractor(tok)


def _cloud_mean(x, plan: WindowPlan, depth: int):
    """(N_t, C) rows of one depth -> (B, C) mean over each cloud's rows (fixed summation order: padded gather)."""
    idx = plan.pad_index_for(depth)
    zero = x.new_zeros(1, x.shape[1])
    xp = torch.cat([x, zero], 0).index_select(0, idx).view(plan.B, -1, x.shape[1])
    cnt = plan.cloud_count(depth).clamp(min=1).to(x.dtype)
    return xp.sum(1) / cnt.unsqueeze(1)


class PoolingWrapper(nn.Module):
    """models/layers/pooling_wrapper.py:11-77"""

    def __init__(self, pool_method, in_dim, output_dim, num_pyramid_levels=None, channels=None,
                 k_pooled_tokens=None):
        super().__init__()
        self.pool_method, self.in_dim, self.output_dim = pool_method, in_dim, output_dim
        self.pooled_feats = 'local'             # flag if local feats or relay tokens are pooled
        if pool_method == 'OctGeM':
            assert in_dim == output_dim
            self.pooling = OctGeM(input_dim=in_dim)
        elif pool_method in ('PyramidOctGeM', 'PyramidOctGeMgc'):
            self.pooling = PyramidOctGeMWrapper(in_dim, output_dim, num_pyramid_levels, list(channels),
                                                gating=pool_method.endswith('gc'))
        elif pool_method == 'PyramidAttnPoolMixer':
            self.pooling = PyramidAttnPoolWrapper(in_dim, output_dim, list(channels), num_pyramid_levels,
                                                  k_pooled_tokens)
        elif pool_method in ('AttnPoolMixer', 'AttnPoolGeM'):
            self.pooled_feats = 'relaytokens'
            self.pooling = AttnPoolWrapper(in_dim, output_dim, k_pooled_tokens,
                                           aggregator='mixer' if pool_method == 'AttnPoolMixer' else 'GeM')
        elif pool_method == 'PyramidNetVLAD':
            raise NotImplementedError(f'Not implemented yet: {pool_method}')       # as the reference
        else:
            raise NotImplementedError('Unknown pooling method: {}'.format(pool_method))

    def forward(self, x, octree=None, depth=None, normalize=False):
        """`normalize`: F.normalize(., dim=1) of the descriptors; the Mixer head folds it into its last launch"""
        if normalize and isinstance(self.pooling, PyramidAttnPoolWrapper):
            return self.pooling(x, octree, depth, normalize=True)
        x = self.pooling(x, octree, depth)
        return F.normalize(x, dim=1) if normalize else x


# ------------------------------------------------------------------------- wrapper
class HOTFormerLoc(nn.Module):
    """models/hotformerloc.py:18-82"""

    def __init__(self, backbone: nn.Module, pooling: PoolingWrapper, normalize_embeddings=False,
                 input_features='P'):
        super().__init__()
        if input_features != 'P':
            raise NotImplementedError("input_features=%r: every shipped config uses 'P'" % input_features)
        self.backbone = backbone
        self.pooling = pooling
        self.normalize_embeddings = normalize_embeddings
        self.input_features = input_features
        self.stats = {}

    def forward(self, batch):
        octree = batch['octree']
        if octree.device.type != 'cuda':
            raise RuntimeError('HOTFormerLoc (MI355X build) needs the octree on a GPU; '
                               'call to_device(batch, "cuda") first -- there is no CPU path')
        octree.construct_all_neigh()                     # no-op when misc/torch_utils.to_device did it
        data = octree.get_input_feature(self.input_features, nempty=True)
        armed = self.training
        if armed:
            arm_drop_paths(self, int(octree.batch_size), data.device, data.dtype)
        try:
            local, relay, plan = self.backbone(data, octree, octree.depth)
        finally:
            if armed:
                disarm_drop_paths(self)
        if self.pooling.pooled_feats == 'local':
            x = local
        elif self.pooling.pooled_feats == 'relaytokens':
            x = relay
        else:
            raise ValueError(f"Invalid option for pooled features: '{self.pooling.pooled_feats}'")
        x = self.pooling(x, octree=plan, normalize=self.normalize_embeddings)
        assert x.dim() == 2 and x.shape[1] == self.pooling.output_dim
        return {'global': x}

    def print_info(self):
        n = sum(p.nelement() for p in self.parameters())
        print('Model class: HOTFormerLoc (MI355X build)')
        print(f'Total parameters: {n}')
        print(f'Pooling method: {self.pooling.pool_method}')
        print(f'Embedding normalization: {self.normalize_embeddings}')
