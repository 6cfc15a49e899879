"""Helpers shared by the attention kernel tests (tests/test_gpu_kernels.py, tests/test_gpu_attention_shapes.py,
tests/test_gpu_dynamic_range.py): the window plans of the oracle and of the package over the same clouds, the float64 window and
relay references over them, and the fp16 (hi, lo) operand layout of the window / relay kernels."""

import numpy as np
import torch

from hotformerloc_amd import build_batch_octree
from hotformerloc_amd import synthetic as syn
from hotformerloc_amd.plan import WindowPlan
from oracle import hotformer_ref
from oracle.testing import oracle_octree

DEV = 'cuda'


def octrees(clouds, octree_depth):
    """(oracle octree, device octree) of one batch of clouds."""
    return oracle_octree(clouds, octree_depth), build_batch_octree(clouds, octree_depth, 2, DEV)


def window_plans(ref, dev, **args):
    """(oracle WindowPlan, package WindowPlan) with the same constructor arguments over the two octrees."""
    return hotformer_ref.WindowPlan(ref, **args), WindowPlan(dev, **args)


def pack_qkv_f16(qkv: torch.Tensor, H: int, q_scale: float) -> torch.Tensor:
    """fp32 (rows, 3C) [q | k | v] -> the operand layout of hfl_linear_x3_qkv (csrc/gemm_x3.hip EPI 2): per region and
    head [16 x hi | 16 x lo] fp16 (any split with |hi + lo - v| <= max(2^-20 |v|, 2^-24) is valid), q times q_scale; returned as an
    opaque float32 (rows, 3C) buffer."""
    rows, c3 = qkv.shape
    C = c3 // 3
    x = qkv.clone().float()
    x[:, :C] *= q_scale
    x = x.view(rows, 3, H, 16)
    hi = x.to(torch.float16)
    lo = (x - hi.float()).to(torch.float16)
    packed = torch.stack([hi, lo], dim=3).contiguous()            # (rows, 3, H, 2, 16) fp16 = 12 C bytes per row
    return packed.view(rows, -1).view(torch.float32).view(rows, c3).contiguous()


# ------------------------------------------------------------------- the clouds and plans of test_gpu_attention_shapes.py
ODEPTH = 7                                 # octree depth: attention at depths 5..2
SIZES = (900, 25, 600)                     # the 25-point cloud lies inside one window, with both its boundaries, at every K
_CACHE = {}


def clouds():
    return [syn.unit_ball_cloud(2100, SIZES[0]), syn.unit_ball_cloud(2101, SIZES[1]), syn.forest_cloud(2102, SIZES[2])]


def oracle_plan(K, D):
    """The oracle's plan alone (no GPU): every depth 5..2 is a relay-token depth, so that `hat_mask` exists at depth 5 too."""
    key = ('oplan', K, D)
    if key not in _CACHE:
        if 'ref' not in _CACHE:
            _CACHE['ref'] = oracle_octree(clouds(), ODEPTH)
        _CACHE[key] = hotformer_ref.WindowPlan(_CACHE['ref'], **plan_args(K, D))
    return _CACHE[key]


def plan_args(K, D):
    return dict(patch_size=K, dilation=D, max_depth=ODEPTH - 2, start_depth=ODEPTH - 5, num_pyramid_levels=4,
                num_octf_levels=0, adape_mode=None)


def plans(K, D):
    key = ('plans', K, D)
    if key not in _CACHE:
        if 'dev' not in _CACHE:
            _CACHE['ref'], _CACHE['dev'] = octrees(clouds(), ODEPTH)
        _CACHE[key] = (oracle_plan(K, D), WindowPlan(_CACHE['dev'], **plan_args(K, D)))
    return _CACHE[key]


def mask_pos(oplan, depth, G, dil):
    if dil > 1:
        return oplan.dilate_mask[depth], oplan.dilate_pos[depth]
    return (oplan.hat_mask[depth] if G else oplan.patch_mask[depth]), oplan.rel_pos[depth]


def windows_ref(oplan, qkv_tok, qkv_rt, table, depth, K, G, dil, H):
    """The reference's materialised window attention in the dtype of its arguments (float64 here): (windows (W, K + G, C),
    token rows (nt, C))."""
    C = H * 16
    xw = oplan.to_windows(qkv_tok, depth, dil > 1)
    if G:
        xw = torch.cat([qkv_rt.unsqueeze(1), xw], 1)
    q, k, v = xw.reshape(-1, K + G, 3, H, 16).permute(2, 0, 3, 1, 4)
    mask, pos = mask_pos(oplan, depth, G, dil)
    bias = mask.to(qkv_tok.dtype).unsqueeze(1)
    if table is not None:
        rpe = hotformer_ref.rpe_bias(table, pos, K, dil)
        if G:
            rpe = torch.nn.functional.pad(rpe, (G, 0, G, 0))
        bias = bias + rpe
    o = hotformer_ref._sdpa(q, k, v, bias, 0.25).transpose(1, 2).reshape(-1, K + G, C)
    return o, oplan.from_windows(o[:, G:], depth, dil > 1)


# ------------------------------------------------------------------------------------------------------- relay attention
def sequence_table(lengths, n_rows, seed):
    """Sequences over a seeded permutation of [0, n_rows): the rows that no sequence lists are orphans."""
    perm = np.random.RandomState(seed).permutation(n_rows).astype(np.int32)
    n = int(sum(lengths))
    assert n < n_rows
    seq_rows = perm[:n]
    seq_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    orphans = np.sort(perm[n:]).astype(np.int32)
    return seq_rows, seq_off, orphans


def relay_ref(qkv, seq_rows, seq_off, H):
    """Per-cloud dense softmax attention in the dtype of qkv; rows of no sequence stay 0."""
    C = H * 16
    out = qkv.new_zeros((qkv.shape[0], C))
    parts = []
    for b in range(len(seq_off) - 1):
        rows = torch.from_numpy(seq_rows[seq_off[b]:seq_off[b + 1]].astype(np.int64))
        if rows.numel() == 0:
            continue
        q, k, v = qkv[rows].view(-1, 3, H, 16).permute(1, 2, 0, 3)
        p = torch.softmax(torch.matmul(q, k.transpose(-2, -1)) * 0.25, dim=-1)
        parts.append((rows, torch.matmul(p, v).transpose(0, 1).reshape(-1, C)))
    for rows, o in parts:
        out = out.index_put((rows,), o)
    return out
