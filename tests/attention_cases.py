"""Helpers shared by the attention kernel tests (tests/test_gpu_kernels.py, tests/test_gpu_attention_shapes.py): the window plans
of the oracle and of the package over the same clouds, and the fp16 (hi, lo) operand layout of the window / relay kernels."""

import torch

from hotformerloc_amd import build_batch_octree
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
    head [16 x hi | 16 x lo] fp16 (any split with hi + lo = v to 22 bits is valid), q times q_scale; returned as an
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
