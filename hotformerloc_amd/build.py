"""Build libhotformerloc_hip.so (gfx950) in-tree with hipcc.

`python -m hotformerloc_amd.build` or `__graft_entry__.build()`.  hipcc
cross-compiles without a GPU; the resulting .so travels to the GPU box with the
repo snapshot (it is git-ignored, not gpurun-ignored).
"""

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIBDIR = os.path.join(HERE, 'lib')
LIBNAME = 'libhotformerloc_hip.so'
ARCH = 'gfx950'
SOURCES = ['capi.hip', 'dwconv.hip', 'octree.hip', 'preprocess.hip', 'augment.hip', 'voxel.hip', 'ground.hip', 'outliers.hip', 'normals.hip', 'keypoints.hip', 'fpfh.hip', 'window_misc.hip', 'attention.hip', 'gemm_x3.hip', 'gemm_x6.hip', 'mlp_fused.hip', 'qkv_fused.hip', 'attn_fused.hip', 'attn_ws.hip', 'relay_block.hip', 'mixer_chain.hip', 'attn_pool.hip', 'wgrad_x3.hip', 'wgrad_f32.hip', 'tapconv.hip', 'gemm_lt.hip', 'loss.hip', 'pairwise.hip', 'batch_hard.hip', 'batch_masks.hip', 'radius.hip', 'overlap.hip', 'registration.hip', 'global_registration.hip', 'spectral.hip', 'consensus.hip', 'ema.hip', 'optim.hip', 'retrieval.hip']
FLAGS = ['--offload-arch=' + ARCH, '-O3', '-std=c++17', '-fPIC', '-fno-gpu-rdc',
         '-Wall', '-Wno-unused-function']
# hipBLASLt for hfl_gemm_bf16 (the ROCm copy that matches the headers; rpath so the loader finds it)
ROCM = os.environ.get('ROCM_PATH', '/opt/rocm')
LINK_FLAGS = ['-L' + os.path.join(ROCM, 'lib'), '-lhipblaslt', '-Wl,-rpath,' + os.path.join(ROCM, 'lib')]
# per-file extras.  attention.hip: MFMA results feed VALU softmax code directly, so keep the MFMA
# destination in arch VGPRs (the default heuristic parks it in AGPRs and pays a v_accvgpr_read per score)
EXTRA_FLAGS = {'attention.hip': ['-mllvm', '-amdgpu-mfma-vgpr-form=1'],
               # mlp_fused.hip: element-wise math runs BETWEEN MFMAs there; packed f32 VALU (what SLP vectorisation of adjacent
               # scalar ops produces) stalls the matrix pipe, plain VALU does not
               'mlp_fused.hip': ['-fno-slp-vectorize'],
               'qkv_fused.hip': ['-fno-slp-vectorize'],
               'attn_fused.hip': ['-fno-slp-vectorize', '-mllvm', '-amdgpu-mfma-vgpr-form=1'],
               'attn_ws.hip': ['-fno-slp-vectorize', '-mllvm', '-amdgpu-mfma-vgpr-form=1'],
               'relay_block.hip': ['-fno-slp-vectorize', '-mllvm', '-amdgpu-mfma-vgpr-form=1'],
               'mixer_chain.hip': ['-fno-slp-vectorize', '-mllvm', '-amdgpu-mfma-vgpr-form=1'],
               # radius.hip: membership must be dx*dx + dy*dy with every operation rounded to float64, bit for bit what numpy
               # computes; the _rn intrinsics alone do not stop hipcc from fusing the second product into the sum (v_fmac_f64)
               'radius.hip': ['-ffp-contract=off'],
               # ground.hip: the cloth filter is defined in fp32 with every operation rounded once, bit for bit what the numpy
               # route computes
               'ground.hip': ['-ffp-contract=off'],
               # outliers.hip: the neighbour distances are defined in fp32, the radius trim in float64, every operation
               # rounded once
               'outliers.hip': ['-ffp-contract=off'],
               # normals.hip: the same search, and float64 sums and a Jacobi that follow the numpy route operation for operation
               'normals.hip': ['-ffp-contract=off'],
               # keypoints.hip: the same search, sums and Jacobi (cov_eigen.h), and float64 products in the ratio tests
               'keypoints.hip': ['-ffp-contract=off'],
               # fpfh.hip: the same search, and float64 pair features whose bins must equal the numpy route's bit for bit
               'fpfh.hip': ['-ffp-contract=off'],
               # global_registration.hip: the float64 edge check and Kabsch solve of a drawn triple follow the numpy route
               # operation for operation; the score kernel's two hypotheses per thread, packed into v_pk_fma_f32 pairs by SLP
               # vectorisation, need 146 VGPRs (three waves per SIMD) where the plain form needs 74 (six)
               'global_registration.hip': ['-ffp-contract=off', '-fno-slp-vectorize'],
               # spectral.hip: every fmaf of the matrix entry and of the sum is explicit and nothing else may be fused: the
               # weights equal the numpy route's bit for bit
               'spectral.hip': ['-ffp-contract=off'],
               # consensus.hip: the same matrix entry, and float64 sums and a Kabsch solve that follow the numpy route
               # operation for operation
               'consensus.hip': ['-ffp-contract=off'],
               # batch_hard.hip: the distances carry the bits of hfl_pairwise_dist, and the terms and the gradient follow the
               # numpy twins operation for operation
               'batch_hard.hip': ['-ffp-contract=off']}


def _hipcc() -> str:
    for cand in (os.environ.get('HIPCC'), shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError('hipcc not found (need ROCm >= 7.0 for gfx950)')


def _newer(target: str, deps) -> bool:
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(d) <= t for d in deps)


def build_library(force: bool = False, verbose: bool = True) -> str:
    os.makedirs(LIBDIR, exist_ok=True)
    objdir = os.path.join(LIBDIR, 'obj')
    os.makedirs(objdir, exist_ok=True)
    hipcc = _hipcc()
    # every header: one that is left out leaves stale objects behind when objects are reused
    headers = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith('.h')) + \
        [os.path.join(HERE, '..', 'include', 'hotformerloc_hip.h')]
    jobs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace('.hip', '.o'))
        if force or not _newer(o, [s] + headers):
            jobs.append((s, o))

    def compile_one(job):
        s, o = job
        cmd = [hipcc] + FLAGS + EXTRA_FLAGS.get(os.path.basename(s), []) + os.environ.get('HFL_EXTRA_HIPCC_FLAGS', '').split() + \
            ['-c', s, '-o', o]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError('hipcc failed for %s:\n%s' % (s, r.stderr))
        if verbose and r.stderr.strip():
            print(r.stderr, file=sys.stderr)
        return o

    if jobs:
        with ThreadPoolExecutor(max_workers=min(4, len(jobs))) as ex:
            list(ex.map(compile_one, jobs))
    objs = [os.path.join(objdir, s.replace('.hip', '.o')) for s in SOURCES]
    for stale in set(os.listdir(objdir)) - {os.path.basename(o) for o in objs}:      # objects whose source is gone
        os.remove(os.path.join(objdir, stale))
    lib = os.path.join(LIBDIR, LIBNAME)
    if force or jobs or not os.path.exists(lib):
        cmd = [hipcc, '--offload-arch=' + ARCH, '-shared', '-fPIC', '-o', lib] + objs + LINK_FLAGS
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError('link failed:\n' + r.stderr)
    if verbose:
        print('built', lib)
    return lib


if __name__ == '__main__':
    build_library(force='--force' in sys.argv)
