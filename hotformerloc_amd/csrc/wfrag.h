// Weight fragments that go from L2 straight into MFMA operand registers (csrc/relay_block.hip, csrc/mixer_chain.hip): the
// pack of one fp32 Linear weight, the step-ahead load ring, and the three-product split MFMA.
//
// pack of W (N, K): [n-tile of 16 features][k-step of 32][hi | lo][lane = fq * 16 + fr][8 bf16: k = 32 ks + 8 fq ..] of
// W[16 nt + fr][k] -- every 16-feature x 32-k fragment is the 1 KiB a wave reads with one 16-B load per lane.
#pragma once
#include "hfl_common.h"
#include "x3_math.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// acc += w_hi x_lo + w_lo x_hi + w_hi x_hi (the order of csrc/qkv_fused.hip and csrc/mlp_fused.hip); weights are the A
// operand, activation rows the B operand: a lane's accumulator holds features 4 fq .. 4 fq + 3 of row fr
__device__ __forceinline__ f32x4 wfrag_x3(bf16x8 whi, bf16x8 wlo, bf16x8 xh, bf16x8 xl, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(whi, xl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wlo, xh, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(whi, xh, acc, 0, 0, 0);
}

// fp32 Linear weight (N, K) -> its pack: one lane per 16-B cell
__global__ void __launch_bounds__(256)
wfrag_pack_kernel(unsigned char* __restrict__ dst, const float* __restrict__ w, int N, int K) {
  const int ks_n = K / 32;
  const int64_t cells = (int64_t)N * K / 8;                    // per (hi | lo) half
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cells; i += (int64_t)gridDim.x * blockDim.x) {
    const int lane = (int)(i & 63);
    const int64_t frag = i >> 6;                                // nt * ks_n + ks
    const int ks = (int)(frag % ks_n), nt = (int)(frag / ks_n);
    const float* src = w + (int64_t)(nt * 16 + (lane & 15)) * K + ks * 32 + (lane >> 4) * 8;
    uint32_t hi[4], lo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t h0 = x3_bf16_rne(src[2 * j]), h1 = x3_bf16_rne(src[2 * j + 1]);
      const uint32_t l0 = x3_bf16_rne(src[2 * j] - __uint_as_float(h0 << 16));
      const uint32_t l1 = x3_bf16_rne(src[2 * j + 1] - __uint_as_float(h1 << 16));
      hi[j] = h0 | (h1 << 16);
      lo[j] = l0 | (l1 << 16);
    }
    unsigned char* d = dst + frag * 2048 + lane * 16;
    *reinterpret_cast<u32x4*>(d) = (u32x4){hi[0], hi[1], hi[2], hi[3]};
    *reinterpret_cast<u32x4*>(d + 1024) = (u32x4){lo[0], lo[1], lo[2], lo[3]};
  }
}

}  // namespace
