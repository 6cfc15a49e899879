// The row arithmetic of LayerNorm, shared by layer_norm_kernel (csrc/window_misc.hip) and the octree convolution's slot sum
// with the caller's norm folded in (csrc/dwconv.hip): ONE body, so that both launches compile the same expressions and the
// fused pass gives bit for bit what the sum followed by the norm gives.
#pragma once
#include "hfl_common.h"

// fp32 -> (hi, lo) bf16 with hi = RNE(v), lo = RNE(v - hi): v ~= hi + lo to 2^-17 relative.
__device__ __forceinline__ uint16_t hfl_bf16_rne(float v) {
  uint32_t u = __float_as_uint(v);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
__device__ __forceinline__ void hfl_split4(const float4 v, uint2& hi, uint2& lo) {
  const uint16_t h0 = hfl_bf16_rne(v.x), h1 = hfl_bf16_rne(v.y), h2 = hfl_bf16_rne(v.z), h3 = hfl_bf16_rne(v.w);
  const uint16_t l0 = hfl_bf16_rne(v.x - __uint_as_float((uint32_t)h0 << 16));
  const uint16_t l1 = hfl_bf16_rne(v.y - __uint_as_float((uint32_t)h1 << 16));
  const uint16_t l2 = hfl_bf16_rne(v.z - __uint_as_float((uint32_t)h2 << 16));
  const uint16_t l3 = hfl_bf16_rne(v.w - __uint_as_float((uint32_t)h3 << 16));
  hi = make_uint2((uint32_t)h0 | ((uint32_t)h1 << 16), (uint32_t)h2 | ((uint32_t)h3 << 16));
  lo = make_uint2((uint32_t)l0 | ((uint32_t)l1 << 16), (uint32_t)l2 | ((uint32_t)l3 << 16));
}
// row of the split-GEMM A operand: [hi (C) | hi (C) | lo (C)] bf16, so that one bf16 GEMM against
// [w_hi | w_lo | w_hi] accumulates hi*hi + hi*lo + lo*hi in fp32
__device__ __forceinline__ void hfl_store_split3(uint16_t* row, int C, int c4, const float4 v) {
  uint2 hi, lo;
  hfl_split4(v, hi, lo);
  reinterpret_cast<uint2*>(row)[c4] = hi;
  reinterpret_cast<uint2*>(row + C)[c4] = hi;
  reinterpret_cast<uint2*>(row + 2 * C)[c4] = lo;
}

// row of the hand-written split GEMM's operand (csrc/gemm_x3.hip): per 32-channel block [32 x hi | 32 x lo]
__device__ __forceinline__ void hfl_store_split2(uint16_t* row, int c4, const float4 v) {
  uint2 hi, lo;
  hfl_split4(v, hi, lo);
  uint16_t* o = row + (c4 >> 3) * 64 + (c4 & 7) * 4;
  *reinterpret_cast<uint2*>(o) = hi;
  *reinterpret_cast<uint2*>(o + 32) = lo;
}

// LayerNorm (+ ReLU) of row r, held as VPL float4 per lane by the TPR lanes that own it (C = 4 * TPR * VPL; a[] of a row that
// is not `live` is zero), and its store.  Two-pass statistics with a corrected mean, by butterfly over the TPR lanes: EVERY lane
// of the wave calls this.
// SPLIT: 0 = fp32 output, 1 = bf16 [hi|hi|lo] (K-concatenated, hipBLASLt route), 2 = bf16 split2 (gemm_x3 route)
template <int TPR, int VPL, int SPLIT>
__device__ __forceinline__ void hfl_ln_row(float* __restrict__ h_out, float4 (&a)[VPL], const float4 (&gm)[VPL],
                                           const float4 (&bt)[VPL], int64_t r, bool live, int tx, float eps, int relu) {
  constexpr int C = TPR * VPL * 4;
  const float inv_c = 1.0f / (float)C;
  float sum = 0.f;
#pragma unroll
  for (int v = 0; v < VPL; ++v) sum += (a[v].x + a[v].y) + (a[v].z + a[v].w);
  const float mean = hfl_group_sum<TPR>(sum) * inv_c;
  // `mean` carries the rounding of a sum of C values of the row's magnitude (2^-9 for a row around 2^14); the residuals do
  // not (x - mean is exact for x near mean), so their own mean `dm` is what the first pass missed: it is taken off the
  // variance and, folded into one fma, off every element.  A constant row comes out as beta whatever its sum rounded to.
  float sq = 0.f, rs = 0.f;
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    a[v].x -= mean; a[v].y -= mean; a[v].z -= mean; a[v].w -= mean;
    rs += (a[v].x + a[v].y) + (a[v].z + a[v].w);
    sq += (a[v].x * a[v].x + a[v].y * a[v].y) + (a[v].z * a[v].z + a[v].w * a[v].w);
  }
  const float dm = hfl_group_sum<TPR>(rs) * inv_c;
  const float rstd = 1.0f / sqrtf(fmaxf(fmaf(-dm, dm, hfl_group_sum<TPR>(sq) * inv_c), 0.f) + eps);
  const float dr = dm * rstd;
  if (live) {
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      float4 o;
      o.x = fmaf(fmaf(a[v].x, rstd, -dr), gm[v].x, bt[v].x);
      o.y = fmaf(fmaf(a[v].y, rstd, -dr), gm[v].y, bt[v].y);
      o.z = fmaf(fmaf(a[v].z, rstd, -dr), gm[v].z, bt[v].z);
      o.w = fmaf(fmaf(a[v].w, rstd, -dr), gm[v].w, bt[v].w);
      if (relu) {                              // conv -> norm -> ReLU of the stem (octformer_layers.py:80-98) in one pass
        o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f);
      }
      if (SPLIT == 1)
        hfl_store_split3(reinterpret_cast<uint16_t*>(h_out) + r * 3 * C, C, v * TPR + tx, o);
      else if (SPLIT == 2)
        hfl_store_split2(reinterpret_cast<uint16_t*>(h_out) + r * 2 * C, v * TPR + tx, o);
      else
        reinterpret_cast<float4*>(h_out + r * C)[v * TPR + tx] = o;
    }
  }
}
