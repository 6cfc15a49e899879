// What the raw-cloud kernels share (csrc/preprocess.hip, csrc/augment.hip): one 1024-lane workgroup per cloud.
#pragma once
#include "hfl_common.h"

constexpr int kPrepThreads = 1024;

// min or max of `v` over the workgroup, returned to every lane; `red` holds kPrepThreads / 64 floats
__device__ __forceinline__ float block_reduce(float v, bool is_max, float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
    const float o = __shfl_xor(v, m, 64);
    v = is_max ? fmaxf(v, o) : fminf(v, o);
  }
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float r = red[0];
  for (int w = 1; w < kPrepThreads / 64; ++w) r = is_max ? fmaxf(r, red[w]) : fminf(r, red[w]);
  return r;
}

__device__ __forceinline__ double interp2(double x, double x0, double x1, double y0, double y1) {
  // numpy arr_interp with two knots: clamp outside, exact knot values, else slope*(x - x0) + y0 (mul, add: 2 roundings)
  if (x > x1) return y1;
  if (x < x0) return y0;
  if (x == x1) return y1;
  if (x == x0) return y0;
  const double slope = __ddiv_rn(__dsub_rn(y1, y0), __dsub_rn(x1, x0));
  return __dadd_rn(__dmul_rn(slope, __dsub_rn(x, x0)), y0);
}

// (x,y,z) inside the unit cube / cylinder -> (rho,phi,z) rescaled to [-1,1] (datasets/coordinate_utils.py:30-45,68-116)
__device__ __forceinline__ void cylindrical_transform(float& x, float& y, float& z) {
  const float phi = atan2f(y, x);
  const float rho = __fsqrt_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)));
  const double kPi = 3.141592653589793;
  x = (float)interp2((double)rho, 0.0, 1.0, -1.0, 1.0);
  y = (float)interp2((double)phi, -kPi, kPi, -1.0, 1.0);
  x = fminf(fmaxf(x, -1.0f), 1.0f);
  y = fminf(fmaxf(y, -1.0f), 1.0f);
  z = fminf(fmaxf(z, -1.0f), 1.0f);
}
