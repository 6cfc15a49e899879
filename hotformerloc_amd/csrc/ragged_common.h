// What the ragged-batch kernels share (csrc/voxel.hip, csrc/ground.hip, csrc/outliers.hip, csrc/overlap.hip): the search for
// a point's cloud and the fixed-order sums the bit-for-bit claims of those files rest on.
#pragma once
#include "hfl_common.h"

// the cloud that holds point i: the largest c in [0, batch) with off[c] <= i
__device__ __forceinline__ int find_cloud(const int64_t* __restrict__ off, int batch, int64_t i) {
  int lo = 0, hi = batch - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// the sum over the wave by the xor butterfly 32 .. 1, the same value in every lane
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int m = HFL_WAVE / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, HFL_WAVE);
  return v;
}

// the sum over a workgroup of THREADS lanes in a fixed order -- `wave_sum`, then the waves in wave order -- the same value in
// every lane; `red` holds THREADS / 64 doubles.  Two barriers: the first lets the previous call's parts be read.
template <int THREADS>
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int lane = threadIdx.x & (HFL_WAVE - 1), wave = threadIdx.x / HFL_WAVE;
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  double r = red[0];
#pragma unroll
  for (int w = 1; w < THREADS / HFL_WAVE; ++w) r += red[w];
  return r;
}
