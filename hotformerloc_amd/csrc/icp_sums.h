// The per-workgroup partials hfl_icp_solve reads, filled and reduced in one order, once, for both evaluations of the rigid
// estimator: icp_correspond_kernel (csrc/registration.hip), which finds its correspondences by the pair scan, and
// ransac_sums_kernel (csrc/global_registration.hip), whose correspondences are fixed.
//
// The row step adds one inlier row to the 17 float64 quantities n, Sp (3), Sq (3), Spq (9, row-major: p' down, q across),
// sum d^2; p' the moved source point, q its target, d their fp32 distance.  Every product is of two widened fp32 values
// and exact in float64, so contracting it into its sum changes no bit: the same result with -ffp-contract=off
// (global_registration.hip) and without (registration.hip).
//
// The reduction: a thread has added its rows in row order, a wave combines its lanes by the xor butterfly 32 .. 1, and the
// wave results are added in wave order, one quantity a thread: the order of pair_stats_kernel.  No atomics, one writer.
#pragma once
#include "ragged_common.h"

namespace {

// one inlier row of the point-to-point sums, in this statement order: pc, qc and dd are the fp32 p', q and d, widened
__device__ __forceinline__ void icp_point_row(double (&acc)[HFL_ICP_SUMS], const double (&pc)[3], const double (&qc)[3],
                                              double dd) {
  acc[0] += 1.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    acc[1 + a] += pc[a];
    acc[4 + a] += qc[a];
#pragma unroll
    for (int b = 0; b < 3; ++b) acc[7 + 3 * a + b] += pc[a] * qc[b];
  }
  acc[16] += dd * dd;
}

// acc[NS] of every thread of a workgroup of THREADS -> row blockIdx.x of the (n_tiles, NS) partials.  `red`: (THREADS / 64,
// NS) doubles of LDS; a caller that reuses an area puts its own barrier in front.  Every thread of the workgroup calls it.
template <int NS, int THREADS>
__device__ __forceinline__ void icp_reduce_partials(double (&acc)[NS], double* red, double* __restrict__ partials) {
  const int lane = threadIdx.x & (HFL_WAVE - 1), wave = threadIdx.x / HFL_WAVE;
#pragma unroll
  for (int k = 0; k < NS; ++k) acc[k] = wave_sum(acc[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NS; ++k) red[wave * NS + k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    double v = red[threadIdx.x];
    for (int w = 1; w < THREADS / HFL_WAVE; ++w) v += red[w * NS + threadIdx.x];
    partials[(int64_t)blockIdx.x * NS + threadIdx.x] = v;
  }
}

}  // namespace
