// What the exact grid k-nearest-neighbour searches share (csrc/outliers.hip: the mean neighbour distance; csrc/normals.hip:
// the neighbourhood covariance): the launch shape, the cell-start table, the fp32 squared distance, the sorted register
// list, the completeness bound and the host check of the grids.  hotformerloc_amd/outliers.py and DESIGN.md section 7g
// define the search; every file that includes this is built with -ffp-contract=off.
#pragma once
#include <math.h>

#include "ragged_common.h"

namespace {

constexpr int kOutThreads = 256;
constexpr int kOutWaves = kOutThreads / HFL_WAVE;
constexpr float kFaceShrink = 1.f - 9.5367431640625e-07f;      // 1 - 2^-20: the relative part of the margin of the bound

// starts[t] = the first sorted position whose key is >= t, for t in [0, n_cells]: cell t holds [starts[t], starts[t + 1])
__global__ void __launch_bounds__(kOutThreads)
knn_cell_starts_kernel(int32_t* __restrict__ starts, const int64_t* __restrict__ skeys, int64_t n, int64_t n_cells) {
  const int64_t t = (int64_t)blockIdx.x * kOutThreads + threadIdx.x;
  if (t > n_cells) return;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (skeys[mid] < t) lo = mid + 1; else hi = mid;
  }
  starts[t] = (int32_t)lo;
}

// (dx dx + dy dy) + dz dz on the differences themselves, every operation rounded once
__device__ __forceinline__ float knn_d2(float px, float py, float pz, const float* __restrict__ q) {
  const float dx = __fsub_rn(px, q[0]), dy = __fsub_rn(py, q[1]), dz = __fsub_rn(pz, q[2]);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// The K smallest values seen, ascending, in registers: every index is a compile-time constant after unrolling, so the list
// never goes to scratch memory.  Inserting v into the sorted list and dropping the largest is, per slot, the median of
// (left neighbour, own value, v).
template <int K>
struct KnnList {
  float v[K];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int i = 0; i < K; ++i) v[i] = INFINITY;
  }
  __device__ __forceinline__ void insert(float d) {
    if (d < v[K - 1]) {
#pragma unroll
      for (int i = K - 1; i > 0; --i) v[i] = fmaxf(v[i - 1], fminf(v[i], d));
      v[0] = fminf(v[0], d);
    }
  }
  __device__ __forceinline__ float kth(int k) const {         // v[k - 1] as the largest of the first k: the list ascends,
    float r = -INFINITY;                                       // and no register is indexed by a run-time value
#pragma unroll
    for (int i = 0; i < K; ++i) r = fmaxf(r, i < k ? v[i] : -INFINITY);
    return r;
  }
  __device__ __forceinline__ void pop() {
#pragma unroll
    for (int i = 0; i + 1 < K; ++i) v[i] = v[i + 1];
    v[K - 1] = INFINITY;
  }
};

// the distance from coordinate p to the nearest face of the scanned cells [c0, c1] that has cells behind it, less the
// absolute margin; +inf when the block reaches both ends of the axis
__device__ __forceinline__ float knn_face_gap(float p, float origin, float cell, int c0, int c1, int top, float margin) {
  const float a = __fsub_rn(p, origin);
  float gap = INFINITY;
  if (c0 > 0) gap = fminf(gap, __fsub_rn(__fsub_rn(a, __fmul_rn((float)c0, cell)), margin));
  if (c1 < top) gap = fminf(gap, __fsub_rn(__fsub_rn(__fmul_rn((float)(c1 + 1), cell), a), margin));
  return gap;
}

// every grid inside the cell table and every field in range, before anything runs
bool knn_grids_ok(const hfl_knn_grid* g, int batch, int64_t n_cells, int* k_max) {
  int big = 0;
  for (int b = 0; b < batch; ++b) {
    const hfl_knn_grid& d = g[b];
    if (d.nx < 1 || d.ny < 1 || d.nz < 1 || d.k < 1 || d.k > HFL_KNN_MAX_NEIGHBOURS) return false;
    const int64_t cells = (int64_t)d.nx * d.ny;
    if (cells > HFL_KNN_MAX_CELLS || cells * d.nz > HFL_KNN_MAX_CELLS) return false;
    if (d.cell_base < 0 || d.cell_base > n_cells || cells * d.nz > n_cells - d.cell_base) return false;
    if (!(d.ox - d.ox == 0.f) || !(d.oy - d.oy == 0.f) || !(d.oz - d.oz == 0.f)) return false;      // finite
    if (!(d.cell > 0.f) || !(d.cell <= 3.4028234e38f)) return false;
    if (!(d.mx >= 0.f) || !(d.my >= 0.f) || !(d.mz >= 0.f)) return false;
    if (d.k > big) big = d.k;
  }
  *k_max = big;
  return true;
}

}  // namespace
