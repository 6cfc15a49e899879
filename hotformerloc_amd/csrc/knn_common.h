// What the exact grid k-nearest-neighbour searches share (csrc/outliers.hip: the mean neighbour distance; csrc/normals.hip:
// the neighbourhood covariance; csrc/fpfh.hip: the descriptor's three passes): the launch shape, the cell-start table, the
// fp32 squared distance, the sorted register list, the completeness bound and the host check of the grids; and, as
// functions, the search itself -- the 3 x 3 x 3 block and its scan, the bound of a block, the merge of a wave's lists, the
// list of unresolved points (`knn_block` .. `knn_append_pending`, which csrc/fpfh.hip runs three times over; the two older
// files spell the same steps out in their query kernels and stay as they are, so that their code objects do not change).
// hotformerloc_amd/outliers.py and DESIGN.md section 7g define the search; every file that includes this is built with
// -ffp-contract=off.
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

// The 3 x 3 x 3 block of cells round cell `local` of grid g, clipped to the grid
struct KnnBlock {
  int x0, x1, y0, y1, z0, z1;
};

__device__ __forceinline__ KnnBlock knn_block(const hfl_knn_grid& g, int64_t local) {
  const int ix = (int)(local % g.nx), iy = (int)((local / g.nx) % g.ny), iz = (int)(local / ((int64_t)g.nx * g.ny));
  KnnBlock b;
  b.x0 = max(ix - 1, 0), b.x1 = min(ix + 1, g.nx - 1);
  b.y0 = max(iy - 1, 0), b.y1 = min(iy + 1, g.ny - 1);
  b.z0 = max(iz - 1, 0), b.z1 = min(iz + 1, g.nz - 1);
  return b;
}

// f(q) for every sorted position q of the block's cells that lies in [first, last), in ascending order of q within a line
// of cells and the lines in (z, y) order: the "sorted-position order" of the sums
template <typename F>
__device__ __forceinline__ void knn_block_scan(const hfl_knn_grid& g, const KnnBlock& b, const int32_t* __restrict__ starts,
                                               int32_t first, int32_t last, F&& f) {
#pragma unroll 1
  for (int z = b.z0; z <= b.z1; ++z)
#pragma unroll 1
    for (int y = b.y0; y <= b.y1; ++y) {
      const int64_t line = g.cell_base + ((int64_t)z * g.ny + y) * g.nx;        // the cells x0 .. x1 of a line are adjacent
      const int32_t s = max(starts[line + b.x0], first), e = min(starts[line + b.x1 + 1], last);
#pragma unroll 1
      for (int32_t q = s; q < e; ++q) f(q);
    }
}

// the square of the conservative distance from p to the nearest face of the block that has cells behind it: a k-th distance
// strictly below it proves that every point within that distance lies in the block
__device__ __forceinline__ float knn_block_bound(float px, float py, float pz, const hfl_knn_grid& g, const KnnBlock& b) {
  float gap = knn_face_gap(px, g.ox, g.cell, b.x0, b.x1, g.nx - 1, g.mx);
  gap = fminf(gap, knn_face_gap(py, g.oy, g.cell, b.y0, b.y1, g.ny - 1, g.my));
  gap = fminf(gap, knn_face_gap(pz, g.oz, g.cell, b.z0, b.z1, g.nz - 1, g.mz));
  gap = __fmul_rn(fmaxf(gap, 0.f), kFaceShrink);
  return __fmul_rn(gap, gap);
}

// the k-th smallest value of the 64 lists of a wave, the same in every lane: the smallest head of the lists, k times; one
// lane gives up one copy per round, so equal values stay a multiset.  The lists are consumed.
template <int K>
__device__ __forceinline__ float knn_wave_kth(KnnList<K>& list, int k, int lane) {
  float r2 = INFINITY;
  for (int r = 0; r < k; ++r) {
    const float head = list.v[0];
    float m = head;
#pragma unroll
    for (int s = HFL_WAVE / 2; s > 0; s >>= 1) m = fminf(m, __shfl_xor(m, s, HFL_WAVE));
    const unsigned long long owners = __ballot(head == m);
    if (lane == __ffsll((long long)owners) - 1) list.pop();
    r2 = m;
  }
  return r2;
}

// appends sorted position j to the list of points the block could not resolve: one integer add per wave, the order of the
// list is free.  Every lane that calls it must be active together (call it under one condition).
__device__ __forceinline__ void knn_append_pending(int32_t* __restrict__ pending, int32_t* __restrict__ counter, int64_t j,
                                                   int64_t n) {
  const unsigned long long mask = __ballot(1);
  const int lane = threadIdx.x & (HFL_WAVE - 1);
  const int leader = __ffsll((long long)mask) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(counter, __popcll(mask));
  base = __shfl(base, leader, HFL_WAVE);
  const int slot = base + __popcll(mask & ((1ull << lane) - 1ull));
  if (slot >= 0 && slot < n) pending[slot] = (int32_t)j;
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
