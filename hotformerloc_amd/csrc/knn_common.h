// The exact grid k-nearest-neighbour search over a ragged batch, once, for everything that runs it (csrc/outliers.hip: the
// mean neighbour distance; csrc/normals.hip: the neighbourhood covariance; csrc/fpfh.hip: the descriptor's three passes).
// Here are the launch shape, the cell-start table, the fp32 squared distance, the sorted register list and the host checks;
// what a thread knows of its point (`KnnPoint`); the first scan of the 3 x 3 x 3 block with its completeness bound
// (`knn_first_scan` on `knn_block`, `knn_block_scan`, `knn_block_bound`); the list of unresolved points
// (`knn_append_pending`) and the wave-per-point walk over it (`knn_for_pending`, `knn_cloud_scan`, `knn_wave_merge`).  The
// kernels of the three files keep only what they do with a neighbour.  hotformerloc_amd/outliers.py and DESIGN.md section
// 7g define the search; every file that includes this is built with -ffp-contract=off.
//
// Radius and hybrid neighbourhoods.  `cap` is R2, the largest fp32 d2 that counts as "within the
// radius", a launch argument, the same for every cloud of a call; +inf is no cap and changes no bit.  Hybrid: the first scan
// and the fallback take r2 = min(k-th smallest, cap).  Radius-only: r2 = cap for every point, so there is no list and no
// first scan -- `knn_radius_first` only asks the bound whether the block holds every point within cap, and the consumer
// does its work in one pass over the block (or over the cloud, for a pending point).
#pragma once
#include <math.h>

#include <type_traits>

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
  __device__ __forceinline__ void pop_if(bool mine) {          // selects, not a branch: a wave runs both sides anyway
#pragma unroll
    for (int i = 0; i + 1 < K; ++i) v[i] = mine ? v[i + 1] : v[i];
    v[K - 1] = mine ? INFINITY : v[K - 1];
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

// What a thread of a query kernel knows of the point at sorted position j: its cloud, the cloud's grid and range of sorted
// positions (clamped to the arrays), its cell on that grid, its coordinates
struct KnnPoint {
  int c;
  hfl_knn_grid g;
  int32_t first, last;
  int64_t local;
  float px, py, pz;
  __device__ __forceinline__ bool in_cells() const { return local >= 0 && local < (int64_t)g.nx * g.ny * g.nz; }
  template <int K>
  __device__ __forceinline__ bool on_grid() const {            // a key off its own grid goes to the whole-cloud scan
    return in_cells() && g.k >= 1 && g.k <= K;
  }
};

__device__ __forceinline__ KnnPoint knn_point(const float* __restrict__ spts, const int64_t* __restrict__ skeys,
                                              const hfl_knn_grid* __restrict__ grids, const int64_t* __restrict__ off,
                                              int batch, int64_t n, int64_t j) {
  KnnPoint p;
  p.c = find_cloud(off, batch, j);
  p.g = grids[p.c];
  p.first = (int32_t)max(off[p.c], (int64_t)0), p.last = (int32_t)min(off[p.c + 1], n);
  p.local = skeys[j] - p.g.cell_base;
  p.px = spts[j * 3 + 0], p.py = spts[j * 3 + 1], p.pz = spts[j * 3 + 2];
  return p;
}

// The first scan of a point: the K smallest squared distances of its block in `list`, r2 the smaller of the k-th smallest
// of them and `cap`, and whether the bound proves that every point with d2 <= r2 lies in the block.  A block with fewer
// than k points has a k-th of +inf and is resolved through the cap alone: every point within the cap lies in the block.
// Off the grid: +inf, not resolved, no block.
struct KnnFirst {
  KnnBlock blk = {};
  float r2 = INFINITY;
  bool resolved = false;
};

template <int K>
__device__ __forceinline__ KnnFirst knn_first_scan(KnnList<K>& list, const KnnPoint& p, const float* __restrict__ spts,
                                                   const int32_t* __restrict__ starts, float cap = INFINITY) {
  KnnFirst f;
  list.clear();
  if (p.on_grid<K>()) {
    f.blk = knn_block(p.g, p.local);
    knn_block_scan(p.g, f.blk, starts, p.first, p.last,
                   [&](int32_t q) { list.insert(knn_d2(p.px, p.py, p.pz, spts + (int64_t)q * 3)); });
    f.r2 = fminf(list.kth(p.g.k), cap);
    f.resolved = f.r2 < knn_block_bound(p.px, p.py, p.pz, p.g, f.blk);
  }
  return f;
}

// what takes the first scan's place when r2 is the cap for every point: the block, and whether the bound proves that every
// point with d2 <= cap lies in it.  The grid's k is not read.  Off the grid: not resolved, no block.
__device__ __forceinline__ KnnFirst knn_radius_first(const KnnPoint& p, float cap) {
  KnnFirst f;
  f.r2 = cap;
  if (p.in_cells()) {
    f.blk = knn_block(p.g, p.local);
    f.resolved = cap < knn_block_bound(p.px, p.py, p.pz, p.g, f.blk);
  }
  return f;
}

__device__ __forceinline__ int knn_lane() { return threadIdx.x & (HFL_WAVE - 1); }

// f(m) for the k smallest values of the 64 lists of a wave in ascending order, m the same in every lane: the smallest head
// of the lists, k times; one lane gives up one copy per round, so equal values stay a multiset.  The lists are consumed.
template <int K, typename F>
__device__ __forceinline__ void knn_wave_merge(KnnList<K>& list, int k, F&& f) {
  const int lane = knn_lane();
  for (int r = 0; r < k; ++r) {
    const float head = list.v[0];
    float m = head;
#pragma unroll
    for (int s = HFL_WAVE / 2; s > 0; s >>= 1) m = fminf(m, __shfl_xor(m, s, HFL_WAVE));
    const unsigned long long owners = __ballot(head == m);
    list.pop_if(lane == __ffsll((long long)owners) - 1);
    f(m);
  }
}

// the smaller of `cap` and the k-th smallest value of the 64 lists: the last of the k rounds
template <int K>
__device__ __forceinline__ float knn_wave_kth(KnnList<K>& list, int k, float cap = INFINITY) {
  float r2 = INFINITY;
  knn_wave_merge(list, k, [&](float m) { r2 = m; });
  return fminf(r2, cap);
}

// a cap is a squared distance or +inf: not negative, not a NaN
inline bool knn_cap_ok(float cap) { return cap >= 0.f; }

// appends sorted position j to the list of points the block could not resolve: one integer add per wave, the order of the
// list is free.  Every lane that calls it must be active together (call it under one condition).
__device__ __forceinline__ void knn_append_pending(int32_t* __restrict__ pending, int32_t* __restrict__ counter, int64_t j,
                                                   int64_t n) {
  const unsigned long long mask = __ballot(1);
  const int lane = knn_lane();
  const int leader = __ffsll((long long)mask) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(counter, __popcll(mask));
  base = __shfl(base, leader, HFL_WAVE);
  const int slot = base + __popcll(mask & ((1ull << lane) - 1ull));
  if (slot >= 0 && slot < n) pending[slot] = (int32_t)j;
}

// f(q) for the sorted positions [first, last) of a cloud, dealt to the lanes of a wave: a lane's points in ascending order
template <typename F>
__device__ __forceinline__ void knn_cloud_scan(int64_t first, int64_t last, F&& f) {
  for (int64_t q = first + knn_lane(); q < last; q += HFL_WAVE) f(q);
}

// the first pass of a fallback kernel: every lane's K smallest squared distances from p to its share of the cloud
template <int K>
__device__ __forceinline__ void knn_cloud_first(KnnList<K>& list, float px, float py, float pz,
                                                const float* __restrict__ spts, int64_t first, int64_t last) {
  list.clear();
  knn_cloud_scan(first, last, [&](int64_t q) { list.insert(knn_d2(px, py, pz, spts + q * 3)); });
}

// The fallback kernels: a wave per pending point, the waves striding over the list; every loop bound is the same in all
// lanes of a wave.  f(j, c, first, last): the sorted position, its cloud and the cloud's range clamped to the arrays.
template <typename F>
__device__ __forceinline__ void knn_for_pending(const int32_t* __restrict__ pending, const int32_t* __restrict__ counter,
                                                const int64_t* __restrict__ off, int batch, int64_t n, F&& f) {
  const int64_t wave = (int64_t)blockIdx.x * kOutWaves + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * kOutWaves;
  const int64_t count = min((int64_t)max(*counter, 0), n);
  for (int64_t e = wave; e < count; e += waves) {
    const int64_t j = pending[e];
    if (j < 0 || j >= n) continue;
    const int c = find_cloud(off, batch, j);
    f(j, c, max(off[c], (int64_t)0), min(off[c + 1], n));
  }
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

// what every entry point of the search checks after its pointers, in this order: the arguments, the capacity, the grids
int knn_call_check(int batch, int64_t n_points, int64_t n_cells, const hfl_knn_grid* grids_host, int* k_max) {
  if (batch < 1 || n_points < batch || n_cells < 1) return HFL_EINVAL;
  if (batch > HFL_VOXEL_MAX_CLOUDS || n_points > HFL_VOXEL_MAX_POINTS || n_cells > HFL_KNN_MAX_CELLS) return HFL_ECAPACITY;
  return knn_grids_ok(grids_host, batch, n_cells, k_max) ? HFL_OK : HFL_EINVAL;
}

// the workgroups of a fallback kernel: a wave per point at the most, eight workgroups a CU
unsigned knn_fallback_blocks(int64_t n, hipStream_t s) {
  return (unsigned)min(hfl_cdiv(n, kOutWaves), (int64_t)hfl_stream_cus(s) * 8);
}

// f(std::integral_constant<int, K>) for the smallest list length K that holds k_max
template <typename F>
int knn_dispatch_k(int k_max, F&& f) {
  if (k_max <= 8) return f(std::integral_constant<int, 8>());
  if (k_max <= 16) return f(std::integral_constant<int, 16>());
  return f(std::integral_constant<int, 32>());
}

// what a search launches before its query kernel: the cell-start table, and the counter of the pending list at zero
int knn_launch_starts(int32_t* starts, int32_t* counter, const int64_t* skeys, int64_t n, int64_t n_cells, int phases,
                      hipStream_t s) {
  if (phases & HFL_KNN_PHASE_STARTS)
    knn_cell_starts_kernel<<<(unsigned)hfl_cdiv(n_cells + 1, kOutThreads), kOutThreads, 0, s>>>(starts, skeys, n, n_cells);
  if (phases & HFL_KNN_PHASE_QUERY) return (int)hipMemsetAsync(counter, 0, sizeof(int32_t), s);
  return HFL_OK;
}

}  // namespace
