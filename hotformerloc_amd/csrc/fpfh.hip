// FPFH descriptors of every point of a ragged batch of clouds, and nearest-neighbour correspondences in descriptor space.
// Both are DEFINED in hotformerloc_amd/fpfh.py (module docstring) and DESIGN.md section 7k; this file and the numpy routes
// there follow that definition.  The search is the exact grid search of knn_common.h, which csrc/outliers.hip and
// csrc/normals.hip run as well, on the batch that `outliers.sorted_batch` lays out; everything here works on SORTED
// positions and only the last kernel un-permutes.
//
//   hfl_fpfh_radius    the cell-start table; one thread per point scans the 3 x 3 x 3 block of cells round its own for r2,
//                      the k-th smallest fp32 squared distance (the sorted register list), and notes whether the
//                      completeness bound proves that every point with d2 <= r2 lies in the block; the others are appended
//                      to a list, and a wave per listed point finds r2 in the point's whole cloud.
//   hfl_fpfh_radius_capped  the same with r2 = min(k-th smallest, R2) (hybrid), or, radius-only, r2 = R2 for every point
//                      with no scan at all: one thread per point asks the completeness bound whether its block holds every
//                      point within R2 and lists the point if not.  The two calls below read r2 and the proof and never k,
//                      so they serve all three kinds of neighbourhood unchanged.
//   hfl_fpfh_spfh      one thread per proven point re-scans its block, a wave per listed point its whole cloud: every
//                      neighbour with d2 <= r2 that forms a pair is binned, in float64, into the thread's 33 counters.  The
//                      counters live in LDS, one column per thread (33 x 256 x 4 B = 33 KiB a workgroup, four workgroups a
//                      CU): a bin index is a run-time value, and registers indexed by one would go to scratch memory.
//   hfl_fpfh_combine   the same scan once more: the neighbours' histograms weighted by 100 / pairs_j / d2 and added in
//                      float64 (33 accumulators in registers, every index a constant), normalised per group, added to the
//                      point's own SPFH, rounded to fp32 and stored at row perm[j].
//   hfl_feature_nn     brute force over descriptor rows on the pieces of pair_scan.h (the workgroup's tile, the rule that
//                      keeps a candidate, the entry point's checks): a workgroup of 256 threads owns 512 consecutive query
//                      rows of one pair, two rows per thread in registers; the pair's target rows stream through a 24 KiB
//                      LDS tile, row after row, every lane reading the same row by broadcast ds_read_b128.  d2 = d0 d0, then
//                      fmaf(dc, dc, d2) for c = 1 .. D - 1, over ascending target rows.  The distance over D columns and
//                      the row-major tile are this file's own.
//
// Histograms and pair counts are integers and the neighbourhood is a pure function of the input, so they do not depend on
// the grid or on any order.  The float64 sums of hfl_fpfh_combine run in an order fixed by the sort and the grid.  No
// floating-point atomics (one integer add per wave appends to the list), one writer per element: two runs give the same
// bits.  Built with -ffp-contract=off: every float64 operation of a pair feature is rounded once, as numpy rounds it.
#include <math.h>

#include "knn_common.h"
#include "pair_scan.h"

namespace {

constexpr int FP_BINS = 11;
constexpr int FP_DIM = 3 * FP_BINS;
constexpr int FP_EDGES = FP_BINS - 1;

// (cos e_k, sin e_k) of the bin edges e_k = -pi + 2 pi k / 11, k = 1 .. 10: the caller's bits, by value
struct ThetaTable {
  double c[FP_EDGES], s[FP_EDGES];
};

// a zero row says "no normal"; so does a row with a component that is not finite
__device__ __forceinline__ bool has_normal(float x, float y, float z) {
  return (x - x == 0.f) && (y - y == 0.f) && (z - z == 0.f) && (x != 0.f || y != 0.f || z != 0.f);
}

// floor(11 (f + 1) / 2) clamped to 0 .. 10
__device__ __forceinline__ int linear_bin(double f) {
  const double t = floor((11.0 * (f + 1.0)) / 2.0);
  return (int)fmin(fmax(t, 0.0), 10.0);
}

// #{k : theta >= e_k} for the direction (x, y), decided by two rounded products per edge and no transcendental function
__device__ __forceinline__ int theta_bin(double x, double y, const ThetaTable& t) {
  int low = 0, high = 0;
#pragma unroll
  for (int k = 0; k < FP_EDGES / 2; ++k) low += (t.c[k] * y >= t.s[k] * x) ? 1 : 0;
#pragma unroll
  for (int k = FP_EDGES / 2; k < FP_EDGES; ++k) high += (t.c[k] * y >= t.s[k] * x) ? 1 : 0;
  if (x == 0.0 && y == 0.0) return FP_EDGES / 2;
  return y < 0.0 ? low : FP_EDGES / 2 + high;
}

// The pair feature of point i (p, n) and its neighbour j (q, m), both with normals: false when the pair is skipped (the
// points coincide, or dp is parallel to the source normal), else the three bins.
__device__ __forceinline__ bool pair_bins(float px, float py, float pz, float nx, float ny, float nz, float qx, float qy,
                                          float qz, float mx, float my, float mz, const ThetaTable& t, int& b_theta,
                                          int& b_f2, int& b_f3) {
  const double dx = (double)qx - (double)px, dy = (double)qy - (double)py, dz = (double)qz - (double)pz;
  const double d = __dsqrt_rn((dx * dx + dy * dy) + dz * dz);
  if (!(d > 0.0)) return false;
  const double a1 = (((double)nx * dx + (double)ny * dy) + (double)nz * dz) / d;
  const double a2 = (((double)mx * dx + (double)my * dy) + (double)mz * dz) / d;
  const bool swap = fabs(a1) < fabs(a2);                       // the source is the end whose normal lies closer to the line
  const double sx = swap ? (double)mx : (double)nx, sy = swap ? (double)my : (double)ny, sz = swap ? (double)mz : (double)nz;
  const double tx = swap ? (double)nx : (double)mx, ty = swap ? (double)ny : (double)my, tz = swap ? (double)nz : (double)mz;
  const double ex = swap ? -dx : dx, ey = swap ? -dy : dy, ez = swap ? -dz : dz;
  const double f3 = swap ? -a2 : a1;
  double vx = ey * sz - ez * sy, vy = ez * sx - ex * sz, vz = ex * sy - ey * sx;
  const double vn = __dsqrt_rn((vx * vx + vy * vy) + vz * vz);
  if (!(vn > 0.0)) return false;
  vx = vx / vn;
  vy = vy / vn;
  vz = vz / vn;
  const double wx = sy * vz - sz * vy, wy = sz * vx - sx * vz, wz = sx * vy - sy * vx;
  const double f2 = (vx * tx + vy * ty) + vz * tz;
  const double x = (sx * tx + sy * ty) + sz * tz;
  const double y = (wx * tx + wy * ty) + wz * tz;
  b_theta = theta_bin(x, y, t);
  b_f2 = linear_bin(f2);
  b_f3 = linear_bin(f3);
  return true;
}

// ---------------------------------------------------------------------------------------------------------------- radius
template <int K>
__global__ void __launch_bounds__(kOutThreads)
fpfh_radius_kernel(float* __restrict__ r2s, uint8_t* __restrict__ proven, int32_t* __restrict__ pending,
                   int32_t* __restrict__ counter, const float* __restrict__ spts, const int64_t* __restrict__ skeys,
                   const int32_t* __restrict__ starts, const hfl_knn_grid* __restrict__ grids,
                   const int64_t* __restrict__ off, int batch, int64_t n, float cap) {
  const int64_t j = (int64_t)blockIdx.x * kOutThreads + threadIdx.x;
  if (j >= n) return;
  const KnnPoint p = knn_point(spts, skeys, grids, off, batch, n, j);
  KnnList<K> list;
  const KnnFirst f = knn_first_scan(list, p, spts, starts, cap);
  r2s[j] = f.r2;
  proven[j] = f.resolved ? 1 : 0;
  if (!f.resolved) knn_append_pending(pending, counter, j, n);
}

// r2 = cap for every point, the pending ones too: nothing is scanned and no fallback follows
__global__ void __launch_bounds__(kOutThreads)
fpfh_radius_only_kernel(float* __restrict__ r2s, uint8_t* __restrict__ proven, int32_t* __restrict__ pending,
                        int32_t* __restrict__ counter, const float* __restrict__ spts, const int64_t* __restrict__ skeys,
                        const hfl_knn_grid* __restrict__ grids, const int64_t* __restrict__ off, int batch, int64_t n,
                        float cap) {
  const int64_t j = (int64_t)blockIdx.x * kOutThreads + threadIdx.x;
  if (j >= n) return;
  const KnnFirst f = knn_radius_first(knn_point(spts, skeys, grids, off, batch, n, j), cap);
  r2s[j] = cap;
  proven[j] = f.resolved ? 1 : 0;
  if (!f.resolved) knn_append_pending(pending, counter, j, n);
}

template <int K>
__global__ void __launch_bounds__(kOutThreads)
fpfh_radius_fallback_kernel(float* __restrict__ r2s, const int32_t* __restrict__ pending,
                            const int32_t* __restrict__ counter, const float* __restrict__ spts,
                            const hfl_knn_grid* __restrict__ grids, const int64_t* __restrict__ off, int batch, int64_t n,
                            float cap) {
  knn_for_pending(pending, counter, off, batch, n, [&](int64_t j, int c, int64_t first, int64_t last) {
    const int k = min(max(grids[c].k, 1), K);
    KnnList<K> list;
    knn_cloud_first(list, spts[j * 3 + 0], spts[j * 3 + 1], spts[j * 3 + 2], spts, first, last);
    const float r2 = knn_wave_kth(list, k, cap);
    if (knn_lane() == 0) r2s[j] = r2;
  });
}

// ------------------------------------------------------------------------------------------------------------------ SPFH
// what both SPFH kernels do with one candidate neighbour q of point j; the counters are column `col` of the LDS array
struct SpfhPoint {
  float px, py, pz, nx, ny, nz, r2;
};

__device__ __forceinline__ SpfhPoint spfh_point(const float* __restrict__ spts, const float* __restrict__ snrm,
                                                const float* __restrict__ r2s, int64_t j) {
  SpfhPoint p;
  p.px = spts[j * 3 + 0], p.py = spts[j * 3 + 1], p.pz = spts[j * 3 + 2];
  p.nx = snrm[j * 3 + 0], p.ny = snrm[j * 3 + 1], p.nz = snrm[j * 3 + 2];
  p.r2 = r2s[j];
  return p;
}

__device__ __forceinline__ int spfh_visit(int32_t (*s_hist)[kOutThreads], int col, const SpfhPoint& p, int64_t j, int64_t q,
                                          const float* __restrict__ spts, const float* __restrict__ snrm,
                                          const ThetaTable& tab) {
  if (q == j) return 0;
  const float* w = spts + q * 3;
  if (!(knn_d2(p.px, p.py, p.pz, w) <= p.r2)) return 0;
  const float mx = snrm[q * 3 + 0], my = snrm[q * 3 + 1], mz = snrm[q * 3 + 2];
  if (!has_normal(mx, my, mz)) return 0;
  int b_theta, b_f2, b_f3;
  if (!pair_bins(p.px, p.py, p.pz, p.nx, p.ny, p.nz, w[0], w[1], w[2], mx, my, mz, tab, b_theta, b_f2, b_f3)) return 0;
  s_hist[b_theta][col] += 1;
  s_hist[FP_BINS + b_f2][col] += 1;
  s_hist[2 * FP_BINS + b_f3][col] += 1;
  return 1;
}

__global__ void __launch_bounds__(kOutThreads)
fpfh_spfh_kernel(int32_t* __restrict__ hist, int32_t* __restrict__ pairs, const float* __restrict__ r2s,
                 const uint8_t* __restrict__ proven, const float* __restrict__ spts, const float* __restrict__ snrm,
                 const int64_t* __restrict__ skeys, const int32_t* __restrict__ starts,
                 const hfl_knn_grid* __restrict__ grids, const int64_t* __restrict__ off, ThetaTable tab, int batch,
                 int64_t n) {
  __shared__ int32_t s_hist[FP_DIM][kOutThreads];               // a column per thread: no barrier, no bank conflict
  const int col = threadIdx.x;
  const int64_t j = (int64_t)blockIdx.x * kOutThreads + threadIdx.x;
  if (j >= n || !proven[j]) return;
  const KnnPoint at = knn_point(spts, skeys, grids, off, batch, n, j);
  if (!at.on_grid<HFL_KNN_MAX_NEIGHBOURS>()) return;             // never with proven[j] set by hfl_fpfh_radius
#pragma unroll
  for (int b = 0; b < FP_DIM; ++b) s_hist[b][col] = 0;
  const SpfhPoint p = spfh_point(spts, snrm, r2s, j);
  int m = 0;
  if (has_normal(p.nx, p.ny, p.nz))
    knn_block_scan(at.g, knn_block(at.g, at.local), starts, at.first, at.last,
                   [&](int32_t q) { m += spfh_visit(s_hist, col, p, j, (int64_t)q, spts, snrm, tab); });
#pragma unroll
  for (int b = 0; b < FP_DIM; ++b) hist[j * FP_DIM + b] = s_hist[b][col];
  pairs[j] = m;
}

__global__ void __launch_bounds__(kOutThreads)
fpfh_spfh_fallback_kernel(int32_t* __restrict__ hist, int32_t* __restrict__ pairs, const float* __restrict__ r2s,
                          const int32_t* __restrict__ pending, const int32_t* __restrict__ counter,
                          const float* __restrict__ spts, const float* __restrict__ snrm,
                          const int64_t* __restrict__ off, ThetaTable tab, int batch, int64_t n) {
  __shared__ int32_t s_hist[FP_DIM][kOutThreads];
  const int col = threadIdx.x, lane = knn_lane();
  knn_for_pending(pending, counter, off, batch, n, [&](int64_t j, int, int64_t first, int64_t last) {
#pragma unroll
    for (int b = 0; b < FP_DIM; ++b) s_hist[b][col] = 0;
    const SpfhPoint p = spfh_point(spts, snrm, r2s, j);
    int m = 0;
    if (has_normal(p.nx, p.ny, p.nz))                          // the same in every lane
      knn_cloud_scan(first, last, [&](int64_t q) { m += spfh_visit(s_hist, col, p, j, q, spts, snrm, tab); });
#pragma unroll
    for (int b = 0; b < FP_DIM; ++b) {                         // integers: any order gives the same sum
      const int32_t v = wave_sum(s_hist[b][col]);
      if (lane == 0) hist[j * FP_DIM + b] = v;
    }
    m = wave_sum(m);
    if (lane == 0) pairs[j] = m;
  });
}

// --------------------------------------------------------------------------------------------------------------- combine
__device__ __forceinline__ void combine_visit(double (&w)[FP_DIM], float px, float py, float pz, float r2, int64_t j,
                                              int64_t q, const float* __restrict__ spts,
                                              const int32_t* __restrict__ hist, const int32_t* __restrict__ pairs) {
  if (q == j) return;
  const float d2 = knn_d2(px, py, pz, spts + q * 3);
  if (!(d2 <= r2) || !(d2 > 0.f)) return;
  const int32_t pq = pairs[q];
  if (pq <= 0) return;
  const double omega = (100.0 / (double)pq) / (double)d2;
  const int32_t* h = hist + q * FP_DIM;
#pragma unroll
  for (int b = 0; b < FP_DIM; ++b) w[b] = w[b] + (double)h[b] * omega;
}

// FPFH(b) = SPFH(b) + (s_g > 0 ? 100 / s_g : 0) W(b), s_g the sum of W over the group in ascending b, rounded once to fp32
__device__ __forceinline__ void combine_finish(float* __restrict__ fpfh, int64_t row, int64_t n, const double (&w)[FP_DIM],
                                               const int32_t* __restrict__ h, int32_t own_pairs) {
  if (row < 0 || row >= n) return;
#pragma unroll
  for (int g = 0; g < 3; ++g) {
    double s = 0.0;
#pragma unroll
    for (int b = 0; b < FP_BINS; ++b) s = s + w[g * FP_BINS + b];
    const double scale = s > 0.0 ? 100.0 / s : 0.0;
#pragma unroll
    for (int b = 0; b < FP_BINS; ++b) {
      const int i = g * FP_BINS + b;
      const double own = own_pairs > 0 ? (100.0 * (double)h[i]) / (double)own_pairs : 0.0;
      fpfh[row * FP_DIM + i] = (float)(own + scale * w[i]);
    }
  }
}

__global__ void __launch_bounds__(kOutThreads)
fpfh_combine_kernel(float* __restrict__ fpfh, const int32_t* __restrict__ hist, const int32_t* __restrict__ pairs,
                    const float* __restrict__ r2s, const uint8_t* __restrict__ proven, const float* __restrict__ spts,
                    const int64_t* __restrict__ skeys, const int64_t* __restrict__ perm, const int32_t* __restrict__ starts,
                    const hfl_knn_grid* __restrict__ grids, const int64_t* __restrict__ off, int batch, int64_t n) {
  const int64_t j = (int64_t)blockIdx.x * kOutThreads + threadIdx.x;
  if (j >= n || !proven[j]) return;
  const KnnPoint p = knn_point(spts, skeys, grids, off, batch, n, j);
  if (!p.on_grid<HFL_KNN_MAX_NEIGHBOURS>()) return;
  const float r2 = r2s[j];
  double w[FP_DIM];
#pragma unroll
  for (int b = 0; b < FP_DIM; ++b) w[b] = 0.0;
  knn_block_scan(p.g, knn_block(p.g, p.local), starts, p.first, p.last,      // sorted-position order
                 [&](int32_t q) { combine_visit(w, p.px, p.py, p.pz, r2, j, (int64_t)q, spts, hist, pairs); });
  combine_finish(fpfh, perm[j], n, w, hist + j * FP_DIM, pairs[j]);
}

__global__ void __launch_bounds__(kOutThreads)
fpfh_combine_fallback_kernel(float* __restrict__ fpfh, const int32_t* __restrict__ hist, const int32_t* __restrict__ pairs,
                             const float* __restrict__ r2s, const int32_t* __restrict__ pending,
                             const int32_t* __restrict__ counter, const float* __restrict__ spts,
                             const int64_t* __restrict__ perm, const int64_t* __restrict__ off, int batch, int64_t n) {
  knn_for_pending(pending, counter, off, batch, n, [&](int64_t j, int, int64_t first, int64_t last) {
    const float px = spts[j * 3 + 0], py = spts[j * 3 + 1], pz = spts[j * 3 + 2], r2 = r2s[j];
    double w[FP_DIM];
#pragma unroll
    for (int b = 0; b < FP_DIM; ++b) w[b] = 0.0;
    knn_cloud_scan(first, last,                                // a lane's points in ascending order
                   [&](int64_t q) { combine_visit(w, px, py, pz, r2, j, q, spts, hist, pairs); });
#pragma unroll
    for (int b = 0; b < FP_DIM; ++b) w[b] = wave_sum(w[b]);     // the lanes by the xor butterfly 32 .. 1
    if (knn_lane() == 0) combine_finish(fpfh, perm[j], n, w, hist + j * FP_DIM, pairs[j]);
  });
}

// ------------------------------------------------------------------------------------------------------------ feature NN
constexpr int FN_THREADS = 256;
constexpr int FN_QPT = HFL_FEATURE_ROWS / FN_THREADS;            // query rows a thread keeps in registers
constexpr int FN_TILE_FLOATS = 6144;                             // 24 KiB of static LDS, as much as the planes of pair_scan3
static_assert(HFL_FEATURE_ROWS % FN_THREADS == 0 && FN_QPT >= 1 && HFL_FEATURE_MAX_DIM <= 64, "whole rows per thread, a launch per D");

// DP: the row length in registers and in LDS, D rounded up to one of a few multiples of four.  The columns past D hold 0 on
// both sides, and fmaf(0, 0, acc) == acc: the padding changes no bit.
template <int DP>
__global__ void __launch_bounds__(FN_THREADS)
feature_nn_kernel(float* __restrict__ dist2, int32_t* __restrict__ idx, const float* __restrict__ queries,
                  const int64_t* __restrict__ q_off, int64_t n_queries, const float* __restrict__ targets,
                  const int64_t* __restrict__ t_off, int64_t n_targets, int dim, const int64_t* __restrict__ tiles,
                  int n_pairs) {
  static_assert(DP % 4 == 0 && DP >= 4 && DP <= HFL_FEATURE_MAX_DIM, "rows of whole float4");
  constexpr int TILE_ROWS = FN_TILE_FLOATS / DP;
  __shared__ __align__(16) float s_t[TILE_ROWS * DP];
  PairTile w;
  if (!pair_tile(w, tiles, n_pairs)) return;
  pair_ranges(w, q_off, n_queries, t_off, n_targets);
  float q[FN_QPT][DP], best[FN_QPT];
  int32_t at[FN_QPT];
#pragma unroll
  for (int r = 0; r < FN_QPT; ++r) {
    const int64_t row = w.row<FN_THREADS>(r);
    const bool valid = row < w.q_end;
#pragma unroll
    for (int c = 0; c < DP; ++c) q[r][c] = (valid && c < dim) ? queries[row * dim + c] : 0.f;
    best[r] = INFINITY;
    at[r] = -1;
  }

  for (int64_t tile = w.t_begin; tile < w.t_end; tile += TILE_ROWS) {
    const int len = (int)min((int64_t)TILE_ROWS, w.t_end - tile);
    __syncthreads();                                             // the previous tile has been read by every wave
    for (int e = threadIdx.x; e < len * DP; e += FN_THREADS) {
      const int r = e / DP, c = e - r * DP;
      s_t[e] = c < dim ? targets[(tile + r) * dim + c] : 0.f;
    }
    __syncthreads();
    const int32_t base = (int32_t)(tile - w.t_begin);            // < 2^31: the entry point bounds n_targets
    for (int k = 0; k < len; ++k) {                              // ascending target row
      const float4* row = reinterpret_cast<const float4*>(&s_t[k * DP]);   // the same address in every lane: broadcast
      float acc[FN_QPT];
#pragma unroll
      for (int c4 = 0; c4 < DP / 4; ++c4) {
        const float4 v = row[c4];
        const float t[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int r = 0; r < FN_QPT; ++r) {
            const float d = q[r][c4 * 4 + u] - t[u];
            acc[r] = (c4 == 0 && u == 0) ? d * d : fmaf(d, d, acc[r]);
          }
      }
#pragma unroll
      for (int r = 0; r < FN_QPT; ++r) pair_keep_closer(acc[r], base + k, best[r], at[r]);
    }
  }

#pragma unroll
  for (int r = 0; r < FN_QPT; ++r) {
    const int64_t row = w.row<FN_THREADS>(r);
    if (row < w.q_end) {
      dist2[row] = best[r];                                      // +inf and -1: an empty target
      idx[row] = at[r];
    }
  }
}

template <int DP>
void feature_nn_launch(float* dist2, int32_t* idx, const float* queries, const int64_t* q_off, int64_t n_q,
                       const float* targets, const int64_t* t_off, int64_t n_t, int dim, const int64_t* tiles,
                       int64_t n_tiles, int n_pairs, hipStream_t s) {
  feature_nn_kernel<DP><<<(unsigned)n_tiles, FN_THREADS, 0, s>>>(dist2, idx, queries, q_off, n_q, targets, t_off, n_t, dim,
                                                                 tiles, n_pairs);
}

}  // namespace

extern "C" int hfl_fpfh_radius_capped(float* r2, uint8_t* proven, int32_t* pending, int32_t* counter, int32_t* cell_starts,
                                      const float* sorted_points, const int64_t* sorted_keys,
                                      const hfl_knn_grid* grids_host, const hfl_knn_grid* grids, int batch, int64_t n_cells,
                                      const int64_t* cloud_offsets, int64_t n_points, float radius2, int radius_only,
                                      hfl_stream_t stream) {
  if (r2 == nullptr || proven == nullptr || pending == nullptr || counter == nullptr || cell_starts == nullptr ||
      sorted_points == nullptr || sorted_keys == nullptr || grids_host == nullptr || grids == nullptr ||
      cloud_offsets == nullptr || !knn_cap_ok(radius2))
    return HFL_EINVAL;
  int k_max = 0;
  if (const int rc = knn_call_check(batch, n_points, n_cells, grids_host, &k_max)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t n = n_points;
  if (const int rc = knn_launch_starts(cell_starts, counter, sorted_keys, n, n_cells, HFL_KNN_PHASE_ALL, s)) return rc;
  if (radius_only) {
    fpfh_radius_only_kernel<<<(unsigned)hfl_cdiv(n, kOutThreads), kOutThreads, 0, s>>>(
        r2, proven, pending, counter, sorted_points, sorted_keys, grids, cloud_offsets, batch, n, radius2);
    HFL_RETURN_LAST_ERROR();
  }
  return knn_dispatch_k(k_max, [&](auto kc) -> int {
    constexpr int K = decltype(kc)::value;
    fpfh_radius_kernel<K><<<(unsigned)hfl_cdiv(n, kOutThreads), kOutThreads, 0, s>>>(
        r2, proven, pending, counter, sorted_points, sorted_keys, cell_starts, grids, cloud_offsets, batch, n, radius2);
    fpfh_radius_fallback_kernel<K><<<knn_fallback_blocks(n, s), kOutThreads, 0, s>>>(
        r2, pending, counter, sorted_points, grids, cloud_offsets, batch, n, radius2);
    HFL_RETURN_LAST_ERROR();
  });
}

extern "C" int hfl_fpfh_radius(float* r2, uint8_t* proven, int32_t* pending, int32_t* counter, int32_t* cell_starts,
                               const float* sorted_points, const int64_t* sorted_keys, const hfl_knn_grid* grids_host,
                               const hfl_knn_grid* grids, int batch, int64_t n_cells, const int64_t* cloud_offsets,
                               int64_t n_points, hfl_stream_t stream) {
  return hfl_fpfh_radius_capped(r2, proven, pending, counter, cell_starts, sorted_points, sorted_keys, grids_host, grids,
                                batch, n_cells, cloud_offsets, n_points, INFINITY, 0, stream);
}

extern "C" int hfl_fpfh_spfh(int32_t* hist, int32_t* pairs, const float* r2, const uint8_t* proven, const int32_t* pending,
                             const int32_t* counter, const int32_t* cell_starts, const float* sorted_points,
                             const float* sorted_normals, const int64_t* sorted_keys, const hfl_knn_grid* grids_host,
                             const hfl_knn_grid* grids, int batch, int64_t n_cells, const int64_t* cloud_offsets,
                             int64_t n_points, const double* theta_table_host, hfl_stream_t stream) {
  if (hist == nullptr || pairs == nullptr || r2 == nullptr || proven == nullptr || pending == nullptr ||
      counter == nullptr || cell_starts == nullptr || sorted_points == nullptr || sorted_normals == nullptr ||
      sorted_keys == nullptr || grids_host == nullptr || grids == nullptr || cloud_offsets == nullptr ||
      theta_table_host == nullptr)
    return HFL_EINVAL;
  int k_max = 0;
  if (const int rc = knn_call_check(batch, n_points, n_cells, grids_host, &k_max)) return rc;
  ThetaTable tab;
  for (int k = 0; k < FP_EDGES; ++k) {                           // rows of (cos e_k, sin e_k)
    tab.c[k] = theta_table_host[2 * k];
    tab.s[k] = theta_table_host[2 * k + 1];
    if (!(tab.c[k] - tab.c[k] == 0.0) || !(tab.s[k] - tab.s[k] == 0.0)) return HFL_EINVAL;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  fpfh_spfh_kernel<<<(unsigned)hfl_cdiv(n_points, kOutThreads), kOutThreads, 0, s>>>(
      hist, pairs, r2, proven, sorted_points, sorted_normals, sorted_keys, cell_starts, grids, cloud_offsets, tab, batch,
      n_points);
  fpfh_spfh_fallback_kernel<<<knn_fallback_blocks(n_points, s), kOutThreads, 0, s>>>(
      hist, pairs, r2, pending, counter, sorted_points, sorted_normals, cloud_offsets, tab, batch, n_points);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int hfl_fpfh_combine(float* fpfh, const int32_t* hist, const int32_t* pairs, const float* r2,
                                const uint8_t* proven, const int32_t* pending, const int32_t* counter,
                                const int32_t* cell_starts, const float* sorted_points, const int64_t* sorted_keys,
                                const int64_t* perm, const hfl_knn_grid* grids_host, const hfl_knn_grid* grids, int batch,
                                int64_t n_cells, const int64_t* cloud_offsets, int64_t n_points, hfl_stream_t stream) {
  if (fpfh == nullptr || hist == nullptr || pairs == nullptr || r2 == nullptr || proven == nullptr || pending == nullptr ||
      counter == nullptr || cell_starts == nullptr || sorted_points == nullptr || sorted_keys == nullptr ||
      perm == nullptr || grids_host == nullptr || grids == nullptr || cloud_offsets == nullptr)
    return HFL_EINVAL;
  int k_max = 0;
  if (const int rc = knn_call_check(batch, n_points, n_cells, grids_host, &k_max)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  fpfh_combine_kernel<<<(unsigned)hfl_cdiv(n_points, kOutThreads), kOutThreads, 0, s>>>(
      fpfh, hist, pairs, r2, proven, sorted_points, sorted_keys, perm, cell_starts, grids, cloud_offsets, batch, n_points);
  fpfh_combine_fallback_kernel<<<knn_fallback_blocks(n_points, s), kOutThreads, 0, s>>>(
      fpfh, hist, pairs, r2, pending, counter, sorted_points, perm, cloud_offsets, batch, n_points);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int hfl_feature_nn(float* dist2, int32_t* idx, const float* queries, const int64_t* q_offsets, int64_t n_queries,
                              const float* targets, const int64_t* t_offsets, int64_t n_targets, int dim,
                              const int64_t* tiles, int64_t n_tiles, int64_t n_pairs, hfl_stream_t stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  return pair_scan_call({dist2, idx, queries, q_offsets, targets, t_offsets, tiles}, dim >= 1 && dim <= HFL_FEATURE_MAX_DIM,
                        n_queries, n_targets, n_tiles, n_pairs, [&] {
#define HFL_FEATURE_NN_CASE(DP)                                                                                        \
  if (dim <= DP)                                                                                                       \
    return feature_nn_launch<DP>(dist2, idx, queries, q_offsets, n_queries, targets, t_offsets, n_targets, dim, tiles, \
                                 n_tiles, (int)n_pairs, s);
    HFL_FEATURE_NN_CASE(4)
    HFL_FEATURE_NN_CASE(8)
    HFL_FEATURE_NN_CASE(16)
    HFL_FEATURE_NN_CASE(24)
    HFL_FEATURE_NN_CASE(36)
    HFL_FEATURE_NN_CASE(48)
    HFL_FEATURE_NN_CASE(64)                                      // dim <= HFL_FEATURE_MAX_DIM = 64: one of them launches
#undef HFL_FEATURE_NN_CASE
  });
}
