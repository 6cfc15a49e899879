// Surface normals and the surface variation of every point of a ragged batch of clouds: the covariance of the point's k
// nearest neighbours and its smallest eigenvector (open3d's estimate_normals with KDTreeSearchParamKNN, plus a curvature).
// The estimate is DEFINED in hotformerloc_amd/normals.py (module docstring) and DESIGN.md section 7j; this file and the
// numpy route there follow that definition.  The search is the exact grid search of knn_common.h, which csrc/outliers.hip
// and csrc/fpfh.hip run as well, on the batch that `outliers.sorted_batch` lays out; this file holds the accumulation on
// top of it.
//
//   hfl_knn_normals   (1) the dense cell-start table (knn_cell_starts_kernel); (2) one thread per point in sorted order
//                     scans the 3 x 3 x 3 block of cells round its own twice: the first scan keeps the K smallest fp32
//                     squared distances in the sorted register list and gives r2, the k-th smallest; when r2 lies strictly
//                     below the square of the conservative distance to the nearest face with cells behind it, every point
//                     with d2 <= r2 is in the block, and the second scan adds, in float64 and in sorted-position order, the
//                     count, sum e and sum e e^T of e = p_j - p_i over those points; else the point is appended to a list;
//                     (3) a wave per listed point scans the point's whole cloud twice: r2 by the merge of the 64 lists, then
//                     the sums, a lane's points in ascending order and the lanes by the xor butterfly 32 .. 1.
//                     Whoever holds the sums finishes: C = S2 / m - (S1 / m)(S1 / m)^T, a one-sided cyclic Jacobi of fixed
//                     sweep count, the eigenvalues in order, the degenerate rule, the sign rule, three stores at perm[j].
//
//   hfl_knn_normals_radius   the same with r2 = min(k-th smallest, R2) in both scans (hybrid), or, radius-only, r2 = R2 for
//                     every point: no list and no first scan -- one pass over the block where the bound proves that it
//                     holds every point within R2, one pass of a wave over the cloud for the others.
//
// The neighbourhood { j : d2(i, j) <= r2 } is a pure function of the input, so counts are the same for any grid; the
// float64 sums run in an order that follows the sort and the grid, fixed for given inputs: two runs give the same bits.  No
// floating-point atomics (one integer add per wave appends to the list); no workgroup waits for another.
#include <math.h>

#include "cov_eigen.h"
#include "knn_common.h"

namespace {

constexpr double NR_RANK_TOL = 1e-12;                            // middle eigenvalue <= this x the largest: no normal

// steps 3 to 7 of the definition for one point: from the sums over its m neighbours (`normal_add` and the eigenvalues are
// cov_eigen.h's) to the stores at `row`
__device__ void normal_finish(float* __restrict__ normals, float* __restrict__ curvature, int32_t* __restrict__ counts,
                              int64_t row, int64_t n, const double (&s)[NR_SUMS], int m, float px, float py, float pz,
                              const double* __restrict__ view) {
  if (row < 0 || row >= n) return;
  double nx = 0.0, ny = 0.0, nz = 0.0, curv = 0.0;
  if (m >= 3) {
    cov_eigen(s, m, [&](double l0, double l1, double l2, const double (&v)[3][3], int i0) {
      if (l1 > NR_RANK_TOL * l2) {                               // false for a NaN and for C = 0 as well
        nx = pick(v, 0, i0);
        ny = pick(v, 1, i0);
        nz = pick(v, 2, i0);
        const double sum = (l0 + l1) + l2;
        curv = sum > 0.0 ? l0 / sum : 0.0;
        // one number decides the sign in either mode: n . (viewpoint - p), or the first of n_z, n_y, n_x that is not zero
        double facing = nz != 0.0 ? nz : (ny != 0.0 ? ny : nx);
        if (view != nullptr)
          facing = (nx * (view[0] - (double)px) + ny * (view[1] - (double)py)) + nz * (view[2] - (double)pz);
        const double turn = facing < 0.0 ? -1.0 : 1.0;           // a product by +-1 is exact
        nx *= turn;
        ny *= turn;
        nz *= turn;
      }
    });
  }
  normals[row * 3 + 0] = (float)nx;
  normals[row * 3 + 1] = (float)ny;
  normals[row * 3 + 2] = (float)nz;
  curvature[row] = (float)curv;
  counts[row] = m;
}

// the second scan of a resolved point: the sums over every point of its block with d2 <= r2, in sorted-position order
__device__ __forceinline__ void normal_block_sums(float* __restrict__ normals, float* __restrict__ curvature,
                                                  int32_t* __restrict__ counts, const KnnPoint& p, const KnnFirst& f,
                                                  const float* __restrict__ spts, int64_t row,
                                                  const int32_t* __restrict__ starts, const double* __restrict__ views,
                                                  int64_t n) {
  double sums[NR_SUMS];
#pragma unroll
  for (int i = 0; i < NR_SUMS; ++i) sums[i] = 0.0;
  int m = 0;
  knn_block_scan(p.g, f.blk, starts, p.first, p.last, [&](int32_t q) {
    const float* w = spts + (int64_t)q * 3;
    if (knn_d2(p.px, p.py, p.pz, w) <= f.r2) {
      normal_add(sums, p.px, p.py, p.pz, w);
      ++m;
    }
  });
  normal_finish(normals, curvature, counts, row, n, sums, m, p.px, p.py, p.pz,
                views != nullptr ? views + 3 * (int64_t)p.c : nullptr);
}

// the second scan of a pending point by its wave: the same sums over the whole cloud, a lane's points in ascending order and
// the lanes by the xor butterfly 32 .. 1; lane 0 finishes
__device__ __forceinline__ void normal_cloud_sums(float* __restrict__ normals, float* __restrict__ curvature,
                                                  int32_t* __restrict__ counts, float px, float py, float pz, float r2,
                                                  const float* __restrict__ spts, int64_t row, int64_t first, int64_t last,
                                                  const double* __restrict__ view, int64_t n) {
  double sums[NR_SUMS];
#pragma unroll
  for (int i = 0; i < NR_SUMS; ++i) sums[i] = 0.0;
  int m = 0;
  knn_cloud_scan(first, last, [&](int64_t q) {
    const float* w = spts + q * 3;
    if (knn_d2(px, py, pz, w) <= r2) {
      normal_add(sums, px, py, pz, w);
      ++m;
    }
  });
#pragma unroll
  for (int i = 0; i < NR_SUMS; ++i) sums[i] = wave_sum(sums[i]);
  m = wave_sum(m);
  if (knn_lane() == 0) normal_finish(normals, curvature, counts, row, n, sums, m, px, py, pz, view);
}

template <int K>
__global__ void __launch_bounds__(kOutThreads)
normals_query_kernel(float* __restrict__ normals, float* __restrict__ curvature, int32_t* __restrict__ counts,
                     int32_t* __restrict__ pending, int32_t* __restrict__ counter, const float* __restrict__ spts,
                     const int64_t* __restrict__ skeys, const int64_t* __restrict__ perm, const int32_t* __restrict__ starts,
                     const hfl_knn_grid* __restrict__ grids, const int64_t* __restrict__ off, const double* __restrict__ views,
                     int batch, int64_t n, float cap) {
  const int64_t j = (int64_t)blockIdx.x * kOutThreads + threadIdx.x;
  if (j >= n) return;
  const KnnPoint p = knn_point(spts, skeys, grids, off, batch, n, j);
  KnnList<K> list;
  const KnnFirst f = knn_first_scan(list, p, spts, starts, cap);
  if (f.resolved) {                                            // the list is dead from here on: the sums take its registers
    normal_block_sums(normals, curvature, counts, p, f, spts, perm[j], starts, views, n);
  } else {
    knn_append_pending(pending, counter, j, n);
  }
}

// r2 = cap for every point: no list, no first scan
__global__ void __launch_bounds__(kOutThreads)
normals_radius_query_kernel(float* __restrict__ normals, float* __restrict__ curvature, int32_t* __restrict__ counts,
                            int32_t* __restrict__ pending, int32_t* __restrict__ counter, const float* __restrict__ spts,
                            const int64_t* __restrict__ skeys, const int64_t* __restrict__ perm,
                            const int32_t* __restrict__ starts, const hfl_knn_grid* __restrict__ grids,
                            const int64_t* __restrict__ off, const double* __restrict__ views, int batch, int64_t n,
                            float cap) {
  const int64_t j = (int64_t)blockIdx.x * kOutThreads + threadIdx.x;
  if (j >= n) return;
  const KnnPoint p = knn_point(spts, skeys, grids, off, batch, n, j);
  const KnnFirst f = knn_radius_first(p, cap);
  if (f.resolved) {
    normal_block_sums(normals, curvature, counts, p, f, spts, perm[j], starts, views, n);
  } else {
    knn_append_pending(pending, counter, j, n);
  }
}

template <int K>
__global__ void __launch_bounds__(kOutThreads)
normals_fallback_kernel(float* __restrict__ normals, float* __restrict__ curvature, int32_t* __restrict__ counts,
                        const int32_t* __restrict__ pending, const int32_t* __restrict__ counter,
                        const float* __restrict__ spts, const int64_t* __restrict__ perm,
                        const hfl_knn_grid* __restrict__ grids, const int64_t* __restrict__ off,
                        const double* __restrict__ views, int batch, int64_t n, float cap) {
  knn_for_pending(pending, counter, off, batch, n, [&](int64_t j, int c, int64_t first, int64_t last) {
    const int k = min(max(grids[c].k, 1), K);
    const float px = spts[j * 3 + 0], py = spts[j * 3 + 1], pz = spts[j * 3 + 2];
    float r2;
    {
      KnnList<K> list;
      knn_cloud_first(list, px, py, pz, spts, first, last);
      r2 = knn_wave_kth(list, k, cap);
    }
    normal_cloud_sums(normals, curvature, counts, px, py, pz, r2, spts, perm[j], first, last,
                      views != nullptr ? views + 3 * (int64_t)c : nullptr, n);
  });
}

__global__ void __launch_bounds__(kOutThreads)
normals_radius_fallback_kernel(float* __restrict__ normals, float* __restrict__ curvature, int32_t* __restrict__ counts,
                               const int32_t* __restrict__ pending, const int32_t* __restrict__ counter,
                               const float* __restrict__ spts, const int64_t* __restrict__ perm,
                               const int64_t* __restrict__ off, const double* __restrict__ views, int batch, int64_t n,
                               float cap) {
  knn_for_pending(pending, counter, off, batch, n, [&](int64_t j, int c, int64_t first, int64_t last) {
    normal_cloud_sums(normals, curvature, counts, spts[j * 3 + 0], spts[j * 3 + 1], spts[j * 3 + 2], cap, spts, perm[j],
                      first, last, views != nullptr ? views + 3 * (int64_t)c : nullptr, n);
  });
}

}  // namespace

extern "C" int hfl_knn_normals_radius(float* normals, float* curvature, int32_t* counts, int32_t* pending,
                                      int32_t* counter, int32_t* cell_starts, const float* sorted_points,
                                      const int64_t* sorted_keys, const int64_t* perm, const hfl_knn_grid* grids_host,
                                      const hfl_knn_grid* grids, int batch, int64_t n_cells, const int64_t* cloud_offsets,
                                      int64_t n_points, const double* viewpoints, float radius2, int radius_only,
                                      int phases, hfl_stream_t stream) {
  if (normals == nullptr || curvature == nullptr || counts == nullptr || pending == nullptr || counter == nullptr ||
      cell_starts == nullptr || sorted_points == nullptr || sorted_keys == nullptr || perm == nullptr ||
      grids_host == nullptr || grids == nullptr || cloud_offsets == nullptr)
    return HFL_EINVAL;
  if (phases < 1 || phases > HFL_KNN_PHASE_ALL || !knn_cap_ok(radius2)) return HFL_EINVAL;
  int k_max = 0;
  if (const int rc = knn_call_check(batch, n_points, n_cells, grids_host, &k_max)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t n = n_points;
  if (const int rc = knn_launch_starts(cell_starts, counter, sorted_keys, n, n_cells, phases, s)) return rc;
  if (radius_only) {
    if (phases & HFL_KNN_PHASE_QUERY)
      normals_radius_query_kernel<<<(unsigned)hfl_cdiv(n, kOutThreads), kOutThreads, 0, s>>>(
          normals, curvature, counts, pending, counter, sorted_points, sorted_keys, perm, cell_starts, grids, cloud_offsets,
          viewpoints, batch, n, radius2);
    if (phases & HFL_KNN_PHASE_FALLBACK)
      normals_radius_fallback_kernel<<<knn_fallback_blocks(n, s), kOutThreads, 0, s>>>(
          normals, curvature, counts, pending, counter, sorted_points, perm, cloud_offsets, viewpoints, batch, n, radius2);
    HFL_RETURN_LAST_ERROR();
  }
  return knn_dispatch_k(k_max, [&](auto kc) -> int {
    constexpr int K = decltype(kc)::value;
    if (phases & HFL_KNN_PHASE_QUERY)
      normals_query_kernel<K><<<(unsigned)hfl_cdiv(n, kOutThreads), kOutThreads, 0, s>>>(
          normals, curvature, counts, pending, counter, sorted_points, sorted_keys, perm, cell_starts, grids, cloud_offsets,
          viewpoints, batch, n, radius2);
    if (phases & HFL_KNN_PHASE_FALLBACK)
      normals_fallback_kernel<K><<<knn_fallback_blocks(n, s), kOutThreads, 0, s>>>(
          normals, curvature, counts, pending, counter, sorted_points, perm, grids, cloud_offsets, viewpoints, batch, n,
          radius2);
    HFL_RETURN_LAST_ERROR();
  });
}

extern "C" int hfl_knn_normals(float* normals, float* curvature, int32_t* counts, int32_t* pending, int32_t* counter,
                               int32_t* cell_starts, const float* sorted_points, const int64_t* sorted_keys,
                               const int64_t* perm, const hfl_knn_grid* grids_host, const hfl_knn_grid* grids, int batch,
                               int64_t n_cells, const int64_t* cloud_offsets, int64_t n_points, const double* viewpoints,
                               int phases, hfl_stream_t stream) {
  return hfl_knn_normals_radius(normals, curvature, counts, pending, counter, cell_starts, sorted_points, sorted_keys, perm,
                                grids_host, grids, batch, n_cells, cloud_offsets, n_points, viewpoints, INFINITY, 0, phases,
                                stream);
}
