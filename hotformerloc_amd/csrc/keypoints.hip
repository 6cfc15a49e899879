// Intrinsic Shape Signatures keypoints (Zhong 2009; open3d's compute_iss_keypoints) for a ragged batch of clouds: the few
// points where the surface bends in all three directions, for the descriptor matcher to work on instead of every point.
// The detector is DEFINED in hotformerloc_amd/keypoints.py (module docstring) and DESIGN.md section 7t; this file and the
// numpy route there follow that definition.  Both launches are radius-only searches of knn_common.h on ONE batch that
// `outliers.sorted_batch` lays out for the larger of the two radii: `knn_radius_first` proves a block per cap, so the grid
// serves the smaller radius as well.
//
//   hfl_iss_saliency   one thread per point in sorted order: where the bound proves that the 3 x 3 x 3 block holds every
//                      point within R2s, one pass over the block adds, in float64 and in sorted-position order, the count,
//                      sum e and sum e e^T of e = p_j - p_i; else the point is appended to a list and a wave scans its whole
//                      cloud, a lane's points in ascending order and the lanes by the xor butterfly 32 .. 1.  Whoever holds
//                      the sums finishes: the ordered eigenvalues of cov_eigen.h (the covariance and Jacobi of
//                      csrc/normals.hip), the two ratio tests in float64 products, the saliency float(l0) or 0, stored at the
//                      sorted position for hfl_iss_select and at perm[j] for the caller, the count at perm[j].
//   hfl_iss_select     one thread per point in sorted order.  A point whose saliency is not > 0 writes 0 and returns.  A
//                      candidate scans its block within R2n, counts, and stops at the first neighbour that beats it (a
//                      larger saliency, or an equal one at a lower input row: `perm` decides ties); a candidate whose block
//                      is not proven goes to a wave over its cloud, the lanes' "beaten" flags combined by a ballot, the
//                      counts by `wave_sum`.  One mask byte at perm[j].
//
// The saliency is rounded to fp32 before anything compares it, and the selection uses integers and comparisons only: the
// mask is a pure function of the points and the fp32 saliency, the same for any grid.  The float64 sums run in an order that
// follows the sort and the grid, fixed for given inputs: two runs give the same bits.  No LDS, no floating-point atomics
// (one integer add per wave appends to the list); no workgroup waits for another.
#include <math.h>

#include "cov_eigen.h"
#include "knn_common.h"

namespace {

// what the definition asks of a neighbourhood beyond `min_neighbors`: fewer than three points have no eigenvalues
constexpr int ISS_MIN_POINTS = 3;

struct IssParams {
  double gamma_21, gamma_32;
  int min_neighbors;
};

// steps 3 and 4 of the definition for the point at sorted position j: from the sums over its m neighbours to the stores
__device__ void saliency_finish(float* __restrict__ saliency, float* __restrict__ sorted_saliency, int32_t* __restrict__ counts,
                                int64_t j, int64_t row, int64_t n, const double (&s)[NR_SUMS], int m, const IssParams& prm) {
  float value = 0.f;
  if (m >= prm.min_neighbors && m >= ISS_MIN_POINTS) {
    cov_eigen(s, m, [&](double l0, double l1, double l2, const double (&)[3][3], int) {
      if (l1 < prm.gamma_21 * l2 && l0 < prm.gamma_32 * l1) value = (float)l0;              // false for a NaN
    });
  }
  sorted_saliency[j] = value;
  if (row < 0 || row >= n) return;
  saliency[row] = value;
  counts[row] = m;
}

__global__ void __launch_bounds__(kOutThreads)
iss_saliency_query_kernel(float* __restrict__ saliency, float* __restrict__ sorted_saliency, int32_t* __restrict__ counts,
                          int32_t* __restrict__ pending, int32_t* __restrict__ counter, const float* __restrict__ spts,
                          const int64_t* __restrict__ skeys, const int64_t* __restrict__ perm,
                          const int32_t* __restrict__ starts, const hfl_knn_grid* __restrict__ grids,
                          const int64_t* __restrict__ off, int batch, int64_t n, float cap, IssParams prm) {
  const int64_t j = (int64_t)blockIdx.x * kOutThreads + threadIdx.x;
  if (j >= n) return;
  const KnnPoint p = knn_point(spts, skeys, grids, off, batch, n, j);
  const KnnFirst f = knn_radius_first(p, cap);
  if (f.resolved) {
    double sums[NR_SUMS];
#pragma unroll
    for (int i = 0; i < NR_SUMS; ++i) sums[i] = 0.0;
    int m = 0;
    knn_block_scan(p.g, f.blk, starts, p.first, p.last, [&](int32_t q) {
      const float* w = spts + (int64_t)q * 3;
      if (knn_d2(p.px, p.py, p.pz, w) <= cap) {
        normal_add(sums, p.px, p.py, p.pz, w);
        ++m;
      }
    });
    saliency_finish(saliency, sorted_saliency, counts, j, perm[j], n, sums, m, prm);
  } else {
    knn_append_pending(pending, counter, j, n);
  }
}

__global__ void __launch_bounds__(kOutThreads)
iss_saliency_fallback_kernel(float* __restrict__ saliency, float* __restrict__ sorted_saliency, int32_t* __restrict__ counts,
                             const int32_t* __restrict__ pending, const int32_t* __restrict__ counter,
                             const float* __restrict__ spts, const int64_t* __restrict__ perm,
                             const int64_t* __restrict__ off, int batch, int64_t n, float cap, IssParams prm) {
  knn_for_pending(pending, counter, off, batch, n, [&](int64_t j, int, int64_t first, int64_t last) {
    const float px = spts[j * 3 + 0], py = spts[j * 3 + 1], pz = spts[j * 3 + 2];
    double sums[NR_SUMS];
#pragma unroll
    for (int i = 0; i < NR_SUMS; ++i) sums[i] = 0.0;
    int m = 0;
    knn_cloud_scan(first, last, [&](int64_t q) {
      const float* w = spts + q * 3;
      if (knn_d2(px, py, pz, w) <= cap) {
        normal_add(sums, px, py, pz, w);
        ++m;
      }
    });
#pragma unroll
    for (int i = 0; i < NR_SUMS; ++i) sums[i] = wave_sum(sums[i]);
    m = wave_sum(m);
    if (knn_lane() == 0) saliency_finish(saliency, sorted_saliency, counts, j, perm[j], n, sums, m, prm);
  });
}

// does the point at sorted position q, with saliency sq, beat a candidate of saliency s at input row `row`?
__device__ __forceinline__ bool iss_beats(float sq, float s, int64_t q, int64_t row, const int64_t* __restrict__ perm) {
  return sq > s || (sq == s && perm[q] < row);                  // the candidate itself: equal, and its row not below
}

__global__ void __launch_bounds__(kOutThreads)
iss_select_query_kernel(uint8_t* __restrict__ mask, int32_t* __restrict__ pending, int32_t* __restrict__ counter,
                        const float* __restrict__ spts, const int64_t* __restrict__ skeys, const int64_t* __restrict__ perm,
                        const float* __restrict__ ssal, const int32_t* __restrict__ starts,
                        const hfl_knn_grid* __restrict__ grids, const int64_t* __restrict__ off, int batch, int64_t n,
                        float cap, int min_neighbors) {
  const int64_t j = (int64_t)blockIdx.x * kOutThreads + threadIdx.x;
  if (j >= n) return;
  const int64_t row = perm[j];
  if (row < 0 || row >= n) return;
  const float s = ssal[j];
  if (!(s > 0.f)) {                                              // most points: no candidate (a NaN neither)
    mask[row] = 0;
    return;
  }
  const KnnPoint p = knn_point(spts, skeys, grids, off, batch, n, j);
  const KnnFirst f = knn_radius_first(p, cap);
  if (f.resolved) {
    // `knn_block_scan` with a way out: the first neighbour that beats the candidate ends it
    int m = 0;
    bool beaten = false;
#pragma unroll 1
    for (int z = f.blk.z0; z <= f.blk.z1 && !beaten; ++z)
#pragma unroll 1
      for (int y = f.blk.y0; y <= f.blk.y1 && !beaten; ++y) {
        const int64_t line = p.g.cell_base + ((int64_t)z * p.g.ny + y) * p.g.nx;
        const int32_t b = max(starts[line + f.blk.x0], p.first), e = min(starts[line + f.blk.x1 + 1], p.last);
#pragma unroll 1
        for (int32_t q = b; q < e && !beaten; ++q)
          if (knn_d2(p.px, p.py, p.pz, spts + (int64_t)q * 3) <= cap) {
            ++m;
            beaten = iss_beats(ssal[q], s, q, row, perm);
          }
      }
    mask[row] = (!beaten && m >= min_neighbors) ? 1 : 0;
  } else {
    knn_append_pending(pending, counter, j, n);
  }
}

__global__ void __launch_bounds__(kOutThreads)
iss_select_fallback_kernel(uint8_t* __restrict__ mask, const int32_t* __restrict__ pending,
                           const int32_t* __restrict__ counter, const float* __restrict__ spts,
                           const int64_t* __restrict__ perm, const float* __restrict__ ssal, const int64_t* __restrict__ off,
                           int batch, int64_t n, float cap, int min_neighbors) {
  knn_for_pending(pending, counter, off, batch, n, [&](int64_t j, int, int64_t first, int64_t last) {
    const float px = spts[j * 3 + 0], py = spts[j * 3 + 1], pz = spts[j * 3 + 2];
    const float s = ssal[j];
    const int64_t row = perm[j];
    int m = 0;
    bool beaten = false;
    knn_cloud_scan(first, last, [&](int64_t q) {
      if (knn_d2(px, py, pz, spts + q * 3) <= cap) {
        ++m;
        beaten = beaten || iss_beats(ssal[q], s, q, row, perm);
      }
    });
    const bool any_beaten = __ballot(beaten) != 0ull;
    m = wave_sum(m);                                             // integers: any order gives the same sum
    if (knn_lane() == 0 && row >= 0 && row < n) mask[row] = (!any_beaten && m >= min_neighbors) ? 1 : 0;
  });
}

bool iss_gamma_ok(double g) { return g > 0.0 && g <= 1.0; }

}  // namespace

extern "C" int hfl_iss_saliency(float* saliency, float* sorted_saliency, int32_t* counts, int32_t* pending, int32_t* counter,
                                int32_t* cell_starts, const float* sorted_points, const int64_t* sorted_keys,
                                const int64_t* perm, const hfl_knn_grid* grids_host, const hfl_knn_grid* grids, int batch,
                                int64_t n_cells, const int64_t* cloud_offsets, int64_t n_points, float radius2, double gamma_21,
                                double gamma_32, int min_neighbors, int phases, hfl_stream_t stream) {
  if (saliency == nullptr || sorted_saliency == nullptr || counts == nullptr || pending == nullptr || counter == nullptr ||
      cell_starts == nullptr || sorted_points == nullptr || sorted_keys == nullptr || perm == nullptr ||
      grids_host == nullptr || grids == nullptr || cloud_offsets == nullptr)
    return HFL_EINVAL;
  if (phases < 1 || phases > HFL_KNN_PHASE_ALL || !knn_cap_ok(radius2)) return HFL_EINVAL;
  if (!iss_gamma_ok(gamma_21) || !iss_gamma_ok(gamma_32) || min_neighbors < 1) return HFL_EINVAL;
  int k_max = 0;
  if (const int rc = knn_call_check(batch, n_points, n_cells, grids_host, &k_max)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t n = n_points;
  const IssParams prm = {gamma_21, gamma_32, min_neighbors};
  if (const int rc = knn_launch_starts(cell_starts, counter, sorted_keys, n, n_cells, phases, s)) return rc;
  if (phases & HFL_KNN_PHASE_QUERY)
    iss_saliency_query_kernel<<<(unsigned)hfl_cdiv(n, kOutThreads), kOutThreads, 0, s>>>(
        saliency, sorted_saliency, counts, pending, counter, sorted_points, sorted_keys, perm, cell_starts, grids,
        cloud_offsets, batch, n, radius2, prm);
  if (phases & HFL_KNN_PHASE_FALLBACK)
    iss_saliency_fallback_kernel<<<knn_fallback_blocks(n, s), kOutThreads, 0, s>>>(
        saliency, sorted_saliency, counts, pending, counter, sorted_points, perm, cloud_offsets, batch, n, radius2, prm);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int hfl_iss_select(uint8_t* mask, int32_t* pending, int32_t* counter, int32_t* cell_starts,
                              const float* sorted_points, const int64_t* sorted_keys, const int64_t* perm,
                              const float* sorted_saliency, const hfl_knn_grid* grids_host, const hfl_knn_grid* grids,
                              int batch, int64_t n_cells, const int64_t* cloud_offsets, int64_t n_points, float radius2,
                              int min_neighbors, int phases, hfl_stream_t stream) {
  if (mask == nullptr || pending == nullptr || counter == nullptr || cell_starts == nullptr || sorted_points == nullptr ||
      sorted_keys == nullptr || perm == nullptr || sorted_saliency == nullptr || grids_host == nullptr || grids == nullptr ||
      cloud_offsets == nullptr)
    return HFL_EINVAL;
  if (phases < 1 || phases > HFL_KNN_PHASE_ALL || !knn_cap_ok(radius2) || min_neighbors < 1) return HFL_EINVAL;
  int k_max = 0;
  if (const int rc = knn_call_check(batch, n_points, n_cells, grids_host, &k_max)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t n = n_points;
  if (const int rc = knn_launch_starts(cell_starts, counter, sorted_keys, n, n_cells, phases, s)) return rc;
  if (phases & HFL_KNN_PHASE_QUERY)
    iss_select_query_kernel<<<(unsigned)hfl_cdiv(n, kOutThreads), kOutThreads, 0, s>>>(
        mask, pending, counter, sorted_points, sorted_keys, perm, sorted_saliency, cell_starts, grids, cloud_offsets, batch, n,
        radius2, min_neighbors);
  if (phases & HFL_KNN_PHASE_FALLBACK)
    iss_select_fallback_kernel<<<knn_fallback_blocks(n, s), kOutThreads, 0, s>>>(
        mask, pending, counter, sorted_points, perm, sorted_saliency, cloud_offsets, batch, n, radius2, min_neighbors);
  HFL_RETURN_LAST_ERROR();
}
