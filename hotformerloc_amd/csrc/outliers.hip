// Statistical outlier removal and the radius trim for raw submaps, batched and ragged on the device: the cleaning steps in
// front of the CS-Wild-Places post-processing (datasets/CSWildPlaces/processing_utils.py remove_outliers, i.e. open3d's
// remove_statistical_outlier, and the radius cut of postprocess_wildplaces_ground.py).  The filter is DEFINED in
// hotformerloc_amd/outliers.py (module docstring) and DESIGN.md section 7g; this file and the numpy route there follow that
// definition operation for operation, every operation rounded once (the file is built with -ffp-contract=off), so the two
// agree to the bit.
//
//   hfl_cloud_nonfinite    flags[b] = 1 when cloud b holds a coordinate that is not finite (integer OR)
//   hfl_knn_cell_keys      one int64 key per point: the cloud's first cell + (iz ny + iy) nx + ix on the cloud's uniform grid
//   hfl_knn_mean_dist      the mean distance to the k nearest points of the own cloud, the point itself included, exact:
//                          (1) a dense cell-start table by one binary search per cell over the sorted keys; (2) one thread
//                          per point in sorted order scans the 3 x 3 x 3 block of cells round its own and keeps the K
//                          smallest squared distances in a sorted register list; the point is resolved when its k-th smallest
//                          is strictly below the square of a conservative distance to the nearest face of the block that has
//                          cells behind it, else it is appended to a list; (3) a wave per listed point scans the point's
//                          whole cloud, a list per lane, and merges the 64 lists by k rounds of a wave minimum
//   hfl_knn_radius_count   counts = the number of points of the own cloud with d2 <= R2, the point itself included (open3d's
//                          remove_radius_outlier counts the same set): no list and no first scan -- one thread per point
//                          counts over its 3 x 3 x 3 block where the bound proves that the block holds every point within
//                          R2, a wave per other point over its whole cloud.  An integer: the same for any grid.
//   hfl_count_mask         keep = counts > nb_points
//   hfl_outlier_threshold  per cloud, in float64 in the order of hfl_pair_stats: mean, std, mean + ratio std, n_valid
//   hfl_outlier_mask       keep = avg > 0 and double(avg) < threshold
//   hfl_radius_mask        keep = sqrt(x x + y y) <= radius_max in float64
//
// The search of (1) to (3) is written in knn_common.h, for this file, csrc/normals.hip and csrc/fpfh.hip; here is what is
// done with the k smallest distances.  The answer of (2) and (3) is a pure function of the multiset of the k smallest
// squared distances, which both find exactly, so it does not depend on the cell size, on which of the two resolved a point,
// or on the order of the list.  No floating-point atomics (one integer add per wave appends to the list); no workgroup
// waits for another.
#include <math.h>

#include "knn_common.h"

namespace {

__global__ void __launch_bounds__(kOutThreads)
cloud_nonfinite_kernel(int32_t* __restrict__ flags, const float* __restrict__ pts, const int64_t* __restrict__ off, int batch,
                       int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kOutThreads + threadIdx.x;
  if (i >= n) return;
  const float x = pts[i * 3 + 0], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
  if (!(x - x == 0.f) || !(y - y == 0.f) || !(z - z == 0.f)) atomicOr(flags + find_cloud(off, batch, i), 1);
}

// int((p - origin) / cell) clamped into [0, top]; what is not >= 0 gives 0
__device__ __forceinline__ int knn_cell(float p, float origin, float cell, int top) {
  const float f = __fdiv_rn(__fsub_rn(p, origin), cell);
  if (!(f >= 0.f)) return 0;
  if (f >= 2147483520.f) return top;                         // the largest float an int holds
  return min((int)f, top);                                   // compared as integers: (float)top may round up
}

__global__ void __launch_bounds__(kOutThreads)
knn_cell_keys_kernel(int64_t* __restrict__ keys, const hfl_knn_grid* __restrict__ grids, const float* __restrict__ pts,
                     const int64_t* __restrict__ off, int batch, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kOutThreads + threadIdx.x;
  if (i >= n) return;
  const hfl_knn_grid g = grids[find_cloud(off, batch, i)];
  const int ix = knn_cell(pts[i * 3 + 0], g.ox, g.cell, g.nx - 1);
  const int iy = knn_cell(pts[i * 3 + 1], g.oy, g.cell, g.ny - 1);
  const int iz = knn_cell(pts[i * 3 + 2], g.oz, g.cell, g.nz - 1);
  keys[i] = g.cell_base + ((int64_t)iz * g.ny + iy) * g.nx + ix;
}

// The correctly rounded fp32 root.  Not __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS the HIP headers map that name to the
// native approximation, which is an ulp off now and then; sqrtf is correctly rounded (hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt), and so is the plain fp32 division behind __fdiv_rn.
__device__ __forceinline__ float knn_sqrt(float x) { return __builtin_sqrtf(x); }

template <int K>
__global__ void __launch_bounds__(kOutThreads)
knn_query_kernel(float* __restrict__ avg, int32_t* __restrict__ pending, int32_t* __restrict__ counter,
                 const float* __restrict__ spts, const int64_t* __restrict__ skeys, const int64_t* __restrict__ perm,
                 const int32_t* __restrict__ starts, const hfl_knn_grid* __restrict__ grids, const int64_t* __restrict__ off,
                 int batch, int64_t n) {
  const int64_t j = (int64_t)blockIdx.x * kOutThreads + threadIdx.x;
  if (j >= n) return;
  const KnnPoint p = knn_point(spts, skeys, grids, off, batch, n, j);
  const int64_t row = perm[j];
  const int k = p.g.k;
  KnnList<K> list;
  if (knn_first_scan(list, p, spts, starts).resolved) {
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < K; ++i)
      if (i < k) sum = __fadd_rn(sum, knn_sqrt(list.v[i]));
    if (row >= 0 && row < n) avg[row] = __fdiv_rn(sum, (float)k);
  } else {
    knn_append_pending(pending, counter, j, n);
  }
}

template <int K>
__global__ void __launch_bounds__(kOutThreads)
knn_fallback_kernel(float* __restrict__ avg, const int32_t* __restrict__ pending, const int32_t* __restrict__ counter,
                    const float* __restrict__ spts, const int64_t* __restrict__ perm, const hfl_knn_grid* __restrict__ grids,
                    const int64_t* __restrict__ off, int batch, int64_t n) {
  knn_for_pending(pending, counter, off, batch, n, [&](int64_t j, int c, int64_t first, int64_t last) {
    const int k = min(max(grids[c].k, 1), K);
    const float px = spts[j * 3 + 0], py = spts[j * 3 + 1], pz = spts[j * 3 + 2];
    KnnList<K> list;
    knn_cloud_first(list, px, py, pz, spts, first, last);
    float sum = 0.f;
    knn_wave_merge(list, k, [&](float m) { sum = __fadd_rn(sum, knn_sqrt(m)); });      // ascending
    const int64_t row = perm[j];
    if (knn_lane() == 0 && row >= 0 && row < n) avg[row] = __fdiv_rn(sum, (float)k);
  });
}

__global__ void __launch_bounds__(kOutThreads)
radius_count_kernel(int32_t* __restrict__ counts, int32_t* __restrict__ pending, int32_t* __restrict__ counter,
                    const float* __restrict__ spts, const int64_t* __restrict__ skeys, const int64_t* __restrict__ perm,
                    const int32_t* __restrict__ starts, const hfl_knn_grid* __restrict__ grids,
                    const int64_t* __restrict__ off, int batch, int64_t n, float cap) {
  const int64_t j = (int64_t)blockIdx.x * kOutThreads + threadIdx.x;
  if (j >= n) return;
  const KnnPoint p = knn_point(spts, skeys, grids, off, batch, n, j);
  const KnnFirst f = knn_radius_first(p, cap);
  if (f.resolved) {
    int m = 0;
    knn_block_scan(p.g, f.blk, starts, p.first, p.last,
                   [&](int32_t q) { m += knn_d2(p.px, p.py, p.pz, spts + (int64_t)q * 3) <= cap ? 1 : 0; });
    const int64_t row = perm[j];
    if (row >= 0 && row < n) counts[row] = m;
  } else {
    knn_append_pending(pending, counter, j, n);
  }
}

__global__ void __launch_bounds__(kOutThreads)
radius_count_fallback_kernel(int32_t* __restrict__ counts, const int32_t* __restrict__ pending,
                             const int32_t* __restrict__ counter, const float* __restrict__ spts,
                             const int64_t* __restrict__ perm, const int64_t* __restrict__ off, int batch, int64_t n,
                             float cap) {
  knn_for_pending(pending, counter, off, batch, n, [&](int64_t j, int, int64_t first, int64_t last) {
    const float px = spts[j * 3 + 0], py = spts[j * 3 + 1], pz = spts[j * 3 + 2];
    int m = 0;
    knn_cloud_scan(first, last, [&](int64_t q) { m += knn_d2(px, py, pz, spts + q * 3) <= cap ? 1 : 0; });
    m = wave_sum(m);                                           // integers: any order gives the same sum
    const int64_t row = perm[j];
    if (knn_lane() == 0 && row >= 0 && row < n) counts[row] = m;
  });
}

__global__ void __launch_bounds__(kOutThreads)
count_mask_kernel(uint8_t* __restrict__ keep, const int32_t* __restrict__ counts, int64_t n, int32_t nb_points) {
  const int64_t i = (int64_t)blockIdx.x * kOutThreads + threadIdx.x;
  if (i < n) keep[i] = counts[i] > nb_points ? 1 : 0;
}

// the sums below are `block_sum` of ragged_common.h, the order of hfl_pair_stats: a thread's rows in ascending order, the
// xor butterfly 32 .. 1 in a wave, the waves in wave order; the same value in every thread
__global__ void __launch_bounds__(kOutThreads)
outlier_threshold_kernel(double* __restrict__ stats, const float* __restrict__ avg, const int64_t* __restrict__ off,
                         int64_t n, double ratio) {
  __shared__ double s_part[kOutWaves];
  const int b = blockIdx.x;
  const int64_t begin = max(off[b], (int64_t)0), end = min(off[b + 1], n);
  double sum = 0.0, cnt = 0.0;
  for (int64_t i = begin + threadIdx.x; i < end; i += kOutThreads) {
    const float a = avg[i];
    if (a > 0.f) { sum += (double)a; cnt += 1.0; }
  }
  sum = block_sum<kOutThreads>(sum, s_part);
  cnt = block_sum<kOutThreads>(cnt, s_part);                   // whole numbers below 2^53: exact in any order
  const double mean = __ddiv_rn(sum, cnt);                     // 0 / 0 = NaN for a cloud without a valid point
  double ss = 0.0;
  for (int64_t i = begin + threadIdx.x; i < end; i += kOutThreads) {
    const float a = avg[i];
    if (a > 0.f) {
      const double d = __dsub_rn((double)a, mean);
      ss += __dmul_rn(d, d);
    }
  }
  ss = block_sum<kOutThreads>(ss, s_part);
  if (threadIdx.x == 0) {
    const double sd = __dsqrt_rn(__ddiv_rn(ss, __dsub_rn(cnt, 1.0)));      // 0 / 0 = NaN for a single valid point
    stats[4 * (int64_t)b + 0] = mean;
    stats[4 * (int64_t)b + 1] = sd;
    stats[4 * (int64_t)b + 2] = __dadd_rn(mean, __dmul_rn(ratio, sd));
    stats[4 * (int64_t)b + 3] = cnt;
  }
}

__global__ void __launch_bounds__(kOutThreads)
outlier_mask_kernel(uint8_t* __restrict__ keep, const float* __restrict__ avg, const double* __restrict__ stats,
                    const int64_t* __restrict__ off, int batch, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kOutThreads + threadIdx.x;
  if (i >= n) return;
  const float a = avg[i];
  const double threshold = stats[4 * (int64_t)find_cloud(off, batch, i) + 2];
  keep[i] = (a > 0.f && (double)a < threshold) ? 1 : 0;        // a NaN threshold keeps nothing
}

__global__ void __launch_bounds__(kOutThreads)
radius_mask_kernel(uint8_t* __restrict__ keep, const float* __restrict__ pts, int64_t n, double radius) {
  const int64_t i = (int64_t)blockIdx.x * kOutThreads + threadIdx.x;
  if (i >= n) return;
  const double x = (double)pts[i * 3 + 0], y = (double)pts[i * 3 + 1];
  keep[i] = __dsqrt_rn(__dadd_rn(__dmul_rn(x, x), __dmul_rn(y, y))) <= radius ? 1 : 0;
}

bool out_batch_ok(int batch, int64_t n_points) { return batch >= 1 && n_points >= batch; }

}  // namespace

extern "C" int hfl_cloud_nonfinite(int32_t* flags, const float* points, const int64_t* cloud_offsets, int batch,
                                   int64_t n_points, hfl_stream_t stream) {
  if (flags == nullptr || points == nullptr || cloud_offsets == nullptr || !out_batch_ok(batch, n_points)) return HFL_EINVAL;
  if (batch > HFL_VOXEL_MAX_CLOUDS || n_points > HFL_VOXEL_MAX_POINTS) return HFL_ECAPACITY;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(flags, 0, sizeof(int32_t) * (size_t)batch, s);
  if (e != hipSuccess) return (int)e;
  cloud_nonfinite_kernel<<<(unsigned)hfl_cdiv(n_points, kOutThreads), kOutThreads, 0, s>>>(flags, points, cloud_offsets, batch,
                                                                                          n_points);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int hfl_knn_cell_keys(int64_t* keys, const hfl_knn_grid* grids_host, const hfl_knn_grid* grids, int batch,
                                 int64_t n_cells, const float* points, const int64_t* cloud_offsets, int64_t n_points,
                                 hfl_stream_t stream) {
  if (keys == nullptr || grids_host == nullptr || grids == nullptr || points == nullptr || cloud_offsets == nullptr)
    return HFL_EINVAL;
  int k_max = 0;
  if (const int rc = knn_call_check(batch, n_points, n_cells, grids_host, &k_max)) return rc;
  knn_cell_keys_kernel<<<(unsigned)hfl_cdiv(n_points, kOutThreads), kOutThreads, 0, static_cast<hipStream_t>(stream)>>>(
      keys, grids, points, cloud_offsets, batch, n_points);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int hfl_knn_mean_dist(float* avg, int32_t* pending, int32_t* counter, int32_t* cell_starts,
                                 const float* sorted_points, const int64_t* sorted_keys, const int64_t* perm,
                                 const hfl_knn_grid* grids_host, const hfl_knn_grid* grids, int batch, int64_t n_cells,
                                 const int64_t* cloud_offsets, int64_t n_points, int phases, hfl_stream_t stream) {
  if (avg == nullptr || pending == nullptr || counter == nullptr || cell_starts == nullptr || sorted_points == nullptr ||
      sorted_keys == nullptr || perm == nullptr || grids_host == nullptr || grids == nullptr || cloud_offsets == nullptr)
    return HFL_EINVAL;
  if (phases < 1 || phases > HFL_KNN_PHASE_ALL) return HFL_EINVAL;
  int k_max = 0;
  if (const int rc = knn_call_check(batch, n_points, n_cells, grids_host, &k_max)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t n = n_points;
  if (const int rc = knn_launch_starts(cell_starts, counter, sorted_keys, n, n_cells, phases, s)) return rc;
  return knn_dispatch_k(k_max, [&](auto kc) -> int {
    constexpr int K = decltype(kc)::value;
    if (phases & HFL_KNN_PHASE_QUERY)
      knn_query_kernel<K><<<(unsigned)hfl_cdiv(n, kOutThreads), kOutThreads, 0, s>>>(
          avg, pending, counter, sorted_points, sorted_keys, perm, cell_starts, grids, cloud_offsets, batch, n);
    if (phases & HFL_KNN_PHASE_FALLBACK)
      knn_fallback_kernel<K><<<knn_fallback_blocks(n, s), kOutThreads, 0, s>>>(avg, pending, counter, sorted_points, perm,
                                                                              grids, cloud_offsets, batch, n);
    HFL_RETURN_LAST_ERROR();
  });
}

extern "C" int hfl_knn_radius_count(int32_t* counts, int32_t* pending, int32_t* counter, int32_t* cell_starts,
                                    const float* sorted_points, const int64_t* sorted_keys, const int64_t* perm,
                                    const hfl_knn_grid* grids_host, const hfl_knn_grid* grids, int batch, int64_t n_cells,
                                    const int64_t* cloud_offsets, int64_t n_points, float radius2, int phases,
                                    hfl_stream_t stream) {
  if (counts == nullptr || pending == nullptr || counter == nullptr || cell_starts == nullptr || sorted_points == nullptr ||
      sorted_keys == nullptr || perm == nullptr || grids_host == nullptr || grids == nullptr || cloud_offsets == nullptr)
    return HFL_EINVAL;
  if (phases < 1 || phases > HFL_KNN_PHASE_ALL || !knn_cap_ok(radius2)) return HFL_EINVAL;
  int k_max = 0;
  if (const int rc = knn_call_check(batch, n_points, n_cells, grids_host, &k_max)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t n = n_points;
  if (const int rc = knn_launch_starts(cell_starts, counter, sorted_keys, n, n_cells, phases, s)) return rc;
  if (phases & HFL_KNN_PHASE_QUERY)
    radius_count_kernel<<<(unsigned)hfl_cdiv(n, kOutThreads), kOutThreads, 0, s>>>(
        counts, pending, counter, sorted_points, sorted_keys, perm, cell_starts, grids, cloud_offsets, batch, n, radius2);
  if (phases & HFL_KNN_PHASE_FALLBACK)
    radius_count_fallback_kernel<<<knn_fallback_blocks(n, s), kOutThreads, 0, s>>>(counts, pending, counter, sorted_points,
                                                                                   perm, cloud_offsets, batch, n, radius2);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int hfl_count_mask(uint8_t* keep, const int32_t* counts, int64_t n_points, int32_t nb_points,
                              hfl_stream_t stream) {
  if (keep == nullptr || counts == nullptr || n_points < 1 || nb_points < 0) return HFL_EINVAL;
  if (n_points > HFL_VOXEL_MAX_POINTS) return HFL_ECAPACITY;
  count_mask_kernel<<<(unsigned)hfl_cdiv(n_points, kOutThreads), kOutThreads, 0, static_cast<hipStream_t>(stream)>>>(
      keep, counts, n_points, nb_points);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int hfl_outlier_threshold(double* stats, const float* avg, const int64_t* cloud_offsets, int batch,
                                     int64_t n_points, double std_ratio, hfl_stream_t stream) {
  if (stats == nullptr || avg == nullptr || cloud_offsets == nullptr || batch < 1 || n_points < 0) return HFL_EINVAL;
  if (!(std_ratio > 0.0) || !(std_ratio - std_ratio == 0.0)) return HFL_EINVAL;
  if (batch > HFL_VOXEL_MAX_CLOUDS) return HFL_ECAPACITY;
  outlier_threshold_kernel<<<(unsigned)batch, kOutThreads, 0, static_cast<hipStream_t>(stream)>>>(stats, avg, cloud_offsets,
                                                                                                 n_points, std_ratio);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int hfl_outlier_mask(uint8_t* keep, const float* avg, const double* stats, const int64_t* cloud_offsets, int batch,
                                int64_t n_points, hfl_stream_t stream) {
  if (keep == nullptr || avg == nullptr || stats == nullptr || cloud_offsets == nullptr || !out_batch_ok(batch, n_points))
    return HFL_EINVAL;
  if (batch > HFL_VOXEL_MAX_CLOUDS || n_points > HFL_VOXEL_MAX_POINTS) return HFL_ECAPACITY;
  outlier_mask_kernel<<<(unsigned)hfl_cdiv(n_points, kOutThreads), kOutThreads, 0, static_cast<hipStream_t>(stream)>>>(
      keep, avg, stats, cloud_offsets, batch, n_points);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int hfl_radius_mask(uint8_t* keep, const float* points, int64_t n_points, double radius_max, hfl_stream_t stream) {
  if (keep == nullptr || points == nullptr || n_points < 1) return HFL_EINVAL;
  if (!(radius_max > 0.0) || !(radius_max - radius_max == 0.0)) return HFL_EINVAL;
  if (n_points > HFL_VOXEL_MAX_POINTS) return HFL_ECAPACITY;
  radius_mask_kernel<<<(unsigned)hfl_cdiv(n_points, kOutThreads), kOutThreads, 0, static_cast<hipStream_t>(stream)>>>(
      keep, points, n_points, radius_max);
  HFL_RETURN_LAST_ERROR();
}
