// Ground-to-aerial submap overlap: align one cloud of a pair into the other's frame, find every point's nearest neighbour in
// the other cloud, and reduce the distances of a pair to sums and threshold counts.  This is the step the reference's
// misc/compute_ground_aerial_overlap.py stops at (`TODO: dist = chamfer_distance(...)`): its apply_transform and the
// distance it never computed.  A batch of P pairs is ragged: the points of all clouds concatenated as (N_total, 3) fp32 with
// (P + 1) int64 offsets, cloud p at rows [off[p], off[p + 1]).
//
// hfl_transform_points: one thread per point, the owning pair found by a binary search over the offsets; every coordinate
// is `rigid_coord` of pair_scan.h.
//
// hfl_nn_dist: brute force, exact: the scan of pair_scan.h.  A workgroup of 256 threads owns OV_ROWS consecutive query rows
// of one pair (the host's tile table says which), each thread keeping OV_QPT = OV_ROWS / 256 query points in registers; the
// pair's target cloud streams through LDS in tiles of OV_TILE points.  d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) in fp32, the
// lowest target index of equal distances, one correctly rounded square root at the end.
//
// hfl_pair_stats: one workgroup per pair; a thread sums rows off[p] + tid, + 256, ... in float64 in that order, a wave
// combines its lanes by the xor butterfly 32, 16, ... 1, and thread 0 adds the four wave results in wave order.
//
// No atomics anywhere; every output element has one writer and a fixed evaluation order: two runs give the same bits.
#include <math.h>

#include "pair_scan.h"

namespace {

constexpr int OV_THREADS = 256;
constexpr int OV_ROWS = HFL_OVERLAP_ROWS;                        // query rows of a workgroup
constexpr int OV_QPT = OV_ROWS / OV_THREADS;                     // query points a thread keeps in registers
constexpr int OV_TILE = HFL_OVERLAP_TILE;                        // target points of an LDS tile
constexpr int OV_MAX_TAUS = HFL_OVERLAP_MAX_TAUS;
static_assert(OV_ROWS % OV_THREADS == 0 && OV_QPT >= 1, "whole query points per thread");
// 3 x 2048 x 4 B = 24 KiB of static LDS: six workgroups fit a CU's 160 KiB, the 32-waves-per-CU cap admits eight of 4 waves.
static_assert(OV_TILE % 4 == 0 && OV_TILE * 12 <= 32 * 1024, "static LDS stays at 32 KiB or less");

__global__ void __launch_bounds__(OV_THREADS)
transform_points_kernel(float* __restrict__ out, const float* __restrict__ points, const int64_t* __restrict__ offsets,
                        const float* __restrict__ transforms, int n_pairs, int64_t n_points) {
  const int64_t i = (int64_t)blockIdx.x * OV_THREADS + threadIdx.x;
  if (i >= n_points) return;
  int lo = 0, hi = n_pairs;                                      // the first pair whose end lies past row i
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid + 1] > i) hi = mid; else lo = mid + 1;
  }
  if (lo >= n_pairs || offsets[lo] > i) return;                  // a row no pair owns is not written
  const float* m = transforms + 12 * (int64_t)lo;
  const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
#pragma unroll
  for (int c = 0; c < 3; ++c) out[3 * i + c] = rigid_coord(m + 4 * c, x, y, z);
}

__global__ void __launch_bounds__(OV_THREADS)
nn_dist_kernel(float* __restrict__ dist, int32_t* __restrict__ idx, const float* __restrict__ queries,
               const int64_t* __restrict__ q_off, int64_t n_queries, const float* __restrict__ targets,
               const int64_t* __restrict__ t_off, int64_t n_targets, const int64_t* __restrict__ tiles, int n_pairs) {
  __shared__ __align__(16) float s_x[OV_TILE], s_y[OV_TILE], s_z[OV_TILE];
  PairTile w;
  if (!pair_tile(w, tiles, n_pairs)) return;
  pair_ranges(w, q_off, n_queries, t_off, n_targets);
  float qx[OV_QPT], qy[OV_QPT], qz[OV_QPT], best[OV_QPT];
  int32_t at[OV_QPT];
#pragma unroll
  for (int r = 0; r < OV_QPT; ++r) {
    const int64_t row = w.row<OV_THREADS>(r);
    const bool valid = row < w.q_end;
    qx[r] = valid ? queries[3 * row] : 0.f;
    qy[r] = valid ? queries[3 * row + 1] : 0.f;
    qz[r] = valid ? queries[3 * row + 2] : 0.f;
  }
  pair_scan3<OV_THREADS>(w, targets, s_x, s_y, s_z, qx, qy, qz, best, at);
#pragma unroll
  for (int r = 0; r < OV_QPT; ++r) {
    const int64_t row = w.row<OV_THREADS>(r);
    if (row < w.q_end) {
      dist[row] = pair_sqrt(best[r]);                            // +inf: an empty target cloud
      idx[row] = at[r];
    }
  }
}

struct Taus {
  float v[OV_MAX_TAUS];
};

__global__ void __launch_bounds__(OV_THREADS)
pair_stats_kernel(double* __restrict__ sums, int64_t* __restrict__ counts, const float* __restrict__ dist,
                  const int64_t* __restrict__ offsets, int64_t n_dist, int n_taus, Taus taus) {
  constexpr int WAVES = OV_THREADS / HFL_WAVE;
  __shared__ double s_sum[WAVES][2];
  __shared__ long long s_cnt[WAVES][OV_MAX_TAUS + 1];
  const int p = blockIdx.x;
  const int64_t begin = max(offsets[p], (int64_t)0), end = min(offsets[p + 1], n_dist);
  double sum = 0.0, sum2 = 0.0;
  long long cnt[OV_MAX_TAUS + 1];
#pragma unroll
  for (int k = 0; k <= OV_MAX_TAUS; ++k) cnt[k] = 0;
  for (int64_t i = begin + threadIdx.x; i < end; i += OV_THREADS) {
    const float d = dist[i];
    if (d == INFINITY) {
      cnt[OV_MAX_TAUS] += 1;                                     // no target: in no sum and no threshold count
    } else {
      const double dd = (double)d;
      sum += dd;
      sum2 += dd * dd;
#pragma unroll
      for (int k = 0; k < OV_MAX_TAUS; ++k) cnt[k] += (k < n_taus && d <= taus.v[k]) ? 1 : 0;
    }
  }
  const int lane = threadIdx.x & (HFL_WAVE - 1), wave = threadIdx.x >> 6;
  sum = wave_sum(sum);
  sum2 = wave_sum(sum2);
#pragma unroll
  for (int k = 0; k <= OV_MAX_TAUS; ++k) cnt[k] = wave_sum(cnt[k]);
  if (lane == 0) {
    s_sum[wave][0] = sum;
    s_sum[wave][1] = sum2;
#pragma unroll
    for (int k = 0; k <= OV_MAX_TAUS; ++k) s_cnt[wave][k] = cnt[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = s_sum[0][0], b = s_sum[0][1];
    for (int w = 1; w < WAVES; ++w) { a += s_sum[w][0]; b += s_sum[w][1]; }
    sums[2 * (int64_t)p] = a;
    sums[2 * (int64_t)p + 1] = b;
  }
  if (threadIdx.x <= n_taus) {                                   // columns 0..K-1 the thresholds, column K the +inf rows
    const int k = threadIdx.x < n_taus ? threadIdx.x : OV_MAX_TAUS;
    long long c = 0;
    for (int w = 0; w < WAVES; ++w) c += s_cnt[w][k];
    counts[(int64_t)p * (n_taus + 1) + threadIdx.x] = c;
  }
}

}  // namespace

extern "C" int hfl_transform_points(float* out, const float* points, const int64_t* offsets, const float* transforms,
                                    int64_t n_pairs, int64_t n_points, hfl_stream_t stream) {
  if (out == nullptr || points == nullptr || offsets == nullptr || transforms == nullptr || n_pairs < 1 || n_points < 0)
    return HFL_EINVAL;
  const int64_t blocks = hfl_cdiv(n_points, OV_THREADS);
  if (n_pairs > 0x7fffffffLL || blocks > 0x7fffffffLL) return HFL_ECAPACITY;
  if (n_points == 0) return HFL_OK;
  transform_points_kernel<<<(unsigned)blocks, OV_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      out, points, offsets, transforms, (int)n_pairs, n_points);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int hfl_nn_dist(float* dist, int32_t* idx, const float* queries, const int64_t* q_offsets, int64_t n_queries,
                           const float* targets, const int64_t* t_offsets, int64_t n_targets, const int64_t* tiles,
                           int64_t n_tiles, int64_t n_pairs, hfl_stream_t stream) {
  return pair_scan_call({dist, idx, queries, q_offsets, targets, t_offsets, tiles}, true, n_queries, n_targets, n_tiles,
                        n_pairs, [&] {
    nn_dist_kernel<<<(unsigned)n_tiles, OV_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
        dist, idx, queries, q_offsets, n_queries, targets, t_offsets, n_targets, tiles, (int)n_pairs);
  });
}

extern "C" int hfl_pair_stats(double* sums, int64_t* counts, const float* dist, const int64_t* offsets, int64_t n_dist,
                              int64_t n_pairs, const float* taus, int n_taus, hfl_stream_t stream) {
  if (sums == nullptr || counts == nullptr || dist == nullptr || offsets == nullptr || n_dist < 0 || n_pairs < 1 ||
      n_taus < 0 || n_taus > OV_MAX_TAUS || (n_taus > 0 && taus == nullptr))
    return HFL_EINVAL;
  if (n_pairs > 0x7fffffffLL) return HFL_ECAPACITY;
  Taus t;
  for (int k = 0; k < OV_MAX_TAUS; ++k) t.v[k] = k < n_taus ? taus[k] : 0.f;
  pair_stats_kernel<<<(unsigned)n_pairs, OV_THREADS, 0, static_cast<hipStream_t>(stream)>>>(sums, counts, dist, offsets,
                                                                                            n_dist, n_taus, t);
  HFL_RETURN_LAST_ERROR();
}
