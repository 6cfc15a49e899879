// The exact brute-force nearest neighbour of a ragged batch of pairs, once, for everything that runs it: hfl_nn_dist
// (csrc/overlap.hip), both hfl_icp_correspond kernels (csrc/registration.hip) and hfl_feature_nn (csrc/fpfh.hip), which keeps
// its own D-column distance and row-major LDS tile and takes the rest.  A workgroup takes one row of the host's tile table:
// a few query rows per thread in registers against the pair's whole target cloud, which streams through LDS.
//
// Tie rule: the lowest target index wins.  A query is scanned by one thread over ascending indices with a strict `<`, so
// there are no partial results to combine: if the scan of one query is ever split, the parts combine by (d2, index)
// lexicographically.  Inputs must be finite and small enough that d2 does not overflow; this is not checked (a query whose
// every d2 is +inf or NaN reports index -1).  Whatever decides a bit here is an explicit fmaf or an expression of one
// operation: the same bits with -ffp-contract=off (fpfh.hip) and without (overlap.hip, registration.hip).
#pragma once
#include <math.h>

#include <initializer_list>

#include "ragged_common.h"

// ops.feature_tiles is ops.overlap_tiles: right only while the workgroups of both kernels own the same number of query rows
static_assert(HFL_FEATURE_ROWS == HFL_OVERLAP_ROWS, "feature_tiles is overlap_tiles");

namespace {

// One coordinate of R x + t from a matrix row (r0 r1 r2 t), one fmaf chain in this order
__device__ __forceinline__ float rigid_coord(const float* __restrict__ m, float x, float y, float z) {
  return fmaf(m[2], z, fmaf(m[1], y, fmaf(m[0], x, m[3])));
}

// What a workgroup owns: query rows [row0, q_end) of `pair`, as far as its threads reach, against the target rows
// [t_begin, t_end); row<THREADS>(r) is a thread's r-th query row.  The offsets are clamped to the arrays, so a wrong table or
// offset cannot make a kernel read or write outside them.
struct PairTile {
  int64_t pair, row0, q_end, t_begin, t_end;
  template <int THREADS>
  __device__ __forceinline__ int64_t row(int r) const { return row0 + r * THREADS + threadIdx.x; }
};

// row blockIdx.x of the tile table; false (uniform over the workgroup) for a row that names no pair: the kernel returns.
// Then the pair's ranges, in a step of their own: icp_correspond_kernel looks at the pair's status in between.
__device__ __forceinline__ bool pair_tile(PairTile& w, const int64_t* __restrict__ tiles, int n_pairs) {
  w.pair = tiles[2 * (int64_t)blockIdx.x], w.row0 = tiles[2 * (int64_t)blockIdx.x + 1];
  return w.pair >= 0 && w.pair < n_pairs && w.row0 >= 0;
}
__device__ __forceinline__ void pair_ranges(PairTile& w, const int64_t* __restrict__ q_off, int64_t n_queries,
                                            const int64_t* __restrict__ t_off, int64_t n_targets) {
  w.q_end = min(q_off[w.pair + 1], n_queries);
  w.t_begin = max(t_off[w.pair], (int64_t)0), w.t_end = min(t_off[w.pair + 1], n_targets);
}

// strict: of equal distances the candidate seen first, the lowest index, stays
__device__ __forceinline__ void pair_keep_closer(float d2, int32_t j, float& best, int32_t& at) {
  const bool closer = d2 < best;
  best = closer ? d2 : best;
  at = closer ? j : at;
}

// The correctly rounded fp32 root, sqrt(+inf) = +inf.  Not __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS the HIP headers
// map that name to the native approximation, an ulp off now and then (csrc/outliers.hip has the same note); sqrtf is
// correctly rounded under hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt, as numpy's float32 sqrt is.
__device__ __forceinline__ float pair_sqrt(float d2) { return __builtin_sqrtf(d2); }

// The length of a difference: the d2 chain of the scan and the correctly rounded root (csrc/spectral.hip, csrc/consensus.hip)
__device__ __forceinline__ float pair_len(float dx, float dy, float dz) {
  return pair_sqrt(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
}

// The scan of (N, 3) points: best[r] and at[r] become the smallest fp32 squared distance from (qx[r], qy[r], qz[r]) to a
// point of the tile's target cloud and that point's index within the cloud, +inf and -1 for an empty cloud.  The cloud
// streams through the three LDS planes in tiles of TILE points; every lane reads the same four target points (three
// broadcast ds_read_b128, conflict-free) for its 4 x QPT tests, fp32 on the differences themselves as in pairwise.hip.
// Every thread of the workgroup calls it; the planes are free again after the caller's next barrier.
template <int THREADS, int QPT, int TILE>
__device__ __forceinline__ void pair_scan3(const PairTile& w, const float* __restrict__ targets, float (&s_x)[TILE],
                                           float (&s_y)[TILE], float (&s_z)[TILE], const float (&qx)[QPT],
                                           const float (&qy)[QPT], const float (&qz)[QPT], float (&best)[QPT],
                                           int32_t (&at)[QPT]) {
  static_assert(TILE % 4 == 0, "whole groups of four target points");
#pragma unroll
  for (int r = 0; r < QPT; ++r) best[r] = INFINITY, at[r] = -1;
  for (int64_t tile = w.t_begin; tile < w.t_end; tile += TILE) {
    const int len = (int)min((int64_t)TILE, w.t_end - tile);
    const int len4 = (len + 3) & ~3;                             // the last tile is padded to whole groups of four
    __syncthreads();                                             // the previous tile has been read by every wave
    for (int k = threadIdx.x; k < len4; k += THREADS) {
      const int64_t j = tile + k;
      const bool real = k < len;                                 // padding lies at +inf: its d2 is +inf, never `<` a best
      s_x[k] = real ? targets[3 * j] : INFINITY;
      s_y[k] = real ? targets[3 * j + 1] : INFINITY;
      s_z[k] = real ? targets[3 * j + 2] : INFINITY;
    }
    __syncthreads();
    const int32_t base = (int32_t)(tile - w.t_begin);            // < 2^31: the entry point bounds n_targets
#pragma unroll 2
    for (int k = 0; k < len4; k += 4) {
      const float4 cx = *reinterpret_cast<const float4*>(&s_x[k]);
      const float4 cy = *reinterpret_cast<const float4*>(&s_y[k]);
      const float4 cz = *reinterpret_cast<const float4*>(&s_z[k]);
      const float tx[4] = {cx.x, cx.y, cx.z, cx.w}, ty[4] = {cy.x, cy.y, cy.z, cy.w}, tz[4] = {cz.x, cz.y, cz.z, cz.w};
#pragma unroll
      for (int u = 0; u < 4; ++u)                                // ascending target index
#pragma unroll
        for (int r = 0; r < QPT; ++r) {
          const float dx = qx[r] - tx[u], dy = qy[r] - ty[u], dz = qz[r] - tz[u];
          pair_keep_closer(fmaf(dz, dz, fmaf(dy, dy, dx * dx)), base + k + u, best[r], at[r]);
        }
    }
  }
}

// What every entry point that launches a scan checks, in this order: the pointers it cannot do without and its own
// conditions (`ok`), the signs, the capacity -- a target index is an int32, the grid is one-dimensional -- and a table
// without rows, which launches nothing.  Then launch().
template <typename F>
int pair_scan_call(std::initializer_list<const void*> required, bool ok, int64_t n_queries, int64_t n_targets,
                   int64_t n_tiles, int64_t n_pairs, F&& launch) {
  for (const void* p : required) ok = ok && p != nullptr;
  if (!ok || n_queries < 0 || n_targets < 0 || n_tiles < 0 || n_pairs < 1) return HFL_EINVAL;
  if (n_targets > 0x7fffffffLL || n_tiles > 0x7fffffffLL || n_pairs > 0x7fffffffLL) return HFL_ECAPACITY;
  if (n_tiles == 0) return HFL_OK;
  launch();
  HFL_RETURN_LAST_ERROR();
}

}  // namespace
