// Global registration of a ragged batch of P pairs from point correspondences: a deterministic RANSAC and the sums of its
// polish.  The definition is in hotformerloc_amd/global_registration.py and DESIGN.md section 7n.  The correspondences of all
// pairs are gathered once into (C, 6) fp32 rows (px, py, pz, qx, qy, qz) with (P + 1) int64 offsets; a hypothesis is twelve
// fp32 values, the row-major (R | t) hfl_transform_points takes; the hypotheses of a pair are rows [pair * H, (pair + 1) * H).
//
// hfl_ransac_hypotheses: one thread per (pair, h).  Philox draws three rows, the edge lengths of the triple are compared in
// float64, `kabsch_solve` (kabsch.h, the solver of hfl_icp_solve) takes the 17 sums of the three pairs, and the pose is
// rounded to fp32.  An invalid hypothesis gets a pose of NaNs and the flag 0.  This file is built with -ffp-contract=off: the
// float64 steps are the numpy route's, operation for operation.
//
// hfl_ransac_score: the hot path, in the pattern of pair_scan.h with the roles turned: RS_ROWS hypotheses of a pair live in
// the registers of a workgroup (two per thread, twelve fp32 each), and one tile of RS_TILE of the pair's correspondences
// lies in LDS as six coordinate planes, which every lane reads by the same 16-byte broadcast loads.  A test is nine fmaf for
// the move, three subtractions, the d2 chain of the pair scan, a compare and an integer add.  The grid is (correspondence tiles
// of the host's table, hypothesis tiles): a single pair with many correspondences still fills the chip.  A workgroup
// adds its counts to counts[pair, h] by integer atomic adds; integer addition is associative, so the counts do not depend on
// the order and two runs give the same bits.  A launch of its own writes 0 or -1 (invalid) first.
//
// hfl_ransac_select: one workgroup per pair finds the largest count and of equal counts the lowest h, and writes the chosen
// pose into the (state, istate) layout of hfl_icp_solve: RUNNING at iteration 0, or HFL_RANSAC_NO_HYPOTHESIS with the
// identity, fitness 0 and rmse NaN where every count is -1.
//
// hfl_ransac_sums: hfl_icp_correspond without the search.  A workgroup owns the RS_TILE correspondences of one row of the
// tile table, moves p by the fp32 rounding of the pair's pose, and adds and reduces the 17 float64 sums of its inliers by the
// row step and the reduction of icp_sums.h, the code icp_correspond_kernel runs (a thread its rows in row order, the xor
// butterfly, the four waves in wave order), into row blockIdx.x of the partials, which hfl_icp_solve reads as it reads those
// of hfl_icp_correspond.  A pair that is not RUNNING makes its workgroups return at once.
#include <math.h>

#include "icp_sums.h"
#include "kabsch.h"
#include "pair_scan.h"
#include "philox.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_ROWS = HFL_RANSAC_ROWS;                         // hypotheses of a workgroup of the score kernel
constexpr int RS_HPT = RS_ROWS / RS_THREADS;                     // hypotheses a thread keeps in registers
constexpr int RS_TILE = HFL_RANSAC_TILE;                         // correspondences of a workgroup: one LDS tile
constexpr int RS_CPT = RS_TILE / RS_THREADS;                     // correspondences a thread of the sums kernel adds
constexpr int RS_SUMS = HFL_ICP_SUMS;
constexpr int RS_WAVES = RS_THREADS / HFL_WAVE;
static_assert(RS_ROWS % RS_THREADS == 0 && RS_HPT >= 1, "whole hypotheses per thread");
static_assert(RS_TILE % RS_THREADS == 0 && RS_TILE % 4 == 0, "whole correspondences per thread, whole groups of four");
static_assert(RS_TILE * 24 <= 32 * 1024, "static LDS stays at 32 KiB or less");

// What a workgroup owns: the correspondences [row0, c_end) of `pair`, at most RS_TILE of them, clamped to the array like
// the ranges of PairTile.  false (uniform over the workgroup) for a table row that names no pair.
struct CorrTile {
  int64_t pair, row0, c_end;
};
__device__ __forceinline__ bool corr_tile(CorrTile& w, const int64_t* __restrict__ tiles, int64_t tile,
                                          const int64_t* __restrict__ c_off, int64_t n_corr, int n_pairs) {
  w.pair = tiles[2 * tile], w.row0 = tiles[2 * tile + 1];
  if (!(w.pair >= 0 && w.pair < n_pairs && w.row0 >= 0)) return false;
  w.c_end = min(min(c_off[w.pair + 1], n_corr), w.row0 + RS_TILE);
  return true;
}

// p' = the row-major (R | t) m on p, and the d2 of the pair scan on p' - q
__device__ __forceinline__ float corr_move_d2(const float* __restrict__ m, float px, float py, float pz, float qx, float qy,
                                              float qz, float (&moved)[3]) {
  moved[0] = rigid_coord(m, px, py, pz), moved[1] = rigid_coord(m + 4, px, py, pz), moved[2] = rigid_coord(m + 8, px, py, pz);
  const float dx = moved[0] - qx, dy = moved[1] - qy, dz = moved[2] - qz;
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}
__device__ __forceinline__ float corr_d2(const float* __restrict__ m, float px, float py, float pz, float qx, float qy,
                                         float qz) {
  float moved[3];
  return corr_move_d2(m, px, py, pz, qx, qy, qz, moved);
}

__device__ __forceinline__ double edge2(const float* __restrict__ a, const float* __restrict__ b) {
  const double dx = (double)a[0] - (double)b[0], dy = (double)a[1] - (double)b[1], dz = (double)a[2] - (double)b[2];
  return (dx * dx + dy * dy) + dz * dz;                          // one rounding per operation: contraction is off
}

__global__ void __launch_bounds__(RS_THREADS)
ransac_hypotheses_kernel(float* __restrict__ poses, uint8_t* __restrict__ valid, int32_t* __restrict__ draws,
                         const float* __restrict__ corr, const int64_t* __restrict__ c_off, int64_t n_corr, int n_pairs,
                         int n_hyp, uint32_t k0, uint32_t k1, double rho2) {
  const int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
  if (i >= (int64_t)n_pairs * n_hyp) return;
  const int pair = (int)(i / n_hyp), h = (int)(i - (int64_t)pair * n_hyp);
  const int64_t begin = min(max(c_off[pair], (int64_t)0), n_corr), end = min(c_off[pair + 1], n_corr);
  const uint64_t c = (uint64_t)max(end - begin, (int64_t)0);     // < 2^31: the entry point bounds n_corr
  const U4 x = philox4x32_10((uint32_t)h, (uint32_t)pair, 0u, 0u, k0, k1);
  const int32_t i0 = (int32_t)(((uint64_t)x.x * c) >> 32), i1 = (int32_t)(((uint64_t)x.y * c) >> 32),
                i2 = (int32_t)(((uint64_t)x.z * c) >> 32);
  draws[3 * i] = i0, draws[3 * i + 1] = i1, draws[3 * i + 2] = i2;

  double r[3][3], t[3];
  bool ok = c >= 3 && i0 != i1 && i0 != i2 && i1 != i2;
  if (ok) {                                                      // 0 <= i_k < c: the gathers stay in the pair's rows
    const float* a = corr + 6 * (begin + i0);
    const float* b = corr + 6 * (begin + i1);
    const float* d = corr + 6 * (begin + i2);
    if (rho2 > 0.0) {
      const double ls01 = edge2(a, b), ls02 = edge2(a, d), ls12 = edge2(b, d);
      const double lt01 = edge2(a + 3, b + 3), lt02 = edge2(a + 3, d + 3), lt12 = edge2(b + 3, d + 3);
      ok = ls01 >= rho2 * lt01 && lt01 >= rho2 * ls01 && ls02 >= rho2 * lt02 && lt02 >= rho2 * ls02 &&
           ls12 >= rho2 * lt12 && lt12 >= rho2 * ls12;
    }
    if (ok) {
      double s[RS_SUMS];
      s[0] = 3.0;
      s[16] = 0.0;
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const double p0 = (double)a[u], p1 = (double)b[u], p2 = (double)d[u];
        s[1 + u] = (p0 + p1) + p2;
        s[4 + u] = ((double)a[3 + u] + (double)b[3 + u]) + (double)d[3 + u];
#pragma unroll
        for (int v = 0; v < 3; ++v)                              // a product of two fp32 values is exact in float64
          s[7 + 3 * u + v] = (p0 * (double)a[3 + v] + p1 * (double)b[3 + v]) + p2 * (double)d[3 + v];
      }
      ok = kabsch_solve(s, r, t);
    }
  }
  float* out = poses + 12 * i;
#pragma unroll
  for (int u = 0; u < 3; ++u) {
#pragma unroll
    for (int v = 0; v < 3; ++v) out[4 * u + v] = ok ? (float)r[u][v] : NAN;
    out[4 * u + 3] = ok ? (float)t[u] : NAN;
  }
  valid[i] = ok ? 1 : 0;
}

__global__ void __launch_bounds__(RS_THREADS)
ransac_score_init_kernel(int32_t* __restrict__ counts, const uint8_t* __restrict__ valid, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
  if (i < n) counts[i] = valid[i] ? 0 : -1;
}

// 24 KiB of static LDS and, built without SLP vectorisation (build.py), 74 VGPRs: six workgroups per CU, six waves per SIMD.
// No amdgpu_waves_per_eu here: with it the scheduler trades registers for latency up to the cap and then spills.
__global__ void __launch_bounds__(RS_THREADS)
ransac_score_kernel(int32_t* __restrict__ counts, const uint8_t* __restrict__ valid, const float* __restrict__ poses,
                    const float* __restrict__ corr, const int64_t* __restrict__ c_off, int64_t n_corr,
                    const int64_t* __restrict__ tiles, int n_pairs, int n_hyp, float d2_max) {
  __shared__ __align__(16) float s_c[6][RS_TILE];                // px, py, pz, qx, qy, qz
  CorrTile w;
  if (!corr_tile(w, tiles, blockIdx.x, c_off, n_corr, n_pairs)) return;
  const int len = (int)max(w.c_end - w.row0, (int64_t)0);
  if (len == 0) return;

  float m[RS_HPT][12];
  bool live[RS_HPT];
  int64_t at[RS_HPT];
#pragma unroll
  for (int r = 0; r < RS_HPT; ++r) {                             // a row past H reads row H - 1 and adds nothing
    const int h = blockIdx.y * RS_ROWS + r * RS_THREADS + threadIdx.x;
    at[r] = w.pair * n_hyp + min(h, n_hyp - 1);
    live[r] = h < n_hyp && valid[at[r]] != 0;
    const float4* row = reinterpret_cast<const float4*>(poses + 12 * at[r]);   // 48-byte rows of a 16-byte aligned array
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float4 v = row[k];
      m[r][4 * k] = v.x, m[r][4 * k + 1] = v.y, m[r][4 * k + 2] = v.z, m[r][4 * k + 3] = v.w;
    }
  }
  const int len4 = (len + 3) & ~3;                               // padded to whole groups of four
  for (int k = threadIdx.x; k < 6 * len4; k += RS_THREADS) {     // consecutive lanes read consecutive floats
    const int row = k / 6, col = k - 6 * row;
    // padding: p = 0 against q = +inf, whose d2 is +inf and never <= the finite d2_max
    s_c[col][row] = row < len ? corr[6 * w.row0 + k] : (col < 3 ? 0.f : INFINITY);
  }
  __syncthreads();

  int32_t n[RS_HPT];
#pragma unroll
  for (int r = 0; r < RS_HPT; ++r) n[r] = 0;
  for (int k = 0; k < len4; k += 4) {
    float c[6][4];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const float4 v = *reinterpret_cast<const float4*>(&s_c[a][k]);
      c[a][0] = v.x, c[a][1] = v.y, c[a][2] = v.z, c[a][3] = v.w;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int r = 0; r < RS_HPT; ++r)
        n[r] += corr_d2(m[r], c[0][u], c[1][u], c[2][u], c[3][u], c[4][u], c[5][u]) <= d2_max ? 1 : 0;
  }
#pragma unroll
  for (int r = 0; r < RS_HPT; ++r)
    if (live[r] && n[r] != 0) atomicAdd(&counts[at[r]], n[r]);
}

// (count + 1, the complement of h) as one key: the largest key is the largest count at the lowest h
__device__ __forceinline__ uint64_t select_key(int32_t count, int h) {
  return ((uint64_t)(uint32_t)(count + 1) << 32) | (uint64_t)(0xffffffffu - (uint32_t)h);
}

__global__ void __launch_bounds__(RS_THREADS)
ransac_select_kernel(double* __restrict__ state, int32_t* __restrict__ istate, int32_t* __restrict__ chosen,
                     const int32_t* __restrict__ counts, const float* __restrict__ poses, int n_hyp) {
  __shared__ uint64_t s_key[RS_THREADS];
  __shared__ int32_t s_valid[RS_THREADS];
  const int64_t pair = blockIdx.x;
  uint64_t best = 0;                                             // the key of count -1 at no h
  int32_t n_valid = 0;
  for (int h = threadIdx.x; h < n_hyp; h += RS_THREADS) {
    const int32_t c = max(counts[pair * n_hyp + h], -1);
    const uint64_t key = select_key(c, h);
    best = key > best ? key : best;
    n_valid += c >= 0 ? 1 : 0;
  }
  s_key[threadIdx.x] = best, s_valid[threadIdx.x] = n_valid;
  __syncthreads();
  for (int step = RS_THREADS / 2; step > 0; step >>= 1) {
    if ((int)threadIdx.x < step) {
      const uint64_t other = s_key[threadIdx.x + step];
      if (other > s_key[threadIdx.x]) s_key[threadIdx.x] = other;
      s_valid[threadIdx.x] += s_valid[threadIdx.x + step];
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  best = s_key[0];
  const int32_t count = (int32_t)(uint32_t)(best >> 32) - 1;
  const bool any = count >= 0;
  const int h = any ? (int)(0xffffffffu - (uint32_t)best) : -1;
  chosen[3 * pair] = h, chosen[3 * pair + 1] = any ? count : -1, chosen[3 * pair + 2] = s_valid[0];
  double* st = state + 16 * pair;
#pragma unroll
  for (int k = 0; k < 12; ++k) st[k] = any ? (double)poses[12 * (pair * n_hyp + h) + k] : ((k % 5) == 0 ? 1.0 : 0.0);
  st[12] = 0.0;
  st[13] = (double)NAN;
  st[14] = 0.0;
  st[15] = (double)NAN;
  istate[2 * pair] = 0;
  istate[2 * pair + 1] = any ? HFL_ICP_RUNNING : HFL_RANSAC_NO_HYPOTHESIS;
}

__global__ void __launch_bounds__(RS_THREADS)
ransac_sums_kernel(double* __restrict__ partials, const float* __restrict__ corr, const int64_t* __restrict__ c_off,
                   int64_t n_corr, const int64_t* __restrict__ tiles, const double* __restrict__ state,
                   const int32_t* __restrict__ istate, int n_pairs, float d2_max) {
  __shared__ double red[RS_WAVES * RS_SUMS];
  CorrTile w;
  if (!corr_tile(w, tiles, blockIdx.x, c_off, n_corr, n_pairs)) return;
  if (istate[2 * w.pair + 1] != HFL_ICP_RUNNING) return;         // the pair has stopped: its partials are not read again
  float m[12];                                                   // the pose, rounded once to fp32
#pragma unroll
  for (int k = 0; k < 12; ++k) m[k] = (float)state[16 * w.pair + k];

  double acc[RS_SUMS];
#pragma unroll
  for (int k = 0; k < RS_SUMS; ++k) acc[k] = 0.0;
#pragma unroll
  for (int r = 0; r < RS_CPT; ++r) {                             // a thread's rows in row order
    const int64_t row = w.row0 + r * RS_THREADS + threadIdx.x;
    if (row < w.c_end) {
      const float* c = corr + 6 * row;
      float p[3];
      const float d2 = corr_move_d2(m, c[0], c[1], c[2], c[3], c[4], c[5], p);
      if (d2 <= d2_max) {
        const double pc[3] = {(double)p[0], (double)p[1], (double)p[2]};
        const double qc[3] = {(double)c[3], (double)c[4], (double)c[5]};
        const double dd = (double)pair_sqrt(d2);
        icp_point_row(acc, pc, qc, dd);
      }
    }
  }
  icp_reduce_partials<RS_SUMS, RS_THREADS>(acc, red, partials);
}

}  // namespace

extern "C" int hfl_ransac_hypotheses(float* poses, uint8_t* valid, int32_t* draws, const float* corr,
                                     const int64_t* c_offsets, int64_t n_corr, int64_t n_pairs, int64_t n_hypotheses,
                                     uint64_t seed, double rho2, hfl_stream_t stream) {
  if (poses == nullptr || valid == nullptr || draws == nullptr || corr == nullptr || c_offsets == nullptr || n_corr < 0 ||
      n_pairs < 1 || n_hypotheses < 1 || !(rho2 >= 0.0))
    return HFL_EINVAL;
  if (n_corr > 0x7fffffffLL || n_pairs > 0x7fffffffLL || n_hypotheses > 0x7fffffffLL) return HFL_ECAPACITY;
  const int64_t blocks = (n_pairs * n_hypotheses + RS_THREADS - 1) / RS_THREADS;
  if (blocks > 0x7fffffffLL) return HFL_ECAPACITY;
  ransac_hypotheses_kernel<<<(unsigned)blocks, RS_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      poses, valid, draws, corr, c_offsets, n_corr, (int)n_pairs, (int)n_hypotheses, (uint32_t)seed, (uint32_t)(seed >> 32),
      rho2);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int hfl_ransac_score(int32_t* counts, const uint8_t* valid, const float* poses, const float* corr,
                                const int64_t* c_offsets, int64_t n_corr, const int64_t* tiles, int64_t n_tiles,
                                int64_t n_pairs, int64_t n_hypotheses, float d2_max, hfl_stream_t stream) {
  if (counts == nullptr || valid == nullptr || poses == nullptr || corr == nullptr || c_offsets == nullptr ||
      tiles == nullptr || n_corr < 0 || n_tiles < 0 || n_pairs < 1 || n_hypotheses < 1)
    return HFL_EINVAL;
  const int64_t total = n_pairs * n_hypotheses, h_tiles = (n_hypotheses + RS_ROWS - 1) / RS_ROWS;
  if (n_corr > 0x7fffffffLL || n_pairs > 0x7fffffffLL || n_hypotheses > 0x7fffffffLL || total > 0x7fffffffLL ||
      n_tiles > 0x7fffffffLL || h_tiles > 65535)                 // the second dimension of a grid
    return HFL_ECAPACITY;
  ransac_score_init_kernel<<<(unsigned)((total + RS_THREADS - 1) / RS_THREADS), RS_THREADS, 0,
                             static_cast<hipStream_t>(stream)>>>(counts, valid, total);
  if (n_tiles > 0)
    ransac_score_kernel<<<dim3((unsigned)n_tiles, (unsigned)h_tiles), RS_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
        counts, valid, poses, corr, c_offsets, n_corr, tiles, (int)n_pairs, (int)n_hypotheses, d2_max);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int hfl_ransac_select(double* state, int32_t* istate, int32_t* chosen, const int32_t* counts, const float* poses,
                                 int64_t n_pairs, int64_t n_hypotheses, hfl_stream_t stream) {
  if (state == nullptr || istate == nullptr || chosen == nullptr || counts == nullptr || poses == nullptr || n_pairs < 1 ||
      n_hypotheses < 1)
    return HFL_EINVAL;
  if (n_pairs > 0x7fffffffLL || n_hypotheses > 0x7fffffffLL || n_pairs * n_hypotheses > 0x7fffffffLL) return HFL_ECAPACITY;
  ransac_select_kernel<<<(unsigned)n_pairs, RS_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      state, istate, chosen, counts, poses, (int)n_hypotheses);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int hfl_ransac_sums(double* partials, const float* corr, const int64_t* c_offsets, int64_t n_corr,
                               const int64_t* tiles, int64_t n_tiles, const double* state, const int32_t* istate,
                               int64_t n_pairs, float d2_max, hfl_stream_t stream) {
  if (partials == nullptr || corr == nullptr || c_offsets == nullptr || tiles == nullptr || state == nullptr ||
      istate == nullptr || n_corr < 0 || n_tiles < 0 || n_pairs < 1)
    return HFL_EINVAL;
  if (n_corr > 0x7fffffffLL || n_tiles > 0x7fffffffLL || n_pairs > 0x7fffffffLL) return HFL_ECAPACITY;
  if (n_tiles == 0) return HFL_OK;
  ransac_sums_kernel<<<(unsigned)n_tiles, RS_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      partials, corr, c_offsets, n_corr, tiles, state, istate, (int)n_pairs, d2_max);
  HFL_RETURN_LAST_ERROR();
}
