// Spectral geometric verification of a ragged batch of P pairs from point correspondences: the power iteration on the
// pairwise length-consistency matrix M of a pair's correspondences, which never exists in memory.  The definition is in
// hotformerloc_amd/spectral.py and DESIGN.md section 7p.  The correspondences come as hfl_ransac_score takes them: (C, 6)
// fp32 rows (px, py, pz, qx, qy, qz) with (P + 1) int64 offsets.
//
// hfl_spectral_matvec: the hot path, one step w = M v, in the pattern of ransac_score_kernel and pair_scan.h.  A workgroup
// owns SP_ROWS correspondences of one pair as rows (two per thread in registers: p_i, q_i, acc) and streams ALL of the
// pair's correspondences past them as columns, in ascending order, through LDS tiles of SP_TILE columns held as seven planes
// (px, py, pz, qx, qy, qz, v), which every lane reads by the same 16-byte broadcast loads.  One thread sweeps every column of
// its row: acc = fmaf(m_ij, v_j, acc) from 0 over j ascending, whatever the tiling constants are.  An entry is six
// subtractions, two d2 chains, two correctly rounded roots, a subtraction, a product, an fmaf and a max; m_ii = 0 is a
// compare and a select, paid only on the SP_ROWS columns that can hold a row's own correspondence.  Padding columns carry
// v = 0 against finite entries and leave acc as it is.  The columns of a row are not split across workgroups, so a single
// small pair fills few CUs: the workload is a batch of pairs.
//
// The normalisation has no launch of its own.  Every workgroup reduces the three float64 sums r = sum v_i w_i, n = sum v_i^2
// and s2 = sum w_i^2 of its rows by the reduction of icp_sums.h into its row of the partials; the workgroups of the NEXT step
// add the pair's partial rows in tile order, form fp32(sqrt(s2)) and divide as they load the v plane (s2 == 0: v = 0, and
// everything after it stays 0).  The first step has v = 1.  hfl_spectral_finish, one wave per pair, does the same once more
// and writes the eigenvalue r / n, the score and v_K.  No atomics, no scratch, one writer per value: two runs give the same
// bits.  This file is built with -ffp-contract=off: the fmaf calls are explicit.
#include <math.h>

#include "icp_sums.h"
#include "pair_scan.h"

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_ROWS = HFL_SPECTRAL_ROWS;                       // rows (correspondences) of a workgroup
constexpr int SP_RPT = SP_ROWS / SP_THREADS;                     // rows a thread keeps in registers
constexpr int SP_TILE = HFL_SPECTRAL_TILE;                       // columns of one LDS tile
constexpr int SP_PLANES = 7;                                     // px, py, pz, qx, qy, qz, v
constexpr int SP_SUMS = HFL_SPECTRAL_SUMS;                       // r, n, s2
constexpr int SP_WAVES = SP_THREADS / HFL_WAVE;
static_assert(SP_ROWS % SP_THREADS == 0 && SP_RPT >= 1, "whole rows per thread");
static_assert(SP_TILE % 4 == 0 && SP_ROWS % 4 == 0, "whole groups of four columns");
static_assert(SP_TILE * SP_PLANES * 4 + SP_WAVES * SP_SUMS * 8 <= 32 * 1024, "static LDS stays at 32 KiB or less");

// m_ij for i != j: max(0, 1 - (|p_i - p_j| - |q_i - q_j|)^2 / sigma^2), symmetric to the bit
__device__ __forceinline__ float spectral_entry(const float (&p)[3], const float (&q)[3], float pjx, float pjy, float pjz,
                                                float qjx, float qjy, float qjz, float inv_s2) {
  const float a = pair_len(p[0] - pjx, p[1] - pjy, p[2] - pjz);
  const float b = pair_len(q[0] - qjx, q[1] - qjy, q[2] - qjz);
  const float e = a - b;
  return fmaxf(0.f, fmaf(-(e * e), inv_s2, 1.f));
}

// The sums (r, n, s2) of a pair: its rows of the partials in tile order.  The offsets are clamped to the table.
__device__ __forceinline__ void spectral_pair_sums(double (&s)[SP_SUMS], const double* __restrict__ partials,
                                                   const int64_t* __restrict__ tile_off, int64_t pair, int64_t n_tiles) {
  const int64_t t0 = max(tile_off[pair], (int64_t)0), t1 = min(tile_off[pair + 1], n_tiles);
#pragma unroll
  for (int k = 0; k < SP_SUMS; ++k) s[k] = 0.0;
  for (int64_t t = t0; t < t1; ++t) {
#pragma unroll
    for (int k = 0; k < SP_SUMS; ++k) s[k] += partials[SP_SUMS * t + k];
  }
}

// v_j of the step from the previous step's w_j: w_j / fp32(sqrt(s2)), an fp32 division; 0 where s2 == 0
__device__ __forceinline__ float spectral_normalised(float w, float norm) { return norm > 0.f ? w / norm : 0.f; }

// columns [k0, k1) of the tile in LDS, whole groups of four, against the thread's rows.  DIAG: a column may be a row's own
// correspondence (local column self[r]), whose entry is 0.
template <bool DIAG>
__device__ __forceinline__ void spectral_sweep(float (&acc)[SP_RPT], const float (*s_c)[SP_TILE], int k0, int k1,
                                               const float (&p)[SP_RPT][3], const float (&q)[SP_RPT][3],
                                               const int (&self)[SP_RPT], float inv_s2) {
#pragma unroll 2
  for (int k = k0; k < k1; k += 4) {
    float c[SP_PLANES][4];
#pragma unroll
    for (int a = 0; a < SP_PLANES; ++a) {
      const float4 v = *reinterpret_cast<const float4*>(&s_c[a][k]);
      c[a][0] = v.x, c[a][1] = v.y, c[a][2] = v.z, c[a][3] = v.w;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)                                  // ascending column
#pragma unroll
      for (int r = 0; r < SP_RPT; ++r) {
        float m = spectral_entry(p[r], q[r], c[0][u], c[1][u], c[2][u], c[3][u], c[4][u], c[5][u], inv_s2);
        if (DIAG) m = (k + u == self[r]) ? 0.f : m;
        acc[r] = fmaf(m, c[6][u], acc[r]);
      }
  }
}

__global__ void __launch_bounds__(SP_THREADS)
spectral_matvec_kernel(float* __restrict__ w_out, double* __restrict__ partials_out, const float* __restrict__ corr,
                       const int64_t* __restrict__ c_off, int64_t n_corr, const int64_t* __restrict__ tiles,
                       int64_t n_tiles, const int64_t* __restrict__ tile_off, const float* __restrict__ w_in,
                       const double* __restrict__ partials_in, int n_pairs, float inv_s2) {
  __shared__ __align__(16) float s_c[SP_PLANES][SP_TILE];
  __shared__ double red[SP_WAVES * SP_SUMS];
  const int64_t pair = tiles[2 * (int64_t)blockIdx.x], row0 = tiles[2 * (int64_t)blockIdx.x + 1];
  if (!(pair >= 0 && pair < n_pairs && row0 >= 0)) return;       // uniform: a table row that names no pair
  const int64_t begin = max(c_off[pair], (int64_t)0), end = min(c_off[pair + 1], n_corr);
  const int64_t r_end = min(end, row0 + SP_ROWS);
  if (row0 < begin || r_end <= row0) return;                     // uniform: no row of this workgroup lies in the pair

  const bool first = w_in == nullptr;                            // v_0 is all ones
  float norm = 1.f;
  if (!first) {
    double s[SP_SUMS];
    spectral_pair_sums(s, partials_in, tile_off, pair, n_tiles);
    norm = (float)sqrt(s[2]);
  }

  float p[SP_RPT][3], q[SP_RPT][3], acc[SP_RPT];
  int64_t row[SP_RPT];
#pragma unroll
  for (int r = 0; r < SP_RPT; ++r) {                             // a row past the end reads the last one and writes nothing
    row[r] = row0 + r * SP_THREADS + threadIdx.x;
    const float* c = corr + 6 * min(row[r], r_end - 1);
    p[r][0] = c[0], p[r][1] = c[1], p[r][2] = c[2], q[r][0] = c[3], q[r][1] = c[4], q[r][2] = c[5];
    acc[r] = 0.f;
  }

  for (int64_t tile = begin; tile < end; tile += SP_TILE) {
    const int len = (int)min((int64_t)SP_TILE, end - tile);
    const int len4 = (len + 3) & ~3;                             // the last tile is padded to whole groups of four
    __syncthreads();                                             // the previous tile has been read by every wave
    for (int k = threadIdx.x; k < 6 * len4; k += SP_THREADS) {   // consecutive lanes read consecutive floats
      const int j = k / 6, col = k - 6 * j;
      s_c[col][j] = j < len ? corr[6 * tile + k] : 0.f;          // padding: finite entries against v = 0
    }
    for (int k = threadIdx.x; k < len4; k += SP_THREADS)
      s_c[6][k] = k < len ? (first ? 1.f : spectral_normalised(w_in[tile + k], norm)) : 0.f;
    __syncthreads();

    // the columns [z0, z1) of this tile are the workgroup's own rows: only there can a column be a row's own correspondence
    const int z0 = (int)min(max(row0 - tile, (int64_t)0), (int64_t)len4) & ~3;
    const int z1 = min(((int)min(max(row0 + SP_ROWS - tile, (int64_t)0), (int64_t)len4) + 3) & ~3, len4);
    int self[SP_RPT];
#pragma unroll
    for (int r = 0; r < SP_RPT; ++r) {
      const int64_t at = row[r] - tile;
      self[r] = at >= 0 && at < SP_TILE ? (int)at : -1;
    }
    spectral_sweep<false>(acc, s_c, 0, z0, p, q, self, inv_s2);
    spectral_sweep<true>(acc, s_c, z0, z1, p, q, self, inv_s2);
    spectral_sweep<false>(acc, s_c, z1, len4, p, q, self, inv_s2);
  }

  double sums[SP_SUMS];
#pragma unroll
  for (int k = 0; k < SP_SUMS; ++k) sums[k] = 0.0;
#pragma unroll
  for (int r = 0; r < SP_RPT; ++r) {                             // a thread's rows in row order
    if (row[r] < r_end) {
      const double v = (double)(first ? 1.f : spectral_normalised(w_in[row[r]], norm)), w = (double)acc[r];
      w_out[row[r]] = acc[r];
      sums[0] += v * w;                                          // products of two widened fp32 values: exact
      sums[1] += v * v;
      sums[2] += w * w;
    }
  }
  icp_reduce_partials<SP_SUMS, SP_THREADS>(sums, red, partials_out);
}

__global__ void __launch_bounds__(HFL_WAVE)
spectral_finish_kernel(double* __restrict__ eigenvalue, double* __restrict__ score, float* __restrict__ weights,
                       const float* __restrict__ w, const double* __restrict__ partials, int64_t n_tiles,
                       const int64_t* __restrict__ tile_off, const int64_t* __restrict__ c_off, int64_t n_corr,
                       const int64_t* __restrict__ n_source) {
  const int64_t pair = blockIdx.x;
  double s[SP_SUMS];
  spectral_pair_sums(s, partials, tile_off, pair, n_tiles);
  const bool none = !(s[2] > 0.0);                               // C < 2 or no consistent pair of correspondences
  const float norm = (float)sqrt(s[2]);
  const double lambda = none ? 0.0 : s[0] / s[1];
  if (threadIdx.x == 0) {
    eigenvalue[pair] = lambda;
    score[pair] = lambda / (double)max(n_source[pair], (int64_t)1);
  }
  const int64_t begin = max(c_off[pair], (int64_t)0), end = min(c_off[pair + 1], n_corr);
  for (int64_t i = begin + threadIdx.x; i < end; i += HFL_WAVE) weights[i] = none ? 0.f : spectral_normalised(w[i], norm);
}

}  // namespace

extern "C" int hfl_spectral_matvec(float* w_out, double* partials_out, const float* corr, const int64_t* c_offsets,
                                   int64_t n_corr, const int64_t* tiles, int64_t n_tiles, const int64_t* tile_offsets,
                                   const float* w_in, const double* partials_in, int64_t n_pairs, float inv_sigma2,
                                   hfl_stream_t stream) {
  if (w_out == nullptr || partials_out == nullptr || corr == nullptr || c_offsets == nullptr || tiles == nullptr ||
      tile_offsets == nullptr || (w_in == nullptr) != (partials_in == nullptr) || w_in == w_out ||
      partials_in == partials_out || n_corr < 0 || n_tiles < 0 || n_pairs < 1 || !(inv_sigma2 > 0.f) || isinf(inv_sigma2))
    return HFL_EINVAL;
  if (n_corr > 0x7fffffffLL || n_tiles > 0x7fffffffLL || n_pairs > 0x7fffffffLL) return HFL_ECAPACITY;
  if (n_tiles == 0) return HFL_OK;
  spectral_matvec_kernel<<<(unsigned)n_tiles, SP_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      w_out, partials_out, corr, c_offsets, n_corr, tiles, n_tiles, tile_offsets, w_in, partials_in, (int)n_pairs, inv_sigma2);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int hfl_spectral_finish(double* eigenvalue, double* score, float* weights, const float* w, const double* partials,
                                   int64_t n_tiles, const int64_t* tile_offsets, const int64_t* c_offsets, int64_t n_corr,
                                   const int64_t* n_source, int64_t n_pairs, hfl_stream_t stream) {
  if (eigenvalue == nullptr || score == nullptr || weights == nullptr || w == nullptr || partials == nullptr ||
      tile_offsets == nullptr || c_offsets == nullptr || n_source == nullptr || n_corr < 0 || n_tiles < 0 || n_pairs < 1)
    return HFL_EINVAL;
  if (n_corr > 0x7fffffffLL || n_tiles > 0x7fffffffLL || n_pairs > 0x7fffffffLL) return HFL_ECAPACITY;
  spectral_finish_kernel<<<(unsigned)n_pairs, HFL_WAVE, 0, static_cast<hipStream_t>(stream)>>>(
      eigenvalue, score, weights, w, partials, n_tiles, tile_offsets, c_offsets, n_corr, n_source);
  HFL_RETURN_LAST_ERROR();
}
