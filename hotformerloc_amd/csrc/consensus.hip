// Consensus registration of a ragged batch of P pairs from point correspondences: the compatibility graph of a pair's
// correspondences as a bit matrix, and one pose hypothesis per seed from the seed's second-order consensus set.  The
// definition is in hotformerloc_amd/consensus.py and DESIGN.md section 7q.  The correspondences come as hfl_ransac_score takes
// them: (C, 6) fp32 rows (px, py, pz, qx, qy, qz) with (P + 1) int64 offsets.
//
// The graph of pair p lies at bits + word_offsets[p]: C rows of W = 4 ceil(C / 128) 32-bit words, row-major, bit (j & 31) of
// word (j >> 5) of row i = B_ij; the bits past column C - 1 are 0.  The host computes the word offsets (it knows every C) and
// the total, which the kernels take as the bound of every access: a wrong table makes a workgroup return, not write.
//
// hfl_consensus_graph: spectral_matvec_kernel with other arithmetic and a bit output.  A workgroup owns CG_ROWS rows of one
// pair (two per thread in registers: p_i, q_i) and streams ALL of the pair's correspondences past them as columns, in ascending
// order, through LDS tiles of CG_TILE columns held as six planes, which every lane reads by the same 16-byte broadcast loads.
// An entry is six subtractions, two d2 chains, two correctly rounded roots, a subtraction, and a compare of the magnitude.  A
// thread packs 32 decisions of a row into one word; a word is masked once -- the columns past the pair's end, and the row's
// own column where the word holds it (B_ii = 0 costs three integer operations per word, not one per entry) -- counted by
// popcount into the row's degree and, four words at a time, stored by one 16-byte store straight into the row: each thread
// writes 128 consecutive bytes of its own row per tile.  The stores are one bit per entry against some thirty VALU
// operations per entry: they are not transposed through LDS for coalescing.
//
// hfl_consensus_poses: one workgroup per (pair, seed slot).  The seed's row B_s goes into LDS (at most 2 KiB); the four waves
// take the words of B_s in turn and, for every set bit j, the lanes stride over the words of rows s and j with AND +
// popcount and add by the xor butterfly: n_sj, a 16-bit count in LDS (at most 32 KiB; 0 where B_sj = 0).  Then consensus_size - 1
// rounds of a workgroup arg-max on the key (n << 16 | 0xffff - j) -- the largest n, of equal ones the lowest j -- each of which
// takes its winner out; a round without a count >= 1 ends them.  The members are ranked into ascending order, one lane adds
// their 17 float64 sums in that order and calls kabsch_solve (kabsch.h).  No atomics, no scratch, one writer per value: two
// runs give the same bits.  This file is built with -ffp-contract=off.
#include <math.h>

#include "kabsch.h"
#include "pair_scan.h"

namespace {

constexpr int CG_THREADS = 256;
constexpr int CG_ROWS = HFL_CONSENSUS_ROWS;                      // rows (correspondences) of a workgroup of the graph kernel
constexpr int CG_RPT = CG_ROWS / CG_THREADS;                     // rows a thread keeps in registers
constexpr int CG_TILE = HFL_CONSENSUS_TILE;                      // columns of one LDS tile
constexpr int CG_GROUP = 128;                                    // columns of one 16-byte store
constexpr int CP_THREADS = 256;
constexpr int CP_WAVES = CP_THREADS / HFL_WAVE;
constexpr int CP_MAX_C = HFL_CONSENSUS_MAX_CORRESPONDENCES;
constexpr int CP_MAX_WORDS = CP_MAX_C / 32;
constexpr int CP_MAX_SIZE = HFL_CONSENSUS_MAX_SIZE;
constexpr int CP_SUMS = 17;
static_assert(CG_ROWS % CG_THREADS == 0 && CG_RPT >= 1, "whole rows per thread");
static_assert(CG_TILE % CG_GROUP == 0 && CG_TILE * 24 <= 32 * 1024, "whole store groups, static LDS at 32 KiB or less");
static_assert(CP_MAX_C % CG_GROUP == 0 && CP_MAX_C <= 0x10000, "a column index and a count fit 16 bits");
static_assert(CP_MAX_SIZE <= HFL_WAVE, "the members are ranked by one wave's worth of threads");

// The graph of one pair: rows [0, c) of `words` 32-bit words at `base`.  false where the table does not fit the array.
struct Graph {
  int64_t begin, base;
  int c, words;
};
__device__ __forceinline__ bool graph_of(Graph& g, int64_t pair, const int64_t* __restrict__ c_off, int64_t n_corr,
                                         const int64_t* __restrict__ word_off, int64_t n_words) {
  g.begin = min(max(c_off[pair], (int64_t)0), n_corr);
  const int64_t c = min(c_off[pair + 1], n_corr) - g.begin;
  g.base = word_off[pair];
  if (c < 0 || c > CP_MAX_C || g.base < 0 || (g.base & 3) != 0) return false;
  g.c = (int)c;
  g.words = 4 * ((g.c + CG_GROUP - 1) / CG_GROUP);
  return g.base + (int64_t)g.c * g.words <= n_words;
}

// B_ij for i != j: | |p_i - p_j| - |q_i - q_j| | <= d, symmetric operation for operation
__device__ __forceinline__ uint32_t consensus_bit(const float (&p)[3], const float (&q)[3], float pjx, float pjy, float pjz,
                                                  float qjx, float qjy, float qjz, float d) {
  const float a = pair_len(p[0] - pjx, p[1] - pjy, p[2] - pjz);
  const float b = pair_len(q[0] - qjx, q[1] - qjy, q[2] - qjz);
  const float e = a - b;
  return fabsf(e) <= d ? 1u : 0u;
}

// 127 VGPRs as built, 24 KiB of static LDS, no scratch: four waves per SIMD, as spectral_matvec_kernel.
__global__ void __launch_bounds__(CG_THREADS)
consensus_graph_kernel(uint32_t* __restrict__ bits, int32_t* __restrict__ degree, const float* __restrict__ corr,
                       const int64_t* __restrict__ c_off, int64_t n_corr, const int64_t* __restrict__ tiles,
                       const int64_t* __restrict__ word_off, int64_t n_words, int n_pairs, float d) {
  __shared__ __align__(16) float s_c[6][CG_TILE];                // px, py, pz, qx, qy, qz
  const int64_t pair = tiles[2 * (int64_t)blockIdx.x], row0 = tiles[2 * (int64_t)blockIdx.x + 1];
  if (!(pair >= 0 && pair < n_pairs && row0 >= 0)) return;       // uniform: a table row that names no pair
  Graph g;
  if (!graph_of(g, pair, c_off, n_corr, word_off, n_words)) return;
  const int64_t end = g.begin + g.c;
  if (row0 < g.begin || row0 >= end) return;                     // uniform: no row of this workgroup lies in the pair
  const int first = (int)(row0 - g.begin);                       // the workgroup's first row within the pair

  float p[CG_RPT][3], q[CG_RPT][3];
  int row[CG_RPT];                                               // within the pair
  int32_t deg[CG_RPT];
#pragma unroll
  for (int r = 0; r < CG_RPT; ++r) {                             // a row past the end reads the last one and writes nothing
    row[r] = first + r * CG_THREADS + (int)threadIdx.x;
    const float* c = corr + 6 * (g.begin + min(row[r], g.c - 1));
    p[r][0] = c[0], p[r][1] = c[1], p[r][2] = c[2], q[r][0] = c[3], q[r][1] = c[4], q[r][2] = c[5];
    deg[r] = 0;
  }

  for (int col0 = 0; col0 < g.c; col0 += CG_TILE) {              // the tile's first column within the pair
    const int len = min(CG_TILE, g.c - col0);
    const int len_g = (len + CG_GROUP - 1) & ~(CG_GROUP - 1);    // the last tile is padded to whole store groups
    __syncthreads();                                             // the previous tile has been read by every wave
    for (int k = threadIdx.x; k < 6 * len_g; k += CG_THREADS) {  // consecutive lanes read consecutive floats
      const int j = k / 6, col = k - 6 * j;
      s_c[col][j] = j < len ? corr[6 * (g.begin + col0) + k] : 0.f;      // padding: finite, and masked below
    }
    __syncthreads();

    for (int grp = 0; grp < len_g; grp += CG_GROUP) {
      uint32_t word[CG_RPT][4];
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int k0 = grp + 32 * w;                             // the word's first column within the tile
        uint32_t acc[CG_RPT];
#pragma unroll
        for (int r = 0; r < CG_RPT; ++r) acc[r] = 0u;
#pragma unroll 1                                                 // unrolled further the kernel passes 128 VGPRs: three waves
        for (int k = 0; k < 32; k += 4) {
          float c[6][4];
#pragma unroll
          for (int a = 0; a < 6; ++a) {
            const float4 v = *reinterpret_cast<const float4*>(&s_c[a][k0 + k]);
            c[a][0] = v.x, c[a][1] = v.y, c[a][2] = v.z, c[a][3] = v.w;
          }
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int r = 0; r < CG_RPT; ++r)
              acc[r] |= consensus_bit(p[r], q[r], c[0][u], c[1][u], c[2][u], c[3][u], c[4][u], c[5][u], d) << (k + u);
        }
        const int real = min(max(len - k0, 0), 32);              // the word's columns that exist
        const uint32_t exist = real >= 32 ? 0xffffffffu : (1u << real) - 1u;
#pragma unroll
        for (int r = 0; r < CG_RPT; ++r) {
          const uint32_t self = (uint32_t)(row[r] - (col0 + k0));        // the row's own column, if this word holds it
          word[r][w] = acc[r] & exist & ~(self < 32u ? 1u << self : 0u);
          deg[r] += __popc(word[r][w]);
        }
      }
#pragma unroll
      for (int r = 0; r < CG_RPT; ++r)
        if (row[r] < g.c)                                        // 16-byte aligned: base, words and the group are multiples of 4
          *reinterpret_cast<uint4*>(bits + g.base + (int64_t)row[r] * g.words + ((col0 + grp) >> 5)) =
              make_uint4(word[r][0], word[r][1], word[r][2], word[r][3]);
    }
  }
#pragma unroll
  for (int r = 0; r < CG_RPT; ++r)
    if (row[r] < g.c) degree[g.begin + row[r]] = deg[r];
}

// the largest value over the wave by the xor butterfly, the same in every lane
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int m = HFL_WAVE / 2; m > 0; m >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, m, HFL_WAVE));
  return v;
}

// 34.6 KiB of static LDS (four workgroups per CU), no scratch: the float64 solve runs in one lane's registers.
__global__ void __launch_bounds__(CP_THREADS)
consensus_poses_kernel(float* __restrict__ poses, uint8_t* __restrict__ valid, int32_t* __restrict__ members,
                       int32_t* __restrict__ support, const int32_t* __restrict__ seeds, const uint32_t* __restrict__ bits,
                       const int64_t* __restrict__ word_off, int64_t n_words, const float* __restrict__ corr,
                       const int64_t* __restrict__ c_off, int64_t n_corr, int n_seeds, int k1) {
  __shared__ uint32_t s_row[CP_MAX_WORDS];
  __shared__ uint16_t s_n[CP_MAX_C];
  __shared__ uint32_t s_red[CP_WAVES];
  __shared__ int32_t s_pick[CP_MAX_SIZE], s_member[CP_MAX_SIZE];
  __shared__ int32_t s_support;
  const int64_t slot = blockIdx.x, pair = slot / n_seeds;
  const int tid = threadIdx.x, lane = tid & (HFL_WAVE - 1), wave = tid / HFL_WAVE;
  float* pose = poses + 12 * slot;
  int32_t* mem = members + slot * k1;

  Graph g;
  const bool fits = graph_of(g, pair, c_off, n_corr, word_off, n_words);
  const int s = seeds[slot];
  int m = 0;                                                     // the size of the consensus set, uniform
  if (fits && s >= 0 && s < g.c) {
    const uint32_t* rows = bits + g.base;
    for (int k = tid; k < g.words; k += CP_THREADS) s_row[k] = rows[(int64_t)s * g.words + k];
    for (int j = tid; j < g.c; j += CP_THREADS) s_n[j] = 0;
    __syncthreads();

    for (int wi = wave; wi < g.words; wi += CP_WAVES) {          // n_sj of every set bit j: uniform over the wave
      uint32_t word = s_row[wi];
      while (word != 0u) {
        const int j = 32 * wi + __ffs((int)word) - 1;
        word &= word - 1u;
        if (j >= g.c) break;                                     // padding bits are 0: not reached
        const uint32_t* rj = rows + (int64_t)j * g.words;
        int32_t n = 0;
        for (int k = lane; k < g.words; k += HFL_WAVE) n += __popc(s_row[k] & rj[k]);
        n = wave_sum(n);
        if (lane == 0) s_n[j] = (uint16_t)n;                     // n <= C - 2 < 2^16
      }
    }
    __syncthreads();

    int picks = 0;
    for (; picks < k1 - 1; ++picks) {                            // the largest n >= 1, of equal ones the lowest j
      uint32_t key = 0u;
      for (int j = tid; j < g.c; j += CP_THREADS) {
        const uint32_t n = s_n[j];
        key = max(key, n != 0u ? (n << 16) | (0xffffu - (uint32_t)j) : 0u);
      }
      key = wave_max(key);
      if (lane == 0) s_red[wave] = key;
      __syncthreads();
      uint32_t best = s_red[0];
#pragma unroll
      for (int w = 1; w < CP_WAVES; ++w) best = max(best, s_red[w]);
      if (best == 0u) break;                                     // uniform: nothing qualifies any more
      if (tid == 0) {
        const int j = (int)(0xffffu - (best & 0xffffu));
        s_pick[picks] = j;
        s_n[j] = 0;
        s_support = (int32_t)(best >> 16);                       // the last one taken is the weakest member
      }
      __syncthreads();                                           // also: s_red is free for the next round
    }
    m = picks + 1;
    __syncthreads();
    if (tid < m) {                                               // ascending members: a member's place is its rank
      const int mine = tid < picks ? s_pick[tid] : s;
      int rank = 0;
      for (int u = 0; u < m; ++u) rank += (u < picks ? s_pick[u] : s) < mine ? 1 : 0;
      s_member[rank] = mine;                                     // the members are distinct: j != s, each j taken once
    }
    __syncthreads();
  }
  if (tid != 0) return;

  double r[3][3], t[3];
  bool ok = m >= 3;
  if (ok) {
    double sums[CP_SUMS];
#pragma unroll
    for (int k = 0; k < CP_SUMS; ++k) sums[k] = 0.0;
    sums[0] = (double)m;
    for (int u = 0; u < m; ++u) {                                // one accumulator per sum, ascending member order
      const float* c = corr + 6 * (g.begin + s_member[u]);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        sums[1 + a] += (double)c[a];
        sums[4 + a] += (double)c[3 + a];
#pragma unroll
        for (int b = 0; b < 3; ++b) sums[7 + 3 * a + b] += (double)c[a] * (double)c[3 + b];      // an exact product
      }
    }
    ok = kabsch_solve(sums, r, t);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) pose[4 * a + b] = ok ? (float)r[a][b] : NAN;
    pose[4 * a + 3] = ok ? (float)t[a] : NAN;
  }
  valid[slot] = ok ? 1 : 0;
  support[slot] = ok ? s_support : 0;
  for (int u = 0; u < k1; ++u) mem[u] = ok && u < m ? s_member[u] : -1;
}

}  // namespace

extern "C" int hfl_consensus_graph(uint32_t* bits, int32_t* degree, const float* corr, const int64_t* c_offsets,
                                   int64_t n_corr, const int64_t* tiles, int64_t n_tiles, const int64_t* word_offsets,
                                   int64_t n_words, int64_t n_pairs, float distance, hfl_stream_t stream) {
  if (bits == nullptr || degree == nullptr || corr == nullptr || c_offsets == nullptr || tiles == nullptr ||
      word_offsets == nullptr || n_corr < 0 || n_tiles < 0 || n_words < 0 || n_pairs < 1 || !(distance > 0.f) ||
      isinf(distance) || (reinterpret_cast<uintptr_t>(bits) & 15) != 0)
    return HFL_EINVAL;
  if (n_corr > 0x7fffffffLL || n_tiles > 0x7fffffffLL || n_pairs > 0x7fffffffLL) return HFL_ECAPACITY;
  if (n_tiles == 0) return HFL_OK;
  consensus_graph_kernel<<<(unsigned)n_tiles, CG_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      bits, degree, corr, c_offsets, n_corr, tiles, word_offsets, n_words, (int)n_pairs, distance);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int hfl_consensus_poses(float* poses, uint8_t* valid, int32_t* members, int32_t* support, const int32_t* seeds,
                                   const uint32_t* bits, const int64_t* word_offsets, int64_t n_words, const float* corr,
                                   const int64_t* c_offsets, int64_t n_corr, int64_t n_pairs, int64_t n_seeds,
                                   int64_t consensus_size, hfl_stream_t stream) {
  if (poses == nullptr || valid == nullptr || members == nullptr || support == nullptr || seeds == nullptr ||
      bits == nullptr || word_offsets == nullptr || corr == nullptr || c_offsets == nullptr || n_corr < 0 || n_words < 0 ||
      n_pairs < 1 || n_seeds < 1 || consensus_size < 3 || consensus_size > CP_MAX_SIZE)
    return HFL_EINVAL;
  if (n_corr > 0x7fffffffLL || n_pairs > 0x7fffffffLL || n_seeds > 0x7fffffffLL || n_pairs * n_seeds > 0x7fffffffLL)
    return HFL_ECAPACITY;
  consensus_poses_kernel<<<(unsigned)(n_pairs * n_seeds), CP_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      poses, valid, members, support, seeds, bits, word_offsets, n_words, corr, c_offsets, n_corr, (int)n_seeds,
      (int)consensus_size);
  HFL_RETURN_LAST_ERROR();
}
