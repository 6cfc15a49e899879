// Streamed flat-L2 top-k search (the FAISS GpuIndexFlatL2 search of eval/pnv_evaluate.py:199-223): for every query row the
// 32 nearest database rows by  ||q||^2 + ||d||^2 - 2 q.d,  without ever storing the (Q, N) distance matrix.
//
// Schedule.  A workgroup of four wavefronts owns a tile of 64 queries (16 per wavefront) and one SEGMENT of the database, a
// run of 128-row tiles.  Per database tile the 64 x D query slab and the 128 x D database slab go through LDS in 64-column
// chunks; every wavefront multiplies its 16 queries with all 128 rows on the fp32-input MFMA (v_mfma_f32_16x16x4_f32: eight
// 16 x 16 accumulator tiles).  That instruction is an fmaf chain in k order; the LDS image is laid out so that the four
// instructions of a 16-column block take k = 0..3, 4..7, 8..11, 12..15, each accumulator starts from zero and every column
// chunk is added in ascending order.  The dot product of a (query, row) pair therefore never depends on the tile, the segment
// or the launch shape that computed it, and neither do the two row norms (one fmaf chain per row, hfl_row_sq_norms).
//
// Selection.  Every wavefront keeps a sorted 32-entry (distance, index) list per query in LDS.  The key is the lexicographic
// pair (distance, index) EVERYWHERE: in the threshold test in front of the insertion (a candidate is dropped when its key is
// not below the list's last key), in the insertion, and in the merge of the segment lists.  A query's lists are private to
// one wavefront, so insertion needs no atomics: the wavefront ballots the lanes whose candidate passes, and for each of them
// the 32 list lanes find the position with one more ballot and shift the tail by one lane.  After the first tiles almost
// every ballot is empty and the selection costs four compares per 128 MFMAs.
//
// Segments.  With fewer than two query tiles per CU the database is cut into up to 64 segments (grid.y); each writes its 32
// entry list per query into the caller's workspace and hfl_flat_l2_merge_kernel (one wavefront per query) merges them with the
// same key.  One segment writes the result directly.  Non-finite descriptors are undefined behaviour of the ORDER only (no
// out-of-range access): indices stay in range because list slots start as (+inf, INT_MAX) and are never written out past
// min(k, N).
//
// Prefix search (hfl_flat_l2_topk_prefix, the PREFIX instantiations).  Query q sees the database rows [0, limits[q]) only:
// its limit takes the place of n_rows in the `pass` predicate and nowhere else, so a pair's distance is the value above and
// query q's list is what the unrestricted search returns for it against database[:limits[q]].  The tile loop holds
// __syncthreads(), so its bound is the workgroup's: the largest limit of the tile's 64 queries, read through LDS; with
// time-ordered queries the tiles above the diagonal are never staged.  A segment beyond a query's limit leaves that
// query's list at (+inf, INT_MAX), which the merge skips; the slots that stay unused leave as (+inf, -1).
#include "hfl_common.h"

#include <limits.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int QT = 64;          // queries per workgroup (16 per wavefront)
constexpr int NT = 128;         // database rows per tile
constexpr int KC = 64;          // columns per LDS chunk
constexpr int LDS_STRIDE = KC + 4;
constexpr int LIST = 32;        // entries of a running list
constexpr int MAX_SEGMENTS = 64;

__device__ __forceinline__ bool key_less(float da, int ia, float db, int ib) {
  return da < db || (da == db && ia < ib);
}

// One fmaf chain per row in ascending k: the value of a row's norm is the same wherever the row sits.
__global__ void __launch_bounds__(256)
row_sq_norms_kernel(float* __restrict__ out, const float* __restrict__ x, int64_t n, int d) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const float4* p = reinterpret_cast<const float4*>(x + r * d);
  float s = 0.f;
  for (int k = 0; k < d / 4; ++k) {
    const float4 v = p[k];
    s = fmaf(v.x, v.x, s);
    s = fmaf(v.y, v.y, s);
    s = fmaf(v.z, v.z, s);
    s = fmaf(v.w, v.w, s);
  }
  out[r] = s;
}

// rows [row0, row0 + ROWS) x columns [k0, k0 + KC) of a (n_rows, d) matrix -> LDS, zero outside the matrix.  A 16-column block
// is stored with column k at position (k % 4) * 4 + k / 4: the lane of MFMA k-group g then reads its four steps' operands
// (columns g, 4 + g, 8 + g, 12 + g) as one 16-byte LDS read.
template <int ROWS>
__device__ __forceinline__ void stage_chunk(float* __restrict__ s, const float* __restrict__ x, int64_t row0, int64_t n_rows,
                                            int d, int k0) {
  const int c4 = threadIdx.x & 15;                 // float4 column of the chunk
  const int blk = c4 >> 2, m = c4 & 3;
  const int k = k0 + c4 * 4;
#pragma unroll
  for (int it = 0; it < ROWS / 16; ++it) {
    const int r = it * 16 + (threadIdx.x >> 4);
    const int64_t gr = row0 + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (gr < n_rows && k < d) v = *reinterpret_cast<const float4*>(x + gr * d + k);
    float* dst = s + r * LDS_STRIDE + blk * 16 + m;
    dst[0] = v.x;
    dst[4] = v.y;
    dst[8] = v.z;
    dst[12] = v.w;
  }
}

// grid (query tiles, segments), 256 threads.  out_d / out_i: (Q, kc) when n_seg == 1, else the workspace lists
// (Q, n_seg, LIST).  PREFIX: limits (Q), query q takes rows below limits[q] clamped to [0, n_rows]; unused result slots get
// index -1.
template <bool PREFIX>
__global__ void __launch_bounds__(256)
flat_l2_topk_kernel(float* __restrict__ out_d, int* __restrict__ out_i, const float* __restrict__ queries,
                    const float* __restrict__ database, const float* __restrict__ q_norm, const float* __restrict__ d_norm,
                    int q_rows, int n_rows, int d, int kc, int tiles_per_seg, int n_seg, const int* __restrict__ limits) {
  __shared__ __attribute__((aligned(16))) float s_q[QT * LDS_STRIDE];
  __shared__ __attribute__((aligned(16))) float s_d[NT * LDS_STRIDE];
  __shared__ __attribute__((aligned(16))) float s_dn[NT];
  __shared__ float s_ld[QT * LIST];
  __shared__ int s_li[QT * LIST];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int64_t q0 = (int64_t)blockIdx.x * QT;
  const int seg = blockIdx.y;
  const int n_tiles = (n_rows + NT - 1) / NT;
  const int tile_lo = seg * tiles_per_seg;
  int tile_hi = min(n_tiles, tile_lo + tiles_per_seg);

  // the wavefront's 16 lists, and each lane's copy of the last key of its query's list
  float* ld = s_ld + wave * 16 * LIST;
  int* li = s_li + wave * 16 * LIST;
  for (int e = lane; e < 16 * LIST; e += 64) {
    ld[e] = INFINITY;
    li[e] = INT_MAX;
  }
  float thr_d = INFINITY;
  int thr_i = INT_MAX;
  const int64_t my_q = q0 + wave * 16 + c;
  const float qn = my_q < q_rows ? q_norm[my_q] : 0.f;

  // the rows this lane's query may take; the tile loop ends at the largest limit of the workgroup's queries
  int my_rows = n_rows;
  if constexpr (PREFIX) {
    __shared__ int s_lim[QT];
    if (threadIdx.x < QT) {
      const int64_t q = q0 + threadIdx.x;
      s_lim[threadIdx.x] = q < q_rows ? min(max(limits[q], 0), n_rows) : 0;
    }
    __syncthreads();
    int max_lim = 0;
    for (int e = 0; e < QT; ++e) max_lim = max(max_lim, s_lim[e]);
    my_rows = s_lim[wave * 16 + c];
    tile_hi = min(tile_hi, (max_lim + NT - 1) / NT);
  }

  for (int tile = tile_lo; tile < tile_hi; ++tile) {
    const int64_t row0 = (int64_t)tile * NT;
    f32x4 acc[NT / 16];
#pragma unroll
    for (int t = 0; t < NT / 16; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int k0 = 0; k0 < d; k0 += KC) {
      __syncthreads();                               // everyone is done with the previous chunk (and with s_dn)
      stage_chunk<QT>(s_q, queries, q0, q_rows, d, k0);
      stage_chunk<NT>(s_d, database, row0, n_rows, d, k0);
      if (k0 == 0 && threadIdx.x < NT) {
        const int64_t r = row0 + threadIdx.x;
        s_dn[threadIdx.x] = r < n_rows ? d_norm[r] : 0.f;
      }
      __syncthreads();
      const int kblocks = (min(KC, d - k0) + 15) / 16;
      for (int kb = 0; kb < kblocks; ++kb) {
        const f32x4 bq = *reinterpret_cast<const f32x4*>(s_q + (wave * 16 + c) * LDS_STRIDE + kb * 16 + g * 4);
        f32x4 a[NT / 16];
#pragma unroll
        for (int t = 0; t < NT / 16; ++t)
          a[t] = *reinterpret_cast<const f32x4*>(s_d + (t * 16 + c) * LDS_STRIDE + kb * 16 + g * 4);
#pragma unroll
        for (int step = 0; step < 4; ++step) {       // columns 4 step .. 4 step + 3 of the block: ascending k
#pragma unroll
          for (int t = 0; t < NT / 16; ++t)
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][step], bq[step], acc[t], 0, 0, 0);
        }
      }
    }

    // accumulator register r of tile t: database row row0 + 16 t + 4 g + r against query c of this wavefront
#pragma unroll
    for (int t = 0; t < NT / 16; ++t) {
      const f32x4 dn = *reinterpret_cast<const f32x4*>(s_dn + t * 16 + g * 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = row0 + t * 16 + g * 4 + r;
        const int idx = (int)row;
        const float dist = fmaf(-2.f, acc[t][r], qn + dn[r]);
        const bool pass = row < my_rows && key_less(dist, idx, thr_d, thr_i);
        unsigned long long mask = __ballot(pass);
        if (mask == 0) continue;
        while (mask != 0) {
          const int src = __ffsll(mask) - 1;
          mask &= mask - 1;
          const float cd = __shfl(dist, src, 64);
          const int ci = __shfl(idx, src, 64);
          const int slot = (src & 15) * LIST + (lane & 31);
          const float od = ld[slot];
          const int oi = li[slot];
          const int pos = __popcll(__ballot(key_less(od, oi, cd, ci)) & 0xffffffffull);
          const float pd = __shfl_up(od, 1, 64);
          const int pi = __shfl_up(oi, 1, 64);
          if (pos < LIST && lane < LIST && lane >= pos) {
            ld[slot] = lane == pos ? cd : pd;
            li[slot] = lane == pos ? ci : pi;
          }
          __builtin_amdgcn_wave_barrier();
        }
        thr_d = ld[c * LIST + LIST - 1];
        thr_i = li[c * LIST + LIST - 1];
      }
    }
  }

  // write the lists: the result itself, or this segment's partial lists
  __builtin_amdgcn_wave_barrier();
  const int width = n_seg == 1 ? kc : LIST;
  for (int e = lane; e < 16 * LIST; e += 64) {
    const int qq = e / LIST, slot = e % LIST;
    const int64_t q = q0 + wave * 16 + qq;
    if (q < q_rows && slot < width) {
      const int64_t o = n_seg == 1 ? q * kc + slot : (q * n_seg + seg) * LIST + slot;
      out_d[o] = ld[e];
      out_i[o] = PREFIX && n_seg == 1 && li[e] == INT_MAX ? -1 : li[e];
    }
  }
}

// One wavefront per query: lanes 0..31 hold the merged list; every segment's sorted list is fed in order and left as soon as
// one of its entries no longer fits (the rest are larger still).  PREFIX: a query may have found fewer than kc rows, or none
// in any segment; the slots left at (+inf, INT_MAX) get index -1.
template <bool PREFIX>
__global__ void __launch_bounds__(256)
flat_l2_merge_kernel(float* __restrict__ out_d, int* __restrict__ out_i, const float* __restrict__ part_d,
                     const int* __restrict__ part_i, int q_rows, int n_seg, int kc) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= q_rows) return;                          // whole wavefront leaves
  float md = INFINITY;
  int mi = INT_MAX;
  for (int s = 0; s < n_seg; ++s) {
    const int64_t base = (q * n_seg + s) * LIST;
    const float sd = lane < LIST ? part_d[base + lane] : INFINITY;
    const int si = lane < LIST ? part_i[base + lane] : INT_MAX;
    for (int e = 0; e < LIST; ++e) {
      const float cd = __shfl(sd, e, 64);
      const int ci = __shfl(si, e, 64);
      if (ci == INT_MAX) break;                     // an unused slot: the segment had fewer rows
      const int pos = __popcll(__ballot(key_less(md, mi, cd, ci)) & 0xffffffffull);
      if (pos >= LIST) break;
      const float pd = __shfl_up(md, 1, 64);
      const int pi = __shfl_up(mi, 1, 64);
      if (lane >= pos) {
        md = lane == pos ? cd : pd;
        mi = lane == pos ? ci : pi;
      }
    }
  }
  if (lane < kc) {
    out_d[q * kc + lane] = md;
    out_i[q * kc + lane] = PREFIX && mi == INT_MAX ? -1 : mi;
  }
}

struct Plan {
  int q_tiles, n_tiles, n_seg, tiles_per_seg;
};

bool shape_ok(int64_t q, int64_t n, int64_t d, int k) {
  return q >= 0 && n >= 1 && n <= INT_MAX - NT && q <= INT_MAX - QT && d >= 4 && d <= 1024 && d % 4 == 0 && k >= 1 && k <= LIST;
}

Plan make_plan(int64_t q, int64_t n) {
  Plan p;
  p.q_tiles = (int)hfl_cdiv(q, QT);
  p.n_tiles = (int)hfl_cdiv(n, NT);
  // two workgroups fit a CU: cut the database until the grid has that many, 64 segments at the most
  int want = p.q_tiles > 0 ? (int)hfl_cdiv(2 * (int64_t)hfl_num_cus(), p.q_tiles) : 1;
  if (want > MAX_SEGMENTS) want = MAX_SEGMENTS;
  if (want > p.n_tiles) want = p.n_tiles;
  if (want < 1) want = 1;
  p.tiles_per_seg = (int)hfl_cdiv(p.n_tiles, want);
  p.n_seg = (int)hfl_cdiv(p.n_tiles, p.tiles_per_seg);        // no empty segment
  return p;
}

int64_t align16(int64_t b) { return (b + 15) / 16 * 16; }

}  // namespace

extern "C" int hfl_row_sq_norms(float* out, const float* x, int64_t n_rows, int dim, hfl_stream_t stream) {
  if (n_rows < 0 || dim < 4 || dim > 1024 || dim % 4 != 0) return HFL_EINVAL;
  if (n_rows == 0) return HFL_OK;
  row_sq_norms_kernel<<<(unsigned)hfl_cdiv(n_rows, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(out, x, n_rows, dim);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int64_t hfl_flat_l2_topk_workspace(int64_t n_queries, int64_t n_database, int64_t dim, int k) {
  if (!shape_ok(n_queries, n_database, dim, k)) return -1;
  const Plan p = make_plan(n_queries, n_database);
  int64_t bytes = align16(n_queries * 4) + align16(n_database * 4);          // both norm vectors
  if (p.n_seg > 1) bytes += 2 * align16(n_queries * p.n_seg * LIST * 4);
  return bytes;
}

namespace {

// Both entry points: the same plan, workspace layout and launches.  PREFIX: kc = k whatever N, and `limits` per query.
template <bool PREFIX>
int launch_topk(float* dist, int32_t* idx, const float* queries, const float* database, const float* database_sq_norms,
                const int32_t* limits, int64_t n_queries, int64_t n_database, int dim, int k, void* workspace,
                int64_t workspace_bytes, hfl_stream_t stream) {
  if (!shape_ok(n_queries, n_database, dim, k)) return HFL_EINVAL;
  if (n_queries == 0) return HFL_OK;
  if (PREFIX && limits == nullptr) return HFL_EINVAL;
  if (workspace == nullptr || workspace_bytes < hfl_flat_l2_topk_workspace(n_queries, n_database, dim, k)) return HFL_EINVAL;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const Plan p = make_plan(n_queries, n_database);
  const int kc = PREFIX ? k : (int)(k < n_database ? k : n_database);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  float* q_norm = reinterpret_cast<float*>(ws);
  float* d_norm_ws = reinterpret_cast<float*>(ws + align16(n_queries * 4));
  float* part_d = reinterpret_cast<float*>(ws + align16(n_queries * 4) + align16(n_database * 4));
  int* part_i = reinterpret_cast<int*>(reinterpret_cast<unsigned char*>(part_d) + align16(n_queries * p.n_seg * LIST * 4));
  int rc = hfl_row_sq_norms(q_norm, queries, n_queries, dim, stream);
  if (rc != HFL_OK) return rc;
  const float* d_norm = database_sq_norms;
  if (d_norm == nullptr) {
    rc = hfl_row_sq_norms(d_norm_ws, database, n_database, dim, stream);
    if (rc != HFL_OK) return rc;
    d_norm = d_norm_ws;
  }
  const dim3 grid((unsigned)p.q_tiles, (unsigned)p.n_seg);
  if (p.n_seg == 1) {
    flat_l2_topk_kernel<PREFIX><<<grid, 256, 0, st>>>(dist, idx, queries, database, q_norm, d_norm, (int)n_queries,
                                                      (int)n_database, dim, kc, p.tiles_per_seg, 1, limits);
  } else {
    flat_l2_topk_kernel<PREFIX><<<grid, 256, 0, st>>>(part_d, part_i, queries, database, q_norm, d_norm, (int)n_queries,
                                                      (int)n_database, dim, kc, p.tiles_per_seg, p.n_seg, limits);
    flat_l2_merge_kernel<PREFIX><<<(unsigned)hfl_cdiv(n_queries, 4), 256, 0, st>>>(dist, idx, part_d, part_i, (int)n_queries,
                                                                                   p.n_seg, kc);
  }
  HFL_RETURN_LAST_ERROR();
}

}  // namespace

extern "C" int hfl_flat_l2_topk(float* dist, int32_t* idx, const float* queries, const float* database,
                                 const float* database_sq_norms, int64_t n_queries, int64_t n_database, int dim, int k,
                                 void* workspace, int64_t workspace_bytes, hfl_stream_t stream) {
  return launch_topk<false>(dist, idx, queries, database, database_sq_norms, nullptr, n_queries, n_database, dim, k, workspace,
                            workspace_bytes, stream);
}

extern "C" int hfl_flat_l2_topk_prefix(float* dist, int32_t* idx, const float* queries, const float* database,
                                        const float* database_sq_norms, const int32_t* limits, int64_t n_queries,
                                        int64_t n_database, int dim, int k, void* workspace, int64_t workspace_bytes,
                                        hfl_stream_t stream) {
  return launch_topk<true>(dist, idx, queries, database, database_sq_norms, limits, n_queries, n_database, dim, k, workspace,
                           workspace_bytes, stream);
}
