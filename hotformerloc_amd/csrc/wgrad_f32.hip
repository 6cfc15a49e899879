// Weight gradient of a Linear layer on the fp32 matrix cores of gfx950 (the matched-precision leg, GEMM mode x6):
//
//     dW (N,K) = dy (M,N)^T . x (M,K)          db (N) = column sums of dy          (all f32 in memory)
//
// What autograd does for torch.nn.Linear in the reference's fp32 training step (training/trainer.py:344-362 over
// models/octformer_backbone.py:70,91 and models/layers/octformer_layers.py:53-59): a contraction over the ~10^5..10^6 token
// rows into a small (N,K) matrix plus a column reduction for the bias.
//
// Arithmetic: v_mfma_f32_16x16x4_f32 -- f32 operands, every product rounded once into an f32 FMA chain (the reference's own
// arithmetic, no operand split).  Its operand layout puts the contraction index on the lane group: lane (c, q) of an MFMA
// holds A[i = c][k = q] and B[k = q][j = c], i.e. element [row q][one channel of lane c] of BOTH row-major operands, so the
// operands are read as they lie in memory (as tap_wgrad_kernel in csrc/tapconv.hip does): lane c loads the 16 B of channels
// 4c .. 4c+3 of a row, one value per 16-channel MFMA block.
//
// Work split (as csrc/wgrad_x3.hip): 128 x 128 output tiles times S row slabs (S sized to the resident workgroups); wave
// (wn, wk) of a workgroup owns the 64 x 64 quarter (n0 + 64 wn, k0 + 64 wk) over all rows of its slab; partial tiles go to a
// workspace (S, N, K) and a second kernel adds the slabs in a fixed order: bitwise reproducible, no atomics.  The bias gradient
// rides in the waves wk = 0 of the first K tile (VALU adds of the dy values they hold anyway).
//
// Accumulation: a slab is up to ~2 x 10^4 rows; one chain that long has a rounding error of ~u sqrt(rows) relative.  Every
// WG_FLUSH rows the running products are added into a second accumulator and restarted, so the chains are WG_FLUSH and
// rows / WG_FLUSH long.
#include "hfl_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct WfParams {
  float* ws;                // (S, N, K) partial weight gradients
  float* wsb;               // (S, N) partial bias gradients or null
  const float* dy;          // (M, N)
  const float* x;           // (M, K)
  int64_t M;
  int N, K;
  int tiles_k, tiles;       // K / 128, (N / 128) * (K / 128)
  int64_t slab_rows;        // rows per slab (multiple of 16)
  int64_t n_wg;
};

constexpr int WG_FLUSH = 256;                   // rows per inner accumulation chain (a multiple of the 16-row group)

__global__ void __launch_bounds__(256, 2)
wgrad_f32_kernel(const WfParams p) {
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave >> 1, wk = wave & 1;
  const int c = lane & 15, q = lane >> 4;

  // consecutive new ids share an XCD (bijective remap): the tiles of one slab re-read its rows from one L2
  int64_t wg = blockIdx.x;
  {
    const int64_t qq = p.n_wg >> 3, r = p.n_wg & 7;
    const int64_t xcd = wg & 7, loc = wg >> 3;
    wg = (xcd < r ? xcd * (qq + 1) : r * (qq + 1) + (xcd - r) * qq) + loc;
  }
  const int64_t slab = wg / p.tiles;
  const int tile = (int)(wg % p.tiles);
  const int n0 = (tile / p.tiles_k) * 128 + wn * 64, k0 = (tile % p.tiles_k) * 128 + wk * 64;
  const int64_t m_begin = slab * p.slab_rows;
  const int64_t m_end = (m_begin + p.slab_rows < p.M) ? m_begin + p.slab_rows : p.M;
  const bool do_bias = p.wsb != nullptr && k0 == 0;                              // wave-uniform

  const float* dyl = p.dy + n0 + 4 * c;
  const float* xl = p.x + k0 + 4 * c;

  f32x4 acc[4][4], tot[4][4];
  float accb[4] = {0.f, 0.f, 0.f, 0.f}, totb[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      tot[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }

  // a 16-row group: four MFMA k-steps of 4 rows, row 4s + q of the group in operand slot s.  Every address is valid (a row
  // past M reads row M - 1; its values are zeroed before use), so nothing is loaded under a branch and the next group is
  // requested while this one's 64 MFMAs run.
  auto load = [&](int64_t m0, f32x4 (&a)[4], f32x4 (&b)[4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      int64_t m = m0 + 4 * s + q;
      m = m < p.M ? m : p.M - 1;
      a[s] = *reinterpret_cast<const f32x4*>(dyl + m * p.N);
      b[s] = *reinterpret_cast<const f32x4*>(xl + m * p.K);
    }
  };
  auto flush = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        tot[i][j] += acc[i][j];
        acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
      totb[i] += accb[i];
      accb[i] = 0.f;
    }
  };

  if (m_begin < m_end) {
    f32x4 a[4], b[4], an[4], bn[4];
    load(m_begin, a, b);
    int in_chain = 0;
    for (int64_t m0 = m_begin; m0 < m_end; m0 += 16) {
      load(m0 + 16, an, bn);                           // the next group (past the slab: valid rows, never used)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < 4; ++s) {                    // rows past the slab contribute nothing
        const bool ok = m0 + 4 * s + q < m_end;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          a[s][i] = ok ? a[s][i] : 0.f;
          b[s][i] = ok ? b[s][i] : 0.f;
        }
      }
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][i], b[s][j], acc[i][j], 0, 0, 0);
      if (do_bias) {                                   // VALU in the shadow of the MFMAs
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int i = 0; i < 4; ++i) accb[i] += a[s][i];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        a[s] = an[s];
        b[s] = bn[s];
      }
      in_chain += 16;
      if (in_chain == WG_FLUSH) {                      // (wave-uniform)
        flush();
        in_chain = 0;
      }
    }
    flush();
  }

  // ---- partial tile.  Block (i, j) of the wave: A row c <-> channel n0 + 4c + i, B column c <-> channel k0 + 4c + j; lane
  // (c, q) holds D rows 4q + e, column c: dW[n0 + 4 (4q + e) + i][k0 + 4c + j] = tot[i][j][e] -- for fixed (i, e) the four j
  // are 16 contiguous bytes, and the 16 lanes of a group write 256 contiguous bytes of one row
  float* wsl = p.ws + slab * (int64_t)p.N * p.K;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n = n0 + 4 * (4 * q + e) + i;
      *reinterpret_cast<f32x4*>(wsl + (int64_t)n * p.K + k0 + 4 * c) =
          (f32x4){tot[i][0][e], tot[i][1][e], tot[i][2][e], tot[i][3][e]};
    }
  if (do_bias) {                                       // lane (c, q) summed rows q (mod 4) of channels n0 + 4c + i: add the 4 q
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      totb[i] += __shfl_xor(totb[i], 16, 64);
      totb[i] += __shfl_xor(totb[i], 32, 64);
    }
    if (q == 0)
      *reinterpret_cast<f32x4*>(p.wsb + slab * (int64_t)p.N + n0 + 4 * c) = (f32x4){totb[0], totb[1], totb[2], totb[3]};
  }
}

// out[i] = sum over the S slabs in ascending order within 4 strided slab groups, the groups added 0..3 (fixed order); the bias
// gradient's slabs ride in the same launch (workgroups past `blocks_a`)
__global__ void __launch_bounds__(256)
wgrad_f32_reduce_kernel(float* out, const float* ws, int64_t n4, int S, int blocks_a, float* out_b, const float* ws_b,
                        int64_t n4_b) {
  __shared__ float4 part[4][64];
  const int col = threadIdx.x & 63, grp = threadIdx.x >> 6;
  int64_t blk = blockIdx.x;
  if ((int)blockIdx.x >= blocks_a) {               // (workgroup-uniform)
    blk -= blocks_a;
    out = out_b;
    ws = ws_b;
    n4 = n4_b;
  }
  const int64_t i = blk * 64 + col;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < n4) {
    const float4* src = reinterpret_cast<const float4*>(ws) + i;
    for (int s = grp; s < S; s += 4) {
      const float4 v = src[(int64_t)s * n4];
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
  }
  part[grp][col] = a;
  __syncthreads();
  if (grp == 0 && i < n4) {
    float4 r = part[0][col];
#pragma unroll
    for (int k = 1; k < 4; ++k) { r.x += part[k][col].x; r.y += part[k][col].y; r.z += part[k][col].z; r.w += part[k][col].w; }
    reinterpret_cast<float4*>(out)[i] = r;
  }
}

struct WfSplit { int S; int64_t slab_rows; };

// two resident 256-lane workgroups per CU (<= 256 registers per lane: two accumulator sets and two operand groups)
WfSplit wf_split(int64_t M, int64_t N, int64_t K) {
  const int64_t tiles = (N / 128) * (K / 128);
  int64_t S = hfl_cdiv(2 * (int64_t)hfl_num_cus(), tiles);
  const int64_t smax = hfl_cdiv(M, 256);               // at least 16 groups per slab
  if (S > smax) S = smax;
  if (S < 1) S = 1;
  const int64_t slab = hfl_cdiv(hfl_cdiv(M, S), 16) * 16;
  S = hfl_cdiv(M, slab);
  return {(int)S, slab};
}

bool wf_shape_ok(int64_t n_rows, int64_t out_features, int64_t in_features) {
  return n_rows > 0 && out_features > 0 && in_features > 0 && out_features % 128 == 0 && in_features % 128 == 0 &&
         out_features <= (1 << 20) && in_features <= (1 << 20);
}

}  // namespace

extern "C" {

int64_t hfl_wgrad_f32_workspace(int64_t n_rows, int64_t out_features, int64_t in_features) {
  if (!wf_shape_ok(n_rows, out_features, in_features)) return 0;
  const WfSplit sp = wf_split(n_rows, out_features, in_features);
  return (int64_t)sp.S * (out_features * in_features + out_features) * 4;
}

int hfl_wgrad_f32(float* dw, float* db, const float* dy, const float* x, int64_t n_rows, int64_t out_features,
                  int64_t in_features, void* workspace, hfl_stream_t stream) {
  if (!wf_shape_ok(n_rows, out_features, in_features)) return HFL_EINVAL;
  if (dw == nullptr || dy == nullptr || x == nullptr || workspace == nullptr) return HFL_EINVAL;
  const WfSplit sp = wf_split(n_rows, out_features, in_features);
  WfParams p;
  p.ws = static_cast<float*>(workspace);
  p.wsb = db != nullptr ? p.ws + (int64_t)sp.S * out_features * in_features : nullptr;
  p.dy = dy;
  p.x = x;
  p.M = n_rows;
  p.N = (int)out_features;
  p.K = (int)in_features;
  p.tiles_k = (int)(in_features / 128);
  p.tiles = (int)((out_features / 128) * (in_features / 128));
  p.slab_rows = sp.slab_rows;
  p.n_wg = (int64_t)sp.S * p.tiles;
  if (p.n_wg > 0x7fffffffLL) return HFL_ECAPACITY;
  hipStream_t s = static_cast<hipStream_t>(stream);
  wgrad_f32_kernel<<<(unsigned)p.n_wg, 256, 0, s>>>(p);
  const int64_t n4 = out_features * in_features / 4;
  const int blocks_a = (int)hfl_cdiv(n4, 64), blocks_b = db != nullptr ? (int)hfl_cdiv(out_features / 4, 64) : 0;
  wgrad_f32_reduce_kernel<<<(unsigned)(blocks_a + blocks_b), 256, 0, s>>>(dw, p.ws, n4, sp.S, blocks_a, db, p.wsb,
                                                                          out_features / 4);
  HFL_RETURN_LAST_ERROR();
}

}  // extern "C"
