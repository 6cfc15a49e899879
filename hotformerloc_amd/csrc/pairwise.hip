// Euclidean affinity of the TruncatedSmoothAP loss (reference: models/losses/loss_utils.py:55-60, `-torch.cdist(E, E)`,
// which is what every shipped training config selects: misc/utils.py:204).  tau1 = 0.01 multiplies every rounding error of
// the affinity by 100 inside the loss's sigmoid, and the pairs that carry the gradient (a query and its closest positives)
// are the near ones, for which |x|^2 + |y|^2 - 2 x.y cancels.  Both kernels therefore work on the differences themselves:
//     dist[i,j] = sqrt(sum_k (e_ik - e_jk)^2),         dE_i = sum_j (g_ij + g_ji) (e_i - e_j) / d_ij   (0 where d_ij == 0).
// fp32, plain VALU code, no atomics; every output element has one writer and a fixed summation order.
#include "hfl_common.h"

namespace {

constexpr int PW_TILE = 64;                   // forward: 64 x 64 outputs per workgroup, 4 x 4 per thread
constexpr int PW_KC = 32;                     // forward: D-chunk staged in LDS per step
constexpr int PW_LDK = PW_TILE + 4;           // k-major rows of 64 + 4 floats: 16-byte aligned, float4 reads conflict-free
constexpr int PW_LDT = PW_TILE + 1;           // transposed result tile

// 64 rows x PW_KC columns of E from (row0, k0), zero beyond B and D, into registers: thread t holds the float4 (row q / 8,
// columns 4 (q % 8)..) for q = t and t + 256.
template <bool VEC>
__device__ __forceinline__ void pw_load_rows(float4 (&r)[2], const float* __restrict__ E, int row0, int k0, int B, int D) {
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int q = threadIdx.x + 256 * m;
    const int row = row0 + (q >> 3), k = k0 + (q & 7) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < B) {
      const float* p = E + (int64_t)row * D + k;
      if (VEC) {                                              // D % 4 == 0: k < D implies k + 3 < D, and p is 16-byte aligned
        if (k < D) v = *reinterpret_cast<const float4*>(p);
      } else {
        if (k < D) v.x = p[0];
        if (k + 1 < D) v.y = p[1];
        if (k + 2 < D) v.z = p[2];
        if (k + 3 < D) v.w = p[3];
      }
    }
    r[m] = v;
  }
}

__device__ __forceinline__ void pw_store_rows(float* __restrict__ s, const float4 (&r)[2]) {      // s[k][row], k-major
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int q = threadIdx.x + 256 * m;
    const int row = q >> 3, k = (q & 7) * 4;
    s[(k + 0) * PW_LDK + row] = r[m].x;
    s[(k + 1) * PW_LDK + row] = r[m].y;
    s[(k + 2) * PW_LDK + row] = r[m].z;
    s[(k + 3) * PW_LDK + row] = r[m].w;
  }
}

// Tiles on or above the diagonal only.  (a - b)^2 and (b - a)^2 are the same float and both triangles of a diagonal tile add
// them in the same order, so a diagonal tile is bitwise symmetric as computed; every other tile is written twice, the second
// time transposed through LDS so that both writes are row-contiguous.
template <bool VEC>
__global__ void __launch_bounds__(256)
pairwise_dist_kernel(float* __restrict__ dist, const float* __restrict__ E, int B, int D) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bi > bj) return;
  __shared__ __attribute__((aligned(16))) float smem[2 * PW_KC * PW_LDK];
  static_assert(2 * PW_KC * PW_LDK >= PW_TILE * PW_LDT, "the transposed tile reuses the staging buffers");
  float* sA = smem;                                           // [PW_KC][PW_LDK] rows of tile bi
  float* sB = bi == bj ? sA : smem + PW_KC * PW_LDK;          // rows of tile bj
  const bool diag = bi == bj;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  float acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
  float4 ra[2], rb[2];
  pw_load_rows<VEC>(ra, E, bi * PW_TILE, 0, B, D);
  if (!diag) pw_load_rows<VEC>(rb, E, bj * PW_TILE, 0, B, D);
  for (int k0 = 0; k0 < D; k0 += PW_KC) {
    pw_store_rows(sA, ra);
    if (!diag) pw_store_rows(sB, rb);
    __syncthreads();
    if (k0 + PW_KC < D) {                                     // next chunk's loads fly under this chunk's arithmetic
      pw_load_rows<VEC>(ra, E, bi * PW_TILE, k0 + PW_KC, B, D);
      if (!diag) pw_load_rows<VEC>(rb, E, bj * PW_TILE, k0 + PW_KC, B, D);
    }
#pragma unroll 8
    for (int k = 0; k < PW_KC; ++k) {
      const float4 a4 = *reinterpret_cast<const float4*>(sA + k * PW_LDK + ty * 4);
      const float4 b4 = *reinterpret_cast<const float4*>(sB + k * PW_LDK + tx * 4);
      const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float d = a[r] - b[c];
          acc[r][c] = fmaf(d, d, acc[r][c]);
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = sqrtf(acc[r][c]);
  const int i0 = bi * PW_TILE, j0 = bj * PW_TILE;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + ty * 4 + r;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = j0 + tx * 4 + c;
      if (i < B && j < B) dist[(int64_t)i * B + j] = acc[r][c];
    }
  }
  if (diag) return;
  float* sT = smem;                                           // [PW_TILE][PW_LDT]; the k loop's last barrier freed it
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) sT[(ty * 4 + r) * PW_LDT + tx * 4 + c] = acc[r][c];
  __syncthreads();
  const int il = threadIdx.x & 63;
  for (int jl = threadIdx.x >> 6; jl < PW_TILE; jl += 4) {
    const int i = i0 + il, j = j0 + jl;
    if (i < B && j < B) dist[(int64_t)j * B + i] = sT[il * PW_LDT + jl];
  }
}

constexpr int PB_ROWS = 32;                   // backward: 32 rows x 64 columns of dE per workgroup, 2 x 4 per thread
constexpr int PB_COLS = 64;
constexpr int PB_J = 64;                      // rows e_j per step
constexpr int PB_LDG = PB_J + 1;              // g_ij / d_ij tiles [i][j], read transposed
constexpr int PB_LDW = PB_ROWS + 2;           // weights [j][i]: even, so the pair of a thread's rows is one 8-byte read
constexpr int PB_LDE = PB_COLS + 4;           // e_j tile [j][k]

struct PbTile {                               // one step's operands in registers
  float g[8], d[8], gt[8];                    // g_ij, d_ij at (i = e / 64, j = e % 64); g_ji at (j = e / 32, i = e % 32); e = t + 256 m
  float4 e[4];                                // e_j: (j = q / 16, k = 4 (q % 16)..), q = t + 256 m
};

template <bool VEC>
__device__ __forceinline__ void pb_load(PbTile& t, const float* __restrict__ G, const float* __restrict__ Dm,
                                        const float* __restrict__ E, int i0, int j0, int k0, int B, int D) {
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int e = threadIdx.x + 256 * m;
    const int i = i0 + (e >> 6), j = j0 + (e & 63);
    const bool ok = i < B && j < B;
    t.g[m] = ok ? G[(int64_t)i * B + j] : 0.f;
    t.d[m] = ok ? Dm[(int64_t)i * B + j] : 0.f;
    const int jt = j0 + (e >> 5), it = i0 + (e & 31);
    t.gt[m] = (it < B && jt < B) ? G[(int64_t)jt * B + it] : 0.f;
  }
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int q = threadIdx.x + 256 * m;
    const int j = j0 + (q >> 4), k = k0 + (q & 15) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < B) {
      const float* p = E + (int64_t)j * D + k;
      if (VEC) {
        if (k < D) v = *reinterpret_cast<const float4*>(p);
      } else {
        if (k < D) v.x = p[0];
        if (k + 1 < D) v.y = p[1];
        if (k + 2 < D) v.z = p[2];
        if (k + 3 < D) v.w = p[3];
      }
    }
    t.e[m] = v;
  }
}

// Workgroup (x, y) owns dE[32 y .. 32 y + 31][64 x .. 64 x + 63] and walks all rows j in steps of 64.  Per step the
// weights w_ij = (g_ij + g_ji) / d_ij are built once in LDS: g_ij and d_ij arrive row-contiguous in j, g_ji row-contiguous
// in i, and the transposition happens in LDS (no strided global load).  Then acc_ik += w_ij (e_ik - e_jk), j ascending.
template <bool VEC>
__global__ void __launch_bounds__(256)
pairwise_dist_bwd_kernel(float* __restrict__ dE, const float* __restrict__ G, const float* __restrict__ Dm,
                         const float* __restrict__ E, int B, int D) {
  __shared__ __attribute__((aligned(16))) float sG[PB_ROWS * PB_LDG];
  __shared__ __attribute__((aligned(16))) float sD[PB_ROWS * PB_LDG];
  __shared__ __attribute__((aligned(16))) float sW[PB_J * PB_LDW];
  __shared__ __attribute__((aligned(16))) float sE[PB_J * PB_LDE];
  const int i0 = blockIdx.y * PB_ROWS, k0 = blockIdx.x * PB_COLS;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  float ei[2][4], acc[2][4];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + ty * 2 + r, k = k0 + tx * 4 + c;
      ei[r][c] = (i < B && k < D) ? E[(int64_t)i * D + k] : 0.f;
      acc[r][c] = 0.f;
    }
  PbTile t;
  pb_load<VEC>(t, G, Dm, E, i0, 0, k0, B, D);
  for (int j0 = 0; j0 < B; j0 += PB_J) {
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int e = threadIdx.x + 256 * m;
      sG[(e >> 6) * PB_LDG + (e & 63)] = t.g[m];
      sD[(e >> 6) * PB_LDG + (e & 63)] = t.d[m];
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int q = threadIdx.x + 256 * m;
      *reinterpret_cast<float4*>(sE + (q >> 4) * PB_LDE + (q & 15) * 4) = t.e[m];
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int e = threadIdx.x + 256 * m;
      const int jl = e >> 5, il = e & 31;
      const float d = sD[il * PB_LDG + jl];
      sW[jl * PB_LDW + il] = d > 0.f ? (sG[il * PB_LDG + jl] + t.gt[m]) / d : 0.f;      // coincident rows: no contribution
    }
    __syncthreads();
    if (j0 + PB_J < B) pb_load<VEC>(t, G, Dm, E, i0, j0 + PB_J, k0, B, D);             // under this step's arithmetic
#pragma unroll 8
    for (int j = 0; j < PB_J; ++j) {
      const float2 w = *reinterpret_cast<const float2*>(sW + j * PB_LDW + ty * 2);
      const float4 e4 = *reinterpret_cast<const float4*>(sE + j * PB_LDE + tx * 4);
      const float ej[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        acc[0][c] = fmaf(w.x, ei[0][c] - ej[c], acc[0][c]);
        acc[1][c] = fmaf(w.y, ei[1][c] - ej[c], acc[1][c]);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + ty * 2 + r, k = k0 + tx * 4 + c;
      if (i < B && k < D) dE[(int64_t)i * D + k] = acc[r][c];
    }
}

}  // namespace

// Both kernels keep their LDS static and below 48 KiB (17 KiB and 42 KiB), so no launch needs hipFuncSetAttribute.
extern "C" int hfl_pairwise_dist(float* dist, const float* emb, int batch, int dim, hfl_stream_t stream) {
  if (batch <= 0 || dim <= 0 || dist == nullptr || emb == nullptr) return HFL_EINVAL;
  const int tiles = (int)hfl_cdiv(batch, PW_TILE);
  if (tiles > 65535) return HFL_ECAPACITY;
  const dim3 grid(tiles, tiles);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (dim % 4 == 0 && (reinterpret_cast<uintptr_t>(emb) & 15) == 0)
    pairwise_dist_kernel<true><<<grid, 256, 0, st>>>(dist, emb, batch, dim);
  else
    pairwise_dist_kernel<false><<<grid, 256, 0, st>>>(dist, emb, batch, dim);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int hfl_pairwise_dist_bwd(float* d_emb, const float* grad_dist, const float* dist, const float* emb, int batch,
                                     int dim, hfl_stream_t stream) {
  if (batch <= 0 || dim <= 0 || d_emb == nullptr || grad_dist == nullptr || dist == nullptr || emb == nullptr)
    return HFL_EINVAL;
  const int64_t row_tiles = hfl_cdiv(batch, PB_ROWS);
  if (row_tiles > 65535) return HFL_ECAPACITY;
  const dim3 grid((unsigned)hfl_cdiv(dim, PB_COLS), (unsigned)row_tiles);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (dim % 4 == 0 && (reinterpret_cast<uintptr_t>(emb) & 15) == 0)
    pairwise_dist_bwd_kernel<true><<<grid, 256, 0, st>>>(d_emb, grad_dist, dist, emb, batch, dim);
  else
    pairwise_dist_bwd_kernel<false><<<grid, 256, 0, st>>>(d_emb, grad_dist, dist, emb, batch, dim);
  HFL_RETURN_LAST_ERROR();
}
