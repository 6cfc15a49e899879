// Every FeatureMixerLayer of the Mixer aggregator (models/layers/salsa.py:58-111), then row_proj, as ONE kernel:
//
//     for l in 0 .. L-1:   x = x + fc2_l(gelu(fc1_l(LN_l(x))))          x (M, C = 256) f32, hidden = C, L <= 4
//     u[row, j] = sum_c x[row, c] Wr[j, c]                               j < D <= 8  (row_proj without its bias)
//
// The launches it replaces (L x hfl_ln_mlp_fused_h + its hidden-split reduce, and the first half of mixer_tail_kernel) carry
// the (M, C) token matrix through HBM L times and read it once more to shrink it to (M, D); at M = 8192 each of them is a
// fill / drain of the chip at the very end of the forward, where nothing overlaps it.
//
// A 512-lane workgroup owns R rows for all L layers; the rows live in LDS as f32 between layers (what crossed HBM before).
// The structure is the MLP half of relay_block_fused_kernel (csrc/relay_block.hip): wave w owns 32 of fc1's and of fc2's
// output features, so every weight fragment is used by exactly one wave of a workgroup and goes from L2 straight into MFMA
// operand registers (csrc/wfrag.h, no LDS ring), MC_PF steps ahead of its use.  The load ring runs through the WHOLE chain:
// the fragments of the next GEMM are on their way while the epilogue, the barriers and the LayerNorm in between run.  Nothing
// else is loaded from global memory inside the chain (a load issued there would be waited for behind every prefetched
// fragment): LayerNorm parameters and biases of all layers are staged in LDS at the start.
//
// Arithmetic at every hand-off is hfl_ln_mlp_fused_h's: two-pass f32 LayerNorm, LN output and GELU output as bf16 (hi, lo)
// round-to-nearest-even, w_hi x_lo + w_lo x_hi + w_hi x_hi in f32, x3_gelu, bias and residual in f32.  Only f32 summation
// orders differ (and the hidden dimension is not split over workgroups and reduced).
#include "hfl_common.h"
#include "x3_math.h"
#include "stage_stream.h"
#include "wfrag.h"

namespace {

constexpr int MC = 256;                     // channels = hidden width
constexpr int MC_W = 8;                     // waves per workgroup
constexpr int MC_KS = MC / 32;              // k-steps of a C-deep product
constexpr int MC_MAXL = 4;                  // layers
constexpr int MC_MAXD = 8;                  // row_proj outputs
constexpr int MC_PF = 4;                    // steps a weight fragment is loaded ahead of its MFMAs
constexpr int MC_ROWS = 32;                 // R of the shipped launch ("The Mixer layers as one launch": 16 and 64 lost)
constexpr size_t MC_LIN_B = (size_t)MC * MC * 4;        // pack of one Linear: bf16 (hi, lo)
constexpr size_t MC_LAYER_B = 2 * MC_LIN_B;             // fc1 | fc2
constexpr int MC_ROW_B = MC * 4 + 16;       // an LDS row: C f32, or [C bf16 hi | C bf16 lo]; the pad spreads the 16 rows of a
                                            // fragment read over all banks
constexpr int MC_PRM_B = MC_MAXL * 4 * MC * 4;          // [layer][gamma | beta | b1 | b2][C] f32

template <int R> constexpr int mc_lds_bytes() { return 2 * R * MC_ROW_B + MC_PRM_B; }

struct MixerChainParams {
  float* out_x;                 // (M, C) or null
  float* out_u;                 // (M, D) or null
  const float* x;               // (M, C)
  const unsigned char* pack;    // [layer][fc1 | fc2] wfrag packs
  const float* gamma[MC_MAXL];
  const float* beta[MC_MAXL];
  const float* b1[MC_MAXL];
  const float* b2[MC_MAXL];
  const float* row_w;           // (D, C) or null
  int64_t M;
  int layers, out_d;
  float eps;
};

template <int R>
__global__ void __launch_bounds__(MC_W * 64) __attribute__((amdgpu_waves_per_eu(2, 2)))
mixer_chain_kernel(const MixerChainParams p) {
  constexpr int T = R / 16;                 // 16-row tiles of the GEMMs
  constexpr int RPW = R / MC_W;             // LayerNorm / row_proj: rows per wave,
  constexpr int LPR = 64 / RPW;             // lanes per row,
  constexpr int NCH = 32 / LPR;             // 8-channel chunks per lane (chunk j * LPR + l of lane l)
  static_assert(R % 16 == 0 && RPW >= 1 && LPR >= 8 && NCH >= 1, "R in {16, 32, 64}");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* xs = smem;                                      // R rows of x, f32
  unsigned char* as = smem + R * MC_ROW_B;                       // R rows of LN(x), then of gelu(fc1), bf16 (hi, lo)
  const float* prm = reinterpret_cast<const float*>(smem + 2 * R * MC_ROW_B);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int L = p.layers;
  const int64_t row0 = (int64_t)blockIdx.x * R;

  // the weight stream of this wave: step s of a layer = (GEMM s / 8, k-step s % 8), fragment f = (n-tile wave * 2 + f / 2, hi | lo)
  const unsigned char* wb = p.pack + (size_t)wave * 2 * MC_KS * 2048 + (uint32_t)lane * 16u;
  auto frag = [&](int layer, int s, int f) {
    return wb + (size_t)layer * MC_LAYER_B + (size_t)(s >> 3) * MC_LIN_B + (size_t)((((f >> 1) * MC_KS + (s & 7)) * 2 + (f & 1)) * 1024);
  };
  bf16x8 ring[MC_PF][4];

  // ---- rows and per-layer vectors -> LDS; the first weight fragments go out behind their loads
  {
    float4 xv[RPW];
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const int row = i * MC_W + wave;
      xv[i] = make_float4(0.f, 0.f, 0.f, 0.f);                    // rows past M are zeros (finite through every layer, never written)
      if (row0 + row < p.M) xv[i] = *reinterpret_cast<const float4*>(p.x + (row0 + row) * MC + lane * 4);
    }
    float4 pv[MC_MAXL];
#pragma unroll
    for (int l = 0; l < MC_MAXL; ++l) {
      pv[l] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (l < L && wave < 4) {
        const float* src = wave == 0 ? p.gamma[l] : wave == 1 ? p.beta[l] : wave == 2 ? p.b1[l] : p.b2[l];
        pv[l] = *reinterpret_cast<const float4*>(src + lane * 4);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    hfl_static_for(std::make_integer_sequence<int, MC_PF>{}, [&](auto sc) {
      constexpr int s = decltype(sc)::value;
#pragma unroll
      for (int f = 0; f < 4; ++f) ring[s][f] = *reinterpret_cast<const bf16x8*>(frag(0, s, f));
    });
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < RPW; ++i)
      *reinterpret_cast<float4*>(xs + (i * MC_W + wave) * MC_ROW_B + lane * 16) = xv[i];
    if (wave < 4) {
#pragma unroll
      for (int l = 0; l < MC_MAXL; ++l)
        *reinterpret_cast<float4*>(smem + 2 * R * MC_ROW_B + ((l * 4 + wave) * MC + lane * 4) * 4) = pv[l];
    }
  }
  __syncthreads();

  // one GEMM of the chain: steps S0 .. S0 + 7 of `layer`; body(k-step, fragments); the step MC_PF ahead (of the next GEMM, of
  // the next layer) is requested as soon as its ring slot is free.  The scheduling barriers keep the loads where they are
  // written: left alone, hipcc sinks every load to just in front of its first use (one L2 round trip per step).
  auto gemm = [&](int layer, auto s0c, auto&& body) {
    constexpr int S0 = decltype(s0c)::value;
    hfl_static_for(std::make_integer_sequence<int, MC_KS>{}, [&](auto kc) {
      constexpr int ks = decltype(kc)::value;
      constexpr int s = S0 + ks;
      bf16x8 cur[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) cur[f] = ring[s % MC_PF][f];
      body(kc, cur);
      __builtin_amdgcn_sched_barrier(0);
      constexpr int sn = s + MC_PF;
      if (sn < 2 * MC_KS || layer + 1 < L) {
        const int ln = sn < 2 * MC_KS ? layer : layer + 1;
#pragma unroll
        for (int f = 0; f < 4; ++f) ring[s % MC_PF][f] = *reinterpret_cast<const bf16x8*>(frag(ln, sn % (2 * MC_KS), f));
      }
      __builtin_amdgcn_sched_barrier(0);
    });
  };
  static_assert((2 * MC_KS) % MC_PF == 0, "a ring slot belongs to the same steps in every layer");

  // LayerNorm / row_proj ownership: row `nrow` of the workgroup, chunks j * LPR + nl
  const int nrow = wave * RPW + lane / LPR, nl = lane % LPR;

#pragma unroll 1
  for (int layer = 0; layer < L; ++layer) {
    const float* lp = prm + layer * 4 * MC;                      // gamma | beta | b1 | b2
    // ---- LayerNorm (two-pass, f32) -> bf16 (hi, lo) operand rows
    {
      float4 a[NCH][2];
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        const unsigned char* src = xs + nrow * MC_ROW_B + (j * LPR + nl) * 32;
        a[j][0] = *reinterpret_cast<const float4*>(src);
        a[j][1] = *reinterpret_cast<const float4*>(src + 16);
        sum += ((a[j][0].x + a[j][0].y) + (a[j][0].z + a[j][0].w)) + ((a[j][1].x + a[j][1].y) + (a[j][1].z + a[j][1].w));
      }
      const float mean = hfl_group_sum<LPR>(sum) * (1.0f / (float)MC);
      float sq = 0.f, rs = 0.f;                 // rs: what the rounding of `sum` left in the residuals (csrc/ln_row.h)
#pragma unroll
      for (int j = 0; j < NCH; ++j)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          a[j][h].x -= mean; a[j][h].y -= mean; a[j][h].z -= mean; a[j][h].w -= mean;
          rs += (a[j][h].x + a[j][h].y) + (a[j][h].z + a[j][h].w);
          sq += (a[j][h].x * a[j][h].x + a[j][h].y * a[j][h].y) + (a[j][h].z * a[j][h].z + a[j][h].w * a[j][h].w);
        }
      const float dm = hfl_group_sum<LPR>(rs) * (1.0f / (float)MC);
      const float rstd = 1.0f / sqrtf(fmaxf(fmaf(-dm, dm, hfl_group_sum<LPR>(sq) * (1.0f / (float)MC)), 0.f) + p.eps);
      const float dr = dm * rstd;
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        const int ch = j * LPR + nl;
        uint32_t hi[4], lo[4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const float4 g = *reinterpret_cast<const float4*>(lp + ch * 8 + h * 4);
          const float4 b = *reinterpret_cast<const float4*>(lp + MC + ch * 8 + h * 4);
          const f32x2 v01 = {fmaf(fmaf(a[j][h].x, rstd, -dr), g.x, b.x), fmaf(fmaf(a[j][h].y, rstd, -dr), g.y, b.y)};
          const f32x2 v23 = {fmaf(fmaf(a[j][h].z, rstd, -dr), g.z, b.z), fmaf(fmaf(a[j][h].w, rstd, -dr), g.w, b.w)};
          x3_split_pair(v01, hi[2 * h], lo[2 * h]);
          x3_split_pair(v23, hi[2 * h + 1], lo[2 * h + 1]);
        }
        unsigned char* dst = as + nrow * MC_ROW_B + ch * 16;
        *reinterpret_cast<u32x4*>(dst) = (u32x4){hi[0], hi[1], hi[2], hi[3]};
        *reinterpret_cast<u32x4*>(dst + MC * 2) = (u32x4){lo[0], lo[1], lo[2], lo[3]};
      }
    }
    __syncthreads();

    f32x4 acc[T][2];
    auto mma = [&](auto kc, bf16x8 (&w)[4]) {
      constexpr int ks = decltype(kc)::value;
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const unsigned char* src = as + (t * 16 + fr) * MC_ROW_B + ks * 64 + fq * 16;
        const bf16x8 xh = *reinterpret_cast<const bf16x8*>(src);
        const bf16x8 xl = *reinterpret_cast<const bf16x8*>(src + MC * 2);
        acc[t][0] = wfrag_x3(w[0], w[1], xh, xl, acc[t][0]);
        acc[t][1] = wfrag_x3(w[2], w[3], xh, xl, acc[t][1]);
      }
    };

    // ---- fc1 + bias + GELU -> bf16 (hi, lo) rows, in place of the LN rows once every wave has read them
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float4 b = *reinterpret_cast<const float4*>(lp + 2 * MC + (wave * 2 + i) * 16 + fq * 4);
#pragma unroll
      for (int t = 0; t < T; ++t) acc[t][i] = (f32x4){b.x, b.y, b.z, b.w};
    }
    gemm(layer, std::integral_constant<int, 0>{}, mma);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        uint32_t h01, l01, h23, l23;
        x3_split_pair_scalar(x3_gelu(acc[t][i][0]), x3_gelu(acc[t][i][1]), h01, l01);
        x3_split_pair_scalar(x3_gelu(acc[t][i][2]), x3_gelu(acc[t][i][3]), h23, l23);
        unsigned char* dst = as + (t * 16 + fr) * MC_ROW_B + ((wave * 2 + i) * 16 + fq * 4) * 2;
        *reinterpret_cast<u32x2*>(dst) = (u32x2){h01, h23};
        *reinterpret_cast<u32x2*>(dst + MC * 2) = (u32x2){l01, l23};
      }
    __syncthreads();

    // ---- fc2 + bias + residual -> x (a lane reads and writes its own elements of the f32 rows)
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int i = 0; i < 2; ++i) acc[t][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    gemm(layer, std::integral_constant<int, MC_KS>{}, mma);
    const bool store = p.out_x != nullptr && layer == L - 1;
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int n = (wave * 2 + i) * 16 + fq * 4;
        const float4 b = *reinterpret_cast<const float4*>(lp + 3 * MC + n);
        float4* xp = reinterpret_cast<float4*>(xs + (t * 16 + fr) * MC_ROW_B + n * 4);
        const float4 x1 = *xp;
        float4 v;
        v.x = acc[t][i][0] + b.x + x1.x; v.y = acc[t][i][1] + b.y + x1.y;
        v.z = acc[t][i][2] + b.z + x1.z; v.w = acc[t][i][3] + b.w + x1.w;
        *xp = v;
        const int64_t row = row0 + t * 16 + fr;
        if (store && row < p.M) *reinterpret_cast<float4*>(p.out_x + row * MC + n) = v;
      }
    __syncthreads();
  }

  // ---- row_proj without its bias: u[row, j] = sum_c x[row, c] Wr[j, c], f32
  if (p.out_u != nullptr) {
    float4 a[NCH][2];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
      const unsigned char* src = xs + nrow * MC_ROW_B + (j * LPR + nl) * 32;
      a[j][0] = *reinterpret_cast<const float4*>(src);
      a[j][1] = *reinterpret_cast<const float4*>(src + 16);
    }
    const int D = p.out_d;
#pragma unroll
    for (int d = 0; d < MC_MAXD; ++d) {
      if (d < D) {
        float v = 0.f;
#pragma unroll
        for (int j = 0; j < NCH; ++j)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const float4 w = *reinterpret_cast<const float4*>(p.row_w + d * MC + (j * LPR + nl) * 8 + h * 4);
            v += (a[j][h].x * w.x + a[j][h].y * w.y) + (a[j][h].z * w.z + a[j][h].w * w.w);
          }
        v = hfl_group_sum<LPR>(v);
        if (nl == 0 && row0 + nrow < p.M) p.out_u[(row0 + nrow) * D + d] = v;
      }
    }
  }
}

template <int R>
int mixer_chain_launch(const MixerChainParams& p, hipStream_t s) {
  const int64_t groups = (p.M + R - 1) / R;
  if (groups > 0x7fffffff) return HFL_ECAPACITY;
  // (every launch: the attribute is per device, and the call is a table write)
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(mixer_chain_kernel<R>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, mc_lds_bytes<R>());
  if (e != hipSuccess) return (int)e;
  mixer_chain_kernel<R><<<(unsigned)groups, MC_W * 64, mc_lds_bytes<R>(), s>>>(p);
  HFL_RETURN_LAST_ERROR();
}

}  // namespace

extern "C" {

int hfl_mixer_chain_ok(int channels, int hidden, int layers, int out_d) {
  return channels == MC && hidden == MC && layers >= 1 && layers <= MC_MAXL && out_d >= 0 && out_d <= MC_MAXD ? 1 : 0;
}

int64_t hfl_mixer_chain_pack_bytes(int layers) {
  return layers >= 1 && layers <= MC_MAXL ? (int64_t)layers * (int64_t)MC_LAYER_B : 0;
}

int hfl_mixer_chain_pack(void* dst, const float* const* w1, const float* const* w2, int layers, hfl_stream_t stream) {
  if (dst == nullptr || w1 == nullptr || w2 == nullptr || layers < 1 || layers > MC_MAXL) return HFL_EINVAL;
  for (int l = 0; l < layers; ++l)
    if (w1[l] == nullptr || w2[l] == nullptr) return HFL_EINVAL;
  unsigned char* d = static_cast<unsigned char*>(dst);
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (int l = 0; l < layers; ++l) {
    wfrag_pack_kernel<<<128, 256, 0, s>>>(d + l * MC_LAYER_B, w1[l], MC, MC);
    wfrag_pack_kernel<<<128, 256, 0, s>>>(d + l * MC_LAYER_B + MC_LIN_B, w2[l], MC, MC);
  }
  HFL_RETURN_LAST_ERROR();
}

int hfl_mixer_chain_x3(float* out_x, float* out_u, const float* x, const void* packs, const float* const* gamma,
                       const float* const* beta, const float* const* b1, const float* const* b2, float eps, const float* row_w,
                       int64_t M, int layers, int out_d, hfl_stream_t stream) {
  if (hfl_mixer_chain_ok(MC, MC, layers, out_d) == 0 || M < 0) return HFL_EINVAL;
  if (x == nullptr || packs == nullptr || gamma == nullptr || beta == nullptr || b1 == nullptr || b2 == nullptr) return HFL_EINVAL;
  if (out_d > 0 ? (row_w == nullptr || out_u == nullptr) : (out_u != nullptr || out_x == nullptr)) return HFL_EINVAL;
  MixerChainParams p = {};
  for (int l = 0; l < layers; ++l) {
    if (gamma[l] == nullptr || beta[l] == nullptr || b1[l] == nullptr || b2[l] == nullptr) return HFL_EINVAL;
    p.gamma[l] = gamma[l]; p.beta[l] = beta[l]; p.b1[l] = b1[l]; p.b2[l] = b2[l];
  }
  if (M == 0) return HFL_OK;
  p.out_x = out_x; p.out_u = out_u; p.x = x;
  p.pack = static_cast<const unsigned char*>(packs);
  p.row_w = row_w;
  p.M = M; p.layers = layers; p.out_d = out_d; p.eps = eps;
  return mixer_chain_launch<MC_ROWS>(p, static_cast<hipStream_t>(stream));
}

}  // extern "C"
