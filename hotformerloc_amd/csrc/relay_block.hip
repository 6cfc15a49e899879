// The relay-token transformer block (RTSA, models/hotformerloc_backbone.py:239-302) of the inference path as ONE kernel:
//
//     x1  = x + proj(attn(LN1(x)))          attn: 16-head self-attention over one cloud's relay tokens
//     out = x1 + fc2(gelu(fc1(LN2(x1))))
//
// for the ~1.7 k relay rows of a batch (C = 256, <= 64 per cloud).  hfl_relay_block_forward_x3 runs this as five launches
// (hfl_ln_qkv_fused_seg, hfl_relay_attention_f16_fwd, hfl_linear_x3_seg, hfl_ln_mlp_fused_ws, mlp_tail_reduce_kernel), each a
// fill / drain of a mostly empty chip on the chain every H-OSA iteration waits for.
//
// Work item = (cloud, 16-row query tile), one 512-lane workgroup each, and NO communication between workgroups: an item
// normalises all rows of its cloud, computes K and V of all of them and Q of its own 16 (K / V are recomputed by the other
// items of the cloud: the price of needing no exchange), runs the attention of its 16 queries, then proj, LN2, fc1, GELU, fc2
// for its 16 rows.  Rows of no sequence (`orphan_rows`: relay tokens of pure padding windows) form items of 16 rows without
// the attention (its output is zero there: x1 = x + proj bias).
//
// Every weight fragment is used by exactly one wave of a workgroup (wave w owns heads 2 w, 2 w + 1 of qkv, 32 of proj's and
// fc2's output features, 128 of fc1's), so the weights go from L2 straight into MFMA operand registers, a few steps ahead of
// their use (no LDS ring): the pack (hfl_relay_block_pack) stores each 16-feature x 32-k fragment as the 1 KiB a wave reads
// with one 16-B load per lane.  Orientation: weights are the A operand, activation rows the B operand, so a lane's
// accumulator holds features 4 fq .. 4 fq + 3 of row fr -- for Q and K that IS the operand layout of the relay attention's
// fp32 MFMAs (dims 4 g .. 4 g + 3 of row c); V is computed with the operands swapped (rows 4 fq + r, feature fr), which is
// what P V wants.  q / k / v therefore never leave registers.
//
// Arithmetic at every hand-off is the five-launch path's: two-pass f32 LayerNorm (csrc/qkv_fused.hip's lane layout and
// summation order), bf16 (hi, lo) operands with w_hi x_lo + w_lo x_hi + w_hi x_hi in f32, q * 0.25 log2 e, q / k / v as fp16
// (hi, lo) = (RTZ(v), RTZ(v - hi)), the attention of relay_attn_f16_kernel statement by statement, attention output and GELU
// output split to bf16 (hi, lo) round-to-nearest-even, x3_gelu.  Only f32 summation orders inside the GEMMs differ.
#include "hfl_common.h"
#include "x3_math.h"
#include "stage_stream.h"
#include "wfrag.h"

namespace {

constexpr int RC = 256;                     // channels
constexpr int RH = 16;                      // heads
constexpr int RHID = 1024;                  // hidden width of the MLP
constexpr int RW = 8;                       // waves per workgroup
constexpr int RKS = RC / 32;                // k-steps of a C-deep product
constexpr int RMAXSEQ = 64;                 // relay tokens per cloud
constexpr float kRelayDead = -1e30f;        // (csrc/attention.hip: kDeadValue)

// pack: per Linear the fragment image of csrc/wfrag.h
constexpr size_t PACK_QKV = 0;
constexpr size_t PACK_PROJ = PACK_QKV + (size_t)3 * RC * RC * 4;
constexpr size_t PACK_FC1 = PACK_PROJ + (size_t)RC * RC * 4;
constexpr size_t PACK_FC2 = PACK_FC1 + (size_t)RHID * RC * 4;
constexpr size_t PACK_BYTES = PACK_FC2 + (size_t)RC * RHID * 4;

// LDS: bf16 (hi, lo) operand rows [C hi | C lo] + 16 B (the pad spreads the 16 rows of a fragment read over all banks)
constexpr int XROW_B = RC * 4 + 16;         // LN1 output, attention output: 1040 B per row
constexpr int GROW_B = RHID * 4 + 16;       // GELU output: 4112 B per row
constexpr int X1ROW_B = RC * 4 + 16;        // x1 f32
constexpr int LDS_XA = 0;                                   // 64 rows of LN1(x); later the 16 rows of gelu(fc1)
constexpr int LDS_XA_B = RMAXSEQ * XROW_B;
static_assert(16 * GROW_B <= LDS_XA_B, "the GELU rows reuse the LN1 rows");
constexpr int LDS_O = LDS_XA + LDS_XA_B;                    // 16 rows of attention output
constexpr int LDS_X1 = LDS_O + 16 * XROW_B;                 // 16 rows of x1
constexpr int LDS_SROW = LDS_X1 + 16 * X1ROW_B;              // the cloud's row table (everything in the dynamic region: its
constexpr int LDS_BYTES = LDS_SROW + RMAXSEQ * 4;           // base stays 16-B aligned)

struct RelayFusedParams {
  float* out;                   // (n_rows, C)
  HflRowSeg x;                  // (n_rows, C) input rows
  const int32_t* seq_rows;
  const int32_t* seq_off;       // (batch + 1)
  const int32_t* orphan_rows;
  const float *g1, *b1, *g2, *b2;
  const float *qkv_b, *proj_b, *fc1_b, *fc2_b;
  const unsigned char* pack;
  int64_t n_rows;
  int n_orphans, batch, qtiles; // qtiles = ceil(max_seq_len / 16): items per cloud in the grid
  float eps, q_scale;
};

// Two-pass LayerNorm of row fr of a 16-row tile, lane (fr, fq) holding channels 32 ks + 8 fq .. + 7: the statements of
// ln_qkv_fused_kernel / ln_mlp_fused_kernel (same summation order), result as bf16 (hi, lo) B fragments.
__device__ __forceinline__ void relay_ln_split(const float* xr, const float* gm, const float* bt, float eps, int fq,
                                               bf16x8 (&xh)[RKS], bf16x8 (&xl)[RKS]) {
  float4 a[RKS][2];
  float sum = 0.f;
#pragma unroll
  for (int ks = 0; ks < RKS; ++ks) {
    a[ks][0] = *reinterpret_cast<const float4*>(xr + ks * 32 + fq * 8);
    a[ks][1] = *reinterpret_cast<const float4*>(xr + ks * 32 + fq * 8 + 4);
    sum += ((a[ks][0].x + a[ks][0].y) + (a[ks][0].z + a[ks][0].w)) + ((a[ks][1].x + a[ks][1].y) + (a[ks][1].z + a[ks][1].w));
  }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  const float mean = sum * (1.0f / (float)RC);
  float sq = 0.f, rs = 0.f;                 // rs: what the rounding of `sum` left in the residuals (csrc/ln_row.h)
#pragma unroll
  for (int ks = 0; ks < RKS; ++ks)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      a[ks][h].x -= mean; a[ks][h].y -= mean; a[ks][h].z -= mean; a[ks][h].w -= mean;
      rs += (a[ks][h].x + a[ks][h].y) + (a[ks][h].z + a[ks][h].w);
      sq += (a[ks][h].x * a[ks][h].x + a[ks][h].y * a[ks][h].y) + (a[ks][h].z * a[ks][h].z + a[ks][h].w * a[ks][h].w);
    }
  rs += __shfl_xor(rs, 16, 64);
  rs += __shfl_xor(rs, 32, 64);
  sq += __shfl_xor(sq, 16, 64);
  sq += __shfl_xor(sq, 32, 64);
  const float dm = rs * (1.0f / (float)RC);
  const float rstd = 1.0f / sqrtf(fmaxf(fmaf(-dm, dm, sq * (1.0f / (float)RC)), 0.f) + eps);
  const float dr = dm * rstd;
#pragma unroll
  for (int ks = 0; ks < RKS; ++ks) {
    uint32_t hi[4], lo[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float4 g = *reinterpret_cast<const float4*>(gm + ks * 32 + fq * 8 + h * 4);
      const float4 b = *reinterpret_cast<const float4*>(bt + ks * 32 + fq * 8 + h * 4);
      const f32x2 v01 = {fmaf(fmaf(a[ks][h].x, rstd, -dr), g.x, b.x), fmaf(fmaf(a[ks][h].y, rstd, -dr), g.y, b.y)};
      const f32x2 v23 = {fmaf(fmaf(a[ks][h].z, rstd, -dr), g.z, b.z), fmaf(fmaf(a[ks][h].w, rstd, -dr), g.w, b.w)};
      x3_split_pair(v01, hi[2 * h], lo[2 * h]);
      x3_split_pair(v23, hi[2 * h + 1], lo[2 * h + 1]);
    }
    xh[ks] = __builtin_bit_cast(bf16x8, (u32x4){hi[0], hi[1], hi[2], hi[3]});
    xl[ks] = __builtin_bit_cast(bf16x8, (u32x4){lo[0], lo[1], lo[2], lo[3]});
  }
}

// NSTEP steps of NF weight fragments each, loaded PF steps ahead of their use: frag(s, f) = address of the lane's 16 B of
// fragment f of step s; body(step constant, fragments of the step).  The scheduling barriers keep the loads where they are
// written: left alone, hipcc sinks every load to just in front of its first use (one L2 round trip per step).
template <int NSTEP, int NF, int PF, class Frag, class Body>
__device__ __forceinline__ void relay_stream(Frag&& frag, Body&& body) {
  bf16x8 ring[PF][NF];
  hfl_static_for(std::make_integer_sequence<int, (PF < NSTEP ? PF : NSTEP)>{}, [&](auto sc) {
    constexpr int s = decltype(sc)::value;
#pragma unroll
    for (int f = 0; f < NF; ++f) ring[s][f] = *reinterpret_cast<const bf16x8*>(frag(s, f));
  });
  __builtin_amdgcn_sched_barrier(0);
  hfl_static_for(std::make_integer_sequence<int, NSTEP>{}, [&](auto sc) {
    constexpr int s = decltype(sc)::value;
    bf16x8 cur[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) cur[f] = ring[s % PF][f];
    body(sc, cur);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (s + PF < NSTEP) {
#pragma unroll
      for (int f = 0; f < NF; ++f) ring[s % PF][f] = *reinterpret_cast<const bf16x8*>(frag(s + PF, f));
      __builtin_amdgcn_sched_barrier(0);
    }
  });
}

// the same product with the activation rows as the A operand: the accumulator holds rows 4 fq + r, feature fr
__device__ __forceinline__ f32x4 relay_x3_t(bf16x8 whi, bf16x8 wlo, bf16x8 xh, bf16x8 xl, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xl, whi, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, wlo, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, whi, acc, 0, 0, 0);
}

// the value the attention reads back from the fp16 (hi, lo) pair hfl_ln_qkv_fused writes: hi = RTZ(v), lo = RTZ(v - hi)
__device__ __forceinline__ float relay_f16_pair(float v) {
  const auto h = __builtin_amdgcn_cvt_pkrtz(v, v);
  const auto l = __builtin_amdgcn_cvt_pkrtz(v - (float)h[0], v - (float)h[0]);
  return (float)h[0] + (float)l[0];
}

__global__ void __launch_bounds__(RW * 64) __attribute__((amdgpu_waves_per_eu(2, 2)))
relay_block_fused_kernel(const RelayFusedParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int* srow = reinterpret_cast<int*>(smem + LDS_SROW);
  unsigned char* xa = smem + LDS_XA;
  unsigned char* gl = smem + LDS_XA;         // (after the attention)
  unsigned char* ol = smem + LDS_O;
  unsigned char* x1l = smem + LDS_X1;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const uint32_t lane_off = (uint32_t)lane * 16u;

  // ---- the item: (cloud, query tile) or 16 orphan rows
  const int bx = blockIdx.x;
  const bool orphan = bx >= p.batch * p.qtiles;
  int R = 0, qt = 0, r0 = 0;
  if (!orphan) {
    const int cloud = bx / p.qtiles;
    qt = bx % p.qtiles;
    r0 = p.seq_off[cloud];
    R = p.seq_off[cloud + 1] - r0;
    if (R > RMAXSEQ) R = RMAXSEQ;            // (the launcher refuses max_seq_len > 64)
    if (qt * 16 >= R) return;
  } else {
    r0 = (bx - p.batch * p.qtiles) * 16;
    R = p.n_orphans - r0 < 16 ? p.n_orphans - r0 : 16;
    if (R <= 0) return;
  }
  const int ntile = (R + 15) / 16;
  if (tid < RMAXSEQ) {
    int r = -1;
    if (tid < R) r = orphan ? p.orphan_rows[r0 + tid] : p.seq_rows[r0 + tid];
    // The tables are trusted, as hfl_relay_attention_f16_fwd trusts them: this check only keeps an index outside the matrix
    // from becoming an access outside it (such a row is read as zeros, still counts as a key, and is never written).
    if (r < 0 || (int64_t)r >= p.n_rows) r = -1;
    srow[tid] = r;
  }
  __syncthreads();
  const int my_row = srow[qt * 16 + fr];                        // the item's own row of this lane (-1: none)
  const float* my_x = hfl_seg_row(p.x, my_row < 0 ? 0 : my_row, RC);

  if (!orphan) {
    // ---- LN1 of every row of the cloud into LDS (wave t: rows 16 t .. 16 t + 15); rows past the sequence are zeros
    if (wave < ntile) {
      const int r = srow[wave * 16 + fr];
      bf16x8 xh[RKS], xl[RKS];
      relay_ln_split(hfl_seg_row(p.x, r < 0 ? 0 : r, RC), p.g1, p.b1, p.eps, fq, xh, xl);
      unsigned char* dst = xa + (wave * 16 + fr) * XROW_B + fq * 16;
      const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int ks = 0; ks < RKS; ++ks) {
        *reinterpret_cast<bf16x8*>(dst + ks * 64) = r < 0 ? z : xh[ks];
        *reinterpret_cast<bf16x8*>(dst + RC * 2 + ks * 64) = r < 0 ? z : xl[ks];
      }
    }
    __syncthreads();

    // ---- per head of this wave (2 w, 2 w + 1, one weight stream of 2 x 8 steps): Q (own tile), K, V (all tiles) of the head,
    // then its attention while the next head's first fragments are on their way
    float4 bq2[2], bk2[2];
    float bv2[2];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {                           // (ahead of the stream: a load issued inside it would be waited
      const int h = wave * 2 + hh;                             //  for behind every prefetched fragment)
      bq2[hh] = *reinterpret_cast<const float4*>(p.qkv_b + h * 16 + fq * 4);
      bk2[hh] = *reinterpret_cast<const float4*>(p.qkv_b + RC + h * 16 + fq * 4);
      bv2[hh] = p.qkv_b[2 * RC + h * 16 + fr];
    }
    f32x4 qa, ka[4], va[4];
    auto reset = [&]() {
      qa = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 4; ++t) { ka[t] = (f32x4){0.f, 0.f, 0.f, 0.f}; va[t] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    };
    auto attend = [&](auto hc) {
      constexpr int hh = decltype(hc)::value;
      const int h = wave * 2 + hh;
      // bias, query scale, fp16 (hi, lo) rounding: what the attention would read from hfl_ln_qkv_fused's rows
      const float4 bq = bq2[hh], bk = bk2[hh];
      const float bv = bv2[hh];
      float4 qf;
      qf.x = relay_f16_pair((qa[0] + bq.x) * p.q_scale);
      qf.y = relay_f16_pair((qa[1] + bq.y) * p.q_scale);
      qf.z = relay_f16_pair((qa[2] + bq.z) * p.q_scale);
      qf.w = relay_f16_pair((qa[3] + bq.w) * p.q_scale);
      float4 kf[4];
      float vv[4][4];
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        kf[kt].x = relay_f16_pair(ka[kt][0] + bk.x);
        kf[kt].y = relay_f16_pair(ka[kt][1] + bk.y);
        kf[kt].z = relay_f16_pair(ka[kt][2] + bk.z);
        kf[kt].w = relay_f16_pair(ka[kt][3] + bk.w);
#pragma unroll
        for (int r = 0; r < 4; ++r) vv[kt][r] = relay_f16_pair(va[kt][r] + bv);
      }
      // the attention of relay_attn_f16_kernel's short-sequence path (c = fr: query / key / dim index, g = fq)
      f32x4 sc4[4];
      float m = kRelayDead;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[kt].x, qf.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[kt].y, qf.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[kt].z, qf.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[kt].w, qf.w, acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          sc4[kt][r] = kt * 16 + 4 * fq + r < R ? acc[r] : kRelayDead;
          m = fmaxf(m, sc4[kt][r]);
        }
      }
      m = fmaxf(m, __shfl_xor(m, 16, 64));
      m = fmaxf(m, __shfl_xor(m, 32, 64));
      float l = 0.f;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          sc4[kt][r] = __builtin_amdgcn_exp2f(sc4[kt][r] - m);
          l += sc4[kt][r];
        }
      l += __shfl_xor(l, 16, 64);
      l += __shfl_xor(l, 32, 64);
      const float inv = 1.0f / l;
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) o = __builtin_amdgcn_mfma_f32_16x16x4f32(sc4[kt][r] * inv, vv[kt][r], o, 0, 0, 0);
      // o[r]: query 4 fq + r of the tile, dim fr of head h -> proj's bf16 (hi, lo) operand row
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t hb = x3_bf16_rne(o[r]);
        const uint32_t lb = x3_bf16_rne(o[r] - __uint_as_float(hb << 16));
        unsigned char* op = ol + (4 * fq + r) * XROW_B + (h * 16 + fr) * 2;
        *reinterpret_cast<unsigned short*>(op) = (unsigned short)hb;
        *reinterpret_cast<unsigned short*>(op + RC * 2) = (unsigned short)lb;
      }
    };
    reset();
    {
      const unsigned char* wq = p.pack + PACK_QKV + lane_off;
      auto frag = [&](int s, int f) {              // step = (head s / 8, k-step s % 8); f: (q, k, v) x (hi, lo); n-tile = region * 16 + head
        return wq + ((size_t)(((f >> 1) * RH + wave * 2 + s / RKS) * RKS + s % RKS) * 2 + (f & 1)) * 1024;
      };
      relay_stream<2 * RKS, 6, 4>(frag, [&](auto sc, bf16x8 (&w)[6]) {
        constexpr int ks = decltype(sc)::value % RKS;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (t < ntile) {
            const unsigned char* src = xa + (t * 16 + fr) * XROW_B + ks * 64 + fq * 16;
            const bf16x8 xh = *reinterpret_cast<const bf16x8*>(src);
            const bf16x8 xl = *reinterpret_cast<const bf16x8*>(src + RC * 2);
            if (t == qt) qa = wfrag_x3(w[0], w[1], xh, xl, qa);
            ka[t] = wfrag_x3(w[2], w[3], xh, xl, ka[t]);
            va[t] = relay_x3_t(w[4], w[5], xh, xl, va[t]);
          }
        }
        if constexpr (ks == RKS - 1) {
          attend(std::integral_constant<int, decltype(sc)::value / RKS>{});
          reset();
        }
      });
    }
    __syncthreads();
  }

  // ---- proj + bias + residual -> x1 (f32, LDS): wave w owns features 32 w .. 32 w + 31
  {
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    if (!orphan) {
      const unsigned char* wp = p.pack + PACK_PROJ + lane_off;
      auto frag = [&](int s, int f) { return wp + ((size_t)((wave * 2 + (f >> 1)) * RKS + s) * 2 + (f & 1)) * 1024; };
      relay_stream<RKS, 4, 8>(frag, [&](auto sc, bf16x8 (&w)[4]) {
        constexpr int ks = decltype(sc)::value;
        const unsigned char* src = ol + fr * XROW_B + ks * 64 + fq * 16;
        const bf16x8 oh = *reinterpret_cast<const bf16x8*>(src);
        const bf16x8 olo = *reinterpret_cast<const bf16x8*>(src + RC * 2);
        acc[0] = wfrag_x3(w[0], w[1], oh, olo, acc[0]);
        acc[1] = wfrag_x3(w[2], w[3], oh, olo, acc[1]);
      });
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int n = (wave * 2 + i) * 16 + fq * 4;
      const float4 b = *reinterpret_cast<const float4*>(p.proj_b + n);
      float4 res = make_float4(0.f, 0.f, 0.f, 0.f);
      if (my_row >= 0) res = *reinterpret_cast<const float4*>(my_x + n);
      float4 v;
      v.x = (acc[i][0] + b.x) + res.x; v.y = (acc[i][1] + b.y) + res.y;
      v.z = (acc[i][2] + b.z) + res.z; v.w = (acc[i][3] + b.w) + res.w;
      *reinterpret_cast<float4*>(x1l + fr * X1ROW_B + n * 4) = v;
    }
  }
  __syncthreads();

  // ---- LN2 (every wave, for itself: the 16 rows as B fragments in registers), fc1 + bias + GELU -> bf16 (hi, lo) rows in LDS:
  // wave w owns hidden features 128 w .. 128 w + 127
  {
    bf16x8 xh[RKS], xl[RKS];
    relay_ln_split(reinterpret_cast<const float*>(x1l + fr * X1ROW_B), p.g2, p.b2, p.eps, fq, xh, xl);
    f32x4 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float4 b = *reinterpret_cast<const float4*>(p.fc1_b + (wave * 8 + i) * 16 + fq * 4);
      acc[i] = (f32x4){b.x, b.y, b.z, b.w};
    }
    const unsigned char* w1 = p.pack + PACK_FC1 + lane_off;
    // step s = (pair of n-tiles s / 8, k-step s % 8)
    auto frag = [&](int s, int f) {
      return w1 + ((size_t)((wave * 8 + (s / RKS) * 2 + (f >> 1)) * RKS + (s % RKS)) * 2 + (f & 1)) * 1024;
    };
    relay_stream<4 * RKS, 4, 6>(frag, [&](auto sc, bf16x8 (&w)[4]) {
      constexpr int s = decltype(sc)::value;
      constexpr int j = s / RKS, ks = s % RKS;
      acc[2 * j] = wfrag_x3(w[0], w[1], xh[ks], xl[ks], acc[2 * j]);
      acc[2 * j + 1] = wfrag_x3(w[2], w[3], xh[ks], xl[ks], acc[2 * j + 1]);
    });
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      uint32_t h01, l01, h23, l23;
      x3_split_pair_scalar(x3_gelu(acc[i][0]), x3_gelu(acc[i][1]), h01, l01);
      x3_split_pair_scalar(x3_gelu(acc[i][2]), x3_gelu(acc[i][3]), h23, l23);
      unsigned char* dst = gl + fr * GROW_B + ((wave * 8 + i) * 16 + fq * 4) * 2;
      *reinterpret_cast<u32x2*>(dst) = (u32x2){h01, h23};
      *reinterpret_cast<u32x2*>(dst + RHID * 2) = (u32x2){l01, l23};
    }
  }
  __syncthreads();

  // ---- fc2 + bias + residual -> out: wave w owns features 32 w .. 32 w + 31
  {
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    constexpr int KS2 = RHID / 32;
    const unsigned char* w2 = p.pack + PACK_FC2 + lane_off;
    auto frag = [&](int s, int f) { return w2 + ((size_t)((wave * 2 + (f >> 1)) * KS2 + s) * 2 + (f & 1)) * 1024; };
    relay_stream<KS2, 4, 8>(frag, [&](auto sc, bf16x8 (&w)[4]) {
      constexpr int ks = decltype(sc)::value;
      const unsigned char* src = gl + fr * GROW_B + ks * 64 + fq * 16;
      const bf16x8 gh = *reinterpret_cast<const bf16x8*>(src);
      const bf16x8 glo = *reinterpret_cast<const bf16x8*>(src + RHID * 2);
      acc[0] = wfrag_x3(w[0], w[1], gh, glo, acc[0]);
      acc[1] = wfrag_x3(w[2], w[3], gh, glo, acc[1]);
    });
    if (my_row >= 0) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int n = (wave * 2 + i) * 16 + fq * 4;
        const float4 b = *reinterpret_cast<const float4*>(p.fc2_b + n);
        const float4 x1 = *reinterpret_cast<const float4*>(x1l + fr * X1ROW_B + n * 4);
        float4 v;
        v.x = acc[i][0] + b.x + x1.x; v.y = acc[i][1] + b.y + x1.y; v.z = acc[i][2] + b.z + x1.z; v.w = acc[i][3] + b.w + x1.w;
        *reinterpret_cast<float4*>(p.out + (int64_t)my_row * RC + n) = v;
      }
    }
  }
}

bool relay_ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return na > 0 && nb > 0 && a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace

extern "C" {

int64_t hfl_relay_block_pack_bytes(int channels) { return channels == RC ? (int64_t)PACK_BYTES : 0; }

int hfl_relay_block_pack(void* pack, const float* qkv_w, const float* proj_w, const float* fc1_w, const float* fc2_w, int channels,
                         hfl_stream_t stream) {
  if (pack == nullptr || qkv_w == nullptr || proj_w == nullptr || fc1_w == nullptr || fc2_w == nullptr || channels != RC)
    return HFL_EINVAL;
  unsigned char* d = static_cast<unsigned char*>(pack);
  hipStream_t s = static_cast<hipStream_t>(stream);
  wfrag_pack_kernel<<<384, 256, 0, s>>>(d + PACK_QKV, qkv_w, 3 * RC, RC);
  wfrag_pack_kernel<<<128, 256, 0, s>>>(d + PACK_PROJ, proj_w, RC, RC);
  wfrag_pack_kernel<<<512, 256, 0, s>>>(d + PACK_FC1, fc1_w, RHID, RC);
  wfrag_pack_kernel<<<512, 256, 0, s>>>(d + PACK_FC2, fc2_w, RC, RHID);
  HFL_RETURN_LAST_ERROR();
}

/* 1 when hfl_relay_block_fused_x3 takes this problem: C = 256 with 16 heads, the relay-block pack present, biases and
 * LayerNorm parameters present, at most 64 relay tokens per cloud */
int hfl_relay_block_fused_ok(const hfl_relay_block_weights* w, const hfl_relay_block_io* io) {
  if (w == nullptr || io == nullptr) return 0;
  if (w->channels != RC || w->n_heads != RH || w->relay_pack == nullptr) return 0;
  if (w->norm1_gamma == nullptr || w->norm1_beta == nullptr || w->norm2_gamma == nullptr || w->norm2_beta == nullptr ||
      w->qkv_b == nullptr || w->proj_b == nullptr || w->fc1_b == nullptr || w->fc2_b == nullptr)
    return 0;
  if (io->max_seq_len < 0 || io->max_seq_len > RMAXSEQ || io->batch <= 0 || io->n_rows < 0 || io->n_orphans < 0) return 0;
  if (io->seq_rows == nullptr || io->seq_off == nullptr || io->out == nullptr) return 0;
  if (io->n_orphans > 0 && io->orphan_rows == nullptr) return 0;
  if (io->x_segments == nullptr && io->x_in == nullptr) return 0;
  return 1;
}

int hfl_relay_block_fused_x3(const hfl_relay_block_weights* w, const hfl_relay_block_io* io, hfl_stream_t stream) {
  if (hfl_relay_block_fused_ok(w, io) == 0) return HFL_EINVAL;
  if (io->n_rows == 0) return HFL_OK;
  RelayFusedParams p;
  if (io->x_segments != nullptr) {
    if (!hfl_seg_from(io->x_segments, io->n_rows, &p.x)) return HFL_EINVAL;
  } else {
    p.x = hfl_seg_single(io->x_in);
  }
  // the kernel reads the other rows of a cloud after some of its rows were written: out must not overlap any input rows
  const size_t row_b = (size_t)RC * 4;
  for (int i = 0; i < p.x.n; ++i) {
    const int64_t end = i + 1 < p.x.n ? (int64_t)p.x.row[i + 1] : io->n_rows;
    const int64_t rows = end - (int64_t)p.x.row[i];
    if (rows < 0) return HFL_EINVAL;
    if (relay_ranges_overlap(io->out, (size_t)io->n_rows * row_b, p.x.ptr[i], (size_t)rows * row_b)) return HFL_EINVAL;
  }
  p.out = io->out;
  p.seq_rows = io->seq_rows; p.seq_off = io->seq_off; p.orphan_rows = io->orphan_rows;
  p.g1 = w->norm1_gamma; p.b1 = w->norm1_beta; p.g2 = w->norm2_gamma; p.b2 = w->norm2_beta;
  p.qkv_b = w->qkv_b; p.proj_b = w->proj_b; p.fc1_b = w->fc1_b; p.fc2_b = w->fc2_b;
  p.pack = static_cast<const unsigned char*>(w->relay_pack);
  p.n_rows = io->n_rows;
  p.n_orphans = io->n_orphans; p.batch = io->batch; p.qtiles = (io->max_seq_len + 15) / 16;
  p.eps = w->eps; p.q_scale = 0.25f * 1.4426950408889634f;
  const int items = p.batch * p.qtiles + (p.n_orphans + 15) / 16;
  if (items <= 0) return HFL_OK;
  // (every launch: the attribute is per device, and the call is a table write)
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(relay_block_fused_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
  if (e != hipSuccess) return (int)e;
  relay_block_fused_kernel<<<(unsigned)items, RW * 64, LDS_BYTES, static_cast<hipStream_t>(stream)>>>(p);
  HFL_RETURN_LAST_ERROR();
}

}  // extern "C"
