// Ranking core of the TruncatedSmoothAP listwise loss, forward and gradient in one pass over each
// query row (reference: models/losses/truncated_smoothap.py:44-93 with the clamped temperature sigmoid
// of models/losses/loss_utils.py:40-48).  The reference materialises five (B, P, B) float tensors
// (s_diff, s_sigmoid, two masked copies, the scatter mask: 5 x 67 MB at B = 2048, P = 4) and autograd
// keeps them for the backward.  Here one workgroup owns one query q: its similarity row and both mask
// rows sit in LDS, and for each of its P selected positives p_j
//     a_j(z) = sigmoid((s_qz - s_qp_j) / tau),   r_p = 1 + sum_{z in Pos, z != p_j} a_j(z),
//     r_w = r_p + sum_{z in Neg} a_j(z),         r_j = r_p / r_w
// are two block reductions; AP_q = sum_j valid_j r_j / n_valid_q.  d AP_q / d s_q. follows in the same
// kernel from  dr/dr_p = N/r_w^2,  dr/dN = -r_p/r_w^2,  da/ds_qz = a(1-a)/tau  (0 where the exponent is
// clamped, as torch.clamp's gradient), -sum_z of it for s_qp_j.  Everything else (E E^T, top-k of the
// positives, the mean over valid queries, dE = (dS + dS^T) E) is dense torch/hipBLASLt work.
#include "hfl_common.h"

namespace {

__device__ __forceinline__ float block_sum(float v, float* s_red) {
  v = hfl_group_sum<64>(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += s_red[i];
  return t;
}

__global__ void __launch_bounds__(256)
smoothap_rows_kernel(float* __restrict__ ap, float* __restrict__ dap_ds, const float* __restrict__ S,
                     const uint8_t* __restrict__ pos, const uint8_t* __restrict__ neg,
                     const int64_t* __restrict__ idx, int B, int P, float tau) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* s_row = reinterpret_cast<float*>(smem);          // [B] similarities of query q
  float* s_g = s_row + B;                                  // [B] d AP_q / d s_qz
  uint8_t* s_m = reinterpret_cast<uint8_t*>(s_g + B);     // [B] bit 0 positive, bit 1 negative
  __shared__ float s_red[4];
  const int q = blockIdx.x;
  for (int z = threadIdx.x; z < B; z += blockDim.x) {
    s_row[z] = S[(int64_t)q * B + z];
    s_g[z] = 0.f;
    s_m[z] = (uint8_t)((pos[(int64_t)q * B + z] ? 1 : 0) | (neg[(int64_t)q * B + z] ? 2 : 0));
  }
  __syncthreads();
  // a slot counts iff its index lies in [0, B) and points at a positive; compared as int64, so that 2^32 + z is not z
  auto slot = [&](int j) -> int {
    const int64_t p = idx[(int64_t)q * P + j];
    return (p >= 0 && p < (int64_t)B && (s_m[p] & 1)) ? (int)p : -1;
  };
  int n_valid = 0;
  for (int j = 0; j < P; ++j) n_valid += slot(j) >= 0;
  float ap_q = 0.f;
  const float inv_tau = 1.0f / tau;
  for (int j = 0; j < P; ++j) {
    const int pj = slot(j);
    if (pj < 0) continue;                                      // fewer than P true positives: slot unused
    const float sp = s_row[pj];
    float sum_p = 0.f, sum_n = 0.f;
    for (int z = threadIdx.x; z < B; z += blockDim.x) {
      const float e = fminf(fmaxf(-(s_row[z] - sp) * inv_tau, -50.f), 50.f);
      const float a = 1.0f / (1.0f + expf(e));
      const uint8_t m = s_m[z];
      if ((m & 1) && z != pj) sum_p += a;
      if (m & 2) sum_n += a;
    }
    const float rp = 1.0f + block_sum(sum_p, s_red);
    const float nn = block_sum(sum_n, s_red);
    const float rw = rp + nn;
    ap_q += rp / rw;
    // the two coefficients multiply every term of this slot: formed in double and rounded once, 1 / tau included
    const double den = (double)rw * (double)rw * (double)n_valid * (double)tau;
    const float c_p = (float)((double)nn / den);             // d(r_j / n_valid) / d r_p / tau
    const float c_n = (float)(-(double)rp / den);            // d(r_j / n_valid) / d N / tau
    float to_pj = 0.f;
    for (int z = threadIdx.x; z < B; z += blockDim.x) {
      const float x = -(s_row[z] - sp) * inv_tau;
      if (x < -50.f || x > 50.f) continue;                    // clamped exponent: zero gradient
      const float ex = expf(x);
      const float a = 1.0f / (1.0f + ex);
      const uint8_t m = s_m[z];
      const float coef = (((m & 1) && z != pj) ? c_p : 0.f) + ((m & 2) ? c_n : 0.f);
      const float gz = coef * (a * (a * ex));                  // 1 - a = a e^x: 1.0f - a is 0 from x = -17 down, e^x is not
      s_g[z] += gz;                                            // thread-private z: no race
      to_pj -= gz;
    }
    const float tp = block_sum(to_pj, s_red);
    if (threadIdx.x == 0) s_g[pj] += tp;
    __syncthreads();
  }
  if (threadIdx.x == 0) ap[q] = n_valid > 0 ? ap_q / (float)n_valid : 0.f;
  for (int z = threadIdx.x; z < B; z += blockDim.x) dap_ds[(int64_t)q * B + z] = s_g[z];
}


// Distillation term of the MESA step (models/losses/loss.py:138-147): per row, with p = softmax(y / T) and q = softmax(t / T),
//     kl = sum_j q_j (log q_j - log p_j),      d kl / d y_j = (p_j - q_j) / T.
// One wavefront owns one row, K = D / 64 elements per lane in registers.  Student and teacher rows are nearly equal (the
// teacher is a moving average of the student), so kl is a small difference of nearly equal numbers; it is therefore built
// from the per-element log ratio of the max-subtracted exponentials
//     delta_j = b_j - a_j,  a_j = (y_j - max y) / T,  b_j = (t_j - max t) / T,   exp(a_j) - exp(b_j) = exp(b_j) expm1(-delta_j)
//     kl = sum_j q_j delta_j + c,   c = log(Zp / Zq) = log1p(sum_j (exp(a_j) - exp(b_j)) / Zq),
//     p_j - q_j = q_j expm1(-(delta_j + c)),
// and not from two log-sum-exps of about log D each.  Where the rows differ grossly (|delta| >= 1) the plain differences are
// exact enough and cannot overflow; where Zp is less than half of Zq the sum of the differences cancels, and Zp is the direct
// sum of the exp(a_j).
template <int K>
__global__ void __launch_bounds__(256)
kd_rows_kernel(float* __restrict__ kl, float* __restrict__ dkl, const float* __restrict__ Y, const float* __restrict__ Tt,
               int B, float inv_t) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;                                      // whole wavefront leaves: no partial shuffles
  const int64_t base = (int64_t)row * (K * 64);
  float y[K], t[K];
  float my = -INFINITY, mt = -INFINITY;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    y[i] = Y[base + i * 64 + lane];
    t[i] = Tt[base + i * 64 + lane];
    my = fmaxf(my, y[i]);
    mt = fmaxf(mt, t[i]);
  }
  my = hfl_group_max<64>(my);
  mt = hfl_group_max<64>(mt);
  const float dm = mt - my;
  float zq = 0.f, zp = 0.f, s_diff = 0.f, s_qd = 0.f;
  float eq[K], dl[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const float a = (y[i] - my) * inv_t, b = (t[i] - mt) * inv_t;
    const float d = ((t[i] - y[i]) - dm) * inv_t;           // b - a, from the two small differences
    const float e = expf(b), ea = expf(a);
    eq[i] = e;
    dl[i] = d;
    zq += e;
    zp += ea;
    s_diff += fabsf(d) < 1.f ? e * expm1f(-d) : ea - e;
    s_qd += e * d;                                           // e == 0 (underflow) times a finite d: 0
  }
  zq = hfl_group_sum<64>(zq);
  zp = hfl_group_sum<64>(zp);
  s_diff = hfl_group_sum<64>(s_diff);
  s_qd = hfl_group_sum<64>(s_qd);
  const float x = s_diff / zq;                               // Zp / Zq - 1  (> -1)
  // Zp < Zq / 2 (a peaked student against a flat teacher): Zq + s_diff is then what is left of a cancellation, with the
  // rounding of sums of Zq's size in it (relative error about D 2^-24); the direct sum of the exp(a_j) has none
  const bool direct = !(x > -0.5f);
  const float c = direct ? logf(zp / zq) : log1pf(x);
  if (lane == 0) kl[row] = s_qd / zq + c;
  const float inv_zq = 1.f / zq, inv_zp = 1.f / (direct ? zp : zq + s_diff);
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const float q = eq[i] * inv_zq;
    const float u = dl[i] + c;                               // log(q_j / p_j)
    const float g = fabsf(u) < 1.f ? q * expm1f(-u) : expf((y[i] - my) * inv_t) * inv_zp - q;
    dkl[base + i * 64 + lane] = g * inv_t;
  }
}

template <int K>
static void kd_launch(float* kl, float* dkl, const float* y, const float* t, int B, float inv_t, hipStream_t st) {
  kd_rows_kernel<K><<<(B + 3) / 4, 256, 0, st>>>(kl, dkl, y, t, B, inv_t);
}

}  // namespace

extern "C" int hfl_smoothap_rows(float* ap, float* dap_ds, const float* sim, const uint8_t* pos_mask,
                                  const uint8_t* neg_mask, const int64_t* closest_pos, int batch,
                                  int positives_per_query, float tau, hfl_stream_t stream) {
  if (batch <= 0 || positives_per_query <= 0 || !(tau > 0.f)) return HFL_EINVAL;
  const size_t lds = (size_t)batch * 9;
  if (lds > 150 * 1024) return HFL_ECAPACITY;               // B <= 17066
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(smoothap_rows_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  smoothap_rows_kernel<<<batch, 256, lds, static_cast<hipStream_t>(stream)>>>(
      ap, dap_ds, sim, pos_mask, neg_mask, closest_pos, batch, positives_per_query, tau);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int hfl_kd_rows(float* kl, float* dkl_dy, const float* y, const float* t, int batch, int dim, float temperature,
                            hfl_stream_t stream) {
  if (batch <= 0 || dim <= 0 || dim % 64 != 0 || dim > 1024 || !(temperature > 0.f)) return HFL_EINVAL;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const float inv_t = 1.0f / temperature;
  switch (dim / 64) {
#define HFL_KD_CASE(K) case K: kd_launch<K>(kl, dkl_dy, y, t, batch, inv_t, st); break;
    HFL_KD_CASE(1) HFL_KD_CASE(2) HFL_KD_CASE(3) HFL_KD_CASE(4) HFL_KD_CASE(5) HFL_KD_CASE(6) HFL_KD_CASE(7) HFL_KD_CASE(8)
    HFL_KD_CASE(9) HFL_KD_CASE(10) HFL_KD_CASE(11) HFL_KD_CASE(12) HFL_KD_CASE(13) HFL_KD_CASE(14) HFL_KD_CASE(15)
    HFL_KD_CASE(16)
#undef HFL_KD_CASE
    default: return HFL_EINVAL;
  }
  HFL_RETURN_LAST_ERROR();
}
