// Adam / AdamW step of a whole model in ONE launch (multi-tensor apply), the weight EMA of csrc/ema.hip folded in.
// Reference: training/trainer.py:140-156 builds torch.optim.Adam (weight decay folded into the gradient) or AdamW (decoupled)
// and steps it once per batch (:356); the EMA teacher follows at :360-361.  The scheme is ema_update_kernel's: the host cuts
// every parameter into chunks of at most HFL_ADAM_CHUNK elements and uploads one table entry per chunk; one workgroup owns
// one chunk.  Chunk starts are multiples of HFL_ADAM_CHUNK elements from the tensor's start, so a chunk is 16-byte aligned
// exactly when its tensors are: such chunks move as float4, the others (views at odd offsets) and the last count % 4 elements
// as scalars.  Hyper-parameters arrive BY VALUE in the kernel arguments, one slot per (param group, step count); a chunk
// names its slot.  Pure streaming: 16 bytes read and 12 written per element for the optimizer, 4 + 4 more for the teacher,
// and the parameter is never re-read for the average.
//
// Per element, in the order of torch's _single_tensor_adam and with its roundings (every product, sum, quotient and square
// root is rounded to fp32 exactly where a torch op ends; contraction is switched off and the two fused multiply-adds are
// written out):
//     L2:         g <- g + wd * p                        (grad.add(param, alpha=wd))
//     decoupled:  p <- p * (1 - lr * wd)                 (param.mul_; the factor is rounded once from double by the host)
//     m <- m + (1 - beta1) * (g - m)                     (exp_avg.lerp_; torch's other branch for a weight >= 0.5)
//     v <- beta2 * v;  v <- v + ((1 - beta2) * g) * g    (mul_, addcmul_)
//     denom = sqrt(v) / bias_correction2_sqrt + eps
//     p <- p + (-step_size * m) / denom                  (addcdiv_)
//     ema <- ema + w * (p - ema)                         (hfl_ema_update's line, on the value just stored)
#include "hfl_common.h"

namespace {

struct adam_slots {
  hfl_adam_slot s[HFL_ADAM_MAX_SLOTS];
};

template <bool GRAD, bool EMA>
__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, float& e, const hfl_adam_slot& h, float w) {
#pragma clang fp contract(off)
  if (GRAD) {
    if (h.decoupled) {
      p = p * h.decay;
    } else {
      g = fmaf(h.decay, p, g);
    }
    const float d = g - m;
    m = h.one_minus_beta1 < 0.5f ? fmaf(h.one_minus_beta1, d, m) : g - d * (1.f - h.one_minus_beta1);
    v = v * h.beta2;
    v = fmaf(h.one_minus_beta2 * g, g, v);
    const float denom = sqrtf(v) / h.bias_correction2_sqrt + h.eps;
    p = p + (-h.step_size * m) / denom;
  }
  if (EMA) e = fmaf(w, p - e, e);
}

template <bool GRAD, bool EMA>
__device__ __forceinline__ void adam_chunk(const hfl_adam_chunk& c, const hfl_adam_slot& h, float w) {
  float* __restrict__ param = c.param;
  const float* __restrict__ grad = c.grad;
  float* __restrict__ exp_avg = c.exp_avg;
  float* __restrict__ exp_avg_sq = c.exp_avg_sq;
  float* __restrict__ ema = c.ema;
  const int n = c.count;
  uintptr_t bits = reinterpret_cast<uintptr_t>(param);
  if (GRAD) bits |= reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(exp_avg) | reinterpret_cast<uintptr_t>(exp_avg_sq);
  if (EMA) bits |= reinterpret_cast<uintptr_t>(ema);
  const int n4 = (bits & 15) == 0 ? n >> 2 : 0;
  for (int i = threadIdx.x; i < n4; i += blockDim.x) {
    float4 p = reinterpret_cast<const float4*>(param)[i];
    float4 g = {0.f, 0.f, 0.f, 0.f}, m = g, v = g, e = g;
    if (GRAD) {
      g = reinterpret_cast<const float4*>(grad)[i];
      m = reinterpret_cast<const float4*>(exp_avg)[i];
      v = reinterpret_cast<const float4*>(exp_avg_sq)[i];
    }
    if (EMA) e = reinterpret_cast<const float4*>(ema)[i];
    adam_element<GRAD, EMA>(p.x, g.x, m.x, v.x, e.x, h, w);
    adam_element<GRAD, EMA>(p.y, g.y, m.y, v.y, e.y, h, w);
    adam_element<GRAD, EMA>(p.z, g.z, m.z, v.z, e.z, h, w);
    adam_element<GRAD, EMA>(p.w, g.w, m.w, v.w, e.w, h, w);
    if (GRAD) {
      reinterpret_cast<float4*>(param)[i] = p;
      reinterpret_cast<float4*>(exp_avg)[i] = m;
      reinterpret_cast<float4*>(exp_avg_sq)[i] = v;
    }
    if (EMA) reinterpret_cast<float4*>(ema)[i] = e;
  }
  for (int i = (n4 << 2) + threadIdx.x; i < n; i += blockDim.x) {
    float p = param[i], g = 0.f, m = 0.f, v = 0.f, e = 0.f;
    if (GRAD) {
      g = grad[i];
      m = exp_avg[i];
      v = exp_avg_sq[i];
    }
    if (EMA) e = ema[i];
    adam_element<GRAD, EMA>(p, g, m, v, e, h, w);
    if (GRAD) {
      param[i] = p;
      exp_avg[i] = m;
      exp_avg_sq[i] = v;
    }
    if (EMA) ema[i] = e;
  }
}

__global__ void __launch_bounds__(256)
adam_step_kernel(const hfl_adam_chunk* __restrict__ table, const adam_slots slots, float w) {
  const hfl_adam_chunk c = table[blockIdx.x];
  // masked: an index the host did not fill reads a slot of the argument block, never past it
  const hfl_adam_slot h = slots.s[c.slot & (HFL_ADAM_MAX_SLOTS - 1)];
  if (c.grad != nullptr) {
    if (c.ema != nullptr) {
      adam_chunk<true, true>(c, h, w);
    } else {
      adam_chunk<true, false>(c, h, w);
    }
  } else if (c.ema != nullptr) {
    adam_chunk<false, true>(c, h, w);
  }
}

}  // namespace

extern "C" int hfl_adam_step(const hfl_adam_chunk* table, int n_chunks, const hfl_adam_slot* slots, int n_slots, float w,
                             hfl_stream_t stream) {
  if (n_chunks < 0 || !(w >= 0.f && w <= 1.f)) return HFL_EINVAL;
  if (n_slots < 0 || n_slots > HFL_ADAM_MAX_SLOTS || (n_slots > 0 && slots == nullptr)) return HFL_EINVAL;
  if (n_chunks == 0) return HFL_OK;
  if (table == nullptr) return HFL_EINVAL;
  adam_slots by_value = {};
  for (int i = 0; i < n_slots; ++i) by_value.s[i] = slots[i];
  adam_step_kernel<<<n_chunks, 256, 0, static_cast<hipStream_t>(stream)>>>(table, by_value, w);
  HFL_RETURN_LAST_ERROR();
}
