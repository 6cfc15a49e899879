// Exponential moving average of a whole model's weights in ONE launch (multi-tensor apply):
//     ema[i] <- ema[i] + w * (src[i] - ema[i]),   w = 1 - decay
// (the formula of torch.lerp for w < 0.5, which is what timm's ModelEmaV3.update applies through torch._foreach_lerp_;
// reference: training/trainer.py:161-163, 360-361).  The shipped CS-Wild-Places model has 726 fp32 tensors between 8 and
// 524 288 elements: a launch per tensor is 726 launches of mostly a few microseconds of work.  Here the host cuts every
// (ema, src) pair into chunks of at most HFL_EMA_CHUNK elements and uploads one table of (ema pointer, src pointer, count)
// per chunk; one workgroup owns one chunk.  Chunk starts are multiples of HFL_EMA_CHUNK elements from the tensor's start, so
// a chunk is 16-byte aligned exactly when its tensor is: such chunks move as float4, the others (views at odd offsets) and
// the last count % 4 elements as scalars.  Pure streaming: 8 bytes read and 4 written per element.
#include "hfl_common.h"

namespace {

__global__ void __launch_bounds__(256)
ema_update_kernel(const hfl_ema_chunk* __restrict__ table, float w) {
  const hfl_ema_chunk c = table[blockIdx.x];
  float* __restrict__ ema = c.ema;
  const float* __restrict__ src = c.src;
  const int n = (int)c.count;
  const bool aligned = ((reinterpret_cast<uintptr_t>(ema) | reinterpret_cast<uintptr_t>(src)) & 15) == 0;
  const int n4 = aligned ? n >> 2 : 0;
  float4* __restrict__ e4 = reinterpret_cast<float4*>(ema);
  const float4* __restrict__ s4 = reinterpret_cast<const float4*>(src);
  for (int i = threadIdx.x; i < n4; i += blockDim.x) {
    float4 e = e4[i];
    const float4 s = s4[i];
    e.x = fmaf(w, s.x - e.x, e.x);
    e.y = fmaf(w, s.y - e.y, e.y);
    e.z = fmaf(w, s.z - e.z, e.z);
    e.w = fmaf(w, s.w - e.w, e.w);
    e4[i] = e;
  }
  for (int i = (n4 << 2) + threadIdx.x; i < n; i += blockDim.x) {
    const float e = ema[i];
    ema[i] = fmaf(w, src[i] - e, e);
  }
}

}  // namespace

extern "C" int hfl_ema_update(const hfl_ema_chunk* table, int n_chunks, float w, hfl_stream_t stream) {
  if (n_chunks < 0 || !(w >= 0.f && w <= 1.f)) return HFL_EINVAL;
  if (n_chunks == 0) return HFL_OK;
  if (table == nullptr) return HFL_EINVAL;
  ema_update_kernel<<<n_chunks, 256, 0, static_cast<hipStream_t>(stream)>>>(table, w);
  HFL_RETURN_LAST_ERROR();
}
