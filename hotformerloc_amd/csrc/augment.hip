// The training augmentation chain of the reference, for a whole batch in one launch, fused with the normalise / mask /
// compaction of csrc/preprocess.hip:
//
//   per cloud   datasets/CSWildPlaces/CSWildPlaces_train.py:19-57 (TrainTransform: Normalize, JitterPoints,
//               RemoveRandomPoints, [RandomRotation about z], RandomTranslation, RemoveRandomBlock), then the masks of
//               datasets/base_datasets.py:77-83
//   per batch   datasets/dataset_utils.py:111-116 (TrainSetTransform: [z rotation], RandomFlip), then the quantizer's
//               cylindrical transform (datasets/coordinate_utils.py)
//
// One 1024-lane workgroup per cloud, no cross-cloud scans, no global atomics.  Up to four passes over the cloud: the
// bounding box of Normalize, a radix select for RemoveRandomPoints (four 256-bin LDS histograms over 32-bit keys that
// are regenerated in every pass, never stored; skipped when k == 0), the bounding box RemoveRandomBlock takes after the
// translation (only when the block coin came up), and the final pass, which recomputes the chain per point, decides the
// masks, applies the batch-wide transform and compacts order-preservingly into the cloud's slot.
//
// Random numbers.  Scalars per cloud and per batch come from the host in a table (hotformerloc_amd/augment.py,
// draw_params).  Per-point numbers are Philox4x32-10 with key = seed and counter = (point index in its cloud, cloud index
// + cloud_base, stream, 0): stream 0 gives the three jitter normals (Box-Muller on the words, uniform = (u32 + 0.5) * 2^-32),
// stream 1 word 0 the point's selection key.  RemoveRandomPoints zeroes the k points with the smallest keys, ties to the
// lower point index: a uniformly random k-subset, the distribution of np.random.choice(replace=False).
//
// Normalize, the block rectangle and the masks are IEEE add / mul / div / sqrt with every rounding of the reference's mix
// of float32 tensors and Python doubles kept (_rn intrinsics, no FMA contraction).  logf / cosf / sinf of the jitter are the
// device library's; a last-bit difference there is 1e-10 in a coordinate.
#include "philox.h"
#include "prep_common.h"

namespace {

__device__ __forceinline__ float unit_open(uint32_t w) {                 // (u32 + 0.5) * 2^-32, in (0, 1]
  return __fmul_rn(__fadd_rn(__uint2float_rn(w), 0.5f), 2.3283064365386963e-10f);
}

struct Cloud {
  const float* p;               // the cloud's raw points
  const uint32_t* keys;         // caller's selection keys of this cloud, or null
  int64_t n;
  uint32_t cloud_id, k0, k1;
  float cx, cy, cz, factor;     // Normalize
  float sigma, clip;
  float rc, rs, tx, ty, tz;     // rotation, translation
  uint32_t thr;                 // RemoveRandomPoints: keys below thr go, keys equal to thr go while index < tie_limit
  int64_t tie_limit;
  int normalize, augment, rotate, remove;
};

__device__ __forceinline__ uint32_t selection_key(const Cloud& c, int64_t i) {
  if (c.keys != nullptr) return c.keys[i];
  return philox4x32_10((uint32_t)i, c.cloud_id, 1u, 0u, c.k0, c.k1).x;
}

// steps 1-5 of the chain for point i
__device__ __forceinline__ void chain(const Cloud& c, int64_t i, float& x, float& y, float& z) {
  x = c.p[i * 3 + 0];
  y = c.p[i * 3 + 1];
  z = c.p[i * 3 + 2];
  if (c.normalize) {
    x = __fmul_rn(__fsub_rn(x, c.cx), c.factor);
    y = __fmul_rn(__fsub_rn(y, c.cy), c.factor);
    z = __fmul_rn(__fsub_rn(z, c.cz), c.factor);
  }
  if (!c.augment) return;
  bool removed = false;
  if (c.remove) {
    const uint32_t key = selection_key(c, i);
    removed = key < c.thr || (key == c.thr && i < c.tie_limit);
  }
  if (removed) {
    x = y = z = 0.f;
  } else {
    const U4 w = philox4x32_10((uint32_t)i, c.cloud_id, 0u, 0u, c.k0, c.k1);
    const float r0 = __fsqrt_rn(__fmul_rn(-2.0f, logf(unit_open(w.x))));
    const float a0 = __fmul_rn(6.2831854820251465f, unit_open(w.y));
    const float r1 = __fsqrt_rn(__fmul_rn(-2.0f, logf(unit_open(w.z))));
    const float a1 = __fmul_rn(6.2831854820251465f, unit_open(w.w));
    const float jx = fminf(fmaxf(__fmul_rn(c.sigma, __fmul_rn(r0, cosf(a0))), -c.clip), c.clip);
    const float jy = fminf(fmaxf(__fmul_rn(c.sigma, __fmul_rn(r0, sinf(a0))), -c.clip), c.clip);
    const float jz = fminf(fmaxf(__fmul_rn(c.sigma, __fmul_rn(r1, cosf(a1))), -c.clip), c.clip);
    x = __fadd_rn(x, jx);
    y = __fadd_rn(y, jy);
    z = __fadd_rn(z, jz);
  }
  if (c.rotate) {
    const float xr = __fadd_rn(__fmul_rn(x, c.rc), __fmul_rn(y, c.rs));
    const float yr = __fadd_rn(__fmul_rn(y, c.rc), -__fmul_rn(x, c.rs));
    x = xr;
    y = yr;
  }
  x = __fadd_rn(x, c.tx);
  y = __fadd_rn(y, c.ty);
  z = __fadd_rn(z, c.tz);
}

__global__ void __launch_bounds__(kPrepThreads)
augment_clouds_kernel(float* __restrict__ out, int32_t* __restrict__ counts, int32_t* __restrict__ index,
                      const float* __restrict__ pts, const int64_t* __restrict__ off,
                      const hfl_augment_cloud* __restrict__ table, hfl_augment_config cfg, uint32_t k0, uint32_t k1,
                      uint32_t cloud_base, const uint32_t* __restrict__ keys) {
  __shared__ float red[kPrepThreads / 64];
  __shared__ int wave_cnt[kPrepThreads / 64];
  __shared__ int running;
  __shared__ unsigned int hist[256];
  __shared__ unsigned int sel_bin, sel_rem, sel_cnt;
  __shared__ long long tie_limit_s;
  const int b = blockIdx.x;
  const int64_t p0 = off[b];
  const int64_t n = off[b + 1] - p0;
  const hfl_augment_cloud t = table[b];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  float* o = out + p0 * 3;
  int32_t* oi = index != nullptr ? index + p0 : nullptr;

  Cloud c;
  c.p = pts + p0 * 3;
  c.keys = keys != nullptr ? keys + p0 : nullptr;
  c.n = n;
  c.cloud_id = cloud_base + (uint32_t)b;
  c.k0 = k0;
  c.k1 = k1;
  c.cx = c.cy = c.cz = 0.f;
  c.factor = 1.f;
  c.sigma = cfg.jitter_sigma;
  c.clip = cfg.jitter_clip;
  c.rc = t.rot_cos;
  c.rs = t.rot_sin;
  c.tx = t.trans[0];
  c.ty = t.trans[1];
  c.tz = t.trans[2];
  c.thr = 0u;
  c.tie_limit = 0;
  c.normalize = cfg.normalize;
  c.augment = cfg.augment;
  c.rotate = cfg.augment && cfg.rotate;
  // the launcher checked 0 <= k <= n on the host copy of the table; the clamp keeps a table that disagrees with it harmless
  const int64_t k = cfg.augment ? (t.remove_k < 0 ? 0 : (t.remove_k > n ? n : (int64_t)t.remove_k)) : 0;
  c.remove = k > 0;

  // ---- pass 1: the bounding box of Normalize
  if (cfg.normalize) {
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = threadIdx.x; i < n; i += kPrepThreads) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float v = c.p[i * 3 + a];
        mn[a] = fminf(mn[a], v);
        mx[a] = fmaxf(mx[a], v);
      }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      mn[a] = block_reduce(mn[a], false, red);
      mx[a] = block_reduce(mx[a], true, red);
    }
    c.cx = __fmul_rn(__fadd_rn(mn[0], mx[0]), 0.5f);
    c.cy = __fmul_rn(__fadd_rn(mn[1], mx[1]), 0.5f);
    c.cz = __fmul_rn(__fadd_rn(mn[2], mx[2]), 0.5f);
    const float ext = fmaxf(fmaxf(__fsub_rn(mx[0], mn[0]), __fsub_rn(mx[1], mn[1])), __fsub_rn(mx[2], mn[2]));
    c.factor = __fdiv_rn(2.0f, __fadd_rn(ext, 1.0e-6f));
  }

  // ---- pass 2: radix select of the k-th smallest selection key, most significant byte first
  if (c.remove) {
    uint32_t prefix = 0u, rem = (uint32_t)k, cnt = 0u;
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      if (threadIdx.x < 256) hist[threadIdx.x] = 0u;
      __syncthreads();
      for (int64_t i = threadIdx.x; i < n; i += kPrepThreads) {
        const uint32_t key = selection_key(c, i);
        if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (threadIdx.x < 256) {
        uint32_t incl = 0u;
        for (int j = 0; j <= (int)threadIdx.x; ++j) incl += hist[j];
        const uint32_t mine = hist[threadIdx.x], excl = incl - mine;
        if (excl < rem && rem <= incl) {         // exactly one bin: 1 <= rem <= number of keys under the prefix
          sel_bin = threadIdx.x;
          sel_rem = rem - excl;
          sel_cnt = mine;
        }
      }
      __syncthreads();
      prefix = (prefix << 8) | sel_bin;
      rem = sel_rem;
      cnt = sel_cnt;
      __syncthreads();
    }
    // cnt points hold the threshold key and the first `rem` of them, in point order, go
    if (threadIdx.x == 0) {
      tie_limit_s = (long long)n;
      running = 0;
    }
    __syncthreads();
    if (rem < cnt) {
      for (int64_t base = 0; base < n; base += kPrepThreads) {
        const int64_t i = base + threadIdx.x;
        const bool tie = i < n && selection_key(c, i) == prefix;
        const unsigned long long m = __ballot(tie);
        if (lane == 0) wave_cnt[wave] = __popcll(m);
        __syncthreads();
        int pos = running;
        for (int w = 0; w < wave; ++w) pos += wave_cnt[w];
        pos += __popcll(m & lt);
        if (tie && (uint32_t)pos == rem - 1u) tie_limit_s = (long long)i + 1;
        __syncthreads();
        if (threadIdx.x == 0) {
          int s = 0;
          for (int w = 0; w < kPrepThreads / 64; ++w) s += wave_cnt[w];
          running += s;
        }
        __syncthreads();
        if ((uint32_t)running >= rem) break;     // uniform: `running` is read after the barrier by every lane
      }
    }
    c.thr = prefix;
    c.tie_limit = tie_limit_s;
  }

  // ---- pass 3: RemoveRandomBlock's rectangle from the bounding box after the translation
  bool block = cfg.augment && t.block != 0;
  float bx0 = 0.f, bx1 = 0.f, by0 = 0.f, by1 = 0.f;
  if (block) {
    float mn[2] = {INFINITY, INFINITY}, mx[2] = {-INFINITY, -INFINITY};
    for (int64_t i = threadIdx.x; i < n; i += kPrepThreads) {
      float x, y, z;
      chain(c, i, x, y, z);
      mn[0] = fminf(mn[0], x);
      mx[0] = fmaxf(mx[0], x);
      mn[1] = fminf(mn[1], y);
      mx[1] = fmaxf(mx[1], y);
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      mn[a] = block_reduce(mn[a], false, red);
      mx[a] = block_reduce(mx[a], true, red);
    }
    // augmentation.py:160-176: float32 tensors, Python doubles only inside math.sqrt
    const float span0 = __fsub_rn(mx[0], mn[0]), span1 = __fsub_rn(mx[1], mn[1]);
    const float area = __fmul_rn(span0, span1);
    const float erase = __fmul_rn(t.block_u[0], area);
    const float h = (float)__dsqrt_rn((double)__fmul_rn(erase, t.block_u[1]));
    const float w = (float)__dsqrt_rn((double)__fdiv_rn(erase, t.block_u[1]));
    bx0 = __fadd_rn(mn[0], __fmul_rn(t.block_u[2], __fsub_rn(span0, w)));
    by0 = __fadd_rn(mn[1], __fmul_rn(t.block_u[3], __fsub_rn(span1, h)));
    bx1 = __fadd_rn(bx0, w);
    by1 = __fadd_rn(by0, h);
  }

  // ---- final pass: chain, block, masks, batch-wide transform, compaction
  __syncthreads();
  if (threadIdx.x == 0) running = 0;
  __syncthreads();
  for (int64_t base = 0; base < n; base += kPrepThreads) {
    const int64_t i = base + threadIdx.x;
    float x = 0.f, y = 0.f, z = 0.f;
    bool keep = false;
    if (i < n) {
      chain(c, i, x, y, z);
      if (block && bx0 < x && x < bx1 && by0 < y && y < by1) x = y = z = 0.f;
      keep = fabsf(x) <= 1.0f && fabsf(y) <= 1.0f && fabsf(z) <= 1.0f;
      if (cfg.cylindrical_mask) keep = keep && __fsqrt_rn(__fmaf_rn(y, y, __fmul_rn(x, x))) <= 1.0f;
      if (keep) {
        if (cfg.set_rotate) {
          const float xr = __fadd_rn(__fmul_rn(x, cfg.set_cos), __fmul_rn(y, cfg.set_sin));
          const float yr = __fadd_rn(__fmul_rn(y, cfg.set_cos), -__fmul_rn(x, cfg.set_sin));
          x = xr;
          y = yr;
        }
        if (cfg.flip_axis == 0) x = -x;
        if (cfg.flip_axis == 1) y = -y;
        if (cfg.flip_axis == 2) z = -z;
        if (cfg.cylindrical_transform) cylindrical_transform(x, y, z);
      }
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int pos = running;
    for (int w = 0; w < wave; ++w) pos += wave_cnt[w];
    pos += __popcll(m & lt);
    if (keep) {                                  // pos < n: at most as many kept points as points
      o[(int64_t)pos * 3 + 0] = x;
      o[(int64_t)pos * 3 + 1] = y;
      o[(int64_t)pos * 3 + 2] = z;
      if (oi != nullptr) oi[pos] = (int32_t)i;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int s = 0;
      for (int w = 0; w < kPrepThreads / 64; ++w) s += wave_cnt[w];
      running += s;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[b] = running;
}

}  // namespace

extern "C" int hfl_augment_clouds(float* out_points, int32_t* out_counts, int32_t* out_index, const float* points,
                                  const int64_t* cloud_offsets, const int64_t* host_cloud_offsets, int batch,
                                  const hfl_augment_cloud* table, const hfl_augment_cloud* host_table,
                                  const hfl_augment_config* config, uint64_t seed, int64_t cloud_base,
                                  const uint32_t* selection_keys, hfl_stream_t stream) {
  if (batch < 0 || out_points == nullptr || out_counts == nullptr || points == nullptr || cloud_offsets == nullptr ||
      host_cloud_offsets == nullptr || table == nullptr || host_table == nullptr || config == nullptr || cloud_base < 0)
    return HFL_EINVAL;
  if (out_points == points) return HFL_EINVAL;        // compaction reads ahead of what it writes only per cloud
  if ((const void*)out_index == (const void*)points || (const void*)out_index == (const void*)out_points ||
      (const void*)out_index == (const void*)out_counts || (const void*)out_counts == (const void*)points ||
      (const void*)out_counts == (const void*)out_points)
    return HFL_EINVAL;
  if (config->flip_axis < -1 || config->flip_axis > 2) return HFL_EINVAL;
  if (host_cloud_offsets[0] < 0) return HFL_EINVAL;
  for (int b = 0; b < batch; ++b) {
    const int64_t n = host_cloud_offsets[b + 1] - host_cloud_offsets[b];
    if (n < 0 || n > INT32_MAX) return HFL_EINVAL;      // the source index and the select's counters are 32-bit
    if (host_table[b].remove_k < 0 || host_table[b].remove_k > n) return HFL_EINVAL;
  }
  if (batch == 0) return HFL_OK;
  augment_clouds_kernel<<<batch, kPrepThreads, 0, static_cast<hipStream_t>(stream)>>>(
      out_points, out_counts, out_index, points, cloud_offsets, table, *config, (uint32_t)seed, (uint32_t)(seed >> 32),
      (uint32_t)cloud_base, selection_keys);
  HFL_RETURN_LAST_ERROR();
}
