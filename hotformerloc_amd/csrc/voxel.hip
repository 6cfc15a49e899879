// Raw submaps -> the clouds `hfl_prepare_clouds` expects, batched and ragged on the device: the CS-Wild-Places submap
// post-processing (datasets/CSWildPlaces/postprocess_submaps.py: processing_utils.voxel_down_sample, which is open3d's
// PointCloud.voxel_down_sample, then processing_utils.normalise_pcl with downsample_number=None).
//
//   hfl_voxel_keys        per-cloud bounds (ordered-integer atomic max, so any number of workgroups per cloud), then one
//                         int64 key per point, cloud << 48 | ix << 32 | iy << 16 | iz, with the cell computed in float64
//                         exactly as open3d does: floor((double(p) - origin) / v), origin = double(min) - 0.5 v
//   (the caller sorts the keys: torch.sort(stable=True), plumbing like torch.topk in the loss)
//   hfl_voxel_reduce      segment heads -> block counts -> scan -> segment starts -> one float64 sum per segment, the fp32
//                         mean written compacted in key order, plus every cloud's first output row
//   hfl_submap_normalise  one workgroup per cloud: float64 centroid, float64 mean radius d, s = 0.5 / d, q' = s (q - c),
//                         |q'| <= 1 mask and an order-preserving compaction (the pattern of csrc/preprocess.hip)
//
// Nothing is sized by a cloud that fits LDS, no workgroup waits for another inside a launch (every dependency is a
// launch boundary), and there is no floating-point atomic: every sum has a fixed order that depends only on a point's
// position within its cloud / cell, so two runs give the same bits and a cloud gives the same bits alone or in a batch.
#include "prep_common.h"
#include "ragged_common.h"

namespace {

constexpr int kVoxThreads = 256;
constexpr int kVoxQuad = 4;                    // points per thread in the per-point kernels: 48 B = three 16-B loads
constexpr int kScanItems = 8;                  // keys per thread in the head count / segment start kernels
constexpr int kScanBlock = kVoxThreads * kScanItems;
constexpr int kScanThreads = 1024;             // the single workgroup that scans the block counts
constexpr int kSerialSegment = 32;             // a longer segment is summed by its whole wave

// monotone map float -> uint32 (a < b  <=>  enc(a) < enc(b)), so min / max become integer atomics
__device__ __forceinline__ uint32_t enc_ordered(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dec_ordered(uint32_t e) {
  return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
}

// the up to four points 4 t .. 4 t + 3 of a thread; a full quad is three aligned 16-byte loads (the array starts 16-B aligned)
__device__ __forceinline__ int load_quad(const float* __restrict__ pts, int64_t i0, int64_t n, float (&v)[12]) {
  if (i0 + kVoxQuad <= n) {
    const float4* p4 = reinterpret_cast<const float4*>(pts + i0 * 3);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float4 q = p4[k];
      v[4 * k + 0] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
    }
    return kVoxQuad;
  }
  const int cnt = (int)(n - i0);
#pragma unroll
  for (int k = 0; k < 3 * kVoxQuad; ++k) v[k] = k < cnt * 3 ? pts[i0 * 3 + k] : 0.f;
  return cnt;
}

// bounds (batch, 6) uint32, zeroed before the launch: [0..2] = max of ~enc(p) (the minimum), [3..5] = max of enc(p)
__device__ __forceinline__ void flush_bounds(uint32_t* __restrict__ bounds, int c, const float (&mn)[3], const float (&mx)[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    atomicMax(bounds + (int64_t)c * 6 + a, ~enc_ordered(mn[a]));
    atomicMax(bounds + (int64_t)c * 6 + 3 + a, enc_ordered(mx[a]));
  }
}

__global__ void __launch_bounds__(kVoxThreads)
voxel_bounds_kernel(uint32_t* __restrict__ bounds, const float* __restrict__ pts, const int64_t* __restrict__ off,
                    int batch, int64_t n) {
  const int64_t i0 = ((int64_t)blockIdx.x * kVoxThreads + threadIdx.x) * kVoxQuad;
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  int c = -1;
  if (i0 < n) {
    float v[12];
    const int cnt = load_quad(pts, i0, n, v);
    c = find_cloud(off, batch, i0);
    int64_t nxt = off[c + 1];
#pragma unroll
    for (int k = 0; k < kVoxQuad; ++k) {
      if (k >= cnt) break;
      if (i0 + k >= nxt && c + 1 < batch) {                 // the quad crosses into the next cloud (clouds are non-empty)
        flush_bounds(bounds, c, mn, mx);
        ++c;
        nxt = off[c + 1];
#pragma unroll
        for (int a = 0; a < 3; ++a) { mn[a] = INFINITY; mx[a] = -INFINITY; }
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        mn[a] = fminf(mn[a], v[3 * k + a]);
        mx[a] = fmaxf(mx[a], v[3 * k + a]);
      }
    }
  }
  // a wave whose lanes all ended in the same cloud (the usual case) sends six atomics, not 384
  int cref = c;
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) cref = max(cref, __shfl_xor(cref, m, 64));
  const bool uniform = __all(c == cref || c < 0);
  if (uniform) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int m = 32; m > 0; m >>= 1) {
        mn[a] = fminf(mn[a], __shfl_xor(mn[a], m, 64));
        mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], m, 64));
      }
    }
    if ((threadIdx.x & 63) == 0 && cref >= 0) flush_bounds(bounds, cref, mn, mx);
  } else if (c >= 0) {
    flush_bounds(bounds, c, mn, mx);
  }
}

// origin of cloud c's grid along `axis`: double(min) - 0.5 v
__device__ __forceinline__ double grid_origin(const uint32_t* __restrict__ bounds, int c, int axis, double v) {
  return __dsub_rn((double)dec_ordered(~bounds[(int64_t)c * 6 + axis]), __dmul_rn(0.5, v));
}

// floor((double(p) - origin) / v), clamped into the key's 16 bits so that a key always names its own cloud
// (a cloud that needs the clamp is flagged and never returned)
__device__ __forceinline__ int64_t cell_of(float p, double origin, double v, bool& over) {
  const double c = floor(__ddiv_rn(__dsub_rn((double)p, origin), v));
  over = !(c < 65535.0);                                     // index 65535 is the 65536th cell of the axis
  return (int64_t)fmax(fmin(c, 65535.0), 0.0);
}

__global__ void __launch_bounds__(kVoxThreads)
voxel_keys_kernel(int64_t* __restrict__ keys, int32_t* __restrict__ flags, const uint32_t* __restrict__ bounds,
                  const float* __restrict__ pts, const int64_t* __restrict__ off, int batch, int64_t n, double voxel) {
  const int64_t i0 = ((int64_t)blockIdx.x * kVoxThreads + threadIdx.x) * kVoxQuad;
  if (i0 >= n) return;
  float v[12];
  const int cnt = load_quad(pts, i0, n, v);
  int c = find_cloud(off, batch, i0);
  int64_t key[kVoxQuad] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < kVoxQuad; ++k) {
    if (k >= cnt) break;
    const int64_t i = i0 + k;
    while (c + 1 < batch && i >= off[c + 1]) ++c;            // the quad crosses into the next cloud (clouds are non-empty)
    const double gx = grid_origin(bounds, c, 0, voxel), gy = grid_origin(bounds, c, 1, voxel),
                 gz = grid_origin(bounds, c, 2, voxel);
    bool ox, oy, oz;
    const int64_t ix = cell_of(v[3 * k + 0], gx, voxel, ox);
    const int64_t iy = cell_of(v[3 * k + 1], gy, voxel, oy);
    const int64_t iz = cell_of(v[3 * k + 2], gz, voxel, oz);
    key[k] = ((int64_t)c << 48) | (ix << 32) | (iy << 16) | iz;
    if (i == off[c]) {                                       // one writer per cloud: the cell of the cloud's maximum
      cell_of(dec_ordered(bounds[(int64_t)c * 6 + 3]), gx, voxel, ox);
      cell_of(dec_ordered(bounds[(int64_t)c * 6 + 4]), gy, voxel, oy);
      cell_of(dec_ordered(bounds[(int64_t)c * 6 + 5]), gz, voxel, oz);
      flags[c] = (ox || oy || oz) ? 1 : 0;
    }
  }
  if (cnt == kVoxQuad) {
    longlong2* k2 = reinterpret_cast<longlong2*>(keys + i0);
    k2[0] = make_longlong2(key[0], key[1]);
    k2[1] = make_longlong2(key[2], key[3]);
  } else {
#pragma unroll
    for (int k = 0; k < kVoxQuad - 1; ++k)
      if (k < cnt) keys[i0 + k] = key[k];
  }
}

// ------------------------------------------------------------------------------------------------ reduce
__device__ __forceinline__ bool is_head(const int64_t* __restrict__ keys, int64_t i) {
  return i == 0 || keys[i] != keys[i - 1];
}

// block_counts[b] = segment heads among keys [b kScanBlock, (b + 1) kScanBlock)
__global__ void __launch_bounds__(kVoxThreads)
voxel_head_count_kernel(int32_t* __restrict__ block_counts, const int64_t* __restrict__ keys, int64_t n) {
  __shared__ int wave_cnt[kVoxThreads / 64];
  const int64_t base = (int64_t)blockIdx.x * kScanBlock;
  int cnt = 0;                                               // wave-uniform
#pragma unroll
  for (int it = 0; it < kScanItems; ++it) {
    const int64_t i = base + it * kVoxThreads + threadIdx.x;
    cnt += __popcll(__ballot(i < n && is_head(keys, i)));
  }
  if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < kVoxThreads / 64; ++w) t += wave_cnt[w];
    block_counts[blockIdx.x] = t;
  }
}

// in place: block_counts[b] <- sum of block_counts[< b]; the total goes to block_counts[n_blocks], to
// out_offsets[batch] and, as the end of the last segment, seg_start[total] = n.  One workgroup.
__global__ void __launch_bounds__(kScanThreads)
voxel_scan_kernel(int32_t* __restrict__ block_counts, int n_blocks, int32_t* __restrict__ seg_start,
                  int64_t* __restrict__ out_offsets, int batch, int64_t n) {
  __shared__ int wave_tot[kScanThreads / 64];
  __shared__ int carry;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < n_blocks; base += kScanThreads) {
    const int i = base + threadIdx.x;
    const int v = i < n_blocks ? block_counts[i] : 0;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(incl, d, 64);
      if (lane >= d) incl += o;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int before = carry;
    for (int w = 0; w < wave; ++w) before += wave_tot[w];
    if (i < n_blocks) block_counts[i] = before + incl - v;
    __syncthreads();
    if (threadIdx.x == kScanThreads - 1) carry = before + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int total = carry;
    block_counts[n_blocks] = total;
    seg_start[total] = (int32_t)n;
    out_offsets[batch] = total;
  }
}

// seg_start[slot] = first sorted position of output row `slot`; out_offsets[c] = first output row of cloud c
__global__ void __launch_bounds__(kVoxThreads)
voxel_seg_start_kernel(int32_t* __restrict__ seg_start, int64_t* __restrict__ out_offsets,
                       const int32_t* __restrict__ block_offsets, const int64_t* __restrict__ keys, int64_t n, int batch) {
  __shared__ int wave_cnt[kVoxThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  const int64_t base = (int64_t)blockIdx.x * kScanBlock;
  int running = block_offsets[blockIdx.x];                   // the same in every thread
  for (int it = 0; it < kScanItems; ++it) {
    const int64_t i = base + it * kVoxThreads + threadIdx.x;
    const bool head = i < n && is_head(keys, i);
    const unsigned long long m = __ballot(head);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int pos = running, tot = 0;
    for (int w = 0; w < kVoxThreads / 64; ++w) {
      if (w < wave) pos += wave_cnt[w];
      tot += wave_cnt[w];
    }
    pos += __popcll(m & lt);
    if (head) {
      seg_start[pos] = (int32_t)i;
      const int64_t c = keys[i] >> 48;
      if ((i == 0 || (keys[i - 1] >> 48) != c) && c >= 0 && c < batch) out_offsets[c] = pos;
    }
    running += tot;
    __syncthreads();
  }
}

// one thread per output row: the float64 sum of its segment's points in sorted (= original, the sort is stable) order; a
// segment longer than kSerialSegment is summed by the whole wave, lane l taking members l, l + 64, ... and a butterfly
__global__ void __launch_bounds__(kVoxThreads)
voxel_mean_kernel(float* __restrict__ out, int32_t* __restrict__ cell_counts, int64_t* __restrict__ out_keys,
                  const int32_t* __restrict__ seg_start, const int32_t* __restrict__ total, const int64_t* __restrict__ keys,
                  const int64_t* __restrict__ perm, const float* __restrict__ pts, int64_t n) {
  const int64_t s = (int64_t)blockIdx.x * kVoxThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool valid = s < *total;
  int start = 0, len = 0;
  if (valid) {
    start = seg_start[s];
    len = seg_start[s + 1] - start;
  }
  double sx = 0.0, sy = 0.0, sz = 0.0;
  if (valid && len <= kSerialSegment) {
    for (int j = 0; j < len; ++j) {
      const int64_t p = perm[(int64_t)start + j];
      sx += (double)pts[p * 3 + 0];
      sy += (double)pts[p * 3 + 1];
      sz += (double)pts[p * 3 + 2];
    }
  }
  unsigned long long todo = __ballot(valid && len > kSerialSegment);
  while (todo) {
    const int l = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int64_t st = __shfl(start, l, 64);
    const int ln = __shfl(len, l, 64);
    double ax = 0.0, ay = 0.0, az = 0.0;
    for (int j = lane; j < ln; j += 64) {
      const int64_t p = perm[st + j];
      ax += (double)pts[p * 3 + 0];
      ay += (double)pts[p * 3 + 1];
      az += (double)pts[p * 3 + 2];
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
      ax += __shfl_xor(ax, m, 64);
      ay += __shfl_xor(ay, m, 64);
      az += __shfl_xor(az, m, 64);
    }
    if (lane == l) { sx = ax; sy = ay; sz = az; }
  }
  if (valid) {
    const double cnt = (double)len;
    out[s * 3 + 0] = (float)__ddiv_rn(sx, cnt);
    out[s * 3 + 1] = (float)__ddiv_rn(sy, cnt);
    out[s * 3 + 2] = (float)__ddiv_rn(sz, cnt);
    if (cell_counts != nullptr) cell_counts[s] = len;
    if (out_keys != nullptr) out_keys[s] = keys[start];
  }
}

// ------------------------------------------------------------------------------------------------ normalise
// centroid c and scale s = 0.5 / d (d = mean |q - c|) of the n >= 1 points at p, float64 in a fixed order, in every lane;
// true when d is not > 0 (a single point, coincident points or a non-finite input), and then s = 0
__device__ __forceinline__ bool submap_stats(const float* __restrict__ p, int64_t n, double* red, double (&c)[3], double& scale) {
  {
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t i = threadIdx.x; i < n; i += kPrepThreads) {
#pragma unroll
      for (int a = 0; a < 3; ++a) s[a] += (double)p[i * 3 + a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = __ddiv_rn(block_sum<kPrepThreads>(s[a], red), (double)n);
  }
  double rs = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kPrepThreads) {
    const double dx = (double)p[i * 3 + 0] - c[0], dy = (double)p[i * 3 + 1] - c[1], dz = (double)p[i * 3 + 2] - c[2];
    rs += sqrt(dx * dx + dy * dy + dz * dz);
  }
  const double d = __ddiv_rn(block_sum<kPrepThreads>(rs, red), (double)n);
  const bool degenerate = !(d > 0.0);                        // a single point, coincident points or a non-finite input
  scale = degenerate ? 0.0 : __ddiv_rn(0.5, d);
  return degenerate;
}

// q' = s (q - c) of one row in float64; true when every |q'| <= 1
__device__ __forceinline__ bool submap_scaled_row(const float* __restrict__ q, const double (&c)[3], double scale, double& x,
                                                  double& y, double& z) {
  x = __dmul_rn(scale, (double)q[0] - c[0]);
  y = __dmul_rn(scale, (double)q[1] - c[1]);
  z = __dmul_rn(scale, (double)q[2] - c[2]);
  return fabs(x) <= 1.0 && fabs(y) <= 1.0 && fabs(z) <= 1.0;
}

__global__ void __launch_bounds__(kPrepThreads)
submap_normalise_kernel(float* __restrict__ out, int32_t* __restrict__ counts, int32_t* __restrict__ flags,
                        const float* __restrict__ pts, const int64_t* __restrict__ off) {
  __shared__ double red[kPrepThreads / 64];
  __shared__ int wave_cnt[kPrepThreads / 64];
  __shared__ int running;
  const int b = blockIdx.x;
  const int64_t p0 = off[b];
  const int64_t n = off[b + 1] - p0;
  const float* p = pts + p0 * 3;
  float* o = out + p0 * 3;
  if (n < 1) {                                               // uniform over the workgroup
    if (threadIdx.x == 0) { counts[b] = 0; flags[b] = 1; }
    return;
  }
  double c[3], scale;
  const bool degenerate = submap_stats(p, n, red, c, scale);
  if (threadIdx.x == 0) running = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  for (int64_t base = 0; base < n; base += kPrepThreads) {
    const int64_t i = base + threadIdx.x;
    double x = 0.0, y = 0.0, z = 0.0;
    bool keep = false;
    if (i < n) keep = submap_scaled_row(p + i * 3, c, scale, x, y, z);
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int pos = running;
    for (int w = 0; w < wave; ++w) pos += wave_cnt[w];
    pos += __popcll(m & lt);
    if (keep) {
      o[(int64_t)pos * 3 + 0] = (float)x;
      o[(int64_t)pos * 3 + 1] = (float)y;
      o[(int64_t)pos * 3 + 2] = (float)z;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int t = 0;
      for (int w = 0; w < kPrepThreads / 64; ++w) t += wave_cnt[w];
      running += t;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    counts[b] = running;
    flags[b] = degenerate ? 1 : 0;
  }
}

// the same c, s and transform for rows drawn from another cloud (the padding loop of normalise_pcl): row j of cloud b,
// j in [row_off[b], row_off[b + 1]), is raw row raw_off[b] + row_index[j]; an index outside the raw cloud, or a cloud
// that cannot be normalised, gives a zero row with keep = 0
__global__ void __launch_bounds__(kPrepThreads)
submap_normalise_rows_kernel(float* __restrict__ out_rows, int32_t* __restrict__ keep, const float* __restrict__ pts,
                             const int64_t* __restrict__ off, const float* __restrict__ raw,
                             const int64_t* __restrict__ raw_off, const int64_t* __restrict__ row_index,
                             const int64_t* __restrict__ row_off) {
  __shared__ double red[kPrepThreads / 64];
  const int b = blockIdx.x;
  const int64_t p0 = off[b];
  const int64_t n = off[b + 1] - p0;
  const int64_t j0 = row_off[b], j1 = row_off[b + 1];
  const int64_t r0 = raw_off[b];
  const int64_t n_raw = raw_off[b + 1] - r0;
  double c[3] = {0.0, 0.0, 0.0}, scale = 0.0;
  bool degenerate = true;
  if (n >= 1) degenerate = submap_stats(pts + p0 * 3, n, red, c, scale);      // uniform over the workgroup
  for (int64_t j = j0 + threadIdx.x; j < j1; j += kPrepThreads) {
    const int64_t idx = row_index[j];
    double x = 0.0, y = 0.0, z = 0.0;
    bool ok = false;
    if (!degenerate && idx >= 0 && idx < n_raw) ok = submap_scaled_row(raw + (r0 + idx) * 3, c, scale, x, y, z);
    else x = y = z = 0.0;
    out_rows[j * 3 + 0] = (float)x;
    out_rows[j * 3 + 1] = (float)y;
    out_rows[j * 3 + 2] = (float)z;
    keep[j] = ok ? 1 : 0;
  }
}

// out[r] = points[index[r]]; an index outside [0, n_points) gives a zero row
__global__ void __launch_bounds__(kVoxThreads)
voxel_gather_rows_kernel(float* __restrict__ out, const float* __restrict__ pts, int64_t n_points,
                         const int64_t* __restrict__ index, int64_t n_rows) {
  const int64_t r = (int64_t)blockIdx.x * kVoxThreads + threadIdx.x;
  if (r >= n_rows) return;
  const int64_t i = index[r];
  const bool ok = i >= 0 && i < n_points;
#pragma unroll
  for (int a = 0; a < 3; ++a) out[r * 3 + a] = ok ? pts[i * 3 + a] : 0.f;
}

// ------------------------------------------------------------------------------------------------ occupancy
// How many cells does cloud c occupy at voxel size v, for many (c, v) candidates in one launch: every candidate owns a
// bitmap of nx ny nz bits (cell (ix, iy, iz) is bit (ix ny + iy) nz + iz) in a zeroed workspace.  gridDim.x workgroups per
// candidate stream the cloud's points with a stride; bits are set with integer OR atomics, so the bitmap -- and the count
// -- is the same whatever the arrival order, and no workgroup waits for another.
//
// A bitmap of up to kOccLdsWords words is built in LDS first and only its non-zero words are merged into the global one
// (one global atomic per touched word and workgroup, not per point).  32 KiB: five workgroups of four waves share a CU's
// 160 KiB, i.e. 20 of its 32 wave slots, which is what the float64 divides of this kernel can use; 262 144 cells covers
// every candidate of the PointNetVLAD search on a 100 m submap down to v = 1 m.  A larger bitmap is set in global memory,
// testing the word first: most points fall into a cell that is already marked.
constexpr int kOccLdsWords = 8192;
constexpr int kOccPointsPerGroup = 8192;        // the least a workgroup should stream to pay for zeroing and merging
constexpr int kOccMaxGroups = 64;               // per candidate

__global__ void __launch_bounds__(kVoxThreads)
voxel_occupancy_kernel(uint32_t* __restrict__ bitmaps, const hfl_voxel_candidate* __restrict__ cand,
                       const uint32_t* __restrict__ bounds, const float* __restrict__ pts, const int64_t* __restrict__ off,
                       int64_t n) {
  __shared__ uint32_t lds[kOccLdsWords];
  const hfl_voxel_candidate cd = cand[blockIdx.y];
  const int c = cd.cloud;
  const int64_t p0 = max(off[c], (int64_t)0), p1 = min(off[c + 1], n);
  // the quads of the whole array that overlap the cloud: a quad starts 16-byte aligned only in the array's numbering
  const int64_t q0 = p0 / kVoxQuad, q1 = (p1 + kVoxQuad - 1) / kVoxQuad;
  const int64_t first = q0 + (int64_t)blockIdx.x * kVoxThreads;
  if (first >= q1) return;                                   // uniform: the cloud is too short to need this workgroup
  const int64_t stride = (int64_t)gridDim.x * kVoxThreads;
  const int64_t nx = cd.nx, ny = cd.ny, nz = cd.nz;
  const int64_t n_words = (nx * ny * nz + 31) >> 5;
  const bool in_lds = n_words <= kOccLdsWords;               // uniform
  uint32_t* g = bitmaps + cd.word_offset;
  if (in_lds) {
    for (int w = threadIdx.x; w < (int)n_words; w += kVoxThreads) lds[w] = 0u;
    __syncthreads();
  }
  const double voxel = cd.voxel;
  const double gx = grid_origin(bounds, c, 0, voxel), gy = grid_origin(bounds, c, 1, voxel),
               gz = grid_origin(bounds, c, 2, voxel);
  const volatile uint32_t* lds_seen = lds;
  const volatile uint32_t* g_seen = g;
  for (int64_t q = first + threadIdx.x; q < q1; q += stride) {
    float v[12];
    const int64_t i0 = q * kVoxQuad;
    const int cnt = load_quad(pts, i0, n, v);
#pragma unroll
    for (int k = 0; k < kVoxQuad; ++k) {
      const int64_t i = i0 + k;
      if (k >= cnt || i < p0 || i >= p1) continue;
      bool ox, oy, oz;
      const int64_t ix = cell_of(v[3 * k + 0], gx, voxel, ox);
      const int64_t iy = cell_of(v[3 * k + 1], gy, voxel, oy);
      const int64_t iz = cell_of(v[3 * k + 2], gz, voxel, oz);
      if (ix >= nx || iy >= ny || iz >= nz) continue;        // never for a table built from the same bounds; no write
      const int64_t bit = (ix * ny + iy) * nz + iz;          // outside the bitmap whatever the table says
      const int64_t w = bit >> 5;
      const uint32_t m = 1u << (bit & 31);
      if (in_lds) {
        if (!(lds_seen[w] & m)) atomicOr(lds + w, m);
      } else {
        if (!(g_seen[w] & m)) atomicOr(g + w, m);
      }
    }
  }
  if (in_lds) {
    __syncthreads();
    for (int w = threadIdx.x; w < (int)n_words; w += kVoxThreads) {
      const uint32_t m = lds[w];
      if (m != 0u) atomicOr(g + w, m);
    }
  }
}

// counts[candidate] = set bits of its bitmap; one workgroup per candidate, integer sums
__global__ void __launch_bounds__(kVoxThreads)
voxel_popcount_kernel(int32_t* __restrict__ counts, const uint32_t* __restrict__ bitmaps,
                      const hfl_voxel_candidate* __restrict__ cand) {
  __shared__ int wave_cnt[kVoxThreads / 64];
  const hfl_voxel_candidate cd = cand[blockIdx.x];
  const int64_t n_words = ((int64_t)cd.nx * cd.ny * cd.nz + 31) >> 5;
  const uint32_t* g = bitmaps + cd.word_offset;
  int t = 0;
  for (int64_t w = threadIdx.x; w < n_words; w += kVoxThreads) t += __popc(g[w]);
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) t += __shfl_xor(t, m, 64);
  if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int w = 0; w < kVoxThreads / 64; ++w) total += wave_cnt[w];
    counts[blockIdx.x] = total;
  }
}

int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

}  // namespace

extern "C" int hfl_voxel_keys(int64_t* keys, int32_t* flags, uint32_t* bounds, const float* points,
                              const int64_t* cloud_offsets, int batch, int64_t n_points, double voxel_size,
                              hfl_stream_t stream) {
  if (keys == nullptr || flags == nullptr || bounds == nullptr || points == nullptr || cloud_offsets == nullptr)
    return HFL_EINVAL;
  if (batch < 1 || n_points < batch || !(voxel_size > 0.0) || !(voxel_size <= 1.7976931348623157e308)) return HFL_EINVAL;
  if (batch > HFL_VOXEL_MAX_CLOUDS || n_points > HFL_VOXEL_MAX_POINTS) return HFL_ECAPACITY;
  if ((reinterpret_cast<uintptr_t>(points) & 15) || (reinterpret_cast<uintptr_t>(keys) & 15)) return HFL_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(bounds, 0, sizeof(uint32_t) * 6 * (size_t)batch, s);
  if (e != hipSuccess) return (int)e;
  const unsigned blocks = (unsigned)hfl_cdiv(n_points, (int64_t)kVoxThreads * kVoxQuad);
  voxel_bounds_kernel<<<blocks, kVoxThreads, 0, s>>>(bounds, points, cloud_offsets, batch, n_points);
  voxel_keys_kernel<<<blocks, kVoxThreads, 0, s>>>(keys, flags, bounds, points, cloud_offsets, batch, n_points, voxel_size);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int64_t hfl_voxel_reduce_workspace(int64_t n_points) {
  if (n_points < 1 || n_points > HFL_VOXEL_MAX_POINTS) return 0;
  const int64_t n_blocks = hfl_cdiv(n_points, kScanBlock);
  return align16(4 * (n_blocks + 1)) + align16(4 * (n_points + 1));
}

extern "C" int hfl_voxel_reduce(float* out_points, int64_t* out_offsets, int32_t* out_cell_counts, int64_t* out_keys,
                                const int64_t* sorted_keys, const int64_t* perm, const float* points, int64_t n_points,
                                int batch, void* workspace, int64_t workspace_bytes, hfl_stream_t stream) {
  if (out_points == nullptr || out_offsets == nullptr || sorted_keys == nullptr || perm == nullptr || points == nullptr ||
      workspace == nullptr || out_points == points)
    return HFL_EINVAL;
  if (batch < 1 || n_points < batch) return HFL_EINVAL;
  if (batch > HFL_VOXEL_MAX_CLOUDS || n_points > HFL_VOXEL_MAX_POINTS) return HFL_ECAPACITY;
  if (workspace_bytes < hfl_voxel_reduce_workspace(n_points) || (reinterpret_cast<uintptr_t>(workspace) & 15))
    return HFL_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int n_blocks = (int)hfl_cdiv(n_points, kScanBlock);
  int32_t* block_counts = static_cast<int32_t*>(workspace);
  int32_t* seg_start = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + align16(4 * ((int64_t)n_blocks + 1)));
  voxel_head_count_kernel<<<n_blocks, kVoxThreads, 0, s>>>(block_counts, sorted_keys, n_points);
  voxel_scan_kernel<<<1, kScanThreads, 0, s>>>(block_counts, n_blocks, seg_start, out_offsets, batch, n_points);
  voxel_seg_start_kernel<<<n_blocks, kVoxThreads, 0, s>>>(seg_start, out_offsets, block_counts, sorted_keys, n_points, batch);
  voxel_mean_kernel<<<(unsigned)hfl_cdiv(n_points, kVoxThreads), kVoxThreads, 0, s>>>(
      out_points, out_cell_counts, out_keys, seg_start, block_counts + n_blocks, sorted_keys, perm, points, n_points);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int hfl_submap_normalise(float* out_points, int32_t* out_counts, int32_t* flags, const float* points,
                                    const int64_t* cloud_offsets, int batch, hfl_stream_t stream) {
  if (batch < 0 || out_points == nullptr || out_counts == nullptr || flags == nullptr || points == nullptr ||
      cloud_offsets == nullptr || out_points == points)
    return HFL_EINVAL;
  if (batch == 0) return HFL_OK;
  submap_normalise_kernel<<<batch, kPrepThreads, 0, static_cast<hipStream_t>(stream)>>>(out_points, out_counts, flags, points,
                                                                                       cloud_offsets);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int hfl_submap_normalise_rows(float* out_rows, int32_t* keep, const float* points, const int64_t* cloud_offsets,
                                         const float* raw_points, const int64_t* raw_offsets, const int64_t* row_index,
                                         const int64_t* row_offsets, int batch, hfl_stream_t stream) {
  if (batch < 0 || out_rows == nullptr || keep == nullptr || points == nullptr || cloud_offsets == nullptr ||
      raw_points == nullptr || raw_offsets == nullptr || row_index == nullptr || row_offsets == nullptr)
    return HFL_EINVAL;
  if (batch == 0) return HFL_OK;
  submap_normalise_rows_kernel<<<batch, kPrepThreads, 0, static_cast<hipStream_t>(stream)>>>(
      out_rows, keep, points, cloud_offsets, raw_points, raw_offsets, row_index, row_offsets);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int hfl_voxel_gather_rows(float* out_points, const float* points, int64_t n_points, const int64_t* index,
                                     int64_t n_rows, hfl_stream_t stream) {
  if (n_rows < 0 || n_points < 0 || out_points == nullptr || points == nullptr || index == nullptr || out_points == points)
    return HFL_EINVAL;
  if (n_rows > HFL_VOXEL_MAX_POINTS) return HFL_ECAPACITY;
  if (n_rows == 0) return HFL_OK;
  voxel_gather_rows_kernel<<<(unsigned)hfl_cdiv(n_rows, kVoxThreads), kVoxThreads, 0, static_cast<hipStream_t>(stream)>>>(
      out_points, points, n_points, index, n_rows);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int hfl_voxel_bounds(uint32_t* bounds, const float* points, const int64_t* cloud_offsets, int batch,
                                int64_t n_points, hfl_stream_t stream) {
  if (bounds == nullptr || points == nullptr || cloud_offsets == nullptr) return HFL_EINVAL;
  if (batch < 1 || n_points < batch) return HFL_EINVAL;
  if (batch > HFL_VOXEL_MAX_CLOUDS || n_points > HFL_VOXEL_MAX_POINTS) return HFL_ECAPACITY;
  if (reinterpret_cast<uintptr_t>(points) & 15) return HFL_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(bounds, 0, sizeof(uint32_t) * 6 * (size_t)batch, s);
  if (e != hipSuccess) return (int)e;
  const unsigned blocks = (unsigned)hfl_cdiv(n_points, (int64_t)kVoxThreads * kVoxQuad);
  voxel_bounds_kernel<<<blocks, kVoxThreads, 0, s>>>(bounds, points, cloud_offsets, batch, n_points);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int64_t hfl_voxel_occupancy_workspace(int n_candidates, int64_t bitmap_words) {
  if (n_candidates < 1 || n_candidates > HFL_VOXEL_OCC_MAX_CANDIDATES || bitmap_words < 1 ||
      bitmap_words > HFL_VOXEL_OCC_MAX_WORDS)
    return 0;
  return align16((int64_t)sizeof(hfl_voxel_candidate) * n_candidates) + align16(4 * bitmap_words);
}

extern "C" int hfl_voxel_occupancy(int32_t* counts, const hfl_voxel_candidate* candidates, int n_candidates,
                                   int64_t bitmap_words, const uint32_t* bounds, const float* points,
                                   const int64_t* cloud_offsets, int batch, int64_t n_points, int64_t max_cloud_points,
                                   void* workspace, int64_t workspace_bytes, hfl_stream_t stream) {
  if (counts == nullptr || candidates == nullptr || bounds == nullptr || points == nullptr || cloud_offsets == nullptr ||
      workspace == nullptr)
    return HFL_EINVAL;
  if (batch < 1 || n_points < batch || max_cloud_points < 1) return HFL_EINVAL;
  if (batch > HFL_VOXEL_MAX_CLOUDS || n_points > HFL_VOXEL_MAX_POINTS) return HFL_ECAPACITY;
  if (n_candidates < 1 || bitmap_words < 1) return HFL_EINVAL;
  if (n_candidates > HFL_VOXEL_OCC_MAX_CANDIDATES || bitmap_words > HFL_VOXEL_OCC_MAX_WORDS) return HFL_ECAPACITY;
  if ((reinterpret_cast<uintptr_t>(points) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 15) ||
      workspace_bytes < hfl_voxel_occupancy_workspace(n_candidates, bitmap_words))
    return HFL_EINVAL;
  for (int k = 0; k < n_candidates; ++k) {                   // every bitmap inside the workspace, before anything runs
    const hfl_voxel_candidate& cd = candidates[k];
    if (cd.cloud < 0 || cd.cloud >= batch || !(cd.voxel > 0.0) || !(cd.voxel <= 1.7976931348623157e308)) return HFL_EINVAL;
    if (cd.nx < 1 || cd.ny < 1 || cd.nz < 1 || cd.nx > HFL_VOXEL_MAX_CELLS || cd.ny > HFL_VOXEL_MAX_CELLS ||
        cd.nz > HFL_VOXEL_MAX_CELLS)
      return HFL_EINVAL;
    const int64_t words = ((int64_t)cd.nx * cd.ny * cd.nz + 31) >> 5;     // < 2^43: no overflow
    if (cd.word_offset < 0 || cd.word_offset > bitmap_words || words > bitmap_words - cd.word_offset) return HFL_EINVAL;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t table_bytes = (int64_t)sizeof(hfl_voxel_candidate) * n_candidates;
  hfl_voxel_candidate* table = static_cast<hfl_voxel_candidate*>(workspace);
  uint32_t* bitmaps = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + align16(table_bytes));
  hipError_t e = hipMemcpyAsync(table, candidates, (size_t)table_bytes, hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return (int)e;
  e = hipMemsetAsync(bitmaps, 0, sizeof(uint32_t) * (size_t)bitmap_words, s);
  if (e != hipSuccess) return (int)e;
  const int64_t groups = hfl_cdiv(max_cloud_points, kOccPointsPerGroup);
  const dim3 grid((unsigned)(groups < kOccMaxGroups ? groups : kOccMaxGroups), (unsigned)n_candidates);
  voxel_occupancy_kernel<<<grid, kVoxThreads, 0, s>>>(bitmaps, table, bounds, points, cloud_offsets, n_points);
  voxel_popcount_kernel<<<n_candidates, kVoxThreads, 0, s>>>(counts, bitmaps, table);
  HFL_RETURN_LAST_ERROR();
}
