// Ground removal for raw submaps by the Cloth Simulation Filter (Zhang et al. 2016), batched and ragged on the device: the
// first link of the CS-Wild-Places post-processing (datasets/CSWildPlaces/postprocess_submaps.py --remove_ground).  The
// filter is DEFINED in hotformerloc_amd/ground.py (module docstring) and DESIGN.md section 7f; this file and the numpy route
// there follow that definition operation for operation in fp32, every operation rounded once (the file is built with
// -ffp-contract=off), so the two agree to the bit.
//
//   hfl_cloth_raster    one 64-bit integer atomic min per point on (bits of the squared horizontal distance << 32 | the
//                       point's index in its cloud), then one thread per particle reads the winner's -z or fills an empty
//                       particle from the rastered ones (row, then column, then nearest)
//   hfl_cloth_simulate  one workgroup of 1024 lanes per cloud; u, u_prev, t and the movable flags stay in LDS for all steps
//                       and for the slope smoothing.  A step is 34 workgroup barriers (Verlet, 2 x 16 constraint sub-passes
//                       of disjoint pairs, the reduction of the largest move); the run is bound by them, not by arithmetic
//   hfl_cloth_classify  per point the bilinear cloth height and the non-ground mask
//
// No floating-point atomics.  No workgroup waits for another.  Every barrier is reached by the whole workgroup: the loop
// conditions are read from LDS by every lane, so all lanes leave a loop together.
#include "ragged_common.h"

namespace {

constexpr int kGroundThreads = 256;
constexpr int kSimThreads = 1024;
constexpr int kSimWaves = kSimThreads / 64;
constexpr int kSimSlots = HFL_CLOTH_MAX_PARTICLES / kSimThreads;      // particles per lane
static_assert(kSimSlots * kSimThreads == HFL_CLOTH_MAX_PARTICLES, "the particle limit is a multiple of the workgroup");
constexpr unsigned long long kNoPoint = ~0ull;

// int(f) clamped into [0, top]; a NaN gives 0 (the host route: where(f >= 0, f, 0), minimum(f, top), truncate)
__device__ __forceinline__ int cloth_index(float f, int top) {
  if (!(f >= 0.f)) return 0;
  if (f >= (float)top) return top;
  return (int)f;
}

// (p - origin) / r
__device__ __forceinline__ float cloth_coord(float p, float origin, float r) {
  return __fdiv_rn(__fsub_rn(p, origin), r);
}

__global__ void __launch_bounds__(kGroundThreads)
cloth_raster_kernel(unsigned long long* __restrict__ keys, const hfl_cloth_desc* __restrict__ desc,
                    const float* __restrict__ pts, const int64_t* __restrict__ off, int batch, int64_t n, float r) {
  const int64_t i = (int64_t)blockIdx.x * kGroundThreads + threadIdx.x;
  if (i >= n) return;
  const int c = find_cloud(off, batch, i);
  const hfl_cloth_desc d = desc[c];
  const float x = pts[i * 3 + 0], y = pts[i * 3 + 1];
  const int col = cloth_index(__fadd_rn(cloth_coord(x, d.ox, r), 0.5f), d.width - 1);
  const int row = cloth_index(__fadd_rn(cloth_coord(y, d.oy, r), 0.5f), d.height - 1);
  const float dx = __fsub_rn(x, __fadd_rn(d.ox, __fmul_rn((float)col, r)));
  const float dy = __fsub_rn(y, __fadd_rn(d.oy, __fmul_rn((float)row, r)));
  const float d2 = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));      // >= +0: its bits order as the values do
  const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)(uint32_t)(i - off[c]);
  unsigned long long* slot = keys + d.cell_offset + (int64_t)row * d.width + col;
  if (key < *reinterpret_cast<volatile unsigned long long*>(slot)) atomicMin(slot, key);   // most points lose: test first
}

// t of every particle: -z of the rastered point, or of the rastered particle the definition names for an empty one
__global__ void __launch_bounds__(kGroundThreads)
cloth_fill_kernel(float* __restrict__ t, const unsigned long long* __restrict__ keys, const hfl_cloth_desc* __restrict__ desc,
                  const float* __restrict__ pts, const int64_t* __restrict__ off) {
  const int c = blockIdx.y;
  const hfl_cloth_desc d = desc[c];
  const int W = d.width, H = d.height;
  const int k = blockIdx.x * kGroundThreads + threadIdx.x;
  if (k >= W * H) return;
  const unsigned long long* K = keys + d.cell_offset;
  const int i = k % W, j = k / W;
  int src = -1;
  if (K[k] != kNoPoint) src = k;
  for (int a = i + 1; src < 0 && a < W; ++a)
    if (K[j * W + a] != kNoPoint) src = j * W + a;
  for (int a = i - 1; src < 0 && a >= 0; --a)
    if (K[j * W + a] != kNoPoint) src = j * W + a;
  for (int b = j - 1; src < 0 && b >= 0; --b)
    if (K[b * W + i] != kNoPoint) src = b * W + i;
  for (int b = j + 1; src < 0 && b < H; ++b)
    if (K[b * W + i] != kNoPoint) src = b * W + i;
  if (src < 0) {                                             // the row and the column are empty: the nearest rastered one
    int best = 0x7fffffff;
    for (int b = 0; b < H; ++b)
      for (int a = 0; a < W; ++a) {
        const int dist = (a - i) * (a - i) + (b - j) * (b - j);
        if (dist < best && K[b * W + a] != kNoPoint) { best = dist; src = b * W + a; }
      }
  }
  float v = 0.f;
  if (src >= 0) {
    const int64_t idx = (int64_t)(K[src] & 0xffffffffull);
    if (idx < off[c + 1] - off[c]) v = -pts[(off[c] + idx) * 3 + 2];
  }
  t[d.cell_offset + k] = v;
}

// the eight constraint offsets in the order of the definition
__constant__ int kOffDx[8] = {1, 0, 1, 1, 2, 0, 2, 2};
__constant__ int kOffDy[8] = {0, 1, 1, -1, 0, 2, 2, -2};

struct SimReduce {
  float move[2][kSimWaves];
  int flag[2][kSimWaves];
};

// (largest `move`, any `flag`) over the workgroup, the same in every lane; one barrier.  `parity` alternates between calls:
// a slot written here is read before the barrier of the next call, and written again only after it
__device__ __forceinline__ void sim_reduce(SimReduce& red, int& parity, float& move, int& flag) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) move = fmaxf(move, __shfl_xor(move, m, 64));
  const int any = __ballot(flag != 0) != 0ull ? 1 : 0;
  if (lane == 0) { red.move[parity][wave] = move; red.flag[parity][wave] = any; }
  __syncthreads();
  float mm = red.move[parity][0];
  int ff = red.flag[parity][0];
#pragma unroll
  for (int w = 1; w < kSimWaves; ++w) { mm = fmaxf(mm, red.move[parity][w]); ff |= red.flag[parity][w]; }
  move = mm;
  flag = ff;
  parity ^= 1;
}

__global__ void __launch_bounds__(kSimThreads)
cloth_simulate_kernel(float* __restrict__ u_out, uint8_t* __restrict__ movable_out, int32_t* __restrict__ steps_out,
                      const float* __restrict__ t_in, const hfl_cloth_desc* __restrict__ desc, int capacity, float f1,
                      float f2, float gravity, float keep, float stop_move, float smooth_threshold, int iterations,
                      int smooth) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ SimReduce red;
  const hfl_cloth_desc d = desc[blockIdx.x];
  const int W = d.width, H = d.height, n = W * H;
  if (W < 2 || H < 2 || n > capacity || capacity > HFL_CLOTH_MAX_PARTICLES) {      // uniform; the host refuses these first
    if (threadIdx.x == 0) steps_out[blockIdx.x] = -1;
    return;
  }
  float* u = reinterpret_cast<float*>(smem);
  float* up = u + capacity;
  float* t = up + capacity;
  uint8_t* mv = reinterpret_cast<uint8_t*>(t + capacity);
  const int tid = threadIdx.x;

  int ij[kSimSlots];                                         // j << 16 | i of this lane's particles tid + s * 1024
#pragma unroll
  for (int s = 0; s < kSimSlots; ++s) {
    const int idx = tid + s * kSimThreads;
    ij[s] = 0;
    if (idx < n) {
      ij[s] = ((idx / W) << 16) | (idx % W);
      u[idx] = d.u0;
      up[idx] = d.u0;
      t[idx] = t_in[d.cell_offset + idx];
      mv[idx] = 1;
    }
  }
  __syncthreads();

  int parity = 0, steps = 0;
  for (int it = 0; it < iterations; ++it) {
    // (a) Verlet
#pragma unroll
    for (int s = 0; s < kSimSlots; ++s) {
      const int idx = tid + s * kSimThreads;
      if (idx < n && mv[idx]) {
        const float cur = u[idx];
        const float nw = __fadd_rn(__fadd_rn(cur, __fmul_rn(__fsub_rn(cur, up[idx]), keep)), gravity);
        up[idx] = cur;
        u[idx] = nw;
      }
    }
    __syncthreads();
    // (b) two sweeps of 16 sub-passes; the pairs of a sub-pass share no particle
    for (int pass = 0; pass < 32; ++pass) {
      const int o = (pass >> 1) & 7, cls = pass & 1;
      const int dx = kOffDx[o], dy = kOffDy[o];
      const int shift = (dx != 0 ? dx : dy) - 1;             // i // 1, i // 2, j // 1 or j // 2
#pragma unroll
      for (int s = 0; s < kSimSlots; ++s) {
        const int p = tid + s * kSimThreads;
        const int i = ij[s] & 0xffff, j = ij[s] >> 16;
        const int sel = (dx != 0 ? i : j) >> shift;
        if (p < n && (sel & 1) == cls && i + dx < W && j + dy >= 0 && j + dy < H) {
          const int q = p + dy * W + dx;
          const float a = u[p], b = u[q];
          const bool mp = mv[p] != 0, mq = mv[q] != 0;
          const float dd = __fsub_rn(b, a);
          if (mp && mq) {
            const float m = __fmul_rn(f2, dd);
            u[p] = __fadd_rn(a, m);
            u[q] = __fsub_rn(b, m);
          } else if (mp) {
            u[p] = __fadd_rn(a, __fmul_rn(f1, dd));
          } else if (mq) {
            u[q] = __fsub_rn(b, __fmul_rn(f1, dd));
          }
        }
      }
      __syncthreads();
    }
    // (c) the largest move of a movable particle, (d) collision
    float move = 0.f;
    int movable = 0;
#pragma unroll
    for (int s = 0; s < kSimSlots; ++s) {
      const int idx = tid + s * kSimThreads;
      if (idx < n && mv[idx]) {
        const float cur = u[idx], ground = t[idx];
        move = fmaxf(move, fabsf(__fsub_rn(cur, up[idx])));
        if (cur < ground) {
          u[idx] = ground;
          mv[idx] = 0;
        } else {
          movable = 1;
        }
      }
    }
    sim_reduce(red, parity, move, movable);
    steps = it + 1;
    if ((move != 0.f && move < stop_move) || movable == 0) break;      // the same in every lane
  }

  if (smooth) {
    for (;;) {
      unsigned take = 0u;
#pragma unroll
      for (int s = 0; s < kSimSlots; ++s) {
        const int p = tid + s * kSimThreads;
        if (p < n && mv[p]) {
          const int i = ij[s] & 0xffff, j = ij[s] >> 16;
          const float tp = t[p];
          if (fabsf(__fsub_rn(u[p], tp)) < smooth_threshold) {
            bool hit = false;
            if (i > 0 && !mv[p - 1] && fabsf(__fsub_rn(tp, t[p - 1])) < smooth_threshold) hit = true;
            if (i + 1 < W && !mv[p + 1] && fabsf(__fsub_rn(tp, t[p + 1])) < smooth_threshold) hit = true;
            if (j > 0 && !mv[p - W] && fabsf(__fsub_rn(tp, t[p - W])) < smooth_threshold) hit = true;
            if (j + 1 < H && !mv[p + W] && fabsf(__fsub_rn(tp, t[p + W])) < smooth_threshold) hit = true;
            if (hit) take |= 1u << s;
          }
        }
      }
      __syncthreads();                                       // every lane has read the flags of this round
#pragma unroll
      for (int s = 0; s < kSimSlots; ++s) {
        const int p = tid + s * kSimThreads;
        if (take & (1u << s)) {
          u[p] = t[p];
          mv[p] = 0;
        }
      }
      float unused = 0.f;
      int changed = take != 0u ? 1 : 0;
      sim_reduce(red, parity, unused, changed);
      if (!changed) break;                                   // the same in every lane
    }
  }

#pragma unroll
  for (int s = 0; s < kSimSlots; ++s) {
    const int idx = tid + s * kSimThreads;
    if (idx < n) {
      u_out[d.cell_offset + idx] = u[idx];
      movable_out[d.cell_offset + idx] = mv[idx];
    }
  }
  if (tid == 0) steps_out[blockIdx.x] = steps;
}

__global__ void __launch_bounds__(kGroundThreads)
cloth_classify_kernel(uint8_t* __restrict__ keep, const float* __restrict__ u, const hfl_cloth_desc* __restrict__ desc,
                      const float* __restrict__ pts, const int64_t* __restrict__ off, int batch, int64_t n, float r,
                      float threshold) {
  const int64_t i = (int64_t)blockIdx.x * kGroundThreads + threadIdx.x;
  if (i >= n) return;
  const int cl = find_cloud(off, batch, i);
  const hfl_cloth_desc d = desc[cl];
  const int W = d.width;
  const float fx = cloth_coord(pts[i * 3 + 0], d.ox, r), fy = cloth_coord(pts[i * 3 + 1], d.oy, r);
  const int c = cloth_index(fx, W - 2), w = cloth_index(fy, d.height - 2);
  const float tx = __fsub_rn(fx, (float)c), ty = __fsub_rn(fy, (float)w);
  const float sx = __fsub_rn(1.f, tx), sy = __fsub_rn(1.f, ty);
  const float* g = u + d.cell_offset + (int64_t)w * W + c;
  float h = __fmul_rn(__fmul_rn(g[0], sx), sy);
  h = __fadd_rn(h, __fmul_rn(__fmul_rn(g[W], sx), ty));
  h = __fadd_rn(h, __fmul_rn(__fmul_rn(g[W + 1], tx), ty));
  h = __fadd_rn(h, __fmul_rn(__fmul_rn(g[1], tx), sy));
  const bool ground = fabsf(__fsub_rn(-pts[i * 3 + 2], h)) < threshold;
  keep[i] = ground ? 0 : 1;
}

// every cloth inside the particle arrays and under the limit, before anything runs; the largest cloth through `largest`
bool cloth_table_ok(const hfl_cloth_desc* descs, int batch, int64_t n_cells, int* largest) {
  int big = 0;
  for (int b = 0; b < batch; ++b) {
    const hfl_cloth_desc& d = descs[b];
    if (d.width < 2 || d.height < 2 || d.width > HFL_CLOTH_MAX_PARTICLES || d.height > HFL_CLOTH_MAX_PARTICLES) return false;
    const int64_t cells = (int64_t)d.width * d.height;
    if (cells > HFL_CLOTH_MAX_PARTICLES) return false;
    if (d.cell_offset < 0 || d.cell_offset > n_cells || cells > n_cells - d.cell_offset) return false;
    if (!(d.ox - d.ox == 0.f) || !(d.oy - d.oy == 0.f) || !(d.u0 - d.u0 == 0.f)) return false;      // finite
    if (cells > big) big = (int)cells;
  }
  *largest = big;
  return true;
}

bool cloth_batch_ok(int batch, int64_t n_points, int64_t n_cells) {
  return batch >= 1 && n_points >= batch && n_cells >= 1;
}

}  // namespace

extern "C" int hfl_cloth_raster(float* terrain, uint64_t* keys, const hfl_cloth_desc* descs_host,
                                const hfl_cloth_desc* descs, int batch, int64_t n_cells, const float* points,
                                const int64_t* cloud_offsets, int64_t n_points, float resolution, hfl_stream_t stream) {
  if (terrain == nullptr || keys == nullptr || descs_host == nullptr || descs == nullptr || points == nullptr ||
      cloud_offsets == nullptr)
    return HFL_EINVAL;
  if (!cloth_batch_ok(batch, n_points, n_cells) || !(resolution > 0.f) || !(resolution <= 3.4028234e38f)) return HFL_EINVAL;
  if (batch > HFL_VOXEL_MAX_CLOUDS || n_points > HFL_VOXEL_MAX_POINTS) return HFL_ECAPACITY;
  int largest = 0;
  if (!cloth_table_ok(descs_host, batch, n_cells, &largest)) return HFL_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(keys, 0xff, sizeof(uint64_t) * (size_t)n_cells, s);
  if (e != hipSuccess) return (int)e;
  cloth_raster_kernel<<<(unsigned)hfl_cdiv(n_points, kGroundThreads), kGroundThreads, 0, s>>>(
      reinterpret_cast<unsigned long long*>(keys), descs, points, cloud_offsets, batch, n_points, resolution);
  const dim3 grid((unsigned)hfl_cdiv(largest, kGroundThreads), (unsigned)batch);
  cloth_fill_kernel<<<grid, kGroundThreads, 0, s>>>(terrain, reinterpret_cast<const unsigned long long*>(keys), descs, points,
                                                    cloud_offsets);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int hfl_cloth_simulate(float* heights, uint8_t* movable, int32_t* steps_run, const float* terrain,
                                  const hfl_cloth_desc* descs_host, const hfl_cloth_desc* descs, int batch, int64_t n_cells,
                                  float f_one, float f_two, float gravity_step, float velocity_keep, int iterations,
                                  int slope_smooth, hfl_stream_t stream) {
  if (heights == nullptr || movable == nullptr || steps_run == nullptr || terrain == nullptr || descs_host == nullptr ||
      descs == nullptr)
    return HFL_EINVAL;
  if (batch < 1 || n_cells < 1 || iterations < 0) return HFL_EINVAL;
  if (batch > HFL_VOXEL_MAX_CLOUDS) return HFL_ECAPACITY;
  int largest = 0;
  if (!cloth_table_ok(descs_host, batch, n_cells, &largest)) return HFL_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int capacity = (largest + 3) & ~3;                   // the byte flags start on a float boundary
  const size_t lds = (size_t)capacity * (3 * sizeof(float) + 1);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(cloth_simulate_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return (int)e;
  cloth_simulate_kernel<<<batch, kSimThreads, lds, s>>>(heights, movable, steps_run, terrain, descs, capacity, f_one, f_two,
                                                        gravity_step, velocity_keep, 0.005f, 0.3f, iterations,
                                                        slope_smooth ? 1 : 0);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int hfl_cloth_classify(uint8_t* keep, const float* heights, const hfl_cloth_desc* descs_host,
                                  const hfl_cloth_desc* descs, int batch, int64_t n_cells, const float* points,
                                  const int64_t* cloud_offsets, int64_t n_points, float resolution, float threshold,
                                  hfl_stream_t stream) {
  if (keep == nullptr || heights == nullptr || descs_host == nullptr || descs == nullptr || points == nullptr ||
      cloud_offsets == nullptr)
    return HFL_EINVAL;
  if (!cloth_batch_ok(batch, n_points, n_cells) || !(resolution > 0.f) || !(resolution <= 3.4028234e38f)) return HFL_EINVAL;
  if (batch > HFL_VOXEL_MAX_CLOUDS || n_points > HFL_VOXEL_MAX_POINTS) return HFL_ECAPACITY;
  int largest = 0;
  if (!cloth_table_ok(descs_host, batch, n_cells, &largest)) return HFL_EINVAL;
  cloth_classify_kernel<<<(unsigned)hfl_cdiv(n_points, kGroundThreads), kGroundThreads, 0, static_cast<hipStream_t>(stream)>>>(
      keep, heights, descs, points, cloud_offsets, batch, n_points, resolution, threshold);
  HFL_RETURN_LAST_ERROR();
}
