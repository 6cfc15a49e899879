// Batch-hard triplet and contrastive losses (reference: models/losses/loss.py:27-135 with pytorch-metric-learning's
// LpDistance(p = 2, power = 1), TripletMarginLoss(swap = True), ContrastiveLoss and AvgNonZeroReducer).
//     mine:   per row a the positive with the largest and the negative with the smallest ||e_a - e_j||, lowest column on ties;
//             the (B, B) distance matrix is never written.
//     terms:  d_pn of the kept rows, the loss terms and their flags (a workgroup per 64 rows), then every count and every sum
//             in one small vector (a second, one-wave launch over the workgroups' partial sums).
//     grad:   dE for unit upstream gradient; a workgroup per embedding row scans the triples in ascending anchor order.
// Every distance is the float hfl_pairwise_dist writes for that entry: one fmaf(diff, diff, acc) chain over k ascending from 0,
// then sqrtf ((a - b)^2 and (b - a)^2 are the same float, zero padding of k leaves the chain alone).  fp32, plain VALU code,
// no float atomics; every output element has one writer and a fixed summation order.  Compiled with -ffp-contract=off: the
// numpy twins (hotformerloc_amd/losses.py) follow the arithmetic operation for operation.
#include "hfl_common.h"

#include <math.h>

namespace {

constexpr int BH_TILE = 64;                   // mine: 64 rows x 64 columns per step, 4 x 4 per thread
constexpr int BH_KC = 32;                     // mine: D-chunk staged in LDS per step
constexpr int BH_LDK = BH_TILE + 4;           // k-major rows of 64 + 4 floats, as in pairwise.hip
constexpr int BH_MAX_SPLITS = 8;              // mine: at most this many workgroups share a band of 64 rows

template <bool VEC>
__device__ __forceinline__ float4 bh_load4(const float* __restrict__ E, int row, int k, int D) {   // row < B checked by the caller
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  const float* p = E + (int64_t)row * D + k;
  if (VEC) {                                                  // D % 4 == 0: k < D implies k + 3 < D, and p is 16-byte aligned
    if (k < D) v = *reinterpret_cast<const float4*>(p);
  } else {
    if (k < D) v.x = p[0];
    if (k + 1 < D) v.y = p[1];
    if (k + 2 < D) v.z = p[2];
    if (k + 3 < D) v.w = p[3];
  }
  return v;
}

// 64 rows x BH_KC columns of E from (row0, k0), zero beyond B and D: thread t holds the float4 (row q / 8, columns 4 (q % 8)..)
// for q = t and t + 256.
template <bool VEC>
__device__ __forceinline__ void bh_load_rows(float4 (&r)[2], const float* __restrict__ E, int row0, int k0, int B, int D) {
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int q = threadIdx.x + 256 * m;
    const int row = row0 + (q >> 3);
    r[m] = row < B ? bh_load4<VEC>(E, row, k0 + (q & 7) * 4, D) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

__device__ __forceinline__ void bh_store_rows(float* __restrict__ s, const float4 (&r)[2]) {      // s[k][row], k-major
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int q = threadIdx.x + 256 * m;
    const int row = q >> 3, k = (q & 7) * 4;
    s[(k + 0) * BH_LDK + row] = r[m].x;
    s[(k + 1) * BH_LDK + row] = r[m].y;
    s[(k + 2) * BH_LDK + row] = r[m].z;
    s[(k + 3) * BH_LDK + row] = r[m].w;
  }
}

// Workgroup (x, y) owns rows [64 y, 64 y + 64) and the column tiles [x tps, (x + 1) tps): per row the hardest positive and
// the hardest negative among those columns, columns ascending with a strict compare, so the lowest column wins a tie.
template <bool VEC>
__global__ void __launch_bounds__(256)
bh_mine_kernel(float* __restrict__ part_pv, int* __restrict__ part_pi, float* __restrict__ part_nv, int* __restrict__ part_ni,
               const float* __restrict__ E, const uint8_t* __restrict__ pos, const uint8_t* __restrict__ neg, int B, int D,
               int tiles, int tps) {
  __shared__ __attribute__((aligned(16))) float smem[2 * BH_KC * BH_LDK];
  float* sA = smem;                                           // [BH_KC][BH_LDK] rows of this band
  float* sB = smem + BH_KC * BH_LDK;                          // rows of the column tile
  const int bi = blockIdx.y, split = blockIdx.x;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int i0 = bi * BH_TILE;
  float pv[4], nv[4];
  int pi[4], ni[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    pv[r] = -1.f;
    nv[r] = INFINITY;
    pi[r] = ni[r] = -1;
  }
  const int t1 = min(tiles, (split + 1) * tps);
  for (int bj = split * tps; bj < t1; ++bj) {
    const int j0 = bj * BH_TILE;
    unsigned pm = 0u, nm = 0u;                                // this thread's 4 x 4 mask bits; the loads fly under the k loop
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int i = i0 + ty * 4 + r, j = j0 + tx * 4 + c;
        if (i < B && j < B) {
          pm |= (pos[(int64_t)i * B + j] != 0 ? 1u : 0u) << (r * 4 + c);
          nm |= (neg[(int64_t)i * B + j] != 0 ? 1u : 0u) << (r * 4 + c);
        }
      }
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
    float4 ra[2], rb[2];
    bh_load_rows<VEC>(ra, E, i0, 0, B, D);
    bh_load_rows<VEC>(rb, E, j0, 0, B, D);
    for (int k0 = 0; k0 < D; k0 += BH_KC) {
      bh_store_rows(sA, ra);
      bh_store_rows(sB, rb);
      __syncthreads();
      if (k0 + BH_KC < D) {                                   // next chunk's loads fly under this chunk's arithmetic
        bh_load_rows<VEC>(ra, E, i0, k0 + BH_KC, B, D);
        bh_load_rows<VEC>(rb, E, j0, k0 + BH_KC, B, D);
      }
#pragma unroll 8
      for (int k = 0; k < BH_KC; ++k) {
        const float4 a4 = *reinterpret_cast<const float4*>(sA + k * BH_LDK + ty * 4);
        const float4 b4 = *reinterpret_cast<const float4*>(sB + k * BH_LDK + tx * 4);
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
      for (int c = 0; c < 4; ++c) {
        const float d = sqrtf(acc[r][c]);
        const int j = j0 + tx * 4 + c;
        if (((pm >> (r * 4 + c)) & 1u) && d > pv[r]) {
          pv[r] = d;
          pi[r] = j;
        }
        if (((nm >> (r * 4 + c)) & 1u) && d < nv[r]) {
          nv[r] = d;
          ni[r] = j;
        }
      }
  }
  // the 16 threads of a row group are 16 consecutive lanes; (value, lowest column) is commutative and associative
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
      const float opv = __shfl_xor(pv[r], m, HFL_WAVE), onv = __shfl_xor(nv[r], m, HFL_WAVE);
      const int opi = __shfl_xor(pi[r], m, HFL_WAVE), oni = __shfl_xor(ni[r], m, HFL_WAVE);
      if (opi >= 0 && (pi[r] < 0 || opv > pv[r] || (opv == pv[r] && opi < pi[r]))) {
        pv[r] = opv;
        pi[r] = opi;
      }
      if (oni >= 0 && (ni[r] < 0 || onv < nv[r] || (onv == nv[r] && oni < ni[r]))) {
        nv[r] = onv;
        ni[r] = oni;
      }
    }
  if (tx == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + ty * 4 + r;
      if (i < B) {
        const int64_t o = (int64_t)split * B + i;
        part_pv[o] = pv[r];
        part_pi[o] = pi[r];
        part_nv[o] = nv[r];
        part_ni[o] = ni[r];
      }
    }
  }
}

// The partial (value, column) pairs of a row, splits (hence columns) ascending with a strict compare.
__global__ void __launch_bounds__(256)
bh_mine_combine_kernel(int* __restrict__ p, float* __restrict__ d_ap, int* __restrict__ n, float* __restrict__ d_an,
                       const float* __restrict__ part_pv, const int* __restrict__ part_pi, const float* __restrict__ part_nv,
                       const int* __restrict__ part_ni, int B, int splits) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  float pv = -1.f, nv = INFINITY;
  int pi = -1, ni = -1;
  for (int s = 0; s < splits; ++s) {
    const int64_t o = (int64_t)s * B + i;
    const int qi = part_pi[o], ri = part_ni[o];
    const float qv = part_pv[o], rv = part_nv[o];
    if (qi >= 0 && qv > pv) {
      pv = qv;
      pi = qi;
    }
    if (ri >= 0 && rv < nv) {
      nv = rv;
      ni = ri;
    }
  }
  p[i] = pi;
  d_ap[i] = pi >= 0 ? pv : 0.f;
  n[i] = ni;
  d_an[i] = ni >= 0 ? nv : 0.f;
}

constexpr int BT_ROWS = 64;                   // terms: rows per workgroup; wave 0 chains d_pn, wave 1 the row norm
constexpr int BT_THREADS = 2 * BT_ROWS;
constexpr int BT_KC = 32;
constexpr int BT_LD = BT_KC + 1;              // odd: a thread per row reads its row conflict-free
constexpr int BT_NRED = 12;                   // per workgroup: 8 sums, then max / min of d_ap, max / min of d_an

__device__ __forceinline__ double bh_wave_sum(double v) {
#pragma unroll
  for (int m = 1; m < HFL_WAVE; m <<= 1) v += __shfl_xor(v, m, HFL_WAVE);
  return v;
}
__device__ __forceinline__ double bh_wave_max(double v) {
#pragma unroll
  for (int m = 1; m < HFL_WAVE; m <<= 1) v = fmax(v, __shfl_xor(v, m, HFL_WAVE));
  return v;
}

// 64 rows x BT_KC columns from k0: e = the rows themselves, d = row p - row n of the kept rows (zero otherwise); thread t holds
// the float4 (row q / 8, columns 4 (q % 8)..) for q = t + 128 m.
template <bool VEC>
__device__ __forceinline__ void bt_load(float4 (&e)[4], float4 (&d)[4], const float* __restrict__ E, const int* sP, const int* sN,
                                        int r0, int k0, int B, int D) {
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int q = threadIdx.x + BT_THREADS * m;
    const int row = q >> 3, k = k0 + (q & 7) * 4;
    e[m] = d[m] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + row < B) e[m] = bh_load4<VEC>(E, r0 + row, k, D);
    const int pr = sP[row];
    if (pr >= 0) {
      const float4 a = bh_load4<VEC>(E, pr, k, D), b = bh_load4<VEC>(E, sN[row], k, D);
      d[m] = make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
    }
  }
}

// Workgroup b owns rows [64 b, 64 b + 64): the p and n rows arrive row-contiguously and their difference is staged in LDS, the
// next chunk's loads in flight under the current chunk's chain; thread t < 64 then runs the d_pn chain of row t and forms its
// terms, thread 64 + t the norm chain of row t.  part[b][.]: the workgroup's float64 sums, by a fixed butterfly.
template <bool VEC>
__global__ void __launch_bounds__(BT_THREADS)
bh_terms_rows_kernel(double* __restrict__ part, float* __restrict__ d_pn, int* __restrict__ flags, const float* __restrict__ E,
                     const int* __restrict__ p, const float* __restrict__ d_ap, const int* __restrict__ n,
                     const float* __restrict__ d_an, int B, int D, int mode, double m0, double m1) {
  __shared__ float sD[BT_ROWS * BT_LD];
  __shared__ float sE[BT_ROWS * BT_LD];
  __shared__ int sP[BT_ROWS], sN[BT_ROWS];
  __shared__ double sRed[BT_NRED];
  const int tid = threadIdx.x, lr = tid & (BT_ROWS - 1);
  const bool norm_half = tid >= BT_ROWS;
  const bool triplet = mode == 0;
  const int r0 = blockIdx.x * BT_ROWS, r = r0 + lr;
  bool kept = false;
  if (!norm_half) {
    const int pp = r < B ? p[r] : -1, nn = r < B ? n[r] : -1;
    kept = pp >= 0 && pp < B && nn >= 0 && nn < B;
    sP[lr] = kept && triplet ? pp : -1;
    sN[lr] = nn;
  }
  __syncthreads();
  float acc = 0.f;
  float4 e[4], d[4];
  bt_load<VEC>(e, d, E, sP, sN, r0, 0, B, D);
  for (int k0 = 0; k0 < D; k0 += BT_KC) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int q = tid + BT_THREADS * m;
      float* se = sE + (q >> 3) * BT_LD + (q & 7) * 4;
      float* sd = sD + (q >> 3) * BT_LD + (q & 7) * 4;
      se[0] = e[m].x; se[1] = e[m].y; se[2] = e[m].z; se[3] = e[m].w;
      sd[0] = d[m].x; sd[1] = d[m].y; sd[2] = d[m].z; sd[3] = d[m].w;
    }
    __syncthreads();
    if (k0 + BT_KC < D) bt_load<VEC>(e, d, E, sP, sN, r0, k0 + BT_KC, B, D);
    const float* s = (norm_half ? sE : sD) + lr * BT_LD;
#pragma unroll 8
    for (int k = 0; k < BT_KC; ++k) acc = fmaf(s[k], s[k], acc);
    __syncthreads();
  }
  const float len = sqrtf(acc);
  double cnt_t = 0., cnt_a = 0., cnt_b = 0., sum_a = 0., sum_b = 0., sum_ap = 0., sum_an = 0., sum_norm = 0.;
  double max_ap = -INFINITY, min_ap = INFINITY, max_an = -INFINITY, min_an = INFINITY;
  if (norm_half) {
    if (r < B) sum_norm = (double)len;
  } else if (r < B) {
    int f = 0;
    if (kept) {
      const float ap = d_ap[r], an = d_an[r];
      cnt_t = 1.;
      sum_ap = max_ap = min_ap = (double)ap;
      sum_an = max_an = min_an = (double)an;
      f = 1;
      if (triplet) {
        const bool swapped = len < an;                        // on an exact tie the anchor-negative pair is differentiated
        const double v = ((double)ap - (double)(swapped ? len : an)) + m0;
        if (v > 0.) {
          f |= 2;
          cnt_a = 1.;
          sum_a = v;
          if (swapped) {
            f |= 4;
            cnt_b = 1.;
          }
        }
      } else {
        const double pt = (double)ap - m0, nt = m1 - (double)an;
        if (pt > 0.) {
          f |= 2;
          cnt_a = 1.;
          sum_a = pt;
        }
        if (nt > 0.) {
          f |= 4;
          cnt_b = 1.;
          sum_b = nt;
        }
      }
    }
    flags[r] = f;
    d_pn[r] = kept && triplet ? len : 0.f;
  }
  // wave 0 holds every term, wave 1 the norms: each reduces what it holds, lane 0 of each writes its share
  if (norm_half) {
    const double v = bh_wave_sum(sum_norm);
    if (lr == 0) sRed[7] = v;
  } else {
    const double red[BT_NRED] = {bh_wave_sum(cnt_t), bh_wave_sum(cnt_a), bh_wave_sum(cnt_b), bh_wave_sum(sum_a),
                                 bh_wave_sum(sum_b), bh_wave_sum(sum_ap), bh_wave_sum(sum_an), 0.,
                                 bh_wave_max(max_ap), -bh_wave_max(-min_ap), bh_wave_max(max_an), -bh_wave_max(-min_an)};
    if (lr == 0) {
#pragma unroll
      for (int s = 0; s < BT_NRED; ++s)
        if (s != 7) sRed[s] = red[s];
    }
  }
  __syncthreads();
  if (tid < BT_NRED) part[(int64_t)blockIdx.x * BT_NRED + tid] = sRed[tid];
}

// One wave: lane l combines the workgroups l, l + 64, .. ascending, then the fixed butterfly; lane 0 writes the vector.
__global__ void __launch_bounds__(HFL_WAVE)
bh_terms_reduce_kernel(double* __restrict__ stats, float* __restrict__ scale, const double* __restrict__ part, int blocks, int B,
                       int mode) {
  double red[BT_NRED];
#pragma unroll
  for (int s = 0; s < BT_NRED; ++s) red[s] = s < 8 ? 0. : (s & 1) ? INFINITY : -INFINITY;
  for (int b = threadIdx.x; b < blocks; b += HFL_WAVE) {
#pragma unroll
    for (int s = 0; s < BT_NRED; ++s) {
      const double v = part[(int64_t)b * BT_NRED + s];
      red[s] = s < 8 ? red[s] + v : (s & 1) ? fmin(red[s], v) : fmax(red[s], v);
    }
  }
#pragma unroll
  for (int s = 0; s < BT_NRED; ++s) red[s] = s < 8 ? bh_wave_sum(red[s]) : (s & 1) ? -bh_wave_max(-red[s]) : bh_wave_max(red[s]);
  if (threadIdx.x != 0) return;
  const bool triplet = mode == 0;
  const double T = red[0], na = red[1], nb = red[2];
  const double mean_a = na > 0. ? red[3] / na : 0., mean_b = nb > 0. ? red[4] / nb : 0.;
  const double loss = triplet ? mean_a : mean_a + mean_b;
  stats[0] = T;
  stats[1] = na;
  stats[2] = nb;
  stats[3] = red[3];
  stats[4] = red[4];
  stats[5] = T > 0. ? red[5] / T : NAN;
  stats[6] = T > 0. ? red[8] : NAN;
  stats[7] = T > 0. ? red[9] : NAN;
  stats[8] = T > 0. ? red[6] / T : NAN;
  stats[9] = T > 0. ? red[10] : NAN;
  stats[10] = T > 0. ? red[11] : NAN;
  stats[11] = red[7] / (double)B;
  stats[12] = loss;
  stats[13] = triplet ? 0. : mean_a;
  stats[14] = triplet ? 0. : mean_b;
  stats[15] = 0.;
  scale[0] = na > 0. ? (float)(1. / na) : 0.f;
  scale[1] = !triplet && nb > 0. ? (float)(1. / nb) : 0.f;
  scale[2] = (float)loss;
  scale[3] = 0.f;
}

constexpr int BG_KM = 4;                      // grad: a thread owns columns t, t + 256, .. of a pass of 1024

// acc_k = fmaf(w, e_i[k] - e_o[k], acc_k) for the columns this thread owns
__device__ __forceinline__ void bg_add(float (&acc)[BG_KM], const float (&ei)[BG_KM], const float* __restrict__ E, int other,
                                       float w, int kb, int D) {
  const float* eo = E + (int64_t)other * D;
#pragma unroll
  for (int m = 0; m < BG_KM; ++m) {
    const int k = kb + threadIdx.x + 256 * m;
    if (k < D) acc[m] = fmaf(w, ei[m] - eo[k], acc[m]);
  }
}

// the pair (x, y) at distance d with derivative c of the loss with respect to d: row i takes part as x, as y or not at all
__device__ __forceinline__ void bg_pair(float (&acc)[BG_KM], const float (&ei)[BG_KM], const float* __restrict__ E, int i,
                                        int x, int y, float c, float d, int kb, int D) {
  if (!(d > 0.f)) return;                                     // coincident rows: no contribution (torch.cdist's convention)
  const float w = c / d;
  if (i == x) bg_add(acc, ei, E, y, w, kb, D);
  if (i == y) bg_add(acc, ei, E, x, w, kb, D);
}

// Workgroup i owns dE[i, :].  The triples are tested 256 at a time, a thread each; the hits are then taken in ascending
// anchor order by the whole workgroup, so that every element sums its addends in one fixed order.
__global__ void __launch_bounds__(256)
bh_grad_kernel(float* __restrict__ dE, const float* __restrict__ E, const int* __restrict__ p, const int* __restrict__ n,
               const float* __restrict__ d_ap, const float* __restrict__ d_an, const float* __restrict__ d_pn,
               const int* __restrict__ flags, const float* __restrict__ scale, int B, int D, int mode) {
  __shared__ unsigned long long sMask[4];
  const int i = blockIdx.x, tid = threadIdx.x;
  const float sa = scale[0], sb = scale[1];
  for (int kb = 0; kb < D; kb += 256 * BG_KM) {
    float ei[BG_KM], acc[BG_KM];
#pragma unroll
    for (int m = 0; m < BG_KM; ++m) {
      const int k = kb + tid + 256 * m;
      ei[m] = k < D ? E[(int64_t)i * D + k] : 0.f;
      acc[m] = 0.f;
    }
    for (int a0 = 0; a0 < B; a0 += 256) {
      const int a = a0 + tid;
      bool hit = false;
      if (a < B) {
        const int f = flags[a];
        hit = (f & 1) && (f & 6) && (a == i || p[a] == i || n[a] == i);
      }
      const unsigned long long mask = __ballot(hit);
      if ((tid & (HFL_WAVE - 1)) == 0) sMask[tid >> 6] = mask;
      __syncthreads();
      for (int w = 0; w < 4; ++w) {
        unsigned long long m = sMask[w];
        while (m != 0ull) {
          const int aa = a0 + w * HFL_WAVE + __builtin_ctzll(m);
          m &= m - 1ull;
          const int f = flags[aa], pa = p[aa], na = n[aa];
          if (pa < 0 || pa >= B || na < 0 || na >= B) continue;
          if (mode == 0) {
            bg_pair(acc, ei, E, i, aa, pa, sa, d_ap[aa], kb, D);
            if (f & 4)
              bg_pair(acc, ei, E, i, pa, na, -sa, d_pn[aa], kb, D);
            else
              bg_pair(acc, ei, E, i, aa, na, -sa, d_an[aa], kb, D);
          } else {
            if (f & 2) bg_pair(acc, ei, E, i, aa, pa, sa, d_ap[aa], kb, D);
            if (f & 4) bg_pair(acc, ei, E, i, aa, na, -sb, d_an[aa], kb, D);
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int m = 0; m < BG_KM; ++m) {
      const int k = kb + tid + 256 * m;
      if (k < D) dE[(int64_t)i * D + k] = acc[m];
    }
  }
}

inline int bh_splits(int tiles, int* tps) {
  *tps = (int)hfl_cdiv(tiles, BH_MAX_SPLITS);
  return (int)hfl_cdiv(tiles, *tps);
}

}  // namespace

extern "C" int64_t hfl_batch_hard_mine_workspace(int batch) {
  if (batch <= 0) return 0;
  int tps;
  const int splits = bh_splits((int)hfl_cdiv(batch, BH_TILE), &tps);
  return (int64_t)splits * batch * 16;
}

extern "C" int hfl_batch_hard_mine(int* p, float* d_ap, int* n, float* d_an, void* workspace, const float* emb,
                                   const uint8_t* pos_mask, const uint8_t* neg_mask, int batch, int dim, hfl_stream_t stream) {
  if (batch <= 0 || dim <= 0 || p == nullptr || d_ap == nullptr || n == nullptr || d_an == nullptr || workspace == nullptr ||
      emb == nullptr || pos_mask == nullptr || neg_mask == nullptr)
    return HFL_EINVAL;
  const int tiles = (int)hfl_cdiv(batch, BH_TILE);
  if (tiles > 65535) return HFL_ECAPACITY;
  int tps;
  const int splits = bh_splits(tiles, &tps);
  const int64_t sb = (int64_t)splits * batch;
  float* part_pv = static_cast<float*>(workspace);
  int* part_pi = reinterpret_cast<int*>(part_pv + sb);
  float* part_nv = part_pv + 2 * sb;
  int* part_ni = reinterpret_cast<int*>(part_pv + 3 * sb);
  const dim3 grid(splits, tiles);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (dim % 4 == 0 && (reinterpret_cast<uintptr_t>(emb) & 15) == 0)
    bh_mine_kernel<true><<<grid, 256, 0, st>>>(part_pv, part_pi, part_nv, part_ni, emb, pos_mask, neg_mask, batch, dim, tiles, tps);
  else
    bh_mine_kernel<false><<<grid, 256, 0, st>>>(part_pv, part_pi, part_nv, part_ni, emb, pos_mask, neg_mask, batch, dim, tiles, tps);
  bh_mine_combine_kernel<<<(unsigned)hfl_cdiv(batch, 256), 256, 0, st>>>(p, d_ap, n, d_an, part_pv, part_pi, part_nv, part_ni,
                                                                        batch, splits);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int64_t hfl_batch_hard_terms_workspace(int batch) {
  return batch <= 0 ? 0 : hfl_cdiv(batch, BT_ROWS) * BT_NRED * (int64_t)sizeof(double);
}

extern "C" int hfl_batch_hard_terms(double* stats, float* scale, float* d_pn, int* flags, void* workspace, const float* emb,
                                    const int* p, const float* d_ap, const int* n, const float* d_an, int batch, int dim,
                                    int mode, double margin0, double margin1, hfl_stream_t stream) {
  if (batch <= 0 || dim <= 0 || (mode != 0 && mode != 1) || stats == nullptr || scale == nullptr || d_pn == nullptr ||
      flags == nullptr || workspace == nullptr || emb == nullptr || p == nullptr || d_ap == nullptr || n == nullptr ||
      d_an == nullptr || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0)
    return HFL_EINVAL;
  const int blocks = (int)hfl_cdiv(batch, BT_ROWS);
  double* part = static_cast<double*>(workspace);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (dim % 4 == 0 && (reinterpret_cast<uintptr_t>(emb) & 15) == 0)
    bh_terms_rows_kernel<true><<<blocks, BT_THREADS, 0, st>>>(part, d_pn, flags, emb, p, d_ap, n, d_an, batch, dim, mode, margin0,
                                                            margin1);
  else
    bh_terms_rows_kernel<false><<<blocks, BT_THREADS, 0, st>>>(part, d_pn, flags, emb, p, d_ap, n, d_an, batch, dim, mode, margin0,
                                                             margin1);
  bh_terms_reduce_kernel<<<1, HFL_WAVE, 0, st>>>(stats, scale, part, blocks, batch, mode);
  HFL_RETURN_LAST_ERROR();
}

extern "C" int hfl_batch_hard_grad(float* d_emb, const float* emb, const int* p, const int* n, const float* d_ap,
                                   const float* d_an, const float* d_pn, const int* flags, const float* scale, int batch, int dim,
                                   int mode, hfl_stream_t stream) {
  if (batch <= 0 || dim <= 0 || (mode != 0 && mode != 1) || d_emb == nullptr || emb == nullptr || p == nullptr || n == nullptr ||
      d_ap == nullptr || d_an == nullptr || d_pn == nullptr || flags == nullptr || scale == nullptr)
    return HFL_EINVAL;
  bh_grad_kernel<<<batch, 256, 0, static_cast<hipStream_t>(stream)>>>(d_emb, emb, p, n, d_ap, d_an, d_pn, flags, scale, batch,
                                                                     dim, mode);
  HFL_RETURN_LAST_ERROR();
}
