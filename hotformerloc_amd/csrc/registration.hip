// Rigid ICP, point-to-point, point-to-plane and generalized, for a ragged batch of P (source, target) pairs: the definition is
// in hotformerloc_amd/registration.py and DESIGN.md sections 7i, 7j and 7r.  The layout is that of overlap.hip: the points of
// all clouds concatenated as (N, 3) fp32 with (P + 1) int64 offsets.  One iteration is two launches, and a whole batch runs
// to convergence without a host read: the state of a pair lives in two plain device arrays,
//     state  (P, 16) float64: the pose as a row-major 3 x 4 (R | t), fitness, rmse, previous fitness, previous rmse
//     istate (P, 2)  int32:   iterations, status (HFL_ICP_RUNNING .. HFL_ICP_DEGENERATE).
//
// hfl_icp_correspond: hfl_nn_dist with the transform in front of it and the reduction behind it.  A workgroup of 256 threads
// owns RG_ROWS consecutive source rows of one pair (the tile table of hfl_nn_dist).  A pair that is no longer RUNNING makes
// its workgroups return at once.  Otherwise the workgroup rounds the pair's float64 pose to fp32, moves its rows by
// `rigid_coord` and scans the pair's target cloud by `pair_scan3`, both of pair_scan.h and both what hfl_transform_points
// and hfl_nn_dist run (so dist and idx have the bits of hfl_nn_dist on the transformed cloud), reads the winner's
// coordinates from global memory once the scan is over, and sums over its inlier rows (d <= max_dist in fp32) the 17
// float64 quantities
//     n, Sp (3), Sq (3), Spq (9, row-major: p' down, q across), sum d^2         p' the moved source point, q its target.
// The row step and the reduction, and with them the order of every addition, are those of icp_sums.h, which hfl_ransac_sums
// (csrc/global_registration.hip) runs as well.  The result is row blockIdx.x of the (n_tiles, 17) partials.
//
// hfl_icp_solve: one wave per pair.  Lanes 0 .. 16 add the pair's tile partials in ascending tile order, one quantity each;
// lane 0 then applies the stop rules, solves for the rigid update and composes the pose, all in float64.  The solve is a
// one-sided cyclic Jacobi on H = Spq - Sp Sq^T / n with a fixed number of sweeps: column pairs (0,1), (0,2), (1,2) of G = H V
// are rotated until they are orthogonal, the column norms are the singular values, G's normalised columns are U.  With u1, u2
// and v1, v2 the columns of the two largest singular values,
//     R = v1 u1^T + v2 u2^T + (v1 x v2) (u1 x u2)^T,
// which is V diag(1, 1, det(V U^T)) U^T without ever dividing by the smallest singular value: det R = +1 whether or not the
// unconstrained optimum is a reflection, and a planar cloud needs no special case.
//
// hfl_icp_correspond_plane / hfl_icp_solve_plane: the point-to-plane estimator, the same two kernels
// instantiated with PLANE.  The scan, dist, idx and the inlier rule are the same code; the winner's normal nq is read from
// global memory beside its coordinates, and the sums are the 29 float64 quantities
//     n, sum d^2, g = sum J r (6), the upper triangle of A = sum J J^T row-major (21),   r = (p' - q) . nq, J = (p' x nq, nq),
// reduced in the same order.  The solve factorises A = L D L^T without pivoting in a fixed order, solves A x = -g for
// x = (alpha, beta, gamma, tx, ty, tz) and builds R = Rz(gamma) Ry(beta) Rx(alpha): det R = +1 by construction.
//
// hfl_icp_correspond_generalized: the generalized (plane-to-plane) estimator, the third instantiation
// of the correspondence kernel.  The row's source normal is loaded beside the point and turned by the fp32 rotation already
// in registers (no translation, no renormalisation); the winner's normal is gathered as PLANE gathers it.  Per inlier row, in
// float64 with every operation rounded once (`icp_generalized_row`): C = 2 I - (1 - eps)(a a^T + b b^T), M = C^-1 by the
// adjugate over the determinant, r = p' - q, J = (-[p']x | I), and the same 29 sums in the same layout,
//     n, sum d^2, g = sum J^T M r (6), the upper triangle of A = sum J^T M J row-major (21),
// which hfl_icp_solve_plane solves as it stands: with M = nq nq^T they are the point-to-plane sums.
//
// No atomics; every output element has one writer and a fixed evaluation order: two runs give the same bits.
#include <math.h>

#include "icp_sums.h"
#include "kabsch.h"
#include "pair_scan.h"

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_ROWS = HFL_OVERLAP_ROWS;                        // source rows of a workgroup
constexpr int RG_QPT = RG_ROWS / RG_THREADS;                     // source points a thread keeps in registers
constexpr int RG_TILE = HFL_OVERLAP_TILE;                        // target points of an LDS tile
constexpr int RG_SUMS = HFL_ICP_SUMS;
constexpr int RG_PLANE_SUMS = HFL_ICP_PLANE_SUMS;
constexpr int RG_WAVES = RG_THREADS / HFL_WAVE;
constexpr double RG_PIVOT_TOL = 1e-12;                           // a pivot of the LDL^T <= this x its diagonal entry: degenerate
static_assert(RG_ROWS % RG_THREADS == 0 && RG_QPT >= 1, "whole source points per thread");
// 3 x 2048 x 4 B = 24 KiB of static LDS, the planes of the scan; the wave results of the reduction reuse the x plane
static_assert(RG_TILE % 4 == 0 && RG_TILE * 12 <= 32 * 1024, "static LDS stays at 32 KiB or less");
static_assert(RG_WAVES * RG_SUMS * sizeof(double) <= RG_TILE * sizeof(float), "the wave results fit the x plane");
static_assert(RG_WAVES * RG_PLANE_SUMS * sizeof(double) <= RG_TILE * sizeof(float), "the wave results fit the x plane");
static_assert(RG_SUMS == 17, "n, Sp, Sq, Spq, sum d^2");
static_assert(RG_PLANE_SUMS == 29, "n, sum d^2, g, the upper triangle of A");

enum { RG_POINT = 0, RG_PLANE = 1, RG_GENERALIZED = 2 };          // the estimator a correspondence kernel sums for

// One inlier row of the generalized sums, in this statement order with every operation rounded once (no contraction: the
// products of M are not exact, and the host route rounds each).  p, q: the moved source point and its target; a: the moved
// source normal; b: the target's normal; all fp32 values widened, a zero normal leaves its cloud's covariance the identity.
// keep = 1 - epsilon.  C = 2 I - keep (a a^T + b b^T) has its eigenvalues in [2 epsilon, 2] for unit or zero normals, so the
// determinant is positive and the reciprocal finite.
__device__ __forceinline__ void icp_generalized_row(double (&acc)[HFL_ICP_PLANE_SUMS], const double (&p)[3],
                                                    const double (&q)[3], const double (&a)[3], const double (&b)[3], double dd,
                                                    double keep) {
#pragma clang fp contract(off)
  const double c00 = 2.0 - keep * (a[0] * a[0] + b[0] * b[0]), c11 = 2.0 - keep * (a[1] * a[1] + b[1] * b[1]),
               c22 = 2.0 - keep * (a[2] * a[2] + b[2] * b[2]);
  const double c01 = -(keep * (a[0] * a[1] + b[0] * b[1])), c02 = -(keep * (a[0] * a[2] + b[0] * b[2])),
               c12 = -(keep * (a[1] * a[2] + b[1] * b[2]));
  // the adjugate (cofactors of a symmetric matrix), the determinant along the first row, one reciprocal
  const double k00 = c11 * c22 - c12 * c12, k01 = c02 * c12 - c01 * c22, k02 = c01 * c12 - c02 * c11;
  const double k11 = c00 * c22 - c02 * c02, k12 = c01 * c02 - c00 * c12, k22 = c00 * c11 - c01 * c01;
  const double rcp = 1.0 / ((c00 * k00 + c01 * k01) + c02 * k02);
  double m[3][3];
  m[0][0] = k00 * rcp, m[1][1] = k11 * rcp, m[2][2] = k22 * rcp;
  m[0][1] = m[1][0] = k01 * rcp, m[0][2] = m[2][0] = k02 * rcp, m[1][2] = m[2][1] = k12 * rcp;
  const double r[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
  double w[3];                                                   // M r
#pragma unroll
  for (int i = 0; i < 3; ++i) w[i] = (m[i][0] * r[0] + m[i][1] * r[1]) + m[i][2] * r[2];
  acc[0] = acc[0] + 1.0;
  acc[1] = acc[1] + dd * dd;
  int slot = 8;
#pragma unroll
  for (int i = 0; i < 3; ++i) {                                  // rows 0 .. 2 of J^T: row i of [p]x
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
    acc[2 + i] = acc[2 + i] + (p[i1] * w[i2] - p[i2] * w[i1]);   // (p x M r)_i
    acc[5 + i] = acc[5 + i] + w[i];
    double t[3];                                                 // row i of [p]x M: (p x column j of M)_i
#pragma unroll
    for (int j = 0; j < 3; ++j) t[j] = p[i1] * m[i2][j] - p[i2] * m[i1][j];
#pragma unroll
    for (int j = i; j < 3; ++j) {                                // row i of [p]x M [p]x^T from the diagonal on
      const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      acc[slot] = acc[slot] + (p[j1] * t[j2] - p[j2] * t[j1]);
      ++slot;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      acc[slot] = acc[slot] + t[j];
      ++slot;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j) {
      acc[slot] = acc[slot] + m[i][j];
      ++slot;
    }
}

// six waves per SIMD, the residency of nn_dist_kernel (six workgroups of 24 KiB per CU): 80 VGPRs, which the reduction's 17
// float64 sums beside the gathered coordinates would otherwise exceed by two.  PLANE is the point-to-plane estimator: the
// same scan, the winner's normal gathered beside its coordinates, 29 sums; those do not fit 80 VGPRs, so that instantiation
// asks for four waves per SIMD.  RG_GENERALIZED keeps the same scan, the row's moved source normal beside its point, both
// normals and `icp_generalized_row` behind the scan, and the 29 sums; it asks for four waves per SIMD as well.
template <int EST>
__global__ void __launch_bounds__(RG_THREADS) __attribute__((amdgpu_waves_per_eu(EST != RG_POINT ? 4 : 6)))
icp_correspond_kernel(double* __restrict__ partials, float* __restrict__ dist, int32_t* __restrict__ idx,
                      const float* __restrict__ source, const int64_t* __restrict__ s_off, int64_t n_source,
                      const float* __restrict__ targets, const float* __restrict__ t_normals,
                      const int64_t* __restrict__ t_off, int64_t n_targets, const int64_t* __restrict__ tiles,
                      const double* __restrict__ state, const int32_t* __restrict__ istate, float max_dist, int n_pairs,
                      const float* __restrict__ s_normals, double epsilon) {   // the last two: RG_GENERALIZED alone
  constexpr bool PLANE = EST == RG_PLANE, GENERALIZED = EST == RG_GENERALIZED;
  constexpr int NS = EST != RG_POINT ? RG_PLANE_SUMS : RG_SUMS;
  __shared__ __align__(16) float s_x[RG_TILE], s_y[RG_TILE], s_z[RG_TILE];
  PairTile w;
  if (!pair_tile(w, tiles, n_pairs)) return;
  if (istate[2 * w.pair + 1] != HFL_ICP_RUNNING) return;         // the pair has stopped: its partials are not read again
  pair_ranges(w, s_off, n_source, t_off, n_targets);
  const int64_t t_begin = w.t_begin;
  float m[12];                                                   // the pose, rounded once to fp32
#pragma unroll
  for (int k = 0; k < 12; ++k) m[k] = (float)state[16 * w.pair + k];

  float qx[RG_QPT], qy[RG_QPT], qz[RG_QPT], best[RG_QPT];
  constexpr int NQ = GENERALIZED ? RG_QPT : 1;
  float ax[NQ], ay[NQ], az[NQ];                                  // the moved source normals (RG_GENERALIZED alone)
  int32_t at[RG_QPT];
#pragma unroll
  for (int r = 0; r < RG_QPT; ++r) {
    const int64_t row = w.row<RG_THREADS>(r);
    const bool valid = row < w.q_end;
    const float x = valid ? source[3 * row] : 0.f, y = valid ? source[3 * row + 1] : 0.f, z = valid ? source[3 * row + 2] : 0.f;
    qx[r] = rigid_coord(m, x, y, z);
    qy[r] = rigid_coord(m + 4, x, y, z);
    qz[r] = rigid_coord(m + 8, x, y, z);
    if constexpr (GENERALIZED) {                                 // R n: rigid_coord without the translation
      const float u = valid ? s_normals[3 * row] : 0.f, v = valid ? s_normals[3 * row + 1] : 0.f,
                  t = valid ? s_normals[3 * row + 2] : 0.f;
      ax[r] = fmaf(m[2], t, fmaf(m[1], v, m[0] * u));
      ay[r] = fmaf(m[6], t, fmaf(m[5], v, m[4] * u));
      az[r] = fmaf(m[10], t, fmaf(m[9], v, m[8] * u));
    }
  }
  const double keep = 1.0 - epsilon;
  pair_scan3<RG_THREADS>(w, targets, s_x, s_y, s_z, qx, qy, qz, best, at);

  double acc[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) acc[k] = 0.0;
#pragma unroll
  for (int r = 0; r < RG_QPT; ++r) {                             // a thread's rows in row order
    const int64_t row = w.row<RG_THREADS>(r);
    if (row < w.q_end) {
      const float d = pair_sqrt(best[r]);                        // +inf: an empty target cloud
      if (dist != nullptr) dist[row] = d;
      if (idx != nullptr) idx[row] = at[r];
      if (at[r] >= 0 && d <= max_dist) {                         // 0 <= at < t_end - t_begin: the gather stays in the cloud
        const float* w = targets + 3 * (t_begin + at[r]);
        const double pc[3] = {(double)qx[r], (double)qy[r], (double)qz[r]};
        const double qc[3] = {(double)w[0], (double)w[1], (double)w[2]};
        const double dd = (double)d;
        if constexpr (PLANE) {
          // the normal at the winner, read once per source row; r, a = p' x n and J = (a, n) with every operation rounded
          // once, so the rows are the host route's to the bit and only the order of the sums differs
          const float* v = t_normals + 3 * (t_begin + at[r]);
          const double nc[3] = {(double)v[0], (double)v[1], (double)v[2]};
          const double res = __dadd_rn(__dadd_rn(__dmul_rn(__dsub_rn(pc[0], qc[0]), nc[0]),
                                                 __dmul_rn(__dsub_rn(pc[1], qc[1]), nc[1])),
                                       __dmul_rn(__dsub_rn(pc[2], qc[2]), nc[2]));
          const double jac[6] = {__dsub_rn(__dmul_rn(pc[1], nc[2]), __dmul_rn(pc[2], nc[1])),
                                 __dsub_rn(__dmul_rn(pc[2], nc[0]), __dmul_rn(pc[0], nc[2])),
                                 __dsub_rn(__dmul_rn(pc[0], nc[1]), __dmul_rn(pc[1], nc[0])), nc[0], nc[1], nc[2]};
          acc[0] += 1.0;
          acc[1] += dd * dd;
          int slot = 8;
#pragma unroll
          for (int a = 0; a < 6; ++a) {
            acc[2 + a] += jac[a] * res;
#pragma unroll
            for (int b = a; b < 6; ++b) acc[slot++] += jac[a] * jac[b];     // a zero normal adds zeros
          }
        } else if constexpr (GENERALIZED) {
          const float* v = t_normals + 3 * (t_begin + at[r]);     // the winner's normal, once per source row
          const double sa[3] = {(double)ax[r], (double)ay[r], (double)az[r]};
          const double nc[3] = {(double)v[0], (double)v[1], (double)v[2]};
          icp_generalized_row(acc, pc, qc, sa, nc, dd, keep);
        } else {
          icp_point_row(acc, pc, qc, dd);
        }
      }
    }
  }

  __syncthreads();                                               // the last tile has been read by every wave
  icp_reduce_partials<NS, RG_THREADS>(acc, reinterpret_cast<double*>(s_x), partials);          // (RG_WAVES, NS) in the x plane
}

// the point-to-plane update (R | t) of the 29 sums: A x = -g by an LDL^T factorisation without pivoting in a fixed operation
// order, x = (alpha, beta, gamma, tx, ty, tz), R = Rz(gamma) Ry(beta) Rx(alpha); false where a pivot is <= RG_PIVOT_TOL x
// its diagonal entry (the correspondences do not determine the six unknowns) or not a number.  Every loop unrolls, so no
// array is indexed by a run-time value.
__device__ bool plane_solve(const double* s, double (&r)[3][3], double (&t)[3]) {
  double a[6][6], d[6], x[6];                                    // the lower triangle of `a` becomes L
  {
    int slot = 8;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) {
        a[i][j] = s[slot];
        a[j][i] = s[slot++];
      }
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const double diag = a[j][j];
    double dj = diag;
#pragma unroll
    for (int k = 0; k < j; ++k) dj -= a[j][k] * a[j][k] * d[k];
    if (!(dj > RG_PIVOT_TOL * diag)) ok = false;
    d[j] = dj;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = a[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= a[i][k] * a[j][k] * d[k];
      a[i][j] = v / dj;
    }
  }
  if (!ok) return false;
#pragma unroll
  for (int i = 0; i < 6; ++i) {                                  // L y = -g
    double v = -s[2 + i];
#pragma unroll
    for (int k = 0; k < i; ++k) v -= a[i][k] * x[k];
    x[i] = v;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] = x[i] / d[i];
#pragma unroll
  for (int i = 5; i >= 0; --i) {                                 // L^T x = z
    double v = x[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) v -= a[k][i] * x[k];
    x[i] = v;
  }
  const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
  r[0][0] = cb * cg;
  r[0][1] = sa * sb * cg - ca * sg;
  r[0][2] = ca * sb * cg + sa * sg;
  r[1][0] = cb * sg;
  r[1][1] = sa * sb * sg + ca * cg;
  r[1][2] = ca * sb * sg - sa * cg;
  r[2][0] = -sb;
  r[2][1] = sa * cb;
  r[2][2] = ca * cb;
  t[0] = x[3];
  t[1] = x[4];
  t[2] = x[5];
  return true;
}

template <bool PLANE>
__global__ void __launch_bounds__(HFL_WAVE)
icp_solve_kernel(double* __restrict__ state, int32_t* __restrict__ istate, double* __restrict__ sums,
                 const double* __restrict__ partials, const int64_t* __restrict__ tile_off, int64_t n_tiles,
                 const int64_t* __restrict__ s_off, int min_corr, double rel_fitness, double rel_rmse, int is_last) {
  const int64_t p = blockIdx.x;
  if (istate[2 * p + 1] != HFL_ICP_RUNNING) return;              // uniform: one wave per pair
  constexpr int NS = PLANE ? RG_PLANE_SUMS : RG_SUMS, SUM_D2 = PLANE ? 1 : 16;
  const int lane = threadIdx.x;
  const int64_t first = max(tile_off[p], (int64_t)0), last = min(tile_off[p + 1], n_tiles);
  double mine = 0.0;
  if (lane < NS)
    for (int64_t tile = first; tile < last; ++tile) mine += partials[tile * NS + lane];        // ascending tile order
  if (sums != nullptr && lane < NS) sums[p * NS + lane] = mine;
  double s[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) s[k] = __shfl(mine, k, HFL_WAVE);
  if (lane != 0) return;

  double* st = state + 16 * p;
  const int k_iter = istate[2 * p];
  const double n = s[0], n_src = (double)max(s_off[p + 1] - s_off[p], (int64_t)0);
  const double fitness = n / n_src;                              // an empty source cloud: 0 / 0 = NaN
  const bool few = n < (double)min_corr;
  const double rmse = (few || n <= 0.0) ? (double)NAN : sqrt(s[SUM_D2] / n);
  st[12] = fitness;
  st[13] = rmse;
  if (few) {
    istate[2 * p + 1] = HFL_ICP_TOO_FEW;
    return;
  }
  if (k_iter >= 1 && fabs(fitness - st[14]) < rel_fitness && fabs(rmse - st[15]) < rel_rmse) {
    istate[2 * p + 1] = HFL_ICP_CONVERGED;
    return;
  }
  if (is_last) {
    istate[2 * p + 1] = HFL_ICP_MAX_ITERATIONS;
    return;
  }
  double r[3][3], t[3];
  bool solved;
  if constexpr (PLANE) solved = plane_solve(s, r, t); else solved = kabsch_solve(s, r, t);
  if (!solved) {
    istate[2 * p + 1] = HFL_ICP_DEGENERATE;
    return;
  }
  double next[12];                                               // (R | t) . T_k
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 4; ++b)
      next[4 * a + b] = r[a][0] * st[b] + r[a][1] * st[4 + b] + r[a][2] * st[8 + b] + (b == 3 ? t[a] : 0.0);
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) st[k] = next[k];
  st[14] = fitness;
  st[15] = rmse;
  istate[2 * p] = k_iter + 1;
}

}  // namespace

namespace {

// `target_normals` is required with RG_PLANE and RG_GENERALIZED and not looked at without; `source_normals` and `epsilon`
// (in (0, 1]; a NaN fails the test) go with RG_GENERALIZED alone
template <int EST>
int icp_correspond_call(double* partials, float* dist, int32_t* idx, const float* source, const float* source_normals,
                        const int64_t* s_offsets, int64_t n_source, const float* targets, const float* target_normals,
                        const int64_t* t_offsets, int64_t n_targets, const int64_t* tiles, int64_t n_tiles, const double* state,
                        const int32_t* istate, float max_dist, double epsilon, int64_t n_pairs, hfl_stream_t stream) {
  const bool ok = (EST == RG_POINT || target_normals != nullptr) &&
                  (EST != RG_GENERALIZED || (source_normals != nullptr && epsilon > 0.0 && epsilon <= 1.0));
  return pair_scan_call({partials, source, s_offsets, targets, t_offsets, tiles, state, istate}, ok, n_source, n_targets,
                        n_tiles, n_pairs, [&] {
    icp_correspond_kernel<EST><<<(unsigned)n_tiles, RG_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
        partials, dist, idx, source, s_offsets, n_source, targets, target_normals, t_offsets, n_targets, tiles, state, istate,
        max_dist, (int)n_pairs, source_normals, epsilon);
  });
}

template <bool PLANE>
int icp_solve_call(double* state, int32_t* istate, double* sums, const double* partials, const int64_t* tile_offsets,
                   int64_t n_tiles, const int64_t* s_offsets, int64_t n_pairs, int min_correspondences,
                   double relative_fitness, double relative_rmse, int is_last, hfl_stream_t stream) {
  if (state == nullptr || istate == nullptr || partials == nullptr || tile_offsets == nullptr || s_offsets == nullptr ||
      n_tiles < 0 || n_pairs < 1 || min_correspondences < 0)
    return HFL_EINVAL;
  if (n_tiles > 0x7fffffffLL || n_pairs > 0x7fffffffLL) return HFL_ECAPACITY;
  icp_solve_kernel<PLANE><<<(unsigned)n_pairs, HFL_WAVE, 0, static_cast<hipStream_t>(stream)>>>(
      state, istate, sums, partials, tile_offsets, n_tiles, s_offsets, min_correspondences, relative_fitness, relative_rmse,
      is_last);
  HFL_RETURN_LAST_ERROR();
}

}  // namespace

extern "C" int hfl_icp_correspond(double* partials, float* dist, int32_t* idx, const float* source, const int64_t* s_offsets,
                                  int64_t n_source, const float* targets, const int64_t* t_offsets, int64_t n_targets,
                                  const int64_t* tiles, int64_t n_tiles, const double* state, const int32_t* istate,
                                  float max_dist, int64_t n_pairs, hfl_stream_t stream) {
  return icp_correspond_call<RG_POINT>(partials, dist, idx, source, nullptr, s_offsets, n_source, targets, nullptr, t_offsets,
                                       n_targets, tiles, n_tiles, state, istate, max_dist, 1.0, n_pairs, stream);
}

extern "C" int hfl_icp_correspond_plane(double* partials, float* dist, int32_t* idx, const float* source,
                                        const int64_t* s_offsets, int64_t n_source, const float* targets,
                                        const float* target_normals, const int64_t* t_offsets, int64_t n_targets,
                                        const int64_t* tiles, int64_t n_tiles, const double* state, const int32_t* istate,
                                        float max_dist, int64_t n_pairs, hfl_stream_t stream) {
  return icp_correspond_call<RG_PLANE>(partials, dist, idx, source, nullptr, s_offsets, n_source, targets, target_normals,
                                       t_offsets, n_targets, tiles, n_tiles, state, istate, max_dist, 1.0, n_pairs, stream);
}

extern "C" int hfl_icp_correspond_generalized(double* partials, float* dist, int32_t* idx, const float* source,
                                              const float* source_normals, const int64_t* s_offsets, int64_t n_source,
                                              const float* targets, const float* target_normals, const int64_t* t_offsets,
                                              int64_t n_targets, const int64_t* tiles, int64_t n_tiles, const double* state,
                                              const int32_t* istate, float max_dist, double epsilon, int64_t n_pairs,
                                              hfl_stream_t stream) {
  return icp_correspond_call<RG_GENERALIZED>(partials, dist, idx, source, source_normals, s_offsets, n_source, targets,
                                             target_normals, t_offsets, n_targets, tiles, n_tiles, state, istate, max_dist,
                                             epsilon, n_pairs, stream);
}

extern "C" int hfl_icp_solve(double* state, int32_t* istate, double* sums, const double* partials,
                             const int64_t* tile_offsets, int64_t n_tiles, const int64_t* s_offsets, int64_t n_pairs,
                             int min_correspondences, double relative_fitness, double relative_rmse, int is_last,
                             hfl_stream_t stream) {
  return icp_solve_call<false>(state, istate, sums, partials, tile_offsets, n_tiles, s_offsets, n_pairs, min_correspondences,
                               relative_fitness, relative_rmse, is_last, stream);
}

extern "C" int hfl_icp_solve_plane(double* state, int32_t* istate, double* sums, const double* partials,
                                   const int64_t* tile_offsets, int64_t n_tiles, const int64_t* s_offsets, int64_t n_pairs,
                                   int min_correspondences, double relative_fitness, double relative_rmse, int is_last,
                                   hfl_stream_t stream) {
  return icp_solve_call<true>(state, istate, sums, partials, tile_offsets, n_tiles, s_offsets, n_pairs, min_correspondences,
                              relative_fitness, relative_rmse, is_last, stream);
}
