// The rigid update (R | t) of the 17 float64 sums n, Sp (3), Sq (3), Spq (9, row-major: p down, q across), sum d^2 of a set
// of point pairs p -> q, once, for everything that solves it: hfl_icp_solve (csrc/registration.hip) on the inliers of an ICP
// iteration and of the RANSAC polish, hfl_ransac_hypotheses (csrc/global_registration.hip) on a drawn triple.  A one-sided
// cyclic Jacobi on H = Spq - Sp Sq^T / n with a fixed number of sweeps; `_host_kabsch_many` of hotformerloc_amd/registration.py
// is its one numpy transcription, line by line on arrays of rows.  No array is indexed by a run-time value.
#pragma once
#include <math.h>

#include "jacobi3.h"

namespace {

constexpr int KABSCH_SWEEPS = 12;                                // a 3 x 3 converges quadratically: 5 or 6 suffice
constexpr double KABSCH_RANK_TOL = 1e-12;                        // second singular value <= this x the largest: degenerate

// the rigid update (R | t) of the 17 sums; false where the correspondences are collinear or coincident
__device__ bool kabsch_solve(const double* s, double (&r)[3][3], double (&t)[3]) {
  const double n = s[0];
  double g[3][3], v[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      g[a][b] = s[7 + 3 * a + b] - s[1 + a] * s[4 + b] / n;      // H
      v[a][b] = a == b ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < KABSCH_SWEEPS; ++sweep) {
    jacobi_rotate<0, 1>(g, v);
    jacobi_rotate<0, 2>(g, v);
    jacobi_rotate<1, 2>(g, v);
  }
  double w[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) w[j] = sqrt(g[0][j] * g[0][j] + g[1][j] * g[1][j] + g[2][j] * g[2][j]);
  // the largest and the second largest, the lowest column on a tie
  const int i1 = (w[0] >= w[1] && w[0] >= w[2]) ? 0 : (w[1] >= w[2] ? 1 : 2);
  const int ja = i1 == 0 ? 1 : 0, jb = i1 == 2 ? 1 : 2;
  const int i2 = w[ja] >= w[jb] ? ja : jb;
  const double w1 = i1 == 0 ? w[0] : (i1 == 1 ? w[1] : w[2]), w2 = i2 == 0 ? w[0] : (i2 == 1 ? w[1] : w[2]);
  if (!(w2 > KABSCH_RANK_TOL * w1)) return false;                // also a NaN, and H = 0
  double u1[3], u2[3], v1[3], v2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    u1[i] = pick(g, i, i1) / w1;
    u2[i] = pick(g, i, i2) / w2;
    v1[i] = pick(v, i, i1);
    v2[i] = pick(v, i, i2);
  }
  const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
  const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
  const double mp[3] = {s[1] / n, s[2] / n, s[3] / n}, mq[3] = {s[4] / n, s[5] / n, s[6] / n};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) r[a][b] = v1[a] * u1[b] + v2[a] * u2[b] + v3[a] * u3[b];
    t[a] = mq[a] - (r[a][0] * mp[0] + r[a][1] * mp[1] + r[a][2] * mp[2]);
  }
  return true;
}

}  // namespace
