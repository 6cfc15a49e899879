// From the float64 sums over a neighbourhood to the ordered eigenvalues of its covariance: steps 3 and 4 of the definition in
// hotformerloc_amd/normals.py, for csrc/normals.hip (the normal and the surface variation) and csrc/keypoints.hip (the ISS
// saliency).  Both files are built with -ffp-contract=off and run these operations in this order, so either agrees with
// `normals._eigen_host` as before.
#pragma once
#include <math.h>

#include "jacobi3.h"

namespace {

constexpr int NR_SWEEPS = 12;                                    // RG_SWEEPS of registration.hip
constexpr int NR_SUMS = 9;                                       // S1 (3), S2 (xx, xy, xz, yy, yz, zz)

// one neighbour's contribution, e = p_j - p_i in float64
__device__ __forceinline__ void normal_add(double (&s)[NR_SUMS], float px, float py, float pz, const float* __restrict__ q) {
  const double ex = (double)q[0] - (double)px, ey = (double)q[1] - (double)py, ez = (double)q[2] - (double)pz;
  s[0] += ex;
  s[1] += ey;
  s[2] += ez;
  s[3] += ex * ex;
  s[4] += ex * ey;
  s[5] += ex * ez;
  s[6] += ey * ey;
  s[7] += ey * ez;
  s[8] += ez * ez;
}

// C from the sums over m >= 1 neighbours, the one-sided cyclic Jacobi of fixed sweep count on it (G = C V with orthogonal
// columns: their norms are the eigenvalues of the positive semi-definite C, V's columns the eigenvectors), the order: the
// largest, then the larger of the other two, the lowest column on a tie.  Then f(l0, l1, l2, V, the column of l0 in V): the
// caller's finish runs inside this function, so that the compiler sees one body, as it did when csrc/normals.hip held all of
// it (a function that returned the eigenvalues cost that file's kernels 6 to 19 VGPRs)
template <typename F>
__device__ inline void cov_eigen(const double (&s)[NR_SUMS], int m, F&& f) {
  const double dm = (double)m;
  const double mu[3] = {s[0] / dm, s[1] / dm, s[2] / dm};
  double g[3][3], v[3][3];
  g[0][0] = s[3] / dm - mu[0] * mu[0];
  g[0][1] = s[4] / dm - mu[0] * mu[1];
  g[0][2] = s[5] / dm - mu[0] * mu[2];
  g[1][1] = s[6] / dm - mu[1] * mu[1];
  g[1][2] = s[7] / dm - mu[1] * mu[2];
  g[2][2] = s[8] / dm - mu[2] * mu[2];
  g[1][0] = g[0][1];
  g[2][0] = g[0][2];
  g[2][1] = g[1][2];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) v[a][b] = a == b ? 1.0 : 0.0;
  for (int sweep = 0; sweep < NR_SWEEPS; ++sweep) {
    jacobi_rotate<0, 1>(g, v);
    jacobi_rotate<0, 2>(g, v);
    jacobi_rotate<1, 2>(g, v);
  }
  double w[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) w[j] = sqrt(g[0][j] * g[0][j] + g[1][j] * g[1][j] + g[2][j] * g[2][j]);
  const int i2 = (w[0] >= w[1] && w[0] >= w[2]) ? 0 : (w[1] >= w[2] ? 1 : 2);
  const int ja = i2 == 0 ? 1 : 0, jb = i2 == 2 ? 1 : 2;
  const int i1 = w[ja] >= w[jb] ? ja : jb, i0 = w[ja] >= w[jb] ? jb : ja;
  const double l0 = i0 == 0 ? w[0] : (i0 == 1 ? w[1] : w[2]);
  const double l1 = i1 == 0 ? w[0] : (i1 == 1 ? w[1] : w[2]);
  const double l2 = i2 == 0 ? w[0] : (i2 == 1 ? w[1] : w[2]);
  f(l0, l1, l2, v, i0);
}

}  // namespace
