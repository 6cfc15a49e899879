// The plane rotation of the one-sided cyclic Jacobi on a 3 x 3 (csrc/registration.hip: the singular vectors of the Kabsch
// update; csrc/normals.hip: the eigenvectors of a neighbourhood covariance) and the run-time pick of a column without a
// run-time register index.
#pragma once
#include <math.h>

#include "hfl_common.h"

namespace {

// columns P and Q of G = H V made orthogonal by one plane rotation, applied to V as well
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&g)[3][3], double (&v)[3][3]) {
  const double alpha = g[0][P] * g[0][P] + g[1][P] * g[1][P] + g[2][P] * g[2][P];
  const double beta = g[0][Q] * g[0][Q] + g[1][Q] * g[1][Q] + g[2][Q] * g[2][Q];
  const double gamma = g[0][P] * g[0][Q] + g[1][P] * g[1][Q] + g[2][P] * g[2][Q];
  if (gamma == 0.0) return;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));    // zeta = +-inf: t = 0
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double gp = g[i][P], gq = g[i][Q], vp = v[i][P], vq = v[i][Q];
    g[i][P] = c * gp - s * gq;
    g[i][Q] = s * gp + c * gq;
    v[i][P] = c * vp - s * vq;
    v[i][Q] = s * vp + c * vq;
  }
}

__device__ __forceinline__ double pick(const double (&a)[3][3], int i, int j) {
  return j == 0 ? a[i][0] : (j == 1 ? a[i][1] : a[i][2]);
}

}  // namespace
