// Projection of a small block onto SO(d), shared by the host-fed rounding kernels (round.hip) and the session's
// (session_round.hip).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace dcora {

// Projection of a D x D matrix (column-major) onto SO(D): one-sided Jacobi SVD M V = U S, result U V^T with the
// least singular direction of U flipped when det(U) det(V) < 0  (ref src/DCORA_utils.cpp:1661-1675)
template <int D>
__device__ void so_project(double (&A)[D * D]) {
  double V[D * D];
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) V[b * D + a] = (a == b) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0;
#pragma unroll
    for (int p = 0; p < D - 1; ++p)
#pragma unroll
      for (int q = p + 1; q < D; ++q) {
        double app = 0, aqq = 0, apq = 0;
#pragma unroll
        for (int i = 0; i < D; ++i) {
          app += A[p * D + i] * A[p * D + i];
          aqq += A[q * D + i] * A[q * D + i];
          apq += A[p * D + i] * A[q * D + i];
        }
        if (fabs(apq) <= 1e-300 || fabs(apq) <= 1e-16 * sqrt(app * aqq)) continue;
        off = fmax(off, fabs(apq) / sqrt(app * aqq));
        const double zeta = (aqq - app) / (2.0 * apq);
        const double tt = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
#pragma unroll
        for (int i = 0; i < D; ++i) {
          double x = A[p * D + i], y = A[q * D + i];
          A[p * D + i] = cs * x - sn * y;
          A[q * D + i] = sn * x + cs * y;
          x = V[p * D + i];
          y = V[q * D + i];
          V[p * D + i] = cs * x - sn * y;
          V[q * D + i] = sn * x + cs * y;
        }
      }
    if (off < 1e-15) break;
  }
  double sig[D];
  int jmin = 0;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    double nn = 0;
#pragma unroll
    for (int i = 0; i < D; ++i) nn += A[j * D + i] * A[j * D + i];
    sig[j] = sqrt(nn);
  }
#pragma unroll
  for (int j = 1; j < D; ++j)
    if (sig[j] < sig[jmin]) jmin = j;
#pragma unroll
  for (int j = 0; j < D; ++j)
    if (sig[j] > 0) {
      const double inv = 1.0 / sig[j];
#pragma unroll
      for (int i = 0; i < D; ++i) A[j * D + i] *= inv;
    }
  // a block of rank D - 1 (R0^T Y_i = diag(1, 0) for R0 = [e1 e2], Y_i = [e1 e3]) leaves one zero column: the frame is
  // completed by the direction orthogonal to the others, which is then the least singular direction, so the flip
  // below picks its sign.  (Rank <= D - 2 has no nearest rotation; such a block stays singular.)
#pragma unroll
  for (int j = 0; j < D; ++j)
    if (!(sig[j] > 0)) {
      jmin = j;
      if (D == 2) {
        const int o = 1 - j;
        A[j * D + 0] = -A[o * D + 1];
        A[j * D + 1] = A[o * D + 0];
      } else {
        const int a = (j + 1) % D, b = (j + 2) % D;
        A[j * D + 0] = A[a * D + 1] * A[b * D + 2] - A[a * D + 2] * A[b * D + 1];
        A[j * D + 1] = A[a * D + 2] * A[b * D + 0] - A[a * D + 0] * A[b * D + 2];
        A[j * D + 2] = A[a * D + 0] * A[b * D + 1] - A[a * D + 1] * A[b * D + 0];
      }
    }
  double P[D * D];
#pragma unroll
  for (int c = 0; c < D; ++c)
#pragma unroll
    for (int i = 0; i < D; ++i) {
      double s = 0;
#pragma unroll
      for (int j = 0; j < D; ++j) s += A[j * D + i] * V[j * D + c];
      P[c * D + i] = s;
    }
  double det;
  if (D == 2)
    det = P[0] * P[3] - P[2] * P[1];
  else
    det = P[0] * (P[4] * P[8] - P[7] * P[5]) - P[3] * (P[1] * P[8] - P[7] * P[2]) + P[6] * (P[1] * P[5] - P[4] * P[2]);
  if (det < 0) {
    // flip the least singular direction: P -= 2 u_min v_min^T
#pragma unroll
    for (int c = 0; c < D; ++c)
#pragma unroll
      for (int i = 0; i < D; ++i) {
        double um = 0, vm = 0;
#pragma unroll
        for (int j = 0; j < D; ++j)
          if (j == jmin) {
            um = A[j * D + i];
            vm = V[j * D + c];
          }
        P[c * D + i] -= 2.0 * um * vm;
      }
  }
#pragma unroll
  for (int i = 0; i < D * D; ++i) A[i] = P[i];
}

}  // namespace dcora
