// The device functions the rounding of a session (session_round.hip) and its projection to rank d
// (session_project.hip) share: where a pose's columns lie in the two orderings, the four-lanes-per-pose projection of a
// rotation block, the normalisation of a unit-sphere column.  Both apply an r x d frame F (the anchor's rotation there,
// the top-d eigenvectors of X X^T here) as F^T x, one fma chain per element in index order, and differ in where the
// result goes.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "so_project.h"

namespace dcora {

constexpr int kQuad = 4;  // lanes per pose: lane c owns column c of the pose's block (k_spmm_bsrq's assignment)

// where column c (c < D: rotation, c == D: translation) of pose i lies in the block
template <int D>
struct SeCols {
  __device__ __forceinline__ long col(int i, int c) const { return (long)i * (D + 1) + c; }
};
template <int D>
struct RaCols {
  int n, l;
  __device__ __forceinline__ long col(int i, int c) const {
    return c < D ? (long)D * i + c : (long)D * n + l + i;
  }
};

// m: what lane c of a quad holds of M = F^T [Y_i | p_i] (column c, D elements).  The quad hands its D rotation columns
// round with quad_perm moves: A = F^T Y_i, column-major, in every lane.  (Every lane of the wave is active here.)
template <int D>
__device__ __forceinline__ void quad_gather(const double *m, double *A) {
  // column cc of M from lane cc of the quad: quad_perm [cc, cc, cc, cc]
#pragma unroll
  for (int a = 0; a < D; ++a) {
    A[0 * D + a] = dpp_move<0x00>(m[a]);
    A[1 * D + a] = dpp_move<0x55>(m[a]);
    if (D == 3) A[(D - 1) * D + a] = dpp_move<0xAA>(m[a]);
  }
}

// ... then every lane projects the whole block (so_project: the same operations on the same bits in the D lanes that
// store), lane c < D keeps column c of Proj_SO(D)(F^T Y_i) in v, lane D its own m.
template <int D>
__device__ __forceinline__ void quad_so_project(const double *m, int c, double *v) {
  double A[D * D];
  quad_gather<D>(m, A);
  so_project<D>(A);
#pragma unroll
  for (int a = 0; a < D; ++a) {
    v[a] = m[a];
#pragma unroll
    for (int cc = 0; cc < D; ++cc)
      if (c == cc) v[a] = A[cc * D + a];
  }
}

// m = F^T y for a frame in LDS (sm[a r + q] = F(q, a)): D sums over q = 0 .. r-1, each ONE fma chain in index order;
// a lane that is not valid reads nothing and gets zeros
template <int D>
__device__ __forceinline__ void frame_dot(int r, const double *sm, const double *__restrict__ y, bool valid,
                                          double *m) {
#pragma unroll
  for (int a = 0; a < D; ++a) m[a] = 0.0;
  for (int q = 0; q < r; ++q) {
    const double yq = valid ? y[q] : 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a) m[a] = fma(sm[a * r + q], yq, m[a]);
  }
}

// m / |m|; a zero column stays zero
template <int D>
__device__ __forceinline__ void unit_or_zero(double *m) {
  double s = 0.0;
#pragma unroll
  for (int a = 0; a < D; ++a) s = fma(m[a], m[a], s);
  s = sqrt(s);
  if (s > 0) {
#pragma unroll
    for (int a = 0; a < D; ++a) m[a] /= s;
  }
}

}  // namespace dcora
