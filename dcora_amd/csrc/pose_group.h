// Per-pose arithmetic of the SE layout with 8 lanes per pose, shared by the fused kernel files (fused_step.hip,
// fused_run.hip, fused_eval.hip, fused_pose.hip): lane t of a group owns row t of the pose's r x (d+1) block, d x d
// Gram matrices are reduced with 3 DPP moves.  Device code, the launch shapes that follow from it (kPosesPerBlock,
// fused_pb) and, at the end, one piece of host dispatch: DCORA_LAUNCH_D, the <3> / <2> launch of a kernel template.
#pragma once
#include "kernels.h"

namespace dcora {

namespace {

constexpr int GW = 8;  // lanes per pose

// Up to 64 partials: every wave loads them itself (lane l takes partial l) and sums them with wave_sum, so the
// total is known in every wave without a barrier or an LDS exchange; more partials go through the block reduction.
// Up to 256 partials without a barrier: every wave loads all of them (lane l takes partials l, l + 64, l + 128, l + 192:
// four predicated loads requested together) and sums them with wave_sum -- __syncthreads() drains vmcnt, i.e. it
// would wait for every gather the kernel has in flight behind the partials (measured in k_fused_hess with the 250
// partials of k_fused_pc: 1.7 us at the reduction).  f_partial4_load / f_partial4_total; beyond 256 the block path.
__device__ __forceinline__ double f_partial4_load(const double *__restrict__ p, int np) {
  const int l = (int)(threadIdx.x & 63u);
  const double a = (l < np) ? p[l] : 0.0, b = (l + 64 < np) ? p[l + 64] : 0.0;
  const double c = (l + 128 < np) ? p[l + 128] : 0.0, d = (l + 192 < np) ? p[l + 192] : 0.0;
  return (a + b) + (c + d);
}
// f_partial_index is the index a thread loads, f_partial_total the matching reduction.
__device__ __forceinline__ int f_partial_index(int np) { return np <= 64 ? (int)(threadIdx.x & 63u) : (int)threadIdx.x; }
__device__ __forceinline__ double f_partial_total(double v, int np, double *sm) {
  return np <= 64 ? wave_sum(v) : block_sum(v, sm);
}
// sum over the 8 lanes of a pose group (every lane of the wave must take part).  The result is re-broadcast from
// the group's first lane: with FMA contraction the butterfly partial sums can differ in the last bit between
// lanes, and the Jacobi / Gram-Schmidt decisions taken from them must be identical across the group.
// DPP row operations (xor 1, xor 2 inside the quads, mirror of the 8 lanes) instead of __shfl / ds_bpermute: the
// Jacobi sweeps of row_polar take dozens of these sums per pose.  The argument is pinned as an already-rounded value
// first, so every add below combines two rounded numbers and, addition being commutative, the eight lanes end with
// bitwise the same sum (same tree as the xor butterfly it replaces).
__device__ __forceinline__ double grp_sum(double v) {
  asm volatile("" : "+v"(v));
  v += dpp_move<0xB1>(v);   // quad_perm [1,0,3,2]
  asm volatile("" : "+v"(v));
  v += dpp_move<0x4E>(v);   // quad_perm [2,3,0,1]
  asm volatile("" : "+v"(v));
  v += dpp_move<0x141>(v);  // row_half_mirror: lane i <- lane 7 - i of its group of eight
  return v;
}

template <int D>
struct Row {
  double e[D + 1];  // D rotation entries + the translation entry of row t
};
template <int D>
__device__ __forceinline__ void ld_row(const double *__restrict__ p, int r, int t, bool active, Row<D> &R) {
#pragma unroll
  for (int a = 0; a <= D; ++a) R.e[a] = active ? p[a * r + t] : 0.0;
}
template <int D>
__device__ __forceinline__ void st_row(double *__restrict__ p, int r, int t, bool active, const Row<D> &R) {
  if (active)
#pragma unroll
    for (int a = 0; a <= D; ++a) p[a * r + t] = R.e[a];
}
// S = sym(Y^T E) over the rotation columns (group-wide result in every lane)
template <int D>
__device__ __forceinline__ void grp_sym_gram(const Row<D> &Y, const Row<D> &E, double (&S)[D][D]) {
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = a; b < D; ++b) {
      const double s = grp_sum(0.5 * (Y.e[a] * E.e[b] + Y.e[b] * E.e[a]));
      S[a][b] = s;
      S[b][a] = s;
    }
}
// V_rot <- V_rot - A_rot S
template <int D>
__device__ __forceinline__ void row_sub_AS(Row<D> &V, const Row<D> &A, const double (&S)[D][D]) {
#pragma unroll
  for (int b = 0; b < D; ++b) {
    double s = 0;
#pragma unroll
    for (int a = 0; a < D; ++a) s += A.e[a] * S[a][b];
    V.e[b] -= s;
  }
}
template <int D>
__device__ __forceinline__ void row_tangent(const Row<D> &Y, Row<D> &V) {
  double S[D][D];
  grp_sym_gram<D>(Y, V, S);
  row_sub_AS<D>(V, Y, S);
}
// QF retraction of the rotation part (modified Gram-Schmidt, one re-orthogonalisation pass)
template <int D>
__device__ __forceinline__ void row_qf(Row<D> &A) {
#pragma unroll
  for (int j = 0; j < D; ++j) {
#pragma unroll
    for (int pass = 0; pass < 2; ++pass)
#pragma unroll
      for (int c = 0; c < D; ++c)
        if (c < j) {
          const double s = grp_sum(A.e[c] * A.e[j]);
          A.e[j] -= s * A.e[c];
        }
    const double nn = grp_sum(A.e[j] * A.e[j]);
    A.e[j] *= 1.0 / sqrt(nn);
  }
}
// polar factor of the rotation part.  The RBCD++ sequences hand in blocks that are orthonormal up to the size of a
// step ((1 - alpha) x + alpha v, v + gamma (x - y): ref src/Agent.cpp:1196-1214 project them with a thin SVD), so the
// common case runs on the Gram matrix: G = A^T A by D (D + 1) / 2 group sums, Z = G^(-1/2) by the coupled Newton-Schulz
// iteration (Y <- Y T, Z <- T Z, T = (3 I - Z Y) / 2: products of D x D symmetric matrices in registers, no division, no
// square root, nothing crosses lanes), A <- A Z.  G is the same in the eight lanes of a pose, so they take the same
// steps; the iteration converges quadratically for |I - G| < 1 and the Gram form loses nothing at condition numbers
// near one.  Blocks further than kPolarGramRadius from orthonormal (set_X of a rough point, a long step) take the
// one-sided Jacobi sweeps below, as every block did before: k_g_nesterov over the 100k lattice 36 us with Jacobi for all
// (the sweeps' divisions and square roots, 12 waves deep per SIMD, not the memory), with this form see DESIGN.md.
constexpr double kPolarGramRadius = 0.25;
template <int D>
__device__ __forceinline__ void sym_mul(const double (&A)[D][D], const double (&B)[D][D], double (&C)[D][D]) {
  // the product of two commuting symmetric matrices is symmetric: upper triangle, mirrored
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = a; b < D; ++b) {
      double s = 0;
#pragma unroll
      for (int c = 0; c < D; ++c) s += A[a][c] * B[c][b];
      C[a][b] = s;
      C[b][a] = s;
    }
}
template <int D>
__device__ __forceinline__ void row_polar(Row<D> &A, bool live) {
  double G[D][D];
  double dist2 = 0;
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = a; b < D; ++b) {
      const double s = grp_sum(A.e[a] * A.e[b]);
      G[a][b] = s;
      G[b][a] = s;
      const double e = s - (a == b ? 1.0 : 0.0);
      dist2 += (a == b ? 1.0 : 2.0) * e * e;
    }
  const bool gram = live && dist2 <= kPolarGramRadius * kPolarGramRadius;  // the same in the lanes of a pose
  if (gram) {
    double Y[D][D], Z[D][D];
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < D; ++b) {
        Y[a][b] = G[a][b];
        Z[a][b] = (a == b) ? 1.0 : 0.0;
      }
    for (int it = 0; it < 12; ++it) {
      double T[D][D], ZY[D][D], Yn[D][D], Zn[D][D];
      sym_mul<D>(Z, Y, ZY);
      double e2 = 0;
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) {
          const double rr = (a == b ? 1.0 : 0.0) - ZY[a][b];
          e2 += rr * rr;
          T[a][b] = (a == b ? 1.0 : 0.0) + 0.5 * rr;
        }
      sym_mul<D>(Y, T, Yn);
      sym_mul<D>(T, Z, Zn);
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) {
          Y[a][b] = Yn[a][b];
          Z[a][b] = Zn[a][b];
        }
      if (e2 < 1e-16) break;  // |I - Z Y| < 1e-8 before this step: below 1e-16 after it
    }
    double o[D];
#pragma unroll
    for (int c = 0; c < D; ++c) {
      double s = 0;
#pragma unroll
      for (int j = 0; j < D; ++j) s += A.e[j] * Z[j][c];
      o[c] = s;
    }
#pragma unroll
    for (int c = 0; c < D; ++c) A.e[c] = o[c];
  }
  // one-sided Jacobi for the others.  The sweep loop is wave-uniform (the group sums are cross-lane operations), but a
  // pose stops rotating once ITS sweep has converged: the result of a pose must not depend on which poses share its
  // wave (a launch over one agent's poses and a launch over the whole graph place a pose next to different neighbours).
  bool settled = !live || gram;
  if (__all(settled)) return;
  const bool jacobi = !settled;
  double Vm[D][D];
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) Vm[a][b] = (a == b) ? 1.0 : 0.0;
  Row<D> B = A;
  for (int sweep = 0; sweep < 40; ++sweep) {
    double off = 0;
#pragma unroll
    for (int p = 0; p < D - 1; ++p)
#pragma unroll
      for (int q = p + 1; q < D; ++q) {
        const double app = grp_sum(B.e[p] * B.e[p]);
        const double aqq = grp_sum(B.e[q] * B.e[q]);
        const double apq = grp_sum(B.e[p] * B.e[q]);
        const double sc = sqrt(app * aqq);
        if (!settled && fabs(apq) > 1e-16 * sc && fabs(apq) > 1e-300) {
          off = fmax(off, fabs(apq) / sc);
          const double zeta = (aqq - app) / (2.0 * apq);
          const double tt = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
          const double x = B.e[p], y = B.e[q];
          B.e[p] = cs * x - sn * y;
          B.e[q] = sn * x + cs * y;
#pragma unroll
          for (int i = 0; i < D; ++i) {
            const double vx = Vm[p][i], vy = Vm[q][i];
            Vm[p][i] = cs * vx - sn * vy;
            Vm[q][i] = sn * vx + cs * vy;
          }
        }
      }
    settled = settled || off < 1e-15;
    if (__all(settled)) break;
  }
  double u[D];
#pragma unroll
  for (int j = 0; j < D; ++j) {
    const double nn = grp_sum(B.e[j] * B.e[j]);
    u[j] = B.e[j] * (nn > 0 ? 1.0 / sqrt(nn) : 0.0);
  }
  if (jacobi)
#pragma unroll
    for (int c = 0; c < D; ++c) {
      double s = 0;
#pragma unroll
      for (int j = 0; j < D; ++j) s += u[j] * Vm[j][c];
      A.e[c] = s;
    }
}

constexpr int kHessTile = 1536;              // nnz staged per pass (18 KiB of LDS)
constexpr int kPosesPerBlock = kBlock / GW;  // 32 (pure per-pose kernels)
constexpr int kBsrTile = 160;                // matrix blocks staged per pass (20 KiB at (d+1)^2 = 16)

// poses per block of the two-phase kernels: phase 1 runs one thread per output element (pose, column, row),
// phase 2 eight lanes per pose
__host__ __device__ constexpr int fused_pb(int r, int dh) {
  const int pb = kBlock / (dh * r);
  return pb > kPosesPerBlock ? kPosesPerBlock : pb;
}

// one launch of KERNEL<3> or KERNEL<2> (kBlock threads, no dynamic LDS), as the pose dimension d says
#define DCORA_LAUNCH_D(KERNEL, d, grid, st, ...)                                                 \
  do {                                                                                           \
    if ((d) == 3) hipLaunchKernelGGL(KERNEL<3>, dim3(grid), dim3(kBlock), 0, st, __VA_ARGS__);   \
    else hipLaunchKernelGGL(KERNEL<2>, dim3(grid), dim3(kBlock), 0, st, __VA_ARGS__);            \
  } while (0)

}  // namespace

}  // namespace dcora
