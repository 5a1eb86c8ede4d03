// What device_chol.hip (the multifrontal factorisation) and dense_inverse.hip (the triangular inverses behind it) share:
// the 64 x 64 tile product on the matrix pipe with the walk over a thread's 16 sums, the 64 x 64 triangular inverse in
// LDS, the job list of a batched inversion and the two host schedules each file borrows from the other.
#pragma once
#include <hip/hip_runtime.h>

#include "device_chol.h"
#include "device_problem.h"

namespace dcora {

constexpr int NB = kCholNb;

struct PieceDev {
  long long off;
  int c, m;
  int parent, rel_off;
};

// one piece of a batched inversion (blockIdx.z): offsets into the arrays the kernels are given
struct InvJob {
  int c, m;
  int ldm;             // leading dimension of M (c for a piece; the padded rows of a dense preconditioner)
  long long l11, f;    // L11 inside the front arena, leading dimension of the front
  long long yt, tinv;  // (L11^-1)^T (c x c) and the inverses of its 64 x 64 diagonal blocks
  long long pk, mt;    // the packed panel; M = L11^-T L11^-1 (c x c) or -1
};

// the arrays a job list indexes and what is wanted of it (enqueue_inverse_jobs)
struct InvBatch {
  const InvJob *jobs = nullptr;  // device
  int count = 0, cmax = 0, mmax = 0;  // widest piece, most rows below a piece
  const double *F = nullptr;     // l11
  double *yt = nullptr, *tinv = nullptr, *packed = nullptr, *M = nullptr;  // yt (zeroed by the caller), tinv, pk, mt
  int tstride = 1;               // 64 x 64 blocks between the inverses of consecutive diagonal blocks in tinv
  bool diag_inverses = true;     // form tinv from L11 (false: the factorisation left the inverses there)
  bool want_panel = true;        // [L11^-1; W = -L21 L11^-1] into the packed panel
  bool want_m = true;            // M of every job whose mt >= 0
};
// dense_inverse.hip: k_tri_inv64, finish(ib) and update(ib) for every block row, k_piece_w, k_piece_pack_inverted,
// k_dense_lauum over the list, enqueued on st; the caller checks hipGetLastError() and keeps the list alive
void enqueue_inverse_jobs(hipStream_t st, const InvBatch &b);
// device_chol.hip: LL^T of `count` whole matrices of order k (pieces[list[q]]: one front each, m = 0), 64 columns at a
// time; the inverse of diagonal block p of matrix q goes to linv + (p panel_stride + q) 64 x 64 doubles
void enqueue_dense_potrf(hipStream_t st, const PieceDev *pieces, const int *list, int count, int k, double *F,
                         double *linv, int panel_stride, int *fail, double *logdet);

// a stream of the device's pool for the length of a scope
struct StreamLease {
  int device;
  hipStream_t st = nullptr;
  explicit StreamLease(int device_) : device(device_) {}
  int acquire() { return stream_acquire(device, &st); }
  ~StreamLease() {
    if (st) stream_release(device, st);
  }
  StreamLease(const StreamLease &) = delete;
  StreamLease &operator=(const StreamLease &) = delete;
};

typedef double v4f64 __attribute__((ext_vector_type(4)));

// ---- the 64 x 64 x 64 product of two LDS tiles, As[k][i] and Bs[k][j]: acc(i, j) += sum_k As[k][i] Bs[k][j] ----
// v_mfma_f64_16x16x4_f64: every wave owns a 32 x 32 quadrant as 2 x 2 blocks; 4 LDS reads per 4 MFMAs (8192 flop), the
// matrix pipe is the bound.  A thread keeps its 16 sums in acc[4][4]: acc[u][v] is entry (acc_row(u, v), acc_col(u, v)).
// (The form with 4 x 4 outputs per thread by FMAs -- 8 LDS reads per 16 FMAs, the LDS port is the bound -- measured
// 126 ms against 98 for the factorisation of the 100k lattice and is gone.)
__device__ __forceinline__ int acc_row(int u, int v) {
  return (int)(threadIdx.x >> 7) * 32 + (u >> 1) * 16 + (int)((threadIdx.x & 63) >> 4) + 4 * v;
}
__device__ __forceinline__ int acc_col(int u, int) {
  return (int)((threadIdx.x >> 6) & 1) * 32 + (u & 1) * 16 + (int)(threadIdx.x & 15);
}
__device__ __forceinline__ void zero_acc(double acc[4][4]) {
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[u][v] = 0;
}
// store(row, col, value) for the 16 sums of this thread
template <class F>
__device__ __forceinline__ void for_each_acc(const double acc[4][4], F &&store) {
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) store(acc_row(u, v), acc_col(u, v), acc[u][v]);
}
__device__ __forceinline__ void tile_inner(const double (*As)[NB + 1], const double (*Bs)[NB + 1], double acc[4][4]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r0 = (w >> 1) * 32 + (lane & 15), c0 = (w & 1) * 32 + (lane & 15), kq = lane >> 4;
  v4f64 c[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) c[u] = v4f64{acc[u][0], acc[u][1], acc[u][2], acc[u][3]};
#pragma unroll 4
  for (int k0 = 0; k0 < NB; k0 += 4) {
    const double a0 = As[k0 + kq][r0], a1 = As[k0 + kq][r0 + 16];
    const double b0 = Bs[k0 + kq][c0], b1 = Bs[k0 + kq][c0 + 16];
    c[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, c[0], 0, 0, 0);
    c[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, c[1], 0, 0, 0);
    c[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, c[2], 0, 0, 0);
    c[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, c[3], 0, 0, 0);
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[u][v] = c[u][v];
}

// acc = sum_k A[i][k] B[j][k]; A and B are row-major with k contiguous; rows beyond arows / brows and k beyond K
// read as zero
__device__ __forceinline__ void chol_tile_product(const double *__restrict__ Ag, long long lda, int arows,
                                                  const double *__restrict__ Bg, long long ldb, int brows, int K,
                                                  double (*As)[NB + 1], double (*Bs)[NB + 1], double acc[4][4]) {
  const int tid = threadIdx.x;
  for (int e = tid; e < NB * NB; e += 256) {
    const int i = e >> 6, k = e & 63;
    As[k][i] = (i < arows && k < K) ? Ag[(long long)i * lda + k] : 0.0;
    Bs[k][i] = (i < brows && k < K) ? Bg[(long long)i * ldb + k] : 0.0;
  }
  __syncthreads();
  zero_acc(acc);
  tile_inner(As, Bs, acc);
}

// acc += A-rows x B-rows^T over K chunks of 64: A(ia, l) and B(ib, l), l in [l0, l1)
__device__ __forceinline__ void tile_product_range(const double *__restrict__ Arow, long long lda, int arows,
                                                   const double *__restrict__ Brow, long long ldb, int brows, int l0,
                                                   int l1, double (*As)[NB + 1], double (*Bs)[NB + 1],
                                                   double acc[4][4]) {
  const int tid = threadIdx.x;
  // software pipeline over the 64-column steps: the operands of step l + 1 are requested (into registers) before the
  // products of step l, so their latency hides behind 64 MFMAs per wave instead of standing between two steps
  constexpr int PER = NB * NB / 256;  // entries of each operand per thread
  const int kk = tid & 63, ib = tid >> 6;  // entry q of a thread: row ib + 4 q, column kk of the step
  double ra[PER], rb[PER];
  auto fetch = [&](int l) {
    const int K = min(NB, l1 - l);
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int i = ib + 4 * q;
      ra[q] = (i < arows && kk < K) ? Arow[(long long)i * lda + l + kk] : 0.0;
      rb[q] = (i < brows && kk < K) ? Brow[(long long)i * ldb + l + kk] : 0.0;
    }
  };
  if (l0 < l1) fetch(l0);
  for (int l = l0; l < l1; l += NB) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      As[kk][ib + 4 * q] = ra[q];
      Bs[kk][ib + 4 * q] = rb[q];
    }
    __syncthreads();
    if (l + NB < l1) fetch(l + NB);
    tile_inner(As, Bs, acc);
  }
}

// Li = T^-1 for a 64 x 64 lower-triangular T in LDS (filled by the caller, identity beyond the matrix' order; behind a
// workgroup barrier on return): column k of the inverse by the four lanes k of a wave's group, forward substitution
__device__ __forceinline__ void tri_inv64_lds(const double (*T)[NB + 1], double (*Li)[NB + 1]) {
  __syncthreads();
  const int k = threadIdx.x >> 2, kq = threadIdx.x & 3;
  for (int r = kq; r < k; r += 4) Li[r][k] = 0.0;
  if (kq == 0) Li[k][k] = 1.0 / T[k][k];
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  for (int r = k + 1; r < NB; ++r) {
    double s = 0;
    for (int l = k + kq; l < r; l += 4) s += T[r][l] * Li[l][k];
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    if (kq == 0) Li[r][k] = -s / T[r][r];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
}
}  // namespace dcora
