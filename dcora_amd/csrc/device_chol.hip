// see device_chol.h
#include "device_chol.h"
#include "env.h"

#include <sys/mman.h>

#include <hip/hip_runtime.h>

#include <chrono>
#include <unistd.h>
#include <cstdlib>
#include <cstring>
#include <list>
#include <mutex>

#include "device_problem.h"
#include "sparse_precond.h"
#include "dense_tiles.h"

namespace dcora {

namespace {

constexpr int kEaRows = 8;  // rows of a child's Schur complement per workgroup of the extend-add

// F[dest[p]] = v[p] for the entries of the lower triangle
__global__ __launch_bounds__(256) void k_chol_scatter(long long nnz, const long long *__restrict__ dest,
                                                      const double *__restrict__ v, double *__restrict__ F) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= nnz) return;
  const long long q = dest[p];
  if (q >= 0) F[q] = v[p];
}

// parent front += Schur complement of one child (children of one slot have distinct parents: no two workgroups of a
// launch touch the same front entry)
__global__ __launch_bounds__(256) void k_chol_extend_add(const PieceDev *__restrict__ pieces,
                                                         const int *__restrict__ children,
                                                         const int *__restrict__ rel, double *__restrict__ F,
                                                         const int *__restrict__ fail) {
  if (*fail) return;
  const PieceDev D = pieces[children[blockIdx.y]];
  const int a0 = blockIdx.x * kEaRows;
  if (a0 >= D.m) return;
  const PieceDev P = pieces[D.parent];
  const long long fd = (long long)D.c + D.m, fp = (long long)P.c + P.m;
  const int *__restrict__ rl = rel + D.rel_off;
  const double *__restrict__ U = F + D.off + (long long)D.c * fd + D.c;
  double *__restrict__ T = F + P.off;
  const int a1 = min(D.m, a0 + kEaRows);
  for (int a = a0; a < a1; ++a) {
    const long long ra = rl[a];
    for (int b = threadIdx.x; b <= a; b += 256) T[ra * fp + rl[b]] += U[(long long)a * fd + b];
  }
}

// ---- 64 x 64 Cholesky and triangular inverse of a workgroup, blocked by 16 (round 3).  The column-by-column form of
//      round 2 (deleted) paid a workgroup barrier per column and a 64-step dependent walk per column of the inverse:
//      83 us per diagonal block, 13 of the 21 ms of the headline's agent set-up and half of
//      sphere2500's PSD test.  Blocked: the 16 x 16 diagonal block is factored by ONE wave (LDS operations of a wave
//      stay in order: no workgroup barrier inside its 16 steps), the panel below it is a 16-step substitution per row,
//      the trailing update a rank-16 product over all threads; the inverse is four 16 x 16 inversions side by side
//      (one per wave) and three rounds of 16 x 16 block products. ----
// L: lower triangle in LDS, identity beyond the matrix' order; returns false (uniformly) on a non-positive pivot
// the value lane K of every 16-lane row holds, in all lanes of that row: DPP row_share (two 32-bit moves; a v_readlane
// goes through an SGPR and pays the VALU -> SGPR -> VALU hazard on every use)
template <int K>
__device__ __forceinline__ double row_share_k(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)b, 0x150 + K, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), 0x150 + K, 0xF, 0xF, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double row_share(double v, int k) {  // k: a constant once the caller's loops are unrolled
  switch (k & 15) {
    case 0: return row_share_k<0>(v);
    case 1: return row_share_k<1>(v);
    case 2: return row_share_k<2>(v);
    case 3: return row_share_k<3>(v);
    case 4: return row_share_k<4>(v);
    case 5: return row_share_k<5>(v);
    case 6: return row_share_k<6>(v);
    case 7: return row_share_k<7>(v);
    case 8: return row_share_k<8>(v);
    case 9: return row_share_k<9>(v);
    case 10: return row_share_k<10>(v);
    case 11: return row_share_k<11>(v);
    case 12: return row_share_k<12>(v);
    case 13: return row_share_k<13>(v);
    case 14: return row_share_k<14>(v);
    default: return row_share_k<15>(v);
  }
}
// 1 / sqrt(d) for a positive pivot: hardware estimate + two Newton steps (1-2 ulp, a dozen dependent instructions; the
// IEEE division and square root are chains of about fifty each and sat on the critical path of every pivot)
__device__ __forceinline__ double fast_rsqrt(double d) {
  double y = __builtin_amdgcn_rsq(d);
  y = y * fma(-0.5 * d * y, y, 1.5);
  y = y * fma(-0.5 * d * y, y, 1.5);
  return y;
}
// 16 x 16 x 16 product on the matrix pipe (v_mfma_f64_16x16x4_f64, four steps): D += A B with A(i, k) = fa(i, k) and
// B(k, j) = fb(k, j); at step s lane l feeds A(l & 15, 4 s + (l >> 4)) and B(4 s + (l >> 4), l & 15) and it receives
// D((l >> 4) + 4 v, l & 15) in d[v].  A result can be the B operand of the next product as it stands: step s wants rows
// 4 s + (l >> 4) of B, which is d[s].
template <class FA, class FB>
__device__ __forceinline__ v4f64 mma16(v4f64 d, FA fa, FB fb) {
  const int lane = threadIdx.x & 63, lo = lane & 15, hi = lane >> 4;
#pragma unroll
  for (int s = 0; s < 4; ++s) d = __builtin_amdgcn_mfma_f64_16x16x4f64(fa(lo, 4 * s + hi), fb(4 * s + hi, lo), d, 0, 0, 0);
  return d;
}
__device__ __forceinline__ bool blocked_potrf64(double (*L)[NB + 1], int *s_bad, double *rd, double (*Dv)[16][17]) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (tid == 0) *s_bad = 0;
  __syncthreads();
#pragma unroll 1
  for (int j0 = 0; j0 < NB; j0 += 16) {
    if (wave == 0) {
      // L D L^T elimination of the 16 x 16 block IN REGISTERS: lane i of every 16-lane row holds row i, the pivot and
      // the entries of column j travel by DPP row_share (the loops are unrolled: every register and lane index is a
      // constant) -- no LDS round trip, no barrier and no IEEE division per column.  The columns keep l_ij d_j until
      // the end, then the scaling to L L^T.  All four rows of the wave compute the same thing; the first stores.
      const int i = lane & 15;
      double x[16], rdv[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) x[k] = (k <= i) ? L[j0 + i][j0 + k] : 0.0;
      bool bad = false;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const double d = row_share(x[j], j);
        bad = bad || !(d > 0.0);  // uniform
        rdv[j] = fast_rsqrt(d);
        const double lij = x[j] * (rdv[j] * rdv[j]);
#pragma unroll
        for (int k = j + 1; k < 16; ++k) x[k] -= lij * row_share(x[j], k);
      }
      if (bad) {
        if (lane == 0) *s_bad = 1;
      } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          // row i of the Cholesky factor of the block: l_ik = (l_ik d_k) / sqrt(d_k), l_ii = d_i / sqrt(d_i)
          x[k] = (k <= i) ? x[k] * rdv[k] : 0.0;
          if (lane == 0) rd[j0 + k] = rdv[k];
          if (k <= i && lane < 16) L[j0 + i][j0 + k] = x[k];
        }
        // the inverse of the block, column `i` by forward substitution in registers; factor(r_, l) is row r_ of lane r_.
        // Kept for the panel below and for blocked_trtri64.
        double y[16];
#pragma unroll
        for (int r_ = 0; r_ < 16; ++r_) {
          double sacc = 0;
#pragma unroll
          for (int l = 0; l < 16; ++l)
            if (l < r_) {
              const double lrl = row_share(x[l], r_);
              sacc += (l >= i) ? lrl * y[l] : 0.0;
            }
          y[r_] = (r_ == i) ? rdv[r_] : (r_ > i ? -sacc * rdv[r_] : 0.0);
        }
#pragma unroll
        for (int r_ = 0; r_ < 16; ++r_)
          if (lane < 16) Dv[j0 >> 4][r_][i] = y[r_];
      }
    }
    __syncthreads();
    if (*s_bad) return false;
    const int nrem = NB - j0 - 16;
    if (nrem > 0) {
      // Round 5: panel and trailing update on the matrix pipe, a 16 x 16 block per wave (the FMA forms of round 4 -- four
      // threads per panel row, a 4 x 4 block of the update per thread -- sat on the LDS port: 6.7 us of the 45 us launch
      // were the update, 14.6 the scalar LDS loops of update + inverse).
      const int lo = lane & 15, hi = lane >> 4, r0 = j0 + 16, nbk = nrem >> 4;
      // panel: rows below times the transposed inverse of the block, X(a, k) = sum_{l <= k} B(a, l) Dinv(k, l); a wave
      // reads only the 16 rows it writes, and writes them after its products
      if (wave < nbk) {
        const int rw = r0 + 16 * wave, bq = j0 >> 4;
        const v4f64 d = mma16(
            v4f64{0, 0, 0, 0}, [&](int i, int k) { return L[rw + i][j0 + k]; },
            [&](int k, int j) { return k <= j ? Dv[bq][j][k] : 0.0; });
#pragma unroll
        for (int v = 0; v < 4; ++v) L[rw + hi + 4 * v][j0 + lo] = d[v];
      }
      __syncthreads();
      // trailing update of the lower triangle by the rank-16 product of the panel with itself: the 6 / 3 / 1 lower blocks
      // of the three steps dealt to the four waves (they read columns j0 .. j0 + 15 and write columns beyond)
      for (int tb = wave; tb < nbk * (nbk + 1) / 2; tb += 4) {
        const int bi = tb < 1 ? 0 : (tb < 3 ? 1 : 2), bj = tb - bi * (bi + 1) / 2;
        const int ia = r0 + 16 * bi, ib = r0 + 16 * bj;
        const v4f64 d = mma16(
            v4f64{0, 0, 0, 0}, [&](int i, int k) { return L[ia + i][j0 + k]; },
            [&](int k, int j) { return L[ib + j][j0 + k]; });
#pragma unroll
        for (int v = 0; v < 4; ++v)
          if (ib + lo <= ia + hi + 4 * v) L[ia + hi + 4 * v][ib + lo] -= d[v];
      }
      __syncthreads();
    }
  }
  return true;
}
// Li = L^-1 (both lower triangular in LDS)
__device__ __forceinline__ void blocked_trtri64(double (*L)[NB + 1], double (*Li)[NB + 1],
                                                const double (*Dv)[16][17] /* inverses of the diagonal blocks */) {
  const int tid = threadIdx.x;
  for (int e = tid; e < NB * NB; e += 256) {
    const int r_ = e >> 6, c_ = e & 63;
    if (c_ > r_ || (r_ >> 4) != (c_ >> 4)) Li[r_][c_] = 0.0;  // above the diagonal and the off-diagonal blocks
  }
  // the diagonal blocks' inverses come from the factorisation (blocked_potrf64)
  for (int e = tid; e < 4 * 256; e += 256) {
    const int bq = e >> 8, a = (e >> 4) & 15, c_ = e & 15;
    if (c_ <= a) Li[16 * bq + a][16 * bq + c_] = Dv[bq][a][c_];
  }
  __syncthreads();
  // block (bi, bj), bi - bj = dist:  Li_ij = -Li_ii (sum_{bk = bj}^{bi - 1} L_i,bk Li_bk,j): one wave per block, both
  // products on the matrix pipe; the inner sum stays in registers (a result is the next product's B operand as it
  // stands), so a distance costs one barrier where the FMA form of round 4 paid two and 32 LDS reads per output
  const int wave = tid >> 6, lo = tid & 15, hi = (tid & 63) >> 4;
  for (int dist = 1; dist < 4; ++dist) {
    if (wave < 4 - dist) {
      const int bj = wave, bi = wave + dist;
      v4f64 t{0, 0, 0, 0};
      for (int bk = bj; bk < bi; ++bk)
        t = mma16(
            t, [&](int i, int k) { return L[16 * bi + i][16 * bk + k]; },
            [&](int k, int j) { return Li[16 * bk + k][16 * bj + j]; });
      v4f64 d{0, 0, 0, 0};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = 4 * s + hi;
        d = __builtin_amdgcn_mfma_f64_16x16x4f64(k <= lo ? Li[16 * bi + lo][16 * bi + k] : 0.0, t[s], d, 0, 0, 0);
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) Li[16 * bi + hi + 4 * v][16 * bj + lo] = -d[v];
    }
    __syncthreads();
  }
}

// diagonal block of the current panel, blocked form (see above): LL^T of up to 64 columns, written back in place, and
// L^-1 for the panel below; a pivot that is not positive raises *fail
__global__ __launch_bounds__(256) void k_chol_potrf(const PieceDev *__restrict__ pieces, const int *__restrict__ list,
                                                    int j0, double *__restrict__ F, double *__restrict__ Linv,
                                                    int *__restrict__ fail, double *__restrict__ logdet,
                                                    int always_inv) {
  if (*fail) return;
  const PieceDev P = pieces[list[blockIdx.x]];
  const int jb = min(NB, P.c - j0);
  const long long f = (long long)P.c + P.m;
  double *__restrict__ M = F + P.off + (long long)j0 * f + j0;
  __shared__ double L[NB][NB + 1];
  __shared__ double Li[NB][NB + 1];
  __shared__ double rd[NB];
  __shared__ double Dv[4][16][17];
  __shared__ int s_bad;
  const int tid = threadIdx.x;
  for (int e = tid; e < NB * NB; e += 256) {
    const int i = e >> 6, j = e & 63;
    L[i][j] = (i < jb && j <= i) ? M[(long long)i * f + j] : (i == j ? 1.0 : 0.0);
  }
  if (!blocked_potrf64(L, &s_bad, rd, Dv)) {
    if (tid == 0) *fail = 1;
    return;
  }
  if (tid < NB) {
    // log det of the factored matrix (a cross-check of the whole factorisation for the tests; order of the sum free)
    double lg = tid < jb ? 2.0 * log(L[tid][tid]) : 0.0;
    for (int o = 32; o > 0; o >>= 1) lg += __shfl_xor(lg, o);
    if (tid == 0) atomicAdd(logdet, lg);
  }
  for (int e = tid; e < jb * jb; e += 256) {
    const int r_ = e / jb, j = e - r_ * jb;
    if (j <= r_) M[(long long)r_ * f + j] = L[r_][j];
  }
  if (!always_inv && P.m == 0 && j0 + jb >= P.c) return;  // nothing below the last panel of a root
  blocked_trtri64(L, Li, Dv);
  double *__restrict__ O = Linv + (size_t)blockIdx.x * NB * NB;
  for (int e = tid; e < NB * NB; e += 256) O[e] = Li[e >> 6][e & 63];
}

constexpr int chol_superpanel_blocks() { return 8; }  // measured: 4 -> 157 ms, 8 -> 99 ms (1: a trailing update per block, 217)

// panel below the diagonal block:  X = B L^-T, 64 rows per workgroup, in place
__global__ __launch_bounds__(256) void k_chol_trsm(const PieceDev *__restrict__ pieces, const int *__restrict__ list,
                                                   int j0, double *__restrict__ F, const double *__restrict__ Linv,
                                                   const int *__restrict__ fail) {
  if (*fail) return;
  const PieceDev P = pieces[list[blockIdx.y]];
  const int jb = min(NB, P.c - j0);
  const int f = P.c + P.m;
  const int r0 = j0 + jb + NB * blockIdx.x;
  if (r0 >= f) return;
  __shared__ double As[NB][NB + 1];
  __shared__ double Bs[NB][NB + 1];
  double *__restrict__ A = F + P.off + (long long)r0 * f + j0;
  double acc[4][4];
  chol_tile_product(A, f, min(NB, f - r0), Linv + (size_t)blockIdx.y * NB * NB, NB, jb, jb, As, Bs, acc);
  __syncthreads();  // the tile is overwritten in place: every read of it (into LDS) is behind us
  for_each_acc(acc, [&](int i, int j, double s) {
    if (r0 + i < f && j < jb) A[(long long)i * f + j] = s;
  });
}

// trailing update: C(ti, tj) -= sum_{l in [k0, base)} X(ti, l) X(tj, l) over 64 x 64 tiles of the lower triangle behind
// base = min(kcap, c).  Two uses (build_image):
//   inside a super-panel (ncb > 0): K = one 64-column block, only the ncb column blocks of the super-panel that are
//     still to be factored are updated (columns < min(ccap, c)), blockIdx.x = ti ncb + tj;
//   behind a super-panel (ncb = 0): K = the whole super-panel (up to 256 columns in 64-column steps through LDS), every
//     tile of the trailing matrix, blockIdx.x = triangular index.  A rank-256 update reads and writes the trailing
//     matrix once where four rank-64 updates did four times: the update is bound by exactly that traffic.
__global__ __launch_bounds__(256) void k_chol_syrk(const PieceDev *__restrict__ pieces, const int *__restrict__ list,
                                                   int k0, int kcap, int ccap, int ncb, double *__restrict__ F,
                                                   const int *__restrict__ fail) {
  if (*fail) return;
  const PieceDev P = pieces[list[blockIdx.y]];
  const int f = P.c + P.m;
  const int base = min(kcap, P.c);
  if (base <= k0) return;
  const int colend = ccap >= 0 ? min(ccap, P.c) : f;
  int ti, tj;
  if (ncb > 0) {
    ti = blockIdx.x / ncb;
    tj = blockIdx.x - ti * ncb;
    if (tj > ti) return;
  } else {
    ti = (int)((sqrtf(8.0f * (float)blockIdx.x + 1.0f) - 1.0f) * 0.5f);
    while ((ti + 1) * (ti + 2) / 2 <= (int)blockIdx.x) ++ti;
    while (ti * (ti + 1) / 2 > (int)blockIdx.x) --ti;
    tj = blockIdx.x - ti * (ti + 1) / 2;
  }
  const int ri0 = base + NB * ti, cj0 = base + NB * tj;
  if (ri0 >= f || cj0 >= colend) return;
  __shared__ double As[NB][NB + 1];
  __shared__ double Bs[NB][NB + 1];
  double *__restrict__ M = F + P.off;
  double acc[4][4];
  zero_acc(acc);
  tile_product_range(M + (long long)ri0 * f, f, min(NB, f - ri0), M + (long long)cj0 * f, f, min(NB, f - cj0), k0, base,
                     As, Bs, acc);
  for_each_acc(acc, [&](int i, int j, double s) {
    const int r = ri0 + i, c = cj0 + j;
    if (r < f && c <= r && c < colend) M[(long long)r * f + c] -= s;
  });
}

__global__ __launch_bounds__(256) void k_count_nonzero(long long n, const double *__restrict__ v,
                                                       unsigned long long *__restrict__ out) {
  unsigned long long c = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) c += v[i] != 0.0;
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}

// the first c columns of every front (diagonal block over the rows below), packed piece after piece
__global__ __launch_bounds__(256) void k_chol_pack(const PieceDev *__restrict__ pieces,
                                                   const long long *__restrict__ panel_off,
                                                   const double *__restrict__ F, double *__restrict__ out) {
  const PieceDev P = pieces[blockIdx.y];
  const int f = P.c + P.m, c = P.c;
  const long long n = (long long)f * c;
  const double *__restrict__ M = F + P.off;
  double *__restrict__ O = out + panel_off[blockIdx.y];
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    const int i = (int)(e / c), j = (int)(e - (long long)i * c);
    O[e] = (i >= c || j <= i) ? M[(long long)i * f + j] : 0.0;
  }
}

// ---- the NARROW pieces (c <= 64: the leaves and the small separators, thousands of them) all at once; the wider ones go
//      through the job list of dense_inverse.hip ----
// rows [0, c) of the packed panel <- L11^-1 (lower triangle): one workgroup per piece
__global__ __launch_bounds__(256) void k_small_inv(const PieceDev *__restrict__ pieces, const int *__restrict__ list,
                                                   const long long *__restrict__ panel_off,
                                                   const double *__restrict__ F, double *__restrict__ out,
                                                   const long long *__restrict__ m_off, double *__restrict__ Mout) {
  __shared__ double T[NB][NB + 1];
  __shared__ double Li[NB][NB + 1];
  const int s = list[blockIdx.x];
  const PieceDev P = pieces[s];
  const int c = P.c;
  const long long f = (long long)P.c + P.m;
  const double *__restrict__ L = F + P.off;
  const int tid = threadIdx.x;
  for (int e = tid; e < NB * NB; e += 256) {
    const int i = e >> 6, j = e & 63;
    T[i][j] = (i < c && j <= i) ? L[(long long)i * f + j] : (i == j ? 1.0 : 0.0);
  }
  tri_inv64_lds(T, Li);
  double *__restrict__ O = out + panel_off[s];
  for (int e = tid; e < c * c; e += 256) {
    const int i = e / c, j = e - i * c;
    O[e] = j <= i ? Li[i][j] : 0.0;
  }
  if (Mout) {  // M = L11^-T L11^-1, both triangles: M(a, b) = sum_{i >= max(a, b)} Li(i, a) Li(i, b), i ascending
    double *__restrict__ Mo = Mout + m_off[s];
    for (int e = tid; e < c * c; e += 256) {
      const int a = e / c, b = e - a * c;
      double sum = 0;
      for (int i = max(a, b); i < c; ++i) sum += Li[i][a] * Li[i][b];
      Mo[e] = sum;
    }
  }
}
// rows [c, c + m) of the packed panel <- W = -L21 L11^-1: 64 rows below per workgroup (blockIdx.x), piece blockIdx.y
__global__ __launch_bounds__(256) void k_small_w(const PieceDev *__restrict__ pieces, const int *__restrict__ list,
                                                 const long long *__restrict__ panel_off,
                                                 const double *__restrict__ F, double *__restrict__ out) {
  const int s = list[blockIdx.y];
  const PieceDev P = pieces[s];
  const int c = P.c, m = P.m, a0 = blockIdx.x * NB;
  if (a0 >= m) return;
  __shared__ double As[NB][NB + 1];
  __shared__ double Bs[NB][NB + 1];
  const long long f = (long long)c + m;
  const double *__restrict__ B = F + P.off + (long long)(c + a0) * f;
  double *__restrict__ O = out + panel_off[s];
  const int na = min(NB, m - a0);
  const int tid = threadIdx.x;
  for (int e = tid; e < NB * NB; e += 256) {
    const int i = e >> 6, kk = e & 63;
    As[kk][i] = (i < na && kk < c) ? B[(long long)i * f + kk] : 0.0;  // L21(a0 + i, kk)
    Bs[i][kk] = (i < c && kk <= i) ? O[(long long)i * c + kk] : 0.0;  // L11^-1(i, kk): [summed index][column]
  }
  __syncthreads();
  double acc[4][4];
  zero_acc(acc);
  tile_inner(As, Bs, acc);
  for_each_acc(acc, [&](int a, int j, double sum) {
    if (a < na && j < c) O[(long long)(c + a0 + a) * c + j] = -sum;
  });
}

inline uint64_t mix64(uint64_t h, uint64_t w) {
  h ^= w;
  h *= 0x9E3779B97F4A7C15ull;
  h ^= h >> 29;
  return h;
}
void hash_ints(const int *p, size_t n, uint64_t *h0, uint64_t *h1) {
  size_t i = 0;
  for (; i + 2 <= n; i += 2) {
    uint64_t w;
    std::memcpy(&w, p + i, 8);
    *h0 = mix64(*h0, w);
    *h1 = mix64(*h1 + 0xD1B54A32D192ED03ull, w ^ (*h0 >> 7));
  }
  uint64_t w = (i < n) ? (uint64_t)(unsigned)p[i] : 0x5bd1e995ull;
  *h0 = mix64(*h0, w ^ n);
  *h1 = mix64(*h1, w + n);
}

struct Launch {
  int kind;  // 0 extend-add, 1 potrf, 2 trsm, 3 syrk
  int list;  // offset into the device list (children or level pieces)
  int gx, gy, j0;
  int kcap = 0, ccap = -1, ncb = 0;  // syrk: K range [j0, min(kcap, c)), column cap (-1: the whole trailing matrix), column blocks
};

struct CholImage {
  std::mutex mu;  // one factorisation at a time per image (arena, values and flags are the image's)
  int device = 0;
  CholSymbolic sym;
  DevBuf<PieceDev> pieces;
  DevBuf<int> rel, lists;  // lists = level_pieces followed by slot_children
  DevBuf<long long> dest;
  DevBuf<double> linv, arena, vals;
  DevBuf<int> fail;
  DevBuf<double> logdet;
  std::vector<Launch> plan;
  double symbolic_ms = 0;
  size_t table_bytes = 0;
  // pinned staging for the values of a factorisation: the copy from the caller's pageable array took 16 - 26 ms now and
  // then (1.3 MB at k = 10 000, inside the certificate's clock) where a copy through this buffer takes 0.1 ms
  double *vals_pinned = nullptr;
  ~CholImage() {
    if (vals_pinned) (void)hipHostFree(vals_pinned);
  }
};

struct CacheSlot {
  uint64_t h0, h1;
  int n, nnz, block, device, top;
  std::shared_ptr<CholImage> img;
};
std::mutex g_mu;
std::list<CacheSlot> g_cache;

int build_image(const HostCsr &A, int block, int top, int device, std::shared_ptr<CholImage> *out) {
  auto img = std::make_shared<CholImage>();
  img->device = device;
  const auto t0 = std::chrono::steady_clock::now();
  chol_symbolic(A, block, &img->sym, top);
  const CholSymbolic &S = img->sym;
  const int np = (int)S.pieces.size();
  std::vector<PieceDev> pd((size_t)np);
  for (int s = 0; s < np; ++s) {
    pd[s].off = S.pieces[s].off;
    pd[s].c = S.pieces[s].c;
    pd[s].m = S.pieces[s].m;
    pd[s].parent = S.pieces[s].parent;
    pd[s].rel_off = S.pieces[s].rows_off;
  }
  std::vector<int> lists(S.level_pieces);
  const int child_base = (int)lists.size();
  lists.insert(lists.end(), S.slot_children.begin(), S.slot_children.end());
  int max_level_count = 1;
  for (int t = 0; t < S.nlev; ++t) {
    max_level_count = std::max(max_level_count, S.level_ptr[t + 1] - S.level_ptr[t]);
    for (int sl = S.slot_level_ptr[t]; sl < S.slot_level_ptr[t + 1]; ++sl) {
      const int first = S.slot_ptr[sl], count = S.slot_ptr[sl + 1] - first;
      int maxm = 0;
      for (int q = 0; q < count; ++q) maxm = std::max(maxm, S.pieces[S.slot_children[first + q]].m);
      if (count > 0 && maxm > 0)
        img->plan.push_back(Launch{0, child_base + first, (maxm + kEaRows - 1) / kEaRows, count, 0});
    }
    const int lp = S.level_ptr[t], ln = S.level_ptr[t + 1] - lp;
    const int cmax = S.pieces[S.level_pieces[lp]].c;
    // super-panels of spb 64-column blocks: inside one, a factored block updates only the column blocks of the
    // super-panel that are still to come; behind it, ONE update of rank 64 spb sweeps the trailing matrix
    const int spb = chol_superpanel_blocks(), spw = spb * NB;
    for (int s0 = 0; s0 < cmax; s0 += spw) {
      int active0 = 0, maxrows2 = 0;
      while (active0 < ln && S.pieces[S.level_pieces[lp + active0]].c > s0) {
        const CholPiece &P = S.pieces[S.level_pieces[lp + active0]];
        maxrows2 = std::max(maxrows2, P.c + P.m - std::min(s0 + spw, P.c));
        ++active0;
      }
      for (int j0 = s0; j0 < std::min(cmax, s0 + spw); j0 += NB) {
        int active = 0, maxrows = 0, maxrows_block = 0;
        while (active < ln && S.pieces[S.level_pieces[lp + active]].c > j0) {
          const CholPiece &P = S.pieces[S.level_pieces[lp + active]];
          const int base = j0 + std::min(NB, P.c - j0);
          maxrows = std::max(maxrows, P.c + P.m - base);
          maxrows_block = std::max(maxrows_block, P.c + P.m - j0);
          ++active;
        }
        // left-looking inside the super-panel: before block j0 is factored, its 64 columns (all rows from j0 down) take
        // ONE update of rank j0 - s0 from the blocks of the super-panel already factored -- the same flops as a rank-64
        // update of the remaining blocks after every block, but the column block is read and written once and the K
        // loop runs pipelined over up to 7 steps (13 -> 30 Tflop/s on these launches)
        if (spb > 1 && j0 > s0)
          img->plan.push_back(Launch{3, lp, (maxrows_block + NB - 1) / NB, active, s0, j0, j0 + NB, 1});
        img->plan.push_back(Launch{1, lp, active, 1, j0});
        if (maxrows > 0) {
          const int T = (maxrows + NB - 1) / NB;
          img->plan.push_back(Launch{2, lp, T, active, j0});
          if (spb == 1) img->plan.push_back(Launch{3, lp, T * (T + 1) / 2, active, j0, j0 + NB, -1, 0});
        }
      }
      if (spb > 1 && maxrows2 > 0) {
        const int T = (maxrows2 + NB - 1) / NB;
        img->plan.push_back(Launch{3, lp, T * (T + 1) / 2, active0, s0, s0 + spw, -1, 0});
      }
    }
  }
  img->symbolic_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  DCORA_HIP(img->pieces.alloc(pd.size()));
  DCORA_HIP(hipMemcpy(img->pieces.p, pd.data(), pd.size() * sizeof(PieceDev), hipMemcpyHostToDevice));
  DCORA_HIP(img->rel.alloc(std::max<size_t>(1, S.rel.size())));
  if (!S.rel.empty()) DCORA_HIP(hipMemcpy(img->rel.p, S.rel.data(), S.rel.size() * sizeof(int), hipMemcpyHostToDevice));
  DCORA_HIP(img->lists.alloc(lists.size()));
  DCORA_HIP(hipMemcpy(img->lists.p, lists.data(), lists.size() * sizeof(int), hipMemcpyHostToDevice));
  DCORA_HIP(img->dest.alloc(S.a_dest.size()));
  DCORA_HIP(hipMemcpy(img->dest.p, S.a_dest.data(), S.a_dest.size() * sizeof(long long), hipMemcpyHostToDevice));
  DCORA_HIP(img->linv.alloc((size_t)max_level_count * NB * NB));
  DCORA_HIP(img->vals.alloc(S.a_dest.size()));
  // (small problems only: there the stall of a pageable copy is the factorisation's whole time several times over; an
  // image of the 100k lattice would pin 80 MB per cached pattern)
  if (S.a_dest.size() * sizeof(double) <= ((size_t)32 << 20) &&
      hipHostMalloc((void **)&img->vals_pinned, (S.a_dest.size() + 2) * sizeof(double), hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    img->vals_pinned = nullptr;  // the pageable copy below still works
  }
  DCORA_HIP(img->fail.alloc(1));
  DCORA_HIP(img->logdet.alloc(1));
  img->table_bytes = pd.size() * sizeof(PieceDev) + (S.rel.size() + lists.size()) * sizeof(int) +
                     S.a_dest.size() * (sizeof(long long) + sizeof(double)) + (size_t)max_level_count * NB * NB * 8;
  *out = img;
  return DCORA_OK;
}

// arenas up to this many bytes stay with the cached image (allocating and freeing tens of GB per factorisation costs
// more than the factorisation); larger ones are allocated per call.  Default: a quarter of the device's memory.
size_t arena_keep_bytes() {
  static const size_t b = [] {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return (size_t)2048 << 20;
    return tot / 4;
  }();
  return b;
}

}  // namespace

void scratch_clear();  // dense_inverse.hip: the dense builds' recycled arenas

void chol_cache_clear() {
  std::lock_guard<std::mutex> lk(g_mu);
  g_cache.clear();
  scratch_clear();
}

int device_chol_prepare(const HostCsr &A, int block, int device) {
  if (A.n <= 0 || (int)A.rp.size() != A.n + 1) {
    set_last_error("sparse Cholesky: empty or malformed matrix");
    return DCORA_ERR_BAD_ARG;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    set_last_error("no HIP device available: libdcora_hip has no CPU fallback");
    return DCORA_ERR_NO_DEVICE;
  }
  DCORA_HIP(hipSetDevice(device));
  uint64_t h0 = 0x243F6A8885A308D3ull, h1 = 0x13198A2E03707344ull;
  hash_ints(A.rp.data(), A.rp.size(), &h0, &h1);
  hash_ints(A.ci.data(), A.ci.size(), &h0, &h1);
  {
    std::lock_guard<std::mutex> lk(g_mu);
    for (const CacheSlot &c : g_cache)
      if (c.h0 == h0 && c.h1 == h1 && c.n == A.n && c.nnz == A.nnz() && c.block == block && c.device == device)
        return DCORA_OK;  // any order serves a verdict
  }
  std::shared_ptr<CholImage> img;
  const int rc = build_image(A, block, 0, device, &img);
  if (rc) return rc;
  const size_t arena_bytes = (size_t)img->sym.arena * sizeof(double);
  if (arena_bytes <= arena_keep_bytes() / 4 && !img->arena.p) DCORA_HIP(img->arena.alloc((size_t)img->sym.arena));
  std::lock_guard<std::mutex> lk(g_mu);
  g_cache.push_front(CacheSlot{h0, h1, A.n, A.nnz(), block, device, 0, img});
  while (g_cache.size() > 8) g_cache.pop_back();
  if (env::init_timing())
    fprintf(stderr, "[factor] prepared: n %d nnz %d block %d, %zu cached, key %016llx\n", A.n, A.nnz(), block, g_cache.size(),
            (unsigned long long)h0);
  return DCORA_OK;
}

namespace {
using Clock = std::chrono::steady_clock;
double ms_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// ---- step 1: the image of the pattern, from the cache or built (and cached) now ----
int find_or_build_image(const HostCsr &A, int block, int top, int device, bool any_order,
                        std::shared_ptr<CholImage> *out, bool *hit) {
  uint64_t h0 = 0x243F6A8885A308D3ull, h1 = 0x13198A2E03707344ull;
  hash_ints(A.rp.data(), A.rp.size(), &h0, &h1);
  hash_ints(A.ci.data(), A.ci.size(), &h0, &h1);
  std::shared_ptr<CholImage> img;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    // a verdict alone (no panels asked for) does not care about the order: an analysis of the same pattern made for
    // the preconditioner (dense top, device_chol.h) serves the PSD test of S = Q - Lambda, which has Q's pattern --
    // the certificate of the 100k lattice saves the 0.25 s analysis and a second 18 GB arena
    for (int pass = 0; pass < (any_order ? 2 : 1) && !img; ++pass)
      for (auto it = g_cache.begin(); it != g_cache.end(); ++it)
        if (it->h0 == h0 && it->h1 == h1 && it->n == A.n && it->nnz == A.nnz() && it->block == block &&
            it->device == device && (it->top == top || pass == 1)) {
          g_cache.splice(g_cache.begin(), g_cache, it);
          img = g_cache.front().img;
          break;
        }
  }
  *hit = img != nullptr;
  if (env::init_timing())
    fprintf(stderr, "[factor] look-up: %s (n %d nnz %d block %d top %d, %zu cached, key %016llx)\n", img ? "hit" : "MISS", A.n,
            A.nnz(), block, top, g_cache.size(), (unsigned long long)h0);
  if (!img) {
    const int rc = build_image(A, block, top, device, &img);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(g_mu);
    g_cache.push_front(CacheSlot{h0, h1, A.n, A.nnz(), block, device, top, img});
    while (g_cache.size() > 8) g_cache.pop_back();
  }
  *out = img;
  return DCORA_OK;
}

// ---- step 2: the arena of the fronts: the image's own (kept between factorisations) or one for this call ----
int choose_arena(const std::shared_ptr<CholImage> &img, DevBuf<double> *local, double **F) {
  const size_t doubles = (size_t)img->sym.arena, bytes = doubles * sizeof(double);
  if (bytes > arena_keep_bytes()) {
    DCORA_HIP(local->alloc(doubles));
    *F = local->p;
    return DCORA_OK;
  }
  if (!img->arena.p) {
    // the arenas kept by all cached images together stay within the same bound: idle images give theirs up
    std::lock_guard<std::mutex> lk(g_mu);
    size_t held = bytes;
    for (CacheSlot &c : g_cache)
      if (c.img != img && c.img->arena.p) {
        held += c.img->arena.n * sizeof(double);
        if (held > arena_keep_bytes() && c.img->mu.try_lock()) {
          held -= c.img->arena.n * sizeof(double);
          c.img->arena.release();
          c.img->mu.unlock();
        }
      }
  }
  if (!img->arena.p) DCORA_HIP(img->arena.alloc(doubles));
  *F = img->arena.p;
  return DCORA_OK;
}

// ---- step 3: the numeric factorisation, enqueued, and its verdict ----
struct EnqueueClock {
  Clock::time_point start, copied, zeroed, enqueued;
};
// vals_dev (may be null): the values in A's CSR order, already on the device and complete once `ready` (may be null: now)
// has passed; A then carries the pattern alone
int enqueue_factorisation(CholImage &img, hipStream_t st, double *F, const HostCsr &A, const double *vals_dev,
                          hipEvent_t ready, EnqueueClock *clk) {
  const long long nnz = (long long)img.sym.a_dest.size();
  clk->start = Clock::now();
  const double *vin = img.vals.p;  // what k_chol_scatter reads
  if (vals_dev) {
    if (ready) DCORA_HIP(hipStreamWaitEvent(st, ready, 0));
    vin = vals_dev;
  } else {
    const double *vsrc = A.v.data();
    if (img.vals_pinned) {
      std::memcpy(img.vals_pinned, A.v.data(), (size_t)nnz * sizeof(double));
      vsrc = img.vals_pinned;
    }
    DCORA_HIP(hipMemcpyAsync(img.vals.p, vsrc, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, st));
  }
  clk->copied = Clock::now();
  DCORA_HIP(hipMemsetAsync(F, 0, (size_t)img.sym.arena * sizeof(double), st));
  clk->zeroed = Clock::now();
  DCORA_HIP(hipMemsetAsync(img.fail.p, 0, sizeof(int), st));
  DCORA_HIP(hipMemsetAsync(img.logdet.p, 0, sizeof(double), st));
  hipLaunchKernelGGL(k_chol_scatter, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, nnz, img.dest.p, vin, F);
  for (const Launch &L : img.plan) {
    const int *list = img.lists.p + L.list;
    switch (L.kind) {
      case 0:
        hipLaunchKernelGGL(k_chol_extend_add, dim3(L.gx, L.gy), dim3(256), 0, st, img.pieces.p, list, img.rel.p, F,
                           img.fail.p);
        break;
      case 1:
        hipLaunchKernelGGL(k_chol_potrf, dim3(L.gx), dim3(256), 0, st, img.pieces.p, list, L.j0, F, img.linv.p,
                           img.fail.p, img.logdet.p, 0);
        break;
      case 2:
        hipLaunchKernelGGL(k_chol_trsm, dim3(L.gx, L.gy), dim3(256), 0, st, img.pieces.p, list, L.j0, F, img.linv.p,
                           img.fail.p);
        break;
      default:
        hipLaunchKernelGGL(k_chol_syrk, dim3(L.gx, L.gy), dim3(256), 0, st, img.pieces.p, list, L.j0, L.kcap, L.ccap,
                           L.ncb, F, img.fail.p);
        break;
    }
  }
  DCORA_HIP(hipGetLastError());
  clk->enqueued = Clock::now();
  return DCORA_OK;
}
int read_verdict(CholImage &img, hipStream_t st, int *failed, double *logdet) {
  if (img.vals_pinned) {  // (the verdict comes back through the pinned buffer's tail: see CholImage)
    double *tail = img.vals_pinned + img.sym.a_dest.size();
    DCORA_HIP(hipMemcpyAsync(tail, img.fail.p, sizeof(int), hipMemcpyDeviceToHost, st));
    DCORA_HIP(hipMemcpyAsync(tail + 1, img.logdet.p, sizeof(double), hipMemcpyDeviceToHost, st));
    DCORA_HIP(hipStreamSynchronize(st));
    std::memcpy(failed, tail, sizeof(int));
    *logdet = tail[1];
  } else {
    DCORA_HIP(hipMemcpyAsync(failed, img.fail.p, sizeof(int), hipMemcpyDeviceToHost, st));
    DCORA_HIP(hipMemcpyAsync(logdet, img.logdet.p, sizeof(double), hipMemcpyDeviceToHost, st));
    DCORA_HIP(hipStreamSynchronize(st));
  }
  return DCORA_OK;
}

// ---- step 4: the factor handed over by pieces: packed on the device, the pieces inverted there by class, one copy to
//      the host ----
// one host block for all panels (and the wide pieces' M): not value-initialised -- the copy writes every entry, and
// zeroing 3 GB first cost 0.76 s for the whole 100k lattice -- and handed to the pieces as views
struct HostBlock {
  double *panels = nullptr, *M = nullptr;
  void *m_tokens = nullptr;  // reserved, unreadable addresses standing for the M that exist on the device only
  size_t m_tokens_bytes = 0;
  DevBuf<double> dev_panels, dev_M;  // device sources of a sink that fills on the device
  ~HostBlock() {
    std::free(panels);
    std::free(M);
    if (m_tokens) munmap(m_tokens, m_tokens_bytes);
  }
};
// 2 MB-aligned and advised as huge pages: first touch and release of 3 GB in 4 KB pages cost 0.4 s each
double *huge_alloc(size_t doubles) {
  const size_t two_mb = (size_t)2 << 20;
  const size_t bytes = ((std::max<size_t>(doubles, 1) * sizeof(double) + two_mb - 1) / two_mb) * two_mb;
  void *p = std::aligned_alloc(two_mb, bytes);
  if (p) (void)madvise(p, bytes, MADV_HUGEPAGE);
  return (double *)p;
}

constexpr int kWide = 384;  // pieces of at least this many columns are inverted one after the other
int piece_class(const CholPiece &P) { return P.c <= NB ? 0 : (P.c < kWide ? 1 : 2); }  // narrow, mid, wide

struct HandOver {
  CholImage &img;
  hipStream_t st;
  const double *F;
  std::vector<long long> poff, moff;  // per piece: its packed panel; its M or -1
  long long mtotal = 0;
  DevBuf<long long> dpoff, dmoff;
  DevBuf<double> packed, mall;  // the panels; with device sources the M of every piece
};

// the narrow pieces by two batched launches
int invert_narrow_pieces(HandOver &h, const std::vector<int> &narrow, bool want_m) {
  if (narrow.empty()) return DCORA_OK;
  int mmax = 0;
  for (int s : narrow) mmax = std::max(mmax, h.img.sym.pieces[s].m);
  DevBuf<int> dlist;
  DCORA_HIP(dlist.alloc(narrow.size()));
  DCORA_HIP(hipMemcpyAsync(dlist.p, narrow.data(), narrow.size() * sizeof(int), hipMemcpyHostToDevice, h.st));
  hipLaunchKernelGGL(k_small_inv, dim3((unsigned)narrow.size()), dim3(256), 0, h.st, h.img.pieces.p, dlist.p, h.dpoff.p, h.F,
                     h.packed.p, (const long long *)h.dmoff.p, want_m ? h.mall.p : (double *)nullptr);
  if (mmax > 0)
    hipLaunchKernelGGL(k_small_w, dim3((mmax + NB - 1) / NB, (unsigned)narrow.size()), dim3(256), 0, h.st, h.img.pieces.p,
                       dlist.p, h.dpoff.p, h.F, h.packed.p);
  DCORA_HIP(hipStreamSynchronize(h.st));  // dlist lives on this frame
  return DCORA_OK;
}
// wider pieces through the job list (enqueue_inverse_jobs).  together: ONE batch, a piece per blockIdx.z, their scratch
// side by side (the two thousand pieces of 64 < c < 384 columns of the whole 100k lattice in 15 launches); otherwise a
// batch per piece, one after the other in the scratch of the widest.  M (may be null) receives the M of the pieces whose
// moff is set.
int invert_pieces(HandOver &h, const std::vector<int> &which, bool together, double *M) {
  if (which.empty()) return DCORA_OK;
  std::vector<InvJob> jobs;
  long long yt_total = 0, tinv_total = 0;
  int cmax = 0, mmax = 0;
  for (int s : which) {
    const CholPiece &P = h.img.sym.pieces[s];
    const long long yt = (long long)P.c * P.c, tinv = (long long)((P.c + NB - 1) / NB) * NB * NB;
    jobs.push_back(InvJob{P.c, P.m, P.c, P.off, (long long)P.c + P.m, together ? yt_total : 0, together ? tinv_total : 0,
                          h.poff[s], h.moff[s]});
    yt_total = together ? yt_total + yt : std::max(yt_total, yt);
    tinv_total = together ? tinv_total + tinv : std::max(tinv_total, tinv);
    cmax = std::max(cmax, P.c);
    mmax = std::max(mmax, P.m);
  }
  DevBuf<InvJob> djobs;
  DevBuf<double> yt, tinv;
  DCORA_HIP(djobs.alloc(jobs.size()));
  DCORA_HIP(yt.alloc((size_t)yt_total));
  DCORA_HIP(tinv.alloc((size_t)tinv_total));
  DCORA_HIP(hipMemcpyAsync(djobs.p, jobs.data(), jobs.size() * sizeof(InvJob), hipMemcpyHostToDevice, h.st));
  InvBatch b;
  b.F = h.F;
  b.yt = yt.p;
  b.tinv = tinv.p;
  b.packed = h.packed.p;
  b.M = M;
  b.want_m = M != nullptr;
  if (together) {
    b.jobs = djobs.p;
    b.count = (int)jobs.size();
    b.cmax = cmax;
    b.mmax = mmax;
    DCORA_HIP(hipMemsetAsync(yt.p, 0, (size_t)yt_total * sizeof(double), h.st));
    enqueue_inverse_jobs(h.st, b);
  } else {
    for (size_t q = 0; q < jobs.size(); ++q) {
      b.jobs = djobs.p + q;
      b.count = 1;
      b.cmax = jobs[q].c;
      b.mmax = jobs[q].m;
      DCORA_HIP(hipMemsetAsync(yt.p, 0, (size_t)jobs[q].c * jobs[q].c * sizeof(double), h.st));
      enqueue_inverse_jobs(h.st, b);
    }
  }
  DCORA_HIP(hipGetLastError());
  DCORA_HIP(hipStreamSynchronize(h.st));  // the job list and the scratch live on this frame
  return DCORA_OK;
}

int hand_over_panels(CholImage &img, hipStream_t st, const double *F, PiecewiseFactor *panels) {
  const CholSymbolic &S = img.sym;
  const bool init_timing = env::init_timing();
  auto tl = Clock::now();
  auto lap = [&](const char *what) {
    if (!init_timing) return;
    const auto now = Clock::now();
    fprintf(stderr, "[factor] %-26s %9.1f ms\n", what, ms_between(tl, now));
    tl = now;
  };
  const int np = (int)S.pieces.size();
  HandOver h{img, st, F};
  h.poff.assign((size_t)np + 1, 0);
  h.moff.assign((size_t)np, -1);
  int fmax = 1;
  for (int s = 0; s < np; ++s) {
    const CholPiece &P = S.pieces[s];
    h.poff[s + 1] = h.poff[s] + (long long)(P.c + P.m) * P.c;
    fmax = std::max(fmax, P.c + P.m);
  }
  const long long ptotal = h.poff[np];
  DCORA_HIP(h.dpoff.alloc(h.poff.size()));
  DCORA_HIP(h.packed.alloc((size_t)std::max<long long>(1, ptotal)));
  DCORA_HIP(hipMemcpyAsync(h.dpoff.p, h.poff.data(), h.poff.size() * sizeof(long long), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_chol_pack, dim3(std::min(64, (fmax + 7) / 8), np), dim3(256), 0, st, img.pieces.p, h.dpoff.p, F,
                     h.packed.p);
  // Without hubs every piece arrives inverted, the inverses formed here instead of by the host's threads (for the whole
  // 100k lattice 310 Gflop, 7.7 s on 16 cores): the narrow ones (c <= 64) by two batched launches, the ones up to 384
  // columns in one batch of the right-looking kernels, the wide ones one after the other.
  const bool inverted = S.nhub == 0;
  // device sources (asked for by the caller whose weight sink fills on the device): the M = L11^-T L11^-1 of every piece
  // is formed here as well and stays here, like the panels; otherwise only the wide pieces' M, which go to the host --
  // the schedule (host_partinv3.cpp) applies the two triangular products of a wide piece as this one symmetric product
  const bool dev_src = panels->want_device_sources && inverted;
  std::vector<int> by_class[3];
  if (inverted)
    for (int s = 0; s < np; ++s) {
      const int cls = piece_class(S.pieces[s]);
      by_class[cls].push_back(s);
      if (dev_src || cls == 2) {
        h.moff[s] = h.mtotal;
        h.mtotal += (long long)S.pieces[s].c * S.pieces[s].c;
      }
    }
  if (dev_src) {
    DCORA_HIP(h.mall.alloc((size_t)std::max<long long>(1, h.mtotal)));
    DCORA_HIP(h.dmoff.alloc((size_t)np));
    DCORA_HIP(hipMemcpyAsync(h.dmoff.p, h.moff.data(), (size_t)np * sizeof(long long), hipMemcpyHostToDevice, st));
  }
  int rc = invert_narrow_pieces(h, by_class[0], dev_src);
  if (rc) return rc;
  rc = invert_pieces(h, by_class[1], true, dev_src ? h.mall.p : nullptr);
  if (rc) return rc;
  if (init_timing) {
    long cnt[3] = {0, 0, 0};
    double vol[3] = {0, 0, 0}, c2[3] = {0, 0, 0};
    for (const CholPiece &P : S.pieces) {
      const int b = piece_class(P);
      ++cnt[b];
      vol[b] += (double)(P.c + P.m) * P.c;
      c2[b] += (double)P.c * P.c;
    }
    fprintf(stderr, "[factor] pieces: narrow %ld (%.0f MB panels, %.0f MB c^2), mid %ld (%.0f MB, %.0f MB), wide %ld (%.0f MB, %.0f MB)\n",
            cnt[0], vol[0] * 8e-6, c2[0] * 8e-6, cnt[1], vol[1] * 8e-6, c2[1] * 8e-6, cnt[2], vol[2] * 8e-6, c2[2] * 8e-6);
  }
  DevBuf<double> mtop_own;  // the wide pieces' M on their way to the host
  if (!dev_src && !by_class[2].empty()) DCORA_HIP(mtop_own.alloc((size_t)std::max<long long>(1, h.mtotal)));
  rc = invert_pieces(h, by_class[2], false, dev_src ? h.mall.p : mtop_own.p);
  if (rc) return rc;
  DCORA_HIP(hipStreamSynchronize(st));
  lap("pack + wide inverses");
  auto blk = std::make_shared<HostBlock>();
  blk->panels = huge_alloc((size_t)ptotal);
  if (dev_src) {
    blk->m_tokens_bytes = (size_t)std::max<long long>(1, h.mtotal) * sizeof(double);
    void *tok = mmap(nullptr, blk->m_tokens_bytes, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (tok == MAP_FAILED) {
      set_last_error("sparse Cholesky: could not reserve the address range of the device-resident M");
      return DCORA_ERR_HIP;
    }
    blk->m_tokens = tok;
  } else {
    blk->M = huge_alloc((size_t)h.mtotal);
  }
  if (!blk->panels || (!dev_src && !blk->M)) {
    set_last_error("sparse Cholesky: no host memory for the factor's panels");
    return DCORA_ERR_HIP;
  }
  double *host = blk->panels, *hostM = dev_src ? (double *)blk->m_tokens : blk->M;
  // non-zeros of the factor (reported as nnz(L)), counted where the factor is
  DevBuf<unsigned long long> dnz;
  DCORA_HIP(dnz.alloc(1));
  DCORA_HIP(hipMemsetAsync(dnz.p, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_count_nonzero, dim3(2048), dim3(256), 0, st, ptotal, h.packed.p, dnz.p);
  unsigned long long nz_dev = 0;
  DCORA_HIP(hipMemcpyAsync(&nz_dev, dnz.p, sizeof nz_dev, hipMemcpyDeviceToHost, st));
  lap("host buffers");
  DCORA_HIP(hipMemcpyAsync(host, h.packed.p, (size_t)ptotal * sizeof(double), hipMemcpyDeviceToHost, st));
  if (h.mtotal > 0 && !dev_src)
    DCORA_HIP(hipMemcpyAsync(hostM, mtop_own.p, (size_t)h.mtotal * sizeof(double), hipMemcpyDeviceToHost, st));
  DCORA_HIP(hipStreamSynchronize(st));
  lap("download");
  PiecewiseFactor &W = *panels;
  W = PiecewiseFactor();
  W.n = S.n;
  W.nhub = S.nhub;
  W.perm = S.perm;
  W.iperm = S.iperm;
  W.pieces.assign((size_t)np, PieceFactor());
  W.block = blk;
  for (int s = 0; s < np; ++s) {
    const CholPiece &P = S.pieces[s];
    PieceFactor &pf = W.pieces[s];
    pf.c0 = P.c0;
    pf.c = P.c;
    pf.rows.assign(S.rows.begin() + P.rows_off, S.rows.begin() + P.rows_off + P.m);
    pf.panel_view = host + h.poff[s];
    pf.inverted = inverted;
    if (h.moff[s] >= 0) pf.Mtop_view = hostM + h.moff[s];
  }
  W.nnzL = (long)nz_dev;
  if (dev_src) {
    W.m_on_device_only = true;
    W.mirrors.push_back(MirrorRange{host, ptotal, h.packed.p});
    W.mirrors.push_back(MirrorRange{hostM, h.mtotal, h.mall.p});
    blk->dev_panels = std::move(h.packed);
    blk->dev_M = std::move(h.mall);
  }
  lap("per-piece copies");
  return DCORA_OK;
}

int factor_on_device(const HostCsr &A, int block, int top, int device, bool *pd, double *info8, PiecewiseFactor *panels,
                     const double *vals_dev = nullptr, hipEvent_t ready = nullptr) {
  if (A.n <= 0 || (int)A.rp.size() != A.n + 1) {
    set_last_error("sparse Cholesky: empty or malformed matrix");
    return DCORA_ERR_BAD_ARG;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    set_last_error("no HIP device available: libdcora_hip has no CPU fallback");
    return DCORA_ERR_NO_DEVICE;
  }
  DCORA_HIP(hipSetDevice(device));
  const auto t0 = Clock::now();
  std::shared_ptr<CholImage> img;
  bool hit = false;
  int rc = find_or_build_image(A, block, top, device, panels == nullptr, &img, &hit);
  if (rc) return rc;
  std::lock_guard<std::mutex> image_lock(img->mu);
  const auto t1 = Clock::now();
  StreamLease lease(device);
  rc = lease.acquire();
  if (rc) return rc;
  hipStream_t st = lease.st;
  DevBuf<double> local_arena;
  double *F = nullptr;
  rc = choose_arena(img, &local_arena, &F);
  if (rc) return rc;
  EnqueueClock clk;
  rc = enqueue_factorisation(*img, st, F, A, vals_dev, ready, &clk);
  if (rc) return rc;
  int failed = 0;
  double logdet = 0;
  rc = read_verdict(*img, st, &failed, &logdet);
  if (rc) return rc;
  *pd = failed == 0;
  const size_t arena_bytes = (size_t)img->sym.arena * sizeof(double);
  if (env::init_timing()) {
    const auto tl = Clock::now();
    fprintf(stderr, "[factor] %-26s %9.1f ms\n[factor] %-26s %9.1f ms (stream + arena %.1f, enqueue %.1f, wait %.1f; arena %.0f MB)\n",
            "hash + analysis / look-up", ms_between(t0, t1), "numeric factorisation", ms_between(t1, tl),
            ms_between(t1, clk.start), ms_between(clk.start, clk.enqueued), ms_between(clk.enqueued, tl), arena_bytes / 1e6);
    fprintf(stderr, "[factor]   enqueue: copy of the values %.2f ms, arena memset %.2f ms, launches %.2f ms\n",
            ms_between(clk.start, clk.copied), ms_between(clk.copied, clk.zeroed), ms_between(clk.zeroed, clk.enqueued));
  }
  if (panels && failed == 0) {
    rc = hand_over_panels(*img, st, F, panels);
    if (rc) return rc;
  }
  if (info8) {
    info8[0] = hit ? 0.0 : img->symbolic_ms;
    info8[1] = ms_between(t1, Clock::now());
    info8[2] = (double)arena_bytes;
    info8[3] = img->sym.flops;
    info8[4] = (double)img->sym.nlev;
    info8[5] = (double)img->plan.size();
    info8[6] = logdet;
    info8[7] = ms_between(t0, t1);  // pattern hash + cache look-up / analysis
  }
  return DCORA_OK;
}
}  // namespace

void enqueue_dense_potrf(hipStream_t st, const PieceDev *pieces, const int *list, int count, int k, double *F,
                         double *linv, int panel_stride, int *fail, double *logdet) {
  const int nb = (k + NB - 1) / NB;
  for (int p = 0; p < nb; ++p) {
    const int j0 = p * NB, jb = std::min(NB, k - j0), rows = k - j0 - jb;
    double *step_inv = linv + (size_t)p * panel_stride * NB * NB;
    hipLaunchKernelGGL(k_chol_potrf, dim3(count), dim3(256), 0, st, pieces, list, j0, F, step_inv, fail, logdet, 1);
    if (rows > 0) {
      const int T = (rows + NB - 1) / NB;
      hipLaunchKernelGGL(k_chol_trsm, dim3(T, count), dim3(256), 0, st, pieces, list, j0, F, (const double *)step_inv,
                         (const int *)fail);
      hipLaunchKernelGGL(k_chol_syrk, dim3(T * (T + 1) / 2, count), dim3(256), 0, st, pieces, list, j0, j0 + NB, -1, 0, F,
                         (const int *)fail);
    }
  }
}

int device_chol_is_pd(const HostCsr &A, int block, int device, bool *pd, double *info8) {
  return factor_on_device(A, block, 0, device, pd, info8, nullptr);
}

int device_chol_is_pd_dev(const HostCsr &pattern, const double *vals_dev, void *ready, int block, int device,
                          bool *pd, double *info8) {
  if (!vals_dev) {
    set_last_error("sparse Cholesky: no device values");
    return DCORA_ERR_BAD_ARG;
  }
  return factor_on_device(pattern, block, 0, device, pd, info8, nullptr, vals_dev, (hipEvent_t)ready);
}

int device_chol_piecewise_factor(const HostCsr &A, int block, int top_unknowns, int device, PiecewiseFactor *out,
                                 double *info8) {
  bool pd = false;
  const int rc = factor_on_device(A, block, top_unknowns, device, &pd, info8, out);
  if (rc) return rc;
  if (!pd) {
    set_last_error("matrix is not positive definite");
    return DCORA_ERR_NOT_PD;
  }
  return DCORA_OK;
}

std::function<bool(const HostCsr &, int, int, const double *, double *)> device_spd_solver(int device) {
  return [device](const HostCsr &A, int block, int nrhs, const double *B, double *X) -> bool {
    if (nrhs < 1 || nrhs > 16) return false;
    if (hipSetDevice(device) != hipSuccess) return false;
    PartInvHost P;
    DeviceWeightSink sink(device);  // the stored weights stream to the device while they are formed
    P.sink = &sink;
    const int nthreads = std::max(2, host_cpus_available());
    if (build_partitioned_inverse_auto(A, block, nthreads, device, &P) != DCORA_OK) return false;
    auto img = std::make_shared<SpImage>();
    if (img->upload(P, &sink) != DCORA_OK) return false;
    P = PartInvHost();  // the host image is no longer needed
    SparsePrecond sp;
    if (sp.attach(img, nrhs) != DCORA_OK) return false;
    const size_t N = (size_t)A.n * nrhs;
    DevBuf<double> dB, dX;
    if (dB.alloc(N) != hipSuccess || dX.alloc(N) != hipSuccess) return false;
    if (hipMemcpy(dB.p, B, N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return false;
    sp.apply(nullptr, nrhs, buf1(dB.p), dX.p, Gate{});
    if (hipMemcpy(X, dX.p, N * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return false;
    return true;
  };
}

int build_partitioned_inverse_auto(const HostCsr &A, int block, int nthreads, int device, PartInvHost *out) {
  const bool host_factor = env::factor_on_host();
  if (host_factor) {
    const bool okh = build_partitioned_inverse(A, block, nthreads, out);
    return okh ? DCORA_OK : (out->weights_ok ? DCORA_ERR_NOT_PD : DCORA_ERR_HIP);
  }
  PiecewiseFactor F;
  // a sink that forms the weights on the device wants the sources left there
  F.want_device_sources = out->sink && out->sink->wants_device_sources();
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = device_chol_piecewise_factor(A, block, nd_top_default(), device, &F);
  if (rc) return rc;
  const auto t1 = std::chrono::steady_clock::now();
  const bool ok = build_partitioned_inverse_from(A, F, nthreads, out);
  if (env::init_timing())
    fprintf(stderr, "[precond] factor on the device %.1f ms, partitioned inverse on the host %.1f ms\n",
            std::chrono::duration<double, std::milli>(t1 - t0).count(),
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
  if (!ok && !out->weights_ok) return DCORA_ERR_HIP;  // the weight sink failed (device or pinned memory): not a verdict
  return ok ? DCORA_OK : DCORA_ERR_NOT_PD;
}

}  // namespace dcora
