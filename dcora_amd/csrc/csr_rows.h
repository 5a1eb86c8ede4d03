// The CSR row walk of the generic SpMM kernels (spmm_csr.hip), stated once: how a workgroup stages the entries of its
// row block in LDS and a thread gathers its row from them, how a long row is cut into slices, and how the slices meet.
// What a gathered column contributes is a functor F with
//   typename F::Op            what is loaded per column (one double, or a pair)
//   Op load(size_t o) const   the loads of element o = column * r + t
//   double value(Op) const    the value the entry's weight multiplies
// load and value are separate so that the eight loads of a batch are issued before the first multiply-add.
// The order of every sum here is part of the results (bitwise): coupling_row (bottom) restates it for k_fused_grad.
#pragma once
#include "kernels.h"

namespace dcora {
#if defined(__HIPCC__)

// ---- row block: one thread per output element, the block's entries staged in LDS a tile at a time ----
// One tile: all trips' loads are issued (clamped index, straight line) before any is stored to LDS -- one memory round
// trip per tile instead of one per 256 entries.  The barriers around it belong to it.
__device__ __forceinline__ void stage_tile(const CsrDev &A, int base, int cnt, int *s_ci, double *s_v) {
  constexpr int SU = kSpmmTile / kBlock;
  int ci_r[SU];
  double v_r[SU];
  const int last = base + cnt - 1;
  __syncthreads();
#pragma unroll
  for (int u = 0; u < SU; ++u) {
    const int i = min(base + (int)threadIdx.x + u * kBlock, last);
    ci_r[u] = A.ci[i];
    v_r[u] = A.v[i];
  }
#pragma unroll
  for (int u = 0; u < SU; ++u) {
    const int i = threadIdx.x + u * kBlock;
    if (i < cnt) {
      s_ci[i] = ci_r[u];
      s_v[i] = v_r[u];
    }
  }
  __syncthreads();
}
// A thread's share [lo, hi) of the staged tile, added to acc: batches of 8 with every load issued before the first use;
// a batch's padding is a zero weight on the segment's first entry.
template <class F>
__device__ __forceinline__ double gather_tile(const F &f, int r, int t, int lo, int hi, const int *s_ci,
                                              const double *s_v, double acc) {
  for (int p = lo; p < hi; p += 8) {
    double w8[8];
    typename F::Op x8[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const bool ok = p + q < hi;
      const int pp = ok ? p + q : lo;
      w8[q] = ok ? s_v[pp] : 0.0;
      x8[q] = f.load((size_t)s_ci[pp] * r + t);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) acc += w8[q] * f.value(x8[q]);
  }
  return acc;
}
// The sum of the thread's row [myb, mye) inside the row block's entries [pbeg, pend), tile by tile.
template <class F>
__device__ __forceinline__ double row_block_sum(const CsrDev &A, const F &f, int r, int t, int pbeg, int pend, int myb,
                                                int mye, int *s_ci, double *s_v) {
  double acc = 0;
  for (int base = pbeg; base < pend; base += kSpmmTile) {
    const int cnt = min(kSpmmTile, pend - base);
    stage_tile(A, base, cnt, s_ci, s_v);
    acc = gather_tile(f, r, t, max(myb, base) - base, min(mye, base + cnt) - base, s_ci, s_v, acc);
  }
  return acc;
}

// ---- long rows: kLongSplit workgroups per row (a landmark ranged from 7789 poses on tiers.pyfg: one workgroup was the
// longest of the launch).  Each takes a slice, its kBlock / r entry groups stride over it, the groups' sums meet in LDS
// and go to a scratch row; the last workgroup to arrive adds the slices in slice order (reproducible) and finishes.
struct LongSlice {
  int li, sl;   // long row and slice of this workgroup
  int j, rb0;   // the row and its first entry
  int pb, pe;   // the slice's entries
};
__device__ __forceinline__ LongSlice long_slice(const CsrDev &A, int main_grid) {
  LongSlice s;
  s.li = ((int)blockIdx.x - main_grid) / kLongSplit;
  s.sl = ((int)blockIdx.x - main_grid) % kLongSplit;
  s.j = A.long_rows[s.li];
  s.rb0 = A.rp[s.j];
  const int re0 = A.rp[s.j + 1];
  const int per = (re0 - s.rb0 + kLongSplit - 1) / kLongSplit;
  s.pb = s.rb0 + s.sl * per;
  s.pe = min(re0, s.pb + per);
  return s;
}
// The thread's part of the slice: eight entries per step with every load in flight before the first use (index clamped,
// weight masked).
template <class F>
__device__ __forceinline__ double slice_sum(const CsrDev &A, const LongSlice &s, int r, const F &f) {
  const int RB = kBlock / r;
  const int lj = threadIdx.x / r, t = threadIdx.x - lj * r;
  double acc = 0;
  if (lj < RB) {
    for (int p = s.pb + lj; p < s.pe; p += 8 * RB) {
      int c8[8];
      double w8[8];
      typename F::Op x8[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int pp = p + q * RB;
        const bool ok = pp < s.pe;
        c8[q] = A.ci[ok ? pp : s.rb0];
        w8[q] = ok ? A.v[pp] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) x8[q] = f.load((size_t)c8[q] * r + t);
#pragma unroll
      for (int q = 0; q < 8; ++q) acc += w8[q] * f.value(x8[q]);
    }
  }
  return acc;
}
// The meeting: the entry groups' sums through s_part (kBlock doubles of LDS), the slice's r sums to long_part, the
// arrival count.  True for the last workgroup to arrive alone, which resets the counter for the next launch and goes on
// to finish the row: its threads < r read the row's sum from slices_total.  Nobody waits for anybody.
__device__ __forceinline__ bool slices_meet(const CsrDev &A, const LongSlice &s, int r, double acc, double *s_part,
                                            int *s_last) {
  const int RB = kBlock / r;
  const int lj = threadIdx.x / r;
  __syncthreads();
  s_part[threadIdx.x] = (lj < RB) ? acc : 0.0;
  __syncthreads();
  if ((int)threadIdx.x < r) {
    double y = 0;
    for (int q = 0; q < RB; ++q) y += s_part[q * r + threadIdx.x];
    __hip_atomic_store(A.long_part + ((size_t)s.li * kLongSplit + s.sl) * 16 + threadIdx.x, y, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0)
    *s_last = (__hip_atomic_fetch_add(A.long_cnt + s.li, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) ==
               kLongSplit - 1);
  __syncthreads();
  if (!*s_last) return false;
  if (threadIdx.x == 0) __hip_atomic_store(A.long_cnt + s.li, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}
// component threadIdx.x (< r) of the row's sum: the slices in slice order
__device__ __forceinline__ double slices_total(const CsrDev &A, const LongSlice &s) {
  double y = 0;
  for (int q = 0; q < kLongSplit; ++q)
    y += __hip_atomic_load(A.long_part + ((size_t)s.li * kLongSplit + q) * 16 + threadIdx.x, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
  return y;
}

// ---- the same sums without the staging (k_fused_grad's RIDE, fused_eval.hip) ----
// G of one output element as k_spmm<false> forms it: the row's entries in batches of 8 that restart at the tile
// borders of k_spmm's row block (rows j0 .. j0 + kBlock / r - 1, kSpmmTile entries from rp[j0]), a batch's padding as
// a zero weight on the segment's first entry, acc = fma(w, x, acc) in index order.
__device__ __forceinline__ double coupling_row(const GradRide &c, int r, int j, int t) {
  const int RB = kBlock / r;
  const int pb0 = c.c_rp[(j / RB) * RB];
  const int myb = c.c_rp[j], mye = c.c_rp[j + 1];
  double acc = 0;
  int lo = myb;
  while (lo < mye) {
    const int hi = min(mye, pb0 + ((lo - pb0) / kSpmmTile + 1) * kSpmmTile);
    for (int p = lo; p < hi; p += 8) {
      double x8[8], w8[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const bool ok = p + q < hi;
        const int pp = ok ? p + q : lo;
        w8[q] = ok ? c.c_v[pp] : 0.0;
        x8[q] = c.c_X[(size_t)c.c_ci[pp] * r + t];
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) acc = fma(w8[q], x8[q], acc);
    }
    lo = hi;
  }
  return acc;
}

#endif
}  // namespace dcora
