// The CSR SpMM kernels of the generic path (any layout, r <= 16): Y = X A (+ G) with its dots (k_spmm), and the Hessian
// SpMM of a tCG iteration with the direction update folded in (k_spmm_dir), with ROPTLIB's EucHvToHv folded in as well
// (k_spmm_dir_fix).  One thread per output element (column j, component t): the r lanes of a row read r contiguous
// doubles of X(:, c) and share one (value, column) pair.  The CSR segment of the block's rows is staged in LDS with
// fully coalesced loads (row blocks of a connection Laplacian are contiguous in CSR); rows of more than kLongRow
// entries are served by kLongSplit workgroups of their own, behind the main grid.  The row walk is csr_rows.h; here
// are what a gathered column contributes and what each kernel does with a finished row.
#include "csr_rows.h"
#include "tcg_rules.h"

namespace dcora {

int spmm_grid(int nrows, int r) {
  const int RB = kBlock / r;
  long nrb = (nrows + RB - 1) / RB;
  if (nrb < 1) nrb = 1;
  if (nrb > kMaxPartials) nrb = kMaxPartials;
  return (int)nrb;
}

namespace {
// a gathered column contributes X[o] ...
struct GatherX {
  const double *__restrict__ X;
  using Op = double;
  __device__ __forceinline__ Op load(size_t o) const { return X[o]; }
  __device__ __forceinline__ double value(Op x) const { return x; }
};
// ... or the new tCG direction delta_new = -z + beta delta_old (iteration 0: -z; delta_old is not read then)
struct GatherDir {
  const double *__restrict__ z, *__restrict__ d_old;
  double beta;
  int iter;
  struct Op {
    double x, y;
  };
  __device__ __forceinline__ Op load(size_t o) const { return Op{z[o], iter > 0 ? d_old[o] : 0.0}; }
  __device__ __forceinline__ double value(Op a) const { return fma(beta, a.y, -a.x); }
  // the direction itself, for the element a thread owns
  __device__ __forceinline__ double own(size_t o) const { return iter > 0 ? fma(beta, d_old[o], -z[o]) : -z[o]; }
};
}  // namespace

// ------------------------------------------------------------------------------------------------------
// SpMM  Y = X * A (+ G); DOTS: the partial dots {<X A, X>, <X, G>}, one slot per workgroup of the main grid and ONE per
// long row, written by whichever slice arrives last.
// ------------------------------------------------------------------------------------------------------
template <bool DOTS>
__global__ __launch_bounds__(kBlock) void k_spmm(int r, CsrDev A, Buf2 Xb, int selX, const double *__restrict__ G,
                                                 Buf2 Yb, int selY, double *__restrict__ partials, Gate g,
                                                 int main_grid) {
  if (gated(g.ctl, g.seq, g.gate)) return;
  __shared__ int s_ci[kSpmmTile];
  __shared__ double s_v[kSpmmTile];
  __shared__ double s_red[16];
  __shared__ int s_last;
  const double *__restrict__ X = pick(Xb, g.ctl, selX);
  double *__restrict__ Y = pick(Yb, g.ctl, selY);
  const GatherX f{X};
  const int RB = kBlock / r;
  const int nrb = (A.nrows + RB - 1) / RB;
  const int lj = threadIdx.x / r, t = threadIdx.x - lj * r;
  double d0 = 0, d1 = 0;
  if ((int)blockIdx.x >= main_grid) {  // a slice of a long row
    const LongSlice s = long_slice(A, main_grid);
    if (!slices_meet(A, s, r, slice_sum(A, s, r, f), s_v, &s_last)) return;
    if ((int)threadIdx.x < r) {
      double y = slices_total(A, s);
      const size_t o = (size_t)s.j * r + threadIdx.x;
      if (DOTS) {
        const double x = X[o];
        d0 = y * x;
        if (G) d1 = x * G[o];
      }
      if (G) y += G[o];
      Y[o] = y;
    }
    if (DOTS) {
      const double a = block_sum(d0, s_red);
      const double b = block_sum(d1, s_red);
      if (threadIdx.x == 0) {
        partials[2 * (main_grid + s.li)] = a;
        partials[2 * (main_grid + s.li) + 1] = b;
      }
    }
    return;
  }
  for (int rb = blockIdx.x; rb < nrb; rb += main_grid) {
    const int j0 = rb * RB;
    const int j1 = min(A.nrows, j0 + RB);
    const int j = j0 + lj;
    const bool active = (lj < RB) && (j < j1);
    const int pbeg = A.rp[j0], pend = A.rp[j1];
    int myb = active ? A.rp[j] : 0, mye = active ? A.rp[j + 1] : 0;
    const bool is_long = A.n_long > 0 && (mye - myb > kLongRow);  // served by its own workgroups
    if (is_long) mye = myb;
    const double acc = row_block_sum(A, f, r, t, pbeg, pend, myb, mye, s_ci, s_v);
    if (active && !is_long) {
      const size_t o = (size_t)j * r + t;
      double y = acc;
      if (DOTS) {
        const double x = X[o];
        d0 += acc * x;
        if (G) d1 += x * G[o];
      }
      if (G) y += G[o];
      Y[o] = y;
    }
  }
  if (DOTS) {
    const double a = block_sum(d0, s_red);
    const double b = block_sum(d1, s_red);
    if (threadIdx.x == 0) {
      partials[2 * blockIdx.x] = a;
      partials[2 * blockIdx.x + 1] = b;
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// Generic-layout tCG, iteration `iter`: the direction update of the previous iteration folded into the Hessian SpMM.
//   delta_new = -z + beta delta_old   (beta = <z, r>_new / <z, r>_old from the partials p3; iter 0: delta_new = -z)
//   W = delta_new Q                   (delta_new formed in the gather, written for the block's own columns)
// and the scalar recurrence of ROPTLIB's tCG_TR (block 0, tcg_rules.h): iteration 0 starts it, later ones finish iteration
// iter - 1 as k_tcg_update2 does after the last one.  delta_old and delta_new are different buffers: other workgroups
// still gather the old direction.  k_hessfix follows it; it runs where k_spmm_dir_fix does not apply.
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_spmm_dir(int r, CsrDev A, const double *__restrict__ z,
                                                     const double *__restrict__ d_old, double *__restrict__ d_new,
                                                     double *__restrict__ W, const double *__restrict__ p3, int np3,
                                                     SolverCtl *ctl, int seq, int iter, int main_grid) {
  if (gated(ctl, seq, 2)) return;
  __shared__ int s_ci[kSpmmTile];
  __shared__ double s_v[kSpmmTile];
  __shared__ double s_red[16];
  __shared__ int s_last;
  const int par = (iter - 1) & 1;
  const double z_r_new = sum_partials(p3, np3, 1, 0, s_red);
  const double beta = iter > 0 ? tcg_beta(z_r_new, ctl->z_r[par]) : 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (iter == 0)
      tcg_put_dir(ctl, 0, tcg_dir_start(z_r_new), 0.0);
    else
      tcg_put_dir(ctl, par ^ 1, tcg_dir_next(z_r_new, beta, ctl->alpha, ctl->d_Pd[par], ctl->e_Pd[par]), ctl->e_Pe_n);
  }
  const GatherDir f{z, d_old, beta, iter};
  const int RB = kBlock / r;
  const int nrb = (A.nrows + RB - 1) / RB;
  const int lj = threadIdx.x / r, t = threadIdx.x - lj * r;
  if ((int)blockIdx.x >= main_grid) {  // a slice of a long row
    const LongSlice s = long_slice(A, main_grid);
    if (!slices_meet(A, s, r, slice_sum(A, s, r, f), s_v, &s_last)) return;
    if ((int)threadIdx.x < r) {
      const size_t o = (size_t)s.j * r + threadIdx.x;
      W[o] = slices_total(A, s);
      d_new[o] = f.own(o);
    }
    return;
  }
  for (int rb = blockIdx.x; rb < nrb; rb += main_grid) {
    const int j0 = rb * RB;
    const int j1 = min(A.nrows, j0 + RB);
    const int j = j0 + lj;
    const bool active = (lj < RB) && (j < j1);
    const int pbeg = A.rp[j0], pend = A.rp[j1];
    int myb = active ? A.rp[j] : 0, mye = active ? A.rp[j + 1] : 0;
    const bool is_long = A.n_long > 0 && (mye - myb > kLongRow);  // served by its own workgroups
    if (is_long) mye = myb;
    const double own = (active && !is_long) ? f.own((size_t)j * r + t) : 0.0;
    const double acc = row_block_sum(A, f, r, t, pbeg, pend, myb, mye, s_ci, s_v);
    if (active && !is_long) {
      const size_t o = (size_t)j * r + t;
      W[o] = acc;
      d_new[o] = own;
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// The same with ROPTLIB's EucHvToHv (k_hessfix) folded in: one launch per tCG iteration instead of two.
//   delta_new = -z + beta delta_old,  W = delta_new Q,  Hd = Proj_X(W - delta_new S),  partial <delta_new, Hd>
// A workgroup owns whole manifold items: its rows-per-block count is a multiple of the rotation block's width (d,
// or d + 1 in the pose layout), so the d columns a Stiefel projection couples sit in one workgroup and meet in LDS.
// Long rows (served by their own workgroups) must be Euclidean columns (DeviceProblem::hess_one_launch()): their Hd is
// W itself.  The arithmetic follows k_hessfix term by term (sub_AS, sym_gram, sub_AS); only the order in which the
// partial sums of <delta, Hd> are added differs.
// ------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kBlock) void k_spmm_dir_fix(ManiDesc m, CsrDev A, Buf2 Xb, Buf2 Sb,
                                                         const double *__restrict__ z,
                                                         const double *__restrict__ d_old, double *__restrict__ d_new,
                                                         double *__restrict__ Hd, const double *__restrict__ p3,
                                                         int np3, double *__restrict__ p1, SolverCtl *ctl, int seq,
                                                         int iter, int main_grid) {
  __shared__ int s_ci[kSpmmTile];
  __shared__ double s_v[kSpmmTile];
  __shared__ double s_red[16];
  __shared__ double s_V[kBlock], s_T[kBlock], s_Y[kBlock];
  __shared__ int s_last;
  const int r = m.r;
  const int par = (iter - 1) & 1;
  // Loads that depend on nothing are requested before the gate is looked at (one round trip instead of four in a row):
  // the partials of <z, r>, its old value, the row pointers of the workgroup's first row block and the thread's own
  // entries of z and delta.  The empty asm keeps the compiler from sinking them behind the early return.
  const GateWords gw = gate_words(ctl);
  double pv = ((int)threadIdx.x < np3) ? p3[threadIdx.x] : 0.0;
  const double zr_old = iter > 0 ? ctl->z_r[par] : 1.0;
  int rp_pre[4] = {0, 0, 0, 0};
  double z_pre = 0, d_pre = 0;
  {
    const int al_ = m.se ? D + 1 : D;
    const int RB_ = ((kBlock / r) / al_) * al_;
    const int j0 = (int)blockIdx.x * RB_, lj_ = threadIdx.x / r;
    if ((int)blockIdx.x < main_grid && j0 < A.nrows) {
      const int j1 = min(A.nrows, j0 + RB_), j = j0 + lj_;
      rp_pre[0] = A.rp[j0];
      rp_pre[1] = A.rp[j1];
      if (lj_ < RB_ && j < j1) {
        rp_pre[2] = A.rp[j];
        rp_pre[3] = A.rp[j + 1];
        const size_t o = (size_t)j * r + (threadIdx.x - lj_ * r);
        z_pre = z[o];
        d_pre = iter > 0 ? d_old[o] : 0.0;
      }
    }
  }
  asm volatile("" ::"v"(pv), "v"(zr_old), "v"(rp_pre[0]), "v"(rp_pre[1]), "v"(rp_pre[2]), "v"(rp_pre[3]), "v"(z_pre),
               "v"(d_pre), "s"(gw.outer), "s"(gw.tcg));
  if (gated(gw, ctl, seq, 2)) return;
  for (int i = threadIdx.x + blockDim.x; i < np3; i += blockDim.x) pv += p3[i];
  const double z_r_new = block_sum(pv, s_red);
  const double beta = iter > 0 ? tcg_beta(z_r_new, zr_old) : 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (iter == 0)
      tcg_put_dir(ctl, 0, tcg_dir_start(z_r_new), 0.0);
    else
      tcg_put_dir(ctl, par ^ 1, tcg_dir_next(z_r_new, beta, ctl->alpha, ctl->d_Pd[par], ctl->e_Pd[par]), ctl->e_Pe_n);
  }
  const GatherDir f{z, d_old, beta, iter};
  const double *X = pick(Xb, ctl, 0);
  const double *Sblk = pick(Sb, ctl, 0);
  const int al = m.se ? D + 1 : D;
  const int RB = ((kBlock / r) / al) * al;  // whole items per workgroup here; a slice's entry groups are kBlock / r
  const int nrb = (A.nrows + RB - 1) / RB;
  const int lj = threadIdx.x / r, t = threadIdx.x - lj * r;
  if ((int)blockIdx.x >= main_grid) {  // a slice of a long (Euclidean) row
    const LongSlice s = long_slice(A, main_grid);
    if (!slices_meet(A, s, r, slice_sum(A, s, r, f), s_v, &s_last)) return;
    if (threadIdx.x < 64) {  // r <= 16: the row's r entries sit in the first wave
      double dot = 0;
      if ((int)threadIdx.x < r) {
        const double y = slices_total(A, s);
        const size_t o = (size_t)s.j * r + threadIdx.x;
        const double dn = f.own(o);
        Hd[o] = y;
        d_new[o] = dn;
        dot = dn * y;
      }
      // ONE slot per long row, written by whichever slice arrives last: a slot per slice would move the row's term
      // around the partial array from run to run, and with it the order of the consumer's sum
      dot = wave_sum(dot);
      if (threadIdx.x == 0) p1[main_grid + s.li] = dot;
    }
    return;
  }
  const int n_rot_rows = m.se ? A.nrows : m.n * D;  // rows below this bound belong to pose items
  double dacc = 0;
  for (int rb = blockIdx.x; rb < nrb; rb += main_grid) {
    const int j0 = rb * RB;
    const int j1 = min(A.nrows, j0 + RB);
    const int j = j0 + lj;
    const bool active = (lj < RB) && (j < j1);
    const bool first = rb == (int)blockIdx.x;  // requested in the prologue
    const int pbeg = first ? rp_pre[0] : A.rp[j0], pend = first ? rp_pre[1] : A.rp[j1];
    int myb = active ? (first ? rp_pre[2] : A.rp[j]) : 0, mye = active ? (first ? rp_pre[3] : A.rp[j + 1]) : 0;
    const bool is_long = A.n_long > 0 && (mye - myb > kLongRow);  // served by its own workgroups
    if (is_long) mye = myb;
    const size_t o = (size_t)(active ? j : j0) * r + t;
    const double own = !active ? 0.0 : !first ? f.own(o) : iter > 0 ? fma(beta, d_pre, -z_pre) : -z_pre;
    const double xo = active ? X[o] : 0.0;
    const double acc = row_block_sum(A, f, r, t, pbeg, pend, myb, mye, s_ci, s_v);
    // ---- EucHvToHv on the block's own items ----
    // kind: 0 rotation column `a` of pose `it`, 1 unit-sphere column, 2 Euclidean column
    int kind = 2, a = 0, it = 0;
    if (active && j < n_rot_rows) {
      const int q = j / al;
      a = j - q * al;
      it = q;
      kind = (a < D) ? 0 : 2;
    } else if (active && !m.se && j < n_rot_rows + m.l) {
      kind = 1;
      it = j - n_rot_rows;
    }
    __syncthreads();
    s_V[threadIdx.x] = own;
    s_Y[threadIdx.x] = xo;
    __syncthreads();
    double T = acc;
    const int l0 = lj - a;  // local row of the item's first column
    if (kind == 0) {
      double sres = 0;
#pragma unroll
      for (int b = 0; b < D; ++b) sres += s_V[(l0 + b) * r + t] * Sblk[(size_t)it * D * D + b + a * D];
      T = acc - sres;
    } else if (kind == 1) {
      T = acc - own * Sblk[(size_t)m.n * D * D + it];
    }
    s_T[threadIdx.x] = T;
    __syncthreads();
    double hv = T;
    if (kind == 0) {
      // S2 = sym(Y^T T); hv = T - sum_a' Y(t, a') S2[a'][a]
      double sres = 0;
#pragma unroll
      for (int b = 0; b < D; ++b) {
        double pba = 0, pab = 0;  // P[b][a] = sum_t Y(t, b) T(t, a), P[a][b] = sum_t Y(t, a) T(t, b)
        for (int u = 0; u < r; ++u) {
          pba += s_Y[(l0 + b) * r + u] * s_T[(l0 + a) * r + u];
          pab += s_Y[(l0 + a) * r + u] * s_T[(l0 + b) * r + u];
        }
        sres += s_Y[(l0 + b) * r + t] * (0.5 * (pba + pab));
      }
      hv = T - sres;
    } else if (kind == 1) {
      double yt = 0;
      for (int u = 0; u < r; ++u) yt += s_Y[lj * r + u] * s_T[lj * r + u];
      hv = T - xo * yt;
    }
    if (active && !is_long) {
      Hd[o] = hv;
      d_new[o] = own;
      dacc += own * hv;
    }
  }
  const double tot = block_sum(dacc, s_red);
  if (threadIdx.x == 0) p1[blockIdx.x] = tot;
}

int spmm_dir_fix_grid(const ManiDesc &m, int nrows) {
  const int al = m.se ? m.d + 1 : m.d;
  const int RB = ((kBlock / m.r) / al) * al;
  if (RB < al) return 0;
  long nrb = (nrows + RB - 1) / RB;
  if (nrb < 1) nrb = 1;
  if (nrb > kMaxPartials) nrb = kMaxPartials;
  return (int)nrb;
}

int launch_spmm_dir_fix(hipStream_t st, const ManiDesc &m, const CsrDev &A, Buf2 X, Buf2 Sblk, const double *z,
                        const double *d_old, double *d_new, double *Hd, const double *p3, int np3, double *p1,
                        SolverCtl *ctl, int seq, int iter) {
  const int main_grid = spmm_dir_fix_grid(m, A.nrows);
  const int grid = main_grid + A.n_long * kLongSplit;
  if (m.d == 3)
    hipLaunchKernelGGL(k_spmm_dir_fix<3>, dim3(grid), dim3(kBlock), 0, st, m, A, X, Sblk, z, d_old, d_new, Hd, p3, np3,
                       p1, ctl, seq, iter, main_grid);
  else
    hipLaunchKernelGGL(k_spmm_dir_fix<2>, dim3(grid), dim3(kBlock), 0, st, m, A, X, Sblk, z, d_old, d_new, Hd, p3, np3,
                       p1, ctl, seq, iter, main_grid);
  return main_grid + A.n_long;
}

void launch_spmm_dir(hipStream_t st, int r, const CsrDev &A, const double *z, const double *d_old, double *d_new,
                     double *W, const double *p3, int np3, SolverCtl *ctl, int seq, int iter) {
  const int main_grid = spmm_grid(A.nrows, r);
  const int grid = main_grid + A.n_long * kLongSplit;
  hipLaunchKernelGGL(k_spmm_dir, dim3(grid), dim3(kBlock), 0, st, r, A, z, d_old, d_new, W, p3, np3, ctl, seq, iter,
                     main_grid);
}

void launch_spmm(hipStream_t st, int r, const CsrDev &A, Buf2 X, int selX, const double *G, Buf2 Y, int selY,
                 double *partials, Gate g) {
  count_launch();
  const int main_grid = spmm_grid(A.nrows, r);
  const int grid = main_grid + A.n_long * kLongSplit;
  if (partials)
    hipLaunchKernelGGL(k_spmm<true>, dim3(grid), dim3(kBlock), 0, st, r, A, X, selX, G, Y, selY, partials, g,
                       main_grid);
  else
    hipLaunchKernelGGL(k_spmm<false>, dim3(grid), dim3(kBlock), 0, st, r, A, X, selX, G, Y, selY, partials, g,
                       main_grid);
}

}  // namespace dcora
