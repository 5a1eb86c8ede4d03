// Hand-written HIP kernels for gfx950 (MI355X): dense preconditioner apply, the device-resident scalar logic of the
// truncated-CG / trust-region solver, vector utilities and the Lanczos steps.  The thread-per-variable manifold kernels
// of the same path are manifold.hip, its connection-Laplacian SpMM is spmm_csr.hip.
//
// Design notes:
//  * wavefront = 64; all block-level reductions are wave shuffles + one LDS hop, in a fixed order;
//  * reductions leave per-block partials in HBM; the consumer kernel sums them in its prologue, so a
//    dot product costs no extra launch and the result is bitwise reproducible;
//  * solver kernels read their trust-region / tCG scalars from a SolverCtl block in HBM and are no-ops once a
//    termination stamp older than their own sequence number is set -- the host never waits for a scalar.
#include "kernels.h"
#include "tcg_rules.h"

namespace dcora {

// ------------------------------------------------------------------------------------------------------
// helpers
// ------------------------------------------------------------------------------------------------------
// N sums of partial arrays at once for the single-block bookkeeping kernels: every load is issued before the first
// reduction (one memory round trip instead of one per sum) and the N wave sums share one LDS exchange (two barriers
// instead of 2 N).  p[q] has np[q] entries of stride st[q] at offset off[q]; sm must hold >= 4 N doubles.
template <int N>
__device__ __forceinline__ void sum_partials_n(const double *const (&p)[N], const int (&np)[N], const int (&st)[N],
                                               const int (&off)[N], double *sm, double (&out)[N]) {
  double v[N];
#pragma unroll
  for (int q = 0; q < N; ++q) v[q] = ((int)threadIdx.x < np[q]) ? p[q][(size_t)threadIdx.x * st[q] + off[q]] : 0.0;
#pragma unroll
  for (int q = 0; q < N; ++q)
    for (int i = threadIdx.x + blockDim.x; i < np[q]; i += blockDim.x) v[q] += p[q][(size_t)i * st[q] + off[q]];
#pragma unroll
  for (int q = 0; q < N; ++q) v[q] = wave_sum(v[q]);
  const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int q = 0; q < N; ++q) sm[q * 4 + w] = v[q];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < N; ++q) {
    double t = 0;
    for (int i = 0; i < nw; ++i) t += sm[q * 4 + i];
    out[q] = t;
  }
}

std::atomic<long> g_chain_launches{0};

int vec_grid(long nelem) {
  long g = (nelem + kBlock - 1) / kBlock;
  if (g < 1) g = 1;
  if (g > kMaxPartials) g = kMaxPartials;
  return (int)g;
}

// ------------------------------------------------------------------------------------------------------
// Dense preconditioner apply  Z = R * Minv  (Minv symmetric => row j of Minv is column j).
// One wave streams RW complete rows of Minv with 16-byte loads; lane l owns columns {2l, 2l+1} + 128 i.
// ------------------------------------------------------------------------------------------------------
template <int RM, int RW>
__global__ __launch_bounds__(kBlock) void k_dense_apply(int r, int k, int ldm, const double *__restrict__ Minv,
                                                        Buf2 Rb, double *__restrict__ Z,
                                                        const double *__restrict__ p2, int np2, Gate g) {
  if (gated(g.ctl, g.seq, g.gate)) return;
  __shared__ double s_red[16];
  if (p2) {
    // residual already below the tCG stopping threshold: the next kernel records the termination
    const double nr = sqrt(sum_partials(p2, np2, 1, 0, s_red));
    if (tcg_residual_done(nr, g.ctl->norm_r0)) return;
  }
  const double *__restrict__ R = pick(Rb, g.ctl, 0);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j0 = (blockIdx.x * (kBlock / 64) + wave) * RW;
  if (j0 >= k) return;
  double acc[RW][RM];
#pragma unroll
  for (int a = 0; a < RW; ++a)
#pragma unroll
    for (int t = 0; t < RM; ++t) acc[a][t] = 0;
  const double *rows[RW];
#pragma unroll
  for (int a = 0; a < RW; ++a) rows[a] = Minv + (size_t)min(j0 + a, k - 1) * ldm;
  for (int c = 2 * lane; c < k; c += 128) {
    const bool two = (c + 1 < k);
    double m0[RW], m1[RW];
#pragma unroll
    for (int a = 0; a < RW; ++a) {
      const double2 mm = *reinterpret_cast<const double2 *>(rows[a] + c);  // ldm is padded: always in bounds
      m0[a] = mm.x;
      m1[a] = two ? mm.y : 0.0;
    }
    const double *rc = R + (size_t)c * r;
#pragma unroll
    for (int t = 0; t < RM; ++t)
      if (t < r) {
        const double x0 = rc[t];
        const double x1 = two ? rc[r + t] : 0.0;
#pragma unroll
        for (int a = 0; a < RW; ++a) acc[a][t] += x0 * m0[a] + x1 * m1[a];
      }
  }
#pragma unroll
  for (int a = 0; a < RW; ++a)
#pragma unroll
    for (int t = 0; t < RM; ++t)
      if (t < r) {
        const double s = wave_sum(acc[a][t]);
        if (lane == 0 && j0 + a < k) Z[(size_t)(j0 + a) * r + t] = s;
      }
}

void launch_dense_apply(hipStream_t st, int r, int k, int ldm, const double *Minv, Buf2 R, double *Z,
                        const double *p2, int np2, Gate g) {
  constexpr int RW = 2;
  const int rows_per_block = (kBlock / 64) * RW;
  const int grid = (k + rows_per_block - 1) / rows_per_block;
  if (r <= 4)
    hipLaunchKernelGGL((k_dense_apply<4, RW>), dim3(grid), dim3(kBlock), 0, st, r, k, ldm, Minv, R, Z, p2, np2, g);
  else if (r <= 8)
    hipLaunchKernelGGL((k_dense_apply<8, RW>), dim3(grid), dim3(kBlock), 0, st, r, k, ldm, Minv, R, Z, p2, np2, g);
  else
    hipLaunchKernelGGL((k_dense_apply<16, RW>), dim3(grid), dim3(kBlock), 0, st, r, k, ldm, Minv, R, Z, p2, np2, g);
}

// ------------------------------------------------------------------------------------------------------
// Trust-region / truncated-CG scalar logic (ROPTLIB RTRNewton + SolversTR::tCG_TR restated).
// Every block recomputes the same scalars from the same partials; block 0 publishes them.
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_rtr_init(const double *pA, int npA, const double *pB, int npB,
                                                     SolverCtl *ctl, HostFlags *hf, int seq, CtlInit ci,
                                                     unsigned *tcg_sync, int nsync) {
  __shared__ double s_red[16];
  for (int i = threadIdx.x; i < nsync; i += kBlock) tcg_sync[i] = 0u;
  if (ci.enable && threadIdx.x == 0) ctl_arm(ctl, ci);  // (saves the separate k_ctl_init launch)
  const double *const ps[3] = {pA, pA, pB};
  const int nps[3] = {npA, npA, npB}, sts[3] = {2, 2, 1}, offs[3] = {0, 1, 0};
  double sums[3];
  sum_partials_n<3>(ps, nps, sts, offs, s_red, sums);
  const double fq = sums[0], fg = sums[1], g2 = sums[2];
  if (threadIdx.x == 0) {
    ctl->f1 = 0.5 * fq + fg;
    ctl->ngf = sqrt(g2);
    ctl->fInit = ctl->f1;
    ctl->gradNormInit = ctl->ngf;
    if (ctl->ngf < ctl->tol || ctl->max_outer <= 0) {  // ref src/QuadraticOptimizer.cpp:54-55
      ctl->outer_done_stamp = seq;
      host_store(&hf->outer_done_seq, seq);
    }
    host_store(&hf->last_seq_done, seq);
  }
}

// start of a tCG run: res = grad (accepted iterate), eta = H eta = 0, termination stamps re-armed
__global__ __launch_bounds__(kBlock) void k_tcg_begin(long nelem, Buf2 gradb, double *__restrict__ eta,
                                                      double *__restrict__ Heta, double *__restrict__ res,
                                                      SolverCtl *ctl, int seq) {
  if (gated(ctl, seq, 1)) return;
  const double *grad = pick(gradb, ctl, 0);
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < nelem; i += (long)gridDim.x * kBlock) {
    eta[i] = 0;
    Heta[i] = 0;
    res[i] = grad[i];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) tcg_begin_run(ctl, ctl->ngf);
}
__global__ __launch_bounds__(kBlock) void k_tcg_update1(long nelem, const double *__restrict__ delta,
                                                        const double *__restrict__ Hd, double *__restrict__ eta,
                                                        double *__restrict__ Heta, double *__restrict__ res,
                                                        const double *__restrict__ p1, int np1,
                                                        double *__restrict__ p2, SolverCtl *ctl, HostFlags *hf,
                                                        int seq, int iter, int r, SpFold sf) {
  __shared__ double s_red[16];
  const int par = iter & 1;
  // Every load that depends on nothing is requested before the gate is looked at: control words, the partials, the
  // thread's first element of every vector and its place in the replay's image -- one memory round trip where the
  // gate, the partial sum, the control scalars and the vectors were four in a row (5.7 us on tiers.pyfg for 0.6 MB
  // vectors).  The empty asm keeps the compiler from sinking the loads behind the early return.
  const long i0 = (long)blockIdx.x * kBlock + threadIdx.x;
  const bool in0 = i0 < nelem;
  const GateWords gw = gate_words(ctl);
  double pv = ((int)threadIdx.x < np1) ? p1[threadIdx.x] : 0.0;
  const double z_r = ctl->z_r[par], d_Pd = ctl->d_Pd[par], e_Pe = ctl->e_Pe[par], e_Pd = ctl->e_Pd[par];
  const double Delta = ctl->Delta;
  double h0 = 0, dl0 = 0, et0 = 0, he0 = 0, rs0 = 0;
  int jp0 = -1;
  const long col0 = in0 ? i0 / r : 0;
  if (in0) {
    h0 = Hd[i0];
    dl0 = delta[i0];
    et0 = eta[i0];
    he0 = Heta[i0];
    rs0 = res[i0];
    if (sf.y) jp0 = sf.in_pos[col0];
  }
  asm volatile("" ::"v"(pv), "v"(h0), "v"(dl0), "v"(et0), "v"(he0), "v"(rs0), "v"(jp0), "s"(gw.outer), "s"(gw.tcg));
  if (gated(gw, ctl, seq, 2)) return;
  for (int i = threadIdx.x + blockDim.x; i < np1; i += blockDim.x) pv += p1[i];
  const double d_Hd = block_sum(pv, s_red);
  const double alpha = tcg_alpha(z_r, d_Hd);
  const double e_Pe_new = tcg_e_Pe_new(alpha, d_Pd, e_Pe, e_Pd);
  const bool boundary = tcg_boundary(d_Hd, e_Pe_new, Delta);
  const double step = boundary ? tcg_tau(d_Pd, e_Pe, e_Pd, Delta) : alpha;
  // a run that goes on says so before the vector work: the host enqueues the sparse replay behind this verdict
  // (DeviceProblem::RtrForm::replay); a run that stops writes tcg_done_seq below
  if (!boundary && blockIdx.x == 0 && threadIdx.x == 0) host_store(&hf->go_seq, seq);
  double acc = 0;
  if (in0) {
    eta[i0] = et0 + step * dl0;
    Heta[i0] = he0 + step * h0;
    if (!boundary) {
      const double rr = rs0 + alpha * h0;
      res[i0] = rr;
      acc += rr * rr;
      if (sf.y && jp0 >= 0) sf.y[(size_t)jp0 * r + (i0 - col0 * r)] = rr;
    }
  }
  for (long i = i0 + (long)gridDim.x * kBlock; i < nelem; i += (long)gridDim.x * kBlock) {
    const double h = Hd[i];
    eta[i] += step * delta[i];
    Heta[i] += step * h;
    if (!boundary) {
      const double rr = res[i] + alpha * h;
      res[i] = rr;
      acc += rr * rr;
      if (sf.y) {  // the replay's permute-in folded in: the new residual goes straight to its place in image 0
        const long col = i / r;
        const int jp = sf.in_pos[col];
        if (jp >= 0) sf.y[(size_t)jp * r + (i - col * r)] = rr;
      }
    }
  }
  const double tot = block_sum(acc, s_red);
  if (threadIdx.x == 0) p2[blockIdx.x] = tot;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ctl->alpha = alpha;
    ctl->e_Pe_n = e_Pe_new;
    if (boundary) tcg_end_run(ctl, hf, seq, tcg_boundary_status(d_Hd), iter + 1);
  }
}

__global__ __launch_bounds__(kBlock) void k_tcg_update2(long nelem, const double *__restrict__ z,
                                                        double *__restrict__ delta, const double *__restrict__ p3,
                                                        int np3, SolverCtl *ctl, HostFlags *hf, int seq, int iter) {
  if (gated(ctl, seq, 2)) return;
  __shared__ double s_red[16];
  const int par = iter & 1;
  const double z_r_new = sum_partials(p3, np3, 1, 0, s_red);
  const double beta = tcg_beta(z_r_new, ctl->z_r[par]);
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < nelem; i += (long)gridDim.x * kBlock)
    delta[i] = -z[i] + beta * delta[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    tcg_put_dir(ctl, par ^ 1, tcg_dir_next(z_r_new, beta, ctl->alpha, ctl->d_Pd[par], ctl->e_Pd[par]), ctl->e_Pe_n);
    if (iter + 1 >= ctl->max_inner) tcg_end_run_at_cap(ctl, hf, seq, iter + 1);
    host_store(&hf->last_seq_done, seq);
  }
}

// rho = (f1 - f2) / -(<eta, g> + 0.5 <eta, H eta>); accept iff rho > 0.1; radius update as RTRNewton
__global__ __launch_bounds__(kBlock) void k_rtr_decide(const double *pA, int npA, const double *pB, int npB,
                                                       const double *pC, int npC, SolverCtl *ctl, HostFlags *hf,
                                                       int seq, unsigned *tcg_sync, int nsync) {
  if (gated(ctl, seq, 1)) return;
  __shared__ double s_red[20];
  for (int i = threadIdx.x; i < nsync; i += kBlock) tcg_sync[i] = 0u;
  const double *const ps[5] = {pA, pA, pB, pC, pC};
  const int nps[5] = {npA, npA, npB, npC, npC}, sts[5] = {2, 2, 1, 2, 2}, offs[5] = {0, 1, 0, 0, 1};
  double sums[5];
  sum_partials_n<5>(ps, nps, sts, offs, s_red, sums);
  const double fq = sums[0], fg = sums[1], g2 = sums[2], eg = sums[3], eh = sums[4];
  if (threadIdx.x == 0) {
    const double f2 = 0.5 * fq + fg;
    const double rho = (ctl->f1 - f2) / (-(eg + 0.5 * eh));
    ctl->f2 = f2;
    ctl->rho = rho;
    if (rho > 0.75) {
      if (ctl->tcg_status == TR_NEGCURVTURE || ctl->tcg_status == TR_EXCREGION) ctl->Delta = fmin(2.0 * ctl->Delta, ctl->maxDelta);
    } else if (rho < 0.25) {
      ctl->Delta *= 0.25;
    }
    const bool accept = (rho > 0.1) && isfinite(rho);
    if (accept) {
      ctl->cur ^= 1;
      ctl->f1 = f2;
      ctl->ngf = sqrt(g2);
      ctl->accepted += 1;
      ctl->last_accepted = 1;
    } else {
      ctl->last_accepted = 0;
      host_store(&hf->reject_seq, seq);  // before last_seq_done below: the host reads it behind that word
    }
    ctl->outer_it += 1;
    if (ctl->ngf < ctl->tol || ctl->outer_it >= ctl->max_outer || (ctl->stop_on_accept && accept)) {
      ctl->outer_done_stamp = seq;
      host_store(&hf->outer_done_seq, seq);
    }
    host_store(&hf->last_seq_done, seq);
  }
}

void launch_rtr_init(hipStream_t st, const double *pA, int npA, const double *pB, int npB, SolverCtl *ctl,
                     HostFlags *hf, int seq, CtlInit ci, unsigned *tcg_sync, int nsync) {
  count_launch();
  hipLaunchKernelGGL(k_rtr_init, dim3(1), dim3(kBlock), 0, st, pA, npA, pB, npB, ctl, hf, seq, ci, tcg_sync, nsync);
}
void launch_tcg_begin(hipStream_t st, long nelem, Buf2 grad, double *eta, double *Heta, double *res,
                      SolverCtl *ctl, int seq) {
  hipLaunchKernelGGL(k_tcg_begin, dim3(vec_grid(nelem)), dim3(kBlock), 0, st, nelem, grad, eta, Heta, res, ctl,
                     seq);
}
void launch_tcg_update1(hipStream_t st, long nelem, const double *delta, const double *Hd, double *eta,
                        double *Heta, double *res, const double *p1, int np1, double *p2, SolverCtl *ctl,
                        HostFlags *hf, int seq, int iter, int r, SpFold sf) {
  hipLaunchKernelGGL(k_tcg_update1, dim3(vec_grid(nelem)), dim3(kBlock), 0, st, nelem, delta, Hd, eta, Heta, res,
                     p1, np1, p2, ctl, hf, seq, iter, r, sf);
}
void launch_tcg_update2(hipStream_t st, long nelem, const double *z, double *delta, const double *p3, int np3,
                        SolverCtl *ctl, HostFlags *hf, int seq, int iter) {
  hipLaunchKernelGGL(k_tcg_update2, dim3(vec_grid(nelem)), dim3(kBlock), 0, st, nelem, z, delta, p3, np3, ctl, hf,
                     seq, iter);
}
void launch_rtr_decide(hipStream_t st, const double *pA, int npA, const double *pB, int npB, const double *pC,
                       int npC, SolverCtl *ctl, HostFlags *hf, int seq, unsigned *tcg_sync, int nsync) {
  count_launch();
  hipLaunchKernelGGL(k_rtr_decide, dim3(1), dim3(kBlock), 0, st, pA, npA, pB, npB, pC, npC, ctl, hf, seq, tcg_sync,
                     nsync);
}

// ------------------------------------------------------------------------------------------------------
// plain vector helpers
// ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_axpby(long nelem, double a, const double *__restrict__ x, double b,
                                                  const double *__restrict__ y, double *__restrict__ out) {
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < nelem; i += (long)gridDim.x * kBlock)
    out[i] = a * x[i] + (y ? b * y[i] : 0.0);
}
void launch_axpby(hipStream_t st, long nelem, double a, const double *x, double b, const double *y, double *out) {
  hipLaunchKernelGGL(k_axpby, dim3(vec_grid(nelem)), dim3(kBlock), 0, st, nelem, a, x, b, y, out);
}

__global__ __launch_bounds__(kBlock) void k_sum_partials(const double *partials, int np, int stride, int count,
                                                         double *out) {
  __shared__ double s_red[16];
  for (int c = 0; c < count; ++c) {
    const double s = sum_partials(partials, np, stride, c, s_red);
    if (threadIdx.x == 0) out[c] = s;
  }
}
void launch_sum_partials(hipStream_t st, const double *partials, int np, int stride, int count, double *out) {
  hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(kBlock), 0, st, partials, np, stride, count, out);
}

__global__ __launch_bounds__(kBlock) void k_dot(long nelem, const double *__restrict__ x,
                                                const double *__restrict__ y, double *__restrict__ partials) {
  __shared__ double s_red[16];
  double acc = 0;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < nelem; i += (long)gridDim.x * kBlock)
    acc += x[i] * y[i];
  const double t = block_sum(acc, s_red);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}
void launch_dot(hipStream_t st, long nelem, const double *x, const double *y, double *partials) {
  hipLaunchKernelGGL(k_dot, dim3(vec_grid(nelem)), dim3(kBlock), 0, st, nelem, x, y, partials);
}

__global__ __launch_bounds__(kBlock) void k_gather_cols(int r, int ncols, const int *__restrict__ src,
                                                        const double *__restrict__ X, double *__restrict__ out) {
  const long N = (long)ncols * r;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < N; i += (long)gridDim.x * kBlock) {
    const int c = (int)(i / r), t = (int)(i - (long)c * r);
    out[i] = X[(size_t)src[c] * r + t];
  }
}
__global__ __launch_bounds__(kBlock) void k_scatter_cols(int r, int ncols, const int *__restrict__ dst,
                                                         const double *__restrict__ in, double *__restrict__ X) {
  const long N = (long)ncols * r;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < N; i += (long)gridDim.x * kBlock) {
    const int c = (int)(i / r), t = (int)(i - (long)c * r);
    X[(size_t)dst[c] * r + t] = in[i];
  }
}
void launch_gather_cols(hipStream_t st, int r, int ncols, const int *src_col, const double *X, double *out) {
  if (ncols <= 0) return;
  hipLaunchKernelGGL(k_gather_cols, dim3(vec_grid((long)ncols * r)), dim3(kBlock), 0, st, r, ncols, src_col, X, out);
}
void launch_scatter_cols(hipStream_t st, int r, int ncols, const int *dst_col, const double *in, double *X) {
  if (ncols <= 0) return;
  hipLaunchKernelGGL(k_scatter_cols, dim3(vec_grid((long)ncols * r)), dim3(kBlock), 0, st, r, ncols, dst_col, in, X);
}

// one block per agent: |A_a|^2 and <A_a, B_a> over the agent's column range
__global__ __launch_bounds__(kBlock) void k_block_dots(int r, const int *__restrict__ cs,
                                                       const double *__restrict__ A, const double *__restrict__ B,
                                                       double *__restrict__ out) {
  __shared__ double s_red[16];
  const int a = blockIdx.x;
  const long lo = (long)cs[a] * r, hi = (long)cs[a + 1] * r;
  double s0 = 0, s1 = 0;
  for (long i = lo + threadIdx.x; i < hi; i += kBlock) {
    const double x = A[i];
    s0 += x * x;
    if (B) s1 += x * B[i];
  }
  const double t0 = block_sum(s0, s_red);
  const double t1 = block_sum(s1, s_red);
  if (threadIdx.x == 0) {
    out[2 * a] = t0;
    out[2 * a + 1] = t1;
  }
}
void launch_block_dots(hipStream_t st, int r, int nagents, const int *col_start, const double *A, const double *B,
                       double *out) {
  hipLaunchKernelGGL(k_block_dots, dim3(nagents), dim3(kBlock), 0, st, r, col_start, A, B, out);
}

// ------------------------------------------------------------------------------------------------------
// Lanczos helpers (certification): basis V is n x nv column-major (ld = n)
// ------------------------------------------------------------------------------------------------------
constexpr int kLanczosMaxV = 24;
__global__ __launch_bounds__(kBlock) void k_lanczos_proj(int n, int nv, const double *__restrict__ V,
                                                         const double *__restrict__ w,
                                                         double *__restrict__ partials) {
  __shared__ double s_red[16];
  double acc[kLanczosMaxV];
#pragma unroll
  for (int i = 0; i < kLanczosMaxV; ++i) acc[i] = 0;
  for (long t = (long)blockIdx.x * kBlock + threadIdx.x; t < n; t += (long)gridDim.x * kBlock) {
    const double wt = w[t];
#pragma unroll
    for (int i = 0; i < kLanczosMaxV; ++i)
      if (i < nv) acc[i] += V[(size_t)i * n + t] * wt;
  }
#pragma unroll
  for (int i = 0; i < kLanczosMaxV; ++i)
    if (i < nv) {
      const double s = block_sum(acc[i], s_red);
      if (threadIdx.x == 0) partials[(size_t)blockIdx.x * kLanczosMaxV + i] = s;
    }
}
__global__ __launch_bounds__(kBlock) void k_lanczos_sub(int n, int nv, const double *__restrict__ V,
                                                        const double *__restrict__ h, double *__restrict__ w) {
  for (long t = (long)blockIdx.x * kBlock + threadIdx.x; t < n; t += (long)gridDim.x * kBlock) {
    double s = 0;
    for (int i = 0; i < nv; ++i) s += V[(size_t)i * n + t] * h[i];
    w[t] -= s;
  }
}
void launch_lanczos_proj(hipStream_t st, int n, int nv, const double *V, const double *w, double *partials) {
  hipLaunchKernelGGL(k_lanczos_proj, dim3(vec_grid(n)), dim3(kBlock), 0, st, n, nv, V, w, partials);
}
void launch_lanczos_sub(hipStream_t st, int n, int nv, const double *V, const double *h, double *w) {
  hipLaunchKernelGGL(k_lanczos_sub, dim3(vec_grid(n)), dim3(kBlock), 0, st, n, nv, V, h, w);
}
// The same subtraction with the sum over the blocks' partial projections in its prologue (every workgroup sums the
// npart x nv partials for itself: for the problem sizes this is used at -- npart <= kLanczosFuseParts -- that is a
// few KB from L2 per workgroup and saves the k_sum_partials launch); block 0 keeps the coefficients for the host,
// which assembles the projected matrix once per restart cycle instead of once per step.
__global__ __launch_bounds__(kBlock) void k_lanczos_sub_sum(int n, int nv, const double *__restrict__ V,
                                                            const double *__restrict__ partials, int npart,
                                                            double *__restrict__ hout, double *__restrict__ w,
                                                            double *__restrict__ dotpart) {
  __shared__ double s_h[kLanczosMaxV];
  __shared__ double s_red[16];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = wave; i < nv; i += kBlock / 64) {
    double s = 0;
    for (int b = lane; b < npart; b += 64) s += partials[(size_t)b * kLanczosMaxV + i];
    s = wave_sum(s);
    if (lane == 0) s_h[i] = s;
  }
  __syncthreads();
  if (blockIdx.x == 0 && (int)threadIdx.x < nv) hout[threadIdx.x] = s_h[threadIdx.x];
  double ww = 0;
  for (long t = (long)blockIdx.x * kBlock + threadIdx.x; t < n; t += (long)gridDim.x * kBlock) {
    double s = 0;
    for (int i = 0; i < nv; ++i) s += V[(size_t)i * n + t] * s_h[i];
    const double wn = w[t] - s;
    w[t] = wn;
    ww += wn * wn;
  }
  if (dotpart) {  // second pass: <w, w> of the finished vector rides along (the norm's own launch saved)
    const double tot = block_sum(ww, s_red);
    if (threadIdx.x == 0) dotpart[blockIdx.x] = tot;
  }
}
// h only (large problems keep k_sum_partials + k_lanczos_sub): copies the summed coefficients to the per-step store
__global__ void k_lanczos_keep(int nv, const double *__restrict__ h, double *__restrict__ hout) {
  if ((int)threadIdx.x < nv) hout[threadIdx.x] = h[threadIdx.x];
}
// next basis vector: beta = |w| from the partial sums of <w, w> (summed by every workgroup in its prologue),
// v_next = w / beta; block 0 keeps beta for the host.  A vanishing beta (invariant subspace) raises *flag and leaves
// v_next = 0: the host redoes that step on its slow path.
__global__ __launch_bounds__(kBlock) void k_lanczos_next(int n, const double *__restrict__ partials, int npart,
                                                         double *__restrict__ beta_out, int *__restrict__ flag,
                                                         const double *__restrict__ w, double *__restrict__ vnext,
                                                         const double *__restrict__ hrow, int nv) {
  __shared__ double s_red[16];
  double s = 0;
  for (int b = threadIdx.x; b < npart; b += kBlock) s += partials[b];
  const double b2 = block_sum(s, s_red);
  const double beta = sqrt(b2);
  // |S v_j|^2 = beta^2 + sum of the squared coefficients taken out by the two passes: a remainder at the rounding level
  // of that norm is no direction (kLanczosDead, shared with the host's per-step form)
  double h2 = 0;
  for (int i = 0; i < nv; ++i) {
    const double h = hrow[i] + hrow[32 + i];
    h2 += h * h;
  }
  const bool dead = !(beta > kLanczosDead * sqrt(h2 + b2)) || !(beta >= 1e-300);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *beta_out = dead ? 0.0 : beta;
    if (dead) *flag = 1;
  }
  const double inv = dead ? 0.0 : 1.0 / beta;
  for (long t = (long)blockIdx.x * kBlock + threadIdx.x; t < n; t += (long)gridDim.x * kBlock) vnext[t] = w[t] * inv;
}
void launch_lanczos_sub_sum(hipStream_t st, int n, int nv, const double *V, const double *partials, int npart,
                            double *hout, double *w, double *dotpart) {
  hipLaunchKernelGGL(k_lanczos_sub_sum, dim3(vec_grid(n)), dim3(kBlock), 0, st, n, nv, V, partials, npart, hout, w,
                     dotpart);
}
void launch_lanczos_keep(hipStream_t st, int nv, const double *h, double *hout) {
  hipLaunchKernelGGL(k_lanczos_keep, dim3(1), dim3(64), 0, st, nv, h, hout);
}
void launch_lanczos_next(hipStream_t st, int n, const double *partials, int npart, double *beta_out, int *flag,
                         const double *w, double *vnext, const double *hrow, int nv) {
  hipLaunchKernelGGL(k_lanczos_next, dim3(vec_grid(n)), dim3(kBlock), 0, st, n, partials, npart, beta_out, flag, w,
                     vnext, hrow, nv);
}
__global__ __launch_bounds__(kBlock) void k_scale_shift(int n, double shift, const double *__restrict__ x,
                                                        double *__restrict__ y) {
  for (long t = (long)blockIdx.x * kBlock + threadIdx.x; t < n; t += (long)gridDim.x * kBlock) y[t] -= shift * x[t];
}
void launch_scale_shift(hipStream_t st, int n, double shift, const double *x, double *y) {
  hipLaunchKernelGGL(k_scale_shift, dim3(vec_grid(n)), dim3(kBlock), 0, st, n, shift, x, y);
}
__global__ __launch_bounds__(kBlock) void k_scale(int n, const double *__restrict__ nrm2,
                                                  const double *__restrict__ w, double *__restrict__ out) {
  const double inv = 1.0 / sqrt(*nrm2);
  for (long t = (long)blockIdx.x * kBlock + threadIdx.x; t < n; t += (long)gridDim.x * kBlock) out[t] = w[t] * inv;
}
void launch_scale(hipStream_t st, int n, const double *nrm2, const double *w, double *out) {
  hipLaunchKernelGGL(k_scale, dim3(vec_grid(n)), dim3(kBlock), 0, st, n, nrm2, w, out);
}

}  // namespace dcora
