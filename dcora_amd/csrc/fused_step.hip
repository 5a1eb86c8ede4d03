// Fused truncated-CG kernels for the SE layout (pose graphs), r <= 8: three launches per tCG iteration.
//
//   A  k_fused_hess     delta = -z + beta delta  (on the fly while gathering),  W = delta Q  (CSR rows staged in
//                       LDS),  H delta = Proj_X(W - delta S),  partial <delta, H delta>
//   B  k_fused_precond  alpha / boundary test, eta += a delta, H eta += a H delta, r += a H delta, partial |r|^2,
//                       Z_s = r (Q + reg I)^-1 restricted to a slice of rows (split-K over the dense inverse)
//   C  k_fused_finish   residual stopping rule, z = Proj_X(sum_s Z_s), partial <z, r>
//
// Every global reduction of the CG recurrence sits exactly on a kernel boundary, so an iteration costs three
// dependent launches instead of six.  Per-pose arithmetic uses 8 lanes per pose: lane t
// of a group owns row t of the pose's r x (d+1) block, d x d Gram matrices are reduced with 3 xor-shuffles.
//
// B + C also run as ONE launch (k_fused_pc) where that wins.  The one-launch run is fused_run.hip, the evaluations
// fused_eval.hip, the manifold kernels fused_pose.hip.
#include <algorithm>

#include "kernels.h"
#include "tcg_rules.h"
#include "pose_group.h"
#include "fused_pc.h"

namespace dcora {

namespace {

// ------------------------------------------------------------------------------------------------------
// A: Hessian-vector product of the tCG direction, with the direction update folded into the gather.
//    Phase 1: W = delta Q, one thread per output element, CSR rows of the block staged in LDS.
//    Phase 2: H delta = Proj_X(W - delta S) with 8 lanes per pose, operands handed over through LDS.
// ------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kBlock) void k_fused_hess(ManiDesc m, CsrDev Q, const double *__restrict__ z,
                                                       const double *__restrict__ d_old,
                                                       double *__restrict__ d_new, Buf2 Xb, Buf2 Sb,
                                                       double *__restrict__ Hd, const double *__restrict__ p3,
                                                       int np3, double *__restrict__ p1, SolverCtl *ctl, int seq,
                                                       int iter) {
  // control scalars first (one batch of scalar loads); the gate itself is evaluated after the data loads below
  // have been issued, so a kernel pays one memory round trip, not two
  const int par = iter & 1;
  const int st_o = ctl->outer_done_stamp, st_t = ctl->tcg_done_stamp, cur = ctl->cur & 1;
  const double c_zr = ctl->z_r[par ^ 1], c_alpha = ctl->alpha, c_dPd = ctl->d_Pd[par ^ 1], c_ePd = ctl->e_Pd[par ^ 1],
               c_ePen = ctl->e_Pe_n;
  __shared__ int s_ci[kHessTile];
  __shared__ double s_v[kHessTile];
  __shared__ double s_W[kBlock], s_D[kBlock];
  __shared__ double s_red[16];
  constexpr int DH = D + 1;
  const int r = m.r;
  const int PB = fused_pb(r, DH);
  const int pose0 = blockIdx.x * PB;
  const int npose = min(PB, m.n - pose0);
  const int j0 = pose0 * DH, ncol = npose * DH, nout = ncol * r;
  // ---- independent loads first: first CSR tile into LDS, own entries, pose operands (latency overlaps the
  //      dependent scalar prologue below) ----
  const int e = threadIdx.x;
  const bool act = e < nout;
  const int lc = e / r, t = e - lc * r;
  const int j = j0 + lc;
  const int pbeg = Q.rp[j0], pend = Q.rp[j0 + ncol];
  const int myb = act ? Q.rp[j] : 0, mye = act ? Q.rp[j + 1] : 0;
  // <z, r> partials first (predicated loads; the loop below only runs for > 256 partials)
  const bool p3_wave = np3 <= 256;
  const int pi3 = f_partial_index(np3);
  double myp = p3_wave ? f_partial4_load(p3, np3) : ((pi3 < np3) ? p3[pi3] : 0.0);
  {
    // first tile of the matrix: all trips' loads are issued before any is stored to LDS (clamped index, straight
    // line), one memory round trip instead of one per 256 entries
    const int cnt = min(kHessTile, pend - pbeg);
    constexpr int SU = kHessTile / kBlock;
    int ci_r[SU];
    double v_r[SU];
    const int last = max(pend - 1, 0);
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const int i = min(pbeg + (int)threadIdx.x + u * kBlock, last);
      ci_r[u] = Q.ci[i];
      v_r[u] = Q.v[i];
    }
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const int i = threadIdx.x + u * kBlock;
      if (i < cnt) {
        s_ci[i] = ci_r[u];
        s_v[i] = v_r[u];
      }
    }
  }
  const size_t oown = (size_t)j * r + t;
  const double z_own = act ? z[oown] : 0.0;
  const double d_own = (act && iter > 0) ? d_old[oown] : 0.0;
  const int g = threadIdx.x >> 3, tt = threadIdx.x & (GW - 1);
  const bool pact = (g < npose) && (tt < r);
  const size_t o = (size_t)(pose0 + g) * DH * r;
  const double *__restrict__ X = Xb.p[cur];
  const double *__restrict__ Sblk = Sb.p[cur];
  Row<D> Y;
  ld_row<D>(X + o, r, tt, pact, Y);
  double S[D][D];
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) S[a][b] = (g < npose) ? Sblk[(size_t)(pose0 + g) * D * D + a + b * D] : 0.0;
  for (int i = threadIdx.x + kBlock; i < np3; i += kBlock) myp += p3[i];
  if (seq > st_o || seq > st_t) return;  // solve or tCG already finished: no-op (uniform over the grid)
  __syncthreads();  // first tile staged
  // first batch of gathers: addresses do not depend on beta, so the loads are issued before the reduction
  constexpr int GB = 16;
  double ga[GB], gz[GB], gw[GB];
  const int lo0 = myb - pbeg;
  const int hi0 = min(mye, pbeg + kHessTile) - pbeg;
#pragma unroll
  for (int q = 0; q < GB; ++q) {
    const bool ok = act && (lo0 + q < hi0);
    const size_t oo = ok ? (size_t)s_ci[lo0 + q] * r + t : 0;
    gw[q] = ok ? s_v[lo0 + q] : 0.0;
    gz[q] = z[oo];
    ga[q] = (iter > 0) ? d_old[oo] : 0.0;
  }
  // ---- scalar recurrence (tcg_rules.h) ----
  const double z_r_new = p3_wave ? wave_sum(myp) : f_partial_total(myp, np3, s_red);
  double beta = 0;
  if (iter > 0) beta = tcg_beta(z_r_new, c_zr);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (iter == 0)
      tcg_put_dir(ctl, 0, tcg_dir_start(z_r_new), 0.0);
    else
      tcg_put_dir(ctl, par, tcg_dir_next(z_r_new, beta, c_alpha, c_dPd, c_ePd), c_ePen);
  }
  // ---- phase 1 ----
  double acc = 0;
#pragma unroll
  for (int q = 0; q < GB; ++q) acc += gw[q] * (beta * ga[q] - gz[q]);
  for (int base = pbeg; base < pend; base += kHessTile) {
    const int cnt = min(kHessTile, pend - base);
    if (base != pbeg) {
      __syncthreads();
      for (int i = threadIdx.x; i < cnt; i += kBlock) {
        s_ci[i] = Q.ci[base + i];
        s_v[i] = Q.v[base + i];
      }
      __syncthreads();
    }
    int lo = max(myb, base) - base;
    const int hi = min(mye, base + cnt) - base;
    if (base == pbeg) lo += GB;  // already consumed above
    for (int p = lo; p < hi; p += 8) {
      double a8[8], b8[8], w8[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const bool ok = p + q < hi;
        const size_t oo = ok ? (size_t)s_ci[p + q] * r + t : 0;
        w8[q] = ok ? s_v[p + q] : 0.0;
        b8[q] = z[oo];
        a8[q] = (iter > 0) ? d_old[oo] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) acc += w8[q] * (beta * a8[q] - b8[q]);
    }
  }
  if (act) {
    const double dn = (iter > 0) ? beta * d_own - z_own : -z_own;
    d_new[oown] = dn;
    s_W[e] = acc;
    s_D[e] = dn;
  }
  __syncthreads();
  // ---- phase 2 ----
  Row<D> V, W;
#pragma unroll
  for (int a = 0; a < DH; ++a) {
    W.e[a] = pact ? s_W[(g * DH + a) * r + tt] : 0.0;
    V.e[a] = pact ? s_D[(g * DH + a) * r + tt] : 0.0;
  }
  row_sub_AS<D>(W, V, S);
  row_tangent<D>(Y, W);
  st_row<D>(Hd + o, r, tt, pact, W);
  double dacc = 0;
#pragma unroll
  for (int a = 0; a < DH; ++a) dacc += V.e[a] * W.e[a];
  const double tot = block_sum(dacc, s_red);
  if (threadIdx.x == 0) p1[blockIdx.x] = tot;
}

// A on the block structure of Q (pose graphs large enough to carry the block-CSR copy): 8 lanes per pose from the
// start, so phase 1 leaves W in the lane layout phase 2 works in (no LDS hand-over), one gather of the neighbour's
// (d+1) r values per matrix block instead of (d+1)^2 scalar entries.  32 poses per workgroup.
template <int D>
__global__ __launch_bounds__(kBlock) void k_fused_hess_bsr(ManiDesc m, BsrDev A, const double *__restrict__ z,
                                                           const double *__restrict__ d_old,
                                                           double *__restrict__ d_new, Buf2 Xb, Buf2 Sb,
                                                           double *__restrict__ Hd, const double *__restrict__ p3,
                                                           int np3, double *__restrict__ p1, SolverCtl *ctl, int seq,
                                                           int iter) {
  const int par = iter & 1;
  const int st_o = ctl->outer_done_stamp, st_t = ctl->tcg_done_stamp, cur = ctl->cur & 1;
  const double c_zr = ctl->z_r[par ^ 1], c_alpha = ctl->alpha, c_dPd = ctl->d_Pd[par ^ 1], c_ePd = ctl->e_Pd[par ^ 1],
               c_ePen = ctl->e_Pe_n;
  constexpr int DH = D + 1, BS = DH * DH;
  __shared__ double s_bv[kBsrTile * BS];
  __shared__ int s_bc[kBsrTile];
  __shared__ double s_red[16];
  const int r = m.r;
  const int pose0 = blockIdx.x * kPosesPerBlock;
  const int g = threadIdx.x >> 3, tt = threadIdx.x & (GW - 1);
  const int pose = pose0 + g;
  const bool inr = pose < m.n;
  const bool pact = inr && (tt < r);
  const size_t o = (size_t)pose * DH * r;
  const int pi3 = f_partial_index(np3);
  double myp = (pi3 < np3) ? p3[pi3] : 0.0;
  const int pend_pose = min(m.n, pose0 + kPosesPerBlock);
  const int bbeg = A.bp[pose0], bend = A.bp[pend_pose];
  const int myb = inr ? A.bp[pose] : 0, mye = inr ? A.bp[pose + 1] : 0;
  // own rows of z / d_old, pose operands
  Row<D> Zo, Do, Y;
  ld_row<D>(z + o, r, tt, pact, Zo);
  if (iter > 0) {
    ld_row<D>(d_old + o, r, tt, pact, Do);
  } else {
#pragma unroll
    for (int a = 0; a < DH; ++a) Do.e[a] = 0.0;
  }
  const double *__restrict__ X = Xb.p[cur];
  const double *__restrict__ Sblk = Sb.p[cur];
  ld_row<D>(X + o, r, tt, pact, Y);
  double S[D][D];
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) S[a][b] = inr ? Sblk[(size_t)pose * D * D + a + b * D] : 0.0;
  for (int i = threadIdx.x + kBlock; i < np3; i += kBlock) myp += p3[i];
  if (seq > st_o || seq > st_t) return;  // solve or tCG already finished: no-op (uniform over the grid)
  const double z_r_new = f_partial_total(myp, np3, s_red);
  double beta = 0;
  if (iter > 0) beta = tcg_beta(z_r_new, c_zr);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (iter == 0)
      tcg_put_dir(ctl, 0, tcg_dir_start(z_r_new), 0.0);
    else
      tcg_put_dir(ctl, par, tcg_dir_next(z_r_new, beta, c_alpha, c_dPd, c_ePd), c_ePen);
  }
  // ---- phase 1: W = d_new Q over the pose's block row, d_new = beta d_old - z formed in the gather ----
  Row<D> W, V;
#pragma unroll
  for (int a = 0; a < DH; ++a) W.e[a] = 0.0;
  for (int base = bbeg; base < bend; base += kBsrTile) {
    const int cnt = min(kBsrTile, bend - base);
    __syncthreads();
    {
      constexpr int SU = (kBsrTile * BS / 2 + kBlock - 1) / kBlock;
      const double2 *__restrict__ src = reinterpret_cast<const double2 *>(A.bv + (size_t)base * BS);
      const int n2 = cnt * BS / 2;
      double2 v_r[SU];
      const int bc_r = A.bc[base + min((int)threadIdx.x, cnt - 1)];
      if ((BS & 1) == 0) {
#pragma unroll
        for (int u = 0; u < SU; ++u) v_r[u] = src[min((int)threadIdx.x + u * kBlock, n2 - 1)];
#pragma unroll
        for (int u = 0; u < SU; ++u) {
          const int i = threadIdx.x + u * kBlock;
          if (i < n2) reinterpret_cast<double2 *>(s_bv)[i] = v_r[u];
        }
      } else {
        for (int i = threadIdx.x; i < cnt * BS; i += kBlock) s_bv[i] = A.bv[(size_t)base * BS + i];
      }
      if ((int)threadIdx.x < cnt) s_bc[threadIdx.x] = bc_r;
      for (int i = threadIdx.x + kBlock; i < cnt; i += kBlock) s_bc[i] = A.bc[base + i];
    }
    __syncthreads();
    const int lo = max(myb, base) - base, hi = min(mye, base + cnt) - base;
    for (int b = lo; b < hi; b += 4) {
      double xz[4][DH], xd[4][DH];
      int bb[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool ok = pact && (b + q < hi);
        bb[q] = (b + q < hi) ? b + q : b;
        const size_t oo = (size_t)s_bc[bb[q]] * DH * r + tt;
#pragma unroll
        for (int c = 0; c < DH; ++c) {
          xz[q][c] = ok ? z[oo + c * r] : 0.0;
          xd[q][c] = (ok && iter > 0) ? d_old[oo + c * r] : 0.0;
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double *__restrict__ Bq = s_bv + bb[q] * BS;
#pragma unroll
        for (int a = 0; a < DH; ++a) {
          double s = 0;
#pragma unroll
          for (int c = 0; c < DH; ++c) s += Bq[c * DH + a] * (beta * xd[q][c] - xz[q][c]);
          W.e[a] += s;
        }
      }
    }
  }
#pragma unroll
  for (int a = 0; a < DH; ++a) V.e[a] = (iter > 0) ? beta * Do.e[a] - Zo.e[a] : -Zo.e[a];
  st_row<D>(d_new + o, r, tt, pact, V);
  // ---- phase 2 ----
  row_sub_AS<D>(W, V, S);
  row_tangent<D>(Y, W);
  st_row<D>(Hd + o, r, tt, pact, W);
  double dacc = 0;
#pragma unroll
  for (int a = 0; a < DH; ++a) dacc += V.e[a] * W.e[a];
  if (!pact) dacc = 0;
  const double tot = block_sum(dacc, s_red);
  if (threadIdx.x == 0) p1[blockIdx.x] = tot;
}

// ------------------------------------------------------------------------------------------------------
// B: step length, vector updates and the dense preconditioner product, split over row slices of Minv.
//    first != 0: start of a tCG run (res = grad, eta = H eta = 0, no step).
//    The updated residual slice is staged once in LDS; each wave then streams whole rows of the symmetric
//    inverse with 16-byte loads (lane l owns output columns 2l, 2l+1 of the block's 128-column chunk),
//    eight rows in flight per lane, and reads the residual entries as LDS broadcasts.
// ------------------------------------------------------------------------------------------------------
constexpr int kJChunk = 128;  // output columns per block
constexpr int kRowChunk = 256;  // residual rows staged per pass

template <int RM, bool HAS_M>
__global__ __launch_bounds__(kBlock) void k_fused_precond(int r, int k, int ldm, int nsplit,
                                                          const double *__restrict__ Minv, Buf2 gradb,
                                                          const double *__restrict__ delta,
                                                          const double *__restrict__ Hd, double *__restrict__ eta,
                                                          double *__restrict__ Heta,
                                                          const double *__restrict__ res_old,
                                                          double *__restrict__ res_new,
                                                          double *__restrict__ Zpart, const double *__restrict__ p1,
                                                          int np1, double *__restrict__ p2, SolverCtl *ctl,
                                                          HostFlags *hf, int seq, int iter, int first, SpFold sf) {
  const int par = iter & 1;
  const int st_o = ctl->outer_done_stamp, st_t = ctl->tcg_done_stamp, cur = ctl->cur & 1;
  const double c_zr = ctl->z_r[par], c_dPd = ctl->d_Pd[par], c_ePe = ctl->e_Pe[par], c_ePd = ctl->e_Pd[par],
               c_Delta = ctl->Delta, c_ngf = ctl->ngf;
  __shared__ double s_red[16];
  __shared__ double s_buf[(kBlock / 64) * RM * kJChunk];  // residual slice, then the cross-wave reduction
  const long N = (long)r * k;
  // ---- row slice of this block / wave, and the first kPre rows of the inverse preloaded into registers: the
  //      loads do not depend on the step length, so their latency overlaps the scalar prologue ----
  constexpr int kPre = 16;
  const int njc = (k + kJChunk - 1) / kJChunk;
  const int jc = blockIdx.x % njc, s = blockIdx.x / njc;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int rows_per_split = (k + nsplit - 1) / nsplit;
  const int c_lo = min(k, s * rows_per_split), c_hi = min(k, c_lo + rows_per_split);
  const int col = jc * kJChunk + 2 * lane;
  const int cn0 = min(kRowChunk, c_hi - c_lo);
  const int per_wave0 = (cn0 + 3) / 4;
  const int w_lo0 = min(cn0, wave * per_wave0);
  const double *__restrict__ rsrc = first ? gradb.p[cur] : res_old;
  // own element of the vector updates and own entries of the residual slice: loaded before alpha is known
  const long i0 = (long)blockIdx.x * kBlock + threadIdx.x;
  const bool own = i0 < N;
  double o_h = 0, o_d = 0, o_eta = 0, o_Heta = 0, o_r = 0;
  if (own) {
    o_r = rsrc[i0];
    if (!first) {
      o_h = Hd[i0];
      o_d = delta[i0];
      o_eta = eta[i0];
      o_Heta = Heta[i0];
    }
  }
  constexpr int kStagePre = 2;  // staged residual entries preloaded per thread
  double st_r[kStagePre], st_h[kStagePre];
#pragma unroll
  for (int u = 0; u < kStagePre; ++u) {
    const int i = threadIdx.x + u * kBlock;
    const bool ok = i < cn0 * r;
    const size_t idx = (size_t)c_lo * r + (ok ? i : 0);
    st_r[u] = ok ? rsrc[idx] : 0.0;
    st_h[u] = (ok && !first) ? Hd[idx] : 0.0;
  }
  // <d, H d> partials: one predicated load per thread (a loop would wait for its loads inside the loop)
  const int pi1 = f_partial_index(np1);
  double myp = (!first && pi1 < np1) ? p1[pi1] : 0.0;
  // The rows of the inverse are requested AFTER the few words the step length needs: vector loads retire in issue
  // order, so the scalar prologue below (two block reductions, the vector updates) waits for those words only and
  // runs while the 64 KB of the slice are still in flight, instead of behind them.
  asm volatile("" ::: "memory");
  // Straight-line loads (row index clamped, value masked afterwards) so that the compiler can count them: behind
  // per-row branches it falls back to s_waitcnt vmcnt(0) at the first use of ANY loaded value.
  double2 pre[kPre];
  if (HAS_M) {
    const int col_c = min(col, ldm - 2);
#pragma unroll
    for (int q = 0; q < kPre; ++q) {
      const int row = min(c_lo + w_lo0 + q, k - 1);
      pre[q] = *reinterpret_cast<const double2 *>(Minv + (size_t)row * ldm + col_c);
    }
  }
  asm volatile("" ::: "memory");
  if (!first)
    for (int i = threadIdx.x + kBlock; i < np1; i += kBlock) myp += p1[i];  // only blocks of > 8192 poses get here
  if (seq > st_o || (!first && seq > st_t)) return;  // finished: no-op (uniform over the grid)
  double alpha = 0, step = 0;
  bool boundary = false;
  if (!first) {
    const double d_Hd = f_partial_total(myp, np1, s_red);
    alpha = tcg_alpha(c_zr, d_Hd);
    const double e_Pe_new = tcg_e_Pe_new(alpha, c_dPd, c_ePe, c_ePd);
    boundary = tcg_boundary(d_Hd, e_Pe_new, c_Delta);
    step = boundary ? tcg_tau(c_dPd, c_ePe, c_ePd, c_Delta) : alpha;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      ctl->alpha = alpha;
      ctl->e_Pe_n = e_Pe_new;
      if (boundary) {
        tcg_end_run(ctl, hf, seq, tcg_boundary_status(d_Hd), iter + 1);
      } else {
        // the host enqueues what follows a B that goes on only once it knows (DeviceProblem::RtrForm::replay)
        host_store(&hf->go_seq, seq);
      }
    }
  }
  if (first && blockIdx.x == 0 && threadIdx.x == 0) tcg_begin_run(ctl, c_ngf);
  // ---- element-wise updates (each element exactly once over the grid) ----
  double acc2 = 0;
  if (own) {
    if (first) {
      eta[i0] = 0;
      Heta[i0] = 0;
      res_new[i0] = o_r;
      if (!HAS_M && sf.y) sf.y[(size_t)sf.in_pos[i0 / r] * r + (i0 % r)] = o_r;
    } else {
      eta[i0] = o_eta + step * o_d;
      Heta[i0] = o_Heta + step * o_h;
      if (!boundary) {
        const double rr = o_r + alpha * o_h;
        res_new[i0] = rr;
        if (!HAS_M && sf.y) sf.y[(size_t)sf.in_pos[i0 / r] * r + (i0 % r)] = rr;
        acc2 += rr * rr;
      }
    }
  }
  for (long i = i0 + (long)gridDim.x * kBlock; i < N; i += (long)gridDim.x * kBlock) {
    if (first) {
      eta[i] = 0;
      Heta[i] = 0;
      res_new[i] = rsrc[i];
      if (!HAS_M && sf.y) sf.y[(size_t)sf.in_pos[i / r] * r + (i % r)] = rsrc[i];
    } else {
      const double h = Hd[i];
      eta[i] += step * delta[i];
      Heta[i] += step * h;
      if (!boundary) {
        const double rr = res_old[i] + alpha * h;
        res_new[i] = rr;
        if (!HAS_M && sf.y) sf.y[(size_t)sf.in_pos[i / r] * r + (i % r)] = rr;
        acc2 += rr * rr;
      }
    }
  }
  if (!first) {
    const double tot = block_sum(acc2, s_red);
    if (threadIdx.x == 0) p2[blockIdx.x] = tot;
  }
  if (boundary || !HAS_M) return;
  // ---- dense product slice: Z_s(:, j) = sum_{c in slice} r(:, c) Minv(c, j) ----
  double a0[RM], a1[RM];
#pragma unroll
  for (int t = 0; t < RM; ++t) a0[t] = a1[t] = 0;
  for (int c0 = c_lo; c0 < c_hi; c0 += kRowChunk) {
    const int cn = min(kRowChunk, c_hi - c0);
    __syncthreads();
    if (c0 == c_lo) {
#pragma unroll
      for (int u = 0; u < kStagePre; ++u) {
        const int i = threadIdx.x + u * kBlock;
        if (i < cn * r) s_buf[i] = st_r[u] + alpha * st_h[u];
      }
    }
    for (int i = threadIdx.x + (c0 == c_lo ? kStagePre * kBlock : 0); i < cn * r; i += kBlock) {
      const size_t idx = (size_t)c0 * r + i;
      double x = rsrc[idx];
      if (!first) x += alpha * Hd[idx];
      s_buf[i] = x;
    }
    __syncthreads();
    const int per_wave = (cn + 3) / 4;
    const int w_lo = min(cn, wave * per_wave), w_hi = min(cn, w_lo + per_wave);
    int c = w_lo;
    if (c0 == c_lo) {
      // rows preloaded before the prologue (those past the wave's range were clamped: masked here)
#pragma unroll
      for (int q = 0; q < kPre; ++q) {
        const bool ok = (w_lo + q < w_hi);
        if (!ok) pre[q].x = pre[q].y = 0.0;
#pragma unroll
        for (int t = 0; t < RM; ++t)
          if (t < r) {
            const double x = ok ? s_buf[(w_lo + q) * r + t] : 0.0;
            a0[t] += x * pre[q].x;
            a1[t] += x * pre[q].y;
          }
      }
      c = min(w_hi, w_lo + kPre);
    }
    const double *__restrict__ mp = Minv + (size_t)(c0 + c) * ldm + col;
    for (; c + 8 <= w_hi; c += 8) {
      double2 mm[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) mm[q] = *reinterpret_cast<const double2 *>(mp + (size_t)q * ldm);
      mp += 8 * (size_t)ldm;
#pragma unroll
      for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int t = 0; t < RM; ++t)
          if (t < r) {
            const double x = s_buf[(c + q) * r + t];
            a0[t] += x * mm[q].x;
            a1[t] += x * mm[q].y;
          }
    }
    for (; c < w_hi; ++c) {
      const double2 m0 = *reinterpret_cast<const double2 *>(mp);
      mp += ldm;
#pragma unroll
      for (int t = 0; t < RM; ++t)
        if (t < r) {
          const double x = s_buf[c * r + t];
          a0[t] += x * m0.x;
          a1[t] += x * m0.y;
        }
    }
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < RM; ++t) {
    s_buf[(wave * RM + t) * kJChunk + 2 * lane] = a0[t];
    s_buf[(wave * RM + t) * kJChunk + 2 * lane + 1] = a1[t];
  }
  __syncthreads();
  const int ncol = min(kJChunk, k - jc * kJChunk);
  double *__restrict__ zp = Zpart + (size_t)s * N + (size_t)jc * kJChunk * r;
  for (int e = threadIdx.x; e < ncol * r; e += kBlock) {
    const int cc = e / r, t = e - cc * r;
    double v = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) v += s_buf[(w * RM + t) * kJChunk + cc];
    zp[e] = v;
  }
}

// ------------------------------------------------------------------------------------------------------
// C: residual stopping rule, z = Proj_X(sum of the split-K slices), partial <z, r>
//    Phase 1 sums the slices with one thread per element (coalesced), phase 2 projects with 8 lanes per pose.
// ------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kBlock) void k_fused_finish(ManiDesc m, int nsplit, Buf2 Xb,
                                                         const double *__restrict__ Zpart,
                                                         const double *__restrict__ res, double *__restrict__ z,
                                                         const double *__restrict__ p2, int np2,
                                                         double *__restrict__ p3, SolverCtl *ctl, HostFlags *hf,
                                                         int seq, int iter, int first, SpFold sf,
                                                         double *__restrict__ zraw) {
  const int st_o = ctl->outer_done_stamp, st_t = ctl->tcg_done_stamp, cur = ctl->cur & 1;
  const double c_n0 = ctl->norm_r0;
  const int c_max_inner = ctl->max_inner;
  __shared__ double s_red[16];
  __shared__ double s_Z[kBlock], s_R[kBlock];
  constexpr int DH = D + 1;
  const int r = m.r;
  const long N = (long)r * m.k;
  const int PB = fused_pb(r, DH);
  const int pose0 = blockIdx.x * PB;
  const int npose = min(PB, m.n - pose0);
  const int nout = npose * DH * r;
  const size_t base = (size_t)pose0 * DH * r;
  // Every load of the kernel is issued before the first value is consumed: the |r|^2 partials the stopping rule
  // needs (two predicated loads per thread; a loop would wait for each trip's load inside the loop), the pose rows,
  // the residual entry and the split-K slices.  One memory round trip instead of three dependent ones.
  const double *__restrict__ X = Xb.p[cur];
  const int g = threadIdx.x >> 3, tt = threadIdx.x & (GW - 1);
  const bool pact = (g < npose) && (tt < r);
  const size_t o = base + (size_t)g * DH * r;
  const int e = threadIdx.x;
  double myp = 0, myp2 = 0;
  if (!first) {
    myp = (e < np2) ? p2[e] : 0.0;
    myp2 = (e + kBlock < np2) ? p2[e + kBlock] : 0.0;
  }
  Row<D> Y, Zr, Rr;
  ld_row<D>(X + o, r, tt, pact, Y);
  // ---- phase 1 (independent of the stopping rule): slice sum, residual entry ----
  if (e < nout) {
    const double rres = res[base + e];
    double zs = 0;
    if (sf.y) {  // sparse preconditioner folded in: the value sits in the replay vector, at its final position
      const size_t ge = base + e;
      zs = sf.y[(size_t)sf.out_pos[ge / r] * r + (ge % r)];
    } else {
      double q[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) q[u] = (u < nsplit) ? Zpart[(size_t)u * N + base + e] : 0.0;
#pragma unroll
      for (int u = 0; u < 32; ++u) zs += q[u];
      for (int s = 32; s < nsplit; ++s) zs += Zpart[(size_t)s * N + base + e];
    }
    s_Z[e] = zs;
    s_R[e] = rres;
    // z0 = P grad of an RTR iteration, unprojected: a rejected step leaves the iterate and its gradient where they
    // were, and the next iteration starts from this copy instead of another application of the preconditioner
    if (zraw) zraw[base + e] = zs;
  }
  myp += myp2;
  if (!first)
    for (int i = e + 2 * kBlock; i < np2; i += kBlock) myp += p2[i];
  if (seq > st_o || (!first && seq > st_t)) return;  // finished: no-op (uniform over the grid)
  if (!first) {
    const double nr = sqrt(block_sum(myp, s_red));
    if (tcg_residual_done(nr, c_n0)) {
      if (blockIdx.x == 0 && threadIdx.x == 0) tcg_end_run(ctl, hf, seq, tcg_residual_status(c_n0), iter + 1);
      return;
    }
  }
  __syncthreads();
  // ---- phase 2 ----
#pragma unroll
  for (int a = 0; a < DH; ++a) {
    Zr.e[a] = pact ? s_Z[(g * DH + a) * r + tt] : 0.0;
    Rr.e[a] = pact ? s_R[(g * DH + a) * r + tt] : 0.0;
  }
  row_tangent<D>(Y, Zr);
  st_row<D>(z + o, r, tt, pact, Zr);
  double acc = 0;
#pragma unroll
  for (int a = 0; a < DH; ++a) acc += Zr.e[a] * Rr.e[a];
  const double tot = block_sum(acc, s_red);
  if (threadIdx.x == 0) p3[blockIdx.x] = tot;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (!first && iter + 1 >= c_max_inner) tcg_end_run_at_cap(ctl, hf, seq, iter + 1);
    host_store(&hf->last_seq_done, seq);
  }
}

// ------------------------------------------------------------------------------------------------------
// B + C in ONE launch for the dense preconditioner (k <= 8000): no split-K, so no slice sum and no boundary between
// the product and its projection.  A workgroup owns PB whole poses = PB (d+1) output columns of z.  By symmetry of
// the inverse, column j of (Q + reg I)^-1 is row j: the workgroup streams its PB (d+1) rows (contiguous, 16-byte
// loads, wave w takes rows w, w + 4, ...) against the WHOLE updated residual, which every workgroup rebuilds for
// itself in LDS from r_old and H delta (2 r k doubles from L2 -- a quarter more bytes than the inverse itself, but
// from the cache level with four times the bandwidth).  Because every workgroup holds the whole residual it also
// knows |r|^2 (same summation order everywhere, bitwise the same value), so the stopping rule needs no kernel
// boundary either.  Per tCG iteration: A, then this kernel -- two dependent launches instead of three.
// ------------------------------------------------------------------------------------------------------
// R: the relaxation rank when it is known at compile time (no predication in the inner loops), 0 = run-time r <= 8.
// MULTI: the residual does not fit one LDS chunk (k > chk): the loop over further chunks is compiled in.
template <int D, int PB, int R, bool MULTI>
__global__ __launch_bounds__(kPcBlock) void k_fused_pc(ManiDesc m, int ldm, int chk, const double *__restrict__ Minv,
                                                       Buf2 gradb, Buf2 Xb, const double *__restrict__ delta,
                                                       const double *__restrict__ Hd, double *__restrict__ eta,
                                                       double *__restrict__ Heta, const double *__restrict__ res_old,
                                                       double *__restrict__ res_new, double *__restrict__ z,
                                                       const double *__restrict__ p1, int np1,
                                                       double *__restrict__ p3, SolverCtl *ctl, HostFlags *hf, int seq,
                                                       int iter, int first, double *__restrict__ pC) {
  constexpr int DH = D + 1, NR = PB * DH, RM = R ? R : 8;
  constexpr int MB = kPcLoads / NR;  // steps of a wave per batch: MB * NR 16-byte loads of the inverse in flight
  extern __shared__ double s_res[];  // the residual chunk, column-major as in memory: cpad * r doubles
  __shared__ double s_P[NR * RM + 1][4 * kPcNW];  // row sums (16 lanes each) of the product columns and of |r|^2
  __shared__ double s_Z[NR * RM + 1], s_R[NR * RM];
  __shared__ double s_red[16];
  const int par = iter & 1;
  const int st_o = ctl->outer_done_stamp, st_t = ctl->tcg_done_stamp, cur = ctl->cur & 1;
  const double c_zr = ctl->z_r[par], c_dPd = ctl->d_Pd[par], c_ePe = ctl->e_Pe[par], c_ePd = ctl->e_Pd[par],
               c_Delta = ctl->Delta, c_ngf = ctl->ngf, c_n0 = ctl->norm_r0;
  const int c_max_inner = ctl->max_inner;
  const int r = R ? R : m.r, k = m.k;
  const int pose0 = blockIdx.x * PB;
  const int npose = min(PB, m.n - pose0);
  const int j0 = pose0 * DH, nrow = npose * DH;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double *__restrict__ rsrc = first ? gradb.p[cur] : res_old;
  // ---- loads first, in the order their values are needed: the <d, H d> partials and the workgroup's own elements,
  //      the first batch of the residual operands, the first batch of the inverse's rows.  None depends on the step
  //      length: their latency overlaps the scalar prologue.
  const int e = threadIdx.x;
  const bool own = e < nrow * r;
  const size_t oown = (size_t)j0 * r + e;
  const int pi1 = (np1 <= 64) ? lane : (int)threadIdx.x;
  // np1 < 0: timing form (time_precond only): <d, H d> is taken from the control block, as it would be if the
  // PRODUCER's last workgroup had summed its partials and stored the scalar -- measured in round 3: it saves nothing
  double myp = (!first && np1 >= 0 && pi1 < np1) ? p1[pi1] : 0.0;
  double o_r = 0, o_h = 0, o_d = 0, o_eta = 0, o_Heta = 0;
  if (own) {
    o_r = rsrc[oown];
    if (!first) {
      o_h = Hd[oown];
      o_d = delta[oown];
      o_eta = eta[oown];
      o_Heta = Heta[oown];
    }
  }
  const int g = threadIdx.x >> 3, tt = threadIdx.x & (GW - 1);
  const bool pact = (g < npose) && (tt < r);
  const size_t o = (size_t)(pose0 + min(g, npose - 1)) * DH * r;
  Row<D> Y;
  ld_row<D>(Xb.p[cur] + o, r, tt, pact, Y);
  const unsigned vec_bytes = (unsigned)((size_t)r * k * sizeof(double));
  const __amdgpu_buffer_rsrc_t rs_r = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(rsrc), 0, vec_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_h =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(first ? rsrc : Hd), 0, vec_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_m = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<double *>(Minv), 0, (unsigned)((size_t)k * ldm * sizeof(double)), 0x00020000);
  const unsigned voff_t = threadIdx.x * 16u, voff_l = (unsigned)lane * 16u;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  double2 xr0[kPcSB], xh0[kPcSB];
#pragma unroll
  for (int u = 0; u < kPcSB; ++u) {
    xr0[u] = pc_ld16(rs_r, voff_t, (unsigned)u * kPcBlock * 16u);
    if (!first) xh0[u] = pc_ld16(rs_h, voff_t, (unsigned)u * kPcBlock * 16u);
  }
  // row q of the workgroup, columns 2 lane, 2 lane + 1 of step (wave + kPcNW * u); rows past the last pose read the
  // rows that follow (or zeros past the end of the matrix) and are never used
  double2 pre[MB][NR];
#pragma unroll
  for (int u = 0; u < MB; ++u) {
#pragma unroll
    for (int q = 0; q < NR; ++q)
      pre[u][q] = pc_ld16(rs_m, voff_l, (unsigned)(((size_t)(j0 + q) * ldm + (size_t)(wave_u + kPcNW * u) * 128) * 8));
  }
  asm volatile("" ::: "memory");
  if (!first)
    for (int i = threadIdx.x + kPcBlock; i < np1; i += kPcBlock) myp += p1[i];
  if (seq > st_o || (!first && seq > st_t)) return;  // finished: no-op (uniform over the grid)
  // The launch in which a tCG run ends (boundary, negative curvature, residual rule, iteration cap -- every workgroup
  // knows: the tests are uniform over the grid) also takes the step: X_trial = Retr_X(eta) for the workgroup's own
  // poses and the partial <eta, grad>, <eta, H eta> of the model decrease, what a launch of k_g_retract did next
  // (pC != null).  Same retraction, same entries; the partials are per workgroup of PB poses instead of 32.
  auto retract_tail = [&]() {
    if (!pC) return;
    __syncthreads();  // (the z part of wave 0 may still be reading s_R)
    double a0 = 0, a1 = 0;
    if (own) {
      const double en = eta[oown], hn = Heta[oown], gr = gradb.p[cur][oown];  // eta, H eta: this thread's own stores
      a0 = en * gr;
      a1 = en * hn;
      const int lc = e / r, t = e - lc * r;
      s_R[lc * RM + t] = en;
    }
    __syncthreads();
    if (wave == 0) {
      Row<D> Yn = Y;
#pragma unroll
      for (int a = 0; a < DH; ++a) Yn.e[a] += 1.0 * (pact ? s_R[(g * DH + a) * RM + tt] : 0.0);
      row_qf<D>(Yn);
      st_row<D>(Xb.p[cur ^ 1] + o, r, tt, pact, Yn);
    }
    const double t0 = block_sum(a0, s_red);
    const double t1 = block_sum(a1, s_red);
    if (threadIdx.x == 0) {
      pC[2 * blockIdx.x] = t0;
      pC[2 * blockIdx.x + 1] = t1;
    }
  };
  // ---- step length / trust-region boundary (ROPTLIB tCG_TR), as in B ----
  double alpha = 0, step = 0;
  bool boundary = false;
  if (!first) {
    const double d_Hd = np1 < 0 ? c_dPd + 1.0 : ((np1 <= 64) ? wave_sum(myp) : block_sum(myp, s_red));
    alpha = tcg_alpha(c_zr, d_Hd);
    const double e_Pe_new = tcg_e_Pe_new(alpha, c_dPd, c_ePe, c_ePd);
    boundary = tcg_boundary(d_Hd, e_Pe_new, c_Delta);
    step = boundary ? tcg_tau(c_dPd, c_ePe, c_ePd, c_Delta) : alpha;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      ctl->alpha = alpha;
      ctl->e_Pe_n = e_Pe_new;
      if (boundary) {
        tcg_end_run(ctl, hf, seq, tcg_boundary_status(d_Hd), iter + 1);
      } else {
        // (the host waits for this word only behind the split form's B: DeviceProblem::RtrForm::replay)
        host_store(&hf->go_seq, seq);
      }
    }
  }
  if (first && blockIdx.x == 0 && threadIdx.x == 0) tcg_begin_run(ctl, c_ngf);
  if (own) {
    const int lc = e / r, t = e - lc * r;
    if (first) {
      eta[oown] = 0;
      Heta[oown] = 0;
      res_new[oown] = o_r;
      s_R[lc * RM + t] = o_r;
    } else {
      eta[oown] = o_eta + step * o_d;
      Heta[oown] = o_Heta + step * o_h;
      if (!boundary) {
        const double rr = fma(alpha, o_h, o_r);
        res_new[oown] = rr;
        s_R[lc * RM + t] = rr;
      }
    }
  }
  if (boundary) {
    retract_tail();
    return;
  }
  // ---- the whole updated residual through LDS, chunk by chunk; product with the workgroup's rows ----
  double acc[NR][RM];
#pragma unroll
  for (int q = 0; q < NR; ++q)
#pragma unroll
    for (int t = 0; t < RM; ++t) acc[q][t] = 0;
  double nrm2 = 0;
  // one batch of staged operands into the LDS image: a straight copy of r_old + alpha H delta
  auto stage = [&](const double2 (&xr)[kPcSB], const double2 (&xh)[kPcSB], int b0, int npair) {
#pragma unroll
    for (int u = 0; u < kPcSB; ++u) {
      const int i = b0 + u * kPcBlock + (int)threadIdx.x;
      if (i < npair) {
        double2 x = xr[u];
        if (!first) {
          x.x = fma(alpha, xh[u].x, x.x);
          x.y = fma(alpha, xh[u].y, x.y);
        }
        nrm2 = fma(x.x, x.x, nrm2);
        nrm2 = fma(x.y, x.y, nrm2);
        reinterpret_cast<double2 *>(s_res)[i] = x;
      }
    }
  };
  // the wave's steps of one batch: a lane's two columns of a step are 2 r contiguous doubles of the image
  auto rows = [&](const double2 (&mm)[MB][NR], int u0, int nstep) {
#pragma unroll
    for (int u = 0; u < MB; ++u) {
      const int sidx = wave_u + kPcNW * (u0 + u);
      if (sidx < nstep) {
        const double *__restrict__ xs = s_res + (size_t)(sidx * 128 + 2 * lane) * r;
        double x0[RM], x1[RM];
#pragma unroll
        for (int t = 0; t < RM; ++t) {
          x0[t] = (R || t < r) ? xs[t] : 0.0;
          x1[t] = (R || t < r) ? xs[r + t] : 0.0;
        }
#pragma unroll
        for (int t = 0; t < RM; ++t)
#pragma unroll
          for (int q = 0; q < NR; ++q) acc[q][t] = fma(x0[t], mm[u][q].x, fma(x1[t], mm[u][q].y, acc[q][t]));
      }
    }
  };
  // One chunk of the residual.  The first chunk consumes the loads requested before the prologue; it is written out
  // as its own instance (FIRST = true) so that those registers are dead in the loop over the remaining chunks.
  auto chunk = [&](int c0, auto first_chunk) {
    constexpr bool FIRST = decltype(first_chunk)::value;
    const int cn = min(chk, k - c0);
    const int cpad = ((cn + 127) / 128) * 128;  // zero-filled up to whole 128-column steps
    const long Nc = (long)cn * r;               // flat (column-major) length of the chunk: contiguous in memory
    const int npair = (int)((Nc + 1) >> 1);     // an odd tail reads its missing half as zero (buffer bounds)
    const unsigned cbase = (unsigned)((size_t)c0 * r * sizeof(double));
    int b0 = 0;
    if constexpr (FIRST) {
      stage(xr0, xh0, 0, npair);
      b0 = kPcSB * kPcBlock;
    } else {
      __syncthreads();
    }
#pragma unroll 1
    for (; b0 < npair; b0 += kPcSB * kPcBlock) {
      double2 xr[kPcSB], xh[kPcSB];
#pragma unroll
      for (int u = 0; u < kPcSB; ++u) {
        xr[u] = pc_ld16(rs_r, voff_t, cbase + (unsigned)(b0 + u * kPcBlock) * 16u);
        if (!first) xh[u] = pc_ld16(rs_h, voff_t, cbase + (unsigned)(b0 + u * kPcBlock) * 16u);
      }
      stage(xr, xh, b0, npair);
    }
    for (long i = 2L * npair + threadIdx.x; i < (long)cpad * r; i += kPcBlock) s_res[i] = 0.0;
    __syncthreads();
    const int nstep = cpad / 128;
    const int nu = (nstep + kPcNW - 1) / kPcNW;  // steps per wave (at most)
    int u0 = 0;
    if constexpr (FIRST) {
      rows(pre, 0, nstep);
      u0 = MB;
    }
#pragma unroll 1
    for (; u0 < nu; u0 += MB) {
      double2 mm[MB][NR];
#pragma unroll
      for (int u = 0; u < MB; ++u) {
#pragma unroll
        for (int q = 0; q < NR; ++q)
          mm[u][q] = pc_ld16(rs_m, voff_l,
                             (unsigned)(((size_t)(j0 + q) * ldm + c0 + (size_t)(wave_u + kPcNW * (u0 + u)) * 128) * 8));
      }
      rows(mm, u0, nstep);
    }
  };
  chunk(0, std::true_type{});
  if constexpr (MULTI) {
#pragma unroll 1
    for (int c0 = chk; c0 < k; c0 += chk) chunk(c0, std::false_type{});
  }
  // ---- sums over the workgroup: every product column and |r|^2.  Four DPP steps give each 16-lane row its sum
  //      (no lane reads, no LDS), one lane per row stores it, NR * RM + 1 threads add the 16 row sums in a fixed order
#pragma unroll
  for (int q = 0; q < NR; ++q)
#pragma unroll
    for (int t = 0; t < RM; ++t) {
      const double v = row16_sum_dpp(acc[q][t]);
      if ((lane & 15) == 0) s_P[q * RM + t][wave * 4 + (lane >> 4)] = v;
    }
  {
    const double v = row16_sum_dpp(nrm2);
    if ((lane & 15) == 0) s_P[NR * RM][wave * 4 + (lane >> 4)] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x <= NR * RM) {
    double v = 0;
#pragma unroll
    for (int w = 0; w < 4 * kPcNW; ++w) v += s_P[threadIdx.x][w];
    s_Z[threadIdx.x] = v;
  }
  __syncthreads();
  // ---- residual stopping rule: every workgroup holds |r|^2 itself (same summation order everywhere) ----
  if (!first) {
    const double nr = sqrt(s_Z[NR * RM]);
    if (tcg_residual_done(nr, c_n0)) {
      if (blockIdx.x == 0 && threadIdx.x == 0) tcg_end_run(ctl, hf, seq, tcg_residual_status(c_n0), iter + 1);
      retract_tail();
      return;
    }
  }
  // ---- z = Proj_X(columns), partial <z, r>: the per-pose lanes all sit in wave 0 (PB <= 4 poses of 8 lanes) ----
  if (wave == 0) {
    Row<D> Zr, Rr;
#pragma unroll
    for (int a = 0; a < DH; ++a) {
      Zr.e[a] = pact ? s_Z[(g * DH + a) * RM + tt] : 0.0;
      Rr.e[a] = pact ? s_R[(g * DH + a) * RM + tt] : 0.0;
    }
    row_tangent<D>(Y, Zr);
    st_row<D>(z + o, r, tt, pact, Zr);
    double zacc = 0;
#pragma unroll
    for (int a = 0; a < DH; ++a) zacc += Zr.e[a] * Rr.e[a];
    const double tot = wave_sum(zacc);
    if (lane == 0) p3[blockIdx.x] = tot;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (!first && iter + 1 >= c_max_inner) tcg_end_run_at_cap(ctl, hf, seq, iter + 1);
    host_store(&hf->last_seq_done, seq);
  }
  if (!first && iter + 1 >= c_max_inner) retract_tail();
}

}  // namespace

bool fused_supported(const ManiDesc &m) {
  // hess / finish leave one partial slot per block in 2 * kMaxPartials-slot buffers
  return m.se && m.r <= GW && m.n > 0 && (m.n + fused_pb(m.r, m.d + 1) - 1) / fused_pb(m.r, m.d + 1) <= 2 * kMaxPartials;
}
int fused_pose_blocks(const ManiDesc &m) {
  const int pb = fused_pb(m.r, m.d + 1);
  return (m.n + pb - 1) / pb;
}
int fused_nsplit(const ManiDesc &m) {
  const int njc = (m.k + kJChunk - 1) / kJChunk;
  const int aim = 512, cap = 32;
  int ns = (aim + njc - 1) / njc;  // aim for ~512 blocks of 4 waves
  if (ns < 1) ns = 1;
  if (ns > cap) ns = cap;
  while (ns > 1 && (m.k + ns - 1) / ns < 16) --ns;
  return ns;
}
int fused_precond_grid(const ManiDesc &m) { return ((m.k + kJChunk - 1) / kJChunk) * fused_nsplit(m); }
int fused_update_grid(const ManiDesc &m) {
  const long blocks = ((long)m.r * m.k + kBlock - 1) / kBlock;
  return (int)(blocks < 1024 ? blocks : 1024);
}

int launch_fused_hess(hipStream_t st, const TcgOperands &o, int seq, int iter, int np3) {
  count_launch();
  const ManiDesc &m = o.m;
  const int par = iter & 1;
  if (o.has_bsr) {  // block structure available: 32 poses per workgroup
    const int gridb = (m.n + kPosesPerBlock - 1) / kPosesPerBlock;
    DCORA_LAUNCH_D(k_fused_hess_bsr, m.d, gridb, st, m, o.Qb, o.z, o.d[par ^ 1], o.d[par], o.X, o.S, o.Hd, o.p3, np3,
                   o.p1, o.ctl, seq, iter);
    return gridb;
  }
  const int grid = fused_pose_blocks(m);
  DCORA_LAUNCH_D(k_fused_hess, m.d, grid, st, m, o.Q, o.z, o.d[par ^ 1], o.d[par], o.X, o.S, o.Hd, o.p3, np3, o.p1,
                 o.ctl, seq, iter);
  return grid;
}
// What B (and B + C) read and write in iteration `iter`; the launch that opens a run (first) takes the gradient as its
// residual and steps nowhere.
namespace {
struct StepVectors {
  const double *delta, *Hd, *res_old, *p1;
  int np1;
  double *res_new;
};
StepVectors step_vectors(const TcgOperands &o, int iter, int first, int np1) {
  if (first) return StepVectors{nullptr, nullptr, nullptr, nullptr, 0, o.res_new(iter, first)};
  return StepVectors{o.d[iter & 1], o.Hd, o.r[iter & 1], o.p1, np1, o.res_new(iter, first)};
}
}  // namespace
void launch_fused_precond(hipStream_t st, const TcgOperands &o, int seq, int iter, int first, int np1) {
  const ManiDesc &m = o.m;
  const StepVectors v = step_vectors(o, iter, first, np1);
  const int grid = o.Minv ? fused_precond_grid(m) : fused_update_grid(m);
  const int ns = o.Minv ? fused_nsplit(m) : 1;
#define DCORA_LAUNCH_PRECOND(RM, HM)                                                                                 \
  hipLaunchKernelGGL((k_fused_precond<RM, HM>), dim3(grid), dim3(kBlock), 0, st, m.r, m.k, o.ldm, ns, o.Minv, o.grad, \
                     v.delta, v.Hd, o.eta, o.Heta, v.res_old, v.res_new, o.Zpart, v.p1, v.np1, o.p2, o.ctl, o.hf, seq, \
                     iter, first, o.sf)
  if (m.r <= 4) {
    if (o.Minv) DCORA_LAUNCH_PRECOND(4, true); else DCORA_LAUNCH_PRECOND(4, false);
  } else {
    if (o.Minv) DCORA_LAUNCH_PRECOND(8, true); else DCORA_LAUNCH_PRECOND(8, false);
  }
#undef DCORA_LAUNCH_PRECOND
}
int fused_pc_blocks(const ManiDesc &m) {
  const int pb = fused_pc_pb(m);
  return (m.n + pb - 1) / pb;
}
// where the one-launch form wins (measured on MI355X, sphere2500 blocks): the whole residual in one LDS chunk and one
// staging batch, r <= 7 -- k = 2000: 11.0 us against 11.3 + 5.1 us for B + C at r = 5, 13.4 / 17.6 at r = 6, 18.0 /
// 18.6 at r = 7; beyond (k = 3332: 29.2 / 29.2, k = 5000: 76 / 48, r = 8: 21.0 / 20.0) the split form stays
bool fused_pc_preferred(const ManiDesc &m, int ldm) {
  return m.k <= pc_chunk(m, ldm) && (long)m.r * m.k <= 2L * kPcSB * kPcBlock && m.r <= 7;
}
// -1 = this device refuses the attribute or the launch; use_pc() asks with prepare_only (fused_pc_ready) before
// choosing the one-launch form.
template <int D, int PB, int R, bool MULTI>
static int pc_launch(hipStream_t st, const TcgOperands &o, int seq, int iter, int first, int np1, bool retract,
                     bool prepare_only) {
  static LdsGrant grant;
  const ManiDesc &m = o.m;
  const int chk = pc_chunk(m, o.ldm);
  const size_t lds = (size_t)chk * m.r * sizeof(double);
  if (!grant.granted(reinterpret_cast<const void *>(&k_fused_pc<D, PB, R, MULTI>), lds, 64 * 1024)) return -1;
  const int grid = (m.n + PB - 1) / PB;
  if (prepare_only) return grid;
  const StepVectors v = step_vectors(o, iter, first, np1);
  hipLaunchKernelGGL((k_fused_pc<D, PB, R, MULTI>), dim3(grid), dim3(kPcBlock), lds, st, m, o.ldm, chk, o.Minv, o.grad,
                     o.X, v.delta, v.Hd, o.eta, o.Heta, v.res_old, v.res_new, o.z, v.p1, v.np1, o.p3, o.ctl, o.hf, seq,
                     iter, first, retract ? o.pC : nullptr);
  if (hipGetLastError() != hipSuccess) return -1;
  return grid;
}
static int fused_pc_dispatch(hipStream_t st, const TcgOperands &o, int seq, int iter, int first, int np1, bool retract,
                             bool prepare_only) {
  const ManiDesc &m = o.m;
#define DCORA_PC(D_, PB_, R_, MULTI_) \
  return pc_launch<D_, PB_, R_, MULTI_>(st, o, seq, iter, first, np1, retract, prepare_only)
#define DCORA_PC_R(PB_, MULTI_) /* d = 3: r = 3 .. 7 fixed at compile time, else read at run time */ \
  do {                                                                                                \
    if (m.r == 3) DCORA_PC(3, PB_, 3, MULTI_);                                                        \
    if (m.r == 4) DCORA_PC(3, PB_, 4, MULTI_);                                                        \
    if (m.r == 5) DCORA_PC(3, PB_, 5, MULTI_);                                                        \
    if (m.r == 6) DCORA_PC(3, PB_, 6, MULTI_);                                                        \
    if (m.r == 7) DCORA_PC(3, PB_, 7, MULTI_);                                                        \
    DCORA_PC(3, PB_, 0, MULTI_);                                                                      \
  } while (0)
  const int pb = fused_pc_pb(m);
  const bool multi = m.k > pc_chunk(m, o.ldm);
  if (m.d == 3) {
    if (pb == 2 && !multi) DCORA_PC_R(2, false);
    if (pb == 2) DCORA_PC_R(2, true);
    // four poses per thread with r only known at run time does not fit the register file (208 B/lane of scratch when
    // it was instantiated), and neither does r = 7 (128 B/lane): r >= 7 beyond 768 poses takes the three-launch form,
    // which fused_pc_preferred() chooses there anyway
    if (m.r == 3) DCORA_PC(3, 4, 3, true);
    if (m.r == 4) DCORA_PC(3, 4, 4, true);
    if (m.r == 5) DCORA_PC(3, 4, 5, true);
    if (m.r == 6) DCORA_PC(3, 4, 6, true);
    return -1;
  }
  if (pb == 2 && !multi) DCORA_PC(2, 2, 0, false);
  if (pb == 2) DCORA_PC(2, 2, 0, true);
  DCORA_PC(2, 4, 0, true);
#undef DCORA_PC_R
#undef DCORA_PC
}
int launch_fused_pc(hipStream_t st, const TcgOperands &o, int seq, int iter, int first, int np1, bool retract) {
  count_launch();
  return fused_pc_dispatch(st, o, seq, iter, first, np1, retract, false);
}
bool fused_pc_ready(const ManiDesc &m, int ldm) {
  TcgOperands none;
  none.m = m;
  none.ldm = ldm;
  return fused_pc_dispatch(nullptr, none, 0, 0, 0, 0, false, true) >= 0;
}
void launch_fused_finish(hipStream_t st, const TcgOperands &o, int seq, int iter, int first, int np2, FinishZ zsrc) {
  const ManiDesc &m = o.m;
  const int grid = fused_pose_blocks(m);
  const int ns = o.Minv ? fused_nsplit(m) : 1;
  const bool raw = zsrc == FinishZ::from_raw;
  DCORA_LAUNCH_D(k_fused_finish, m.d, grid, st, m, ns, o.X, raw ? o.W : o.Zpart, o.res_new(iter, first), o.z,
                 first ? nullptr : o.p2, first ? 0 : np2, o.p3, o.ctl, o.hf, seq, iter, first, raw ? SpFold{} : o.sf,
                 zsrc == FinishZ::keep_raw ? o.W : nullptr);
}

}  // namespace dcora
