// Evaluations of the SE layout: cost and gradient in one launch on the CSR rows (k_fused_grad) or on the block
// structure of Q (k_spmm_bsrq, which is also the block Q-apply), the evaluation epilogue of an RBCD pass
// (k_eval_partial, k_eval_finish) and the start-of-solve control block (k_ctl_init).
#include <algorithm>
#include <cstddef>
#include <stdexcept>

#include "csr_rows.h"
#include "tcg_rules.h"
#include "pose_group.h"

namespace dcora {

namespace {

// ------------------------------------------------------------------------------------------------------
// Cost and gradient of an RTR evaluation in ONE launch (small pose-graph blocks, CSR): EG = X Q + G with the partial
// dots {<X Q, X>, <X, G>} (what k_spmm<true> does), then RG = Proj_X(EG), S_i = sym(Y_i^T EG_i) and the partial |RG|^2
// (what k_g_rgrad does) -- phase 1 one thread per output element with the block's CSR rows staged in LDS, phase 2
// eight lanes per pose, operands handed over through LDS, exactly as k_fused_hess.  Saves one dependent launch per
// evaluation (4 per local solve, 1 per central evaluation).
// ------------------------------------------------------------------------------------------------------
// RIDE (GradRide, kernels.h): the start-point evaluation forms G from the agent's coupling block first -- every thread
// for its own element (coupling_row, csr_rows.h), nothing another workgroup of the launch writes is read.
//
// The loads ahead of the sums are three memory round trips (they were ten to twelve waits in a row: gate words one by
// one, cur, row pointers, own element, tile, and the gather eight entries at a time, every index read predicated):
//   1. the gate words, cur and the row pointers of Q, requested as one straight-line batch before the gate is looked
//      at -- all of it memory that is valid whether or not the gate closes; a gated-off launch still writes nothing;
//   2. the ci / v tile first, behind it the thread's own element of X and of G;
//   3. the gather of a row in one batch of kGradGB entries (k_tcg_run's kRunGB) with the weights read from LDS where
//      they are used; chunks of 8 only for what a row holds beyond it.
// Only when a load is issued differs from the plain form: every sum keeps its operands, order and expression.
// What the form costs and assumes: every thread issues the kGradGB gathers of a tile pass, also one without entries in
// the pass (a zero weight on a column of the tile: finite X assumed, as the padding of a batch always did), and it
// holds 142 registers -- right for this kernel's one workgroup per 12-16 poses, a wave per SIMD; a row block that had
// to share a CU with others would want the narrower batch back.  tile_request reads Q.ci / Q.v at a clamped index
// whatever the block holds: Q has entries (DeviceProblem runs the fused kernels on nnz > 0 only).
// RIDE keeps coupling_row's own chain (row pointers -> indices -> gather) behind trip 2's requests: its loads riding
// in trips 1-3 were built and did not pay in the trace (profiles/eval_chains.txt, section 4).
constexpr int kGradGB = 24;
template <int D, bool RIDE>
__global__ __launch_bounds__(kBlock) void k_fused_grad(ManiDesc m, CsrDev Q, Buf2 Xb, const double *__restrict__ G,
                                                       Buf2 EGb, Buf2 RGb, Buf2 Sb, int sel,
                                                       double *__restrict__ pA, double *__restrict__ pB,
                                                       double *__restrict__ posenorm, Gate g, GradRide ride) {
  __shared__ int s_ci[kHessTile];
  __shared__ double s_v[kHessTile];
  __shared__ double s_W[kBlock], s_X[kBlock];
  __shared__ double s_red[16];
  constexpr int DH = D + 1;
  constexpr int SU = kHessTile / kBlock;
  const int r = m.r;
  const int PB = fused_pb(r, DH);
  const int pose0 = blockIdx.x * PB;
  const int npose = min(PB, m.n - pose0);
  const int j0 = pose0 * DH, ncol = npose * DH, nout = ncol * r;
  const int e = threadIdx.x;
  const bool act = e < nout;
  const int lc = e / r, t = e - lc * r;
  const int j = j0 + lc;
  // ---- trip 1 (the empty asm keeps the loads from sinking behind the early return).  Straight-line code, so that it
  // is issued as one batch: a clamped row instead of a predicated load, and without a control block (the central
  // evaluation) the three control words are read from Q.rp, which is there, and replaced ----
  const bool has_ctl = g.ctl != nullptr;
  const char *cb = has_ctl ? reinterpret_cast<const char *>(g.ctl) : reinterpret_cast<const char *>(Q.rp);
  auto ctl_word = [&](size_t off) { return *reinterpret_cast<const int *>(cb + (has_ctl ? off : 0)); };
  const int w_outer = ctl_word(offsetof(SolverCtl, outer_done_stamp));
  const int w_tcg = ctl_word(offsetof(SolverCtl, tcg_done_stamp));
  const int w_cur = ctl_word(offsetof(SolverCtl, cur));
  const int jc = act ? j : j0;
  const int pbeg = Q.rp[j0], pend = Q.rp[j0 + ncol];
  const int rb = Q.rp[jc], re = Q.rp[jc + 1];
  asm volatile("" ::"s"(w_outer), "s"(w_tcg), "s"(w_cur), "s"(pbeg), "s"(pend), "v"(rb), "v"(re));
  const GateWords gw{has_ctl ? w_outer : 0x7fffffff, has_ctl ? w_tcg : 0x7fffffff};
  const int cur = has_ctl ? w_cur : 0;
  const int myb = act ? rb : 0, mye = act ? re : 0;
  if (gated(gw, g.ctl, g.seq, g.gate)) return;
  // (a select between the two pointers of a pair, both kernel arguments: indexing the pair with idx is one more load)
  const bool idx = g.ctl && ((cur ^ sel) & 1);
  const double *__restrict__ X = idx ? Xb.p[1] : Xb.p[0];
  double *__restrict__ EG = idx ? EGb.p[1] : EGb.p[0];
  double *__restrict__ RG = idx ? RGb.p[1] : RGb.p[0];
  double *__restrict__ Sblk = idx ? Sb.p[1] : Sb.p[0];
  // ---- trip 2: the first tile, then the thread's own element of X and of G ----
  int ci_r[SU];
  double v_r[SU];
  const int last = max(pend - 1, 0);
  auto tile_request = [&](int base) {
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const int i = min(base + (int)threadIdx.x + u * kBlock, last);
      ci_r[u] = Q.ci[i];
      v_r[u] = Q.v[i];
    }
  };
  tile_request(pbeg);
  const size_t oown = (size_t)j * r + t;
  const double x_ld = X[(size_t)jc * r + (act ? t : 0)];
  const double x_own = act ? x_ld : 0.0;
  double g_own = 0.0;
  if (RIDE) {  // (its own chain of row pointers, indices and gathers, with the tile in flight)
    if (act) {
      g_own = coupling_row(ride, r, j, t);
      ride.G_out[oown] = g_own;
    }
  } else {
    g_own = (act && G) ? G[oown] : 0.0;
  }
  // ---- phase 1: EG = X Q + G ----
  double acc = 0;
  for (int base = pbeg; base < pend; base += kHessTile) {
    const int cnt = min(kHessTile, pend - base);
    if (base != pbeg) {
      __syncthreads();
      tile_request(base);
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
    const int lo = max(myb, base) - base, hi = min(mye, base + cnt) - base;
    // ---- trip 3: the first kGradGB entries of the row in one batch ----
    // (the index reads are clamped, not predicated -- a batch's padding gathers the row's last column again, or the
    // tile's first, under a zero weight: one wait for all the index reads instead of one LDS round trip each)
    double bg[kGradGB];
#pragma unroll
    for (int q = 0; q < kGradGB; ++q) bg[q] = X[(size_t)s_ci[max(min(lo + q, hi - 1), 0)] * r + t];
    __builtin_amdgcn_sched_barrier(0);  // (every request of the trip before the first sum)
#pragma unroll
    for (int q = 0; q < kGradGB; ++q) {
      const double wq = s_v[max(min(lo + q, hi - 1), 0)];  // (the weights come from LDS when they are used)
      acc += ((lo + q < hi) ? wq : 0.0) * bg[q];
    }
    for (int p = lo + kGradGB; p < hi; p += 8) {
      double b8[8], w8[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int pq = min(p + q, hi - 1);
        w8[q] = (p + q < hi) ? s_v[pq] : 0.0;
        b8[q] = X[(size_t)s_ci[pq] * r + t];
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) acc += w8[q] * b8[q];
    }
  }
  double d0 = 0, d1 = 0;
  if (act) {
    const double eg = acc + g_own;
    EG[oown] = eg;
    s_W[e] = eg;
    s_X[e] = x_own;
    d0 = acc * x_own;
    d1 = x_own * g_own;
  }
  __syncthreads();
  // ---- phase 2: RG = Proj_X(EG), S_i = sym(Y_i^T EG_i) ----
  const int gp = threadIdx.x >> 3, tt = threadIdx.x & (GW - 1);
  const bool pact = (gp < npose) && (tt < r);
  const int pose = pose0 + gp;
  const size_t o = (size_t)pose * DH * r;
  Row<D> Y, E;
#pragma unroll
  for (int a = 0; a < DH; ++a) {
    E.e[a] = pact ? s_W[(gp * DH + a) * r + tt] : 0.0;
    Y.e[a] = pact ? s_X[(gp * DH + a) * r + tt] : 0.0;
  }
  double S[D][D];
  grp_sym_gram<D>(Y, E, S);
  if (Sblk && gp < npose && tt == 0)
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < D; ++b) Sblk[(size_t)pose * D * D + a + b * D] = S[a][b];
  row_sub_AS<D>(E, Y, S);
  double pa = 0;
#pragma unroll
  for (int a = 0; a < DH; ++a) pa += E.e[a] * E.e[a];
  if (posenorm) {
    const double ps = grp_sum(pa);
    if (gp < npose && tt == 0) posenorm[pose] = ps;
  }
  st_row<D>(RG + o, r, tt, pact, E);
  const double t0 = block_sum(d0, s_red);
  const double t1 = block_sum(d1, s_red);
  const double t2 = block_sum(pact ? pa : 0.0, s_red);
  if (threadIdx.x == 0) {
    pA[2 * blockIdx.x] = t0;
    pA[2 * blockIdx.x + 1] = t1;
    pB[blockIdx.x] = t2;
  }
}

// ------------------------------------------------------------------------------------------------------
// Q-apply on the block structure of the connection Laplacian: Y = X Q (+ G), Q in BSR with (d+1)^2 blocks stored
// column-major.  History of the forms (all measured on the 100k lattice, r = 5, warm / cold us): LDS-staged blocks with 8
// lanes per pose 27.4 / 33.9; the LDS-free 8-lanes-per-pose form (lane t = row t of the pose's block, four 8-byte gathers
// and two 16-byte block loads per lane and block, the block's other rows by DPP quad broadcasts) 24.6 / 33.2 -- rounds
// 2-4, unmoved by gather depth, software pipelining, non-temporal accesses, a symmetric store of the blocks, r lanes
// per pose, 16-byte gathers of row pairs, a per-pose header, locality orderings and XCD-aware grids: it was bound by
// the NUMBER of gather instructions (each serves 8 poses).  Round 5: the quad-per-pose form below, 22.6 / 27.5.
// ------------------------------------------------------------------------------------------------------
template <int A_>
__device__ __forceinline__ double quad_bcast(double v) {
  return dpp_move<A_ * 0x55>(v);  // quad_perm [A, A, A, A]
}
// GRAD: the whole evaluation of an RTR iteration in this launch -- a lane group already holds EG_i = (X Q + G)_i in the
// layout k_g_rgrad works in, so RG_i = Proj_X(EG_i), S_i = sym(Y_i^T EG_i), the partial |RG|^2 and the per-pose norms
// follow as an epilogue (the same operations in the same order as k_g_rgrad) instead of a launch of their own that
// reads EG and X back: one dependent launch less per evaluation, four per local solve of a large block.
struct BsrGradOut {
  Buf2 RG, S;
  double *pB = nullptr;        // partial |RG|^2, one per workgroup
  double *posenorm = nullptr;  // |RG_i|^2 per pose, or null
  // central evaluation of an RBCD pass: the workgroups are dealt to the agents (wg_per_agent each, a slice of the
  // agent's poses per workgroup), so pB holds every agent's |rgrad_b|^2 in wg_per_agent consecutive slots and the
  // epilogue kernel adds those -- no per-pose norms, no launch that sums them per agent
  const int *agent_start = nullptr;
  int wg_per_agent = 0;
};
// ------------------------------------------------------------------------------------------------------
// The block Q-apply (round 5): FOUR lanes per pose, lane c owns COLUMN c of the pose's r x (d+1) block.
// A column is r contiguous doubles, so the neighbour's block arrives by ceil(r / 2) 16-byte loads per lane (8-byte
// aligned; r = 5: 16 + 16 + 8 bytes) in instructions that serve 16 poses each, and the d + 1 weights lane c needs --
// column c of the (d+1)^2 block, stored column-major -- are one contiguous run (two 16-byte loads, no duplicate loads by
// a second quad, no DPP broadcast in the inner loop): 5 load instructions per 16 (pose, block) pairs where the
// 8-lanes-per-pose form issues 6 per 8, and no idle lanes at r = 5.  Lane c accumulates ITS column's contribution to
// all d + 1 output columns (r (d+1) sums in registers); the four partials of a pose meet once per pose in a quad
// reduce-scatter (lane a ends with output column a), then G, the dots and the store run on contiguous columns again.
// GRAD: the whole evaluation of an RTR iteration as the epilogue (E and Y columns handed round the quad by DPP).
// ------------------------------------------------------------------------------------------------------
typedef double q_v2f64u __attribute__((ext_vector_type(2), aligned(8)));
template <int N>
__device__ __forceinline__ void ld_run(const double *__restrict__ p, bool ok, double (&x)[N]) {
#pragma unroll
  for (int i = 0; i + 1 < N; i += 2) {
    q_v2f64u v = {0.0, 0.0};
    if (ok) v = *reinterpret_cast<const q_v2f64u *>(p + i);
    x[i] = v.x;
    x[i + 1] = v.y;
  }
  if (N & 1) x[N - 1] = ok ? p[N - 1] : 0.0;
}
template <int N>
__device__ __forceinline__ void st_run(double *__restrict__ p, bool ok, const double (&x)[N]) {
  if (!ok) return;
#pragma unroll
  for (int i = 0; i + 1 < N; i += 2) {
    q_v2f64u v = {x[i], x[i + 1]};
    *reinterpret_cast<q_v2f64u *>(p + i) = v;
  }
  if (N & 1) p[N - 1] = x[N - 1];
}
template <int A_>
__device__ __forceinline__ int quad_bcast_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, A_ * 0x55, 0xF, 0xF, true);
}
__device__ __forceinline__ double quad_sum(double v) {
  asm volatile("" : "+v"(v));
  v += dpp_move<0xB1>(v);  // quad_perm [1,0,3,2]
  asm volatile("" : "+v"(v));
  v += dpp_move<0x4E>(v);  // quad_perm [2,3,0,1]
  return v;
}
// Measured on the 100k lattice at r = 5, warm / cold us (gfx950, round 5): this form 22.6 / 27.5; its loads requested two
// or one (pose, block) pair at a time instead of four 22.6-22.8 / 27.6; 256-thread workgroups 22.7 / 28.3; the pose's
// own column of X and of G requested before the block loop (136 registers, 3 waves per SIMD) 23.6 / 27.6; half as many
// workgroups of two passes each 25.1 / 30.1; forced to 5 or 6 waves per SIMD (176 / 320 bytes of scratch per lane)
// 72 / 128 us.  The 8-lanes-per-pose form it replaces: 24.6 / 33.2.
constexpr int kQBlock = 128;  // threads per workgroup: 32 poses, as the 8-lanes-per-pose kernels' workgroups hold
template <int D, int R, bool DOTS, bool GRAD>
__global__ __launch_bounds__(kQBlock) void k_spmm_bsrq(BsrDev A, Buf2 Xb, int selX, const double *__restrict__ G, Buf2 Yb,
                                                       int selY, double *__restrict__ partials, Gate g, BsrGradOut go) {
  if (gated(g.ctl, g.seq, g.gate)) return;
  constexpr int DH = D + 1, BS = DH * DH, PW = kQBlock / 4;
  // (pose, block) pairs whose loads a lane requests together: the four column indices of one index load, two at a time
  // at r >= 7 where four columns of the neighbours alone are 56-64 registers
  constexpr int kQGather = R >= 7 ? 2 : 4;
  __shared__ double s_red[16];
  const int cur = g.ctl ? (g.ctl->cur & 1) : 0;
  const double *__restrict__ X = Xb.p[g.ctl ? ((cur ^ selX) & 1) : 0];
  double *__restrict__ Y = Yb.p[g.ctl ? ((cur ^ selY) & 1) : 0];
  double *__restrict__ RG = GRAD ? go.RG.p[g.ctl ? ((cur ^ selY) & 1) : 0] : nullptr;
  double *__restrict__ Sblk = GRAD ? go.S.p[g.ctl ? ((cur ^ selY) & 1) : 0] : nullptr;
  const int c = threadIdx.x & 3;
  const bool lane_on = c < DH;  // d = 2: the fourth lane of a quad carries zeros
  const int cc = lane_on ? c : 0;
  const bool odd = (c & 1) != 0, upper = (c & 2) != 0;
  double d0 = 0, d1 = 0, dg = 0;
  int range_lo = (int)((long)A.nbrows * blockIdx.x / gridDim.x);
  int range_hi = (int)((long)A.nbrows * (blockIdx.x + 1) / gridDim.x);
  if (GRAD && go.agent_start) {
    const int a = blockIdx.x / go.wg_per_agent, sl = blockIdx.x - a * go.wg_per_agent;
    const int lo = go.agent_start[a], hi = go.agent_start[a + 1];
    range_lo = lo + (int)((long)(hi - lo) * sl / go.wg_per_agent);
    range_hi = lo + (int)((long)(hi - lo) * (sl + 1) / go.wg_per_agent);
  }
  const int npass = max(1, (range_hi - range_lo + PW - 1) / PW);
  const int per_pass = (range_hi - range_lo + npass - 1) / npass;
  for (int pose0 = range_lo; pose0 < range_hi; pose0 += per_pass) {
    const int pend_pose = min(range_hi, pose0 + per_pass);
    const int pose = pose0 + (threadIdx.x >> 2);
    const bool inr = pose < pend_pose;
    const bool active = inr && lane_on;
    const int myb = inr ? A.bp[pose] : 0, mye = inr ? A.bp[pose + 1] : 0;
    double acc[4][R];  // acc[a][.]: this lane's (column c's) part of output column a
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int i = 0; i < R; ++i) acc[a][i] = 0.0;
    for (int b0 = myb; b0 < mye; b0 += 4) {
      const int nb = min(4, mye - b0);
      const int mybc = (c < nb) ? A.bc[b0 + c] : 0;
#pragma unroll
      for (int h = 0; h < 4; h += kQGather) {
        double x[kQGather][R], w[kQGather][DH];
#pragma unroll
        for (int q = 0; q < kQGather; ++q) {
          const bool ok = active && (h + q < nb);
          const int col = (h + q == 0) ? quad_bcast_i<0>(mybc) : (h + q == 1) ? quad_bcast_i<1>(mybc)
                        : (h + q == 2) ? quad_bcast_i<2>(mybc) : quad_bcast_i<3>(mybc);
          ld_run<R>(X + ((size_t)col * DH + cc) * R, ok, x[q]);
          ld_run<DH>(A.bv + (size_t)(b0 + h + q) * BS + cc * DH, ok, w[q]);
        }
#pragma unroll
        for (int q = 0; q < kQGather; ++q)
#pragma unroll
          for (int a = 0; a < DH; ++a)
#pragma unroll
            for (int i = 0; i < R; ++i) acc[a][i] += w[q][a] * x[q][i];
        if (kQGather < 4) __builtin_amdgcn_sched_barrier(0);  // the next pair's loads stay behind this pair's sums
      }
    }
    // quad reduce-scatter: lane a ends with output column a = the sum of the four lanes' acc[a][.]
    double e[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      // pairs {0,1}, {2,3}: a lane keeps the column of its own parity and sends the other to its partner
      const double keep0 = odd ? acc[1][i] : acc[0][i], send0 = odd ? acc[0][i] : acc[1][i];
      const double keep1 = odd ? acc[3][i] : acc[2][i], send1 = odd ? acc[2][i] : acc[3][i];
      const double t0 = keep0 + dpp_move<0xB1>(send0);  // columns (c & 1) over lanes c, c ^ 1
      const double t1 = keep1 + dpp_move<0xB1>(send1);  // columns 2 + (c & 1)
      const double keep = upper ? t1 : t0, send = upper ? t0 : t1;
      e[i] = keep + dpp_move<0x4E>(send);
    }
    const size_t oc = ((size_t)(inr ? pose : 0) * DH + cc) * R;
    double xo[R], gg[R];
    if (DOTS || GRAD) ld_run<R>(X + oc, active, xo);
    ld_run<R>(G + oc, active && G != nullptr, gg);
    if (DOTS || GRAD) {
#pragma unroll
      for (int i = 0; i < R; ++i) {
        d0 += e[i] * xo[i];
        d1 += xo[i] * gg[i];
      }
    }
#pragma unroll
    for (int i = 0; i < R; ++i) e[i] = active ? e[i] + gg[i] : 0.0;
    if (Y) st_run<R>(Y + oc, active, e);
    if (GRAD) {
      // columns of Y (= X_i) and E handed round the quad; every lane forms S = sym(Y^T E) over the rotation columns
      double Yc[D][R], Ec[D][R];
#pragma unroll
      for (int i = 0; i < R; ++i) {
        Yc[0][i] = quad_bcast<0>(xo[i]);
        Ec[0][i] = quad_bcast<0>(e[i]);
        Yc[1][i] = quad_bcast<1>(xo[i]);
        Ec[1][i] = quad_bcast<1>(e[i]);
        if (D == 3) {
          Yc[D - 1][i] = quad_bcast<2>(xo[i]);
          Ec[D - 1][i] = quad_bcast<2>(e[i]);
        }
      }
      double S[D][D];
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = a; b < D; ++b) {
          double s = 0;
#pragma unroll
          for (int i = 0; i < R; ++i) s += 0.5 * (Yc[a][i] * Ec[b][i] + Yc[b][i] * Ec[a][i]);
          S[a][b] = s;
          S[b][a] = s;
        }
      if (Sblk && inr && c < D) {  // lane b stores column b of the D x D block
#pragma unroll
        for (int a = 0; a < D; ++a) {
          const double s = (c == 0) ? S[a][0] : (c == 1) ? S[a][1] : S[a][D - 1];
          Sblk[(size_t)pose * D * D + a + c * D] = s;
        }
      }
      // RG column b = E column b - sum_a Y column a S[a][b] (rotation columns; the translation column stays)
      if (c < D) {
#pragma unroll
        for (int i = 0; i < R; ++i) {
          double s = 0;
#pragma unroll
          for (int a = 0; a < D; ++a) s += Yc[a][i] * ((c == 0) ? S[a][0] : (c == 1) ? S[a][1] : S[a][D - 1]);
          e[i] -= s;
        }
      }
      double pa = 0;
#pragma unroll
      for (int i = 0; i < R; ++i) pa += e[i] * e[i];
      if (!active) pa = 0;
      dg += pa;
      if (go.posenorm) {
        const double ps = quad_sum(pa);
        if (inr && c == 0) go.posenorm[pose] = ps;
      }
      if (RG) st_run<R>(RG + oc, active, e);
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
  if (GRAD) {
    const double cs = block_sum(dg, s_red);
    if (threadIdx.x == 0) go.pB[blockIdx.x] = cs;
  }
}

// (Measured and dropped, round 3: a third form with HALF the load instructions -- lanes as (column pair, row pair) of a
// pose, two 16-byte gathers and one 16-byte block load per lane and block instead of six loads -- was slower everywhere,
// also at even r where every gather is 16-byte aligned: r = 5 28.6 / 36.7 us warm / cold against 24.6 / 33.1.  Round 4:
// a locality ordering of the poses (sub-cubes of the lattice, 4x4x2 .. 2x2x8, instead of the trajectory order) changed
// nothing: 24.0-24.3 / 32.8-33.3 against 24.0 / 32.6, tools/qapply_order.py.  The Q-apply is bound by the dependent
// chain (row pointer -> column indices -> gather) at the head of its ~3000 short-lived workgroups.)

}  // namespace

// start-of-solve control block, written on the device so that a solve needs no host-to-device copy
__global__ void k_ctl_init(SolverCtl *c, double tol, double Delta, double maxDelta, int max_outer, int stop_on_accept,
                           int max_inner) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  c->f1 = c->ngf = c->fInit = c->gradNormInit = 0;
  CtlInit ci;
  ci.tol = tol;
  ci.Delta = Delta;
  ci.maxDelta = maxDelta;
  ci.max_outer = max_outer;
  ci.stop_on_accept = stop_on_accept;
  ci.max_inner = max_inner;
  ctl_arm(c, ci);
}
void launch_ctl_init(hipStream_t st, SolverCtl *c, double tol, double Delta, double maxDelta, int max_outer,
                     int stop_on_accept, int max_inner) {
  hipLaunchKernelGGL(k_ctl_init, dim3(1), dim3(64), 0, st, c, tol, Delta, maxDelta, max_outer, stop_on_accept,
                     max_inner);
}

// Evaluation epilogue of one RBCD pass (ref examples/MultiRobotExample.cpp:264-305): per-agent |rgrad_b| from the
// per-pose squared norms, 2 f from the Q-apply partials, greedy argmax; results go to host-mapped memory and are
// published by a sequence word, so the host never calls into the runtime to read them.
// Large graphs (100k poses: one workgroup walked 12 500 norms per agent in 24 dependent steps, 27 us per RBCD
// iteration): the per-agent sums are split over kEvalSplit workgroups per agent first, fixed slices, fixed order.
constexpr int kEvalSplit = 32;
__global__ __launch_bounds__(kBlock) void k_eval_partial(const int *__restrict__ pose_start,
                                                         const double *__restrict__ posenorm,
                                                         double *__restrict__ part) {
  __shared__ double s_red[16];
  const int b = blockIdx.x / kEvalSplit, sl = blockIdx.x - b * kEvalSplit;
  const int lo = pose_start[b], hi = pose_start[b + 1];
  const int per = (hi - lo + kEvalSplit - 1) / kEvalSplit;
  const int i0 = lo + sl * per, i1 = min(hi, i0 + per);
  double v = 0;
  for (int i = i0 + (int)threadIdx.x; i < i1; i += kBlock) v += posenorm[i];
  v = block_sum(v, s_red);
  if (threadIdx.x == 0) part[blockIdx.x] = v;
}
__global__ __launch_bounds__(kBlock) void k_eval_finish(int R, const int *__restrict__ pose_start,
                                                        const double *__restrict__ posenorm,
                                                        const double *__restrict__ pA, int npA, EvalOut *out,
                                                        int seq, const double *__restrict__ part,
                                                        const double *__restrict__ agent_partials, int wpa) {
  __shared__ double s_red[16];
  __shared__ double s_bn[kMaxAgents];
  // the cost partials first (loads in flight under the per-agent sums below)
  double q0 = ((int)threadIdx.x < npA) ? pA[2 * threadIdx.x] : 0.0;
  double q1 = ((int)threadIdx.x < npA) ? pA[2 * threadIdx.x + 1] : 0.0;
  if (agent_partials) {  // wpa consecutive partials per agent, written by the evaluation itself (BsrGradOut): one wave
                         // per agent, eight loads in flight per lane, fixed order
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = kBlock / 64;
    for (int b = w; b < R; b += nw) {
      const int lo = b * wpa, hi = lo + wpa;
      double v = 0;
      for (int i0 = lo + lane; i0 < hi; i0 += 64 * 8) {
        double t8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t8[u] = agent_partials[min(i0 + 64 * u, hi - 1)];
#pragma unroll
        for (int u = 0; u < 8; ++u) v += (i0 + 64 * u < hi) ? t8[u] : 0.0;
      }
      v = wave_sum(v);
      if (lane == 0) s_bn[b] = v;
    }
  } else if (part) {  // the slices of k_eval_partial, in slice order
    if ((int)threadIdx.x < R) {
      double v = 0;
      for (int u = 0; u < kEvalSplit; ++u) v += part[threadIdx.x * kEvalSplit + u];
      s_bn[threadIdx.x] = v;
    }
  } else
  // one wave per agent (waves stride over the agents): eight loads in flight per lane, a wave-level sum, no barrier
  {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = kBlock / 64;
    for (int b = w; b < R; b += nw) {
      const int lo = pose_start[b], hi = pose_start[b + 1];
      double v = 0;
      for (int i0 = lo + lane; i0 < hi; i0 += 64 * 8) {
        double t8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t8[u] = posenorm[min(i0 + 64 * u, hi - 1)];
#pragma unroll
        for (int u = 0; u < 8; ++u) v += (i0 + 64 * u < hi) ? t8[u] : 0.0;
      }
      v = wave_sum(v);
      if (lane == 0) s_bn[b] = v;
    }
  }
  // (the block evaluation of a large graph leaves thousands of partials: eight trips' loads in flight at once, added in
  // the order a plain loop would add them)
  for (int i0 = threadIdx.x + kBlock; i0 < npA; i0 += 8 * kBlock) {
    double a8[8], c8[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + u * kBlock;
      a8[u] = i < npA ? pA[2 * i] : 0.0;
      c8[u] = i < npA ? pA[2 * i + 1] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      q0 += a8[u];
      q1 += c8[u];
    }
  }
  const double fq = block_sum(q0, s_red);  // (its barriers also publish s_bn)
  const double fg = block_sum(q1, s_red);
  if (threadIdx.x == 0) {
    double g2 = 0, best = -1;
    int arg = 0;
    for (int b = 0; b < R; ++b) {
      const double nb = sqrt(s_bn[b]);
      out->block_norms[b] = nb;
      g2 += s_bn[b];
      if (nb > best) {
        best = nb;
        arg = b;
      }
    }
    out->cost2 = 2.0 * (0.5 * fq + fg);
    out->gradnorm = sqrt(g2);
    out->next = arg;
    __threadfence_system();
    __hip_atomic_store(const_cast<int *>(&out->seq), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
void launch_eval_finish(hipStream_t st, int R, const int *pose_start, const double *posenorm, const double *pA,
                        int npA, EvalOut *out_dev, int seq, double *split_scratch, int nposes,
                        const double *agent_partials, int wg_per_agent) {
  count_launch();
  const bool split = !agent_partials && split_scratch && nposes >= 16384;
  if (split)
    hipLaunchKernelGGL(k_eval_partial, dim3(R * kEvalSplit), dim3(kBlock), 0, st, pose_start, posenorm, split_scratch);
  hipLaunchKernelGGL(k_eval_finish, dim3(1), dim3(kBlock), 0, st, R, pose_start, posenorm, pA, npA, out_dev, seq,
                     split ? split_scratch : nullptr, agent_partials, wg_per_agent);
}
int eval_split_doubles() { return kMaxAgents * kEvalSplit; }

// one chunk of 32 poses per workgroup up to kBsrMaxGrid workgroups (the Q-apply partial buffer holds that many
// slots): at 100k poses more resident workgroups mean more gathers in flight (34.9 us at 1024, 30.1 us at 2048)
int spmm_bsr_grid(int nbrows) {
  // one resident round: 8 workgroups of 256 threads per CU on 256 CUs
  const int cap = kBsrMaxGrid, per = kPosesPerBlock;
  long g = ((long)nbrows + per - 1) / per;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}
// the quad-per-pose form for every (d, r) the block structure is built for (d <= r <= 8)
template <bool DOTS, bool GRAD>
static bool launch_bsrq(hipStream_t st, int grid, int r, int d, const BsrDev &A, Buf2 X, int selX, const double *G, Buf2 Y,
                        int selY, double *partials, Gate g, const BsrGradOut &go) {
#define DCORA_BSRQ(D_, R_)                                                                                              \
  if (d == D_ && r == R_) {                                                                                             \
    hipLaunchKernelGGL((k_spmm_bsrq<D_, R_, DOTS, GRAD>), dim3(grid), dim3(kQBlock), 0, st, A, X, selX, G, Y, selY, \
                       partials, g, go);                                                                                \
    return true;                                                                                                        \
  }
  DCORA_BSRQ(3, 3) DCORA_BSRQ(3, 4) DCORA_BSRQ(3, 5) DCORA_BSRQ(3, 6) DCORA_BSRQ(3, 7) DCORA_BSRQ(3, 8)
  DCORA_BSRQ(2, 2) DCORA_BSRQ(2, 3) DCORA_BSRQ(2, 4) DCORA_BSRQ(2, 5) DCORA_BSRQ(2, 6) DCORA_BSRQ(2, 7) DCORA_BSRQ(2, 8)
#undef DCORA_BSRQ
  return false;
}
void launch_spmm_bsr(hipStream_t st, int r, int d, const BsrDev &A, Buf2 X, int selX, const double *G, Buf2 Y,
                     int selY, double *partials, Gate g) {
  const int grid = spmm_bsr_grid(A.nbrows);
  const BsrGradOut none{};
  const bool ok = partials ? launch_bsrq<true, false>(st, grid, r, d, A, X, selX, G, Y, selY, partials, g, none)
                           : launch_bsrq<false, false>(st, grid, r, d, A, X, selX, G, Y, selY, partials, g, none);
  if (!ok) throw std::logic_error("block Q-apply: no instantiation for this (d, r); the block structure is built for d <= r <= 8 only");
}
// EG = X Q + G, RG = Proj_X(EG), S blocks, partials {<XQ,X>, <X,G>} in pA (2 per block), |RG|^2 in pB (1 per block) and
// the per-pose norms in ONE launch on the block structure of Q; returns the number of blocks
int launch_fused_grad_bsr(hipStream_t st, int r, int d, const BsrDev &A, Buf2 X, const double *G, Buf2 EG, Buf2 RG, Buf2 S,
                          int sel, double *pA, double *pB, double *posenorm, Gate g, const int *agent_start, int agents,
                          int *wg_per_agent) {
  int grid = spmm_bsr_grid(A.nbrows);
  BsrGradOut go;
  go.RG = RG;
  go.S = S;
  go.pB = pB;
  go.posenorm = posenorm;
  if (agent_start && agents > 0 && wg_per_agent) {
    const int wpa = std::max(1, grid / agents);
    grid = wpa * agents;
    go.agent_start = agent_start;
    go.wg_per_agent = wpa;
    go.posenorm = nullptr;
    *wg_per_agent = wpa;
  }
  if (!launch_bsrq<true, true>(st, grid, r, d, A, X, sel, G, EG, sel, pA, g, go))
    throw std::logic_error("block evaluation: no instantiation for this (d, r); the block structure is built for d <= r <= 8 only");
  return grid;
}
// EG = X Q + G, RG = Proj_X(EG), S blocks, partials {<XQ,X>, <X,G>} in pA (2 per block) and |RG|^2 in pB (1 per
// block); returns the number of blocks.  Small SE blocks without long rows only (the caller checks).
int launch_fused_grad(hipStream_t st, const ManiDesc &m, const CsrDev &Q, Buf2 X, const double *G, Buf2 EG, Buf2 RG,
                      Buf2 Sblk, int sel, double *pA, double *pB, double *posenorm, Gate g, const GradRide *ride) {
  const int grid = fused_pose_blocks(m);
  const GradRide rd = ride ? *ride : GradRide();
  count_launch();
#define DCORA_FUSED_GRAD(D_, RIDE_)                                                                                  \
  hipLaunchKernelGGL((k_fused_grad<D_, RIDE_>), dim3(grid), dim3(kBlock), 0, st, m, Q, X, G, EG, RG, Sblk, sel, pA, pB, \
                     posenorm, g, rd)
  if (m.d == 3) {
    if (rd.c_rp) DCORA_FUSED_GRAD(3, true);
    else DCORA_FUSED_GRAD(3, false);
  } else {
    if (rd.c_rp) DCORA_FUSED_GRAD(2, true);
    else DCORA_FUSED_GRAD(2, false);
  }
#undef DCORA_FUSED_GRAD
  return grid;
}

}  // namespace dcora
