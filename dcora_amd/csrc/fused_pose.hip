// The 8-lanes-per-pose manifold kernels of the SE layout: Riemannian gradient, retraction, Nesterov bookkeeping.
#include "kernels.h"
#include "pose_group.h"

namespace dcora {

namespace {

// ------------------------------------------------------------------------------------------------------
// group-style versions of the per-outer-iteration kernels (SE layout)
// ------------------------------------------------------------------------------------------------------
// RG = Proj_X(EG), S_i = sym(Y_i^T EG_i), partial |RG|^2
template <int D>
__global__ __launch_bounds__(kBlock) void k_g_rgrad(ManiDesc m, Buf2 Xb, Buf2 EGb, Buf2 RGb, Buf2 Sb, int sel,
                                                    double *__restrict__ partials, double *__restrict__ posenorm,
                                                    Gate g) {
  if (gated(g.ctl, g.seq, g.gate)) return;
  __shared__ double s_red[16];
  constexpr int DH = D + 1;
  const int idx = g.ctl ? ((g.ctl->cur ^ sel) & 1) : 0;
  const double *__restrict__ X = Xb.p[idx];
  const double *__restrict__ EG = EGb.p[idx];
  double *__restrict__ RG = RGb.p[idx];
  double *__restrict__ Sblk = Sb.p[idx];
  const int r = m.r;
  const int t = threadIdx.x & (GW - 1);
  double acc = 0;
  for (int pose0 = blockIdx.x * kPosesPerBlock; pose0 < m.n; pose0 += gridDim.x * kPosesPerBlock) {
    const int pose = pose0 + (threadIdx.x >> 3);
    const bool active = (pose < m.n) && (t < r);
    const size_t o = (size_t)pose * DH * r;
    Row<D> Y, E;
    ld_row<D>(X + o, r, t, active, Y);
    ld_row<D>(EG + o, r, t, active, E);
    double S[D][D];
    grp_sym_gram<D>(Y, E, S);
    if (Sblk && pose < m.n && t == 0)
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) Sblk[(size_t)pose * D * D + a + b * D] = S[a][b];
    row_sub_AS<D>(E, Y, S);
    double pa = 0;
#pragma unroll
    for (int a = 0; a < DH; ++a) pa += E.e[a] * E.e[a];
    acc += pa;
    if (posenorm) {  // |RG_i|^2 per pose, for the per-agent block norms of the evaluation
      const double ps = grp_sum(pa);
      if (pose < m.n && t == 0) posenorm[pose] = ps;
    }
    if (RG) st_row<D>(RG + o, r, t, active, E);
  }
  const double tot = block_sum(acc, s_red);
  if (threadIdx.x == 0 && partials) partials[blockIdx.x] = tot;
}

// out = Retr_X(alpha V), partial {<V, grad>, <V, HV>}
template <int D>
__global__ __launch_bounds__(kBlock) void k_g_retract(ManiDesc m, Buf2 Xb, const double *__restrict__ V,
                                                      double alpha, Buf2 Ob, int selOut, Buf2 gradb,
                                                      const double *__restrict__ HV, double *__restrict__ partials,
                                                      Gate g) {
  if (gated(g.ctl, g.seq, g.gate)) return;
  __shared__ double s_red[16];
  constexpr int DH = D + 1;
  const int cur = g.ctl ? (g.ctl->cur & 1) : 0;
  const double *__restrict__ X = Xb.p[cur];
  double *__restrict__ out = Ob.p[g.ctl ? ((cur ^ selOut) & 1) : 0];
  const double *__restrict__ grad = partials ? gradb.p[cur] : nullptr;
  const int r = m.r;
  const int t = threadIdx.x & (GW - 1);
  double a0 = 0, a1 = 0;
  for (int pose0 = blockIdx.x * kPosesPerBlock; pose0 < m.n; pose0 += gridDim.x * kPosesPerBlock) {
    const int pose = pose0 + (threadIdx.x >> 3);
    const bool active = (pose < m.n) && (t < r);
    const size_t o = (size_t)pose * DH * r;
    Row<D> Y, Vr;
    ld_row<D>(X + o, r, t, active, Y);
    ld_row<D>(V + o, r, t, active, Vr);
    if (partials) {
      Row<D> Gr, Hr;
      ld_row<D>(grad + o, r, t, active, Gr);
      ld_row<D>(HV + o, r, t, active, Hr);
#pragma unroll
      for (int a = 0; a < DH; ++a) {
        a0 += Vr.e[a] * Gr.e[a];
        a1 += Vr.e[a] * Hr.e[a];
      }
    }
#pragma unroll
    for (int a = 0; a < DH; ++a) Y.e[a] += alpha * Vr.e[a];
    row_qf<D>(Y);
    st_row<D>(out + o, r, t, active, Y);
  }
  if (partials) {
    const double t0 = block_sum(a0, s_red);
    const double t1 = block_sum(a1, s_red);
    if (threadIdx.x == 0) {
      partials[2 * blockIdx.x] = t0;
      partials[2 * blockIdx.x + 1] = t1;
    }
  }
}

// RBCD++ Nesterov bookkeeping (modes as k_nesterov in manifold.hip)
struct GNesterovArgs {
  int mode, restart, skip_lo, skip_hi;
  double alpha, gamma;
  double *X, *V, *Y, *XPrev, *Yloc;
  double *inner_Yloc;     // mode 0 only: when set, the skipped poses run mode 1 instead (Y and this buffer <- their y)
  Buf2 Xloc;              // result buffers of the local solve
  const SolverCtl *ctl;   // picks Xloc.p[ctl->cur] when non-null
};
template <int D>
__global__ __launch_bounds__(kBlock) void k_g_nesterov(ManiDesc m, GNesterovArgs a) {
  const double *__restrict__ Xloc = a.Xloc.p[a.ctl ? (a.ctl->cur & 1) : 0];
  constexpr int DH = D + 1;
  const int r = m.r;
  const int t = threadIdx.x & (GW - 1);
  for (int pose0 = blockIdx.x * kPosesPerBlock; pose0 < m.n; pose0 += gridDim.x * kPosesPerBlock) {
    const int pose = pose0 + (threadIdx.x >> 3);
    const bool skipped = pose >= a.skip_lo && pose < a.skip_hi;
    const bool inner = skipped && a.inner_Yloc != nullptr && pose < m.n;  // the selected agent's poses, staged here
    const bool inrange = (pose < m.n) && (!skipped || inner);
    const bool active = inrange && (t < r);
    const size_t o = (size_t)pose * DH * r;
    Row<D> x, v, y;
    if (a.mode <= 1) {
      ld_row<D>(a.X + o, r, t, active, x);
      ld_row<D>(a.V + o, r, t, active, v);
#pragma unroll
      for (int c = 0; c < DH; ++c) y.e[c] = (1.0 - a.alpha) * x.e[c] + a.alpha * v.e[c];
      const double yt = y.e[D];
      row_polar<D>(y, inrange);
      y.e[D] = yt;
      st_row<D>(a.XPrev + o, r, t, active, x);
      if (a.mode == 1 || inner) {
        st_row<D>(a.Y + o, r, t, active, y);
        double *yl = inner ? a.inner_Yloc + (size_t)(pose - a.skip_lo) * DH * r : a.Yloc + o;
        st_row<D>(yl, r, t, active, y);
      } else if (a.restart & 1) {
        st_row<D>(a.V + o, r, t, active, x);
        st_row<D>(a.Y + o, r, t, active, x);
        // uniform control flow for the second polar below is not needed: restart is a kernel argument
      } else {
        st_row<D>(a.Y + o, r, t, active, y);
        st_row<D>(a.X + o, r, t, active, y);
        // V <- proj(V + gamma (X - Y)) with X == Y.  Bit 1 of `restart`: V is known to be feasible (it is the output
        // of a projection or a copy of a feasible X since the last set_X), its re-projection is the identity.
        if (!(a.restart & 2)) {
          const double vt = v.e[D];
          row_polar<D>(v, inrange);
          v.e[D] = vt;
          st_row<D>(a.V + o, r, t, active, v);
        }
      }
    } else {
      ld_row<D>(Xloc + o, r, t, active, x);
      st_row<D>(a.X + o, r, t, active, x);
      if (a.mode == 2) {
        ld_row<D>(a.V + o, r, t, active, v);
        ld_row<D>(a.Y + o, r, t, active, y);
#pragma unroll
        for (int c = 0; c < DH; ++c) v.e[c] += a.gamma * (x.e[c] - y.e[c]);
        const double vt = v.e[D];
        row_polar<D>(v, inrange);
        v.e[D] = vt;
        st_row<D>(a.V + o, r, t, active, v);
      } else {
        st_row<D>(a.V + o, r, t, active, x);
        st_row<D>(a.Y + o, r, t, active, x);
      }
    }
  }
}

int group_grid(int n) {
  long g = ((long)n + kPosesPerBlock - 1) / kPosesPerBlock;
  if (g < 1) g = 1;
  if (g > kMaxPartials) g = kMaxPartials;
  return (int)g;
}

}  // namespace

// the 8-lanes-per-pose kernels (rgrad / retract / Nesterov / BSR Q-apply) walk the poses with a capped grid: any n
bool group_supported(const ManiDesc &m) { return m.se && m.r <= GW && m.n > 0; }
int launch_g_rgrad(hipStream_t st, const ManiDesc &m, Buf2 X, Buf2 EG, Buf2 RG, Buf2 Sblk, int sel, double *partials,
                   double *posenorm, Gate g) {
  const int grid = group_grid(m.n);
  DCORA_LAUNCH_D(k_g_rgrad, m.d, grid, st, m, X, EG, RG, Sblk, sel, partials, posenorm, g);
  return grid;
}
int launch_g_retract(hipStream_t st, const ManiDesc &m, Buf2 X, const double *V, double alpha, Buf2 out, int selOut,
                     Buf2 grad, const double *HV, double *partials, Gate g) {
  const int grid = group_grid(m.n);
  DCORA_LAUNCH_D(k_g_retract, m.d, grid, st, m, X, V, alpha, out, selOut, grad, HV, partials, g);
  return grid;
}
void launch_g_nesterov(hipStream_t st, const ManiDesc &m, int mode, int restart, int skip_lo, int skip_hi,
                       double alpha, double gamma, double *X, double *V, double *Y, double *XPrev, double *Yloc,
                       Buf2 Xloc, const SolverCtl *ctl, double *inner_Yloc) {
  count_launch();
  GNesterovArgs a{mode, restart, skip_lo, skip_hi, alpha, gamma, X, V, Y, XPrev, Yloc, inner_Yloc, Xloc, ctl};
  const int grid = group_grid(m.n);
  DCORA_LAUNCH_D(k_g_nesterov, m.d, grid, st, m, a);
}

}  // namespace dcora
