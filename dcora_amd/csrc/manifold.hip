// Thread-per-variable kernels of the product manifold St(d, r)^n x S^(r-1)^l x R^r x ...: tangent projection, Riemannian
// Hessian correction, QF retraction, metric projection, the dual certificate's Lambda blocks and the RBCD++ Nesterov
// bookkeeping.  They carry the RA layout, every rank above 8, DCORA_SOLVER=generic and the host-pointer operator API.
// Each kernel walks the num_items() items of its ManiDesc (kernels.h) by grid stride, one thread per item: Stiefel
// blocks first, then sphere columns, then Euclidean columns, as ManiDesc::item numbers them.
#include "kernels.h"
#include "tcg_rules.h"

namespace dcora {

// ------------------------------------------------------------------------------------------------------
// per-pose register-resident blocks: D columns of RM (>= r) rows, statically indexed
// ------------------------------------------------------------------------------------------------------
template <int D, int RM>
struct Blk {
  double a[D][RM];
};
template <int D, int RM>
__device__ __forceinline__ void ld_blk(const double *__restrict__ p, int r, Blk<D, RM> &B) {
#pragma unroll
  for (int c = 0; c < D; ++c)
#pragma unroll
    for (int t = 0; t < RM; ++t) B.a[c][t] = (t < r) ? p[c * r + t] : 0.0;
}
template <int D, int RM>
__device__ __forceinline__ void st_blk(double *__restrict__ p, int r, const Blk<D, RM> &B) {
#pragma unroll
  for (int c = 0; c < D; ++c)
#pragma unroll
    for (int t = 0; t < RM; ++t)
      if (t < r) p[c * r + t] = B.a[c][t];
}
// S = sym(Y^T E)
template <int D, int RM>
__device__ __forceinline__ void sym_gram(const Blk<D, RM> &Y, const Blk<D, RM> &E, double (&S)[D][D]) {
  double P[D][D];
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) {
      double s = 0;
#pragma unroll
      for (int t = 0; t < RM; ++t) s += Y.a[a][t] * E.a[b][t];
      P[a][b] = s;
    }
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) S[a][b] = 0.5 * (P[a][b] + P[b][a]);
}
// V <- V - A S   (A, V: RM x D blocks; S: D x D)
template <int D, int RM>
__device__ __forceinline__ void sub_AS(Blk<D, RM> &V, const Blk<D, RM> &A, const double (&S)[D][D]) {
#pragma unroll
  for (int b = 0; b < D; ++b)
#pragma unroll
    for (int t = 0; t < RM; ++t) {
      double s = 0;
#pragma unroll
      for (int a = 0; a < D; ++a) s += A.a[a][t] * S[a][b];
      V.a[b][t] -= s;
    }
}
template <int D, int RM>
__device__ __forceinline__ double blk_dot(const Blk<D, RM> &A, const Blk<D, RM> &B) {
  double s = 0;
#pragma unroll
  for (int c = 0; c < D; ++c)
#pragma unroll
    for (int t = 0; t < RM; ++t) s += A.a[c][t] * B.a[c][t];
  return s;
}
// thin QR by modified Gram-Schmidt with one re-orthogonalisation pass; returns Q (R has positive diagonal)
template <int D, int RM>
__device__ __forceinline__ void qf_blk(Blk<D, RM> &A) {
#pragma unroll
  for (int j = 0; j < D; ++j) {
#pragma unroll
    for (int pass = 0; pass < 2; ++pass)
#pragma unroll
      for (int c = 0; c < D; ++c)
        if (c < j) {
          double s = 0;
#pragma unroll
          for (int t = 0; t < RM; ++t) s += A.a[c][t] * A.a[j][t];
#pragma unroll
          for (int t = 0; t < RM; ++t) A.a[j][t] -= s * A.a[c][t];
        }
    double nn = 0;
#pragma unroll
    for (int t = 0; t < RM; ++t) nn += A.a[j][t] * A.a[j][t];
    const double inv = 1.0 / sqrt(nn);
#pragma unroll
    for (int t = 0; t < RM; ++t) A.a[j][t] *= inv;
  }
}
// polar factor U V^T by one-sided (Hestenes) Jacobi: rotate column pairs until mutually orthogonal
template <int D, int RM>
__device__ __forceinline__ void polar_blk(Blk<D, RM> &A) {
  double Vm[D][D];
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) Vm[a][b] = (a == b) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 40; ++sweep) {
    double off = 0;
#pragma unroll
    for (int p = 0; p < D - 1; ++p)
#pragma unroll
      for (int q = p + 1; q < D; ++q) {
        double app = 0, aqq = 0, apq = 0;
#pragma unroll
        for (int t = 0; t < RM; ++t) {
          app += A.a[p][t] * A.a[p][t];
          aqq += A.a[q][t] * A.a[q][t];
          apq += A.a[p][t] * A.a[q][t];
        }
        const double sc = sqrt(app * aqq);
        if (fabs(apq) > 1e-16 * sc && fabs(apq) > 1e-300) {
          off = fmax(off, fabs(apq) / sc);
          const double zeta = (aqq - app) / (2.0 * apq);
          const double tt = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
#pragma unroll
          for (int t = 0; t < RM; ++t) {
            const double x = A.a[p][t], y = A.a[q][t];
            A.a[p][t] = cs * x - sn * y;
            A.a[q][t] = sn * x + cs * y;
          }
#pragma unroll
          for (int i = 0; i < D; ++i) {
            const double x = Vm[p][i], y = Vm[q][i];
            Vm[p][i] = cs * x - sn * y;
            Vm[q][i] = sn * x + cs * y;
          }
        }
      }
    if (off < 1e-15) break;
  }
  // columns of A are U Sigma; Vm[j][i] = V(i, j)
#pragma unroll
  for (int j = 0; j < D; ++j) {
    double nn = 0;
#pragma unroll
    for (int t = 0; t < RM; ++t) nn += A.a[j][t] * A.a[j][t];
    const double inv = nn > 0 ? 1.0 / sqrt(nn) : 0.0;
#pragma unroll
    for (int t = 0; t < RM; ++t) A.a[j][t] *= inv;
  }
  Blk<D, RM> O;
#pragma unroll
  for (int c = 0; c < D; ++c)
#pragma unroll
    for (int t = 0; t < RM; ++t) {
      double s = 0;
#pragma unroll
      for (int j = 0; j < D; ++j) s += A.a[j][t] * Vm[j][c];
      O.a[c][t] = s;
    }
  A = O;
}

int pose_grid(const ManiDesc &m) {
  long g = (m.num_items() + kBlock - 1) / kBlock;
  if (g < 1) g = 1;
  if (g > kMaxPartials) g = kMaxPartials;
  return (int)g;
}

// ---- Riemannian gradient: RG = Proj_X(EG), S_i = sym(Y_i^T EG_i) ----------------------------------------
template <int D, int RM>
__global__ __launch_bounds__(kBlock) void k_rgrad(ManiDesc m, Buf2 Xb, Buf2 EGb, Buf2 RGb, Buf2 Sb, int sel,
                                                  double *__restrict__ partials, Gate g) {
  if (gated(g.ctl, g.seq, g.gate)) return;
  __shared__ double s_red[16];
  const double *X = pick(Xb, g.ctl, sel);
  const double *EG = pick(EGb, g.ctl, sel);
  double *RG = pick(RGb, g.ctl, sel);
  double *Sblk = pick(Sb, g.ctl, sel);
  const int r = m.r;
  const long items = m.num_items();
  double acc = 0;
  for (long it = (long)blockIdx.x * kBlock + threadIdx.x; it < items; it += (long)gridDim.x * kBlock) {
    if (it < m.n) {
      const size_t o = (size_t)m.rot_col((int)it) * r;
      Blk<D, RM> Y, E;
      ld_blk<D, RM>(X + o, r, Y);
      ld_blk<D, RM>(EG + o, r, E);
      double S[D][D];
      sym_gram<D, RM>(Y, E, S);
      if (Sblk)
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
          for (int b = 0; b < D; ++b) Sblk[(size_t)it * D * D + a + b * D] = S[a][b];
      sub_AS<D, RM>(E, Y, S);
      acc += blk_dot<D, RM>(E, E);
      if (RG) st_blk<D, RM>(RG + o, r, E);
    } else if (it < m.n + m.l) {
      const int i = (int)(it - m.n);
      const size_t o = (size_t)m.sphere_col(i) * r;
      double s = 0;
      for (int t = 0; t < r; ++t) s += X[o + t] * EG[o + t];
      if (Sblk) Sblk[(size_t)m.n * D * D + i] = s;
      for (int t = 0; t < r; ++t) {
        const double v = EG[o + t] - X[o + t] * s;
        acc += v * v;
        if (RG) RG[o + t] = v;
      }
    } else {
      const size_t o = (size_t)m.euc_col((int)(it - m.n - m.l)) * r;
      for (int t = 0; t < r; ++t) {
        const double v = EG[o + t];
        acc += v * v;
        if (RG) RG[o + t] = v;
      }
    }
  }
  const double tot = block_sum(acc, s_red);
  if (threadIdx.x == 0 && partials) partials[blockIdx.x] = tot;
}

// ---- out = Proj_X(V), partial <out, R>; optional tCG residual stopping rule in the prologue ---------------
template <int D, int RM>
__global__ __launch_bounds__(kBlock) void k_tangent(ManiDesc m, Buf2 Xb, const double *__restrict__ V,
                                                    double *__restrict__ out, const double *__restrict__ R,
                                                    double *__restrict__ partials, const double *__restrict__ p2,
                                                    int np2, SolverCtl *ctl, HostFlags *hf, int seq, int gate,
                                                    int iter, SpFold sf) {
  __shared__ double s_red[16];
  __shared__ double s_x2[64 * 16];
  // Loads that depend on nothing are requested before the gate is looked at -- the stopping rule's partials and |r0|,
  // the hub's index, the places of the thread's first columns in the replay's images: with the gate they are one
  // memory round trip where they were five in a row (k_tangent on tiers.pyfg: 9.9 us for 0.6 MB vectors, all of it
  // dependent round trips).  The empty asm keeps the compiler from sinking them behind the early return.
  const int r = m.r;
  const long items = m.num_items();
  const bool folded = sf.y != nullptr;
  const GateWords gw = gate_words(ctl);
  double pv = (p2 && (int)threadIdx.x < np2) ? p2[threadIdx.x] : 0.0;
  const double n0 = p2 ? ctl->norm_r0 : 0.0;
  const bool hub0 = folded && sf.h > 0 && (int)threadIdx.x < sf.h * r;
  double x2_0 = hub0 ? sf.hub_x2[threadIdx.x] : 0.0;
  const long it0 = (long)blockIdx.x * kBlock + threadIdx.x;
  int jp_pre[D], op_pre[D];
#pragma unroll
  for (int a = 0; a < D; ++a) jp_pre[a] = op_pre[a] = 0;
  if (folded && it0 < items) {
    const ManiItem e0 = m.item(it0);
    const size_t c0 = (size_t)e0.col;
    const int nc0 = e0.kind == Factor::Stiefel ? D : 1;
#pragma unroll
    for (int a = 0; a < D; ++a)
      if (a < nc0) {
        jp_pre[a] = sf.in_pos[c0 + a];
        op_pre[a] = sf.out_pos[c0 + a];
      }
  }
#pragma unroll
  for (int a = 0; a < D; ++a) asm volatile("" ::"v"(jp_pre[a]), "v"(op_pre[a]));
  asm volatile("" ::"v"(pv), "v"(n0), "v"(x2_0), "s"(gw.outer), "s"(gw.tcg));
  if (gated(gw, ctl, seq, gate)) return;
  if (p2) {
    for (int i = threadIdx.x + blockDim.x; i < np2; i += blockDim.x) pv += p2[i];
    const double nr = sqrt(block_sum(pv, s_red));
    if (tcg_residual_done(nr, n0)) {
      if (blockIdx.x == 0 && threadIdx.x == 0) tcg_end_run(ctl, hf, seq, tcg_residual_status(n0), iter + 1);
      return;
    }
  }
  const double *X = pick(Xb, ctl, 0);
  // sparse preconditioner folded in (generic layout): V(col, t) is read from where the level replay left it, with the
  // hub correction of k_sp_permute_out_hub; x2 = Sinv (R(hub) - U^T r1) comes ready from the replay's second launch
  // (round 4 rebuilt it here in every workgroup: two dependent rounds of loads and two barriers in front of the items)
  if (folded && sf.h > 0) {
    if (hub0) s_x2[threadIdx.x] = x2_0;
    for (int e = threadIdx.x + kBlock; e < sf.h * r; e += kBlock) s_x2[e] = sf.hub_x2[e];
    __syncthreads();
  }
  // NC consecutive columns starting at col0: positions first (the thread's first item: requested in the prologue), then
  // every value, straight line (a hub column -- rare -- is patched afterwards)
  auto vcols = [&](size_t col0, auto nc_tag, double (*vv)[RM], bool first) {
    constexpr int NC = decltype(nc_tag)::value;
    int jp[NC], op[NC];
#pragma unroll
    for (int a = 0; a < NC; ++a) {
      jp[a] = first ? jp_pre[a] : sf.in_pos[col0 + a];
      op[a] = first ? op_pre[a] : sf.out_pos[col0 + a];
    }
#pragma unroll
    for (int a = 0; a < NC; ++a)
#pragma unroll
      for (int t = 0; t < RM; ++t) vv[a][t] = (t < r) ? sf.y[(size_t)max(op[a], 0) * r + t] : 0.0;
    for (int q = 0; q < sf.h; ++q) {
      double u[NC];
#pragma unroll
      for (int a = 0; a < NC; ++a) u[a] = sf.hub_U[(size_t)max(jp[a], 0) * sf.h + q];
#pragma unroll
      for (int a = 0; a < NC; ++a)
#pragma unroll
        for (int t = 0; t < RM; ++t)
          if (t < r) vv[a][t] -= u[a] * s_x2[q * r + t];
    }
#pragma unroll
    for (int a = 0; a < NC; ++a)
      if (jp[a] < 0) {
#pragma unroll
        for (int t = 0; t < RM; ++t) vv[a][t] = 0.0;
        for (int q = 0; q < sf.h; ++q)
          if ((size_t)sf.hub_idx[q] == col0 + a)
#pragma unroll
            for (int t = 0; t < RM; ++t)
              if (t < r) vv[a][t] = s_x2[q * r + t];
      }
  };
  double acc = 0;
  for (long it = (long)blockIdx.x * kBlock + threadIdx.x; it < items; it += (long)gridDim.x * kBlock) {
    if (it < m.n) {
      const size_t o = (size_t)m.rot_col((int)it) * r;
      Blk<D, RM> Y, W;
      ld_blk<D, RM>(X + o, r, Y);
      if (folded) {
        vcols((size_t)m.rot_col((int)it), std::integral_constant<int, D>{}, W.a, it == it0);
      } else {
        ld_blk<D, RM>(V + o, r, W);
      }
      double S[D][D];
      sym_gram<D, RM>(Y, W, S);
      sub_AS<D, RM>(W, Y, S);
      if (R) {
        Blk<D, RM> Rr;
        ld_blk<D, RM>(R + o, r, Rr);
        acc += blk_dot<D, RM>(W, Rr);
      }
      st_blk<D, RM>(out + o, r, W);
    } else if (it < m.n + m.l) {
      const size_t col = (size_t)m.sphere_col((int)(it - m.n));
      const size_t o = col * r;
      double vv1[1][RM];
      if (folded) {
        vcols(col, std::integral_constant<int, 1>{}, vv1, it == it0);
      } else {
#pragma unroll
        for (int t = 0; t < RM; ++t) vv1[0][t] = (t < r) ? V[o + t] : 0.0;
      }
      const double *vv = vv1[0];
      double s = 0;
#pragma unroll
      for (int t = 0; t < RM; ++t)
        if (t < r) s += X[o + t] * vv[t];
#pragma unroll
      for (int t = 0; t < RM; ++t)
        if (t < r) {
          const double v = vv[t] - X[o + t] * s;
          if (R) acc += v * R[o + t];
          out[o + t] = v;
        }
    } else {
      const size_t col = (size_t)m.euc_col((int)(it - m.n - m.l));
      const size_t o = col * r;
      double ve[1][RM];
      if (folded) {
        vcols(col, std::integral_constant<int, 1>{}, ve, it == it0);
      } else {
#pragma unroll
        for (int t = 0; t < RM; ++t) ve[0][t] = (t < r) ? V[o + t] : 0.0;
      }
#pragma unroll
      for (int t = 0; t < RM; ++t)
        if (t < r) {
          const double v = ve[0][t];
          if (R) acc += v * R[o + t];
          out[o + t] = v;
        }
    }
  }
  if (partials) {
    const double tot = block_sum(acc, s_red);
    if (threadIdx.x == 0) partials[blockIdx.x] = tot;
  }
  // the last kernel of a tCG iteration when the direction update is folded into the next SpMM: paces the host
  if (hf && gate == 2 && blockIdx.x == 0 && threadIdx.x == 0) host_store(&hf->last_seq_done, seq);
}

// ---- HV = Proj_X(W - V S), partial <V, HV>  (ROPTLIB EucHvToHv for the Euclidean metric) -----------------
template <int D, int RM>
__global__ __launch_bounds__(kBlock) void k_hessfix(ManiDesc m, Buf2 Xb, Buf2 Sb, const double *__restrict__ V,
                                                    const double *__restrict__ W, double *__restrict__ HV,
                                                    double *__restrict__ partials, Gate g) {
  if (gated(g.ctl, g.seq, g.gate)) return;
  __shared__ double s_red[16];
  const double *X = pick(Xb, g.ctl, 0);
  const double *Sblk = pick(Sb, g.ctl, 0);
  const int r = m.r;
  const long items = m.num_items();
  double acc = 0;
  for (long it = (long)blockIdx.x * kBlock + threadIdx.x; it < items; it += (long)gridDim.x * kBlock) {
    if (it < m.n) {
      const size_t o = (size_t)m.rot_col((int)it) * r;
      Blk<D, RM> Y, Vb, T;
      ld_blk<D, RM>(X + o, r, Y);
      ld_blk<D, RM>(V + o, r, Vb);
      ld_blk<D, RM>(W + o, r, T);
      double S[D][D];
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) S[a][b] = Sblk[(size_t)it * D * D + a + b * D];
      sub_AS<D, RM>(T, Vb, S);
      double S2[D][D];
      sym_gram<D, RM>(Y, T, S2);
      sub_AS<D, RM>(T, Y, S2);
      acc += blk_dot<D, RM>(Vb, T);
      st_blk<D, RM>(HV + o, r, T);
    } else if (it < m.n + m.l) {
      const int i = (int)(it - m.n);
      const size_t o = (size_t)m.sphere_col(i) * r;
      const double s = Sblk[(size_t)m.n * D * D + i];
      double yt = 0;
      for (int t = 0; t < r; ++t) yt += X[o + t] * (W[o + t] - V[o + t] * s);
      for (int t = 0; t < r; ++t) {
        const double v = (W[o + t] - V[o + t] * s) - X[o + t] * yt;
        acc += V[o + t] * v;
        HV[o + t] = v;
      }
    } else {
      const size_t o = (size_t)m.euc_col((int)(it - m.n - m.l)) * r;
      for (int t = 0; t < r; ++t) {
        const double v = W[o + t];
        acc += V[o + t] * v;
        HV[o + t] = v;
      }
    }
  }
  const double tot = block_sum(acc, s_red);
  if (threadIdx.x == 0 && partials) partials[blockIdx.x] = tot;
}

// ---- out = Retr_X(alpha V): QF on Stiefel blocks, normalise spheres, add on Euclidean columns --------------
template <int D, int RM>
__global__ __launch_bounds__(kBlock) void k_retract(ManiDesc m, Buf2 Xb, const double *__restrict__ V,
                                                    double alpha, Buf2 Ob, int selOut, Buf2 gradb,
                                                    const double *__restrict__ HV, double *__restrict__ partials,
                                                    Gate g) {
  if (gated(g.ctl, g.seq, g.gate)) return;
  __shared__ double s_red[16];
  const double *X = pick(Xb, g.ctl, 0);
  double *out = pick(Ob, g.ctl, selOut);
  const double *grad = partials ? pick(gradb, g.ctl, 0) : nullptr;
  const int r = m.r;
  const long items = m.num_items();
  double a0 = 0, a1 = 0;
  for (long it = (long)blockIdx.x * kBlock + threadIdx.x; it < items; it += (long)gridDim.x * kBlock) {
    size_t o;
    int ncol;
    if (it < m.n) {
      o = (size_t)m.rot_col((int)it) * r;
      ncol = D;
      Blk<D, RM> Y, Vb;
      ld_blk<D, RM>(X + o, r, Y);
      ld_blk<D, RM>(V + o, r, Vb);
#pragma unroll
      for (int c = 0; c < D; ++c)
#pragma unroll
        for (int t = 0; t < RM; ++t) Y.a[c][t] += alpha * Vb.a[c][t];
      qf_blk<D, RM>(Y);
      st_blk<D, RM>(out + o, r, Y);
    } else if (it < m.n + m.l) {
      o = (size_t)m.sphere_col((int)(it - m.n)) * r;
      ncol = 1;
      double nn = 0;
      for (int t = 0; t < r; ++t) {
        const double w = X[o + t] + alpha * V[o + t];
        nn += w * w;
      }
      const double inv = 1.0 / sqrt(nn);
      for (int t = 0; t < r; ++t) out[o + t] = (X[o + t] + alpha * V[o + t]) * inv;
    } else {
      o = (size_t)m.euc_col((int)(it - m.n - m.l)) * r;
      ncol = 1;
      for (int t = 0; t < r; ++t) out[o + t] = X[o + t] + alpha * V[o + t];
    }
    if (partials)
      for (int e = 0; e < ncol * r; ++e) {
        const double v = V[o + e];
        a0 += v * grad[o + e];
        a1 += v * HV[o + e];
      }
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

// ---- out = P_M(c0 A + c1 B + c2 C): polar factor per Stiefel block, normalised spheres --------------------
template <int D, int RM>
__global__ __launch_bounds__(kBlock) void k_polar(ManiDesc m, double c0, const double *__restrict__ A, double c1,
                                                  const double *__restrict__ B, double c2,
                                                  const double *__restrict__ C, double *__restrict__ out) {
  const int r = m.r;
  const long items = m.num_items();
  for (long it = (long)blockIdx.x * kBlock + threadIdx.x; it < items; it += (long)gridDim.x * kBlock) {
    if (it < m.n) {
      const size_t o = (size_t)m.rot_col((int)it) * r;
      Blk<D, RM> M, T;
      ld_blk<D, RM>(A + o, r, M);
#pragma unroll
      for (int c = 0; c < D; ++c)
#pragma unroll
        for (int t = 0; t < RM; ++t) M.a[c][t] *= c0;
      if (B) {
        ld_blk<D, RM>(B + o, r, T);
#pragma unroll
        for (int c = 0; c < D; ++c)
#pragma unroll
          for (int t = 0; t < RM; ++t) M.a[c][t] += c1 * T.a[c][t];
      }
      if (C) {
        ld_blk<D, RM>(C + o, r, T);
#pragma unroll
        for (int c = 0; c < D; ++c)
#pragma unroll
          for (int t = 0; t < RM; ++t) M.a[c][t] += c2 * T.a[c][t];
      }
      polar_blk<D, RM>(M);
      st_blk<D, RM>(out + o, r, M);
    } else {
      const bool sph = it < m.n + m.l;
      const size_t o = (size_t)(sph ? m.sphere_col((int)(it - m.n)) : m.euc_col((int)(it - m.n - m.l))) * r;
      double nn = 0;
      for (int t = 0; t < r; ++t) {
        double w = c0 * A[o + t];
        if (B) w += c1 * B[o + t];
        if (C) w += c2 * C[o + t];
        nn += w * w;
      }
      const double inv = sph ? 1.0 / sqrt(nn) : 1.0;
      for (int t = 0; t < r; ++t) {
        double w = c0 * A[o + t];
        if (B) w += c1 * B[o + t];
        if (C) w += c2 * C[o + t];
        out[o + t] = w * inv;
      }
    }
  }
}

// ---- Lambda blocks of the dual certificate -----------------------------------------------------------------
template <int D, int RM>
__global__ __launch_bounds__(kBlock) void k_lambda(ManiDesc m, const double *__restrict__ X,
                                                   const double *__restrict__ XQ, double *__restrict__ L) {
  const int r = m.r;
  const long items = (long)m.n + m.l;
  for (long it = (long)blockIdx.x * kBlock + threadIdx.x; it < items; it += (long)gridDim.x * kBlock) {
    if (it < m.n) {
      const size_t o = (size_t)m.rot_col((int)it) * r;
      Blk<D, RM> Y, E;
      ld_blk<D, RM>(X + o, r, Y);
      ld_blk<D, RM>(XQ + o, r, E);
      double S[D][D];
      sym_gram<D, RM>(E, Y, S);
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) L[(size_t)it * D * D + a + b * D] = S[a][b];
    } else {
      const int i = (int)(it - m.n);
      const size_t o = (size_t)m.sphere_col(i) * r;
      double s = 0;
      for (int t = 0; t < r; ++t) s += X[o + t] * XQ[o + t];
      L[(size_t)m.n * D * D + i] = s;
    }
  }
}

// ---- RBCD++ Nesterov bookkeeping on a range of poses (ref src/Agent.cpp:545-551, 1158-1214) ---------------
//  mode 0 (agent not selected): XPrev = X; Y = P((1-a) X + a V); X = Y; V = P(V + g (X - Y));
//                               on restart: X = XPrev; V = X; Y = X
//  mode 1 (selected, before the local solve): XPrev = X; Y = P((1-a) X + a V); Yloc = Y
//  mode 2 (selected, after the local solve):  X = Xloc; V = P(V + g (X - Y))
//  mode 3 (selected, after the restart solve): X = Xloc; V = X; Y = X
// Global arrays (X, V, Y, XPrev) are offset to the range's first column; Yloc / Xloc are agent-local buffers.
struct NesterovArgs {
  int mode, restart, skip_lo, skip_hi;
  double alpha, gamma;
  double *X, *V, *Y, *XPrev, *Yloc;
  const double *Xloc;
};
template <int D, int RM>
__global__ __launch_bounds__(kBlock) void k_nesterov(ManiDesc m, NesterovArgs a) {
  const int r = m.r;
  const long items = m.num_items();
  for (long it = (long)blockIdx.x * kBlock + threadIdx.x; it < items; it += (long)gridDim.x * kBlock) {
    int kind;  // 0 Stiefel, 1 sphere, 2 Euclidean
    size_t o;
    long pose = -1;
    if (it < m.n) {
      kind = 0;
      o = (size_t)m.rot_col((int)it) * r;
      pose = it;
    } else if (it < m.n + m.l) {
      kind = 1;
      o = (size_t)m.sphere_col((int)(it - m.n)) * r;
    } else {
      kind = 2;
      const int e = (int)(it - m.n - m.l);
      o = (size_t)m.euc_col(e) * r;
      if (m.se) pose = e;
    }
    if (pose >= a.skip_lo && pose < a.skip_hi) continue;
    if (kind == 0) {
      Blk<D, RM> x, v, y;
      if (a.mode <= 1) {
        ld_blk<D, RM>(a.X + o, r, x);
        ld_blk<D, RM>(a.V + o, r, v);
        st_blk<D, RM>(a.XPrev + o, r, x);
#pragma unroll
        for (int c = 0; c < D; ++c)
#pragma unroll
          for (int t = 0; t < RM; ++t) y.a[c][t] = (1.0 - a.alpha) * x.a[c][t] + a.alpha * v.a[c][t];
        polar_blk<D, RM>(y);
        if (a.mode == 1) {
          st_blk<D, RM>(a.Y + o, r, y);
          st_blk<D, RM>(a.Yloc + o, r, y);
        } else if (a.restart) {
          st_blk<D, RM>(a.X + o, r, x);
          st_blk<D, RM>(a.V + o, r, x);
          st_blk<D, RM>(a.Y + o, r, x);
        } else {
          polar_blk<D, RM>(v);  // V + g (X - Y) with X == Y
          st_blk<D, RM>(a.Y + o, r, y);
          st_blk<D, RM>(a.X + o, r, y);
          st_blk<D, RM>(a.V + o, r, v);
        }
      } else {
        ld_blk<D, RM>(a.Xloc + o, r, x);
        st_blk<D, RM>(a.X + o, r, x);
        if (a.mode == 2) {
          ld_blk<D, RM>(a.V + o, r, v);
          ld_blk<D, RM>(a.Y + o, r, y);
#pragma unroll
          for (int c = 0; c < D; ++c)
#pragma unroll
            for (int t = 0; t < RM; ++t) v.a[c][t] += a.gamma * (x.a[c][t] - y.a[c][t]);
          polar_blk<D, RM>(v);
          st_blk<D, RM>(a.V + o, r, v);
        } else {
          st_blk<D, RM>(a.V + o, r, x);
          st_blk<D, RM>(a.Y + o, r, x);
        }
      }
    } else {
      // single column: sphere (normalise) or Euclidean (identity)
      const bool sph = (kind == 1);
      if (a.mode <= 1) {
        double nn = 0;
        for (int t = 0; t < r; ++t) {
          const double w = (1.0 - a.alpha) * a.X[o + t] + a.alpha * a.V[o + t];
          nn += w * w;
        }
        const double inv = sph ? 1.0 / sqrt(nn) : 1.0;
        double vn = 0;
        for (int t = 0; t < r; ++t) vn += a.V[o + t] * a.V[o + t];
        const double vinv = sph ? 1.0 / sqrt(vn) : 1.0;
        for (int t = 0; t < r; ++t) {
          const double x = a.X[o + t], v = a.V[o + t];
          const double y = ((1.0 - a.alpha) * x + a.alpha * v) * inv;
          a.XPrev[o + t] = x;
          if (a.mode == 1) {
            a.Y[o + t] = y;
            a.Yloc[o + t] = y;
          } else if (a.restart) {
            a.V[o + t] = x;
            a.Y[o + t] = x;
          } else {
            a.Y[o + t] = y;
            a.X[o + t] = y;
            a.V[o + t] = v * vinv;
          }
        }
      } else if (a.mode == 2) {
        double nn = 0;
        for (int t = 0; t < r; ++t) {
          const double w = a.V[o + t] + a.gamma * (a.Xloc[o + t] - a.Y[o + t]);
          nn += w * w;
        }
        const double inv = sph ? 1.0 / sqrt(nn) : 1.0;
        for (int t = 0; t < r; ++t) {
          const double x = a.Xloc[o + t];
          const double w = a.V[o + t] + a.gamma * (x - a.Y[o + t]);
          a.X[o + t] = x;
          a.V[o + t] = w * inv;
        }
      } else {
        for (int t = 0; t < r; ++t) {
          const double x = a.Xloc[o + t];
          a.X[o + t] = x;
          a.V[o + t] = x;
          a.Y[o + t] = x;
        }
      }
    }
  }
}

#define DCORA_DISPATCH_POSE(KERNEL, m, grid, st, ...)                                              \
  do {                                                                                             \
    const int rm_ = (m).r <= 4 ? 4 : ((m).r <= 8 ? 8 : 16);                                        \
    if ((m).d == 3) {                                                                              \
      if (rm_ == 4) hipLaunchKernelGGL((KERNEL<3, 4>), dim3(grid), dim3(kBlock), 0, st, __VA_ARGS__);       \
      else if (rm_ == 8) hipLaunchKernelGGL((KERNEL<3, 8>), dim3(grid), dim3(kBlock), 0, st, __VA_ARGS__);  \
      else hipLaunchKernelGGL((KERNEL<3, 16>), dim3(grid), dim3(kBlock), 0, st, __VA_ARGS__);               \
    } else {                                                                                       \
      if (rm_ == 4) hipLaunchKernelGGL((KERNEL<2, 4>), dim3(grid), dim3(kBlock), 0, st, __VA_ARGS__);       \
      else if (rm_ == 8) hipLaunchKernelGGL((KERNEL<2, 8>), dim3(grid), dim3(kBlock), 0, st, __VA_ARGS__);  \
      else hipLaunchKernelGGL((KERNEL<2, 16>), dim3(grid), dim3(kBlock), 0, st, __VA_ARGS__);               \
    }                                                                                              \
  } while (0)

void launch_rgrad(hipStream_t st, const ManiDesc &m, Buf2 X, Buf2 EG, Buf2 RG, Buf2 Sblk, int sel,
                  double *partials, Gate g) {
  const int grid = pose_grid(m);
  DCORA_DISPATCH_POSE(k_rgrad, m, grid, st, m, X, EG, RG, Sblk, sel, partials, g);
}
void launch_tangent(hipStream_t st, const ManiDesc &m, Buf2 X, const double *V, double *out, const double *R,
                    double *partials, const double *p2, int np2, SolverCtl *ctl, HostFlags *hf, int seq,
                    int gate, int iter, SpFold sf) {
  const int grid = pose_grid(m);
  DCORA_DISPATCH_POSE(k_tangent, m, grid, st, m, X, V, out, R, partials, p2, np2, ctl, hf, seq, gate, iter, sf);
}
void launch_hessfix(hipStream_t st, const ManiDesc &m, Buf2 X, Buf2 Sblk, const double *V, const double *W,
                    double *HV, double *partials, Gate g) {
  const int grid = pose_grid(m);
  DCORA_DISPATCH_POSE(k_hessfix, m, grid, st, m, X, Sblk, V, W, HV, partials, g);
}
void launch_retract(hipStream_t st, const ManiDesc &m, Buf2 X, const double *V, double alpha, Buf2 out,
                    int selOut, Buf2 grad, const double *HV, double *partials, Gate g) {
  const int grid = pose_grid(m);
  DCORA_DISPATCH_POSE(k_retract, m, grid, st, m, X, V, alpha, out, selOut, grad, HV, partials, g);
}
void launch_polar(hipStream_t st, const ManiDesc &m, double c0, const double *A, double c1, const double *B,
                  double c2, const double *C, double *out) {
  const int grid = pose_grid(m);
  DCORA_DISPATCH_POSE(k_polar, m, grid, st, m, c0, A, c1, B, c2, C, out);
}
void launch_nesterov(hipStream_t st, const ManiDesc &m, int mode, int restart, int skip_lo, int skip_hi, double alpha,
                     double gamma, double *X, double *V, double *Y, double *XPrev, double *Yloc,
                     const double *Xloc) {
  NesterovArgs a{mode, restart, skip_lo, skip_hi, alpha, gamma, X, V, Y, XPrev, Yloc, Xloc};
  const int grid = pose_grid(m);
  DCORA_DISPATCH_POSE(k_nesterov, m, grid, st, m, a);
}
void launch_lambda_blocks(hipStream_t st, const ManiDesc &m, const double *X, const double *XQ, double *Lblk) {
  const int grid = pose_grid(m);
  DCORA_DISPATCH_POSE(k_lambda, m, grid, st, m, X, XQ, Lblk);
}

}  // namespace dcora
