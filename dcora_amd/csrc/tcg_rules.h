// The scalar rules of ROPTLIB's truncated CG (SolversTR::tCG_TR), stated once for every tCG kernel form: the generic
// launches (k_spmm_dir, k_spmm_dir_fix, k_tcg_update1, k_tcg_update2, k_tangent), the split launches (k_fused_hess,
// k_fused_hess_bsr, k_fused_precond, k_fused_finish), the pc launches (k_fused_hess*, k_fused_pc) and the one-launch
// run (k_tcg_run).  Device code only.
//
// The value functions take scalars that are already loaded and return scalars: the launch forms keep the recurrence in
// SolverCtl, k_tcg_run keeps it in registers for the whole run, and both compute it here.  The one-lane writers store
// into the control block; nothing here loads from it, so every kernel keeps its loads where it issues them (several
// request them before the gate, so that their latency overlaps).
#pragma once
#include "kernels.h"

namespace dcora {

// residual stopping rule |r| <= |r0| min(|r0|^theta, kappa)
constexpr double kTcgKappa = 0.1;
constexpr double kTcgTheta = 1.0;
static_assert(kTcgTheta == 1.0, "tcg_residual_done takes |r0|^theta as |r0|");

// ---- direction recurrence: the scalars of iteration i, kept in slot i & 1 of the control block -----------------
struct TcgDir {
  double z_r, e_Pd, d_Pd;  // <z, r>, <eta, P delta>, <delta, P delta>; <eta, P eta> is the step's e_Pe_new
};
// iteration 0: delta = -z, eta = 0 (so <eta, P delta> = <eta, P eta> = 0)
__device__ __forceinline__ TcgDir tcg_dir_start(double z_r) { return TcgDir{z_r, 0.0, z_r}; }
// iteration i + 1 from iteration i's d_Pd, e_Pd and step alpha: delta = -z + beta delta, beta = <z, r>_new / <z, r>_old
__device__ __forceinline__ double tcg_beta(double z_r_new, double z_r_old) { return z_r_new / z_r_old; }
__device__ __forceinline__ TcgDir tcg_dir_next(double z_r_new, double beta, double alpha, double d_Pd, double e_Pd) {
  return TcgDir{z_r_new, beta * (e_Pd + alpha * d_Pd), z_r_new + beta * beta * d_Pd};
}
// one lane: iteration `slot`'s scalars into the control block.  e_Pe is taken by reference so that a kernel that hands
// in ctl->e_Pe_n reads that word here, behind the other three stores.
__device__ __forceinline__ void tcg_put_dir(SolverCtl *ctl, int slot, const TcgDir &v, const double &e_Pe) {
  ctl->z_r[slot] = v.z_r;
  ctl->e_Pd[slot] = v.e_Pd;
  ctl->d_Pd[slot] = v.d_Pd;
  ctl->e_Pe[slot] = e_Pe;
}

// ---- step length and trust-region boundary of one iteration ------------------------------------------------------
__device__ __forceinline__ double tcg_alpha(double z_r, double d_Hd) { return z_r / d_Hd; }
// <eta + alpha delta, P (eta + alpha delta)>
__device__ __forceinline__ double tcg_e_Pe_new(double alpha, double d_Pd, double e_Pe, double e_Pd) {
  return e_Pe + 2.0 * alpha * e_Pd + alpha * alpha * d_Pd;
}
// negative curvature, or the CG step leaves the trust region: the run ends with the step tcg_tau
__device__ __forceinline__ bool tcg_boundary(double d_Hd, double e_Pe_new, double Delta) {
  return (d_Hd <= 0) || (e_Pe_new >= Delta * Delta);
}
// the step tau >= 0 along delta that reaches the trust-region boundary: |eta + tau delta|_P = Delta
__device__ __forceinline__ double tcg_tau(double d_Pd, double e_Pe, double e_Pd, double Delta) {
  return (-e_Pd + sqrt(e_Pd * e_Pd + d_Pd * (Delta * Delta - e_Pe))) / d_Pd;
}
__device__ __forceinline__ int tcg_boundary_status(double d_Hd) { return d_Hd <= 0 ? TR_NEGCURVTURE : TR_EXCREGION; }

// ---- residual stopping rule ------------------------------------------------------------------------------------
__device__ __forceinline__ bool tcg_residual_done(double norm_r, double norm_r0) {
  return norm_r <= norm_r0 * fmin(norm_r0, kTcgKappa);
}
__device__ __forceinline__ int tcg_residual_status(double norm_r0) { return kTcgKappa < norm_r0 ? TR_LCON : TR_SCON; }

// ---- one-lane control-block writes ---------------------------------------------------------------------------
// the start of a run: |r0| = |grad|, status TR_MAXITER until a rule ends the run, the tCG gate open
__device__ __forceinline__ void tcg_begin_run(SolverCtl *ctl, double norm_r0) {
  ctl->norm_r0 = norm_r0;
  ctl->tcg_status = TR_MAXITER;
  ctl->tcg_iters = 0;
  ctl->tcg_done_stamp = INT_MAX;
}
// the end of a run after `iters` iterations, in launch `seq`: at the iteration cap the status stays TR_MAXITER
__device__ __forceinline__ void tcg_end_run_at_cap(SolverCtl *ctl, HostFlags *hf, int seq, int iters) {
  ctl->tcg_iters = iters;
  ctl->inner_total += iters;
  ctl->tcg_done_stamp = seq;
  host_store(&hf->tcg_done_seq, seq);
}
__device__ __forceinline__ void tcg_end_run(SolverCtl *ctl, HostFlags *hf, int seq, int status, int iters) {
  ctl->tcg_status = status;
  tcg_end_run_at_cap(ctl, hf, seq, iters);
}

// the start of a solve: every word but the evaluation's (f1, ngf, fInit, gradNormInit, written by k_rtr_init)
__device__ __forceinline__ void ctl_arm(SolverCtl *c, const CtlInit &ci) {
  c->f2 = c->rho = 0;
  c->Delta = ci.Delta;
  c->maxDelta = ci.maxDelta;
  c->tol = ci.tol;
  c->cur = 0;
  c->outer_it = 0;
  c->max_outer = ci.max_outer;
  c->accepted = 0;
  c->last_accepted = 0;
  c->stop_on_accept = ci.stop_on_accept;
  c->outer_done_stamp = INT_MAX;
  c->alpha = c->e_Pe_n = c->norm_r0 = 0;
  c->tcg_done_stamp = INT_MAX;
  c->tcg_status = TR_MAXITER;
  c->tcg_iters = 0;
  c->inner_total = 0;
  c->max_inner = ci.max_inner;
}

}  // namespace dcora
