// extern "C" surface of libdcora_hip.so (declared in include/dcora_hip.h).  Every entry point with a failure path runs
// its body through abi_call (host_threads.h): NULL required pointers and exceptions end there, never across the ABI.
#include <cstdio>
#include <cstring>
#include <new>

#include "../../include/dcora_hip.h"
#include "cert.h"
#include "column_slots.h"
#include "device_chol.h"
#include "device_problem.h"
#include "host_graph.h"
#include "host_threads.h"
#include "ra_rbcd.h"
#include "rbcd.h"
#include "precond_cache.h"
#include "exchange.h"
#include "host_robust.h"
#include "robust.h"
#include "round.h"

namespace dcora {
const std::string &get_last_error();
}
using namespace dcora;

struct dcora_problem_s {
  DeviceProblem p;
};
struct dcora_csr_s {
  HostCsr m;
};
struct dcora_dataset_s {
  HostDataset ds;
};
struct dcora_rbcd_s {
  RbcdSession s;
  std::vector<int> sel_trace;
};
struct dcora_exchange_s {
  Exchange e;
  bool ranked = false;  // created with its robust session (dcora_rbcd_ / dcora_ra_rbcd_create_robust_ranks)
};

namespace {
HostCsr view_csr(int n, const int *rp, const int *ci, const double *v) {
  HostCsr A;
  A.n = n;
  A.ncols = n;
  A.rp.assign(rp, rp + n + 1);
  A.ci.assign(ci, ci + rp[n]);
  A.v.assign(v, v + rp[n]);
  return A;
}
std::vector<PoseMeas> view_meas(int d, int m, const int *ids, const double *vals) {
  const int stride = d * d + d + 3;
  std::vector<PoseMeas> out(m);
  for (int k = 0; k < m; ++k) {
    PoseMeas &e = out[k];
    e.r1 = ids[4 * k];
    e.p1 = ids[4 * k + 1];
    e.r2 = ids[4 * k + 2];
    e.p2 = ids[4 * k + 3];
    const double *q = vals + (size_t)k * stride;
    for (int i = 0; i < d * d; ++i) e.R[i] = q[i];
    for (int i = 0; i < d; ++i) e.t[i] = q[d * d + i];
    e.kappa = q[d * d + d];
    e.tau = q[d * d + d + 1];
    e.weight = q[d * d + d + 2];
  }
  return out;
}
int bad(const std::string &msg) {
  set_last_error(msg);
  return DCORA_ERR_BAD_ARG;
}
// DCORA_LAYOUT_SE names a pose graph: it cannot hold unit spheres or landmarks
bool layout_ok(const dcora_dims *dims) {
  return dims->layout >= DCORA_LAYOUT_AUTO && dims->layout <= DCORA_LAYOUT_RA &&
         !(dims->layout == DCORA_LAYOUT_SE && (dims->l != 0 || dims->b != 0));
}
int no_device() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) return DCORA_OK;
  set_last_error("no HIP device available: libdcora_hip has no CPU fallback");
  return DCORA_ERR_NO_DEVICE;
}
// a handle's result in *out, or the handle dropped when `init` fails
template <class H, class Init>
int create(H **out, Init &&init) {
  std::unique_ptr<H> h(new H);
  const int rc = init(*h);
  if (rc) return rc;
  *out = h.release();
  return DCORA_OK;
}
// dcora_rbcd_run / dcora_ra_rbcd_run: passes until |rgrad| < rgrad_tol, at most max_iters
template <class Session>
int run_passes(Session &s, int max_iters, double rgrad_tol, int *iters_done, double *cost2_trace,
               double *gradnorm_trace, int *selected_trace) {
  int selected = 0, it = 0;
  for (; it < max_iters; ++it) {
    double c2 = 0, gn = 0;
    int nxt = selected;
    const int rc = s.iterate(selected, &c2, &gn, nullptr, &nxt);
    if (rc) return rc;
    if (cost2_trace) cost2_trace[it] = c2;
    if (gradnorm_trace) gradnorm_trace[it] = gn;
    if (selected_trace) selected_trace[it] = selected;
    if (gn < rgrad_tol) {
      ++it;
      break;
    }
    selected = nxt;
  }
  if (iters_done) *iters_done = it;
  return DCORA_OK;
}
// dcora_rbcd_run_coloured / dcora_ra_rbcd_run_coloured: sweeps of one tick per colour, each followed by the session's
// central evaluation
template <class Session>
int run_coloured(Session &s, int max_sweeps, double rgrad_tol, int *sweeps_done, double *cost2_trace,
                 double *gradnorm_trace) {
  std::vector<int> colours((size_t)s.R, 0);
  int nc = 0;
  const int rc = s.agent_colours(colours.data(), &nc);
  if (rc) return rc;
  return run_coloured_sweeps(
      colours, nc, [&](const int *set, int count) { return s.iterate_set(set, count, 0); },
      [&](double *c2, double *gn) { return s.evaluate(c2, gn, nullptr, nullptr); }, max_sweeps, rgrad_tol, sweeps_done,
      cost2_trace, gradnorm_trace);
}

// ---- robust and team sessions of either kind: the messages name the kind by the session's tag ("rbcd" / "ra_rbcd"),
// which is also the middle of its entries' names (dcora_<tag>_...)
std::string robust_tag(const SessionCore &s) { return std::string(s.tag()) + " robust: "; }
// dcora_rbcd_create_robust / dcora_ra_rbcd_create_robust (H: the handle, ds: the kind's dataset handle)
template <class H, class Dataset>
int create_robust(Dataset ds, const dcora_rbcd_options *opt, const dcora_robust_params *robust, const int *fixed_weight,
                  H **out) {
  return create(out, [&](H &h) -> int {
    if (opt->world_size != 1) {
      const std::string entry = std::string("dcora_") + h.s.tag() + "_create_robust";
      set_last_error(robust_tag(h.s) + entry + " makes single-process sessions (world_size 1); a multi-rank job "
                     "creates its sessions with " + entry + "_ranks");
      return DCORA_ERR_UNSUPPORTED;
    }
    return h.s.init_robust(ds->ds, *opt, *robust, fixed_weight);
  });
}
// the robust session of one rank and its exchange, created together (weight updates are collective), with room for the
// ranks to come (SessionCore::reserve_rank between the two)
template <class H, class Dataset>
int create_robust_ranks(Dataset ds, const dcora_rbcd_options *opt, const dcora_robust_params *robust,
                        const int *fixed_weight, int r_reserve, const char *job_name, H **session,
                        dcora_exchange_t *ex) {
  std::unique_ptr<H> h(new H);  // (destroyed on every failure below)
  if (reserve_rank_check(ds->ds.d, opt->r, r_reserve, true))
    return bad(robust_tag(h->s) + "r_reserve is 0 (no reserve) or d <= r <= r_reserve <= 16");
  int rc = h->s.init_robust(ds->ds, *opt, *robust, fixed_weight, true);
  if (rc) return rc;
  if (r_reserve && (rc = h->s.reserve_rank(r_reserve))) return rc;
  std::unique_ptr<dcora_exchange_s> x(new dcora_exchange_s);
  rc = x->e.init(&h->s, job_name, h->s.weights_count());
  if (rc) return rc;
  rc = x->e.publish_weights();
  if (rc) return rc;
  x->ranked = true;
  *session = h.release();
  *ex = x.release();
  return DCORA_OK;
}
// the robust entries' refusals: multi-process sessions first, then sessions without robust state
int robust_session(const SessionCore &s) {
  if (s.robust) return DCORA_OK;
  if (s.opt.world_size != 1) {
    set_last_error(robust_tag(s) + "only single-process sessions (world_size 1) update weights");
    return DCORA_ERR_UNSUPPORTED;
  }
  return bad(robust_tag(s) + "the session was not created by dcora_" + s.tag() + "_create_robust");
}
// ... and the session-level weight changes, which are not collective, on a session of a _create_robust_ranks entry
int local_robust_session(const SessionCore &s, const char *collective) {
  const int rc = robust_session(s);
  if (rc || !s.robust->ranked) return rc;
  set_last_error(robust_tag(s) + "the session belongs to a multi-rank job (dcora_" + s.tag() +
                 "_create_robust_ranks): its weights change through " + collective);
  return DCORA_ERR_UNSUPPORTED;
}
int robust_info(const SessionCore &s, double *mu, int *updates) {
  const int rc = robust_session(s);
  if (rc) return rc;
  if (mu) *mu = s.robust->cost.mu();
  if (updates) *updates = s.robust->updates;
  return DCORA_OK;
}
int team_session(const SessionCore &s) {
  return s.team ? (int)DCORA_OK
                : bad(std::string(s.tag()) + " team: the session has not called dcora_" + s.tag() + "_team_enable");
}
}  // namespace

extern "C" {

const char *dcora_status_string(int s) {
  switch (s) {
    case DCORA_OK: return "ok";
    case DCORA_ERR_BAD_ARG: return "bad argument";
    case DCORA_ERR_NO_DEVICE: return "no HIP device (no CPU fallback)";
    case DCORA_ERR_HIP: return "HIP runtime error";
    case DCORA_ERR_NOT_PD: return "matrix not positive definite";
    case DCORA_ERR_NO_CONVERGENCE: return "eigensolver did not converge";
    case DCORA_ERR_NO_PRECONDITIONER: return "preconditioner missing";
    case DCORA_ERR_IO: return "I/O error";
    case DCORA_ERR_UNSUPPORTED: return "unsupported configuration";
  }
  return "unknown";
}
const char *dcora_last_error(void) { return get_last_error().c_str(); }
int dcora_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void dcora_ropt_params_default(dcora_ropt_params *p) {
  if (!p) return;
  p->method = 0;
  p->verbose = 0;
  p->gradnorm_tol = 1e-2;
  p->RGD_stepsize = 1e-3;
  p->RGD_use_preconditioner = 1;
  p->RTR_iterations = 3;
  p->RTR_tCG_iterations = 50;
  p->RTR_initial_radius = 100;
}

// ---- problem ----------------------------------------------------------------------------------------------
int dcora_problem_create(const dcora_dims *dims, const int *rowptr, const int *colidx, const double *vals,
                         const double *G, double precond_reg, int device, dcora_problem_t *out) {
  return abi_call({dims, rowptr, colidx, vals, out}, [&]() -> int {
    if (!layout_ok(dims)) return bad("dims: layout SE needs l = b = 0");
    const int k = (dims->d + 1) * dims->n + dims->l + dims->b;
    return create(out, [&](dcora_problem_s &h) {
      return h.p.init(*dims, view_csr(k, rowptr, colidx, vals), G, precond_reg, device, nullptr);
    });
  });
}
int dcora_problem_destroy(dcora_problem_t p) {
  delete p;
  return DCORA_OK;
}
int dcora_problem_set_linear_term(dcora_problem_t p, const double *G) {
  return abi_call({p}, [&] { return p->p.set_G_host(G); });
}
int dcora_problem_cost(dcora_problem_t p, const double *X, double *f) {
  return abi_call({p, X, f}, [&] { return p->p.cost(X, f); });
}
int dcora_problem_eucgrad(dcora_problem_t p, const double *X, double *out) {
  return abi_call({p, X, out}, [&] { return p->p.eucgrad(X, out); });
}
int dcora_problem_riegrad(dcora_problem_t p, const double *X, double *out, double *norm) {
  return abi_call({p, X}, [&] { return p->p.riegrad(X, out, norm); });
}
int dcora_problem_hessvec(dcora_problem_t p, const double *X, const double *V, double *out) {
  return abi_call({p, X, V, out}, [&] { return p->p.hessvec(X, V, out); });
}
int dcora_debug_hessvec_solver_form(dcora_problem_t p, const double *X, const double *V, double *out, double *dots) {
  return abi_call({p, X, V, out, dots}, [&] { return p->p.hessvec_solver_form(X, V, out, dots); });
}
int dcora_problem_precondition(dcora_problem_t p, const double *X, const double *V, double *out) {
  return abi_call({p, X, V, out}, [&] { return p->p.precondition(X, V, out); });
}
int dcora_problem_retract(dcora_problem_t p, const double *X, const double *V, double *out) {
  return abi_call({p, X, V, out}, [&] { return p->p.retract(X, V, out); });
}
int dcora_problem_tangent_project(dcora_problem_t p, const double *X, const double *V, double *out) {
  return abi_call({p, X, V, out}, [&] { return p->p.tangent_project(X, V, out); });
}
int dcora_problem_escape_saddle(dcora_problem_t p, const double *Xopt, double theta, const double *v, double gtol,
                                double pgtol, int is_second_order, double *Xout, int *success) {
  return abi_call({p, Xopt, v, Xout, success}, [&] {
    return p->p.escape_saddle(Xopt, theta, v, gtol, pgtol, is_second_order != 0, Xout, success);
  });
}
int dcora_manifold_project(const dcora_dims *dims, const double *M, double *out, int device) {
  return abi_call({dims, M, out}, [&]() -> int {
    if (!layout_ok(dims)) return bad("dims: layout SE needs l = b = 0");
    if (no_device()) return DCORA_ERR_NO_DEVICE;
    DCORA_HIP(hipSetDevice(device));
    const ManiDesc m = make_mani(*dims);
    const size_t N = (size_t)m.r * m.k;
    DevBuf<double> a, b;
    DCORA_HIP(a.alloc(N));
    DCORA_HIP(b.alloc(N));
    DCORA_HIP(hipMemcpy(a.p, M, N * sizeof(double), hipMemcpyHostToDevice));
    launch_polar(nullptr, m, 1.0, a.p, 0.0, nullptr, 0.0, nullptr, b.p);
    DCORA_HIP(hipDeviceSynchronize());
    DCORA_HIP(hipMemcpy(out, b.p, N * sizeof(double), hipMemcpyDeviceToHost));
    return DCORA_OK;
  });
}
int dcora_optimizer_optimize(dcora_problem_t p, const dcora_ropt_params *params, const double *X0, double *Xout,
                             dcora_ropt_result *result) {
  return abi_call({p, params, X0, Xout}, [&] { return p->p.optimize(*params, X0, Xout, result); });
}
int dcora_problem_time_qapply(dcora_problem_t p, int reps, double *avg_ms, double *bytes) {
  return abi_call({p, avg_ms, bytes}, [&] { return p->p.time_qapply(reps, avg_ms, bytes); });
}

// the Q-apply of `count` problems in turn on one stream: with distinct (Q, X, Y) sets whose bytes add up to more than
// the 256 MiB Infinity Cache every launch streams from HBM
int dcora_problem_time_qapply_rotating(const dcora_problem_t *ps, int count, int reps, double *avg_ms) {
  return abi_call({ps, avg_ms}, [&]() -> int {
    if (count < 1) return bad("null");
    for (int i = 0; i < count; ++i)
      if (!ps[i]) return bad("null problem");
    DeviceProblem &P0 = ps[0]->p;
    DCORA_HIP(hipSetDevice(P0.device));
    std::vector<hipStream_t> keep(count);
    for (int i = 0; i < count; ++i) {
      DCORA_HIP(hipStreamSynchronize(ps[i]->p.st));
      keep[i] = ps[i]->p.st;
      ps[i]->p.st = P0.st;
    }
    hipEvent_t e0, e1;
    DCORA_HIP(hipEventCreate(&e0));
    DCORA_HIP(hipEventCreate(&e1));
    for (int i = 0; i < count; ++i) ps[i]->p.enqueue_egrad(ps[i]->p.X0.p, ps[i]->p.EG0.p, nullptr);
    DCORA_HIP(hipEventRecord(e0, P0.st));
    for (int i = 0; i < reps; ++i) {
      DeviceProblem &P = ps[i % count]->p;
      P.enqueue_egrad(P.X0.p, P.EG0.p, nullptr);
    }
    DCORA_HIP(hipEventRecord(e1, P0.st));
    DCORA_HIP(hipEventSynchronize(e1));
    float ms = 0;
    DCORA_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    for (int i = 0; i < count; ++i) ps[i]->p.st = keep[i];
    *avg_ms = (double)ms / reps;
    return DCORA_OK;
  });
}
int dcora_problem_qapply_info(dcora_problem_t p, double *info) {
  return abi_call({p, info}, [&]() -> int {
    const DeviceProblem &P = p->p;
    info[0] = P.has_bsr ? 1 : 0;
    info[1] = (double)P.Q.nnz;
    info[2] = P.has_bsr ? (double)P.Qb.nblocks : 0.0;
    // bytes of the matrix in the form the kernel reads
    info[3] = P.has_bsr ? P.Qb.nblocks * (8.0 * (P.m.d + 1) * (P.m.d + 1) + 4.0) + 4.0 * (P.m.n + 1)
                        : 12.0 * P.Q.nnz + 4.0 * (P.m.k + 1);
    return DCORA_OK;
  });
}

// how the dense tCG iteration runs on this problem: info[0] = 0 three launches or the sparse preconditioner, 1 = A + (B and C
// in one launch), 2 = the whole tCG run in ONE launch (k_tcg_run; falls back to 1 for good after a run that gave up)
int dcora_problem_solver_info(dcora_problem_t p, double *info) {
  return abi_call({p, info}, [&]() -> int {
    const DeviceProblem &P = p->p;
    info[0] = !P.use_pc() ? 0 : (P.tcg_run_ok ? 2 : 1);
    return DCORA_OK;
  });
}
// the column-slot map the one-launch run gathers by: info[0] = 1 a map was built for this problem, info[1] its workgroups,
// info[2] those that overflow, info[3] the most pose blocks a workgroup names, info[4] = 1 the run form applies and fetches columns
// once per workgroup (a map without overflow), 0: every row gathers its entries' columns, or there is no run form
int dcora_problem_gather_info(dcora_problem_t p, double *info) {
  return abi_call({p, info}, [&]() -> int {
    const DeviceProblem &P = p->p;
    info[0] = P.run_cols.p ? 1 : 0;
    info[1] = P.run_cols_nwg;
    info[2] = P.run_cols_overflow;
    info[3] = P.run_cols_max;
    info[4] = P.run_cols_used() && P.tcg_run_ok ? 1 : 0;
    return DCORA_OK;
  });
}
int dcora_debug_problem_rerank(dcora_problem_t p, int r_new) {
  return abi_call({p}, [&] { return p->p.rerank(r_new); });
}
int dcora_debug_column_slots(const int *rowptr, const int *colidx, int n, int dh, int pb, int cap_cols, int list_cap,
                             int *lp, int *list, int *count, int *overflow, int *slot) {
  return abi_call({rowptr, colidx, lp, list, count, overflow, slot}, [&]() -> int {
    if (n < 1 || dh < 1 || pb < 1 || cap_cols < dh) return bad("dcora_debug_column_slots: n, dh, pb >= 1 and cap_cols >= dh");
    const ColumnSlots cs = column_slots(rowptr, colidx, n, dh, pb, cap_cols);
    if ((int)cs.list.size() > list_cap) return bad("dcora_debug_column_slots: list_cap is too small");
    std::copy(cs.lp.begin(), cs.lp.end(), lp);
    std::copy(cs.list.begin(), cs.list.end(), list);
    std::copy(cs.count.begin(), cs.count.end(), count);
    for (int w = 0; w < cs.nwg; ++w) overflow[w] = cs.overflow[(size_t)w];
    for (size_t i = 0; i < cs.slot.size(); ++i) slot[i] = cs.slot[i];
    return DCORA_OK;
  });
}
int dcora_debug_tcg_run_fault(int runs) {
  g_tcg_run_fault_skip.store(0);
  g_tcg_run_fault.store(runs < 0 ? 0 : runs);
  return DCORA_OK;
}
int dcora_debug_tcg_run_fault_at(int skip, int runs) {
  g_tcg_run_fault_skip.store(skip < 0 ? 0 : skip);
  g_tcg_run_fault.store(runs < 0 ? 0 : runs);
  return DCORA_OK;
}
int dcora_debug_wg_sums(int nv, const double *in, double *out) {
  return abi_call({in, out}, [&]() -> int {
    if (no_device()) return DCORA_ERR_NO_DEVICE;
    if (nv != 33 && nv != 41 && nv != 49) return bad("dcora_debug_wg_sums: nv is 33, 41 or 49 (8 r + 1 at r = 4, 5, 6)");
    const size_t nin = (size_t)nv * 256, nout = (size_t)2 * nv * 17;
    DevBuf<double> I, O;
    DCORA_HIP(I.alloc(nin));
    DCORA_HIP(O.alloc(nout));
    DCORA_HIP(hipMemcpy(I.p, in, nin * sizeof(double), hipMemcpyHostToDevice));
    DCORA_HIP(hipMemset(O.p, 0, nout * sizeof(double)));
    if (launch_debug_wg_sums(nullptr, nv, I.p, O.p) < 0) return bad("dcora_debug_wg_sums: the launch failed");
    DCORA_HIP(hipDeviceSynchronize());
    DCORA_HIP(hipMemcpy(out, O.p, nout * sizeof(double), hipMemcpyDeviceToHost));
    return DCORA_OK;
  });
}
// the 8-lanes-per-pose retraction and both Nesterov kernels on host arrays (tests/test_group_factors_gpu.py)
int dcora_debug_group_retract(int r, int d, int n, const double *X, const double *V, double alpha, const double *grad,
                              const double *HV, double *out, double *partials_out, int *npartials_out) {
  return abi_call({X, V, out, partials_out, npartials_out}, [&]() -> int {
    if (no_device()) return DCORA_ERR_NO_DEVICE;
    if ((d != 2 && d != 3) || r < d || n < 1) return bad("dcora_debug_group_retract: d is 2 or 3, r >= d, n >= 1");
    if ((grad == nullptr) != (HV == nullptr)) return bad("dcora_debug_group_retract: grad and HV come together");
    const ManiDesc m = make_mani(r, d, n, 0, 0, 1);
    if (!group_supported(m)) return bad("dcora_debug_group_retract: the group kernels need the SE layout at r <= 8");
    const size_t nx = (size_t)r * (d + 1) * n, np = (size_t)2 * kMaxPartials;
    DevBuf<double> Xd, Vd, Gd, Hd, Od, Pd;
    for (DevBuf<double> *b : {&Xd, &Vd, &Od}) DCORA_HIP(b->alloc(nx));
    DCORA_HIP(hipMemcpy(Xd.p, X, sizeof(double) * nx, hipMemcpyHostToDevice));
    DCORA_HIP(hipMemcpy(Vd.p, V, sizeof(double) * nx, hipMemcpyHostToDevice));
    DCORA_HIP(hipMemset(Od.p, 0xff, sizeof(double) * nx));  // (NaN where the kernel must write)
    if (grad) {
      for (DevBuf<double> *b : {&Gd, &Hd}) DCORA_HIP(b->alloc(nx));
      DCORA_HIP(Pd.alloc(np));
      DCORA_HIP(hipMemcpy(Gd.p, grad, sizeof(double) * nx, hipMemcpyHostToDevice));
      DCORA_HIP(hipMemcpy(Hd.p, HV, sizeof(double) * nx, hipMemcpyHostToDevice));
      DCORA_HIP(hipMemset(Pd.p, 0xff, sizeof(double) * np));
    }
    const int grid = launch_g_retract(nullptr, m, buf1(Xd.p), Vd.p, alpha, buf1(Od.p), 0, buf1(Gd.p), Hd.p, Pd.p, Gate{});
    DCORA_HIP(hipGetLastError());
    DCORA_HIP(hipDeviceSynchronize());
    DCORA_HIP(hipMemcpy(out, Od.p, sizeof(double) * nx, hipMemcpyDeviceToHost));
    if (grad) DCORA_HIP(hipMemcpy(partials_out, Pd.p, sizeof(double) * 2 * grid, hipMemcpyDeviceToHost));
    *npartials_out = grad ? grid : 0;
    return DCORA_OK;
  });
}
int dcora_debug_nesterov(int form, int r, int d, int n, int mode, int restart_bits, int skip_lo, int skip_hi,
                         double alpha, double gamma, double *X, double *V, double *Y, double *XPrev, double *Yloc,
                         const double *Xloc0, const double *Xloc1, int cur, double *inner_Yloc) {
  return abi_call({X, V, Y, XPrev, Yloc, Xloc0, Xloc1}, [&]() -> int {
    if (no_device()) return DCORA_ERR_NO_DEVICE;
    if ((d != 2 && d != 3) || r < d || r > kMaxRank || n < 1 || mode < 0 || mode > 3)
      return bad("dcora_debug_nesterov: d is 2 or 3, d <= r <= 16, n >= 1, mode is 0 .. 3");
    if (form != 0 && form != 1) return bad("dcora_debug_nesterov: form is 0 (k_nesterov) or 1 (k_g_nesterov)");
    const ManiDesc m = make_mani(r, d, n, 0, 0, 1);
    if (form == 1 && !group_supported(m)) return bad("dcora_debug_nesterov: form 1 needs the SE layout at r <= 8");
    if (form == 1 && (cur < -1 || cur > 1)) return bad("dcora_debug_nesterov: cur is 0, 1 or -1 (no control block)");
    if (form == 0 && inner_Yloc) return bad("dcora_debug_nesterov: form 0 has no inner_Yloc");
    if (inner_Yloc && (skip_lo < 0 || skip_hi < skip_lo || skip_hi > n))
      return bad("dcora_debug_nesterov: inner_Yloc holds the poses [skip_lo, skip_hi) of the n");
    const size_t nx = (size_t)r * (d + 1) * n, ni = inner_Yloc ? (size_t)r * (d + 1) * (skip_hi - skip_lo) : 0;
    double *state[5] = {X, V, Y, XPrev, Yloc};
    DevBuf<double> S[5], L[2], I;
    DevBuf<SolverCtl> ctl;
    for (int i = 0; i < 5; ++i) {
      DCORA_HIP(S[i].alloc(nx));
      DCORA_HIP(hipMemcpy(S[i].p, state[i], sizeof(double) * nx, hipMemcpyHostToDevice));
    }
    for (int i = 0; i < 2; ++i) {
      DCORA_HIP(L[i].alloc(nx));
      DCORA_HIP(hipMemcpy(L[i].p, i ? Xloc1 : Xloc0, sizeof(double) * nx, hipMemcpyHostToDevice));
    }
    if (ni) {
      DCORA_HIP(I.alloc(ni));
      DCORA_HIP(hipMemcpy(I.p, inner_Yloc, sizeof(double) * ni, hipMemcpyHostToDevice));
    }
    if (form == 1 && cur >= 0) {
      SolverCtl c{};
      c.cur = cur;
      DCORA_HIP(ctl.alloc(1));
      DCORA_HIP(hipMemcpy(ctl.p, &c, sizeof(c), hipMemcpyHostToDevice));
    }
    if (form == 1)
      launch_g_nesterov(nullptr, m, mode, restart_bits, skip_lo, skip_hi, alpha, gamma, S[0].p, S[1].p, S[2].p, S[3].p,
                        S[4].p, Buf2{{L[0].p, L[1].p}}, ctl.p, ni ? I.p : nullptr);
    else  // as rbcd.hip calls it
      launch_nesterov(nullptr, m, mode, restart_bits & 1, skip_lo, skip_hi, alpha, gamma, S[0].p, S[1].p, S[2].p, S[3].p,
                      S[4].p, L[0].p);
    DCORA_HIP(hipGetLastError());
    DCORA_HIP(hipDeviceSynchronize());
    for (int i = 0; i < 5; ++i) DCORA_HIP(hipMemcpy(state[i], S[i].p, sizeof(double) * nx, hipMemcpyDeviceToHost));
    if (ni) DCORA_HIP(hipMemcpy(inner_Yloc, I.p, sizeof(double) * ni, hipMemcpyDeviceToHost));
    return DCORA_OK;
  });
}
int dcora_debug_run_image(int r, int k, int *off, int *lanes, int *bytes) {
  return abi_call({off, lanes, bytes}, [&]() -> int {
    const int b = tcg_run_image_map(r, k, off, lanes);
    if (b < 0) return bad("dcora_debug_run_image: r is 4, 5 or 6 and 1 <= k <= 2048");
    *bytes = b;
    return DCORA_OK;
  });
}
int dcora_problem_time_precond(dcora_problem_t p, int reps, double *avg_ms, double *bytes) {
  return abi_call({p, avg_ms, bytes}, [&] { return p->p.time_precond(reps, avg_ms, bytes); });
}
int dcora_problem_precond_info(dcora_problem_t p, double *info) {
  return abi_call({p, info}, [&]() -> int {
    const DeviceProblem &P = p->p;
    info[0] = !P.has_precond ? 0 : (P.sparse_precond ? 2 : 1);
    info[1] = !P.has_precond ? 0 : (P.sparse_precond ? P.sp.launches() : 1);
    info[2] = (double)P.precond_nnzL;
    info[3] = P.precond_setup_ms;
    info[4] = !P.has_precond ? 0 : (P.sparse_precond ? P.sp.weights_per_apply : (double)P.m.k * P.m.k);
    return DCORA_OK;
  });
}

// debug / test hook (not part of the public header): a digest of the stored weights of a problem's sparse
// preconditioner image, read back from the device: {count, sum, sum of |w|, sum of w (i mod 97 + 1)} -- the last one
// moves when a weight lands in another place.  Compares the ways the weights can be formed (device fill, streamed host
// fill, one-piece upload).
int dcora_debug_sparse_weights_digest(dcora_problem_t p, double *out4) {
  return abi_call({p, out4}, [&]() -> int {
    const DeviceProblem &P = p->p;
    if (!P.sparse_precond || !P.sp.im) return bad("the problem has no sparse preconditioner");
    const DevBuf<double> &v = P.sp.im->vals;
    std::vector<double> h(v.n);
    DCORA_HIP(hipSetDevice(P.device));
    DCORA_HIP(hipMemcpy(h.data(), v.p, v.n * sizeof(double), hipMemcpyDeviceToHost));
    long double s0 = 0, s1 = 0, s2 = 0;
    for (size_t i = 0; i < h.size(); ++i) {
      s0 += h[i];
      s1 += std::fabs(h[i]);
      s2 += h[i] * (double)(i % 97 + 1);
    }
    out4[0] = (double)h.size();
    out4[1] = (double)s0;
    out4[2] = (double)s1;
    out4[3] = (double)s2;
    return DCORA_OK;
  });
}

}  // extern "C"

// A CERTIFIED lower bound of the smallest eigenvalue of a matrix the PSD test has accepted.  Lanczos (full
// re-orthogonalisation) on M^-1, M = S + eta I, through the sparse Cholesky factor the test computes (host), gives a
// Ritz value theta <= theta_max(M^-1) -- so 1 / theta - eta errs UPWARD and is only an estimate.  The candidate bound
// 1 / (theta + |beta_m s_m|) - eta (Ritz residual added) is then VERIFIED the way the certificate itself is
// (ref src/DCORA_utils.cpp:1737-1747): S - lambda I must have a Cholesky factorisation.  What is returned is the
// verified shift; when the verification fails the only certified figure, -eta, is returned.
namespace {
// largest eigenvalue of the symmetric tridiagonal (a, b) of order m by bisection on the Sturm count
double tridiag_largest(const std::vector<double> &a, const std::vector<double> &b, int m) {
  double lo = a[0], hi = a[0];
  for (int i = 0; i < m; ++i) {
    const double rad = (i > 0 ? std::fabs(b[i - 1]) : 0.0) + (i + 1 < m ? std::fabs(b[i]) : 0.0);
    lo = std::min(lo, a[i] - rad);
    hi = std::max(hi, a[i] + rad);
  }
  auto count_below = [&](double x) {  // eigenvalues < x
    int c = 0;
    double d = a[0] - x;
    if (d < 0) ++c;
    for (int i = 1; i < m; ++i) {
      if (d == 0) d = 1e-300;
      d = a[i] - x - b[i - 1] * b[i - 1] / d;
      if (d < 0) ++c;
    }
    return c;
  };
  for (int it = 0; it < 200 && hi - lo > 1e-15 * std::max(std::fabs(hi), std::fabs(lo)); ++it) {
    const double mid = 0.5 * (lo + hi);
    if (count_below(mid) >= m) hi = mid; else lo = mid;
  }
  return 0.5 * (lo + hi);
}
int lambda_min_certified(int k, const int *rp, const int *ci, const double *v, double eta, int block,
                         int max_iterations, double *lambda_min, int *iterations) {
  const HostCsr S = view_csr(k, rp, ci, v);
  SparseChol chol;
  if (!chol.factor(csr_shift_diag(S, eta), block)) {
    set_last_error("lambda_min_certified: S + eta I is not positive definite (the certificate was not accepted)");
    return DCORA_ERR_NOT_PD;
  }
  const int mmax = std::max(2, std::min(max_iterations, k));
  std::vector<std::vector<double>> V;
  std::vector<double> alpha, beta, w((size_t)k);
  std::vector<double> q((size_t)k);
  uint64_t sdd = 0x9E3779B97F4A7C15ull;
  double n2 = 0;
  for (int i = 0; i < k; ++i) {
    sdd = sdd * 6364136223846793005ull + 1442695040888963407ull;
    q[i] = (double)(sdd >> 11) / 9007199254740992.0 - 0.5;
    n2 += q[i] * q[i];
  }
  for (double &t : q) t /= std::sqrt(n2);
  double lam = 0, prev = 1e300, th_last = 0, bn_last = 0;
  int j = 0;
  for (; j < mmax; ++j) {
    V.push_back(q);
    chol.solve_vec(q.data(), w.data());  // w = M^-1 q
    double a = 0;
    for (int i = 0; i < k; ++i) a += q[i] * w[i];
    alpha.push_back(a);
    for (int pass = 0; pass < 2; ++pass)  // full re-orthogonalisation, twice
      for (const std::vector<double> &u : V) {
        double c = 0;
        for (int i = 0; i < k; ++i) c += u[i] * w[i];
        for (int i = 0; i < k; ++i) w[i] -= c * u[i];
      }
    double bn = 0;
    for (int i = 0; i < k; ++i) bn += w[i] * w[i];
    bn = std::sqrt(bn);
    const int m = (int)alpha.size();
    const bool check = (m % 5 == 0) || bn < 1e-14 * std::fabs(a) || j + 1 == mmax;
    if (check) {
      const double th = tridiag_largest(alpha, beta, m);
      th_last = th;
      bn_last = bn;
      lam = 1.0 / th - eta;
      if (std::fabs(prev - lam) <= 1e-3 * std::fabs(lam) + 1e-15 || bn < 1e-14 * std::fabs(a)) {
        ++j;
        break;
      }
      prev = lam;
    }
    beta.push_back(bn);
    for (int i = 0; i < k; ++i) q[i] = w[i] / bn;
  }
  // Ritz residual |beta_m s_m|: s = eigenvector of the tridiagonal for th_last, by its three-term recurrence
  double resid = 0;
  {
    const int m = (int)alpha.size();
    std::vector<double> sv((size_t)m, 0.0);
    sv[0] = 1.0;
    double nrm = 1.0;
    for (int i = 0; i + 1 < m; ++i) {
      const double b = (i < (int)beta.size() && beta[i] != 0.0) ? beta[i] : 1e-300;
      double t = (th_last - alpha[i]) * sv[i];
      if (i > 0) t -= beta[i - 1] * sv[i - 1];
      sv[i + 1] = t / b;
      nrm += sv[i + 1] * sv[i + 1];
      if (nrm > 1e200) {  // rescale
        for (int u = 0; u <= i + 1; ++u) sv[u] *= 1e-100;
        nrm *= 1e-200;
      }
    }
    resid = std::fabs(bn_last * sv[m - 1]) / std::sqrt(nrm);
  }
  const double cand = 1.0 / (th_last + resid) - eta;
  // verification: S - shift I factors  <=>  lambda_min(S) > shift (up to the rounding of the factorisation)
  double shift = cand - 1e-3 * std::fabs(cand) - 1e-13;
  if (!(shift > -eta)) shift = -eta;
  double bound = -eta;
  if (shift > -eta) {
    SparseChol verify;
    if (verify.factor(csr_shift_diag(S, -shift), block)) bound = shift;
  }
  (void)lam;
  *lambda_min = bound;
  if (iterations) *iterations = j;
  return DCORA_OK;
}
}  // namespace

extern "C" {

int dcora_cert_lambda_min_certified(int k, const int *rp, const int *ci, const double *v, double eta, int block,
                                    int max_iterations, double *lambda_min, int *iterations) {
  return abi_call({rp, ci, v, lambda_min}, [&] {
    return lambda_min_certified(k, rp, ci, v, eta, block, max_iterations, lambda_min, iterations);
  });
}

int dcora_cert_suboptimality_gap(const dcora_dims *dims, const double *X, double lambda_lower_bound, double *gap,
                                 double *n_eff) {
  return abi_call({dims, X, gap}, [&]() -> int {
    if (!layout_ok(dims)) return bad("dims: layout SE needs l = b = 0");
    const ManiDesc m = make_mani(*dims);
    const int r = m.r;
    double rot = 0;
    for (int i = 0; i < m.n; ++i)
      for (int c = 0; c < m.d; ++c)
        for (int t = 0; t < r; ++t) {
          const double x = X[(size_t)(m.rot_col(i) + c) * r + t];
          rot += x * x;
        }
    for (int i = 0; i < m.l; ++i)
      for (int t = 0; t < r; ++t) {
        const double x = X[(size_t)m.sphere_col(i) * r + t];
        rot += x * x;
      }
    const int ne = m.num_euc();
    std::vector<double> mean((size_t)r, 0.0);
    for (int e = 0; e < ne; ++e)
      for (int t = 0; t < r; ++t) mean[t] += X[(size_t)m.euc_col(e) * r + t];
    for (int t = 0; t < r; ++t) mean[t] /= std::max(ne, 1);
    double euc = 0;
    for (int e = 0; e < ne; ++e)
      for (int t = 0; t < r; ++t) {
        const double x = X[(size_t)m.euc_col(e) * r + t] - mean[t];
        euc += x * x;
      }
    const double tr = rot + euc;
    if (n_eff) *n_eff = tr;
    *gap = 0.5 * std::max(0.0, -lambda_lower_bound) * tr;
    return DCORA_OK;
  });
}

int dcora_precond_cache_info(double *info4) {
  return abi_call({info4}, [&] {
    precond_cache_stats(info4);
    return DCORA_OK;
  });
}
int dcora_precond_cache_clear(void) {
  return abi_call({}, [&] {
    precond_cache_clear();
    return DCORA_OK;
  });
}

// ---- CSR handles --------------------------------------------------------------------------------------------
int dcora_csr_info(dcora_csr_t m, int *n, int *nnz) {
  return abi_call({m, n, nnz}, [&] {
    *n = m->m.n;
    *nnz = m->m.nnz();
    return DCORA_OK;
  });
}
int dcora_csr_copy(dcora_csr_t m, int *rp, int *ci, double *v) {
  return abi_call({m, rp, ci, v}, [&] {
    std::copy(m->m.rp.begin(), m->m.rp.end(), rp);
    std::copy(m->m.ci.begin(), m->m.ci.end(), ci);
    std::copy(m->m.v.begin(), m->m.v.end(), v);
    return DCORA_OK;
  });
}
int dcora_csr_destroy(dcora_csr_t m) {
  delete m;
  return DCORA_OK;
}

// ---- certification --------------------------------------------------------------------------------------------
int dcora_cert_dual_matrix(const dcora_dims *dims, const double *X, const int *rp, const int *ci, const double *v,
                           int device, dcora_csr_t *S) {
  return abi_call({dims, X, rp, ci, v, S}, [&]() -> int {
    if (!layout_ok(dims)) return bad("dims: layout SE needs l = b = 0");
    const int k = (dims->d + 1) * dims->n + dims->l + dims->b;
    return create(S, [&](dcora_csr_s &h) { return device_dual_certificate(*dims, X, view_csr(k, rp, ci, v), device, &h.m); });
  });
}
int dcora_cert_is_psd(int k, const int *rp, const int *ci, const double *v, int block, int *is_psd) {
  return abi_call({rp, ci, v, is_psd}, [&] {
    bool psd = false;
    const int rc = host_is_psd(view_csr(k, rp, ci, v), block, &psd);
    *is_psd = psd ? 1 : 0;
    return rc;
  });
}
int dcora_cert_prepare(const dcora_dims *dims, const int *rp, const int *ci, int block, int device) {
  return abi_call({dims, rp, ci}, [&]() -> int {
    if (!layout_ok(dims)) return bad("dims: layout SE needs l = b = 0");
    const ManiDesc m = make_mani(*dims);
    const int n = m.k;
    if (n <= 0) return bad("empty pattern");
    // the caller's pattern is read only after it has been checked: the library cannot see the length of rp
    if (rp[0] != 0) return bad("cert_prepare: rowptr[0] must be 0");
    for (int i = 0; i < n; ++i)
      if (rp[i + 1] < rp[i]) return bad("cert_prepare: rowptr decreases");
    for (int p = 0; p < rp[n]; ++p)
      if (ci[p] < 0 || ci[p] >= n) return bad("cert_prepare: column index out of range");
    // the pattern dcora_cert_dual_matrix will hand to the PSD test: Q's entries, the entries of Lambda (present in Q's
    // pattern unless an entry of Q is structurally zero), every diagonal
    std::vector<int> I, J;
    I.reserve((size_t)rp[n] + (size_t)m.n * m.d * m.d + m.l);
    J.reserve(I.capacity());
    for (int i = 0; i < n; ++i)
      for (int p = rp[i]; p < rp[i + 1]; ++p) {
        I.push_back(i);
        J.push_back(ci[p]);
      }
    lambda_entries(m, I, J);
    const std::vector<double> V(I.size(), 1.0);
    const HostCsr A = csr_shift_diag(csr_from_coo(n, n, I, J, V), 1.0);
    return device_chol_prepare(A, block < 1 ? 1 : block, device);
  });
}
int dcora_cert_is_psd_device(int k, const int *rp, const int *ci, const double *v, int block, int device, int *is_psd,
                             double *info8) {
  return abi_call({rp, ci, v, is_psd}, [&] {
    bool pd = false;
    const int rc = device_chol_is_pd(view_csr(k, rp, ci, v), block, device, &pd, info8);
    *is_psd = pd ? 1 : 0;
    return rc;
  });
}
int dcora_chol_host_selftest(int k, const int *rp, const int *ci, const double *v, int block, int *is_pd,
                             double *resid, double *info4) {
  return abi_call({rp, ci, v, is_pd}, [&]() -> int {
    if (k > 4096) {
      set_last_error("dcora_chol_host_selftest: dense check, k <= 4096");
      return DCORA_ERR_BAD_ARG;
    }
    const HostCsr A = view_csr(k, rp, ci, v);
    CholSymbolic S;
    chol_symbolic(A, block, &S);
    std::vector<double> F;
    const bool ok = chol_numeric_host(S, v, &F);
    *is_pd = ok ? 1 : 0;
    if (info4) {
      info4[0] = (double)S.pieces.size();
      info4[1] = (double)S.nlev;
      info4[2] = (double)S.arena;
      info4[3] = S.flops;
    }
    if (resid) *resid = 0;
    if (!ok || !resid) return DCORA_OK;
    std::vector<double> L((size_t)k * k, 0.0), M((size_t)k * k, 0.0);
    for (const CholPiece &P : S.pieces) {
      const long long f = (long long)P.c + P.m;
      for (int j = 0; j < P.c; ++j) {
        for (int i = j; i < P.c; ++i) L[(size_t)(P.c0 + i) * k + P.c0 + j] = F[(size_t)(P.off + i * f + j)];
        for (int a = 0; a < P.m; ++a)
          L[(size_t)S.rows[(size_t)P.rows_off + a] * k + P.c0 + j] = F[(size_t)(P.off + (P.c + a) * f + j)];
      }
    }
    for (int io = 0; io < k; ++io)
      for (int p = rp[io]; p < rp[io + 1]; ++p) M[(size_t)S.iperm[io] * k + S.iperm[ci[p]]] = v[p];
    double worst = 0;
    for (int i = 0; i < k; ++i)
      for (int j = 0; j <= i; ++j) {
        double s = 0;
        for (int l = 0; l <= j; ++l) s += L[(size_t)i * k + l] * L[(size_t)j * k + l];
        worst = std::max(worst, std::fabs(s - M[(size_t)i * k + j]));
      }
    *resid = worst;
    return DCORA_OK;
  });
}
int dcora_chol_cache_clear(void) {
  return abi_call({}, [&] {
    chol_cache_clear();
    return DCORA_OK;
  });
}
int dcora_cert_min_eig(int k, const int *rp, const int *ci, const double *v, int max_iterations, double tol, int ncv,
                       unsigned long long seed, int device, double *lambda_min, double *vec, long *num_matvecs) {
  return abi_call({rp, ci, v}, [&] {
    LanczosResult e;
    const int rc = device_min_eig(view_csr(k, rp, ci, v), max_iterations, tol, ncv, seed, device, &e);
    if (lambda_min) *lambda_min = e.lambda;
    if (vec && (int)e.v.size() == k) std::copy(e.v.begin(), e.v.end(), vec);
    if (num_matvecs) *num_matvecs = e.matvecs;
    return rc;
  });
}
int dcora_cert_fast_verification(int k, const int *rp, const int *ci, const double *v, double eta, int block,
                                 int device, int *is_psd, double *theta, double *x, double *lambda_min) {
  return abi_call({rp, ci, v, is_psd}, [&] {
    bool psd = false;
    std::vector<double> vec;
    double th = 0, lm = 0;
    long mv = 0;
    const int rc = device_fast_verification(view_csr(k, rp, ci, v), eta, block, device, &psd, &th, &vec, &lm, &mv);
    *is_psd = psd ? 1 : 0;
    if (!psd) {
      if (theta) *theta = th;
      if (lambda_min) *lambda_min = lm;
      if (x && (int)vec.size() == k) std::copy(vec.begin(), vec.end(), x);
    }
    return rc;
  });
}

// ---- data feed ------------------------------------------------------------------------------------------------
int dcora_dataset_load_g2o(const char *path, dcora_dataset_t *out) {
  return abi_call({path, out}, [&] {
    return create(out, [&](dcora_dataset_s &h) -> int {
      std::string err;
      if (load_g2o(path, h.ds, err)) return DCORA_OK;
      set_last_error(err);
      return DCORA_ERR_IO;
    });
  });
}
int dcora_dataset_create(int d, int n, int m, const int *ids, const double *vals, dcora_dataset_t *out) {
  return abi_call({out}, [&]() -> int {
    if ((d != 2 && d != 3) || n < 1 || m < 0) return bad("bad dataset shape");
    if (m > 0 && (!ids || !vals)) return bad("null argument");
    return create(out, [&](dcora_dataset_s &h) {
      h.ds.d = d;
      h.ds.n = n;
      h.ds.meas = view_meas(d, m, ids, vals);
      return DCORA_OK;
    });
  });
}
int dcora_dataset_info(dcora_dataset_t ds, int *d, int *n, int *m) {
  return abi_call({ds, d, n, m}, [&] {
    *d = ds->ds.d;
    *n = ds->ds.n;
    *m = (int)ds->ds.meas.size();
    return DCORA_OK;
  });
}
int dcora_dataset_copy(dcora_dataset_t h, int *ids, double *vals) {
  return abi_call({h, ids, vals}, [&] {
    const int d = h->ds.d, stride = d * d + d + 3;
    for (size_t k = 0; k < h->ds.meas.size(); ++k) {
      const PoseMeas &e = h->ds.meas[k];
      ids[4 * k] = e.r1;
      ids[4 * k + 1] = e.p1;
      ids[4 * k + 2] = e.r2;
      ids[4 * k + 3] = e.p2;
      double *q = vals + k * stride;
      for (int i = 0; i < d * d; ++i) q[i] = e.R[i];
      for (int i = 0; i < d; ++i) q[d * d + i] = e.t[i];
      q[d * d + d] = e.kappa;
      q[d * d + d + 1] = e.tau;
      q[d * d + d + 2] = e.weight;
    }
    return DCORA_OK;
  });
}
int dcora_dataset_destroy(dcora_dataset_t ds) {
  delete ds;
  return DCORA_OK;
}
int dcora_dataset_chordal_init(dcora_dataset_t ds, double *T) {
  return abi_call({ds, T}, [&]() -> int {
    std::vector<double> out;
    if (!chordal_initialization(ds->ds, out)) {
      set_last_error("chordal initialisation: reduced Laplacian not positive definite (disconnected graph?)");
      return DCORA_ERR_NOT_PD;
    }
    std::copy(out.begin(), out.end(), T);
    return DCORA_OK;
  });
}
int dcora_dataset_chordal_init_device(dcora_dataset_t ds, int device, double *T) {
  return abi_call({ds, T}, [&]() -> int {
    if (no_device()) return DCORA_ERR_NO_DEVICE;
    std::vector<double> out;
    if (!chordal_initialization(ds->ds, out, device_spd_solver(device))) {
      set_last_error("chordal initialisation: reduced Laplacian not positive definite (disconnected graph?)");
      return DCORA_ERR_NOT_PD;
    }
    std::copy(out.begin(), out.end(), T);
    return DCORA_OK;
  });
}
int dcora_graph_build_Q_pgo(int d, int n, int agent_id, int m, const int *ids, const double *vals, dcora_csr_t *Q) {
  return abi_call({Q}, [&]() -> int {
    if (m > 0 && (!ids || !vals)) return bad("null argument");
    return create(Q, [&](dcora_csr_s &h) {
      h.m = build_Q_pgo(d, n, agent_id, view_meas(d, m, ids, vals));
      return DCORA_OK;
    });
  });
}

// ---- range-aided SLAM data feed (centralised) -----------------------------------------------------------------------
struct dcora_radataset_s {
  HostRADataset ds;
};
int dcora_radataset_load_pyfg(const char *path, dcora_radataset_t *out) {
  return abi_call({path, out}, [&] {
    return create(out, [&](dcora_radataset_s &h) -> int {
      std::string err;
      if (load_pyfg(path, h.ds, err)) return DCORA_OK;
      set_last_error(err);
      return DCORA_ERR_IO;
    });
  });
}
// Graph::setMeasurements(const RelativeMeasurements &) of a range-aided graph (ref src/Graph.cpp:374-470): the three
// kinds of measurements as arrays, states numbered as the Graph numbers them (poses 0 .. n - 1, unit spheres 0 .. l - 1 --
// one per range measurement --, landmarks 0 .. b - 1); every state is owned by robot 0 (the centralised agent)
int dcora_radataset_create(int d, int n, int l, int b, int m_pp, const int *pp_ids, const double *pp_vals, int m_pl,
                           const int *pl_ids, const double *pl_vals, int m_rg, const int *rg_ids, const double *rg_vals,
                           const double *gt, dcora_radataset_t *out) {
  return abi_call({out}, [&]() -> int {
    if ((m_pp > 0 && (!pp_ids || !pp_vals)) || (m_pl > 0 && (!pl_ids || !pl_vals)) ||
        (m_rg > 0 && (!rg_ids || !rg_vals)))
      return bad("null argument");
    if ((d != 2 && d != 3) || n < 0 || l < 0 || b < 0 || m_pp < 0 || m_pl < 0 || m_rg < 0)
      return bad("bad dimensions");
    auto h = std::make_unique<dcora_radataset_s>();
    HostRADataset &ds = h->ds;
    ds.d = d;
    ds.n = n;
    ds.l = l;
    ds.b = b;
    const int w = d * d + d + 3;
    for (int i = 0; i < m_pp; ++i) {
      PoseMeas m;
      m.p1 = pp_ids[2 * i];
      m.p2 = pp_ids[2 * i + 1];
      if (m.p1 < 0 || m.p1 >= n || m.p2 < 0 || m.p2 >= n) return bad("pose-pose measurement: pose out of range");
      const double *v = pp_vals + (size_t)i * w;
      for (int c = 0; c < d; ++c)
        for (int a = 0; a < d; ++a) m.R[c * d + a] = v[c * d + a];
      for (int a = 0; a < d; ++a) m.t[a] = v[d * d + a];
      m.kappa = v[d * d + d];
      m.tau = v[d * d + d + 1];
      m.weight = v[d * d + d + 2];
      ds.pose_pose.push_back(m);
    }
    for (int i = 0; i < m_pl; ++i) {
      PoseLandmarkMeasH m;
      m.i = pl_ids[2 * i];
      m.j = pl_ids[2 * i + 1];
      if (m.i < 0 || m.i >= n || m.j < 0 || m.j >= b) return bad("pose-landmark measurement: state out of range");
      const double *v = pl_vals + (size_t)i * (d + 2);
      for (int a = 0; a < d; ++a) m.t[a] = v[a];
      m.tau = v[d];
      m.weight = v[d + 1];
      ds.pose_landmark.push_back(m);
    }
    for (int i = 0; i < m_rg; ++i) {
      RangeMeasH m;
      m.type1 = rg_ids[5 * i];
      m.i = rg_ids[5 * i + 1];
      m.type2 = rg_ids[5 * i + 2];
      m.j = rg_ids[5 * i + 3];
      m.l = rg_ids[5 * i + 4];
      const bool ok1 = m.type1 == 0 ? (m.i >= 0 && m.i < n) : (m.type1 == 1 && m.i >= 0 && m.i < b);
      const bool ok2 = m.type2 == 0 ? (m.j >= 0 && m.j < n) : (m.type2 == 1 && m.j >= 0 && m.j < b);
      if (!ok1 || !ok2 || m.l < 0 || m.l >= l) return bad("range measurement: state out of range");
      m.range = rg_vals[3 * i];
      m.precision = rg_vals[3 * i + 1];
      m.weight = rg_vals[3 * i + 2];
      ds.ranges.push_back(m);
    }
    ds.gt.assign((size_t)d * ds.k(), 0.0);
    if (gt) std::copy(gt, gt + (size_t)d * ds.k(), ds.gt.begin());
    ds.pose_robot.assign((size_t)n, 0);
    ds.sphere_robot.assign((size_t)l, 0);
    ds.landmark_robot.assign((size_t)b, 0);
    *out = h.release();
    return DCORA_OK;
  });
}
// the measurements of a dataset in the arrays dcora_radataset_create takes (sizes: dcora_radataset_info); any may be NULL
int dcora_radataset_copy(dcora_radataset_t h, int *pp_ids, double *pp_vals, int *pl_ids, double *pl_vals, int *rg_ids,
                         double *rg_vals) {
  return abi_call({h}, [&] {
    const HostRADataset &ds = h->ds;
    const int d = ds.d, w = d * d + d + 3;
    for (size_t i = 0; i < ds.pose_pose.size(); ++i) {
      const PoseMeas &m = ds.pose_pose[i];
      if (pp_ids) {
        pp_ids[2 * i] = m.p1;
        pp_ids[2 * i + 1] = m.p2;
      }
      if (pp_vals) {
        double *v = pp_vals + i * w;
        for (int c = 0; c < d * d; ++c) v[c] = m.R[c];
        for (int a = 0; a < d; ++a) v[d * d + a] = m.t[a];
        v[d * d + d] = m.kappa;
        v[d * d + d + 1] = m.tau;
        v[d * d + d + 2] = m.weight;
      }
    }
    for (size_t i = 0; i < ds.pose_landmark.size(); ++i) {
      const PoseLandmarkMeasH &m = ds.pose_landmark[i];
      if (pl_ids) {
        pl_ids[2 * i] = m.i;
        pl_ids[2 * i + 1] = m.j;
      }
      if (pl_vals) {
        double *v = pl_vals + i * (d + 2);
        for (int a = 0; a < d; ++a) v[a] = m.t[a];
        v[d] = m.tau;
        v[d + 1] = m.weight;
      }
    }
    for (size_t i = 0; i < ds.ranges.size(); ++i) {
      const RangeMeasH &m = ds.ranges[i];
      if (rg_ids) {
        rg_ids[5 * i] = m.type1;
        rg_ids[5 * i + 1] = m.i;
        rg_ids[5 * i + 2] = m.type2;
        rg_ids[5 * i + 3] = m.j;
        rg_ids[5 * i + 4] = m.l;
      }
      if (rg_vals) {
        rg_vals[3 * i] = m.range;
        rg_vals[3 * i + 1] = m.precision;
        rg_vals[3 * i + 2] = m.weight;
      }
    }
    return DCORA_OK;
  });
}
int dcora_radataset_info(dcora_radataset_t h, int *info) {
  return abi_call({h, info}, [&] {
    info[0] = h->ds.d;
    info[1] = h->ds.n;
    info[2] = h->ds.l;
    info[3] = h->ds.b;
    info[4] = (int)h->ds.pose_pose.size();
    info[5] = (int)h->ds.pose_landmark.size();
    info[6] = (int)h->ds.ranges.size();
    return DCORA_OK;
  });
}
int dcora_radataset_ground_truth(dcora_radataset_t h, double *gt) {
  return abi_call({h, gt}, [&] {
    std::copy(h->ds.gt.begin(), h->ds.gt.end(), gt);
    return DCORA_OK;
  });
}
int dcora_radataset_build_Q(dcora_radataset_t h, dcora_csr_t *Q) {
  return abi_call({h, Q}, [&] {
    return create(Q, [&](dcora_csr_s &c) {
      c.m = build_Q_ra(h->ds);
      return DCORA_OK;
    });
  });
}
int dcora_radataset_odometry_init(dcora_radataset_t h, unsigned long long seed, double *X0) {
  return abi_call({h, X0}, [&] {
    std::vector<double> x;
    ra_odometry_initialization(h->ds, seed, x);
    std::copy(x.begin(), x.end(), X0);
    return DCORA_OK;
  });
}
int dcora_radataset_ownership(dcora_radataset_t h, int *pose_robot, int *sphere_robot, int *landmark_robot) {
  return abi_call({h}, [&] {
    if (pose_robot) std::copy(h->ds.pose_robot.begin(), h->ds.pose_robot.end(), pose_robot);
    if (sphere_robot) std::copy(h->ds.sphere_robot.begin(), h->ds.sphere_robot.end(), sphere_robot);
    if (landmark_robot) std::copy(h->ds.landmark_robot.begin(), h->ds.landmark_robot.end(), landmark_robot);
    return DCORA_OK;
  });
}
int dcora_radataset_agent_columns(dcora_radataset_t h, int robot, int *dims3, int *own, int *k_a) {
  return abi_call({h, dims3, k_a}, [&] {
    std::vector<int> o;
    ra_agent_columns(h->ds, robot, dims3, o);
    *k_a = (int)o.size();
    if (own) std::copy(o.begin(), o.end(), own);
    return DCORA_OK;
  });
}
int dcora_radataset_agent_colours(dcora_radataset_t h, int *colours, int *ncolours) {
  return abi_call({h, colours}, [&] {
    std::vector<int> robots;
    std::vector<std::vector<int>> nbr;
    ra_agent_adjacency(h->ds, &robots, &nbr);
    const int nc = greedy_agent_colours((int)robots.size(),
                                        [&](int a) -> const std::vector<int> & { return nbr[(size_t)a]; }, colours);
    if (ncolours) *ncolours = nc;
    return DCORA_OK;
  });
}
int dcora_radataset_loop_closures(dcora_radataset_t h, int *mask) {
  return abi_call({h, mask}, [&] {
    ra_loop_closures(h->ds, mask);
    return DCORA_OK;
  });
}
// the host rule of a ranked robust session (ra_rank_edges): one flag per pose-pose measurement
int dcora_radataset_rank_edges(dcora_radataset_t h, int rank, int world_size, int *touches, int *owns) {
  return abi_call({h, touches, owns}, [&]() -> int {
    if (world_size < 1 || rank < 0 || rank >= world_size) return bad("rank_edges: bad rank / world_size");
    if (h->ds.pose_robot.size() != (size_t)h->ds.n) return bad("rank_edges: the dataset has no pose owners");
    for (const PoseMeas &q : h->ds.pose_pose)
      if (q.p1 < 0 || q.p1 >= h->ds.n || q.p2 < 0 || q.p2 >= h->ds.n) return bad("rank_edges: pose index out of range");
    std::vector<int> ids;
    std::vector<char> own;
    ra_rank_edges(h->ds, rank, world_size, &ids, &own);
    std::fill(touches, touches + h->ds.pose_pose.size(), 0);
    std::fill(owns, owns + h->ds.pose_pose.size(), 0);
    for (size_t i = 0; i < ids.size(); ++i) {
      touches[ids[i]] = 1;
      owns[ids[i]] = own[i] ? 1 : 0;
    }
    return DCORA_OK;
  });
}
int dcora_radataset_set_pose_pose_weights(dcora_radataset_t h, const double *w) {
  return abi_call({h, w}, [&]() -> int {
    const size_t m = h->ds.pose_pose.size();
    for (size_t e = 0; e < m; ++e)
      if (!std::isfinite(w[e]) || w[e] < 0) return bad("pose-pose weights must be finite and >= 0");
    for (size_t e = 0; e < m; ++e) h->ds.pose_pose[e].weight = w[e];
    return DCORA_OK;
  });
}
// Graph::statistics (ref src/Graph.cpp:475-521) of one robot of the file, host only
int dcora_radataset_loop_closure_stats(dcora_radataset_t h, int robot, int counts[3]) {
  return abi_call({h, counts}, [&] {
    std::vector<TeamLoopClosure> lcs;
    ra_team_loop_closures(h->ds, &lcs);
    // robots 0 (this one) and 1 (everybody else): the counter's agents
    std::vector<int> c(6, 0);
    for (TeamLoopClosure &q : lcs) {
      q.a1 = q.a1 == robot ? 0 : 1;
      q.a2 = q.a2 == robot ? 0 : 1;
      team_count_loop_closure(c.data(), q, q.w0);
    }
    for (int i = 0; i < 3; ++i) counts[i] = c[(size_t)i];
    return DCORA_OK;
  });
}
int dcora_graph_extract_agent_blocks(int k, const int *rp, const int *ci, const double *v, int k_a, const int *own,
                                     dcora_csr_t *Qaa, dcora_csr_t *C) {
  return abi_call({rp, ci, v, own, Qaa, C}, [&]() -> int {
    for (int a = 0; a < k_a; ++a)
      if (own[a] < 0 || own[a] >= k) return bad("extract_agent_blocks: column index out of range");
    std::unique_ptr<dcora_csr_s> q(new dcora_csr_s), c(new dcora_csr_s);
    extract_agent_blocks(view_csr(k, rp, ci, v), std::vector<int>(own, own + k_a), &q->m, &c->m);
    *Qaa = q.release();
    *C = c.release();
    return DCORA_OK;
  });
}
int dcora_radataset_destroy(dcora_radataset_t h) {
  delete h;
  return DCORA_OK;
}
int dcora_graph_precond_regularization(int k, const int *rp, const int *ci, const double *v, int device, double *reg) {
  return abi_call({rp, ci, v, reg}, [&] { return device_precond_regularization(view_csr(k, rp, ci, v), device, reg); });
}

// ---- RBCD session -----------------------------------------------------------------------------------------------
void dcora_rbcd_options_default(dcora_rbcd_options *o) {
  if (!o) return;
  o->num_robots = 5;
  o->r = 5;
  o->acceleration = 1;
  o->restart_interval = 30;
  dcora_ropt_params_default(&o->local);
  o->rank = 0;
  o->world_size = 1;
  o->device = 0;
  o->stream = nullptr;
}
int dcora_rbcd_create(dcora_dataset_t ds, const dcora_rbcd_options *opt, dcora_rbcd_t *out) {
  return abi_call({ds, opt, out}, [&] { return create(out, [&](dcora_rbcd_s &h) { return h.s.init(ds->ds, *opt); }); });
}
// Agent::initializeRobustOptimization (ref src/Agent.cpp:1332-1346) of every agent at creation
int dcora_rbcd_create_robust(dcora_dataset_t ds, const dcora_rbcd_options *opt, const dcora_robust_params *robust,
                             const int *fixed_weight, dcora_rbcd_t *out) {
  return abi_call({ds, opt, robust, out}, [&] { return create_robust(ds, opt, robust, fixed_weight, out); });
}
// the robust session of one rank and its exchange, created together: weight updates are collective
int dcora_rbcd_create_robust_ranks(dcora_dataset_t ds, const dcora_rbcd_options *opt, const dcora_robust_params *robust,
                                   const int *fixed_weight, const char *job_name, dcora_rbcd_t *session,
                                   dcora_exchange_t *ex) {
  return dcora_rbcd_create_robust_ranks_reserved(ds, opt, robust, fixed_weight, 0, job_name, session, ex);
}
// ... with room for the ranks to come (SessionCore::reserve_rank between the two)
int dcora_rbcd_create_robust_ranks_reserved(dcora_dataset_t ds, const dcora_rbcd_options *opt,
                                            const dcora_robust_params *robust, const int *fixed_weight, int r_reserve,
                                            const char *job_name, dcora_rbcd_t *session, dcora_exchange_t *ex) {
  return abi_call({ds, opt, robust, job_name, session, ex}, [&] {
    return create_robust_ranks(ds, opt, robust, fixed_weight, r_reserve, job_name, session, ex);
  });
}
namespace {
int ranked_exchange(dcora_exchange_t ex) {
  return ex->ranked ? DCORA_OK
                    : bad("exchange robust: the exchange was not created by dcora_rbcd_create_robust_ranks or "
                          "dcora_ra_rbcd_create_robust_ranks");
}
}  // namespace
// Agent::updateMeasurementWeights (ref src/Agent.cpp:1397-1441) of every agent
int dcora_rbcd_update_weights(dcora_rbcd_t s, int reset_to_initial, int counts[3]) {
  return abi_call({s}, [&] {
    const int rc = local_robust_session(s->s, "dcora_exchange_update_weights");
    return rc ? rc : s->s.update_weights(reset_to_initial != 0, counts);
  });
}
// Agent::setMeasurementWeight (ref src/Agent.cpp:1443-1454) of every measurement
int dcora_rbcd_set_weights(dcora_rbcd_t s, const double *w) {
  return abi_call({s, w}, [&] {
    const int rc = local_robust_session(s->s, "dcora_exchange_set_weights");
    return rc ? rc : s->s.set_weights(w);
  });
}
int dcora_rbcd_get_weights(dcora_rbcd_t s, double *w) {
  return abi_call({s, w}, [&] {
    const int rc = robust_session(s->s);
    return rc ? rc : s->s.get_weights(w);
  });
}
int dcora_rbcd_robust_info(dcora_rbcd_t s, double *mu, int *updates) {
  return abi_call({s}, [&] { return robust_info(s->s, mu, updates); });
}
int dcora_rbcd_destroy(dcora_rbcd_t s) {
  delete s;
  return DCORA_OK;
}
int dcora_rbcd_set_X(dcora_rbcd_t s, const double *X) {
  return abi_call({s, X}, [&] { return s->s.set_X(X); });
}
int dcora_rbcd_get_X(dcora_rbcd_t s, double *X) {
  return abi_call({s, X}, [&] { return s->s.get_X(X); });
}
int dcora_rbcd_iterate(dcora_rbcd_t s, int selected, double *cost2, double *gradnorm, double *block_norms,
                       int *next_selected) {
  return abi_call({s}, [&] { return s->s.iterate(selected, cost2, gradnorm, block_norms, next_selected); });
}
int dcora_rbcd_run(dcora_rbcd_t s, int max_iters, double rgrad_tol, int *iters_done, double *cost2_trace,
                   double *gradnorm_trace, int *selected_trace) {
  return abi_call({s}, [&] {
    return run_passes(s->s, max_iters, rgrad_tol, iters_done, cost2_trace, gradnorm_trace, selected_trace);
  });
}
int dcora_rbcd_iterate_set(dcora_rbcd_t s, const int *set, int count, int allow_adjacent) {
  return abi_call({s}, [&] {
    return count > 0 && !set ? bad("null argument") : s->s.iterate_set(set, count, allow_adjacent);
  });
}
int dcora_rbcd_set_acceleration(dcora_rbcd_t s, int acceleration) {
  return abi_call({s}, [&] { return s->s.set_acceleration(acceleration != 0); });
}
int dcora_rbcd_agent_colours(dcora_rbcd_t s, int *colours, int *ncolours) {
  return abi_call({s, colours}, [&] { return s->s.agent_colours(colours, ncolours); });
}
int dcora_rbcd_run_coloured(dcora_rbcd_t s, int max_sweeps, double rgrad_tol, int *sweeps_done, double *cost2_trace,
                            double *gradnorm_trace) {
  return abi_call({s}, [&] {
    return run_coloured(s->s, max_sweeps, rgrad_tol, sweeps_done, cost2_trace, gradnorm_trace);
  });
}
int dcora_rbcd_evaluate(dcora_rbcd_t s, double *cost2, double *gradnorm, double *block_norms, int *next_selected) {
  return abi_call({s}, [&] { return s->s.evaluate(cost2, gradnorm, block_norms, next_selected); });
}
int dcora_rbcd_agent_iterate(dcora_rbcd_t s, int agent, int do_optimization) {
  return abi_call({s}, [&] { return s->s.agent_iterate(agent, do_optimization != 0); });
}
int dcora_rbcd_agent_update_neighbor(dcora_rbcd_t s, int agent, int neighbor, int count, const int *frames,
                                     const double *poses, int auxiliary) {
  return abi_call({s}, [&] {
    if (count > 0 && (!frames || !poses)) return bad("null argument");
    return s->s.agent_update_neighbor(agent, neighbor, count, frames, poses, auxiliary != 0);
  });
}
namespace {
bool agent_ok(dcora_rbcd_t s, int agent) { return agent >= 0 && agent < s->s.R; }
}  // namespace
int dcora_rbcd_agent_last_skipped(dcora_rbcd_t s, int agent, int *skipped) {
  return abi_call({s, skipped}, [&] {
    if (!agent_ok(s, agent)) return bad("bad agent");
    *skipped = s->s.agents[agent].last_skipped ? 1 : 0;
    return (int)DCORA_OK;
  });
}
int dcora_rbcd_agent_get_X(dcora_rbcd_t s, int agent, double *X) {
  return abi_call({s, X}, [&] { return s->s.agent_get_X(agent, X); });
}
int dcora_rbcd_agent_set_X(dcora_rbcd_t s, int agent, const double *X) {
  return abi_call({s, X}, [&] { return s->s.agent_set_X(agent, X); });
}
int dcora_rbcd_agent_info(dcora_rbcd_t s, int agent, int *num_poses, int *first_pose, int *iteration_number) {
  return abi_call({s}, [&] {
    if (!agent_ok(s, agent)) return bad("bad agent");
    const AgentDev &a = s->s.agents[agent];
    if (num_poses) *num_poses = a.n;
    if (first_pose) *first_pose = a.col0 / (s->s.d + 1);
    if (iteration_number) *iteration_number = s->s.agent_iteration_number(agent);
    return (int)DCORA_OK;
  });
}
// ---- agent status and the team's decisions -------------------------------------------------------------------------
// AgentParameters' defaults of the fields the rules read (ref include/DCORA/Agent.h:113-125)
void dcora_team_params_default(dcora_team_params *p) {
  if (p) *p = team_params_default();
}
// the local termination rule of Agent::iterate (ref src/Agent.cpp:567-585)
int dcora_team_ready_to_terminate(const dcora_team_params *params, int robust, int weight_update_count, int success,
                                  double relative_change, int accepted, int rejected, int total, int *ready) {
  return abi_call({params, ready}, [&] {
    *ready = team_ready_to_terminate(*params, robust != 0, weight_update_count, success != 0, relative_change, accepted,
                                     rejected, total) ? 1 : 0;
    return (int)DCORA_OK;
  });
}
// Agent::shouldTerminate and Agent::shouldUpdateMeasurementWeights (ref src/Agent.cpp:1123-1156, 1280-1330)
int dcora_team_decide(const dcora_team_params *params, int robust, int iteration_number, int weight_update_count,
                      int inner_iter, int latest_weight_update_iteration, const dcora_agent_status *statuses,
                      const int *have, const int *active, int num_robots, int *should_terminate,
                      int *should_update_weights) {
  return abi_call({params}, [&] {
    if (num_robots < 0 || (num_robots > 0 && (!statuses || !have))) return bad("null argument");
    const TeamView v{robust != 0, iteration_number, weight_update_count, inner_iter, latest_weight_update_iteration,
                     statuses, have, active, num_robots};
    if (should_terminate) *should_terminate = team_should_terminate(*params, v) ? 1 : 0;
    if (should_update_weights) *should_update_weights = team_should_update_weights(*params, v) ? 1 : 0;
    return (int)DCORA_OK;
  });
}
// LiftedArray::maxTranslationDistance (ref src/manifold/Elements.cpp:59-69) through k_rel_change
int dcora_max_translation_distance(int r, int d, int n, const double *X, const double *Y, double *out) {
  return abi_call({X, Y, out}, [&] { return max_translation_distance(r, d, n, X, Y, out); });
}
// the same over the poses of two arrays in the RA ordering, through k_rel_change's range-aided form
int dcora_ra_max_translation_distance(int r, int d, int n, int l, int b, const double *X, const double *Y,
                                      double *out) {
  return abi_call({X, Y, out}, [&] { return ra_max_translation_distance(r, d, n, l, b, X, Y, out); });
}
namespace {
// the team's queries over the session that holds the statuses: a single session's own, or the one of a job's rank
// (dcora_rbcd_* and dcora_exchange_* differ in how they reach it and in the refusal above)
int team_agent_status(SessionCore &s, int agent, dcora_agent_status *status, int *known) {
  if (agent < 0 || agent >= s.R) return bad("bad agent");
  return s.team_agent_status(agent, status, known);
}
int team_loop_closure_stats(SessionCore &s, int agent, int counts[3]) {
  if (agent < 0 || agent >= s.R) return bad("bad agent");
  for (int c = 0; c < 3; ++c) counts[c] = s.team->lc[(size_t)agent * 3 + c];
  return (int)DCORA_OK;
}
int team_info(SessionCore &s, int info[4]) {
  info[0] = s.team_inner_iter();
  info[1] = s.team->latest_weight_update_iteration;
  info[2] = s.team_weight_updates();
  info[3] = s.team->resets_done;
  return (int)DCORA_OK;
}
}  // namespace
// the opt-in to Agent::iterate's status block (ref src/Agent.cpp:558-586) and the bookkeeping of :1417-1424
int dcora_rbcd_team_enable(dcora_rbcd_t s, const dcora_team_params *params) {
  return abi_call({s, params}, [&] { return s->s.team_enable(*params); });
}
// Agent::getStatus (ref include/DCORA/Agent.h:427-433) of one agent of the session
int dcora_rbcd_agent_status(dcora_rbcd_t s, int agent, dcora_agent_status *status, int *known) {
  return abi_call({s, status}, [&] {
    const int rc = team_session(s->s);
    return rc ? rc : team_agent_status(s->s, agent, status, known);
  });
}
// Graph::statistics (ref src/Graph.cpp:475-521) of one agent
int dcora_rbcd_loop_closure_stats(dcora_rbcd_t s, int agent, int counts[3]) {
  return abi_call({s, counts}, [&] {
    const int rc = team_session(s->s);
    return rc ? rc : team_loop_closure_stats(s->s, agent, counts);
  });
}
// Agent::shouldTerminate (ref src/Agent.cpp:1123-1156) over the statuses the session holds
int dcora_rbcd_should_terminate(dcora_rbcd_t s, int *yes) {
  return abi_call({s, yes}, [&] {
    const int rc = team_session(s->s);
    return rc ? rc : s->s.team_decide(yes, nullptr);
  });
}
// Agent::shouldUpdateMeasurementWeights (ref src/Agent.cpp:1280-1330) over the statuses the session holds
int dcora_rbcd_should_update_weights(dcora_rbcd_t s, int *yes) {
  return abi_call({s, yes}, [&] {
    const int rc = team_session(s->s);
    return rc ? rc : s->s.team_decide(nullptr, yes);
  });
}
// mRobustOptInnerIter, mLatestWeightUpdateIteration, mWeightUpdateCount, mTrajectoryResetCount (ref
// include/DCORA/Agent.h:720-735)
int dcora_rbcd_team_info(dcora_rbcd_t s, int info[4]) {
  return abi_call({s, info}, [&] {
    const int rc = team_session(s->s);
    return rc ? rc : team_info(s->s, info);
  });
}
// the optimisation loop of the agents (ref src/Agent.cpp:650-678 with :1123-1156, 1280-1330, 1397-1441) on the
// synchronous schedule of dcora_rbcd_run
int dcora_rbcd_run_team(dcora_rbcd_t s, int *iters_done, double *cost2_trace, double *gradnorm_trace,
                        int *selected_trace, int *updated_trace, int *weight_updates, int *stop_reason) {
  return abi_call({s}, [&] {
    const int rc = team_session(s->s);
    return rc ? rc
              : s->s.run_team(iters_done, cost2_trace, gradnorm_trace, selected_trace, updated_trace, weight_updates,
                              stop_reason);
  });
}
int dcora_rbcd_last_result(dcora_rbcd_t s, dcora_ropt_result *res) {
  return abi_call({s, res}, [&] { return s->s.last_result(res); });
}
namespace {
// dcora_rbcd_certify / dcora_ra_rbcd_certify: the outputs of SessionCore::certify as dcora_cert_fast_verification
// reports them (theta, lambda_min and v only when the certificate is refused)
int session_certify_out(SessionCore &s, double eta, int *certified, double *theta, double *lambda_min, double *v,
                        long long *matvecs, double *info8) {
  CertifyResult res;
  const int rc = s.certify(eta, &res, info8);
  *certified = res.psd ? 1 : 0;
  if (matvecs) *matvecs = res.matvecs;
  if (!res.psd) {
    if (theta) *theta = res.theta;
    if (lambda_min) *lambda_min = res.lambda_min;
    if (v && (long)res.v.size() == s.num_cols()) std::copy(res.v.begin(), res.v.end(), v);
  }
  return rc;
}
}  // namespace
int dcora_rbcd_certify(dcora_rbcd_t s, double eta, int *certified, double *theta, double *lambda_min, double *v,
                       long long *matvecs, double *info8) {
  return abi_call({s, certified}, [&] {
    return session_certify_out(s->s, eta, certified, theta, lambda_min, v, matvecs, info8);
  });
}
// The staircase's step in place (ref examples/MultiRobotExample.cpp:352-366, examples/MultiRobotExample_RASLAM.cpp,
// src/QuadraticProblem.cpp:138-234): SessionCore::lift of either kind
int dcora_lift_params_default(dcora_lift_params *p) {
  return abi_call({p}, [&] {
    p->gradient_tolerance = 1e-6;
    p->preconditioned_gradient_tolerance = 1e-6;
    p->is_second_order = 0;
    p->central_reg = -1.0;
    return (int)DCORA_OK;
  });
}
// (ref examples/MultiRobotExample.cpp:352-366, examples/MultiRobotExample_RASLAM.cpp, src/QuadraticProblem.cpp:138-234)
int dcora_rbcd_lift(dcora_rbcd_t s, double theta, const double *v, const dcora_lift_params *p, int *escaped,
                    double *info8) {
  return abi_call({s, v, p, escaped}, [&] { return s->s.lift(theta, v, *p, escaped, info8); });
}
// the drivers' last step on the live session: getSharedPose(0) -> setGlobalAnchor -> getTrajectoryInGlobalFrame (ref
// examples/MultiRobotExample.cpp:341-347, src/Agent.cpp:1014-1033): SessionCore::round
int dcora_rbcd_round(dcora_rbcd_t s, int anchor_pose, const double *anchor, double *trajectory, double *cost2,
                     double *info4) {
  return abi_call({s, trajectory}, [&] {
    return s->s.round(anchor_pose, anchor, trajectory, nullptr, nullptr, cost2, info4);
  });
}
// the certified flow's last step on the live session (ref examples/SingleRobotExample_RASLAM.cpp:220-234,
// src/DCORA_utils.cpp:1984-2031): SessionCore::project of either kind
int dcora_rbcd_project(dcora_rbcd_t s, double *sigma, double *basis, double *gram, double *cost2, double *info8) {
  return abi_call({s}, [&] { return s->s.project(sigma, basis, gram, cost2, info8); });
}
// k_gram_mfma / k_gram_finish on a host array (tests/test_session_project_gpu.py)
int dcora_debug_project_gram(int r, long long k, const double *X, double *gram, int *chunk) {
  return abi_call({X, gram}, [&]() -> int {
    if (r < 1 || r > kMaxRank || k < 1) return bad("dcora_debug_project_gram: 1 <= r <= 16, k >= 1");
    if (chunk) *chunk = kGramCols;
    DevBuf<double> Xd, P, G;
    DCORA_HIP(Xd.alloc((size_t)r * (size_t)k));
    DCORA_HIP(P.alloc(256 * (size_t)gram_workgroups(k)));
    DCORA_HIP(G.alloc((size_t)r * r));
    DCORA_HIP(hipMemcpy(Xd.p, X, sizeof(double) * (size_t)r * (size_t)k, hipMemcpyHostToDevice));
    // (NaN where the kernels must write: an element they skip shows)
    DCORA_HIP(hipMemset(P.p, 0xff, sizeof(double) * 256 * (size_t)gram_workgroups(k)));
    DCORA_HIP(hipMemset(G.p, 0xff, sizeof(double) * (size_t)r * r));
    launch_gram(nullptr, r, k, Xd.p, P.p, G.p);
    DCORA_HIP(hipGetLastError());
    DCORA_HIP(hipDeviceSynchronize());
    DCORA_HIP(hipMemcpy(gram, G.p, sizeof(double) * (size_t)r * r, hipMemcpyDeviceToHost));
    return (int)DCORA_OK;
  });
}
// k_gram_blocks_mfma / k_gram_blocks_finish on host arrays (tests/test_project_ranks_gpu.py)
int dcora_debug_project_gram_blocks(int r, int nblocks, const long long *k, const double *X, double *grams,
                                    int *chunk) {
  return abi_call({k, X, grams}, [&]() -> int {
    if (r < 1 || r > kMaxRank || nblocks < 1)
      return bad("dcora_debug_project_gram_blocks: 1 <= r <= 16, nblocks >= 1, every k >= 0");
    for (int b = 0; b < nblocks; ++b)
      if (k[b] < 0) return bad("dcora_debug_project_gram_blocks: 1 <= r <= 16, nblocks >= 1, every k >= 0");
    if (chunk) *chunk = kGramCols;
    size_t cols = 0;
    long nwg = 0;
    for (int b = 0; b < nblocks; ++b) cols += (size_t)k[b], nwg += gram_workgroups_of((long)k[b]);
    DevBuf<double> Xd, P, G;
    DevBuf<GramBlock> T;
    const size_t np = 256 * (size_t)std::max<long>(nwg, 1), ng = (size_t)nblocks * r * r;
    DCORA_HIP(Xd.alloc((size_t)r * std::max<size_t>(cols, 1)));
    DCORA_HIP(P.alloc(np));
    DCORA_HIP(G.alloc(ng));
    DCORA_HIP(T.alloc((size_t)nblocks + 1));
    std::vector<GramBlock> table;
    size_t c0 = 0;
    long w0 = 0;
    for (int b = 0; b < nblocks; ++b) {
      table.push_back(GramBlock{Xd.p + (size_t)r * c0, (long)k[b], w0});
      c0 += (size_t)k[b], w0 += gram_workgroups_of((long)k[b]);
    }
    table.push_back(GramBlock{nullptr, 0, w0});
    if (cols) DCORA_HIP(hipMemcpy(Xd.p, X, sizeof(double) * (size_t)r * cols, hipMemcpyHostToDevice));
    DCORA_HIP(hipMemcpy(T.p, table.data(), sizeof(GramBlock) * table.size(), hipMemcpyHostToDevice));
    // (NaN where the kernels must write: an element they skip shows)
    DCORA_HIP(hipMemset(P.p, 0xff, sizeof(double) * np));
    DCORA_HIP(hipMemset(G.p, 0xff, sizeof(double) * ng));
    launch_gram_blocks(nullptr, r, nblocks, nwg, T.p, P.p, G.p);
    DCORA_HIP(hipGetLastError());
    DCORA_HIP(hipDeviceSynchronize());
    DCORA_HIP(hipMemcpy(grams, G.p, sizeof(double) * ng, hipMemcpyDeviceToHost));
    return (int)DCORA_OK;
  });
}
// the block-list pair against a loop of launch_gram over the same blocks, alternated, in event time
// (tools/project_ranks_cost.py)
int dcora_debug_project_gram_time(int r, int nblocks, const long long *k, int reps, double *loop_us, double *pair_us) {
  return abi_call({k, loop_us, pair_us}, [&]() -> int {
    if (r < 1 || r > kMaxRank || nblocks < 1 || reps < 1)
      return bad("dcora_debug_project_gram_time: 1 <= r <= 16, nblocks >= 1, reps >= 1, every k >= 1");
    size_t cols = 0;
    long nwg = 0;
    for (int b = 0; b < nblocks; ++b) {
      if (k[b] < 1) return bad("dcora_debug_project_gram_time: 1 <= r <= 16, nblocks >= 1, reps >= 1, every k >= 1");
      cols += (size_t)k[b], nwg += gram_workgroups_of((long)k[b]);
    }
    DevBuf<double> Xd, P, G;
    DevBuf<GramBlock> T;
    DCORA_HIP(Xd.alloc((size_t)r * cols));
    DCORA_HIP(P.alloc(256 * (size_t)nwg));
    DCORA_HIP(G.alloc((size_t)nblocks * r * r));
    DCORA_HIP(T.alloc((size_t)nblocks + 1));
    std::vector<GramBlock> table;
    size_t c0 = 0;
    long w0 = 0;
    for (int b = 0; b < nblocks; ++b) {
      table.push_back(GramBlock{Xd.p + (size_t)r * c0, (long)k[b], w0});
      c0 += (size_t)k[b], w0 += gram_workgroups_of((long)k[b]);
    }
    table.push_back(GramBlock{nullptr, 0, w0});
    DCORA_HIP(hipMemset(Xd.p, 0, sizeof(double) * (size_t)r * cols));
    DCORA_HIP(hipMemcpy(T.p, table.data(), sizeof(GramBlock) * table.size(), hipMemcpyHostToDevice));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    DCORA_HIP(hipEventCreate(&e0));
    DCORA_HIP(hipEventCreate(&e1));
    for (int i = 0; i < 2 * reps + 2; ++i) {  // (the first of each form warms up and is not kept)
      const bool pair = i & 1;
      DCORA_HIP(hipEventRecord(e0, nullptr));
      if (pair)
        launch_gram_blocks(nullptr, r, nblocks, nwg, T.p, P.p, G.p);
      else
        for (int b = 0; b < nblocks; ++b)
          launch_gram(nullptr, r, table[(size_t)b].k, table[(size_t)b].X, P.p + 256 * table[(size_t)b].wg0,
                      G.p + (size_t)b * r * r);
      DCORA_HIP(hipEventRecord(e1, nullptr));
      DCORA_HIP(hipEventSynchronize(e1));
      float ms = 0;
      DCORA_HIP(hipEventElapsedTime(&ms, e0, e1));
      if (i >= 2) (pair ? pair_us : loop_us)[(i - 2) / 2] = 1e3 * ms;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    DCORA_HIP(hipGetLastError());
    return (int)DCORA_OK;
  });
}
// (ref examples/MultiRobotExample.cpp:352-366, examples/MultiRobotExample_RASLAM.cpp, src/QuadraticProblem.cpp:138-234)
int dcora_rbcd_rank(dcora_rbcd_t s, int *r) {
  return abi_call({s, r}, [&] {
    *r = s->s.r;
    return (int)DCORA_OK;
  });
}
int dcora_rbcd_reserve_rank(dcora_rbcd_t s, int r_reserve) {
  return abi_call({s}, [&] { return s->s.reserve_rank(r_reserve); });
}
// the agent form of k_lift_images on host arrays (tests/test_lift_images_gpu.py)
int dcora_debug_lift_images(int r, int ka, const double *Xa, int kglobal, const double *v, const int *cols, int col0,
                            double *Xplus, double *dir) {
  return abi_call({Xa, v, Xplus, dir}, [&]() -> int {
    if (r < 1 || r + 1 > kMaxRank || ka < 1 || kglobal < 1) return bad("dcora_debug_lift_images: 1 <= r <= 15, ka >= 1");
    for (int j = 0; j < ka; ++j) {
      const long c = cols ? (long)cols[j] : (long)col0 + j;
      if (c < 0 || c >= kglobal) return bad("dcora_debug_lift_images: a column outside the global v");
    }
    const size_t nx = (size_t)r * ka, ni = (size_t)(r + 1) * ka;
    DevBuf<double> X, V, P, D;
    DevBuf<int> Cm;
    DCORA_HIP(X.alloc(nx));
    DCORA_HIP(V.alloc((size_t)kglobal));
    DCORA_HIP(P.alloc(ni));
    DCORA_HIP(D.alloc(ni));
    DCORA_HIP(hipMemcpy(X.p, Xa, sizeof(double) * nx, hipMemcpyHostToDevice));
    DCORA_HIP(hipMemcpy(V.p, v, sizeof(double) * (size_t)kglobal, hipMemcpyHostToDevice));
    if (cols) {
      DCORA_HIP(Cm.alloc((size_t)ka));
      DCORA_HIP(hipMemcpy(Cm.p, cols, sizeof(int) * (size_t)ka, hipMemcpyHostToDevice));
    }
    // (NaN where the kernel must write: an element it skips shows)
    DCORA_HIP(hipMemset(P.p, 0xff, sizeof(double) * ni));
    DCORA_HIP(hipMemset(D.p, 0xff, sizeof(double) * ni));
    launch_lift_images_agent(nullptr, r, ka, X.p, V.p, cols ? Cm.p : nullptr, col0, P.p, D.p);
    DCORA_HIP(hipGetLastError());
    DCORA_HIP(hipDeviceSynchronize());
    DCORA_HIP(hipMemcpy(Xplus, P.p, sizeof(double) * ni, hipMemcpyDeviceToHost));
    DCORA_HIP(hipMemcpy(dir, D.p, sizeof(double) * ni, hipMemcpyDeviceToHost));
    return (int)DCORA_OK;
  });
}
int dcora_rbcd_X_device_ptr(dcora_rbcd_t s, double **X_dev) {
  return abi_call({s, X_dev}, [&] {
    *X_dev = s->s.Xg.p;
    return DCORA_OK;
  });
}
int dcora_rbcd_public_count(dcora_rbcd_t s, int agent, int *count) {
  return abi_call({s, count}, [&] {
    if (!agent_ok(s, agent)) return bad("bad agent");
    *count = (int)s->s.agents[agent].public_poses.size();
    return (int)DCORA_OK;
  });
}
int dcora_rbcd_public_indices(dcora_rbcd_t s, int agent, int *idx) {
  return abi_call({s, idx}, [&] {
    if (!agent_ok(s, agent)) return bad("bad agent");
    const auto &v = s->s.agents[agent].public_poses;
    std::copy(v.begin(), v.end(), idx);
    return (int)DCORA_OK;
  });
}
// (an agent without public poses moves no data: its buffer may be NULL)
int dcora_rbcd_pack_public_dev(dcora_rbcd_t s, int agent, double *packed_dev) {
  return abi_call({s}, [&] {
    if (!agent_ok(s, agent)) return bad("bad agent");
    if (!packed_dev && !s->s.agents[agent].public_poses.empty()) return bad("null argument");
    return s->s.pack_public(agent, packed_dev);
  });
}
int dcora_rbcd_unpack_public_dev(dcora_rbcd_t s, int agent, const double *packed_dev) {
  return abi_call({s}, [&] {
    if (!agent_ok(s, agent)) return bad("bad agent");
    if (!packed_dev && !s->s.agents[agent].public_poses.empty()) return bad("null argument");
    return s->s.unpack_public(agent, packed_dev);
  });
}
int dcora_rbcd_phase_nonselected(dcora_rbcd_t s, int selected) {
  return abi_call({s}, [&] { return s->s.phase_nonselected(selected); });
}
int dcora_rbcd_phase_selected(dcora_rbcd_t s, int selected) {
  return abi_call({s}, [&] { return s->s.phase_selected(selected); });
}
int dcora_debug_rbcd_launches(dcora_rbcd_t s, long long *launches) {
  return abi_call({s, launches}, [&] {
    *launches = s->s.chain_launches;
    return (int)DCORA_OK;
  });
}
int dcora_debug_launch_count(long long *launches) {
  return abi_call({launches}, [&] {
    *launches = g_chain_launches.load(std::memory_order_relaxed);
    return (int)DCORA_OK;
  });
}
int dcora_rbcd_phase_evaluate_dev(dcora_rbcd_t s, double *out_dev) {
  return abi_call({s, out_dev}, [&] { return s->s.phase_evaluate_dev(out_dev); });
}
// measurement hook of bench.py's roofline: HIP events around the one-launch tCG runs of the session's agents
int dcora_rbcd_profile_tcg_runs(dcora_rbcd_t s, int enable) {
  return abi_call({s}, [&] {
    for (auto &a : s->s.agents)
      if (a.prob) a.prob->profile_tcg_runs = enable != 0;
    return DCORA_OK;
  });
}
int dcora_rbcd_profile_tcg_read(dcora_rbcd_t s, double *out2) {
  return abi_call({s, out2}, [&] {
    out2[0] = out2[1] = 0;
    for (auto &a : s->s.agents) {
      if (!a.prob) continue;
      double n = 0, us = 0;
      const int rc = a.prob->profile_tcg_read(&n, &us);
      if (rc) return rc;
      out2[0] += n;
      out2[1] += us;
    }
    return (int)DCORA_OK;
  });
}
int dcora_rbcd_synchronize(dcora_rbcd_t s) {
  return abi_call({s}, [&]() -> int {
    DCORA_HIP(hipStreamSynchronize(s->s.st));
    return DCORA_OK;
  });
}

// ---- neighbour exchange between ranks ------------------------------------------------------------------------------
int dcora_exchange_create(dcora_rbcd_t s, const char *job_name, dcora_exchange_t *out) {
  return abi_call({s, job_name, out}, [&] {
    return create(out, [&](dcora_exchange_s &h) { return h.e.init(&s->s, job_name); });
  });
}
int dcora_exchange_destroy(dcora_exchange_t ex) {
  delete ex;
  return DCORA_OK;
}
int dcora_exchange_info(dcora_exchange_t ex, double *info) {
  return abi_call({ex, info}, [&] {
    const Exchange &e = ex->e;
    info[0] = e.mode;
    info[1] = e.num_peers();
    info[2] = (double)e.posts;
    info[3] = (double)e.waits;
    info[4] = e.bytes_posted;
    info[5] = e.post_s;
    info[6] = e.wait_s;
    info[7] = e.eval_wait_s;
    info[8] = e.halo_is_finegrained() ? 1 : 0;
    info[9] = e.waits_on_device() ? 1 : 0;
    return DCORA_OK;
  });
}
int dcora_debug_exchange_probe_fault(int rounds) {
  g_probe_fault_rounds.store(rounds);
  return DCORA_OK;
}
int dcora_exchange_link_report(dcora_exchange_t ex, double *out4) {
  return abi_call({ex, out4}, [&] {
    const Exchange &e = ex->e;
    out4[0] = e.link_rounds;
    out4[1] = e.link_gave_up_device_wait;
    out4[2] = e.link_gave_up_ipc;
    out4[3] = e.link_last_us;
    return DCORA_OK;
  });
}
int dcora_exchange_post(dcora_exchange_t ex, const int *agents, int count) {
  return abi_call({ex}, [&] { return !agents && count > 0 ? bad("null argument") : ex->e.post(agents, count); });
}
int dcora_exchange_wait(dcora_exchange_t ex, const int *agents, int count) {
  return abi_call({ex}, [&] { return !agents && count > 0 ? bad("null argument") : ex->e.wait(agents, count); });
}
int dcora_exchange_evaluate(dcora_exchange_t ex, double *cost2, double *gradnorm, double *block_norms,
                            int *next_selected) {
  return abi_call({ex}, [&] { return ex->e.evaluate(cost2, gradnorm, block_norms, next_selected); });
}
int dcora_exchange_rbcd_iterate(dcora_exchange_t ex, int selected, double *cost2, double *gradnorm,
                                double *block_norms, int *next_selected) {
  return abi_call({ex}, [&] { return ex->e.rbcd_iterate(selected, cost2, gradnorm, block_norms, next_selected); });
}
int dcora_exchange_rbcd_tick(dcora_exchange_t ex, const int *set, int count, int allow_adjacent) {
  return abi_call({ex, set}, [&] { return ex->e.rbcd_tick(set, count, allow_adjacent); });
}
int dcora_exchange_run_coloured(dcora_exchange_t ex, int max_sweeps, double rgrad_tol, int *sweeps_done,
                                double *cost2_trace, double *gradnorm_trace) {
  return abi_call({ex}, [&] {
    return ex->e.run_coloured(max_sweeps, rgrad_tol, sweeps_done, cost2_trace, gradnorm_trace);
  });
}
int dcora_exchange_set_X(dcora_exchange_t ex, const double *X) {
  return abi_call({ex, X}, [&] { return ex->e.set_X(X); });
}
int dcora_exchange_gather_X(dcora_exchange_t ex, double *X) {
  return abi_call({ex, X}, [&] { return ex->e.gather_X(X); });
}
// every agent's own trajectory against the shared anchor, on the rank that hosts it (ref
// examples/MultiRobotExample.cpp:341-347, examples/MultiRobotExample_RASLAM.cpp:488-495, src/Agent.cpp:1014-1033); a NULL
// trajectory is refused inside, before any collective step, on every rank alike
int dcora_exchange_round(dcora_exchange_t ex, int anchor_pose, const double *anchor, double *trajectory,
                         double *unit_spheres, double *landmarks) {
  return abi_call({ex}, [&] { return ex->e.round(anchor_pose, anchor, trajectory, unit_spheres, landmarks); });
}
// the staircase's step of the whole job (ref examples/MultiRobotExample.cpp:352-366, src/QuadraticProblem.cpp:138-234);
// a NULL v is refused like a non-finite one, on every rank alike
int dcora_exchange_lift(dcora_exchange_t ex, double theta, const double *v, const dcora_lift_params *params,
                        int *escaped, double *info8) {
  return abi_call({ex, params, escaped}, [&] { return ex->e.lift(theta, v, *params, escaped, info8); });
}
// the certified flow's last step of the whole job (ref examples/SingleRobotExample_RASLAM.cpp:220-234,
// projectSolutionRASLAM src/DCORA_utils.cpp:1984-2031): Exchange::project on either session kind
int dcora_exchange_project(dcora_exchange_t ex, double *sigma, double *basis, double *gram, double *cost2,
                           double *info8) {
  return abi_call({ex}, [&] { return ex->e.project(sigma, basis, gram, cost2, info8); });
}
int dcora_debug_exchange_project_sums(int on) {
  g_project_gram_sums.store(on ? 1 : 0);
  return DCORA_OK;
}
int dcora_exchange_host_selftest(const char *job_name, int rank, int world_size, int num_agents, int rounds,
                                 double *checksum) {
  return abi_call({job_name}, [&] {
    Exchange e;
    return e.host_selftest(job_name, rank, world_size, num_agents, rounds, checksum);
  });
}
// Q is needed on rank 0 only: a pattern with any of its three arrays NULL counts as absent
int dcora_exchange_certify(dcora_exchange_t ex, int k, const int *rowptr, const int *colidx, const double *vals,
                           double eta, int *certified, double *theta, double *lambda_min, double *v, long long *matvecs,
                           int *distributed) {
  return abi_call({ex}, [&] {
    if (rowptr && colidx && vals) {
      const HostCsr Q = view_csr(k, rowptr, colidx, vals);
      return ex->e.certify(&Q, eta, certified, theta, lambda_min, v, matvecs, distributed);
    }
    return ex->e.certify(nullptr, eta, certified, theta, lambda_min, v, matvecs, distributed);
  });
}
// the certificate of the matrices the ranks hold (ref src/DCORA_utils.cpp:1713-1735, 1898-1982,
// examples/MultiRobotExample.cpp:321-335); a NULL certified is refused inside, like a bad eta, on every rank alike
int dcora_exchange_certify_live(dcora_exchange_t ex, double eta, int *certified, double *theta, double *lambda_min,
                                double *v, long long *matvecs, int *distributed, double *info10) {
  return abi_call({ex}, [&] {
    return ex->e.certify_live(eta, certified, theta, lambda_min, v, matvecs, distributed, info10);
  });
}
// the table builder of dcora_exchange_certify_live on host arrays, a host loop in the kernel's place
// (tests/test_certify_ranks_cpu.py)
int dcora_debug_cert_rows(const dcora_dims *dims, const int *rp, const int *ci, const double *vals,
                          const dcora_dims *agent_dims, const int *cols, const double *lambda, double eta, long long lo,
                          long long hi, long long round_size, double *window, unsigned char *written,
                          long long *nnz_pattern, long long corrupt_entry) {
  return abi_call({dims, rp, ci, vals, agent_dims, cols, lambda}, [&]() -> int {
    if (!layout_ok(dims) || !layout_ok(agent_dims)) return bad("dims: layout SE needs l = b = 0");
    const ManiDesc mg = make_mani(*dims), ma = make_mani(*agent_dims);
    if (mg.k < 1 || ma.k < 1 || ma.k > mg.k || ma.d != mg.d) return bad("dcora_debug_cert_rows: bad dims");
    if (rp[0] != 0) return bad("dcora_debug_cert_rows: rowptr[0] must be 0");
    for (int i = 0; i < mg.k; ++i)
      if (rp[i + 1] < rp[i]) return bad("dcora_debug_cert_rows: rowptr decreases");
    for (int p = 0; p < rp[mg.k]; ++p)
      if (ci[p] < 0 || ci[p] >= mg.k) return bad("dcora_debug_cert_rows: column index out of range");
    const std::vector<int> own(cols, cols + ma.k);
    for (int c : own)
      if (c < 0 || c >= mg.k) return bad("dcora_debug_cert_rows: a column outside the job");
    const HostCsr Q = view_csr(mg.k, rp, ci, vals);
    const HostCsr P = dual_certificate_pattern(mg, Q);
    if (nnz_pattern) *nnz_pattern = P.nnz();
    HostCsr Qaa, C;
    extract_agent_blocks(Q, own, &Qaa, &C);
    CertRowTable t;
    int rc = build_cert_row_table(P, own, Qaa, C, ma, &t);
    if (rc) return rc;
    if (corrupt_entry >= 0 && corrupt_entry < (long long)t.size()) t.src[(size_t)corrupt_entry] = Qaa.nnz() + C.nnz() + 7;
    rc = check_cert_row_table(t, P.nnz(), Qaa.nnz(), C.nnz(), (long)ma.n * ma.d * ma.d + ma.l);
    if (rc) return rc;
    if (lo < 0 || hi < lo || hi > P.nnz()) return bad("dcora_debug_cert_rows: the window leaves the value array");
    if (hi > lo && (!window || !written)) return bad("null argument");
    // the job's walk: round c carries [lo + c round_size, lo + (c + 1) round_size), each through its own window base
    const long long step = round_size > 0 ? round_size : std::max<long long>(hi - lo, 1);
    for (long long a = lo; a < hi; a += step) {
      const long long b = std::min(hi, a + step);
      size_t first = 0, last = 0;
      cert_row_window(t.pos, (long)a, (long)b, &first, &last);
      cert_rows_host(t, first, last, Qaa.v.data(), C.v.data(), lambda, eta, (long)a, window + (a - lo), written + (a - lo));
    }
    return (int)DCORA_OK;
  });
}
int dcora_exchange_all_ready(dcora_exchange_t ex, int ready, int *all_ready) {
  return abi_call({ex, all_ready}, [&] {
    double notready = ready ? 0.0 : 1.0;
    const int rc = ex->e.allreduce_sum(&notready, 1);
    if (rc) return rc;
    *all_ready = notready == 0.0 ? 1 : 0;
    return (int)DCORA_OK;
  });
}
int dcora_debug_exchange_leave_stale(const char *job_name, int world_size, int num_agents) {
  return abi_call({job_name}, [&] {
    Exchange e;
    return e.debug_leave_stale(job_name, world_size, num_agents);
  });
}
int dcora_exchange_barrier(dcora_exchange_t ex) {
  return abi_call({ex}, [&] { return ex->e.barrier(); });
}
int dcora_exchange_update_weights(dcora_exchange_t ex, int reset_to_initial, int counts[3]) {
  return abi_call({ex, counts}, [&] {
    const int rc = ranked_exchange(ex);
    return rc ? rc : ex->e.update_weights(reset_to_initial != 0, counts);
  });
}
int dcora_exchange_set_weights(dcora_exchange_t ex, const double *w) {
  return abi_call({ex, w}, [&] {
    const int rc = ranked_exchange(ex);
    return rc ? rc : ex->e.set_weights(w);
  });
}
int dcora_exchange_get_weights(dcora_exchange_t ex, double *w) {
  return abi_call({ex, w}, [&] {
    const int rc = ranked_exchange(ex);
    return rc ? rc : ex->e.get_weights(w);
  });
}
// ---- the team protocol across the ranks (Exchange::team_enable) ----
namespace {
int team_exchange(dcora_exchange_t ex) {
  return ex->e.team_on() ? (int)DCORA_OK
                         : bad("exchange team: the exchange has not called dcora_exchange_team_enable / "
                               "dcora_exchange_team_enable_ra");
}
}  // namespace
int dcora_exchange_team_enable(dcora_exchange_t ex, const dcora_team_params *params) {
  return abi_call({ex, params}, [&] { return ex->e.team_enable(*params, false); });
}
int dcora_exchange_team_enable_ra(dcora_exchange_t ex, const dcora_team_params *params) {
  return abi_call({ex, params}, [&] { return ex->e.team_enable(*params, true); });
}
int dcora_exchange_agent_status(dcora_exchange_t ex, int agent, dcora_agent_status *status, int *known) {
  return abi_call({ex, status}, [&] {
    const int rc = team_exchange(ex);
    return rc ? rc : team_agent_status(*ex->e.team_session(), agent, status, known);
  });
}
int dcora_exchange_loop_closure_stats(dcora_exchange_t ex, int agent, int counts[3]) {
  return abi_call({ex, counts}, [&] {
    const int rc = team_exchange(ex);
    return rc ? rc : team_loop_closure_stats(*ex->e.team_session(), agent, counts);
  });
}
int dcora_exchange_should_terminate(dcora_exchange_t ex, int *yes) {
  return abi_call({ex, yes}, [&] {
    const int rc = team_exchange(ex);
    return rc ? rc : ex->e.team_session()->team_decide(yes, nullptr);
  });
}
int dcora_exchange_should_update_weights(dcora_exchange_t ex, int *yes) {
  return abi_call({ex, yes}, [&] {
    const int rc = team_exchange(ex);
    return rc ? rc : ex->e.team_session()->team_decide(nullptr, yes);
  });
}
int dcora_exchange_team_info(dcora_exchange_t ex, int info[4]) {
  return abi_call({ex, info}, [&] {
    const int rc = team_exchange(ex);
    return rc ? rc : team_info(*ex->e.team_session(), info);
  });
}
int dcora_exchange_run_team(dcora_exchange_t ex, int *iters_done, double *cost2_trace, double *gradnorm_trace,
                            int *selected_trace, int *updated_trace, int *weight_updates, int *stop_reason) {
  return abi_call({ex}, [&] {
    const int rc = team_exchange(ex);
    return rc ? rc
              : ex->e.run_team(iters_done, cost2_trace, gradnorm_trace, selected_trace, updated_trace, weight_updates,
                               stop_reason);
  });
}
int dcora_exchange_host_selftest_team(const char *job_name, int rank, int world_size, int num_agents, int rounds,
                                      int skew_us, double *checksum) {
  return abi_call({job_name}, [&] {
    Exchange e;
    return e.host_selftest_team(job_name, rank, world_size, num_agents, rounds, skew_us, checksum);
  });
}

// ---- RBCD session, range-aided SLAM ----------------------------------------------------------------------------
struct dcora_ra_rbcd_s {
  RaRbcdSession s;
};
int dcora_ra_rbcd_create(dcora_radataset_t ds, const dcora_rbcd_options *opt, dcora_ra_rbcd_t *out) {
  return abi_call({ds, opt, out}, [&] {
    return create(out, [&](dcora_ra_rbcd_s &h) { return h.s.init(ds->ds, *opt); });
  });
}
int dcora_exchange_create_ra(dcora_ra_rbcd_t s, const char *job_name, dcora_exchange_t *out) {
  return abi_call({s, job_name, out}, [&] {
    return create(out, [&](dcora_exchange_s &h) { return h.e.init(&s->s, job_name); });
  });
}
int dcora_ra_rbcd_destroy(dcora_ra_rbcd_t s) {
  delete s;
  return DCORA_OK;
}
int dcora_ra_rbcd_info(dcora_ra_rbcd_t s, int *num_agents, int *robots) {
  return abi_call({s, num_agents}, [&] {
    *num_agents = s->s.R;
    if (robots)
      for (int i = 0; i < s->s.R; ++i) robots[i] = s->s.agents[i].robot;
    return DCORA_OK;
  });
}
int dcora_ra_rbcd_set_X(dcora_ra_rbcd_t s, const double *X) {
  return abi_call({s, X}, [&] { return s->s.set_X(X); });
}
int dcora_ra_rbcd_get_X(dcora_ra_rbcd_t s, double *X) {
  return abi_call({s, X}, [&] { return s->s.get_X(X); });
}
int dcora_ra_rbcd_iterate(dcora_ra_rbcd_t s, int selected, double *cost2, double *gradnorm, double *block_norms,
                          int *next_selected) {
  return abi_call({s}, [&] { return s->s.iterate(selected, cost2, gradnorm, block_norms, next_selected); });
}
int dcora_ra_rbcd_evaluate(dcora_ra_rbcd_t s, double *cost2, double *gradnorm, double *block_norms,
                           int *next_selected) {
  return abi_call({s}, [&] { return s->s.evaluate(cost2, gradnorm, block_norms, next_selected); });
}
int dcora_ra_rbcd_run(dcora_ra_rbcd_t s, int max_iters, double rgrad_tol, int *iters_done, double *cost2_trace,
                      double *gradnorm_trace, int *selected_trace) {
  return abi_call({s}, [&] {
    return run_passes(s->s, max_iters, rgrad_tol, iters_done, cost2_trace, gradnorm_trace, selected_trace);
  });
}
int dcora_ra_rbcd_iterate_set(dcora_ra_rbcd_t s, const int *set, int count, int allow_adjacent) {
  return abi_call({s}, [&] {
    return count > 0 && !set ? bad("null argument") : s->s.iterate_set(set, count, allow_adjacent);
  });
}
int dcora_ra_rbcd_set_acceleration(dcora_ra_rbcd_t s, int acceleration) {
  return abi_call({s}, [&] { return s->s.set_acceleration(acceleration != 0); });
}
int dcora_ra_rbcd_agent_colours(dcora_ra_rbcd_t s, int *colours, int *ncolours) {
  return abi_call({s, colours}, [&] { return s->s.agent_colours(colours, ncolours); });
}
int dcora_ra_rbcd_run_coloured(dcora_ra_rbcd_t s, int max_sweeps, double rgrad_tol, int *sweeps_done,
                               double *cost2_trace, double *gradnorm_trace) {
  return abi_call({s}, [&] {
    return run_coloured(s->s, max_sweeps, rgrad_tol, sweeps_done, cost2_trace, gradnorm_trace);
  });
}
int dcora_ra_rbcd_last_result(dcora_ra_rbcd_t s, dcora_ropt_result *res) {
  return abi_call({s, res}, [&] { return s->s.last_result(res); });
}
int dcora_ra_rbcd_certify(dcora_ra_rbcd_t s, double eta, int *certified, double *theta, double *lambda_min, double *v,
                          long long *matvecs, double *info8) {
  return abi_call({s, certified}, [&] {
    return session_certify_out(s->s, eta, certified, theta, lambda_min, v, matvecs, info8);
  });
}
// (ref examples/MultiRobotExample.cpp:352-366, examples/MultiRobotExample_RASLAM.cpp, src/QuadraticProblem.cpp:138-234)
// (ref examples/MultiRobotExample_RASLAM.cpp:488-495, src/Agent.cpp:1014-1033; the evaluated point's sphere columns as
// projectSolutionRASLAM's, src/DCORA_utils.cpp:1984-2031)
int dcora_ra_rbcd_round(dcora_ra_rbcd_t s, int anchor_pose, const double *anchor, double *trajectory,
                        double *unit_spheres, double *landmarks, double *cost2, double *info4) {
  return abi_call({s, trajectory}, [&] {
    return s->s.round(anchor_pose, anchor, trajectory, unit_spheres, landmarks, cost2, info4);
  });
}
int dcora_ra_rbcd_project(dcora_ra_rbcd_t s, double *sigma, double *basis, double *gram, double *cost2,
                          double *info8) {
  return abi_call({s}, [&] { return s->s.project(sigma, basis, gram, cost2, info8); });
}
int dcora_ra_rbcd_lift(dcora_ra_rbcd_t s, double theta, const double *v, const dcora_lift_params *p, int *escaped,
                       double *info8) {
  return abi_call({s, v, p, escaped}, [&] { return s->s.lift(theta, v, *p, escaped, info8); });
}
// (ref examples/MultiRobotExample.cpp:352-366, examples/MultiRobotExample_RASLAM.cpp, src/QuadraticProblem.cpp:138-234)
int dcora_ra_rbcd_reserve_rank(dcora_ra_rbcd_t s, int r_reserve) {
  return abi_call({s}, [&] { return s->s.reserve_rank(r_reserve); });
}
int dcora_ra_rbcd_rank(dcora_ra_rbcd_t s, int *r) {
  return abi_call({s, r}, [&] {
    *r = s->s.r;
    return (int)DCORA_OK;
  });
}
// Agent::initializeRobustOptimization (ref src/Agent.cpp:1332-1346) of every agent of a RangeAidedSLAMGraph at creation
int dcora_ra_rbcd_create_robust(dcora_radataset_t ds, const dcora_rbcd_options *opt, const dcora_robust_params *robust,
                                const int *fixed_weight, dcora_ra_rbcd_t *out) {
  return abi_call({ds, opt, robust, out}, [&] { return create_robust(ds, opt, robust, fixed_weight, out); });
}
// the robust session of one rank of a range-aided job and its exchange, created together: weight updates are collective
int dcora_ra_rbcd_create_robust_ranks(dcora_radataset_t ds, const dcora_rbcd_options *opt,
                                      const dcora_robust_params *robust, const int *fixed_weight, const char *job_name,
                                      dcora_ra_rbcd_t *session, dcora_exchange_t *ex) {
  return dcora_ra_rbcd_create_robust_ranks_reserved(ds, opt, robust, fixed_weight, 0, job_name, session, ex);
}
int dcora_ra_rbcd_create_robust_ranks_reserved(dcora_radataset_t ds, const dcora_rbcd_options *opt,
                                               const dcora_robust_params *robust, const int *fixed_weight,
                                               int r_reserve, const char *job_name, dcora_ra_rbcd_t *session,
                                               dcora_exchange_t *ex) {
  return abi_call({ds, opt, robust, job_name, session, ex}, [&] {
    return create_robust_ranks(ds, opt, robust, fixed_weight, r_reserve, job_name, session, ex);
  });
}
// Agent::updateMeasurementWeights (ref src/Agent.cpp:1397-1441) of every agent
int dcora_ra_rbcd_update_weights(dcora_ra_rbcd_t s, int reset_to_initial, int counts[3]) {
  return abi_call({s}, [&] {
    const int rc = local_robust_session(s->s, "dcora_exchange_update_weights");
    return rc ? rc : s->s.update_weights(reset_to_initial != 0, counts);
  });
}
// Agent::setMeasurementWeight (ref src/Agent.cpp:1443-1454) of every pose-pose measurement
int dcora_ra_rbcd_set_weights(dcora_ra_rbcd_t s, const double *w) {
  return abi_call({s, w}, [&] {
    const int rc = local_robust_session(s->s, "dcora_exchange_set_weights");
    return rc ? rc : s->s.set_weights(w);
  });
}
int dcora_ra_rbcd_get_weights(dcora_ra_rbcd_t s, double *w) {
  return abi_call({s, w}, [&] {
    const int rc = robust_session(s->s);
    return rc ? rc : s->s.get_weights(w);
  });
}
int dcora_ra_rbcd_robust_info(dcora_ra_rbcd_t s, double *mu, int *updates) {
  return abi_call({s}, [&] { return robust_info(s->s, mu, updates); });
}
// ---- agent status and the team's decisions on a range-aided session (the dcora_rbcd_* namesakes' contracts) ----
// the opt-in to Agent::iterate's status block (ref src/Agent.cpp:558-586) and the bookkeeping of :1417-1424
int dcora_ra_rbcd_team_enable(dcora_ra_rbcd_t s, const dcora_team_params *params) {
  return abi_call({s, params}, [&] { return s->s.team_enable(*params); });
}
// Agent::getStatus (ref include/DCORA/Agent.h:427-433) of one agent of the session
int dcora_ra_rbcd_agent_status(dcora_ra_rbcd_t s, int agent, dcora_agent_status *status, int *known) {
  return abi_call({s, status}, [&] {
    const int rc = team_session(s->s);
    return rc ? rc : team_agent_status(s->s, agent, status, known);
  });
}
// Graph::statistics (ref src/Graph.cpp:475-521) of one agent's RangeAidedSLAMGraph
int dcora_ra_rbcd_loop_closure_stats(dcora_ra_rbcd_t s, int agent, int counts[3]) {
  return abi_call({s, counts}, [&] {
    const int rc = team_session(s->s);
    return rc ? rc : team_loop_closure_stats(s->s, agent, counts);
  });
}
// Agent::shouldTerminate (ref src/Agent.cpp:1123-1156) over the statuses the session holds
int dcora_ra_rbcd_should_terminate(dcora_ra_rbcd_t s, int *yes) {
  return abi_call({s, yes}, [&] {
    const int rc = team_session(s->s);
    return rc ? rc : s->s.team_decide(yes, nullptr);
  });
}
// Agent::shouldUpdateMeasurementWeights (ref src/Agent.cpp:1280-1330) over the statuses the session holds
int dcora_ra_rbcd_should_update_weights(dcora_ra_rbcd_t s, int *yes) {
  return abi_call({s, yes}, [&] {
    const int rc = team_session(s->s);
    return rc ? rc : s->s.team_decide(nullptr, yes);
  });
}
// mRobustOptInnerIter, mLatestWeightUpdateIteration, mWeightUpdateCount, mTrajectoryResetCount (ref
// include/DCORA/Agent.h:720-735)
int dcora_ra_rbcd_team_info(dcora_ra_rbcd_t s, int info[4]) {
  return abi_call({s, info}, [&] {
    const int rc = team_session(s->s);
    return rc ? rc : team_info(s->s, info);
  });
}
// the optimisation loop of the agents (ref src/Agent.cpp:650-678 with :1123-1156, 1280-1330, 1397-1441) on the
// synchronous schedule of dcora_ra_rbcd_run
int dcora_ra_rbcd_run_team(dcora_ra_rbcd_t s, int *iters_done, double *cost2_trace, double *gradnorm_trace,
                           int *selected_trace, int *updated_trace, int *weight_updates, int *stop_reason) {
  return abi_call({s}, [&] {
    const int rc = team_session(s->s);
    return rc ? rc
              : s->s.run_team(iters_done, cost2_trace, gradnorm_trace, selected_trace, updated_trace, weight_updates,
                              stop_reason);
  });
}

// ---- robust estimation ---------------------------------------------------------------------------------------
void dcora_robust_params_default(dcora_robust_params *p) {
  if (!p) return;
  p->cost_type = DCORA_ROBUST_L2;
  p->GNCMaxNumIters = 20;
  p->GNCBarc = 5.0;
  p->GNCMuStep = 1.4;
  p->GNCInitMu = 1e-4;
  p->HuberThreshold = 3;
  p->TLSThreshold = 10;
}
int dcora_robust_weights(const dcora_robust_params *p, int num_updates, int n, const double *r, double *w) {
  return abi_call({p, r, w}, [&] {
    if (p->cost_type < DCORA_ROBUST_L2 || p->cost_type > DCORA_ROBUST_GNC_TLS) return bad("unknown robust cost type");
    RobustCost c(*p);
    for (int i = 0; i < num_updates; ++i) c.update();
    for (int i = 0; i < n; ++i) w[i] = c.weight(r[i]);
    return (int)DCORA_OK;
  });
}
int dcora_chi2inv(double quantile, int dof, double *out) {
  return abi_call({out}, [&] {
    if (!(quantile > 0) || !(quantile < 1) || dof < 1) return bad("chi2inv: need 0 < quantile < 1, dof >= 1");
    *out = chi2inv(quantile, dof);
    return (int)DCORA_OK;
  });
}
int dcora_robust_error_threshold_at_quantile(double quantile, int dimension, double *out) {
  return abi_call({out}, [&] {
    if (!error_threshold_at_quantile(quantile, dimension, out))
      return bad("quantile function currently only supports 3D problems and quantile > 0");
    return (int)DCORA_OK;
  });
}
int dcora_robust_single_rotation_averaging(int d, int n, const double *R, const double *kappa, double thr,
                                           double *Ropt, int *inlier) {
  return abi_call({R, Ropt, inlier}, [&] {
    if (n < 1 || (d != 2 && d != 3)) return bad("bad argument");
    std::vector<int> in;
    robust_single_rotation_averaging(d, n, R, kappa, thr, Ropt, in);
    std::fill(inlier, inlier + n, 0);
    for (int i : in) inlier[i] = 1;
    return (int)DCORA_OK;
  });
}
int dcora_robust_single_pose_averaging(int d, int n, const double *R, const double *t, const double *kappa,
                                       const double *tau, double thr, double *Ropt, double *topt, int *inlier) {
  return abi_call({R, t, Ropt, topt, inlier}, [&] {
    if (n < 1 || (d != 2 && d != 3)) return bad("bad argument");
    std::vector<int> in;
    robust_single_pose_averaging(d, n, R, t, kappa, tau, thr, Ropt, topt, in);
    std::fill(inlier, inlier + n, 0);
    for (int i : in) inlier[i] = 1;
    return (int)DCORA_OK;
  });
}
int dcora_agent_neighbor_transforms(int d, int m, const int *incoming, const double *meas_R, const double *meas_t,
                                    const double *nbr_pose, const double *my_pose, double *T_out) {
  return abi_call({incoming, meas_R, meas_t, nbr_pose, my_pose, T_out}, [&] {
    if (m < 0 || (d != 2 && d != 3)) return bad("bad argument");
    const int ps = d * (d + 1);
    for (int i = 0; i < m; ++i)
      neighbor_transform(d, incoming[i] != 0, meas_R + (size_t)i * d * d, meas_t + (size_t)i * d,
                         nbr_pose + (size_t)i * ps, my_pose + (size_t)i * ps, T_out + (size_t)i * ps);
    return (int)DCORA_OK;
  });
}
int dcora_agent_robust_neighbor_transform(int d, int m, const double *candidates, int two_stage, int min_inliers,
                                          double *T_world_robot, int *num_inliers, int *ok) {
  return abi_call({candidates, T_world_robot, ok}, [&] {
    if (m < 0 || (d != 2 && d != 3)) return bad("bad argument");
    *ok = robust_neighbor_transform(d, m, candidates, two_stage != 0, min_inliers, T_world_robot, num_inliers) ? 1 : 0;
    return (int)DCORA_OK;
  });
}
int dcora_log_trajectory(const char *path, int d, int n, const double *T) {
  return abi_call({path, T}, [&]() -> int {
    if (n < 0 || (d != 2 && d != 3)) return bad("bad argument");
    FILE *f = std::fopen(path, "w");
    if (!f) {
      set_last_error(std::string("cannot log trajectory to ") + path);
      return DCORA_ERR_IO;
    }
    std::fprintf(f, "# pose_index x y z qx qy qz qw\n");
    const int dh = d + 1;
    for (int i = 0; i < n; ++i) {
      double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, t[3] = {0, 0, 0};
      const double *Ti = T + (size_t)i * dh * d;
      for (int c = 0; c < d; ++c)
        for (int a = 0; a < d; ++a) R[a][c] = Ti[a + c * d];
      for (int a = 0; a < d; ++a) t[a] = Ti[a + d * d];
      // rotation matrix -> quaternion with the branch rule of Eigen::Quaterniond(Matrix3d) the reference relies on
      double q[4];  // x y z w
      double tr = R[0][0] + R[1][1] + R[2][2];
      if (tr > 0) {
        double s = std::sqrt(tr + 1.0);
        q[3] = 0.5 * s;
        s = 0.5 / s;
        q[0] = (R[2][1] - R[1][2]) * s;
        q[1] = (R[0][2] - R[2][0]) * s;
        q[2] = (R[1][0] - R[0][1]) * s;
      } else {
        int a = 0;
        if (R[1][1] > R[0][0]) a = 1;
        if (R[2][2] > R[a][a]) a = 2;
        const int b = (a + 1) % 3, c = (b + 1) % 3;
        double s = std::sqrt(R[a][a] - R[b][b] - R[c][c] + 1.0);
        q[a] = 0.5 * s;
        s = 0.5 / s;
        q[3] = (R[c][b] - R[b][c]) * s;
        q[b] = (R[b][a] + R[a][b]) * s;
        q[c] = (R[c][a] + R[a][c]) * s;
      }
      std::fprintf(f, "%d %.9f %.9f %.9f %.9f %.9f %.9f %.9f\n", i, t[0], t[1], t[2], q[0], q[1], q[2], q[3]);
    }
    std::fclose(f);
    return DCORA_OK;
  });
}
int dcora_fixed_stiefel_variable(int r, int d, double *Y) {
  return abi_call({Y}, [&] {
    if (d < 1 || r < d) return bad("fixed_stiefel_variable: need r >= d >= 1");
    fixed_stiefel_variable(r, d, Y);
    return (int)DCORA_OK;
  });
}
int dcora_agent_initialize_in_global_frame(const dcora_dims *dims, const double *T_world_robot,
                                           const double *T_local, const double *YLift, double *X) {
  return abi_call({dims, T_world_robot, T_local, YLift, X}, [&] {
    if ((dims->d != 2 && dims->d != 3) || dims->r < dims->d || dims->n < 1) return bad("bad dims");
    if (!layout_ok(dims)) return bad("dims: layout SE needs l = b = 0");
    initialize_in_global_frame(dims->r, dims->d, dims->n, dims->l, dims->b, make_mani(*dims).se != 0, T_world_robot,
                               T_local, YLift, X);
    return (int)DCORA_OK;
  });
}
int dcora_measurement_errors(dcora_dataset_t ds, int r, const double *X, double *out, int device) {
  return abi_call({ds, X, out}, [&] {
    if (r < ds->ds.d || r > 16) return bad("measurement_errors: need d <= r <= 16");
    return measurement_errors(ds->ds, r, X, out, device);
  });
}
int dcora_ra_measurement_errors(dcora_radataset_t ds, int r, const double *X, double *out, int device) {
  return abi_call({ds, X, out}, [&] {
    if (r < ds->ds.d || r > 16) return bad("measurement_errors: need d <= r <= 16");
    return ra_measurement_errors(ds->ds, r, X, out, device);
  });
}
int dcora_solve_pgo(dcora_dataset_t ds, const dcora_ropt_params *params, const double *T0, double *Tout,
                    dcora_ropt_result *result, int device) {
  return abi_call({ds, params, Tout}, [&] { return solve_pgo(ds->ds, *params, T0, Tout, device, result); });
}
int dcora_solve_robust_pgo(dcora_dataset_t ds, const dcora_ropt_params *params, const dcora_robust_params *robust,
                           const int *fixed_weight, const double *T0, double *Tout, double *weights_out, int device) {
  return abi_call({ds, params, robust, Tout}, [&] {
    return solve_robust_pgo(ds->ds, *params, *robust, fixed_weight, T0, Tout, weights_out, device);
  });
}

// ---- rounding ----------------------------------------------------------------------------------------------
int dcora_round_align_trajectory(const dcora_dims *dims, const double *X, const double *anchor, int global_alignment,
                                 double *trajectory, double *unit_spheres, double *landmarks, int device) {
  return abi_call({dims, X, trajectory}, [&] {
    if (!layout_ok(dims)) return bad("dims: layout SE needs l = b = 0");
    return round_align(*dims, X, anchor, global_alignment, trajectory, unit_spheres, landmarks, device);
  });
}
int dcora_round_project_solution_raslam(const dcora_dims *dims, const double *X, double *out, int device) {
  return abi_call({dims, X, out}, [&] {
    if (!layout_ok(dims)) return bad("dims: layout SE needs l = b = 0");
    return round_project_solution(*dims, X, out, device);
  });
}

}  // extern "C"

// debug / test hook (not part of the public header): builds the partitioned inverse of an SPD matrix on the host
// and replays its schedule on the host against a plain sparse Cholesky solve -- checks the builder without a GPU.
// info = {levels (forward + backward), pieces, nnz(L), stored weights per apply}
extern "C" int dcora_debug_partinv_selftest(int n, const int *rp, const int *ci, const double *v, int block, int r,
                                            double *max_rel_err, double *info) {
  return abi_call({rp, ci, v, max_rel_err, info}, [&]() -> int {
    const HostCsr A = view_csr(n, rp, ci, v);
    PartInvHost P;
    if (!build_partitioned_inverse(A, block, 4, &P)) {
      set_last_error("matrix is not positive definite");
      return DCORA_ERR_NOT_PD;
    }
    SparseChol chol;
    if (!chol.factor(A, block)) return DCORA_ERR_NOT_PD;
    std::vector<double> R((size_t)n * r), Z((size_t)n * r), col((size_t)n), sol((size_t)n);
    unsigned long long s = 88172645463325252ull;
    for (double &x : R) {
      s ^= s << 13;
      s ^= s >> 7;
      s ^= s << 17;
      x = (double)(s >> 11) / 9007199254740992.0 - 0.5;
    }
    partitioned_inverse_apply_host(P, r, R.data(), Z.data());
    double err = 0, ref = 0;
    for (int t = 0; t < r; ++t) {
      for (int i = 0; i < n; ++i) col[i] = R[(size_t)i * r + t];
      chol.solve_vec(col.data(), sol.data());
      for (int i = 0; i < n; ++i) {
        err = std::max(err, std::fabs(sol[i] - Z[(size_t)i * r + t]));
        ref = std::max(ref, std::fabs(sol[i]));
      }
    }
    *max_rel_err = err / std::max(ref, 1e-300);
    info[0] = (double)P.levels.size();
    info[1] = (double)P.npieces;
    info[2] = (double)P.nnzL;
    info[3] = P.weights_read_per_apply;
    return DCORA_OK;
  });
}

// debug / test hook (not part of the public header): the stored weights of the same matrix once written to host memory
// in one piece and once STREAMED through a WeightSink in chunks of at most `cap` doubles (what the product does towards
// the device, DeviceWeightSink) -- runs without a GPU.  out = {weights, chunks, weights that differ, largest chunk}
extern "C" int dcora_debug_partinv_stream_check(int n, const int *rp, const int *ci, const double *v, int block,
                                                long long cap, double *out) {
  return abi_call({rp, ci, v, out}, [&]() -> int {
    const HostCsr A = view_csr(n, rp, ci, v);
    PartInvHost P, Q;
    if (!build_partitioned_inverse(A, block, 4, &P)) return DCORA_ERR_NOT_PD;
    struct HostSink : WeightSink {
      std::vector<double> all, buf;
      long long cap = 0, chunks = 0, largest = 0, expect = 0;
      bool ordered = true, ended = false;
      bool begin(long long total) override {
        all.assign((size_t)total, -12345.0);  // a weight the sink never receives keeps this value
        buf.resize((size_t)cap);
        return true;
      }
      long long chunk_cap() const override { return cap; }
      double *acquire(long long m) override {
        if (m > cap) return nullptr;
        std::fill(buf.begin(), buf.end(), 777.0);  // the builder must write (or zero) everything it commits
        return buf.data();
      }
      bool commit(long long off, long long m) override {
        ordered = ordered && off == expect;
        expect = off + m;
        ++chunks;
        largest = std::max(largest, m);
        std::copy(buf.begin(), buf.begin() + m, all.begin() + off);
        return true;
      }
      bool end() override {
        ended = true;
        return true;
      }
    } sink;
    sink.cap = cap;
    Q.sink = &sink;
    if (!build_partitioned_inverse(A, block, 3, &Q)) {
      set_last_error("the streamed build failed (a fill larger than the chunk?)");
      return DCORA_ERR_BAD_ARG;
    }
    long long differ = 0;
    if ((long long)P.vals.size() != Q.nvals || !Q.vals.empty() || !sink.ordered || !sink.ended ||
        sink.expect != Q.nvals)
      differ = -1;
    else
      for (size_t i = 0; i < P.vals.size(); ++i) differ += std::memcmp(&P.vals[i], &sink.all[i], sizeof(double)) != 0;
    out[0] = (double)Q.nvals;
    out[1] = (double)sink.chunks;
    out[2] = (double)differ;
    out[3] = (double)sink.largest;
    return DCORA_OK;
  });
}

// measurement hook (bench.py, SURVEY 8(d): "verify with a stream-triad on the box"): a[i] = b[i] + s c[i] over three
// arrays of n doubles, `reps` launches back to back between two HIP events; GB/s counts 24 n bytes per launch
namespace {
__global__ __launch_bounds__(256) void k_stream_triad(size_t n2, const double2 *__restrict__ b,
                                                      const double2 *__restrict__ c, double2 *__restrict__ a,
                                                      double s) {
  // four 16-byte loads per array in flight per lane
  const size_t stride = (size_t)gridDim.x * 256;
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + 3 * stride < n2; i += 4 * stride) {
    double2 x[4], y[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      x[u] = b[i + u * stride];
      y[u] = c[i + u * stride];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      a[i + u * stride] = make_double2(x[u].x + s * y[u].x, x[u].y + s * y[u].y);
  }
  for (; i < n2; i += stride) {
    const double2 x = b[i], y = c[i];
    a[i] = make_double2(x.x + s * y.x, x.y + s * y.y);
  }
}
}  // namespace
extern "C" int dcora_debug_stream_triad(int device, size_t n, int reps, double *gbps) {
  return abi_call({gbps}, [&]() -> int {
    if (no_device()) return DCORA_ERR_NO_DEVICE;
    DCORA_HIP(hipSetDevice(device));
    n &= ~(size_t)1;
    DevBuf<double> A, B, Cc;
    DCORA_HIP(A.alloc(n));
    DCORA_HIP(B.alloc(n));
    DCORA_HIP(Cc.alloc(n));
    DCORA_HIP(hipMemset(B.p, 0, n * sizeof(double)));
    DCORA_HIP(hipMemset(Cc.p, 0, n * sizeof(double)));
    hipEvent_t e0, e1;
    DCORA_HIP(hipEventCreate(&e0));
    DCORA_HIP(hipEventCreate(&e1));
    const int grid = 1024;  // 1024 / 2048 / 8192 workgroups: 5.01 / 4.85 / 4.48 TB/s
    for (int w = 0; w < 3; ++w)
      hipLaunchKernelGGL(k_stream_triad, dim3(grid), dim3(256), 0, nullptr, n / 2, (const double2 *)B.p,
                         (const double2 *)Cc.p, (double2 *)A.p, 0.5);
    DCORA_HIP(hipEventRecord(e0, nullptr));
    for (int w = 0; w < reps; ++w)
      hipLaunchKernelGGL(k_stream_triad, dim3(grid), dim3(256), 0, nullptr, n / 2, (const double2 *)B.p,
                         (const double2 *)Cc.p, (double2 *)A.p, 0.5);
    DCORA_HIP(hipEventRecord(e1, nullptr));
    DCORA_HIP(hipEventSynchronize(e1));
    float ms = 0;
    DCORA_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *gbps = 24.0 * (double)n * reps / (ms * 1e-3) / 1e9;
    return DCORA_OK;
  });
}
