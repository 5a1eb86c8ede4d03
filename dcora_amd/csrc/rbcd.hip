// RBCD++ session on the device (see rbcd.h).
#include "rbcd.h"
#include "env.h"
#include "host_threads.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <set>

namespace dcora {

static bool group_kernels(const ManiDesc &m) {
  return group_supported(m) && !env::generic_solver();
}

static void nesterov(hipStream_t st, const ManiDesc &m, int mode, int restart, int skip_lo, int skip_hi, double alpha,
                     double gamma, double *X, double *V, double *Y, double *XPrev, double *Yloc, Buf2 Xloc,
                     const SolverCtl *ctl) {
  if (group_kernels(m))
    launch_g_nesterov(st, m, mode, restart, skip_lo, skip_hi, alpha, gamma, X, V, Y, XPrev, Yloc, Xloc, ctl);
  else  // thread-per-pose kernels: the caller resolved the result pointer (ctl == nullptr)
    launch_nesterov(st, m, mode, restart & 1, skip_lo, skip_hi, alpha, gamma, X, V, Y, XPrev, Yloc, Xloc.p[0]);
}

// Nesterov bookkeeping whose X is the result of pb's last solve: the 8-lanes-per-pose kernels pick its buffer on the
// device, the thread-per-pose ones take it resolved on the host
static int nesterov_solved(hipStream_t st, DeviceProblem &pb, int mode, double alpha, double gamma, double *X,
                           double *V, double *Y, double *XPrev) {
  const SolverCtl *c = nullptr;
  Buf2 Xres = pb.result_pick(&c);
  if (!group_kernels(pb.m)) {
    const int rc = pb.result(&Xres.p[0]);
    if (rc) return rc;
    c = nullptr;
  }
  nesterov(st, pb.m, mode, 0, -1, -1, alpha, gamma, X, V, Y, XPrev, nullptr, Xres, c);
  return DCORA_OK;
}

namespace {
constexpr double kPrecondReg = 0.1;  // reg = 1e-1 of the agents' (Q_bb + reg I)^-1, ref src/Graph.cpp:1906
constexpr int kAgentThreads = 8;     // host threads of the per-agent set-up work, at most

// the first failing agent's status, its text as the last error
int first_failure(const std::vector<int> &rcs, const std::vector<std::string> &errs) {
  for (size_t i = 0; i < rcs.size(); ++i)
    if (rcs[i]) {
      set_last_error(errs[i]);
      return rcs[i];
    }
  return DCORA_OK;
}
}  // namespace

// Measurements with global pose indices as the host builders take them (the partition, ref
// examples/MultiRobotExample.cpp:56-118): touching[b], with owners and local indices, is what agent b's Q_bb is built
// from; global (r1 = r2 = 0) what the coupling blocks and the central Q are built from
struct RbcdSession::MeasSplit {
  std::vector<std::vector<PoseMeas>> touching;
  std::vector<PoseMeas> global;
  MeasSplit(const std::vector<PoseMeas> &meas, const Partition &P) : touching((size_t)P.R), global(meas) {
    for (PoseMeas e : meas) {
      e.r1 = P.robot_of(e.p1);
      e.r2 = P.robot_of(e.p2);
      e.p1 -= P.start(e.r1);
      e.p2 -= P.start(e.r2);
      touching[(size_t)e.r1].push_back(e);
      if (e.r2 != e.r1) touching[(size_t)e.r2].push_back(e);
    }
    for (PoseMeas &e : global) e.r1 = e.r2 = 0;
  }
};

RbcdSession::~RbcdSession() {
  if (eval_host) (void)hipHostFree((void *)eval_host);
  if (x_stage) (void)hipHostFree((void *)x_stage);
  team.reset();
  for (AgentDev &a : agents) release_tick_resources(a);
  agents.clear();
  central.reset();
  release_stream();
}

int RbcdSession::init(const HostDataset &ds, const dcora_rbcd_options &o) {
  t0_ = std::chrono::steady_clock::now();
  opt = o;
  chain_rides_ = env::chain_rides();
  d = ds.d;
  n = ds.n;
  r = o.r;
  R = o.num_robots;
  if (R < 1 || n / R < 1 || o.world_size < 1 || o.rank < 0 || o.rank >= o.world_size) {
    set_last_error("rbcd: bad num_robots / rank / world_size");
    return DCORA_ERR_BAD_ARG;
  }
  if (o.acceleration && o.restart_interval < 1) {
    set_last_error("rbcd: acceleration needs restart_interval >= 1 (AgentParameters::restartInterval)");
    return DCORA_ERR_BAD_ARG;
  }
  if (r < d || r > 16) {
    set_last_error("rbcd: relaxation rank must satisfy d <= r <= 16");
    return DCORA_ERR_BAD_ARG;
  }
  P.R = R;
  P.n = n;
  P.per = n / R;
  const int dh = d + 1;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    set_last_error("no HIP device available: libdcora_hip has no CPU fallback");
    return DCORA_ERR_NO_DEVICE;
  }
  DCORA_HIP(hipSetDevice(o.device));
  {
    const int rcs = acquire_stream(o.stream);
    if (rcs) return rcs;
  }
  mg = make_mani(r, d, n, 0, 0);
  const size_t N = (size_t)r * dh * n;
  DCORA_HIP(Xg.alloc(N));
  DCORA_HIP(Vg.alloc(N));
  DCORA_HIP(Yg.alloc(N));
  DCORA_HIP(XPrevg.alloc(N));
  if (R > kMaxAgents) {
    set_last_error("rbcd: more agents than kMaxAgents");
    return DCORA_ERR_UNSUPPORTED;
  }
  DCORA_HIP(posenorm.alloc(n));
  DCORA_HIP(eval_split.alloc((size_t)eval_split_doubles()));
  DCORA_HIP(hipHostMalloc((void **)&eval_host, sizeof(EvalOut), hipHostMallocMapped));
  std::memset((void *)eval_host, 0, sizeof(EvalOut));
  DCORA_HIP(hipHostGetDevicePointer((void **)&eval_dev, (void *)eval_host, 0));
  DCORA_HIP(hipHostMalloc((void **)&x_stage, sizeof(double) * N, hipHostMallocDefault));
  // the first device-to-host copy of a process pays ~8 ms of runtime set-up: pay it here, not in get_X
  DCORA_HIP(hipMemcpyAsync(x_stage, Xg.p, sizeof(double) * N, hipMemcpyDeviceToHost, st));
  DCORA_HIP(hipStreamSynchronize(st));
  DCORA_HIP(evalbuf.alloc(2 * R + 16));
  DCORA_HIP(hipMemset(evalbuf.p, 0, sizeof(double) * (2 * R + 16)));

  lap("buffers");
  const MeasSplit split(ds.meas, P);
  for (size_t e = 0; e < ds.meas.size(); ++e) {
    const PoseMeas &q = ds.meas[e];
    const int r1 = P.robot_of(q.p1), r2 = P.robot_of(q.p2);
    if (r1 == r2 && q.p2 == q.p1 + 1) continue;  // odometry
    team_lcs_.push_back(TeamLoopClosure{(int)e, r1, r2, q.weight});
  }
  agents.resize(R);
  std::vector<int> cs(R + 1);
  for (int b = 0; b < R; ++b) {
    AgentDev &a = agents[b];
    a.id = b;
    a.n = P.end(b) - P.start(b);
    a.col0 = P.start(b) * dh;
    cs[b] = a.col0;
    a.hosted = (b / ((R + o.world_size - 1) / o.world_size)) == o.rank;  // consecutive agents share a rank
    // my public poses, my neighbours and the poses of theirs that I require: the two ends of every measurement of
    // mine that another agent shares
    std::set<int> pub, nb, req;
    for (const PoseMeas &e : split.touching[(size_t)b]) {
      if (e.r1 == e.r2) continue;
      const bool first = e.r1 == b;
      const int other = first ? e.r2 : e.r1;
      pub.insert(P.start(b) + (first ? e.p1 : e.p2));
      req.insert(P.start(other) + (first ? e.p2 : e.p1));
      nb.insert(other);
    }
    a.public_poses.assign(pub.begin(), pub.end());
    a.neighbors.assign(nb.begin(), nb.end());
    a.required.assign(req.begin(), req.end());
    std::vector<int> cols;
    for (int p : a.public_poses)
      for (int c = 0; c < dh; ++c) cols.push_back(p * dh + c);
    a.n_public_cols = (int)cols.size();
    DCORA_HIP(a.public_cols.alloc(std::max<size_t>(cols.size(), 1)));
    if (!cols.empty())
      DCORA_HIP(hipMemcpy(a.public_cols.p, cols.data(), sizeof(int) * cols.size(), hipMemcpyHostToDevice));
  }
  // the pose / column offsets of the agents: uploaded before the builds (a copy queued behind them waited 16 ms)
  cs[R] = dh * n;
  {
    std::vector<int> ps(R + 1);
    for (int b = 0; b <= R; ++b) ps[b] = cs[b] / dh;
    DCORA_HIP(pose_start.alloc(R + 1));
    DCORA_HIP(col_start.alloc(R + 1));
    DCORA_HIP(hipMemcpyAsync(pose_start.p, ps.data(), sizeof(int) * (R + 1), hipMemcpyHostToDevice, st));
    DCORA_HIP(hipMemcpyAsync(col_start.p, cs.data(), sizeof(int) * (R + 1), hipMemcpyHostToDevice, st));
    DCORA_HIP(hipStreamSynchronize(st));
  }
  if (const int rcf = create_fork_event()) return rcf;
  const int rc = assemble(
      split, nullptr,
      [&](const Assembly &A) {
        return attach_preconditioners(A.Q, [&](size_t i) {
          AgentDev &a = agents[(size_t)A.ids[i]];
          a.prob.reset(new DeviceProblem);
          int rca = a.prob->init(dcora_dims{r, d, a.n, 0, 0}, A.Q[i], nullptr, kPrecondReg, o.device, st);
          if (!rca) rca = a.coupling.upload(A.C[i]);
          if (!rca && robust) {
            robust->Qpat[(size_t)a.id] = pattern_of(A.Q[i]);
            robust->Cpat[(size_t)a.id] = pattern_of(A.C[i]);
          }
          return rca ? rca : acquire_tick_resources(a);
        });
      },
      [&](const HostCsr &Qc) {  // (the evaluation's problem: Q of all poses, no preconditioner)
        central.reset(new DeviceProblem);
        if (robust) robust->central_pat = pattern_of(Qc);
        return central->init(dcora_dims{r, d, n, 0, 0}, Qc, nullptr, -1.0, o.device, st);
      });
  if (rc) return rc;
  lap("agents built");
  lap("ready");
  iteration = 0;
  gamma = alpha = 0;
  setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0_).count();
  return DCORA_OK;
}

// "[session] <what> after <ms since init began>" under DCORA_INIT_TIMING; silent once init has set setup_ms
void RbcdSession::lap(const char *what) const {
  if (setup_ms == 0 && env::init_timing())
    fprintf(stderr, "[session] %s after %.1f ms\n", what,
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0_).count());
}

// The one path from a measurement list to the session's host matrices, at creation and on every re-weight: Q_bb and
// the coupling block of each hosted agent and, in a single-process session, the central Q, all from the host builders.
// The agents' matrices are built side by side on host threads (a matrix takes a millisecond of host work); each(i, A),
// if given, runs on the thread that built those of agent A.ids[i], agents_ready(A) once all of them stand.  The
// whole-graph problem of the evaluation depends on none of the agents: its assembly (0.15 s of one host thread for the
// 100k lattice) and central_ready(Qc) run on a thread of their own beside all of that.  The agents' status is reported
// before the central problem's.
int RbcdSession::assemble(const MeasSplit &split, const std::function<void(size_t, const Assembly &)> &each,
                          const std::function<int(const Assembly &)> &agents_ready,
                          const std::function<int(const HostCsr &)> &central_ready) {
  Assembly A;
  for (const AgentDev &a : agents)
    if (a.hosted) A.ids.push_back(a.id);
  const int nh = (int)A.ids.size();
  A.Q.resize((size_t)nh);
  A.C.resize((size_t)nh);
  int rc = DCORA_OK, central_rc = DCORA_OK;
  std::string central_err;
  run_threads(2, [&](int t) {
    if (t == 0) {
      parallel_for(nh, kAgentThreads, 1, [&](int i) {
        const int b = A.ids[(size_t)i];
        A.Q[(size_t)i] = build_Q_pgo(d, agents[(size_t)b].n, b, split.touching[(size_t)b]);
        A.C[(size_t)i] = build_coupling_pgo(d, P, b, split.global);
        if (each) each((size_t)i, A);
      });
      rc = agents_ready(A);
    } else if (opt.world_size == 1) {
      if (hipSetDevice(opt.device) != hipSuccess) {
        central_rc = DCORA_ERR_HIP;
        central_err = "hipSetDevice failed";
        return;
      }
      central_rc = central_ready(build_Q_pgo(d, n, 0, split.global));
      if (central_rc) central_err = dcora_last_error();
    } else if (job_pat.n == 0) {
      // a rank of a job, at creation: no central problem, but the whole Q's pattern is what the job-wide certificate is
      // laid out on (Exchange::certify_live) -- taken here, beside the agents' builds, and never again
      job_pat = pattern_of(build_Q_pgo(d, n, 0, split.global));
    }
  });
  if (rc) return rc;
  if (central_rc) set_last_error(central_err);
  return central_rc;
}

// The preconditioners of the hosted agents' matrices Q (index i as in Assembly).  Blocks small enough for the dense
// inverse: all inverses in ONE batch of launches first (five builds on five streams do not overlap), so that the
// problems attach to the cached images.  Then attach(i) for every agent: DeviceProblem::init at creation,
// build_preconditioner on a re-weight.  The factorisation of one large block is partly serial (the separators above
// the sub-trees): eight blocks of the 100k lattice take 9 s one after the other and 2-3 s side by side on host
// threads; small blocks take well under a millisecond of host work each, where threads do not pay off.
int RbcdSession::attach_preconditioners(const std::vector<HostCsr> &Q, const std::function<int(size_t)> &attach) {
  const int nh = (int)Q.size(), dh = d + 1;
  const bool dense_batch = (long)(n / R + 1) * dh <= kDensePrecondMaxK && nh > 1;
  const bool threads_pay = (long)(n / R) * dh >= 1024;
  if (dense_batch) {
    std::vector<const HostCsr *> ptrs;
    for (const HostCsr &Qi : Q) ptrs.push_back(&Qi);
    const int prc = precond_prebuild_dense(ptrs, kPrecondReg, dh, opt.device);
    if (prc) return prc;
    lap("dense inverses prebuilt");
  }
  std::vector<int> rcs((size_t)nh, DCORA_OK);
  std::vector<std::string> errs((size_t)nh);
  parallel_for(nh, threads_pay ? kAgentThreads : 1, 1, [&](int i) {
    if (hipSetDevice(opt.device) != hipSuccess) {
      rcs[(size_t)i] = DCORA_ERR_HIP;
      return;
    }
    rcs[(size_t)i] = attach((size_t)i);
    if (rcs[(size_t)i]) errs[(size_t)i] = dcora_last_error();
  });
  return first_failure(rcs, errs);
}

// Agent::setX + initializeAcceleration for every agent (ref src/Agent.cpp:64-77, 1178-1187)
int RbcdSession::set_X(const double *Xh) { return adopt_X(Xh, hipMemcpyHostToDevice); }

int RbcdSession::adopt_X(const double *X, hipMemcpyKind kind) {
  staged_selected_ = -1;  // a step staged by an interrupted round does not survive a new start point
  DCORA_HIP(hipSetDevice(opt.device));
  const size_t B = sizeof(double) * (size_t)r * (d + 1) * n;
  DCORA_HIP(hipMemcpyAsync(Xg.p, X, B, kind, st));
  DCORA_HIP(hipMemcpyAsync(Vg.p, Xg.p, B, hipMemcpyDeviceToDevice, st));
  DCORA_HIP(hipMemcpyAsync(Yg.p, Xg.p, B, hipMemcpyDeviceToDevice, st));
  DCORA_HIP(hipMemcpyAsync(XPrevg.p, Xg.p, B, hipMemcpyDeviceToDevice, st));
  if (robust) DCORA_HIP(hipMemcpyAsync(robust->X_initial.p, Xg.p, B, hipMemcpyDeviceToDevice, st));
  DCORA_HIP(hipStreamSynchronize(st));
  gamma = alpha = 0;
  iteration = 0;
  seq_advanced_ = false;
  pending_reset_ = false;
  agent_it.assign(R, 0);
  set_marks_.assign(R, 0);
  team_restart_rounds();
  for (AgentDev &a : agents) a.v_feasible = false;  // V = X as handed over: projected in the next round
  return DCORA_OK;
}
// initializeAcceleration / acceleration off for every agent (ref src/Agent.cpp:1178-1187)
int RbcdSession::set_acceleration(bool on) {
  staged_selected_ = -1;
  DCORA_HIP(hipSetDevice(opt.device));
  opt.acceleration = on ? 1 : 0;
  const size_t B = sizeof(double) * (size_t)r * (d + 1) * n;
  DCORA_HIP(hipMemcpyAsync(Vg.p, Xg.p, B, hipMemcpyDeviceToDevice, st));
  DCORA_HIP(hipMemcpyAsync(Yg.p, Xg.p, B, hipMemcpyDeviceToDevice, st));
  DCORA_HIP(hipMemcpyAsync(XPrevg.p, Xg.p, B, hipMemcpyDeviceToDevice, st));
  gamma = alpha = 0;
  iteration = 0;
  seq_advanced_ = false;
  pending_reset_ = false;
  agent_it.assign(R, 0);
  set_marks_.assign(R, 0);
  team_restart_rounds();
  for (AgentDev &a : agents) a.v_feasible = false;
  return DCORA_OK;
}
int RbcdSession::get_X(double *Xh) {
  DCORA_HIP(hipSetDevice(opt.device));
  const size_t B = sizeof(double) * (size_t)r * (d + 1) * n;
  // through a pinned staging buffer: an asynchronous copy into pageable memory takes milliseconds on this runtime
  if (!x_stage) DCORA_HIP(hipHostMalloc((void **)&x_stage, B, hipHostMallocDefault));
  DCORA_HIP(hipMemcpyAsync(x_stage, Xg.p, B, hipMemcpyDeviceToHost, st));
  DCORA_HIP(hipStreamSynchronize(st));
  std::memcpy(Xh, x_stage, B);
  return DCORA_OK;
}

// ---- the staircase step in place: SessionCore::lift's hooks -------------------------------------------------------
int RbcdSession::lift_default_reg(const HostCsr &, double *reg) {
  *reg = kPrecondReg;
  return DCORA_OK;
}

int RbcdSession::lift_buffers(int r_new) {
  const size_t N = (size_t)r_new * (d + 1) * n;
  DevBuf<double> X, V, Y, XP, XI;
  for (DevBuf<double> *b : {&X, &V, &Y, &XP}) DCORA_HIP(b->alloc(N));
  if (robust) DCORA_HIP(XI.alloc(N));
  double *stage_new = nullptr;
  DCORA_HIP(hipHostMalloc((void **)&stage_new, sizeof(double) * N, hipHostMallocDefault));
  // the swap: nothing below fails
  Xg = std::move(X);
  Vg = std::move(V);
  Yg = std::move(Y);
  XPrevg = std::move(XP);
  if (robust) robust->X_initial = std::move(XI);
  if (x_stage) (void)hipHostFree((void *)x_stage);
  x_stage = stage_new;
  r = r_new;
  opt.r = r_new;
  mg = make_mani(r, d, n, 0, 0);
  for (AgentDev &a : agents) {  // handed neighbour poses have the old rank: the agents read the mirror again
    a.detached = false;
    a.last_skipped = false;
    for (int w = 0; w < 2; ++w) {
      a.nbr[w].release();
      a.got[w].clear();
    }
  }
  return DCORA_OK;
}

AgentBlock RbcdSession::agent_block(int id) {
  const AgentDev &a = agents[(size_t)id];
  AgentBlock blk;
  blk.X = Xg.p + (size_t)a.col0 * r;
  blk.k = (d + 1) * a.n;
  blk.n = a.n;
  blk.col0 = a.col0;
  return blk;
}

// ---- robust sessions (RobustState, session_core.h): what is this kind's own -----------------------------------------
// A loop closure is every measurement but odometry, i.e. but p2 == p1 + 1 inside one agent of the contiguous partition
// (driver.loop_closure_mask).  A rank of a multi-rank job (ranked) builds the patterns of its hosted agents only and
// uploads the edges touching them.
int RbcdSession::init_robust(const HostDataset &ds, const dcora_rbcd_options &o, const dcora_robust_params &p,
                             const int *fixed, bool ranked) {
  if (o.num_robots < 1 || ds.n / o.num_robots < 1) {
    set_last_error("rbcd: bad num_robots / rank / world_size");
    return DCORA_ERR_BAD_ARG;
  }
  int rc = robust_check_args(ds.meas, ds.n, o, p, ranked);
  if (rc) return rc;
  Partition Pt;
  Pt.R = o.num_robots;
  Pt.n = ds.n;
  Pt.per = ds.n / o.num_robots;
  const size_t m = ds.meas.size();
  std::vector<char> lc(m);
  for (size_t e = 0; e < m; ++e) {
    const PoseMeas &q = ds.meas[e];
    lc[e] = !(Pt.robot_of(q.p1) == Pt.robot_of(q.p2) && q.p2 == q.p1 + 1);
  }
  robust_begin(ds.meas, lc, p, fixed, ranked);
  robust_ds_ = ds;
  for (size_t e = 0; e < m; ++e) robust_ds_.meas[e].weight = robust->w[e];
  robust->Qpat.assign((size_t)o.num_robots, HostCsr());
  robust->Cpat.assign((size_t)o.num_robots, HostCsr());
  rc = init(robust_ds_, o);
  return rc ? rc : robust_finish();
}

// the edges touching a hosted agent (a single process: all); the rank owns those whose p1 it hosts
int RbcdSession::robust_upload_edges() {
  RobustState &rs = *robust;
  std::vector<char> own;
  for (size_t e = 0; e < robust_ds_.meas.size(); ++e) {
    const PoseMeas &q = robust_ds_.meas[e];
    const bool h1 = agents[(size_t)P.robot_of(q.p1)].hosted, h2 = agents[(size_t)P.robot_of(q.p2)].hosted;
    rs.owned[e] = h1 ? 1 : 0;
    if (!h1 && !h2) continue;
    rs.edge_ids.push_back((int)e);
    own.push_back(rs.owned[e]);
  }
  return rs.ranked ? rs.edges.upload_ranked(robust_ds_, rs.update, rs.edge_ids, own)
                   : rs.edges.upload(robust_ds_, rs.update);
}

// Through the assembly of creation.  The matrices as the builders give them (no explicit zeros) go to the
// preconditioners, so the cache sees the keys of a fresh session: a new image is attached, an image somebody else still
// holds is never written.  Their values scattered onto the creation patterns (a weight of 0 leaves explicit zeros) are
// what is uploaded.  Together: every value of the re-weighted session equals a fresh session's bit for bit.
int RbcdSession::robust_rebuild(const std::vector<double> &w) {
  RobustState &rs = *robust;
  std::vector<PoseMeas> meas = robust_ds_.meas;
  for (size_t e = 0; e < meas.size(); ++e) meas[e].weight = w[e];
  const char *outside = "rbcd robust: the weights give a matrix entry outside the session's pattern";
  // host images of the uploads (by agent id), alive until the stream has been synchronised
  std::vector<HostCsr> Qs((size_t)R), Cs((size_t)R);
  std::vector<std::vector<double>> stage((size_t)R);
  std::vector<char> ok((size_t)R, 1);
  HostCsr Qcs;
  std::vector<double> cstage;
  const int rc = assemble(
      MeasSplit(meas, P),
      [&](size_t i, const Assembly &A) {
        const size_t b = (size_t)A.ids[i];
        ok[b] = scatter_on_pattern(A.Q[i], rs.Qpat[b], &Qs[b]) && scatter_on_pattern(A.C[i], rs.Cpat[b], &Cs[b]);
      },
      [&](const Assembly &A) {
        if (std::count(ok.begin(), ok.end(), 0)) {
          set_last_error(outside);
          return (int)DCORA_ERR_BAD_ARG;
        }
        return attach_preconditioners(A.Q, [&](size_t i) {
          const size_t b = (size_t)A.ids[i];
          int rca = agents[b].prob->set_values(Qs[b], st, &stage[b]);
          if (!rca) rca = agents[b].coupling.set_values(Cs[b], st);
          return rca ? rca : agents[b].prob->build_preconditioner(A.Q[i], kPrecondReg);
        });
      },
      [&](const HostCsr &Qc) {
        if (scatter_on_pattern(Qc, rs.central_pat, &Qcs)) return central->set_values(Qcs, st, &cstage);
        set_last_error(outside);
        return (int)DCORA_ERR_BAD_ARG;
      });
  const hipError_t synced = hipStreamSynchronize(st);  // (also after a failure: copies may be in flight)
  if (rc) return rc;
  DCORA_HIP(synced);
  return DCORA_OK;
}

// no staged Nesterov step; unlike set_acceleration the iteration counter goes on (mIterationNumber)
int RbcdSession::robust_restart_acceleration() {
  staged_selected_ = -1;
  const size_t B = sizeof(double) * (size_t)r * (d + 1) * n;
  DCORA_HIP(hipMemcpyAsync(Vg.p, Xg.p, B, hipMemcpyDeviceToDevice, st));
  DCORA_HIP(hipMemcpyAsync(Yg.p, Xg.p, B, hipMemcpyDeviceToDevice, st));
  DCORA_HIP(hipMemcpyAsync(XPrevg.p, Xg.p, B, hipMemcpyDeviceToDevice, st));
  DCORA_HIP(hipStreamSynchronize(st));
  gamma = alpha = 0;
  seq_advanced_ = false;
  pending_reset_ = false;
  for (AgentDev &a : agents) a.v_feasible = false;
  return DCORA_OK;
}

// Agent::iterate(false) for every hosted agent except `selected`
int RbcdSession::phase_nonselected(int selected) {
  if (const int rc = check_selected(selected)) return rc;
  DCORA_HIP(hipSetDevice(opt.device));
  advance_sequences();
  seq_advanced_ = true;
  set_marks_.assign(R, 0);
  staged_selected_ = -1;
  if (!opt.acceleration) return DCORA_OK;
  // bit 1: after the first round every V is the output of a projection (or a copy of X): skip its re-projection.
  // An Agent::setX of a single agent (which may hand over an X that is not exactly feasible) clears the flag until
  // the next round has projected every V again.
  bool all_feasible = true;
  for (const AgentDev &a : agents)
    if (a.id != selected) all_feasible = all_feasible && a.v_feasible;
  const int restart = (restart_now() ? 1 : 0) | (all_feasible ? 2 : 0);
  if (opt.world_size == 1) {
    // one launch over the whole graph; the selected agent's poses take their own step of the same kernel (Y and the
    // local solver's start point <- proj((1 - alpha) X + alpha V), what update_selected_agent would launch next)
    if (group_kernels(mg) && agents[selected].hosted && agents[selected].prob) {
      launch_g_nesterov(st, mg, 0, restart, P.start(selected), P.end(selected), alpha, gamma, Xg.p, Vg.p, Yg.p, XPrevg.p,
                        nullptr, Buf2{{nullptr, nullptr}}, nullptr, agents[selected].prob->X0.p);
      staged_selected_ = selected;
      staged_iteration_ = iteration;
    } else {
      nesterov(st, mg, 0, restart, P.start(selected), P.end(selected), alpha, gamma, Xg.p, Vg.p, Yg.p, XPrevg.p, nullptr,
               Buf2{{nullptr, nullptr}}, nullptr);
    }
    for (AgentDev &a : agents)
      if (a.id != selected) a.v_feasible = true;
  } else {
    for (AgentDev &a : agents) {
      if (!a.hosted || a.id == selected) continue;
      const int rc = update_nonselected_agent(a, (restart & 1) != 0);
      if (rc) return rc;
    }
  }
  return DCORA_OK;
}

int RbcdSession::update_nonselected_agent(AgentDev &a, bool restart) {
  const size_t off = (size_t)a.col0 * r;
  // bit 1: V is known to be feasible (output of a projection since the agent's last setX): skip its re-projection
  nesterov(st, a.prob->m, 0, (restart ? 1 : 0) | (a.v_feasible ? 2 : 0), -1, -1, alpha, gamma, Xg.p + off, Vg.p + off,
           Yg.p + off, XPrevg.p + off, nullptr, Buf2{{nullptr, nullptr}}, nullptr);
  a.v_feasible = true;
  return DCORA_OK;
}

// Agent::iterate(true) for `selected` when hosted here (ref src/Agent.cpp:535-551, 1158-1176, 1216-1278)
int RbcdSession::phase_selected(int selected) {
  if (const int rc = check_selected(selected)) return rc;
  DCORA_HIP(hipSetDevice(opt.device));
  if (!seq_advanced_) advance_sequences();
  seq_advanced_ = false;
  const bool restart = restart_now();
  AgentDev &a = agents[selected];
  if (a.hosted) {
    int rc = update_selected_agent(a, restart);
    if (!rc && team) rc = team_note_optimized(&selected, 1);
    if (rc) return rc;
  }
  if (restart) gamma = alpha = 0;
  return DCORA_OK;
}

// which: the plain (0) or the auxiliary (1) cache of a detached agent holds every pose the agent requires
static bool cache_complete(const AgentDev &a, int which) {
  return std::find(a.got[which].begin(), a.got[which].end(), 0) == a.got[which].end();
}

// restartNesterovAcceleration of the selected agent: X = XPrev; updateX(true, false), which for a detached agent reads
// the PLAIN cache (ref src/Agent.cpp:1237-1240); V = X; Y = X.  No G can be built from an incomplete cache: then
// X = XPrev without the solve.  `success` of Agent::iterate is the FIRST updateX's result, this one's is discarded (ref
// src/Agent.cpp:548-553): last_skipped stays what that one left.
int RbcdSession::restart_step(AgentDev &a) {
  DeviceProblem &pb = *a.prob;
  const size_t off = (size_t)a.col0 * r;
  if (a.detached && !cache_complete(a, 0)) {
    const Buf2 Xprev{{XPrevg.p + off, XPrevg.p + off}};
    nesterov(st, pb.m, 3, 0, -1, -1, alpha, gamma, Xg.p + off, Vg.p + off, Yg.p + off, XPrevg.p + off, nullptr, Xprev,
             nullptr);
    return DCORA_OK;
  }
  if (a.detached)
    launch_spmm(st, r, a.coupling.view(), buf1(a.nbr[0].p), 0, nullptr, buf1(pb.G.p), 0, nullptr, Gate{});
  pb.has_G = true;
  last_solver = &pb;
  DCORA_HIP(hipMemcpyAsync(pb.X0.p, XPrevg.p + off, sizeof(double) * (size_t)pb.nelem(), hipMemcpyDeviceToDevice, st));
  const int rc = pb.optimize_dev(opt.local);
  return rc ? rc : nesterov_solved(st, pb, 3, alpha, gamma, Xg.p + off, Vg.p + off, Yg.p + off, XPrevg.p + off);
}

int RbcdSession::update_selected_agent(AgentDev &a, bool restart) {
  int rc = DCORA_OK;
  {
    DeviceProblem &pb = *a.prob;
    const size_t off = (size_t)a.col0 * r;
    const size_t B = sizeof(double) * (size_t)pb.nelem();
    // Graph::constructLinearCostTermPGO: G_b = sum_c X_c Q_cb from the neighbours' public poses
    // (ref src/Graph.cpp:685-822); the mirror Xg holds them after the pull / unpack -- or, for an agent that has been
    // handed poses through Agent::updateNeighborStates, its own cache of them: the auxiliary one when it optimises
    // from Y (ref src/Agent.cpp:1234-1240)
    a.last_skipped = false;
    if (a.detached && !cache_complete(a, opt.acceleration ? 1 : 0)) {
      // "cannot construct data matrices... Skip optimization" (ref src/Agent.cpp:1243-1249): only updateX is skipped;
      // updateGamma / updateAlpha / updateY have run before it and updateV and the restart follow (Agent::iterate, ref
      // src/Agent.cpp:535-596) -- X stays, Y <- proj((1 - alpha) X + alpha V), V <- proj(V + gamma (X - Y))
      a.last_skipped = true;
      if (opt.acceleration) {
        if (staged_selected_ != a.id || staged_iteration_ != iteration)
          nesterov(st, pb.m, 1, 0, -1, -1, alpha, gamma, Xg.p + off, Vg.p + off, Yg.p + off, XPrevg.p + off, pb.X0.p,
                   Buf2{{nullptr, nullptr}}, nullptr);
        staged_selected_ = -1;
        const Buf2 Xself{{Xg.p + off, Xg.p + off}};
        nesterov(st, pb.m, 2, 0, -1, -1, alpha, gamma, Xg.p + off, Vg.p + off, Yg.p + off, XPrevg.p + off, nullptr, Xself,
                 nullptr);
        a.v_feasible = true;
        if (restart) return restart_step(a);
      }
      return DCORA_OK;
    }
    const double *nsrc = a.detached ? a.nbr[opt.acceleration ? 1 : 0].p : Xg.p;
    // (chain: G is formed by the solve's start-point evaluation where that is k_fused_grad)
    const CsrDev Cv = a.coupling.view();
    if (chain_rides_ && !a.detached && Cv.n_long == 0)
      pb.ride_G(Cv, nsrc);
    else
      launch_spmm(st, r, Cv, buf1(nsrc), 0, nullptr, buf1(pb.G.p), 0, nullptr, Gate{});
    pb.has_G = true;
    last_solver = &pb;
    if (opt.acceleration) {
      // (skipped only when the non-selected agents' launch of THIS round has taken the step already)
      if (staged_selected_ != a.id || staged_iteration_ != iteration)
        nesterov(st, pb.m, 1, 0, -1, -1, alpha, gamma, Xg.p + off, Vg.p + off, Yg.p + off, XPrevg.p + off, pb.X0.p,
                 Buf2{{nullptr, nullptr}}, nullptr);
      staged_selected_ = -1;
      rc = pb.optimize_dev(opt.local);
      if (!rc) rc = nesterov_solved(st, pb, 2, alpha, gamma, Xg.p + off, Vg.p + off, Yg.p + off, XPrevg.p + off);
      if (rc) return rc;
      a.v_feasible = true;  // V = proj(V + gamma (X - Y))
      if (restart) return restart_step(a);
    } else {
      DCORA_HIP(hipMemcpyAsync(XPrevg.p + off, Xg.p + off, B, hipMemcpyDeviceToDevice, st));
      DCORA_HIP(hipMemcpyAsync(pb.X0.p, Xg.p + off, B, hipMemcpyDeviceToDevice, st));
      double *Xres = nullptr;  // resolved on the host: the non-accelerated path is not latency critical
      if ((rc = pb.optimize_dev(opt.local)) || (rc = pb.result(&Xres))) return rc;
      DCORA_HIP(hipMemcpyAsync(Xg.p + off, Xres, B, hipMemcpyDeviceToDevice, st));
    }
  }
  return DCORA_OK;
}

// Agent::iterate(doOptimization) of one agent (ref src/Agent.cpp:535-596).  The driver calls every agent once per
// round (examples/MultiRobotExample.cpp:223-262): the first call of a round advances the shared gamma / alpha
// sequences (identical for all agents, :1189-1200), a restart round zeroes them when the next round begins.
int RbcdSession::agent_iterate(int agent, bool do_optimization) {
  staged_selected_ = -1;  // the per-agent API never rides in a whole-graph launch
  if (agent < 0 || agent >= R) {
    set_last_error("rbcd: agent out of range");
    return DCORA_ERR_BAD_ARG;
  }
  AgentDev &a = agents[agent];
  if (!a.hosted) {
    set_last_error("rbcd: agent is hosted by another rank");
    return DCORA_ERR_BAD_ARG;
  }
  if (team && team->ranked) {
    set_last_error("rbcd team: the agents of a multi-rank team optimise through their exchange "
                   "(dcora_exchange_rbcd_iterate / _rbcd_tick), which carries their statuses to every rank");
    return DCORA_ERR_UNSUPPORTED;
  }
  DCORA_HIP(hipSetDevice(opt.device));
  set_marks_.assign(R, 0);
  // Agent::iteration_number() of every agent; between rounds they are all equal to the session's round counter
  // (also after the session-level calls, which advance whole rounds)
  bool level = (int)agent_it.size() == R;
  for (int q = 0; level && q < R; ++q) level = !agents[q].hosted || agent_it[q] == agent_it[agent];
  if ((int)agent_it.size() != R || (level && agent_it[agent] != iteration)) agent_it.assign(R, iteration);
  if (agent_it[agent] == iteration) {  // this agent opens round iteration + 1: everybody has finished the last one
    for (int q = 0; q < R; ++q)
      if (agents[q].hosted && agent_it[q] != iteration) {
        set_last_error("rbcd: agent " + std::to_string(agent) + " starts a new round before agent " +
                       std::to_string(q) + " has iterated in the current one (agents advance in lockstep)");
        return DCORA_ERR_BAD_ARG;
      }
    if (pending_reset_) gamma = alpha = 0;
    pending_reset_ = false;
    advance_sequences();
    seq_advanced_ = false;
    for (int q = 0; q < R; ++q)
      if (!agents[q].hosted) agent_it[q] = iteration;
  } else if (agent_it[agent] != iteration - 1) {
    set_last_error("rbcd: agents advance in lockstep");
    return DCORA_ERR_BAD_ARG;
  }
  agent_it[agent] = iteration;
  const bool restart = restart_now();
  int rc;
  if (do_optimization) {
    rc = update_selected_agent(a, restart);
    if (!rc && team) rc = team_note_optimized(&agent, 1);
  } else {
    rc = opt.acceleration ? update_nonselected_agent(a, restart) : DCORA_OK;
  }
  if (restart) pending_reset_ = true;
  return rc;
}

// Agent::updateNeighborStates (ref src/Agent.cpp:844-906): poses the agent does not require are ignored
// (Graph::requireNeighborPose); the others go into its plain or auxiliary cache
int RbcdSession::agent_update_neighbor(int agent, int neighbor, int count, const int *frames, const double *poses,
                                       bool aux) {
  if (agent < 0 || agent >= R || neighbor < 0 || neighbor >= R || neighbor == agent || count < 0) {
    set_last_error("rbcd: bad agent / neighbour");
    return DCORA_ERR_BAD_ARG;
  }
  AgentDev &a = agents[agent];
  if (!a.hosted) {
    set_last_error("rbcd: agent is hosted by another rank");
    return DCORA_ERR_BAD_ARG;
  }
  DCORA_HIP(hipSetDevice(opt.device));
  const int dh = d + 1;
  const size_t blk = (size_t)r * dh;
  if (!a.detached) {
    const size_t N = (size_t)r * dh * n;
    for (int w = 0; w < 2; ++w) {
      DCORA_HIP(a.nbr[w].alloc(N));
      DCORA_HIP(hipMemsetAsync(a.nbr[w].p, 0, sizeof(double) * N, st));
      a.got[w].assign(a.required.size(), 0);
    }
    a.detached = true;
  }
  const int which = aux ? 1 : 0;
  std::vector<double> packed;
  std::vector<int> cols;
  for (int q = 0; q < count; ++q) {
    const int f = frames[q];
    if (f < 0 || f >= agents[neighbor].n) {
      set_last_error("rbcd: frame out of range");
      return DCORA_ERR_BAD_ARG;
    }
    const int gp = P.start(neighbor) + f;
    const auto it = std::lower_bound(a.required.begin(), a.required.end(), gp);
    if (it == a.required.end() || *it != gp) continue;  // not required: ignored, as in the reference
    a.got[which][(size_t)(it - a.required.begin())] = 1;
    packed.insert(packed.end(), poses + (size_t)q * blk, poses + (size_t)(q + 1) * blk);
    for (int c = 0; c < dh; ++c) cols.push_back(gp * dh + c);
  }
  if (!cols.empty()) {
    DevBuf<double> dp;
    DevBuf<int> dc;
    DCORA_HIP(dp.alloc(packed.size()));
    DCORA_HIP(dc.alloc(cols.size()));
    DCORA_HIP(hipMemcpyAsync(dp.p, packed.data(), sizeof(double) * packed.size(), hipMemcpyHostToDevice, st));
    DCORA_HIP(hipMemcpyAsync(dc.p, cols.data(), sizeof(int) * cols.size(), hipMemcpyHostToDevice, st));
    launch_scatter_cols(st, r, (int)cols.size(), dc.p, dp.p, a.nbr[which].p);
    DCORA_HIP(hipStreamSynchronize(st));  // the staging buffers leave scope
  }
  return DCORA_OK;
}

int RbcdSession::agent_get_X(int agent, double *Xh) {
  if (agent < 0 || agent >= R) {
    set_last_error("rbcd: agent out of range");
    return DCORA_ERR_BAD_ARG;
  }
  DCORA_HIP(hipSetDevice(opt.device));
  const AgentDev &a = agents[agent];
  const size_t B = sizeof(double) * (size_t)r * (d + 1) * a.n;
  DCORA_HIP(hipMemcpyAsync(Xh, Xg.p + (size_t)a.col0 * r, B, hipMemcpyDeviceToHost, st));
  DCORA_HIP(hipStreamSynchronize(st));
  return DCORA_OK;
}

// Agent::setX + initializeAcceleration (ref src/Agent.cpp:64-77, 1178-1187)
int RbcdSession::agent_set_X(int agent, const double *Xh) {
  staged_selected_ = -1;
  if (agent < 0 || agent >= R) {
    set_last_error("rbcd: agent out of range");
    return DCORA_ERR_BAD_ARG;
  }
  DCORA_HIP(hipSetDevice(opt.device));
  const AgentDev &a = agents[agent];
  const size_t off = (size_t)a.col0 * r;
  const size_t B = sizeof(double) * (size_t)r * (d + 1) * a.n;
  DCORA_HIP(hipMemcpyAsync(Xg.p + off, Xh, B, hipMemcpyHostToDevice, st));
  DCORA_HIP(hipMemcpyAsync(Vg.p + off, Xg.p + off, B, hipMemcpyDeviceToDevice, st));
  DCORA_HIP(hipMemcpyAsync(Yg.p + off, Xg.p + off, B, hipMemcpyDeviceToDevice, st));
  DCORA_HIP(hipMemcpyAsync(XPrevg.p + off, Xg.p + off, B, hipMemcpyDeviceToDevice, st));
  DCORA_HIP(hipStreamSynchronize(st));
  // initializeAcceleration of this agent: its V is the X it was handed (not necessarily feasible) until the next
  // projection; once EVERY agent has been set since the last round, the shared sequences restart as after set_X
  agents[agent].v_feasible = false;
  if ((int)set_marks_.size() != R) set_marks_.assign(R, 0);
  set_marks_[agent] = 1;
  bool all = true;
  for (int q = 0; q < R; ++q) all = all && (set_marks_[q] || !agents[q].hosted);
  if (all) {
    gamma = alpha = 0;
    iteration = 0;
    seq_advanced_ = false;
    pending_reset_ = false;
    agent_it.assign(R, 0);
    set_marks_.assign(R, 0);
    team_restart_rounds();
  }
  return DCORA_OK;
}

// central evaluation of the driver (ref examples/MultiRobotExample.cpp:264-305): 2 f, |rgrad|, greedy selection
int RbcdSession::evaluate(double *cost2, double *gradnorm, double *block_norms, int *next_selected) {
  if (!central) {
    set_last_error("central evaluation needs world_size == 1");
    return DCORA_ERR_UNSUPPORTED;
  }
  DeviceProblem &c = *central;
  const bool gf = c.group && c.fused && !c.has_bsr && c.Q.n_long == 0;
  const bool gfb = c.group && c.has_bsr;  // the same on the block structure of Q (large graphs: any number of poses)
  if (!gf && !gfb) c.enqueue_egrad(Xg.p, c.EG0.p, c.pA.p);
  if (c.group) {
    int nA = c.npA();
    int wpa = 0;  // > 0: the evaluation dealt its workgroups to the agents and pB holds their sums (BsrGradOut)
    if (gf)  // X Q, the cost dots, the Riemannian gradient and the per-pose norms in one launch
      nA = launch_fused_grad(st, c.m, c.Q.view(), buf1(Xg.p), nullptr, buf1(c.EG0.p), buf1(c.RG0.p),
                             Buf2{{nullptr, nullptr}}, 0, c.pA.p, c.pB.p, posenorm.p, Gate{});
    else if (gfb)
      // (only the dots and the per-pose norms leave the kernel: writing EG and RG of the whole graph, 2 x 16 MB on the
      // 100k lattice, would be written back at the kernel's end for nobody)
      nA = launch_fused_grad_bsr(st, c.m.r, c.m.d, c.Qb.view(), buf1(Xg.p), nullptr, Buf2{{nullptr, nullptr}},
                                 Buf2{{nullptr, nullptr}}, Buf2{{nullptr, nullptr}}, 0, c.pA.p, c.pB.p, posenorm.p,
                                 Gate{}, pose_start.p, R, &wpa);
    else
      c.enq_rgrad(buf1(Xg.p), buf1(c.EG0.p), buf1(c.RG0.p), Buf2{{nullptr, nullptr}}, 0, c.pB.p, Gate{}, posenorm.p);
    const int want = ++eval_seq;
    launch_eval_finish(st, R, pose_start.p, posenorm.p, c.pA.p, nA, eval_dev, want, eval_split.p, n,
                       wpa > 0 ? c.pB.p : nullptr, wpa);
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    while (eval_host->seq != want) {
      if ((++spins & 4095u) == 0 &&
          std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 20.0) {
        set_last_error("rbcd: evaluation epilogue did not complete (spin timeout)");
        return DCORA_ERR_HIP;
      }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (block_norms)
      for (int b = 0; b < R; ++b) block_norms[b] = eval_host->block_norms[b];
    if (cost2) *cost2 = eval_host->cost2;
    if (gradnorm) *gradnorm = eval_host->gradnorm;
    if (next_selected) *next_selected = eval_host->next;
    return team ? team_settle(true) : (int)DCORA_OK;
  }
  launch_rgrad(st, mg, buf1(Xg.p), buf1(c.EG0.p), buf1(c.RG0.p), Buf2{{nullptr, nullptr}}, 0, c.pB.p, Gate{});
  launch_block_dots(st, r, R, col_start.p, c.RG0.p, nullptr, evalbuf.p);
  launch_sum_partials(st, c.pA.p, c.npA(), 2, 2, evalbuf.p + 2 * R);
  std::vector<double> h(2 * R + 2);
  DCORA_HIP(hipMemcpyAsync(h.data(), evalbuf.p, sizeof(double) * (2 * R + 2), hipMemcpyDeviceToHost, st));
  DCORA_HIP(hipStreamSynchronize(st));
  double g2 = 0, best = -1;
  int arg = 0;
  for (int b = 0; b < R; ++b) {
    const double nb = std::sqrt(h[2 * b]);
    if (block_norms) block_norms[b] = nb;
    g2 += h[2 * b];
    if (nb > best) {
      best = nb;
      arg = b;
    }
  }
  if (cost2) *cost2 = 2.0 * (0.5 * h[2 * R] + h[2 * R + 1]);
  if (gradnorm) *gradnorm = std::sqrt(g2);
  if (next_selected) *next_selected = arg;
  return team ? team_settle(true) : (int)DCORA_OK;
}

int RbcdSession::last_result(dcora_ropt_result *res) {
  if (last_solver) return last_solver->fetch_result(res);
  *res = last;
  return DCORA_OK;
}

// distributed form of the same evaluation: per hosted agent |Proj(X_b Q_bb + G_b)|^2 and <X_b, X_b Q_bb + G_b>
int RbcdSession::phase_evaluate_dev(double *out_dev) {
  DCORA_HIP(hipSetDevice(opt.device));
  DCORA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * 2 * R, st));
  for (AgentDev &a : agents) {
    if (!a.hosted) continue;
    DeviceProblem &pb = *a.prob;
    const double *Xb = Xg.p + (size_t)a.col0 * r;
    launch_spmm(st, r, a.coupling.view(), buf1(Xg.p), 0, nullptr, buf1(pb.G.p), 0, nullptr, Gate{});
    pb.has_G = true;
    pb.enqueue_egrad(Xb, pb.EG1.p, nullptr);
    launch_rgrad(st, pb.m, buf1(Xb), buf1(pb.EG1.p), buf1(pb.RG1.p), Buf2{{nullptr, nullptr}}, 0, pb.pB.p, Gate{});
    launch_sum_partials(st, pb.pB.p, pb.npPose(), 1, 1, out_dev + 2 * a.id);
    launch_dot(st, pb.nelem(), Xb, pb.EG1.p, pb.p3.p);
    launch_sum_partials(st, pb.p3.p, pb.npVec(), 1, 1, out_dev + 2 * a.id + 1);
  }
  return DCORA_OK;
}

int RbcdSession::iterate(int selected, double *cost2, double *gradnorm, double *block_norms, int *next_selected) {
  int rc = check_selected(selected);
  if (rc) return rc;
  const long launches0 = g_chain_launches.load(std::memory_order_relaxed);
  rc = phase_nonselected(selected);
  if (rc) return rc;
  // world_size == 1: the "pull" of public poses (ref examples/MultiRobotExample.cpp:236-258) is the identity,
  // all agents' blocks live in the same mirror Xg
  rc = phase_selected(selected);
  if (rc) return rc;
  int nxt = selected;
  rc = evaluate(cost2, gradnorm, block_norms, &nxt);
  chain_launches += g_chain_launches.load(std::memory_order_relaxed) - launches0;
  if (rc) return rc;
  // greedy selection only when the selected agent has neighbours (:290-292)
  if (next_selected) *next_selected = (agents[selected].coupling.nnz > 0) ? nxt : selected;
  return DCORA_OK;
}

// The tick's hooks (SessionCore::iterate_set).  A step staged by an interrupted round, an advance of the sequences that
// waits for its phase_selected and the setX marks do not survive a tick.
void RbcdSession::tick_begins() {
  staged_selected_ = -1;
  seq_advanced_ = false;
  set_marks_.assign(R, 0);
}

int RbcdSession::stage(AgentCore &core) {
  AgentDev &a = static_cast<AgentDev &>(core);
  DeviceProblem &pb = *a.prob;
  const size_t off = (size_t)a.col0 * r;
  const size_t B = sizeof(double) * (size_t)pb.nelem();
  launch_spmm(st, r, a.coupling.view(), buf1(Xg.p), 0, nullptr, buf1(pb.G.p), 0, nullptr, Gate{});
  pb.has_G = true;
  DCORA_HIP(hipMemcpyAsync(XPrevg.p + off, Xg.p + off, B, hipMemcpyDeviceToDevice, st));
  DCORA_HIP(hipMemcpyAsync(pb.X0.p, Xg.p + off, B, hipMemcpyDeviceToDevice, st));
  return DCORA_OK;
}

// the accepted iterate goes back into the mirror without a host round trip when the solver keeps its choice on the device
int RbcdSession::write_back(AgentCore &core, hipStream_t run_on) {
  AgentDev &a = static_cast<AgentDev &>(core);
  DeviceProblem &pb = *a.prob;
  const size_t off = (size_t)a.col0 * r;
  if (group_kernels(pb.m))
    return nesterov_solved(run_on, pb, 3, 0.0, 0.0, Xg.p + off, Vg.p + off, Yg.p + off, XPrevg.p + off);
  double *Xres = nullptr;
  const int rc = pb.result(&Xres);
  if (rc) return rc;
  DCORA_HIP(hipMemcpyAsync(Xg.p + off, Xres, sizeof(double) * (size_t)pb.nelem(), hipMemcpyDeviceToDevice, run_on));
  return DCORA_OK;
}

// Blocks whose tCG runs fit ONE launch (dense preconditioner, n / 2 co-resident workgroups): one after the other on the
// session's stream -- 3 launches per RTR iteration each -- is faster on one device than side by side on the launches per
// iteration (sphere2500 / 5 agents: 2420 -> see DESIGN.md block updates/s), and the two forms give the same bits.
bool RbcdSession::serial_set(const std::vector<AgentCore *> &work) {
  bool serial = true;
  for (const AgentCore *a : work) serial = serial && a->prob->tcg_run_ok && a->prob->use_pc();
  return serial;
}

int RbcdSession::tick_done(const std::vector<AgentCore *> &work) {
  if (!team) return DCORA_OK;
  std::vector<int> ids;
  for (const AgentCore *a : work) ids.push_back(static_cast<const AgentDev *>(a)->id);
  return team_note_optimized(ids.data(), (int)ids.size());
}

int RbcdSession::pack_public(int agent, double *packed_dev) {
  AgentDev &a = agents[agent];
  launch_gather_cols(st, r, (int)a.public_poses.size() * (d + 1), a.public_cols.p, Xg.p, packed_dev);
  return DCORA_OK;
}
int RbcdSession::unpack_public(int agent, const double *packed_dev) {
  AgentDev &a = agents[agent];
  launch_scatter_cols(st, r, (int)a.public_poses.size() * (d + 1), a.public_cols.p, packed_dev, Xg.p);
  return DCORA_OK;
}

// ---- the team protocol ----------------------------------------------------------------------------------------------
// Agent::iteration_number() of one agent: its own count inside a round of per-agent calls, the session's round counter
// whenever the agents are level (the session-level calls advance whole rounds without touching agent_it)
int RbcdSession::agent_iteration_number(int agent) const {
  if ((int)agent_it.size() != R) return iteration;
  for (int q = 0; q < R; ++q)
    if (agents[(size_t)q].hosted && agent_it[(size_t)q] != agent_it[(size_t)agent]) return agent_it[(size_t)agent];
  return iteration;
}

// the session's relative-change launch for agents just marked: one launch behind everything their updates enqueued on
// the session's stream, compares the X the round leaves with the XPrev it saved.  Ranked: into the agents' status slots
int RbcdSession::team_launch_rel_change(const std::vector<int> &ids) {
  RelChangeSet set{};
  for (int b : ids) set.agent[set.count++] = b;
  if (team->ranked)
    launch_rel_change_ranked(st, r, d, Xg.p, XPrevg.p, pose_start.p, set, team_publish_slots(ids));
  else
    launch_rel_change(st, r, d, Xg.p, XPrevg.p, pose_start.p, set, team->rel_dev);
  DCORA_HIP(hipGetLastError());
  return DCORA_OK;
}

}  // namespace dcora
