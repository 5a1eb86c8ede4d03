// RBCD++ session for multi-robot range-aided SLAM on the device (see ra_rbcd.h).
#include "ra_rbcd.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <set>
#include <string>

#include "cert.h"

namespace dcora {

RaRbcdSession::~RaRbcdSession() {
  for (RaAgentDev &a : agents) release_tick_resources(a);
  agents.clear();
  central.reset();
  release_stream();
}

int RaRbcdSession::init(const HostRADataset &ds, const dcora_rbcd_options &o) {
  const auto t0 = std::chrono::steady_clock::now();
  opt = o;
  d = ds.d;
  n = ds.n;
  l = ds.l;
  b = ds.b;
  k = ds.k();
  r = o.r;
  if (o.world_size < 1 || o.rank < 0 || o.rank >= o.world_size) {
    set_last_error("ra_rbcd: bad rank / world_size");
    return DCORA_ERR_BAD_ARG;
  }
  if (r < d || r > 16) {
    set_last_error("ra_rbcd: need d <= r <= 16");
    return DCORA_ERR_BAD_ARG;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    set_last_error("no HIP device available: libdcora_hip has no CPU fallback");
    return DCORA_ERR_NO_DEVICE;
  }
  DCORA_HIP(hipSetDevice(o.device));
  // agents = the robots that own poses, in id order; every unit sphere and landmark must belong to one of them
  // (the reference's map agent is passive, src/Agent.cpp:541: variables it would own are never optimised)
  std::set<int> robots(ds.pose_robot.begin(), ds.pose_robot.end());
  for (int q : ds.sphere_robot)
    if (!robots.count(q)) {
      set_last_error("ra_rbcd: a unit sphere is owned by a robot without poses (map agent): not optimisable here");
      return DCORA_ERR_UNSUPPORTED;
    }
  for (int q : ds.landmark_robot)
    if (!robots.count(q)) {
      set_last_error("ra_rbcd: a landmark is owned by a robot without poses (map agent): not optimisable here");
      return DCORA_ERR_UNSUPPORTED;
    }
  R = (int)robots.size();
  if (R < 1 || R > kMaxAgents) {
    set_last_error("ra_rbcd: bad number of robots");
    return DCORA_ERR_UNSUPPORTED;
  }
  {
    const int rcs = acquire_stream(nullptr);
    if (rcs) return rcs;
  }
  const size_t N = (size_t)r * k;
  DCORA_HIP(Xg.alloc(N));
  DCORA_HIP(hipMemset(Xg.p, 0, sizeof(double) * N));
  DCORA_HIP(evalbuf.alloc(R + 8));
  agents.resize(R);
  int idx = 0;
  for (int robot : robots) {
    RaAgentDev &a = agents[idx];
    a.robot = robot;
    a.hosted = ra_rank_of_agent(idx, R, o.world_size) == o.rank;  // consecutive agents share a rank
    int dims3[3];
    ra_agent_columns(ds, robot, dims3, a.own_host);
    a.n = dims3[0];
    a.l = dims3[1];
    a.b = dims3[2];
    a.k = (int)a.own_host.size();
    ++idx;
  }
  // the team's loop closures, the agents (positions in the sorted robot list) owning their ends for the robots
  ra_team_loop_closures(ds, &team_lcs_);
  {
    const std::vector<int> sorted(robots.begin(), robots.end());
    auto agent_of = [&](int robot) {
      return (int)(std::lower_bound(sorted.begin(), sorted.end(), robot) - sorted.begin());
    };
    for (TeamLoopClosure &q : team_lcs_) {  // (every owner is one of `robots`: checked above)
      q.a1 = agent_of(q.a1);
      q.a2 = agent_of(q.a2);
    }
  }
  const int rc = assemble(ds, true);
  if (rc) return rc;
  iteration = 0;
  gamma = alpha = 0;
  setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return DCORA_OK;
}

// The one path from a dataset's measurements to the session's matrices, at creation and on every re-weight
// (Graph::clearDataMatrices + constructDataMatrices, ref src/Agent.cpp:1416): build_Q_ra, every agent's Q_aa and coupling
// block cut out of it, the agent's regularisation recomputed from its Q_aa (the reference recomputes it whenever the data
// matrices are rebuilt, ref src/Graph.cpp:1906, 1921), the central Q.
// Creation: the device problems, buffers and tick resources are made, who neighbours whom is read off the coupling
// blocks, and a robust session records the patterns.
// Re-weight (robust sessions; the caller has synchronised every stream): the matrices as the builders give
// them (no explicit zeros) go to build_preconditioner, so the cache sees the keys of a fresh session -- a new image is
// attached, an image somebody else still holds is never written --, and their values scattered onto the creation
// patterns (a weight of 0 leaves explicit zeros) are what is uploaded.  Nothing on the device is touched before every
// matrix has been found to fit its pattern.
// A rank of a job (world_size > 1) has no central problem, and patterns and device matrices of its hosted agents only.
// A hosted agent's rows of Q hold the measurements touching that agent and no other, so the weights this rank keeps for
// the rest of the job (the last it was told) reach nothing that is uploaded.
int RaRbcdSession::assemble(const HostRADataset &ds, bool creation) {
  const dcora_rbcd_options &o = opt;
  const HostCsr Q = build_Q_ra(ds);
  std::vector<HostCsr> Qaa((size_t)R), C((size_t)R);
  for (int i = 0; i < R; ++i) extract_agent_blocks(Q, agents[(size_t)i].own_host, &Qaa[(size_t)i], &C[(size_t)i]);
  // re-weight: host images of the uploads, alive until the stream has been synchronised
  std::vector<HostCsr> Qs, Cs;
  std::vector<std::vector<double>> stage;
  HostCsr Qcs;
  std::vector<double> cstage;
  if (creation) {
    if (robust) {
      robust->Qpat.assign((size_t)R, HostCsr());
      robust->Cpat.assign((size_t)R, HostCsr());
    }
  } else {
    Qs.resize((size_t)R);
    Cs.resize((size_t)R);
    stage.resize((size_t)R);
    bool ok = !central || scatter_on_pattern(Q, robust->central_pat, &Qcs);
    for (int i = 0; i < R && ok; ++i)
      ok = !agents[(size_t)i].hosted ||
           (scatter_on_pattern(Qaa[(size_t)i], robust->Qpat[(size_t)i], &Qs[(size_t)i]) &&
            scatter_on_pattern(C[(size_t)i], robust->Cpat[(size_t)i], &Cs[(size_t)i]));
    if (!ok) {
      set_last_error("ra_rbcd robust: the weights give a matrix entry outside the session's pattern");
      return DCORA_ERR_BAD_ARG;
    }
  }
  int rc = DCORA_OK;
  for (int i = 0; i < R && !rc; ++i) {
    RaAgentDev &a = agents[(size_t)i];
    if (!a.hosted) continue;  // agents of other ranks: their columns and public variables are all this rank keeps
    rc = device_precond_regularization(Qaa[(size_t)i], o.device, &a.reg);  // ref src/Graph.cpp:1901-1960, per agent
    if (rc) break;
    if (!creation) {
      rc = a.prob->set_values(Qs[(size_t)i], st, &stage[(size_t)i]);
      if (!rc) rc = a.coupling.set_values(Cs[(size_t)i], st);
      if (!rc) rc = a.prob->build_preconditioner(Qaa[(size_t)i], a.reg);
      continue;
    }
    a.prob.reset(new DeviceProblem);
    dcora_dims dims{r, d, a.n, a.l, a.b, DCORA_LAYOUT_RA};  // an agent without ranges / landmarks keeps the RA ordering
    rc = a.prob->init(dims, Qaa[(size_t)i], nullptr, a.reg, o.device, st);
    if (rc) break;
    rc = a.coupling.upload(C[(size_t)i]);
    if (rc) break;
    if (robust) {
      robust->Qpat[(size_t)i] = pattern_of(Qaa[(size_t)i]);
      robust->Cpat[(size_t)i] = pattern_of(C[(size_t)i]);
    }
    DCORA_HIP(a.own.alloc(a.own_host.size()));
    DCORA_HIP(hipMemcpy(a.own.p, a.own_host.data(), sizeof(int) * a.own_host.size(), hipMemcpyHostToDevice));
    const size_t Na = (size_t)r * a.k;
    DCORA_HIP(a.X.alloc(Na));
    DCORA_HIP(a.V.alloc(Na));
    DCORA_HIP(a.Y.alloc(Na));
    DCORA_HIP(a.XPrev.alloc(Na));
    DCORA_HIP(a.tmp.alloc(Na));
    rc = acquire_tick_resources(a);
  }
  if (!creation) {
    if (!rc && central) rc = central->set_values(Qcs, st, &cstage);
    const hipError_t synced = hipStreamSynchronize(st);  // (also after a failure: copies may be in flight)
    if (rc) return rc;
    DCORA_HIP(synced);
    if (central) {
      robust->live_pat = pattern_of(Q);  // the next certificate is a fresh session's: over these weights' entries
      cert_.reset();
    }
    return DCORA_OK;
  }
  if (rc) return rc;
  rc = create_fork_event();
  if (rc) return rc;
  // the columns of OTHER agents an agent's coupling block reaches are their public variables; their owners its neighbours
  std::vector<int> owner_of((size_t)k, -1);  // global column -> agent
  for (int i = 0; i < R; ++i)
    for (int c : agents[(size_t)i].own_host) owner_of[(size_t)c] = i;
  std::vector<std::set<int>> pub((size_t)R), nbr((size_t)R);
  for (int me = 0; me < R; ++me)
    for (int c : C[(size_t)me].ci) {
      const int q = owner_of[(size_t)c];
      if (q >= 0 && q != me) {
        pub[(size_t)q].insert(c);
        nbr[(size_t)me].insert(q);
        nbr[(size_t)q].insert(me);
      }
    }
  for (int i = 0; i < R; ++i) {
    RaAgentDev &a = agents[(size_t)i];
    a.neighbors.assign(nbr[(size_t)i].begin(), nbr[(size_t)i].end());
    std::vector<int> pc(pub[(size_t)i].begin(), pub[(size_t)i].end());
    a.n_public_cols = (int)pc.size();
    DCORA_HIP(a.public_cols.alloc(std::max<size_t>(pc.size(), 1)));
    if (!pc.empty()) DCORA_HIP(hipMemcpy(a.public_cols.p, pc.data(), sizeof(int) * pc.size(), hipMemcpyHostToDevice));
  }
  if (o.world_size == 1) {  // the central evaluation of the one-process loop; ranks evaluate agent by agent
    central.reset(new DeviceProblem);
    dcora_dims dims{r, d, n, l, b, DCORA_LAYOUT_RA};
    rc = central->init(dims, Q, nullptr, -1.0, o.device, st);
    if (rc) return rc;
    if (robust) robust->live_pat = robust->central_pat = pattern_of(Q);
  } else {
    job_pat = pattern_of(Q);  // (what the job-wide certificate is laid out on: Exchange::certify_live)
  }
  return DCORA_OK;
}

// ---- robust sessions (RobustState, session_core.h): what is this kind's own -------------------------------------------
// The loop closures are ra_loop_closures': every pose-pose measurement but odometry.  A rank of a multi-rank job (ranked)
// builds the patterns of its hosted agents only and uploads the pose-pose measurements touching them (ra_rank_edges), to
// be read from its mirror in the RA ordering of the whole problem.
int RaRbcdSession::init_robust(const HostRADataset &ds, const dcora_rbcd_options &o, const dcora_robust_params &p,
                               const int *fixed, bool ranked) {
  int rc = robust_check_args(ds.pose_pose, ds.n, o, p, ranked);
  if (rc) return rc;
  if (ds.pose_robot.size() != (size_t)ds.n) {
    set_last_error("ra_rbcd robust: the dataset has no pose owners");
    return DCORA_ERR_BAD_ARG;
  }
  const size_t m = ds.pose_pose.size();
  std::vector<int> lc(m);
  ra_loop_closures(ds, lc.data());
  robust_begin(ds.pose_pose, std::vector<char>(lc.begin(), lc.end()), p, fixed, ranked);
  robust_ds_ = ds;
  for (size_t e = 0; e < m; ++e) robust_ds_.pose_pose[e].weight = robust->w[e];
  rc = init(robust_ds_, o);
  return rc ? rc : robust_finish();
}

int RaRbcdSession::robust_upload_edges() {
  RobustState &rs = *robust;
  if (!rs.ranked) {
    for (size_t e = 0; e < rs.w.size(); ++e) rs.edge_ids.push_back((int)e);
    return rs.edges.upload_ra(robust_ds_, rs.update);
  }
  std::vector<char> own;
  ra_rank_edges(robust_ds_, opt.rank, opt.world_size, &rs.edge_ids, &own);
  for (size_t i = 0; i < rs.edge_ids.size(); ++i) rs.owned[(size_t)rs.edge_ids[i]] = own[i];
  return rs.edges.upload_ra_ranked(robust_ds_, rs.update, rs.edge_ids, own);
}

int RaRbcdSession::robust_rebuild(const std::vector<double> &w) {
  HostRADataset next = robust_ds_;
  for (size_t e = 0; e < w.size(); ++e) next.pose_pose[e].weight = w[e];
  return assemble(next, false);
}

int RaRbcdSession::robust_restart_acceleration() {
  const int rc = gather_agents();  // (after a reset the agents' own X comes from the mirror; otherwise it is what they hold)
  if (rc) return rc;
  DCORA_HIP(hipStreamSynchronize(st));
  gamma = alpha = 0;
  return DCORA_OK;
}

int RaRbcdSession::gather_agents() {
  for (RaAgentDev &a : agents) {
    if (!a.hosted) continue;
    const size_t Ba = sizeof(double) * (size_t)r * a.k;
    launch_gather_cols(st, r, a.k, a.own.p, Xg.p, a.X.p);
    DCORA_HIP(hipMemcpyAsync(a.V.p, a.X.p, Ba, hipMemcpyDeviceToDevice, st));
    DCORA_HIP(hipMemcpyAsync(a.Y.p, a.X.p, Ba, hipMemcpyDeviceToDevice, st));
    DCORA_HIP(hipMemcpyAsync(a.XPrev.p, a.X.p, Ba, hipMemcpyDeviceToDevice, st));
  }
  return DCORA_OK;
}

int RaRbcdSession::set_X(const double *Xh) { return adopt_X(Xh, hipMemcpyHostToDevice); }

// ---- the staircase step in place: SessionCore::lift's hooks ------------------------------------------------------
int RaRbcdSession::lift_default_reg(const HostCsr &Qc, double *reg) {
  return device_precond_regularization(Qc, opt.device, reg);
}

int RaRbcdSession::lift_buffers(int r_new) {
  DevBuf<double> X, XI;
  DCORA_HIP(X.alloc((size_t)r_new * k));
  if (robust) DCORA_HIP(XI.alloc((size_t)r_new * k));
  std::vector<DevBuf<double>> own((size_t)R * 5);  // per hosted agent: X, V, Y, XPrev, tmp
  for (int i = 0; i < R; ++i)
    for (int q = 0; q < 5 && agents[(size_t)i].hosted; ++q)
      DCORA_HIP(own[(size_t)i * 5 + q].alloc((size_t)r_new * agents[(size_t)i].k));
  // the swap: nothing below fails
  Xg = std::move(X);
  if (robust) robust->X_initial = std::move(XI);
  for (int i = 0; i < R; ++i) {
    RaAgentDev &a = agents[(size_t)i];
    if (!a.hosted) continue;
    DevBuf<double> *mine[5] = {&a.X, &a.V, &a.Y, &a.XPrev, &a.tmp};
    for (int q = 0; q < 5; ++q) *mine[q] = std::move(own[(size_t)i * 5 + q]);
  }
  r = r_new;
  opt.r = r_new;
  return DCORA_OK;
}

AgentBlock RaRbcdSession::agent_block(int id) {
  const RaAgentDev &a = agents[(size_t)id];
  AgentBlock blk;
  blk.X = a.X.p;
  blk.k = a.k;
  blk.n = a.n, blk.l = a.l, blk.b = a.b;
  blk.se = (a.l == 0 && a.b == 0) ? 1 : 0;
  blk.cols_dev = a.own.p;
  blk.cols_host = a.own_host.data();
  return blk;
}

int RaRbcdSession::adopt_X(const double *X, hipMemcpyKind kind) {
  DCORA_HIP(hipSetDevice(opt.device));
  const size_t B = sizeof(double) * (size_t)r * k;
  DCORA_HIP(hipMemcpyAsync(Xg.p, X, B, kind, st));
  if (robust) DCORA_HIP(hipMemcpyAsync(robust->X_initial.p, Xg.p, B, hipMemcpyDeviceToDevice, st));
  const int rc = gather_agents();
  if (rc) return rc;
  DCORA_HIP(hipStreamSynchronize(st));
  gamma = alpha = 0;
  iteration = 0;
  team_restart_rounds();
  return DCORA_OK;
}

int RaRbcdSession::get_X(double *Xh) {
  DCORA_HIP(hipSetDevice(opt.device));
  DCORA_HIP(hipMemcpyAsync(Xh, Xg.p, sizeof(double) * (size_t)r * k, hipMemcpyDeviceToHost, st));
  DCORA_HIP(hipStreamSynchronize(st));
  return DCORA_OK;
}

int RaRbcdSession::scatter(RaAgentDev &a) {
  launch_scatter_cols(st, r, a.k, a.own.p, a.X.p, Xg.p);
  return DCORA_OK;
}

// updateX(doOptimization = true): G from the neighbours' public states in the mirror, local solve from `start`
// (ref src/Agent.cpp:1216-1278, src/Graph.cpp:1190-1772)
int RaRbcdSession::solve(RaAgentDev &a, const double *start, double **result) {
  DeviceProblem &pb = *a.prob;
  launch_spmm(st, r, a.coupling.view(), buf1(Xg.p), 0, nullptr, buf1(pb.G.p), 0, nullptr, Gate{});
  pb.has_G = true;
  DCORA_HIP(hipMemcpyAsync(pb.X0.p, start, sizeof(double) * (size_t)r * a.k, hipMemcpyDeviceToDevice, st));
  int rc = pb.optimize_dev(opt.local);
  if (!rc) rc = pb.result(result);
  if (rc) return rc;
  last_solver = &pb;
  return DCORA_OK;
}

// Agent::iterate(false) of the hosted non-selected agents (ref src/Agent.cpp:535-551, 1202-1214): the shared Nesterov
// sequences advance once per round on every rank alike
int RaRbcdSession::phase_nonselected(int selected) {
  if (const int rc = check_selected(selected)) return rc;
  DCORA_HIP(hipSetDevice(opt.device));
  advance_sequences();
  const bool accel = opt.acceleration != 0;
  const bool restart = restart_now();
  // Y = proj((1 - alpha) X + alpha V), X = Y, V = proj(V)
  for (int i = 0; i < R; ++i) {
    if (i == selected) continue;
    RaAgentDev &a = agents[i];
    if (!a.hosted) continue;
    const ManiDesc &m = a.prob->m;
    const size_t Ba = sizeof(double) * (size_t)r * a.k;
    DCORA_HIP(hipMemcpyAsync(a.XPrev.p, a.X.p, Ba, hipMemcpyDeviceToDevice, st));
    if (!accel) continue;
    if (restart) {  // restartNesterovAcceleration(false): X = XPrev, V = Y = X
      DCORA_HIP(hipMemcpyAsync(a.V.p, a.X.p, Ba, hipMemcpyDeviceToDevice, st));
      DCORA_HIP(hipMemcpyAsync(a.Y.p, a.X.p, Ba, hipMemcpyDeviceToDevice, st));
    } else {
      launch_polar(st, m, 1.0 - alpha, a.X.p, alpha, a.V.p, 0.0, nullptr, a.Y.p);
      DCORA_HIP(hipMemcpyAsync(a.X.p, a.Y.p, Ba, hipMemcpyDeviceToDevice, st));
      launch_polar(st, m, 1.0, a.V.p, 0.0, nullptr, 0.0, nullptr, a.V.p);
      scatter(a);
    }
  }
  return DCORA_OK;
}

// Agent::iterate(true) of the selected agent, where it lives
int RaRbcdSession::phase_selected(int selected) {
  if (const int rc = check_selected(selected)) return rc;
  DCORA_HIP(hipSetDevice(opt.device));
  const bool accel = opt.acceleration != 0;
  const bool restart = restart_now();
  RaAgentDev &a = agents[selected];
  if (a.hosted) {
    const ManiDesc &m = a.prob->m;
    const size_t Ba = sizeof(double) * (size_t)r * a.k;
    DCORA_HIP(hipMemcpyAsync(a.XPrev.p, a.X.p, Ba, hipMemcpyDeviceToDevice, st));
    double *res = nullptr;
    if (accel) {
      launch_polar(st, m, 1.0 - alpha, a.X.p, alpha, a.V.p, 0.0, nullptr, a.Y.p);
      int rc = solve(a, a.Y.p, &res);
      if (rc) return rc;
      DCORA_HIP(hipMemcpyAsync(a.X.p, res, Ba, hipMemcpyDeviceToDevice, st));
      launch_polar(st, m, 1.0, a.V.p, gamma, a.X.p, -gamma, a.Y.p, a.V.p);  // V = proj(V + gamma (X - Y))
      if (restart) {  // X = XPrev; updateX(true, false); V = Y = X
        rc = solve(a, a.XPrev.p, &res);
        if (rc) return rc;
        DCORA_HIP(hipMemcpyAsync(a.X.p, res, Ba, hipMemcpyDeviceToDevice, st));
        DCORA_HIP(hipMemcpyAsync(a.V.p, a.X.p, Ba, hipMemcpyDeviceToDevice, st));
        DCORA_HIP(hipMemcpyAsync(a.Y.p, a.X.p, Ba, hipMemcpyDeviceToDevice, st));
      }
    } else {
      int rc = solve(a, a.X.p, &res);
      if (rc) return rc;
      DCORA_HIP(hipMemcpyAsync(a.X.p, res, Ba, hipMemcpyDeviceToDevice, st));
    }
    scatter(a);
    if (team) {  // behind both solves of a restart round: the X the round leaves against the XPrev it saved
      const int rc = team_note_optimized(&selected, 1);
      if (rc) return rc;
    }
  }
  if (restart) gamma = alpha = 0;
  return DCORA_OK;
}

int RaRbcdSession::iterate(int selected, double *cost2, double *gradnorm, double *block_norms, int *next_selected) {
  if (opt.world_size != 1) {
    set_last_error("ra_rbcd: with one process per GPU the loop body is dcora_exchange_rbcd_iterate");
    return DCORA_ERR_UNSUPPORTED;
  }
  int rc = phase_nonselected(selected);
  if (rc) return rc;
  rc = phase_selected(selected);
  if (rc) return rc;
  int nxt = selected;
  rc = evaluate(cost2, gradnorm, block_norms, &nxt);
  if (rc) return rc;
  if (next_selected) *next_selected = (agents[selected].coupling.nnz > 0) ? nxt : selected;
  return DCORA_OK;
}

// distributed form of the evaluation: per hosted agent |Proj(X_a Q_aa + G_a)|^2 and <X_a, X_a Q_aa + G_a>, G_a from the
// neighbours' public variables in the mirror
int RaRbcdSession::phase_evaluate_dev(double *out_dev) {
  DCORA_HIP(hipSetDevice(opt.device));
  DCORA_HIP(hipMemsetAsync(out_dev, 0, sizeof(double) * 2 * R, st));
  for (int i = 0; i < R; ++i) {
    RaAgentDev &a = agents[i];
    if (!a.hosted) continue;
    DeviceProblem &pb = *a.prob;
    launch_spmm(st, r, a.coupling.view(), buf1(Xg.p), 0, nullptr, buf1(pb.G.p), 0, nullptr, Gate{});
    pb.has_G = true;
    pb.enqueue_egrad(a.X.p, pb.EG1.p, nullptr);
    launch_rgrad(st, pb.m, buf1(a.X.p), buf1(pb.EG1.p), buf1(pb.RG1.p), Buf2{{nullptr, nullptr}}, 0, pb.pB.p, Gate{});
    launch_sum_partials(st, pb.pB.p, pb.npPose(), 1, 1, out_dev + 2 * i);
    launch_dot(st, pb.nelem(), a.X.p, pb.EG1.p, pb.p3.p);
    launch_sum_partials(st, pb.p3.p, pb.npVec(), 1, 1, out_dev + 2 * i + 1);
  }
  return DCORA_OK;
}

// initializeAcceleration / acceleration off for every agent (ref src/Agent.cpp:1178-1187)
int RaRbcdSession::set_acceleration(bool on) {
  DCORA_HIP(hipSetDevice(opt.device));
  opt.acceleration = on ? 1 : 0;
  for (RaAgentDev &a : agents) {
    if (!a.hosted) continue;
    const size_t Ba = sizeof(double) * (size_t)r * a.k;
    DCORA_HIP(hipMemcpyAsync(a.V.p, a.X.p, Ba, hipMemcpyDeviceToDevice, st));
    DCORA_HIP(hipMemcpyAsync(a.Y.p, a.X.p, Ba, hipMemcpyDeviceToDevice, st));
    DCORA_HIP(hipMemcpyAsync(a.XPrev.p, a.X.p, Ba, hipMemcpyDeviceToDevice, st));
  }
  gamma = alpha = 0;
  iteration = 0;
  team_restart_rounds();
  return DCORA_OK;
}

// the tick's staging: XPrev, G_a = X_mirror C_a^T (launch_spmm, as solve() forms it) and the start point
int RaRbcdSession::stage(AgentCore &core) {
  RaAgentDev &a = static_cast<RaAgentDev &>(core);
  DeviceProblem &pb = *a.prob;
  const size_t Ba = sizeof(double) * (size_t)r * a.k;
  DCORA_HIP(hipMemcpyAsync(a.XPrev.p, a.X.p, Ba, hipMemcpyDeviceToDevice, st));
  launch_spmm(st, r, a.coupling.view(), buf1(Xg.p), 0, nullptr, buf1(pb.G.p), 0, nullptr, Gate{});
  pb.has_G = true;
  DCORA_HIP(hipMemcpyAsync(pb.X0.p, a.X.p, Ba, hipMemcpyDeviceToDevice, st));
  return DCORA_OK;
}

int RaRbcdSession::write_back(AgentCore &core, hipStream_t run_on) {
  RaAgentDev &a = static_cast<RaAgentDev &>(core);
  double *res = nullptr;
  const int rc = a.prob->result(&res);  // (the solver paces from the host: this waits for run_on)
  if (rc) return rc;
  DCORA_HIP(hipMemcpyAsync(a.X.p, res, sizeof(double) * (size_t)r * a.k, hipMemcpyDeviceToDevice, run_on));
  launch_scatter_cols(run_on, r, a.k, a.own.p, a.X.p, Xg.p);
  return DCORA_OK;
}

// the tick's updates are all enqueued and the session's stream waits for every one of them
int RaRbcdSession::tick_done(const std::vector<AgentCore *> &work) {
  if (!team) return DCORA_OK;
  std::vector<int> ids;
  for (const AgentCore *a : work) ids.push_back((int)(static_cast<const RaAgentDev *>(a) - agents.data()));
  return team_note_optimized(ids.data(), (int)ids.size());
}

// Agent::iterate's maxTranslationDistance(X, XPrev) (ref src/Agent.cpp:564-565) of agents just marked, over their poses
// only: one launch on the session's stream, every agent's own two buffers and its translations' first column by value
int RaRbcdSession::team_launch_rel_change(const std::vector<int> &ids) {
  RaRelChangeSet set{};
  for (int b : ids) {
    const RaAgentDev &a = agents[(size_t)b];
    set.agent[set.count] = b;
    set.X[set.count] = a.X.p;
    set.XPrev[set.count] = a.XPrev.p;
    set.n[set.count] = a.n;
    set.toff[set.count] = d * a.n + a.l;
    set.count++;
  }
  if (team->ranked)  // a rank of a job: into the agents' status slots of the segment, as the pose-graph kind does
    launch_rel_change_ra_ranked(st, r, set, team_publish_slots(ids));
  else
    launch_rel_change_ra(st, r, set, team->rel_dev);
  DCORA_HIP(hipGetLastError());
  return DCORA_OK;
}

// central evaluation of the driver: 2 f, |rgrad| of the merged problem, per-agent |rgrad_a|, greedy selection
int RaRbcdSession::evaluate(double *cost2, double *gradnorm, double *block_norms, int *next_selected) {
  if (!central) {
    set_last_error("ra_rbcd: the central evaluation needs world_size == 1 (ranks: dcora_exchange_evaluate)");
    return DCORA_ERR_UNSUPPORTED;
  }
  DCORA_HIP(hipSetDevice(opt.device));
  DeviceProblem &c = *central;
  c.enqueue_egrad(Xg.p, c.EG0.p, c.pA.p);
  launch_rgrad(st, c.m, buf1(Xg.p), buf1(c.EG0.p), buf1(c.RG0.p), Buf2{{nullptr, nullptr}}, 0, c.pB.p, Gate{});
  launch_sum_partials(st, c.pA.p, c.npA(), 2, 2, evalbuf.p);
  launch_sum_partials(st, c.pB.p, c.npPose(), 1, 1, evalbuf.p + 2);
  for (int i = 0; i < R; ++i) {
    RaAgentDev &a = agents[i];
    const long Na = (long)r * a.k;
    launch_gather_cols(st, r, a.k, a.own.p, c.RG0.p, a.tmp.p);
    launch_dot(st, Na, a.tmp.p, a.tmp.p, c.p3.p);
    launch_sum_partials(st, c.p3.p, vec_grid(Na), 1, 1, evalbuf.p + 3 + i);
  }
  std::vector<double> h(R + 3);
  DCORA_HIP(hipMemcpyAsync(h.data(), evalbuf.p, sizeof(double) * (R + 3), hipMemcpyDeviceToHost, st));
  DCORA_HIP(hipStreamSynchronize(st));
  double best = -1;
  int arg = 0;
  for (int i = 0; i < R; ++i) {
    const double nb = std::sqrt(h[3 + i]);
    if (block_norms) block_norms[i] = nb;
    if (nb > best) {
      best = nb;
      arg = i;
    }
  }
  if (cost2) *cost2 = 2.0 * (0.5 * h[0] + h[1]);
  if (gradnorm) *gradnorm = std::sqrt(h[2]);
  if (next_selected) *next_selected = arg;
  return team ? team_settle(true) : (int)DCORA_OK;  // (the stream has been synchronised past the statuses' launch)
}

int RaRbcdSession::last_result(dcora_ropt_result *res) {
  if (!last_solver) {
    set_last_error("ra_rbcd: no local solve yet");
    return DCORA_ERR_BAD_ARG;
  }
  return last_solver->fetch_result(res);
}

}  // namespace dcora
