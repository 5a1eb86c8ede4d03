// The session core on the host (see session_core.h).
#include "session_core.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>

#include "escape_rule.h"
#include "exchange_slots.h"
#include "host_graph.h"
#include "host_threads.h"

namespace dcora {

void SessionCore::advance_sequences() {
  iteration++;
  inner_rounds++;
  if (opt.acceleration) {
    gamma = (1 + std::sqrt(1 + 4.0 * R * R * gamma * gamma)) / (2.0 * R);
    alpha = 1.0 / (gamma * R);
  }
}

int SessionCore::check_selected(int selected) const {
  if (selected >= 0 && selected < R) return DCORA_OK;
  set_last_error(std::string(tag_) + ": selected agent out of range");
  return DCORA_ERR_BAD_ARG;
}

int SessionCore::agent_colours(int *colours, int *ncolours) {
  const int nc = greedy_agent_colours(R, [&](int a) -> const std::vector<int> & { return agent_core(a).neighbors; },
                                      colours);
  if (ncolours) *ncolours = nc;
  return DCORA_OK;
}

int SessionCore::drain(bool then_session) {
  for (int a = 0; a < R; ++a)
    if (agent_core(a).own_st) DCORA_HIP(hipStreamSynchronize(agent_core(a).own_st));
  if (then_session) DCORA_HIP(hipStreamSynchronize(st));
  return DCORA_OK;
}

int SessionCore::redimension(const char *what, int r_new, const double *X_dev, RankChange<DeviceProblem> &change) {
  DevBuf<double> xq;
  if (cert_.built && hipSuccess != xq.alloc((size_t)r_new * (size_t)num_cols())) {
    (void)hipGetLastError();
    set_last_error(std::string(tag_) + " " + what + ": out of device memory");
    return DCORA_ERR_HIP;
  }
  int rc = lift_buffers(r_new);
  if (rc) return rc;
  if (cert_.built) cert_.XQ = std::move(xq);
  change.commit();  // (the session is at r_new from here on: nothing is left to take back)
  rc = lift_adopt(X_dev);
  if (rc) return rc;
  DCORA_HIP(hipStreamSynchronize(st));
  return DCORA_OK;
}

int SessionCore::scatter_block(const AgentBlock &blk, int rows, const double *block, double *mirror) {
  if (blk.contiguous())
    DCORA_HIP(hipMemcpyAsync(mirror + (size_t)blk.col0 * rows, block, sizeof(double) * (size_t)rows * blk.k,
                             hipMemcpyDeviceToDevice, st));
  else
    launch_scatter_cols(st, rows, blk.k, blk.cols_dev, block, mirror);
  return DCORA_OK;
}

int SessionCore::x_stage_hosted(double *host_area) {
  DCORA_HIP(hipSetDevice(opt.device));
  bool listed = false;
  for (int a = 0; a < R; ++a) {
    if (!agent_core(a).hosted) continue;
    const AgentBlock blk = agent_block(a);
    if (blk.contiguous())
      DCORA_HIP(hipMemcpyAsync(host_area + (size_t)blk.col0 * r, blk.X, sizeof(double) * (size_t)r * blk.k,
                               hipMemcpyDeviceToHost, st));
    else
      listed = true;
  }
  std::vector<double> whole(listed ? (size_t)r * (size_t)num_cols() : 0);
  if (listed) DCORA_HIP(hipMemcpyAsync(whole.data(), Xg.p, sizeof(double) * whole.size(), hipMemcpyDeviceToHost, st));
  DCORA_HIP(hipStreamSynchronize(st));
  for (int a = 0; listed && a < R; ++a) {
    if (!agent_core(a).hosted) continue;
    const AgentBlock blk = agent_block(a);
    for (int j = 0; j < blk.k; ++j) {
      const size_t c = (size_t)blk.cols_host[j];
      std::copy(&whole[c * r], &whole[c * r] + r, host_area + c * r);
    }
  }
  return DCORA_OK;
}

int SessionCore::certify(double eta, CertifyResult *out, double *info8) {
  DeviceProblem *central = opt.world_size == 1 ? central_problem() : nullptr;
  if (!central) {
    set_last_error(std::string(tag_) + ": certify serves single-process sessions (world_size 1); the ranks of a job "
                   "certify together through dcora_exchange_certify");
    return DCORA_ERR_UNSUPPORTED;
  }
  DCORA_HIP(hipSetDevice(opt.device));
  // the mirror is complete: nothing of the session is in flight on an agent's own stream
  int rc = drain(false);
  if (rc) return rc;
  // a robust session keeps a host copy of the central pattern and, where it certifies over those alone, of the stored
  // entries the current weights give (session_cert.h; an empty live pattern is none)
  return session_certify(cert_, *central, robust ? &robust->central_pat : nullptr,
                         robust ? &robust->live_pat : nullptr, Xg.p, cert_block(), eta, out, info8);
}

int SessionCore::lift(double theta, const double *v, const dcora_lift_params &p, int *escaped, double *info8) {
  const std::string tag = std::string(tag_) + " lift: ";
  using clock = std::chrono::steady_clock;
  auto ms_since = [](clock::time_point t) { return std::chrono::duration<double, std::milli>(clock::now() - t).count(); };
  *escaped = 0;
  if (info8) std::fill(info8, info8 + 8, 0.0);
  DeviceProblem *central = opt.world_size == 1 ? central_problem() : nullptr;
  if (!central || weights_ranked() || (team && team->ranked) || exchange_attached) {
    set_last_error(tag + "serves single-process sessions without an exchange; the ranks of a job, and a session an "
                   "exchange was created on, lift together through dcora_exchange_lift");
    return DCORA_ERR_UNSUPPORTED;
  }
  if (r + 1 > kMaxRank) {
    set_last_error(tag + "the session is at rank 16, the largest the kernels are built for");
    return DCORA_ERR_BAD_ARG;
  }
  const long k = num_cols();
  if (!lift_args_finite(theta, v, k, p.gradient_tolerance, p.preconditioned_gradient_tolerance) ||
      !std::isfinite(p.central_reg)) {
    set_last_error(tag + "v must be k finite numbers, theta, the tolerances and central_reg finite");
    return DCORA_ERR_BAD_ARG;
  }
  const auto t0 = clock::now();
  DCORA_HIP(hipSetDevice(opt.device));
  // a. nothing of the session is in flight
  int rc = drain(true);
  if (rc) return rc;
  // b. escapeSaddle's PreCondition: of the central Q as the device holds it now (the current weights)
  if (!central->has_precond || central->precond_stale) {
    const auto tb = clock::now();
    HostCsr Qc;
    rc = central->Q.download(&Qc);
    if (rc) return rc;
    double reg = p.central_reg;
    if (reg < 0 && (rc = lift_default_reg(Qc, &reg))) return rc;
    rc = central->build_preconditioner(Qc, reg);
    if (rc) return rc;
    if (info8) info8[4] = 1, info8[5] = ms_since(tb);
  }
  // c. the central problem at r + 1, the escape from the mirror; v is all that comes from the host
  const int r_new = r + 1;
  RankChange<DeviceProblem> change(r);  // (what it holds goes back to r on every way out before the commit)
  rc = change.add(central, r_new);
  if (rc) return rc;
  int ok = 0;
  double stats[4] = {0, 0, 0, 0};
  // (v into a slice of the central workspace the search does not use)
  if (hipMemcpyAsync(central->Hd.p, v, sizeof(double) * (size_t)k, hipMemcpyHostToDevice, st) != hipSuccess) {
    set_last_error(tag + "the copy of v to the device failed");
    rc = DCORA_ERR_HIP;
  }
  if (!rc)
    rc = central->escape_saddle_dev(Xg.p, central->Hd.p, theta, p.gradient_tolerance,
                                    p.preconditioned_gradient_tolerance, p.is_second_order != 0, &ok, stats);
  if (info8) std::copy(stats, stats + 4, info8);
  if (rc || !ok) {  // d.
    change.rollback();
    if (info8) info8[7] = ms_since(t0);
    return rc;
  }
  // e. the agents' problems, then the session re-dimensioned at the accepted point
  const auto te = clock::now();
  for (int a = 0; a < R; ++a) {
    if (!agent_core(a).hosted) continue;
    rc = change.add(agent_core(a).prob.get(), r_new);
    if (rc) return rc;
  }
  rc = redimension("lift", r_new, central->X1.p, change);
  if (rc) return rc;
  *escaped = 1;
  if (info8) info8[6] = ms_since(te), info8[7] = ms_since(t0);
  return DCORA_OK;
}

int SessionCore::reserve_rank(int r_reserve) {
  const std::string tag = std::string(tag_) + " reserve_rank: ";
  if (exchange_attached) {
    set_last_error(tag + "an exchange exists on the session: its segment is mapped and its halo buffers are shared "
                   "(reserve before dcora_exchange_create / _create_ra, or create with a *_ranks_reserved entry)");
    return DCORA_ERR_UNSUPPORTED;
  }
  if (reserve_rank_check(dim(), r, r_reserve, false)) {
    set_last_error(tag + "need d <= r <= r_reserve <= 16");
    return DCORA_ERR_BAD_ARG;
  }
  reserve_r = r_reserve;
  return DCORA_OK;
}

// ---- the session's half of the collective lift (session_core.h) -----------------------------------------------------
int SessionCore::lift_trial_begin(const double *v_host) {
  const std::string tag = std::string(tag_) + " lift: ";
  DCORA_HIP(hipSetDevice(opt.device));
  int rc = drain(true);
  if (rc) return rc;
  std::unique_ptr<LiftTrial> t(new LiftTrial(r));  // (leaving before it is the session's takes its re-ranks back)
  const int r_new = r + 1;
  const size_t k = (size_t)num_cols();
  for (int a = 0; a < R; ++a) {
    if (!agent_core(a).hosted) continue;
    if (!agent_core(a).prob->has_precond) {
      set_last_error(tag + "agent " + std::to_string(a) + " has no preconditioner");
      return DCORA_ERR_NO_PRECONDITIONER;
    }
    t->hosted.push_back(a);
  }
  if (hipSuccess != t->mirror.alloc((size_t)r_new * k) || hipSuccess != t->v.alloc(k) ||
      hipSuccess != t->scal.alloc(4 * std::max<size_t>(t->hosted.size(), 1))) {
    (void)hipGetLastError();
    set_last_error(tag + "out of device memory");
    return DCORA_ERR_HIP;
  }
  // (columns no hosted agent owns and no neighbour publishes are read by nobody: zero, as a fresh mirror has them)
  DCORA_HIP(hipMemsetAsync(t->mirror.p, 0, sizeof(double) * (size_t)r_new * k, st));
  DCORA_HIP(hipMemcpyAsync(t->v.p, v_host, sizeof(double) * k, hipMemcpyHostToDevice, st));
  DCORA_HIP(hipStreamSynchronize(st));  // (the caller's pageable v has been read)
  const auto tr = std::chrono::steady_clock::now();
  for (int id : t->hosted) {  // (a failure: what has been re-ranked so far goes back; the agents behind never left r)
    rc = t->change.add(agent_core(id).prob.get(), r_new);
    if (rc) return rc;
  }
  t->rerank_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tr).count();
  for (int id : t->hosted) {
    const AgentBlock blk = agent_block(id);
    DeviceProblem &pb = *agent_core(id).prob;
    launch_lift_images_agent(st, r, pb.m.k, blk.X, t->v.p, blk.cols_dev, blk.col0, pb.X0.p, pb.eta.p);
  }
  lift_trial_ = std::move(t);
  DCORA_HIP(hipGetLastError());
  return DCORA_OK;
}

int SessionCore::lift_trial_point(double alpha, double **mirror) {
  LiftTrial &t = *lift_trial_;
  DCORA_HIP(hipSetDevice(opt.device));
  for (int id : t.hosted) {
    DeviceProblem &pb = *agent_core(id).prob;
    pb.escape_trial_point(alpha);
    const int rc = scatter_block(agent_block(id), t.change.r_old() + 1, pb.X1.p, t.mirror.p);
    if (rc) return rc;
  }
  DCORA_HIP(hipGetLastError());
  *mirror = t.mirror.p;
  return DCORA_OK;
}

int SessionCore::lift_trial_scalars(double out3[3]) {
  LiftTrial &t = *lift_trial_;
  DCORA_HIP(hipSetDevice(opt.device));
  const int r_new = t.change.r_old() + 1;
  for (size_t i = 0; i < t.hosted.size(); ++i) {
    AgentCore &a = agent_core(t.hosted[i]);
    DeviceProblem &pb = *a.prob;
    launch_spmm(st, r_new, a.coupling.view(), buf1(t.mirror.p), 0, nullptr, buf1(pb.G.p), 0, nullptr, Gate{});
    pb.has_G = true;
    pb.escape_trial_scalars(t.scal.p + 4 * i);
  }
  DCORA_HIP(hipGetLastError());
  std::vector<double> h(4 * std::max<size_t>(t.hosted.size(), 1), 0.0);
  if (!t.hosted.empty())
    DCORA_HIP(hipMemcpyAsync(h.data(), t.scal.p, sizeof(double) * 4 * t.hosted.size(), hipMemcpyDeviceToHost, st));
  DCORA_HIP(hipStreamSynchronize(st));  // the trial's one wait (a rank without agents still drains its scatters)
  out3[0] = out3[1] = out3[2] = 0;
  for (size_t i = 0; i < t.hosted.size(); ++i) {  // agent order
    out3[0] += h[4 * i] + h[4 * i + 1];
    out3[1] += h[4 * i + 2];
    out3[2] += h[4 * i + 3];
  }
  return DCORA_OK;
}

void SessionCore::lift_trial_abort() {
  if (!lift_trial_) return;
  (void)hipSetDevice(opt.device);
  lift_trial_.reset();  // (its RankChange rolls back)
}

int SessionCore::lift_trial_commit(double *redim_ms) {
  const auto te = std::chrono::steady_clock::now();
  LiftTrial &t = *lift_trial_;
  const int r_new = t.change.r_old() + 1;
  DCORA_HIP(hipSetDevice(opt.device));
  int rc = DCORA_OK;
  if (DeviceProblem *central = central_problem()) {  // (a one-rank job keeps its whole-graph evaluation)
    rc = t.change.add(central, r_new);
    if (rc) return rc;
  }
  // (a failure before redimension's commit leaves the re-ranks to lift_trial_abort; after it nothing is left to it)
  rc = redimension("lift", r_new, t.mirror.p, t.change);
  if (rc) return rc;
  // (what SessionCore::lift counts in the same slot: the agents' re-ranks, made when the trials began, with the rest)
  if (redim_ms)
    *redim_ms = t.rerank_ms + std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - te).count();
  lift_trial_.reset();
  return DCORA_OK;
}

int SessionCore::acquire_stream(void *borrowed) {
  own_stream_ = !borrowed;
  if (borrowed) st = (hipStream_t)borrowed;
  return borrowed ? DCORA_OK : stream_acquire(opt.device, &st);
}

int SessionCore::acquire_tick_resources(AgentCore &a) {
  const int rc = stream_acquire(opt.device, &a.own_st);  // (at most kMaxAgents of them: R <= kMaxAgents)
  if (rc) return rc;
  DCORA_HIP(hipEventCreateWithFlags(&a.done, hipEventDisableTiming));
  return DCORA_OK;
}

int SessionCore::create_fork_event() {
  DCORA_HIP(hipEventCreateWithFlags(&fork_ev_, hipEventDisableTiming));
  return DCORA_OK;
}

void SessionCore::release_tick_resources(AgentCore &a) {
  if (a.own_st) stream_release(opt.device, a.own_st);
  if (a.done) (void)hipEventDestroy(a.done);
  a.own_st = nullptr;
  a.done = nullptr;
}

void SessionCore::release_stream() {
  if (fork_ev_) (void)hipEventDestroy(fork_ev_);
  if (st && own_stream_) stream_release(opt.device, st);
  fork_ev_ = nullptr;
  st = nullptr;
}

// Local solve of one agent of a tick from what stage() enqueued, then its block into the mirror: on the session's stream
// (serial: the set's solves one after the other, each free to run its tCG runs as ONE launch, k_tcg_run) or on the
// agent's own, side by side with the set's other solves, on the launches per iteration.
int SessionCore::solve_block(AgentCore &a, std::string *err, bool serial) {
  auto fail = [&](int rc) {
    *err = dcora_last_error();
    return rc;
  };
  if (hipSetDevice(opt.device) != hipSuccess) return fail(DCORA_ERR_HIP);
  DeviceProblem &pb = *a.prob;
  hipStream_t keep = pb.st;
  hipStream_t run_on = serial ? st : a.own_st;
  pb.st = run_on;
  pb.concurrent_solves = !serial;  // several solves share the device: no co-resident one-launch tCG run
  int rc = pb.optimize_dev(opt.local);
  pb.concurrent_solves = false;
  if (!rc) rc = write_back(a, run_on);
  if (!rc && !serial && hipEventRecord(a.done, a.own_st) != hipSuccess) rc = DCORA_ERR_HIP;
  pb.st = keep;
  return rc ? fail(rc) : DCORA_OK;
}

int SessionCore::iterate_set(const int *set, int count, int allow_adjacent) {
  const std::string tag = std::string(tag_) + ": ";
  if (opt.acceleration) {
    set_last_error(tag + "simultaneous updates need acceleration off (ref src/Agent.cpp:651-653)");
    return DCORA_ERR_UNSUPPORTED;
  }
  if (!set || count < 1 || count > R) {
    set_last_error(tag + "bad agent set");
    return DCORA_ERR_BAD_ARG;
  }
  std::vector<char> in((size_t)R, 0);
  for (int i = 0; i < count; ++i) {
    if (set[i] < 0 || set[i] >= R || in[(size_t)set[i]]) {
      set_last_error(tag + "agent set has an id out of range or twice");
      return DCORA_ERR_BAD_ARG;
    }
    in[(size_t)set[i]] = 1;
  }
  if (!allow_adjacent)
    for (int i = 0; i < count; ++i)
      for (int q : agent_core(set[i]).neighbors)
        if (in[(size_t)q]) {
          set_last_error(tag + "agents " + std::to_string(set[i]) + " and " + std::to_string(q) +
                         " share measurements; pass allow_adjacent to update them from one snapshot anyway");
          return DCORA_ERR_BAD_ARG;
        }
  DCORA_HIP(hipSetDevice(opt.device));
  iteration++;
  inner_rounds++;
  tick_begins();
  std::vector<AgentCore *> work;
  for (int i = 0; i < count; ++i)
    if (agent_core(set[i]).hosted) work.push_back(&agent_core(set[i]));
  if (work.empty()) return DCORA_OK;
  // snapshot: every G, every start point and every XPrev is taken before any block is written back
  for (AgentCore *a : work) {
    const int rc = stage(*a);
    if (rc) return rc;
  }
  std::vector<int> rcs(work.size(), DCORA_OK);
  std::vector<std::string> errs(work.size());
  auto failed = [&](size_t i) {
    if (rcs[i]) set_last_error(errs[i]);
    return rcs[i];
  };
  if (serial_set(work)) {  // in set order; the staged G / start points make the order immaterial
    for (size_t i = 0; i < work.size(); ++i) {
      rcs[i] = solve_block(*work[i], &errs[i], true);
      if (failed(i)) return rcs[i];
    }
    last_solver = work.back()->prob.get();
    return tick_done(work);
  }
  DCORA_HIP(hipEventRecord(fork_ev_, st));
  for (AgentCore *a : work) DCORA_HIP(hipStreamWaitEvent(a->own_st, fork_ev_, 0));
  if (work.size() == 1) {
    rcs[0] = solve_block(*work[0], &errs[0], false);
  } else {
    // the solver paces each solve from the host (device_problem.hip): one host thread per concurrent solve
    run_threads((int)work.size(),
                [&](int i) { rcs[(size_t)i] = solve_block(*work[(size_t)i], &errs[(size_t)i], false); });
  }
  last_solver = work.back()->prob.get();
  for (size_t i = 0; i < work.size(); ++i) {
    if (failed(i)) return rcs[i];
    DCORA_HIP(hipStreamWaitEvent(st, work[i]->done, 0));
  }
  return tick_done(work);
}

// ---- the team protocol ----------------------------------------------------------------------------------------------
int SessionCore::team_enable(const dcora_team_params &p) {
  const std::string tag = std::string(tag_) + " team: ";
  if (opt.world_size != 1) {
    set_last_error(tag + "only single-process sessions (world_size 1) keep the team's statuses by themselves; "
                   "the ranks of a job, pose-graph or range-aided, enable the team through their exchange "
                   "(dcora_exchange_team_enable, on a range-aided job dcora_exchange_team_enable_ra)");
    return DCORA_ERR_UNSUPPORTED;
  }
  if (team && team->ranked) {
    set_last_error(tag + "the session's team was enabled through its exchange (dcora_exchange_team_enable / _ra)");
    return DCORA_ERR_UNSUPPORTED;
  }
  if (!team) {
    std::unique_ptr<TeamState> t(new TeamState);
    DCORA_HIP(hipSetDevice(opt.device));
    DCORA_HIP(hipHostMalloc((void **)&t->rel_host, sizeof(double) * kMaxAgents, hipHostMallocMapped));
    std::memset((void *)t->rel_host, 0, sizeof(double) * kMaxAgents);
    DCORA_HIP(hipHostGetDevicePointer((void **)&t->rel_dev, (void *)t->rel_host, 0));
    team = std::move(t);
    team_clear_statuses();
    team->latest_weight_update_iteration = 0;
    team_refresh_counts();
  }
  team->params = p;
  return DCORA_OK;
}

// The half of a rank of a job, through its exchange only: the status area and the job's weights the exchange keeps.
int SessionCore::team_enable_ranked(const dcora_team_params &p, ShmStatus *slots, ShmStatus *slots_dev,
                                    const double *job_w) {
  if (team && !team->ranked) {
    set_last_error(std::string(tag_) + " team: the session's team was enabled by dcora_" + tag_ + "_team_enable");
    return DCORA_ERR_UNSUPPORTED;
  }
  if (!team) {
    team.reset(new TeamState);
    team->ranked = true;
    team->slots = slots;
    team->slots_dev = slots_dev;
    team->seq.assign((size_t)R, 0);
    team_clear_statuses();
    team->latest_weight_update_iteration = 0;
  }
  team->job_w = job_w;
  team_refresh_counts();
  team->params = p;
  return DCORA_OK;
}

void SessionCore::team_clear_statuses() {
  if (!team) return;
  team->status.assign((size_t)R, dcora_agent_status{});
  team->have.assign((size_t)R, 0);
  team->pending.assign((size_t)R, TeamState::Pending());
}

// a weight update has been made in this round: mLatestWeightUpdateIteration, mRobustOptInnerIter = 0,
// mTeamStatus.clear() (ref src/Agent.cpp:1418-1424)
void SessionCore::team_weights_updated() {
  inner_rounds = 0;
  if (!team) return;
  team->latest_weight_update_iteration = iteration;
  team_clear_statuses();
}

// the round counter restarts (set_X, set_acceleration, Agent::setX of every agent): what the team counts in rounds
// restarts with it
void SessionCore::team_restart_rounds() {
  inner_rounds = 0;
  if (!team) return;
  team->latest_weight_update_iteration = 0;
  team_clear_statuses();
}

void SessionCore::team_refresh_counts() {
  team->lc.assign((size_t)R * 3, 0);
  for (const TeamLoopClosure &q : team_lcs_) team_count_loop_closure(team->lc.data(), q, team_lc_weight(q));
}

// Agent::iterate's status block (ref src/Agent.cpp:558-586) for the agents that just optimised: marked, then the session
// kind's one launch behind everything their updates enqueued on the session's stream
int SessionCore::team_note_optimized(const int *ids, int count) {
  std::vector<int> marked;
  for (int i = 0; i < count && (int)marked.size() < kMaxAgents; ++i) {
    const int b = ids[i];
    if (b < 0 || b >= R || !agent_core(b).hosted) continue;
    team_mark_optimized(b, team_last_success(b));
    marked.push_back(b);
  }
  return team_launch_rel_change(marked);
}

// what every rank knows of an optimisation of agent b in this round (ranked: hosted here or not)
void SessionCore::team_mark_optimized(int b, bool success) {
  dcora_agent_status &s = team->status[(size_t)b];
  s.agent_id = b;
  s.state = DCORA_AGENT_INITIALIZED;
  s.instance_number = 0;
  s.iteration_number = iteration;
  s.ready_to_terminate = 0;
  s.relative_change = 0;
  team->have[(size_t)b] = 1;
  TeamState::Pending &p = team->pending[(size_t)b];
  p.on = true;
  p.success = success;
  p.updates = team_weight_updates();
  for (int c = 0; c < 3; ++c) p.lc[c] = team->lc[(size_t)b * 3 + c];
  if (team->ranked) team->seq[(size_t)b]++;
}

// ranked: what team_note_optimized keeps for those agents of ids that live on another rank
void SessionCore::team_note_elsewhere(const int *ids, int count) {
  for (int i = 0; i < count; ++i) {
    const int b = ids[i];
    if (b >= 0 && b < R && !agent_core(b).hosted) team_mark_optimized(b, false);  // (success arrives with the slot)
  }
}

// ranked, for hosted agents just marked: `success` into the slot their optimisation publishes into (released by
// Exchange::team_clear_to_write before the agent's update was enqueued), visible before the kernel's stores; the
// ranked k_rel_change's argument
RelChangePublish SessionCore::team_publish_slots(const std::vector<int> &ids) {
  RelChangePublish pub{};
  int i = 0;
  for (int b : ids) {
    const uint64_t q = team->seq[(size_t)b];
    team->slots[(size_t)(q & 1) * R + b].success = team->pending[(size_t)b].success ? 1u : 0u;
    pub.seq[i++] = q;
  }
  std::atomic_thread_fence(std::memory_order_release);
  pub.slots = team->slots_dev;
  pub.R = R;
  return pub;
}

// ranked: the two facts the hosting rank published for one agent settled into its status
void SessionCore::team_settle_published(int b, bool success, double relative_change) {
  TeamState::Pending &p = team->pending[(size_t)b];
  if (!p.on) return;
  p.on = false;
  p.success = success;
  dcora_agent_status &s = team->status[(size_t)b];
  s.relative_change = relative_change;
  s.ready_to_terminate = team_ready_to_terminate(team->params, team_robust(), p.updates, p.success, s.relative_change,
                                                 p.lc[0], p.lc[1], p.lc[2]) ? 1 : 0;
}

int SessionCore::team_settle(bool visible) {
  bool any = false;
  for (const TeamState::Pending &p : team->pending) any = any || p.on;
  if (!any || team->ranked) return DCORA_OK;  // (ranked: settled by the exchange's collective calls alone)
  if (!visible) {
    DCORA_HIP(hipSetDevice(opt.device));
    DCORA_HIP(hipStreamSynchronize(st));
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  for (int b = 0; b < R; ++b) {
    TeamState::Pending &p = team->pending[(size_t)b];
    if (!p.on) continue;
    p.on = false;
    dcora_agent_status &s = team->status[(size_t)b];
    s.relative_change = const_cast<const volatile double *>(team->rel_host)[b];
    s.ready_to_terminate = team_ready_to_terminate(team->params, team_robust(), p.updates, p.success,
                                                   s.relative_change, p.lc[0], p.lc[1], p.lc[2]) ? 1 : 0;
  }
  return DCORA_OK;
}

int SessionCore::team_agent_status(int agent, dcora_agent_status *status, int *known) {
  const int rc = team_settle(false);
  if (rc) return rc;
  if (team->have[(size_t)agent]) {
    *status = team->status[(size_t)agent];
  } else {
    *status = dcora_agent_status{};
    status->agent_id = agent;
    status->state = DCORA_AGENT_INITIALIZED;
    status->iteration_number = team_iteration_number(agent);
  }
  if (known) *known = team->have[(size_t)agent];
  return DCORA_OK;
}

int SessionCore::team_decide(int *should_terminate, int *should_update_weights) {
  const int rc = team_settle(false);
  if (rc) return rc;
  const TeamView v{team_robust(), iteration, team_weight_updates(), team_inner_iter(),
                   team->latest_weight_update_iteration, team->status.data(), team->have.data(), nullptr, R};
  if (should_terminate) *should_terminate = team_should_terminate(team->params, v) ? 1 : 0;
  if (should_update_weights) *should_update_weights = team_should_update_weights(team->params, v) ? 1 : 0;
  return DCORA_OK;
}

// the agents' own loop (ref src/Agent.cpp:650-678 shape, the synchronous schedule of examples/MultiRobotExample.cpp):
// stop and re-weight by the team rules instead of a central gradient norm and fixed counts
int SessionCore::run_team(int *iters_done, double *cost2_trace, double *gradnorm_trace, int *selected_trace,
                          int *updated_trace, int *weight_updates, int *stop_reason) {
  const int cap = team->params.max_num_iters;
  int selected = 0, it = 0, nupd = 0;
  for (;;) {
    int stop = 0, upd = 0;
    int rc = team_decide(&stop, nullptr);
    if (rc) return rc;
    if (stop || it >= cap) break;
    rc = team_decide(nullptr, &upd);
    if (rc) return rc;
    if (updated_trace) updated_trace[it] = upd;
    if (upd) {
      const bool reset = team->resets_done < team->params.robust_opt_num_resets;
      rc = update_weights(reset, nullptr);
      if (rc) return rc;
      if (reset) team->resets_done++;
      nupd++;
    }
    double c2 = 0, gn = 0;
    int nxt = selected;
    rc = team_iterate(selected, &c2, &gn, &nxt);
    if (rc) return rc;
    if (cost2_trace) cost2_trace[it] = c2;
    if (gradnorm_trace) gradnorm_trace[it] = gn;
    if (selected_trace) selected_trace[it] = selected;
    selected = nxt;
    ++it;
  }
  if (iters_done) *iters_done = it;
  if (weight_updates) *weight_updates = nupd;
  if (stop_reason) *stop_reason = iteration >= cap ? DCORA_TEAM_STOP_MAX_ITERS : DCORA_TEAM_STOP_ALL_READY;
  return DCORA_OK;
}

}  // namespace dcora
