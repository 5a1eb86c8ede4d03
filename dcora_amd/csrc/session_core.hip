// The session core on the host (see session_core.h).
#include "session_core.h"

#include <cmath>

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

int SessionCore::certify(double eta, CertifyResult *out, double *info8) {
  DeviceProblem *central = opt.world_size == 1 ? central_problem() : nullptr;
  if (!central) {
    set_last_error(std::string(tag_) + ": certify serves single-process sessions (world_size 1); the ranks of a job "
                   "certify together through dcora_exchange_certify");
    return DCORA_ERR_UNSUPPORTED;
  }
  DCORA_HIP(hipSetDevice(opt.device));
  // the mirror is complete: nothing of the session is in flight on an agent's own stream
  for (int a = 0; a < R; ++a)
    if (agent_core(a).own_st) DCORA_HIP(hipStreamSynchronize(agent_core(a).own_st));
  return session_certify(cert_, *central, central_pattern(), central_live_pattern(), Xg.p, cert_block(), eta, out,
                         info8);
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

}  // namespace dcora
