// The team protocol's three rules, stated once (host only, no HIP): what an agent calls itself after an optimisation
// (Agent::iterate, ref src/Agent.cpp:567-585), when the team stops (Agent::shouldTerminate, :1123-1156) and when it
// re-weights its measurements (Agent::shouldUpdateMeasurementWeights, :1280-1330).  The session (rbcd.hip) and the
// facade (DCORA/Agent.h, through the C ABI) both decide through these, each with its own knowledge of the team.
#pragma once
#include "../../include/dcora_hip.h"

namespace dcora {

inline dcora_team_params team_params_default() {  // ref include/DCORA/Agent.h:113-125
  dcora_team_params p;
  p.max_num_iters = 500;
  p.rel_change_tol = 5e-3;
  p.robust_opt_num_weight_updates = 10;
  p.robust_opt_num_resets = 0;
  p.robust_opt_inner_iters = 30;
  p.robust_opt_min_convergence_ratio = 0.8;
  return p;
}

// ref src/Agent.cpp:567-585
inline bool team_ready_to_terminate(const dcora_team_params &p, bool robust, int weight_update_count, bool success,
                                    double relative_change, int accepted, int rejected, int total) {
  bool ready = true;
  if (!success) ready = false;
  double tol = p.rel_change_tol;
  if (robust && weight_update_count == 0) tol = 5;  // loose threshold during the initial inner iterations
  if (relative_change > tol) ready = false;
  // share of the loop closures whose weight is decided; 0 / 0 is NaN and compares false, as in the reference
  const double ratio = ((double)accepted + (double)rejected) / (double)total;
  if (ratio < p.robust_opt_min_convergence_ratio) ready = false;
  return ready;
}

// Graph::statistics (ref src/Graph.cpp:475-521) over private_lcs_ and shared_lcs_, which by Graph::addMeasurement
// (:121-134) hold every measurement but pose-pose odometry.  One entry per such measurement: the agents owning its two
// ends (it counts at each, once when they are the same), its weight at creation, and id: where its current weight is
// kept when a session re-weights it (a measurement index; < 0: the weight never changes).
struct TeamLoopClosure {
  int id, a1, a2;
  double w0;
};
// counts: 3 per agent -- accepted (weight == 1 exactly), rejected (weight == 0 exactly), all
inline void team_count_loop_closure(int *counts, const TeamLoopClosure &q, double weight) {
  auto count = [&](int a) {
    int *c = counts + 3 * (long)a;
    if (weight == 1) c[0]++;
    else if (weight == 0) c[1]++;
    c[2]++;
  };
  count(q.a1);
  if (q.a2 != q.a1) count(q.a2);
}

struct TeamView {
  bool robust;
  int iteration_number, weight_update_count, inner_iter, latest_weight_update_iteration;
  const dcora_agent_status *statuses;
  const int *have, *active;  // active == nullptr: every robot is active
  int num_robots;
  bool is_active(int q) const { return !active || active[q]; }
};

// ref src/Agent.cpp:1123-1156
inline bool team_should_terminate(const dcora_team_params &p, const TeamView &t) {
  if (t.iteration_number >= p.max_num_iters) return true;
  if (t.robust && t.weight_update_count < p.robust_opt_num_weight_updates) return false;
  for (int q = 0; q < t.num_robots; ++q) {
    if (!t.is_active(q)) continue;
    if (!t.have[q]) return false;
    if (t.statuses[q].state != DCORA_AGENT_INITIALIZED) return false;
    if (!t.statuses[q].ready_to_terminate) return false;
  }
  return true;
}

// ref src/Agent.cpp:1280-1330
inline bool team_should_update_weights(const dcora_team_params &p, const TeamView &t) {
  if (!t.robust) return false;
  if (t.weight_update_count >= p.robust_opt_num_weight_updates) return false;
  if (t.inner_iter >= p.robust_opt_inner_iters) return true;
  for (int q = 0; q < t.num_robots; ++q) {
    if (!t.is_active(q)) continue;
    if (!t.have[q]) return false;
    if (t.statuses[q].iteration_number < t.latest_weight_update_iteration) return false;  // outdated
    if (t.statuses[q].state != DCORA_AGENT_INITIALIZED) return false;
    if (!t.statuses[q].ready_to_terminate) return false;
  }
  return true;
}

}  // namespace dcora
