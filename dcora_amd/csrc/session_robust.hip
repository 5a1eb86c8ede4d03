// Robust measurement weights of a live session, for both session kinds (see RobustState in session_core.h).
#include <cmath>

#include "session_core.h"

namespace dcora {

int SessionCore::robust_check_args(const std::vector<PoseMeas> &meas, int num_poses, const dcora_rbcd_options &o,
                                   const dcora_robust_params &p, bool ranked) const {
  const std::string tag = std::string(tag_) + " robust: ";
  if (o.world_size != 1 && !ranked) {
    set_last_error(tag + "only single-process sessions (world_size 1) update weights here; a multi-rank job creates its "
                   "sessions with dcora_" + tag_ + "_create_robust_ranks");
    return DCORA_ERR_UNSUPPORTED;
  }
  if (p.cost_type < DCORA_ROBUST_L2 || p.cost_type > DCORA_ROBUST_GNC_TLS) {
    set_last_error(tag + "unknown robust cost type");
    return DCORA_ERR_BAD_ARG;
  }
  for (const PoseMeas &q : meas)
    if (q.p1 < 0 || q.p1 >= num_poses || q.p2 < 0 || q.p2 >= num_poses) {
      set_last_error(tag + "pose index out of range");
      return DCORA_ERR_BAD_ARG;
    }
  return DCORA_OK;
}

// Agent::initializeRobustOptimization for every agent (ref src/Agent.cpp:1332-1346): weight 1 on every loop closure
// whose weight is not fixed.  With weights 1 the patterns are the largest any later weights can give: the kind records
// them when it creates itself, and a weight change only rewrites values.
void SessionCore::robust_begin(const std::vector<PoseMeas> &meas, const std::vector<char> &lc,
                               const dcora_robust_params &p, const int *fixed, bool ranked) {
  robust.reset(new RobustState(p));
  RobustState &rs = *robust;
  rs.ranked = ranked;
  const size_t m = meas.size();
  rs.w.resize(m);
  rs.update.assign(m, 0);
  rs.meas_zero.assign(m, 0);
  rs.owned.assign(m, 0);
  for (size_t e = 0; e < m; ++e) {
    rs.update[e] = lc[e] && !(fixed && fixed[e]);
    rs.w[e] = rs.update[e] ? 1.0 : meas[e].weight;
    rs.meas_zero[e] = rs.w[e] == 0.0;
  }
}

int SessionCore::robust_finish() {
  RobustState &rs = *robust;
  const int rc = robust_upload_edges();
  if (rc) return rc;
  const size_t N = (size_t)r * (size_t)num_cols();
  DCORA_HIP(rs.X_initial.alloc(N));
  DCORA_HIP(hipMemsetAsync(rs.X_initial.p, 0, sizeof(double) * N, st));
  DCORA_HIP(hipStreamSynchronize(st));
  return DCORA_OK;
}

// Agent::updateMeasurementWeights for every agent (ref src/Agent.cpp:1397-1441): the weights of the current iterate
// (k_robust_weights reads the mirror), the data matrices rebuilt, RobustCost::update, optionally X back to the last
// set_X (robustOptNumResets), acceleration re-initialised
int SessionCore::update_weights(bool reset_to_initial, int counts[3]) {
  std::vector<double> w;
  double cnt[3] = {0, 0, 0};
  int rc = compute_weights(nullptr, &w, cnt);
  if (rc) return rc;
  rc = apply_weights(w, reset_to_initial);
  if (rc) return rc;
  if (counts)
    for (int c = 0; c < 3; ++c) counts[c] = (int)cnt[c];
  return DCORA_OK;
}

// w: the weights of the session's edges (RobustState::edge_ids order), counts as launch_robust_weights gives them
int SessionCore::compute_weights(double *shared_w, std::vector<double> *w, double counts[3]) {
  RobustState &rs = *robust;
  if (rs.ranked && !shared_w && !rs.edge_ids.empty()) {
    set_last_error(std::string(tag_) + " robust: a ranked session's weights are computed by its exchange "
                   "(dcora_exchange_update_weights)");
    return DCORA_ERR_UNSUPPORTED;
  }
  DCORA_HIP(hipSetDevice(opt.device));
  const int rc = drain(false);  // the mirror is complete
  if (rc) return rc;
  const size_t m = rs.edge_ids.size();
  w->assign(m, 0.0);
  for (int c = 0; c < 3; ++c) counts[c] = 0;
  if (m) {
    launch_robust_weights(st, rs.edges, r, Xg.p, rs.params, rs.cost.mu(), shared_w);
    DCORA_HIP(hipGetLastError());
    DCORA_HIP(hipMemcpyAsync(w->data(), rs.edges.w.p, sizeof(double) * m, hipMemcpyDeviceToHost, st));
    DCORA_HIP(hipMemcpyAsync(counts, rs.edges.counts.p, sizeof(double) * 3, hipMemcpyDeviceToHost, st));
  }
  DCORA_HIP(hipStreamSynchronize(st));
  return DCORA_OK;
}

// The shared tail of both ways to change weights: the matrices rebuilt for w, the device's weights made the ones the
// matrices hold -- the old ones after a refusal, the new ones unless the device computed them itself (from_device) --,
// optionally X back to the last set_X, acceleration re-initialised
int SessionCore::adopt_weights(std::vector<double> &w, bool from_device, bool reset_to_initial) {
  RobustState &rs = *robust;
  int rc = DCORA_OK;
  // a pattern holds every entry of its creation weights; only a weight that was 0 then can reach outside it
  for (size_t e = 0; e < w.size() && !rc; ++e)
    if (rs.meas_zero[e] && w[e] != 0.0) {
      set_last_error(std::string(tag_) + " robust: a weight that was 0 at creation cannot become nonzero (the session's "
                     "patterns do not hold that measurement)");
      rc = DCORA_ERR_BAD_ARG;
    }
  DCORA_HIP(hipSetDevice(opt.device));
  // nothing of the session is in flight while its matrices and preconditioner images change
  const int drained = drain(true);
  if (drained) return drained;
  if (!rc) rc = robust_rebuild(w);
  if (!rc) rs.w.swap(w);
  const size_t m = rs.edge_ids.size();
  if (m && (rc || !from_device)) {
    std::vector<double> held(m);
    for (size_t i = 0; i < m; ++i) held[i] = rs.w[(size_t)rs.edge_ids[i]];
    DCORA_HIP(hipMemcpy(rs.edges.w.p, held.data(), sizeof(double) * m, hipMemcpyHostToDevice));
  }
  if (rc) return rc;
  if (team) team_refresh_counts();
  if (reset_to_initial)
    DCORA_HIP(hipMemcpyAsync(Xg.p, rs.X_initial.p, sizeof(double) * (size_t)r * (size_t)num_cols(),
                             hipMemcpyDeviceToDevice, st));
  return robust_restart_acceleration();
}

int SessionCore::apply_weights(const std::vector<double> &w, bool reset_to_initial) {
  RobustState &rs = *robust;
  std::vector<double> next = rs.w;
  for (size_t i = 0; i < rs.edge_ids.size(); ++i) next[(size_t)rs.edge_ids[i]] = w[i];
  const int rc = adopt_weights(next, true, reset_to_initial);
  if (rc) return rc;
  rs.cost.update();
  rs.updates++;
  // mLatestWeightUpdateIteration, mRobustOptInnerIter = 0, mTeamStatus.clear() (ref src/Agent.cpp:1418-1424)
  team_weights_updated();
  return DCORA_OK;
}

// Agent::setMeasurementWeight (ref src/Agent.cpp:1443-1454) of every measurement
int SessionCore::set_weights(const double *w) {
  const size_t m = robust->w.size();
  for (size_t e = 0; e < m; ++e)
    if (!std::isfinite(w[e]) || w[e] < 0) {
      set_last_error(std::string(tag_) + " robust: weights must be finite and >= 0");
      return DCORA_ERR_BAD_ARG;
    }
  std::vector<double> next(w, w + m);
  return adopt_weights(next, false, false);
}

int SessionCore::get_weights(double *w) const {
  const RobustState &rs = *robust;
  if (rs.ranked)
    for (size_t e = 0; e < rs.w.size(); ++e) w[e] = std::nan("");
  for (int e : rs.edge_ids) w[e] = rs.w[(size_t)e];
  return DCORA_OK;
}

// A rank keeps current weights only of the measurements touching its hosted agents: on a team of a job the counts of all
// R agents come from the exchange's copy of the job's weights, which is in the job's order like q.id.
double SessionCore::team_lc_weight(const TeamLoopClosure &q) const {
  if (q.id < 0) return q.w0;  // not one of the job's measurements (pose-landmark, range): never re-weighted
  return team->job_w ? team->job_w[(size_t)q.id] : robust ? robust->w[(size_t)q.id] : q.w0;
}

}  // namespace dcora
