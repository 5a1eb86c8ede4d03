// RBCD++ session for multi-robot range-aided SLAM: the agents of a merged pyfg problem, their device-resident state
// and the synchronous driver loop (replaces Agent::iterate / updateX / getSharedStateDicts / updateNeighborStates on
// the RangeAidedSLAMGraph, ref src/Agent.cpp:535-596, 1158-1278, src/Graph.cpp:824-1772, and the loop body of
// examples/MultiRobotExample_RASLAM.cpp).
//
// Variables are owned as the reference assigns them (poses by robot symbol, landmarks by symbol, unit spheres by the
// source robot of their range); an agent's columns are scattered over the global RA ordering, so each agent keeps its
// X / V / Y / XPrev in its own RA ordering [rotations | unit spheres | translations | landmarks] and the global
// iterate is a mirror that the coupling products (G_a = X_global C_a^T) and the central evaluation read.
//
// Robust sessions (dcora_ra_rbcd_create_robust for one process, dcora_ra_rbcd_create_robust_ranks for one rank of a job,
// whose weight changes are collective: Exchange::update_weights) run the agents' GNC loop in place, as the reference's
// Agent does on a RangeAidedSLAMGraph just as on a pose graph: Agent::initializeRobustOptimization at creation,
// Agent::updateMeasurementWeights / setMeasurementWeight afterwards (ref src/Agent.cpp:1332-1346, 1397-1441, 1443-1454),
// over the graph's pose-pose loop closures only (computeMeasurementResidual, :1349-1395, refuses every other measurement
// type; range and pose-landmark weights never change).  A weight change rebuilds the VALUES of every agent's Q_aa, of
// its coupling block and of the central Q on the patterns recorded at creation, through the path creation takes.  A rank
// of a job has the matrices of its hosted agents only, and those hold the measurements touching them: the weight it keeps
// for any other measurement is the last it was told (creation, set_weights) and reaches no device matrix.  What
// depends on the patterns stays as created: neighbours, public columns and colours (a weight of 0 on the only
// measurement joining two agents would take them apart in a fresh session; the live session keeps its creation adjacency,
// as the reference keeps a weight-0 measurement in its graph), the one-launch tCG eligibility, the hub rows of the
// Q-apply and the sparse / dense choice of the preconditioner.
//
// The team protocol (dcora_ra_rbcd_team_enable in one process, dcora_exchange_team_enable_ra on the ranks of a job) is
// the session core's: the reference's agents run the status block of Agent::iterate, shouldTerminate and
// shouldUpdateMeasurementWeights on either graph type (ref src/Agent.cpp:558-586, 1123-1156, 1280-1330).  What is this
// kind's own: the relative change is taken over the agent's poses in ITS ordering (k_rel_change's RA form), and its loop closures are every measurement but pose-pose odometry --
// pose-pose closures, pose-landmark measurements, ranges (ref src/Graph.cpp:121-134, 475-521).  On a rank of a job the
// relative change goes into the agent's status slot (the ranked RA form) and a pose-pose closure's weight is the job's.
// This kind has no per-agent entry that optimises an agent outside the exchange (RbcdSession::agent_iterate has no
// namesake here; iterate refuses a rank), so nothing else has to refuse on a ranked team.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "device_problem.h"
#include "host_graph.h"
#include "host_robust.h"
#include "robust.h"
#include "session_core.h"

namespace dcora {

struct RaAgentDev : AgentCore {
  int robot = 0;                 // robot id ('A' = 0, ...)
  int n = 0, l = 0, b = 0, k = 0;
  std::vector<int> own_host;     // my columns in the global ordering (host copy: gather of the whole X)
  DevBuf<int> own;               // my columns in the global ordering
  DevBuf<double> X, V, Y, XPrev, tmp;   // r x k, my ordering
  double reg = 0;
};

class RaRbcdSession : public SessionCore {
 public:
  int d = 0, n = 0, l = 0, b = 0, k = 0;
  std::vector<RaAgentDev> agents;
  std::unique_ptr<DeviceProblem> central;  // global Q: cost and Riemannian gradient of the merged problem
  DevBuf<double> evalbuf;

  RaRbcdSession() : SessionCore(SessionKind::RangeAided) {}
  ~RaRbcdSession();
  int init(const HostRADataset &ds, const dcora_rbcd_options &o);
  // robust sessions (RobustState, session_core.h; the job's measurements are the pose-pose ones): weight 1 on every
  // loop closure that is not fixed (fixed: m_pp flags or null), then init.  ranked: a rank of a multi-rank job
  // (world_size >= 1), its weight updates driven by the exchange
  int init_robust(const HostRADataset &ds, const dcora_rbcd_options &o, const dcora_robust_params &p, const int *fixed,
                  bool ranked = false);
  int set_X(const double *Xh) override;  // r x k global; V = Y = XPrev = X for every agent
  int get_X(double *Xh);
  // one pass of the driver's loop body with agent index `selected` (position in the sorted robot list)
  int iterate(int selected, double *cost2, double *gradnorm, double *block_norms, int *next_selected);
  int evaluate(double *cost2, double *gradnorm, double *block_norms, int *next_selected);
  int last_result(dcora_ropt_result *res);
  int set_acceleration(bool on);
  // the loop body in the phases the exchange interleaves with its posts and waits (one process per GPU)
  int phase_nonselected(int selected) override;
  int phase_selected(int selected) override;
  int phase_evaluate_dev(double *out_dev) override;
  AgentCore &agent_core(int a) override { return agents[(size_t)a]; }
  long num_cols() const override { return k; }
  int dim() const override { return d; }
  DeviceProblem *central_problem() override { return central.get(); }
  int cert_block() const override { return 1; }
  ManiDesc global_manifold() const override { return make_mani(r, d, n, l, b, DCORA_LAYOUT_RA); }
  // its own X with the `own` list; its ordering is ra_agent_columns': [rotations | unit spheres | translations |
  // landmarks], or the SE ordering where it owns neither a unit sphere nor a landmark
  AgentBlock agent_block(int a) override;

 private:
  // the one path from a dataset's measurements to the session's matrices, at creation and on every re-weight
  int assemble(const HostRADataset &ds, bool creation);
  // a robust session's part (session_core.h)
  HostRADataset robust_ds_;  // the dataset as created; the pose-pose weights live in robust->w
  int robust_upload_edges() override;
  int robust_rebuild(const std::vector<double> &w) override;
  int robust_restart_acceleration() override;
  // set_X's body for a point on the host or on the device (kind: the copy into the mirror)
  int adopt_X(const double *X, hipMemcpyKind kind);
  // the rank change's hooks: the mirror, X_initial and the agents' X, V, Y, XPrev, tmp re-dimensioned; the central
  // preconditioner's regularisation is device_precond_regularization(central Q), as driver.py passes
  int lift_default_reg(const HostCsr &Qc, double *reg) override;
  int lift_buffers(int r_new) override;
  int lift_adopt(const double *X_dev) override { return adopt_X(X_dev, hipMemcpyDeviceToDevice); }
  int gather_agents();         // every hosted agent's X from the mirror, V = Y = XPrev = X (enqueued)
  int scatter(RaAgentDev &a);  // my X into the global mirror
  int solve(RaAgentDev &a, const double *start, double **result);
  // the tick: a set of one hosted agent has nothing to run beside and stays on the session's stream
  int stage(AgentCore &a) override;
  int write_back(AgentCore &a, hipStream_t run_on) override;
  bool serial_set(const std::vector<AgentCore *> &work) override { return work.size() == 1; }
  int tick_done(const std::vector<AgentCore *> &work) override;
  // the session kind's part of the team protocol: k_rel_change's RA form over the agents' own X / XPrev; the loop
  // closures are ra_team_loop_closures' with agents for robots
  int team_launch_rel_change(const std::vector<int> &ids) override;
  int team_iterate(int selected, double *cost2, double *gradnorm, int *next_selected) override {
    return iterate(selected, cost2, gradnorm, nullptr, next_selected);
  }
};

// lambda_max(Q) / (1e6 - 1) by a Lanczos run on the device (cert.hip, with the other clients of that eigensolver)
int device_precond_regularization(const HostCsr &Q, int device, double *reg);

}  // namespace dcora
