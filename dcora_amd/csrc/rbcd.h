// RBCD++ session: the agents of one process, their device-resident state and the synchronous driver loop
// (replaces Agent::iterate / updateX / getSharedStateDicts / updateNeighborStates, ref src/Agent.cpp:113-152,
// 535-596, 844-906, 1158-1278, and the loop body of examples/MultiRobotExample.cpp:223-307).
#pragma once
#include <chrono>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "device_problem.h"
#include "host_graph.h"
#include "host_robust.h"
#include "robust.h"
#include "session_core.h"
#include "team_rules.h"

namespace dcora {

struct AgentDev : AgentCore {    // prob: Q_bb, (Q_bb + 0.1 I)^-1, solver workspace
  int id = 0, n = 0, col0 = 0;  // poses, first global column
  bool v_feasible = false;  // V is the output of a projection since the agent's last setX
  std::vector<int> public_poses;  // global pose indices of my public poses: public_cols holds (d+1) columns per pose
  // Agent::updateNeighborStates (ref src/Agent.cpp:844-906): once an agent has been HANDED neighbour poses it
  // optimises against what it was handed -- its own cache of them (neighborPoseDict / neighborAuxPoseDict), stale or
  // not -- instead of the session's shared mirror.  required: the global poses of other agents my measurements
  // reach (Graph::requireNeighborPose); nbr[0 / 1]: my copies (plain / auxiliary), laid out like the mirror; got:
  // which required poses each cache holds.  An optimisation whose cache misses a required pose is skipped
  // (constructDataMatrices fails, ref src/Agent.cpp:1243-1249).
  std::vector<int> required;
  bool detached = false;
  DevBuf<double> nbr[2];
  std::vector<char> got[2];
  bool last_skipped = false;
};

class RbcdSession : public SessionCore {
 public:
  int d = 0, n = 0;
  Partition P;
  ManiDesc mg{};  // global manifold (n poses)
  std::vector<AgentDev> agents;
  std::unique_ptr<DeviceProblem> central;  // global Q (evaluation); world_size == 1 only
  DevBuf<double> Vg, Yg, XPrevg;           // r x (d+1) n, laid out like the mirror Xg
  DevBuf<int> col_start;                   // R + 1 global column offsets
  DevBuf<double> evalbuf, posenorm, eval_split;
  DevBuf<int> pose_start;          // R + 1 global pose offsets
  EvalOut *eval_host = nullptr;    // host-mapped results of the evaluation epilogue
  double *x_stage = nullptr;       // pinned staging buffer of get_X
  EvalOut *eval_dev = nullptr;
  int eval_seq = 0;
  dcora_ropt_result last{};
  int last_result(dcora_ropt_result *res);

  RbcdSession() : SessionCore(SessionKind::PoseGraph) { R = 1; }
  ~RbcdSession();
  int init(const HostDataset &ds, const dcora_rbcd_options &o);
  // robust sessions (RobustState, session_core.h): weight 1 on every loop closure that is not fixed (fixed: m flags or
  // null), then init.  ranked: a rank of a multi-rank job (world_size >= 1), its weight updates driven by the exchange
  int init_robust(const HostDataset &ds, const dcora_rbcd_options &o, const dcora_robust_params &p, const int *fixed,
                  bool ranked = false);
  int set_X(const double *Xh) override;
  int get_X(double *Xh);
  int set_acceleration(bool on);
  int phase_nonselected(int selected) override;
  int phase_selected(int selected) override;
  int evaluate(double *cost2, double *gradnorm, double *block_norms, int *next_selected);
  int phase_evaluate_dev(double *out_dev) override;
  int iterate(int selected, double *cost2, double *gradnorm, double *block_norms, int *next_selected);
  // Agent::iterate(doOptimization) of one agent; the agents of a session advance in lockstep (one call per agent
  // and round, as the reference driver makes them)
  int agent_iterate(int agent, bool do_optimization);
  int agent_get_X(int agent, double *Xh);
  int agent_set_X(int agent, const double *Xh);
  // count poses of `neighbor` (frames local to it, each r x (d+1) column-major in `poses`) handed to `agent`
  int agent_update_neighbor(int agent, int neighbor, int count, const int *frames, const double *poses, bool aux);
  std::vector<int> agent_it;  // Agent::iteration_number() of every agent
  int agent_iteration_number(int agent) const;
  int pack_public(int agent, double *packed_dev);
  int unpack_public(int agent, const double *packed_dev);

  AgentCore &agent_core(int a) override { return agents[(size_t)a]; }
  long num_cols() const override { return (long)(d + 1) * n; }
  int dim() const override { return d; }
  DeviceProblem *central_problem() override { return central.get(); }
  int cert_block() const override { return d + 1; }
  ManiDesc global_manifold() const override { return mg; }
  AgentBlock agent_block(int a) override;  // (its contiguous range of the mirror, SE ordering)

 private:
  bool chain_rides_ = false;  // env::chain_rides() when the session was created
  bool seq_advanced_ = false;  // phase_nonselected has advanced the sequences of the round phase_selected finishes
  int staged_selected_ = -1;  // agent whose Nesterov step rode in the non-selected agents' launch of this round
  int staged_iteration_ = -1; // the round it was staged in: honoured by update_selected_agent in that round only
  bool pending_reset_ = false;  // gamma = alpha = 0 after a restart round, applied when the next round begins
  std::vector<char> set_marks_;  // agents that received Agent::setX since the last round
  // set_X's body for a point on the host or on the device (kind: the copy into the mirror)
  int adopt_X(const double *X, hipMemcpyKind kind);
  // the rank change's hooks: Xg, Vg, Yg, XPrevg, X_initial and the staging buffer of get_X re-dimensioned, the agents'
  // handed neighbour caches dropped; the central preconditioner's regularisation is the agents' (driver.py passes 0.1)
  int lift_default_reg(const HostCsr &Qc, double *reg) override;
  int lift_buffers(int r_new) override;
  int lift_adopt(const double *X_dev) override { return adopt_X(X_dev, hipMemcpyDeviceToDevice); }
  int update_nonselected_agent(AgentDev &a, bool restart);
  int update_selected_agent(AgentDev &a, bool restart);
  int restart_step(AgentDev &a);
  // the tick
  void tick_begins() override;
  int stage(AgentCore &a) override;
  int write_back(AgentCore &a, hipStream_t run_on) override;
  bool serial_set(const std::vector<AgentCore *> &work) override;
  int tick_done(const std::vector<AgentCore *> &work) override;
  // the session kind's part of the team protocol (session_core.h)
  int team_launch_rel_change(const std::vector<int> &ids) override;
  bool team_last_success(int agent) const override { return !agents[(size_t)agent].last_skipped; }
  int team_iteration_number(int agent) const override { return agent_iteration_number(agent); }
  int team_iterate(int selected, double *cost2, double *gradnorm, int *next_selected) override {
    return iterate(selected, cost2, gradnorm, nullptr, next_selected);
  }
  // session assembly (rbcd.hip): the host matrices of the hosted agents -- Q[i] = Q_bb, C[i] = coupling block of agent
  // ids[i] -- as the host builders give them
  struct MeasSplit;
  struct Assembly {
    std::vector<int> ids;
    std::vector<HostCsr> Q, C;
  };
  int assemble(const MeasSplit &split, const std::function<void(size_t, const Assembly &)> &each,
               const std::function<int(const Assembly &)> &agents_ready,
               const std::function<int(const HostCsr &)> &central_ready);
  int attach_preconditioners(const std::vector<HostCsr> &Q, const std::function<int(size_t)> &attach);
  std::chrono::steady_clock::time_point t0_;  // init began
  void lap(const char *what) const;
  // a robust session's part (session_core.h)
  HostDataset robust_ds_;  // the dataset (global pose indices) as created; the weights live in robust->w
  int robust_upload_edges() override;
  int robust_rebuild(const std::vector<double> &w) override;
  int robust_restart_acceleration() override;
};

}  // namespace dcora
