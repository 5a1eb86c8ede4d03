// RBCD++ session for multi-robot range-aided SLAM: the agents of a merged pyfg problem, their device-resident state
// and the synchronous driver loop (replaces Agent::iterate / updateX / getSharedStateDicts / updateNeighborStates on
// the RangeAidedSLAMGraph, ref src/Agent.cpp:535-596, 1158-1278, src/Graph.cpp:824-1772, and the loop body of
// examples/MultiRobotExample_RASLAM.cpp).
//
// Variables are owned as the reference assigns them (poses by robot symbol, landmarks by symbol, unit spheres by the
// source robot of their range); an agent's columns are scattered over the global RA ordering, so each agent keeps its
// X / V / Y / XPrev in its own RA ordering [rotations | unit spheres | translations | landmarks] and the global
// iterate is a mirror that the coupling products (G_a = X_global C_a^T) and the central evaluation read.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "device_problem.h"
#include "host_graph.h"
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

  RaRbcdSession() : SessionCore("ra_rbcd") {}
  ~RaRbcdSession();
  int init(const HostRADataset &ds, const dcora_rbcd_options &o);
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
  DeviceProblem *central_problem() override { return central.get(); }
  int cert_block() const override { return 1; }
  int x_stage_hosted(double *host_area) override;

 private:
  int scatter(RaAgentDev &a);  // my X into the global mirror
  int solve(RaAgentDev &a, const double *start, double **result);
  // the tick: a set of one hosted agent has nothing to run beside and stays on the session's stream
  int stage(AgentCore &a) override;
  int write_back(AgentCore &a, hipStream_t run_on) override;
  bool serial_set(const std::vector<AgentCore *> &work) override { return work.size() == 1; }
};

int device_precond_regularization(const HostCsr &Q, int device, double *reg);

}  // namespace dcora
