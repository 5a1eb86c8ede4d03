// Robust pose-graph optimisation drivers (robust.hip)
#pragma once
#include "../../include/dcora_hip.h"
#include "device_problem.h"
#include "host_graph.h"

namespace dcora {
// the measurements of a dataset on the device: p1, p2, R (d*d per edge, column-major), t (d per edge), kappa, tau
struct EdgeTable {
  DevBuf<int> dp1, dp2;
  DevBuf<double> dR, dt, dk, dta;
  int upload(const HostDataset &ds);
};
// the measurement table of a robust RBCD session (rbcd.h), uploaded once at creation, and the weights in dataset order
struct RobustEdges : EdgeTable {
  int m = 0, d = 0;
  bool ranked = false;         // the edges of one rank of a multi-rank session (upload_ranked)
  bool ra = false;             // X is in the RA ordering of a problem with n poses and l unit spheres (upload_ra*)
  int n = 0, l = 0;
  DevBuf<int> dupd;  // dupd: the weight is rewritten by the update (a loop closure whose weight is not fixed)
  DevBuf<int> down, dgidx;     // ranked: the rank owns the edge (hosts the agent of p1); the edge's dataset index
  DevBuf<double> w, partials, counts;
  int upload(const HostDataset &ds, const std::vector<char> &update);
  // the pose-pose measurements of a range-aided dataset (HostRADataset::pose_pose, in that order)
  int upload_ra(const HostRADataset &ds, const std::vector<char> &update);
  // the edges ids (dataset order) of ds only; own: one flag per id
  int upload_ranked(const HostDataset &ds, const std::vector<char> &update, const std::vector<int> &ids,
                    const std::vector<char> &own);
  // ... of ds.pose_pose, read from a mirror in the RA ordering of the whole problem (a rank of a range-aided job)
  int upload_ra_ranked(const HostRADataset &ds, const std::vector<char> &update, const std::vector<int> &ids,
                       const std::vector<char> &own);
};
// w[e] = RobustCost::weight(sqrt(error_e(X))) with RobustCost's mu for the edges flagged dupd; counts[3] = accepted,
// rejected, undecided among them (per-block partials summed by one more launch: deterministic, no atomics).
// Ranked edges: counts over the owned edges only, and the owned edges' weights also go to shared_w[dataset index]
void launch_robust_weights(hipStream_t st, const RobustEdges &T, int r, const double *X, const dcora_robust_params &p,
                           double mu, double *shared_w = nullptr);
int measurement_errors(const HostDataset &ds, int r, const double *X, double *out, int device);
// ... of the pose-pose measurements of a range-aided dataset, X r x k in the global RA ordering (the other measurement
// types have no residual here: Agent::computeMeasurementResidual refuses them, ref src/Agent.cpp:1349-1395)
int ra_measurement_errors(const HostRADataset &ds, int r, const double *X, double *out, int device);
int solve_pgo(const HostDataset &ds, const dcora_ropt_params &prm, const double *T0, double *Tout, int device,
              dcora_ropt_result *res);
int solve_robust_pgo(HostDataset &ds, const dcora_ropt_params &prm, const dcora_robust_params &rp, const int *fixed,
                     const double *T0, double *Tout, double *weights_out, int device);
}  // namespace dcora
