// Robust pose-graph optimisation around the local solver:
//   measurement_errors : computeMeasurementError of every edge at once (ref src/DCORA_utils.cpp:2095-2101;
//                        Agent::computeMeasurementResidual, ref src/Agent.cpp:1342-1389, with lifted poses), in the SE
//                        ordering of a pose graph or the RA ordering of a range-aided graph's pose-pose measurements
//   solve_pgo          : solvePGO (ref src/DCORA_solver.cpp:304-328) -- chordal start, one optimize() at rank d
//   solve_robust_pgo   : solveRobustPGO (ref :330-409) -- GNC-TLS outer loop around solve_pgo
#include <algorithm>
#include <cmath>
#include <vector>

#include "device_problem.h"
#include "host_graph.h"
#include "host_robust.h"
#include "robust.h"

namespace dcora {

namespace {

struct EdgeDev {
  const int *p1, *p2;
  const double *R, *t, *kappa, *tau;  // R: d*d per edge (column-major), t: d per edge
  int n, l;                           // poses and unit spheres of the problem: read by the RA ordering only
};
struct RankedEdges {
  const int *own, *gidx;  // the rank owns the edge (hosts the agent of p1); its index in the dataset
  double *shared_w;       // device view of the exchange's weights area (m doubles, dataset order)
};
// Where pose p lives in X (r rows, column-major): its rotation's D columns and its translation column.
// SE ordering [Y1 p1 ... Yn pn]: columns (D+1) p .. (D+1) p + D.  RA ordering [Y1..Yn | s1..sl | p1..pn | L1..Lb]:
// rotation at D p, translation at D n + l + p.
struct SeCols {
  template <int D>
  static __device__ __forceinline__ const double *rot(const EdgeDev &, const double *X, int p, int r) {
    return X + (size_t)p * (D + 1) * r;
  }
  template <int D>
  static __device__ __forceinline__ const double *trans(const EdgeDev &, const double *X, int p, int r) {
    return X + (size_t)p * (D + 1) * r + (size_t)D * r;
  }
};
struct RaCols {
  template <int D>
  static __device__ __forceinline__ const double *rot(const EdgeDev &E, const double *X, int p, int r) {
    return X + (size_t)p * D * r;
  }
  template <int D>
  static __device__ __forceinline__ const double *trans(const EdgeDev &E, const double *X, int p, int r) {
    return X + ((size_t)D * E.n + E.l + p) * r;
  }
};
// kappa |Y1 R - Y2|^2 + tau |p2 - p1 - Y1 t|^2 of edge e with Y r x d, p r-vectors, addressed through Cols: one
// expression for every kernel below and both orderings, so the sessions' weight updates see the residuals
// dcora_measurement_errors / dcora_ra_measurement_errors report, bit for bit (Agent::computeMeasurementResidual, ref
// src/Agent.cpp:1349-1395: pose-pose measurements only, on either graph type)
template <int D, class Cols>
__device__ __forceinline__ double edge_error(int r, int e, const EdgeDev &E, const double *__restrict__ X) {
  const double *Y1 = Cols::template rot<D>(E, X, E.p1[e], r), *Y2 = Cols::template rot<D>(E, X, E.p2[e], r);
  const double *T1 = Cols::template trans<D>(E, X, E.p1[e], r), *T2 = Cols::template trans<D>(E, X, E.p2[e], r);
  const double *Re = E.R + (size_t)e * D * D, *te = E.t + (size_t)e * D;
  double rot = 0, tr = 0;
  for (int q = 0; q < r; ++q) {
    double y1[D];
#pragma unroll
    for (int a = 0; a < D; ++a) y1[a] = Y1[(size_t)a * r + q];
#pragma unroll
    for (int c = 0; c < D; ++c) {
      double s = 0;
#pragma unroll
      for (int a = 0; a < D; ++a) s += y1[a] * Re[c * D + a];
      const double dlt = s - Y2[(size_t)c * r + q];
      rot += dlt * dlt;
    }
    double s = T2[q] - T1[q];
#pragma unroll
    for (int a = 0; a < D; ++a) s -= y1[a] * te[a];
    tr += s * s;
  }
  return E.kappa[e] * rot + E.tau[e] * tr;
}

// one thread per edge
template <int D, class Cols>
__global__ __launch_bounds__(kBlock) void k_measurement_errors(int r, int m, EdgeDev E, const double *__restrict__ X,
                                                               double *__restrict__ out) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= m) return;
  out[e] = edge_error<D, Cols>(r, e, E, X);
}

// RobustCost::weight (host_robust.cpp, ref src/DCORA_robust.cpp:56-100) with the same operations in the same order
__device__ double robust_weight(const dcora_robust_params &p, double mu, double r) {
  switch (p.cost_type) {
    case DCORA_ROBUST_L2: return 1;
    case DCORA_ROBUST_L1: return 1 / r;
    case DCORA_ROBUST_HUBER: return r < p.HuberThreshold ? 1 : p.HuberThreshold / r;
    case DCORA_ROBUST_TLS: return r < p.TLSThreshold ? 1 : 0;
    case DCORA_ROBUST_GM: {
      const double a = fma(r, r, 1.0);  // (the host build contracts 1 + r * r into this FMA)
      return 1 / (a * a);
    }
    case DCORA_ROBUST_GNC_TLS: {
      const double rSq = r * r, bSq = p.GNCBarc * p.GNCBarc;
      const double ub = (mu + 1) / mu * bSq, lb = mu / (mu + 1) * bSq;
      if (rSq >= ub) return 0;
      if (rSq <= lb) return 1;
      return sqrt(bSq * mu * (mu + 1) / rSq) - mu;
    }
  }
  return 1;
}

// Agent::updateMeasurementWeights on the session's iterate (ref src/Agent.cpp:1397-1413): one thread per edge, the
// edges flagged upd (loop closures whose weight is not fixed) get RobustCost::weight(sqrt(error)); the rest keep theirs.
// Per-block partials of {accepted (w > 1 - 1e-8), rejected (w < 1e-8), undecided} among the updated edges.
// Ranked (a session of one rank, RobustEdges::upload_ranked / upload_ra_ranked, in either ordering): the edges are those
// touching a hosted agent, X is the rank's mirror; the edges the rank owns also store their weight into the shared
// segment at their dataset index (plain stores, then a system-scope fence), and only they are counted, so that the job
// counts every edge once.
template <int D, bool Ranked, class Cols>
__global__ __launch_bounds__(kBlock) void k_robust_weights(int r, int m, EdgeDev E, const int *__restrict__ upd,
                                                           const double *__restrict__ X, dcora_robust_params p,
                                                           double mu, double *__restrict__ w,
                                                           double *__restrict__ partials, RankedEdges rk) {
  __shared__ double s_red[16];
  const int e = blockIdx.x * kBlock + threadIdx.x;
  double acc = 0, rej = 0, und = 0;
  if (e < m && upd[e]) {
    const double we = robust_weight(p, mu, sqrt(edge_error<D, Cols>(r, e, E, X)));
    w[e] = we;
    const double w_tol = 1e-8;
    if (!Ranked || rk.own[e]) {
      acc = we > 1 - w_tol ? 1 : 0;
      rej = we < w_tol ? 1 : 0;
      und = 1 - acc - rej;
    }
  }
  if (Ranked) {
    if (e < m && rk.own[e]) rk.shared_w[rk.gidx[e]] = w[e];
    __threadfence_system();
  }
  acc = block_sum(acc, s_red);
  rej = block_sum(rej, s_red);
  und = block_sum(und, s_red);
  if (threadIdx.x == 0) {
    partials[(size_t)blockIdx.x * 3] = acc;
    partials[(size_t)blockIdx.x * 3 + 1] = rej;
    partials[(size_t)blockIdx.x * 3 + 2] = und;
  }
}

int no_device() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    set_last_error("no HIP device available: libdcora_hip has no CPU fallback");
    return DCORA_ERR_NO_DEVICE;
  }
  return DCORA_OK;
}

EdgeDev edge_view(const EdgeTable &T, int n = 0, int l = 0) {
  return EdgeDev{T.dp1.p, T.dp2.p, T.dR.p, T.dt.p, T.dk.p, T.dta.p, n, l};
}

template <class T>
int to_device(const std::vector<T> &h, DevBuf<T> *dev) {
  DCORA_HIP(dev->alloc(h.size()));
  DCORA_HIP(hipMemcpy(dev->p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
  return DCORA_OK;
}

}  // namespace

// the measurements of ds packed and uploaded: what EdgeDev points into
int EdgeTable::upload(const HostDataset &ds) {
  const int d = ds.d;
  const size_t m = ds.meas.size();
  std::vector<int> p1(m), p2(m);
  std::vector<double> R(m * d * d), t(m * d), ka(m), ta(m);
  for (size_t e = 0; e < m; ++e) {
    const PoseMeas &q = ds.meas[e];
    p1[e] = q.p1;
    p2[e] = q.p2;
    for (int i = 0; i < d * d; ++i) R[e * d * d + i] = q.R[i];
    for (int i = 0; i < d; ++i) t[e * d + i] = q.t[i];
    ka[e] = q.kappa;
    ta[e] = q.tau;
  }
  int rc = to_device(p1, &dp1);
  if (!rc) rc = to_device(p2, &dp2);
  if (!rc) rc = to_device(R, &dR);
  if (!rc) rc = to_device(t, &dt);
  if (!rc) rc = to_device(ka, &dk);
  if (!rc) rc = to_device(ta, &dta);
  return rc;
}

int RobustEdges::upload(const HostDataset &ds, const std::vector<char> &update) {
  m = (int)ds.meas.size();
  d = ds.d;
  if (m == 0) return DCORA_OK;
  std::vector<int> up(update.begin(), update.begin() + m);
  for (int &u : up) u = u ? 1 : 0;
  std::vector<double> wh((size_t)m);
  for (int e = 0; e < m; ++e) wh[(size_t)e] = ds.meas[(size_t)e].weight;
  int rc = EdgeTable::upload(ds);
  if (!rc) rc = to_device(up, &dupd);
  if (!rc) rc = to_device(wh, &w);
  if (rc) return rc;
  DCORA_HIP(partials.alloc((size_t)((m + kBlock - 1) / kBlock) * 3));
  DCORA_HIP(counts.alloc(3));
  return DCORA_OK;
}

// the pose-pose measurements of a range-aided dataset, read from X in the RA ordering
int RobustEdges::upload_ra(const HostRADataset &ds, const std::vector<char> &update) {
  HostDataset pp;
  pp.d = ds.d;
  pp.n = ds.n;
  pp.meas = ds.pose_pose;
  ra = true;
  n = ds.n;
  l = ds.l;
  return upload(pp, update);
}

// the edges of one rank: ids (dataset order) are those touching a hosted agent, own[i] flags the ones it owns
int RobustEdges::upload_ranked(const HostDataset &ds, const std::vector<char> &update, const std::vector<int> &ids,
                               const std::vector<char> &own) {
  HostDataset sub;
  sub.d = ds.d;
  sub.n = ds.n;
  std::vector<char> up;
  for (int e : ids) {
    sub.meas.push_back(ds.meas[(size_t)e]);
    up.push_back(update[(size_t)e]);
  }
  int rc = upload(sub, up);
  if (rc) return rc;
  ranked = true;
  if (m == 0) return DCORA_OK;
  rc = to_device(std::vector<int>(own.begin(), own.end()), &down);
  return rc ? rc : to_device(ids, &dgidx);
}

// ... of a range-aided job: ids index ds.pose_pose, and the poses are read from the rank's mirror, which has the RA
// ordering of the WHOLE problem (n, l are the job's, not the rank's)
int RobustEdges::upload_ra_ranked(const HostRADataset &ds, const std::vector<char> &update, const std::vector<int> &ids,
                                  const std::vector<char> &own) {
  HostDataset pp;
  pp.d = ds.d;
  pp.n = ds.n;
  pp.meas = ds.pose_pose;
  ra = true;
  n = ds.n;
  l = ds.l;
  return upload_ranked(pp, update, ids, own);
}

namespace {
using WeightsKernel = void (*)(int, int, EdgeDev, const int *, const double *, dcora_robust_params, double, double *,
                               double *, RankedEdges);
// the kernel of one (ordering, ranked) pair in dimension D: every combination is a form of the one template
template <int D>
WeightsKernel weights_kernel(bool ra, bool ranked) {
  static const WeightsKernel forms[2][2] = {
      {k_robust_weights<D, false, SeCols>, k_robust_weights<D, true, SeCols>},
      {k_robust_weights<D, false, RaCols>, k_robust_weights<D, true, RaCols>}};
  return forms[ra ? 1 : 0][ranked ? 1 : 0];
}
}  // namespace

void launch_robust_weights(hipStream_t st, const RobustEdges &T, int r, const double *X, const dcora_robust_params &p,
                           double mu, double *shared_w) {
  if (T.m == 0) return;
  const EdgeDev E = edge_view(T, T.n, T.l);
  const int grid = (T.m + kBlock - 1) / kBlock;
  const RankedEdges rk{T.down.p, T.dgidx.p, shared_w};
  const WeightsKernel kernel = T.d == 3 ? weights_kernel<3>(T.ra, T.ranked) : weights_kernel<2>(T.ra, T.ranked);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, st, r, T.m, E, T.dupd.p, X, p, mu, T.w.p, T.partials.p, rk);
  launch_sum_partials(st, T.partials.p, grid, 3, 3, T.counts.p);
}

namespace {
// the errors of ds.meas at X (r x cols host, poses addressed through Cols; n, l: what RaCols reads)
template <class Cols>
int errors_on_device(const HostDataset &ds, int n, int l, size_t cols, int r, const double *X, double *out, int device) {
  int rc = no_device();
  if (rc) return rc;
  DCORA_HIP(hipSetDevice(device));
  const int d = ds.d, m = (int)ds.meas.size();
  if (m == 0) return DCORA_OK;
  for (const PoseMeas &q : ds.meas)
    if (q.p1 < 0 || q.p1 >= ds.n || q.p2 < 0 || q.p2 >= ds.n) {
      set_last_error("measurement_errors: pose index out of range");
      return DCORA_ERR_BAD_ARG;
    }
  EdgeTable T;
  rc = T.upload(ds);
  if (rc) return rc;
  DevBuf<double> dX, dout;
  const size_t N = (size_t)r * cols;
  DCORA_HIP(dX.alloc(N));
  DCORA_HIP(dout.alloc(m));
  DCORA_HIP(hipMemcpy(dX.p, X, sizeof(double) * N, hipMemcpyHostToDevice));
  const EdgeDev E = edge_view(T, n, l);
  const int grid = (m + kBlock - 1) / kBlock;
  if (d == 3)
    hipLaunchKernelGGL((k_measurement_errors<3, Cols>), dim3(grid), dim3(kBlock), 0, nullptr, r, m, E, dX.p, dout.p);
  else
    hipLaunchKernelGGL((k_measurement_errors<2, Cols>), dim3(grid), dim3(kBlock), 0, nullptr, r, m, E, dX.p, dout.p);
  DCORA_HIP(hipDeviceSynchronize());
  DCORA_HIP(hipMemcpy(out, dout.p, sizeof(double) * m, hipMemcpyDeviceToHost));
  return DCORA_OK;
}
}  // namespace

// X: r x (d+1) n host (SE ordering, r >= d); out: one squared error per measurement (weights not applied)
int measurement_errors(const HostDataset &ds, int r, const double *X, double *out, int device) {
  return errors_on_device<SeCols>(ds, 0, 0, (size_t)(ds.d + 1) * ds.n, r, X, out, device);
}

// the same of a range-aided dataset's pose-pose measurements; X: r x k host in the global RA ordering
int ra_measurement_errors(const HostRADataset &ds, int r, const double *X, double *out, int device) {
  HostDataset pp;
  pp.d = ds.d;
  pp.n = ds.n;
  pp.meas = ds.pose_pose;
  return errors_on_device<RaCols>(pp, ds.n, ds.l, (size_t)ds.k(), r, X, out, device);
}

// T0 (d x (d+1) n) may be null => chordal initialisation; Tout d x (d+1) n
int solve_pgo(const HostDataset &ds, const dcora_ropt_params &prm, const double *T0, double *Tout, int device,
              dcora_ropt_result *res) {
  int rc = no_device();
  if (rc) return rc;
  const int d = ds.d, n = ds.n;
  const size_t N = (size_t)d * (d + 1) * n;
  std::vector<double> T;
  if (T0) {
    T.assign(T0, T0 + N);
  } else if (!chordal_initialization(ds, T)) {
    set_last_error("solve_pgo: chordal initialisation failed (disconnected measurement graph?)");
    return DCORA_ERR_NOT_PD;
  }
  const int id = ds.meas.empty() ? 0 : ds.meas[0].r1;
  const HostCsr Q = build_Q_pgo(d, n, id, ds.meas);
  DeviceProblem P;
  dcora_dims dims{d, d, n, 0, 0};
  rc = P.init(dims, Q, nullptr, 0.1, device, nullptr);
  if (rc) return rc;
  dcora_ropt_result tmp;
  return P.optimize(prm, T.data(), Tout, res ? res : &tmp);
}

// fixed: m flags (fixedWeight of the reference); weights (in/out through ds.meas[i].weight, also copied to weights_out)
int solve_robust_pgo(HostDataset &ds, const dcora_ropt_params &prm, const dcora_robust_params &rp, const int *fixed,
                     const double *T0, double *Tout, double *weights_out, int device) {
  const double w_tol = 1e-8;
  const int m = (int)ds.meas.size(), d = ds.d;
  if (rp.cost_type != DCORA_ROBUST_GNC_TLS) {
    set_last_error("solve_robust_pgo: only GNC_TLS is supported (CHECK of the reference, src/DCORA_solver.cpp:347)");
    return DCORA_ERR_BAD_ARG;
  }
  int rc = solve_pgo(ds, prm, T0, Tout, device, nullptr);
  if (rc) return rc;
  std::vector<double> rsq((size_t)m);
  for (PoseMeas &q : ds.meas) q.weight = 1.0;
  rc = measurement_errors(ds, d, Tout, rsq.data(), device);
  if (rc) return rc;
  const double rmax = m ? *std::max_element(rsq.begin(), rsq.end()) : 0.0;
  const double barcSq = rp.GNCBarc * rp.GNCBarc;
  const double muInit = barcSq / (2 * rmax - barcSq);
  if (muInit > 0) {  // negative: small residuals, GNC skipped
    dcora_robust_params g = rp;
    g.GNCInitMu = muInit;
    RobustCost cost(g);
    for (int iter = 0; iter < g.GNCMaxNumIters; ++iter) {
      rc = solve_pgo(ds, prm, T0, Tout, device, nullptr);
      if (rc) return rc;
      rc = measurement_errors(ds, d, Tout, rsq.data(), device);
      if (rc) return rc;
      int undecided = 0;
      for (int i = 0; i < m; ++i) {
        if (fixed && fixed[i]) continue;
        const double w = cost.weight(std::sqrt(rsq[i]));
        ds.meas[i].weight = w;
        if (!(w < w_tol) && !(w > 1.0 - w_tol)) ++undecided;
      }
      if (undecided == 0) break;
      cost.update();
    }
  }
  rc = solve_pgo(ds, prm, T0, Tout, device, nullptr);
  if (rc) return rc;
  if (weights_out)
    for (int i = 0; i < m; ++i) weights_out[i] = ds.meas[i].weight;
  return DCORA_OK;
}

}  // namespace dcora
