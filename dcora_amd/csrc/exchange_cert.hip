// Certification across the ranks of an exchange (SURVEY 8(e) "Collective": row-block S v with the halo exchange of the
// RBCD loop, scalar all-reduces for the Lanczos recurrences; ref src/DCORA_utils.cpp:1713-1735, 1809-1896).
// Two entries share the flow: certify takes the global Q from the caller on rank 0 and the gathered X; certify_live
// forms M = (Q - Lambda) + eta I from the matrices the ranks hold on the device (cert_rows.h, k_cert_rows) and moves
// only those values to rank 0 (ref src/DCORA_utils.cpp:1713-1735, 1898-1982; examples/MultiRobotExample.cpp:321-335).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>

#include "cert.h"
#include "device_chol.h"
#include "exchange.h"

namespace dcora {

namespace {

// w += eta v - Lambda v on the variables of one agent, r = 1 vectors in the agent's ordering: Lambda is block diagonal
// -- a d x d block (column-major) on the d rotation columns of every pose, a scalar on every unit sphere, nothing on
// translations and landmarks (ref constructDualCertificateMatrixPGO / ...RASLAM, src/DCORA_utils.cpp:1898-1982); L as
// k_lambda leaves it: n blocks, then l scalars.  Pose layout: d + 1 entries per pose; range-aided layout: rotations,
// unit spheres, translations, landmarks.
__global__ __launch_bounds__(256) void k_apply_lambda(ManiDesc m, const double *__restrict__ L, double eta,
                                                      const double *__restrict__ v, double *__restrict__ w) {
  const int d = m.d;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < (long)m.k; e += (long)gridDim.x * 256) {
    double acc = eta * v[e];
    if (m.se) {
      const int dh = d + 1, i = (int)(e / dh), c = (int)(e - (long)i * dh);
      if (c < d) {
        const double *__restrict__ Li = L + (size_t)i * d * d;
        for (int b = 0; b < d; ++b) acc -= Li[c + b * d] * v[(size_t)i * dh + b];
      }
    } else if (e < (long)d * m.n) {
      const int i = (int)(e / d), c = (int)(e - (long)i * d);
      const double *__restrict__ Li = L + (size_t)i * d * d;
      for (int b = 0; b < d; ++b) acc -= Li[c + b * d] * v[(size_t)i * d + b];
    } else if (e < (long)d * m.n + m.l) {
      acc -= L[(size_t)m.n * d * d + (e - (long)d * m.n)] * v[e];
    }
    w[e] += acc;
  }
}

// whole[map[i]] = local[i]
__global__ __launch_bounds__(256) void k_scatter_rows(int n, const int *__restrict__ map, const double *__restrict__ local,
                                                      double *__restrict__ whole) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) whole[map[i]] = local[i];
}

// one hosted agent of either session kind, as the row-block operator sees it
struct CertBlock {
  int k = 0;                     // its unknowns
  int loc0 = 0;                  // where they start in this rank's local vectors
  int col0 = 0;                  // pose-graph session: its first column of the global ordering (contiguous)
  const int *own_dev = nullptr;  // range-aided session: the global column of each of its columns
  DeviceProblem *prob = nullptr;
  CsrDev coupling;
  const double *X = nullptr;     // r x k, its ordering
  DevBuf<double> L, tmp;
};

// The values of one agent's rows of M = (Q - Lambda) + eta I that fall into the window [lo, lo + window size) of the
// job-wide value array, one thread per stored entry, gather form like k_cert_values: entry t reads the Q_aa or the
// coupling value its source index names (or nothing), its Lambda value (or none), adds eta on a diagonal -- the host
// assembly's order -- and stores to its own place.  No atomics, no scatter among threads: the same bits on every call.
// The host launches it on the table entries whose positions lie in the window (cert_row_window), so pos[t] - lo is
// inside the window; every index was checked against its array when the table was built (check_cert_row_table).
__global__ __launch_bounds__(kBlock) void k_cert_rows(int count, const int *__restrict__ pos, const int *__restrict__ src,
                                                      const int *__restrict__ slot,
                                                      const unsigned char *__restrict__ diag,
                                                      const double *__restrict__ Qv, const double *__restrict__ Cv,
                                                      const double *__restrict__ L, double eta, int lo,
                                                      double *__restrict__ window) {
  const long t = (long)blockIdx.x * kBlock + threadIdx.x;
  if (t >= count) return;
  const int s = src[t], q = slot[t];
  double v = s >= 0 ? Qv[s] : (s <= -2 ? Cv[-2 - s] : 0.0);
  if (q >= 0) v -= L[q];
  if (diag[t]) v += eta;
  window[pos[t] - lo] = v;
}

// `count` doubles from the device (stream st) through pinned staging where there is some
int fetch_values(hipStream_t st, const double *dev, size_t count, double *host) {
  const size_t bytes = count * sizeof(double);
  char *pin = bytes ? pinned_acquire(bytes) : nullptr;
  const hipError_t e1 = hipMemcpyAsync(pin ? (void *)pin : (void *)host, dev, bytes, hipMemcpyDeviceToHost, st);
  const hipError_t e2 = hipStreamSynchronize(st);
  if (pin && e1 == hipSuccess && e2 == hipSuccess) std::memcpy(host, pin, bytes);
  if (pin) pinned_release(pin, bytes);
  DCORA_HIP(e1);
  DCORA_HIP(e2);
  return DCORA_OK;
}

int bad_table(const char *what) {
  set_last_error(std::string("certificate row table: ") + what);
  return DCORA_ERR_BAD_ARG;
}

}  // namespace

int build_cert_row_table(const HostCsr &P, const std::vector<int> &own, const HostCsr &Qaa, const HostCsr &C,
                         const ManiDesc &m, CertRowTable *out) {
  const int ka = (int)own.size();
  if (ka != m.k || Qaa.n != ka || C.n != ka || (int)Qaa.rp.size() != ka + 1 || (int)C.rp.size() != ka + 1 ||
      (int)P.rp.size() != P.n + 1)
    return bad_table("the agent's matrices do not have one row per column of its map");
  std::vector<int> local((size_t)P.n, -1);
  for (int i = 0; i < ka; ++i) {
    if (own[(size_t)i] < 0 || own[(size_t)i] >= P.n || local[(size_t)own[(size_t)i]] >= 0)
      return bad_table("the agent's column map leaves the job's columns or names one twice");
    local[(size_t)own[(size_t)i]] = i;
  }
  for (int c : Qaa.ci)
    if (c < 0 || c >= ka) return bad_table("a column of the agent's matrix outside the agent");
  for (int c : C.ci)
    if (c < 0 || c >= P.n) return bad_table("a column of the coupling block outside the job");
  // the Lambda values of every row of the agent: (local column, index of the value)
  std::vector<int> LI, LJ;
  lambda_entries(m, LI, LJ);
  std::vector<std::vector<std::pair<int, int>>> lam((size_t)ka);
  for (size_t q = 0; q < LI.size(); ++q) lam[(size_t)LI[q]].push_back({LJ[q], (int)q});
  struct Entry {
    int pos, src, slot;
    unsigned char diag;
  };
  std::vector<Entry> entries;
  std::vector<std::pair<int, int>> from;  // one row: (global column, source code), sorted
  for (int i = 0; i < ka; ++i) {
    const int g = own[(size_t)i];
    from.clear();
    for (int p = Qaa.rp[i]; p < Qaa.rp[i + 1]; ++p) from.push_back({own[(size_t)Qaa.ci[p]], p});
    for (int p = C.rp[i]; p < C.rp[i + 1]; ++p) from.push_back({C.ci[p], -2 - p});
    std::sort(from.begin(), from.end());
    for (size_t u = 1; u < from.size(); ++u)
      if (from[u].first == from[u - 1].first) return bad_table("an entry stored twice in an agent's row");
    size_t found = 0, found_lambda = 0;
    bool has_diag = false;
    for (int p = P.rp[g]; p < P.rp[g + 1]; ++p) {
      const int j = P.ci[p];
      Entry e{p, -1, -1, (unsigned char)(j == g)};
      const auto it = std::lower_bound(from.begin(), from.end(), std::make_pair(j, INT_MIN));
      if (it != from.end() && it->first == j) {
        e.src = it->second;
        ++found;
      }
      const int jl = j >= 0 && j < P.n ? local[(size_t)j] : -1;
      if (jl >= 0)
        for (const auto &lq : lam[(size_t)i])
          if (lq.first == jl) {
            e.slot = lq.second;
            ++found_lambda;
          }
      has_diag = has_diag || j == g;
      entries.push_back(e);
    }
    if (found != from.size() || found_lambda != lam[(size_t)i].size() || !has_diag)
      return bad_table("an entry of an agent's row, of Lambda or of the diagonal lies outside the job's pattern");
  }
  std::sort(entries.begin(), entries.end(), [](const Entry &a, const Entry &b) { return a.pos < b.pos; });
  *out = CertRowTable();
  for (const Entry &e : entries) {
    out->pos.push_back(e.pos);
    out->src.push_back(e.src);
    out->slot.push_back(e.slot);
    out->diag.push_back(e.diag);
  }
  return DCORA_OK;
}

int check_cert_row_table(const CertRowTable &t, long nnz_p, long nnz_q, long nnz_c, long n_lambda) {
  const size_t n = t.pos.size();
  if (t.src.size() != n || t.slot.size() != n || t.diag.size() != n) return bad_table("arrays of unequal length");
  for (size_t e = 0; e < n; ++e) {
    if (t.pos[e] < 0 || t.pos[e] >= nnz_p || (e > 0 && t.pos[e] <= t.pos[e - 1]))
      return bad_table("a position outside the value array, or positions not ascending");
    const long s = t.src[e];
    if (s >= nnz_q || (s <= -2 && -2 - s >= nnz_c)) return bad_table("a source index outside the matrix it names");
    if (t.slot[e] < -1 || t.slot[e] >= n_lambda) return bad_table("a Lambda index outside the Lambda values");
  }
  return DCORA_OK;
}

void cert_row_window(const std::vector<int> &pos, long lo, long hi, size_t *first, size_t *last) {
  *first = (size_t)(std::lower_bound(pos.begin(), pos.end(), lo) - pos.begin());
  *last = (size_t)(std::lower_bound(pos.begin(), pos.end(), hi) - pos.begin());
}

void cert_rows_host(const CertRowTable &t, size_t first, size_t last, const double *Qv, const double *Cv,
                    const double *L, double eta, long lo, double *window, unsigned char *written) {
  for (size_t e = first; e < last; ++e) {
    const int s = t.src[e], q = t.slot[e];
    double v = s >= 0 ? Qv[s] : (s <= -2 ? Cv[-2 - s] : 0.0);
    if (q >= 0) v -= L[q];
    if (t.diag[e]) v += eta;
    window[t.pos[e] - lo] = v;
    if (written) ++written[t.pos[e] - lo];
  }
}

int Exchange::allreduce_sum(double *vals, int count) {
  if (count < 0 || count > 31) return usage("allreduce_sum: at most 31 values", DCORA_ERR_BAD_ARG);
  if (world == 1) return DCORA_OK;
  const ExchangeSlots sl = slots();
  int whom = 0;
  const int rc = sl.allreduce_sum(sl.wait(), ++red_seq_, vals, count, &whom);
  return rc ? wait_failed(rc, "rank " + std::to_string(whom) + " never joined a sum") : DCORA_OK;
}

// the hosted agents as the row-block operator sees them, with their Lambda blocks at the current iterate
struct Exchange::CertRows {
  std::vector<CertBlock> blocks;
  int nloc = 0, lo = 0;      // this rank's rows; pose-graph session: the first of them in the global ordering
  std::vector<int> row_map;  // global index of every local row (range-aided sessions)
  std::vector<int> all;      // every agent of the job
};

// The pose-graph and the range-aided session through one flow: what differs is where an agent's variables sit in the
// global ordering (a contiguous range / scattered: the session's AgentBlock) and the layout its Lambda blocks act on.  Post and wait of
// all agents -- every rank's mirror holds its neighbours' current public poses --, then the Lambda blocks of the hosted
// agents: EG_b = X_b Q_bb + X C_b, Lambda = SymBlockDiag(X_b^T EG_b).
int Exchange::cert_rows_begin(CertRows *rows) {
  hipStream_t st = s_->st;
  const int R = s_->R, r = s_->r;
  double *mirror = s_->Xg.p;
  std::vector<int> &all = rows->all;
  all.resize((size_t)R);
  for (int a = 0; a < R; ++a) all[(size_t)a] = a;
  int rc = post(all.data(), R);
  if (rc) return rc;
  rc = wait(all.data(), R);
  if (rc) return rc;
  std::vector<CertBlock> &blocks = rows->blocks;
  int nloc = 0, lo = -1;
  for (int a = 0; a < R; ++a) {
    AgentCore &core = s_->agent_core(a);
    if (!core.hosted) continue;
    const AgentBlock blk = s_->agent_block(a);
    CertBlock B;
    B.k = blk.k;
    B.loc0 = nloc;
    B.col0 = (int)blk.col0;
    B.own_dev = blk.cols_dev;
    B.prob = core.prob.get();
    B.coupling = core.coupling.view();
    B.X = blk.X;
    if (!blk.contiguous())
      rows->row_map.insert(rows->row_map.end(), blk.cols_host, blk.cols_host + blk.k);
    else if (lo < 0)
      lo = (int)blk.col0;
    nloc += B.k;
    blocks.push_back(std::move(B));
  }
  rows->nloc = nloc;
  rows->lo = lo < 0 ? 0 : lo;
  for (CertBlock &B : blocks) {
    DeviceProblem &pb = *B.prob;
    launch_spmm(st, r, B.coupling, buf1(mirror), 0, nullptr, buf1(pb.G.p), 0, nullptr, Gate{});
    pb.has_G = true;
    pb.enqueue_egrad(B.X, pb.EG1.p, nullptr);
    DCORA_HIP(B.L.alloc((size_t)pb.m.n * pb.m.d * pb.m.d + (size_t)std::max(pb.m.l, 1)));
    DCORA_HIP(B.tmp.alloc((size_t)B.k));
    launch_lambda_blocks(st, pb.m, B.X, pb.EG1.p, B.L.p);
  }
  DCORA_HIP(hipGetLastError());
  return DCORA_OK;
}

int Exchange::certify(const HostCsr *Qglobal, double eta, int *certified, double *theta, double *lambda_min, double *v,
                      long long *matvecs, int *distributed) {
  const int device = s_->opt.device;
  DCORA_HIP(hipSetDevice(device));
  const int r = s_->r, ktot = (int)s_->num_cols();
  const ManiDesc mg = s_->global_manifold();
  const dcora_dims dims{r, mg.d, mg.n, mg.l, mg.b, mg.se ? DCORA_LAYOUT_AUTO : DCORA_LAYOUT_RA};
  const int chol_block = s_->cert_block();
  if (certified) *certified = 0;
  if (theta) *theta = 0;
  if (lambda_min) *lambda_min = 0;
  if (matvecs) *matvecs = 0;
  if (distributed) *distributed = 0;
  CertRows rows;
  int rc = cert_rows_begin(&rows);
  if (rc) return rc;
  // ---- the PSD test, on rank 0: S = Q - Lambda(X) from the gathered X ----
  std::vector<double> Xh((size_t)r * ktot);
  rc = gather_X(Xh.data());
  if (rc) return rc;
  HostCsr M;
  double verdict[2] = {0, 0};  // {1 = PSD, 2 = not PSD; error code}
  if (rank == 0) {
    if (!Qglobal) {
      verdict[1] = DCORA_ERR_BAD_ARG;
    } else {
      HostCsr Sh;
      int c = device_dual_certificate(dims, Xh.data(), *Qglobal, device, &Sh);
      bool psd = false;
      if (!c) {
        M = csr_shift_diag(Sh, eta);
        c = device_chol_is_pd(M, chol_block, device, &psd);
      }
      verdict[0] = c ? 0 : (psd ? 1 : 2);
      verdict[1] = c;
    }
  }
  rc = allreduce_sum(verdict, 2);  // the other ranks add zeros: a broadcast
  if (rc) return rc;
  // (every rank learns the code from the sum above and leaves the call together: a missing Q on rank 0 is a usage error
  // of the caller, not a failure of the job)
  if ((int)verdict[1] == DCORA_ERR_BAD_ARG) return usage("certify: rank 0 needs the global Q", DCORA_ERR_BAD_ARG);
  if (verdict[1] != 0) return fail("certify: the PSD test failed on rank 0", (int)verdict[1]);
  if (verdict[0] == 1) {
    if (certified) *certified = 1;
    return DCORA_OK;
  }
  return cert_min_eigenpair(rows, M, eta, false, theta, lambda_min, v, matvecs, distributed);
}

// One vector of the whole problem from the ranks to every rank, through the segment's X area: `store` writes this
// rank's part there (all of it on rank 0, or every rank its own rows), barrier, every rank copies it out, barrier.
int Exchange::share_whole_vector(const std::function<void(double *x_area)> &store, double *whole) {
  store(lay_.x(map_));
  int rc = barrier();
  if (rc) return rc;
  std::memcpy(whole, lay_.x(map_), sizeof(double) * s_->num_cols());
  return barrier();
}

// ---- minimum eigenpair of M = S + eta I by all ranks (M: on rank 0, for the second run's start vector and the
// shift-and-invert fallback; the operator is the ranks' own matrices and Lambda blocks) ----
int Exchange::cert_min_eigenpair(CertRows &rows, const HostCsr &M, double eta, bool skip_hopeless, double *theta,
                                 double *lambda_min, double *v, long long *matvecs, int *distributed) {
  const int device = s_->opt.device;
  hipStream_t st = s_->st;
  const int R = s_->R, ktot = (int)s_->num_cols();
  std::vector<CertBlock> &blocks = rows.blocks;
  const std::vector<int> &row_map = rows.row_map, &all = rows.all;
  const int nloc = rows.nloc, lo = rows.lo;
  int rc = DCORA_OK;
  DevBuf<double> vg;  // the Lanczos vector of the whole problem: own entries + the neighbours' public ones are current
  DCORA_HIP(vg.alloc((size_t)ktot));
  DCORA_HIP(hipMemsetAsync(vg.p, 0, sizeof(double) * ktot, st));
  DeviceLanczos L;
  rc = L.init_rows(nloc, ktot, lo, device, st);
  if (rc) return rc;
  L.ranks.row_map = row_map;
  L.ranks.allreduce = [this](double *vals, int count) { return allreduce_sum(vals, count); };
  L.op = [&](const double *vj, double *w) -> int {
    for (CertBlock &B : blocks) {
      if (B.own_dev)
        hipLaunchKernelGGL(k_scatter_rows, dim3(std::min((B.k + 255) / 256, 1024)), dim3(256), 0, st, B.k, B.own_dev,
                           vj + B.loc0, vg.p);
      else
        DCORA_HIP(hipMemcpyAsync(vg.p + B.col0, vj + B.loc0, sizeof(double) * B.k, hipMemcpyDeviceToDevice, st));
    }
    int c = post_arr(all.data(), R, 1, vg.p);
    if (c) return c;
    c = wait_arr(all.data(), R, 1, vg.p);
    if (c) return c;
    for (CertBlock &B : blocks) {
      DeviceProblem &pb = *B.prob;
      double *wa = w + B.loc0;
      launch_spmm(st, 1, B.coupling, buf1(vg.p), 0, nullptr, buf1(B.tmp.p), 0, nullptr, Gate{});
      launch_spmm(st, 1, pb.Q.view(), buf1(vj + B.loc0), 0, B.tmp.p, buf1(wa), 0, nullptr, Gate{});
      hipLaunchKernelGGL(k_apply_lambda, dim3(std::min((B.k + 255) / 256, 1024)), dim3(256), 0, st, pb.m, B.L.p, eta,
                         vj + B.loc0, wa);
    }
    DCORA_HIP(hipGetLastError());
    return DCORA_OK;
  };
  // The plan of min_eig_plan.h with collective runs.  Every quantity its decisions read was summed in rank order, so
  // every rank decides alike.  The shortcut is certify_live's choice (as on one GPU, a spectrum as wide as tiers.pyfg's
  // 2e6 gives the spectrum-shifted run no chance worth up to 1000 restarts of collective steps); certify keeps making
  // the run.  The fallback needs a factorisation of the whole matrix and is rank 0's, which holds it.
  using After = MinEigPlan::AfterFirst;
  const MinEigPlan plan{MinEigPlan::Shortcut::when_asked, MinEigPlan::OnFailedFirst::fallback};
  const uint64_t seed = 12345;
  const int ncv = std::min(20, ktot);
  auto lanczos = [&](const MinEigPlan::Run &run, const double *x0, LanczosResult *res) {
    return L.largest_magnitude(run.shift, run.ncv, run.maxit, run.tol, x0, seed, res);
  };
  LanczosResult res;
  rc = lanczos(plan.first_run(ncv, 1000), nullptr, &res);
  if (rc) return rc;
  long mv = res.matvecs;
  const After after = plan.after_first_run(res.ok, res.lambda, eta, skip_hopeless);
  bool fallback = plan.goes_to_fallback(after);
  if (after == After::shifted) {
    // its start vector comes from the first row of M, which rank 0 holds
    const double lambda_lm = res.lambda;
    std::vector<double> x0((size_t)ktot, 0.0);
    if (rank == 0) x0 = min_eig_second_start(M, seed);
    rc = share_whole_vector([&](double *x) { std::memcpy(x, x0.data(), rank == 0 ? sizeof(double) * ktot : 0); }, x0.data());
    if (rc) return rc;
    rc = lanczos(plan.shifted_run(lambda_lm, eta, ncv, 1000), x0.data(), &res);
    if (rc) return rc;
    mv += res.matvecs;
    fallback = !res.ok;
    res.lambda = plan.shifted_eigenvalue(res.lambda, lambda_lm);
  }
  double flag = fallback ? 1 : 0;  // (identical on all ranks)
  rc = allreduce_sum(&flag, 1);
  if (rc) return rc;
  std::vector<double> vfull((size_t)ktot, 0.0);
  if (flag != 0) {
    // the shortcut, or a collective run that did not converge (ref :1878-1888)
    double out2[3] = {0, 0, 0};  // {lambda; error code; rank 0's matvecs: the count is the same on every rank}
    if (rank == 0) {
      LanczosResult e;
      const int c = device_min_eig(M, 1000, eta, 20, seed, device, &e);
      if (c && c != DCORA_ERR_NO_CONVERGENCE) out2[1] = c;
      out2[0] = e.lambda;
      out2[2] = (double)e.matvecs;
      if (e.v.size() == (size_t)ktot) vfull = e.v;
    }
    rc = allreduce_sum(out2, 3);
    if (rc) return rc;
    if (out2[1] != 0) return fail("certify: the minimum eigenpair could not be computed", (int)out2[1]);
    res.lambda = out2[0];
    mv += (long)out2[2];
    rc = share_whole_vector([&](double *x) { std::memcpy(x, vfull.data(), rank == 0 ? sizeof(double) * ktot : 0); },
                            vfull.data());
    if (rc) return rc;
  } else {
    if (distributed) *distributed = 1;
    // every rank its own rows of the shared vector
    rc = share_whole_vector(
        [&](double *x) {
          for (int i = 0; i < nloc; ++i) x[row_map.empty() ? (size_t)lo + i : (size_t)row_map[(size_t)i]] = res.v[(size_t)i];
        },
        vfull.data());
    if (rc) return rc;
  }
  // theta = v^T S v = v^T M v - eta (|v| = 1), with the row-block operator
  {
    DevBuf<double> vl, wl;
    DCORA_HIP(vl.alloc((size_t)std::max(nloc, 1)));
    DCORA_HIP(wl.alloc((size_t)std::max(nloc, 1)));
    std::vector<double> vloc((size_t)std::max(nloc, 1));
    L.ranks.slice(vfull.data(), nloc, vloc.data());
    if (nloc > 0) DCORA_HIP(hipMemcpyAsync(vl.p, vloc.data(), sizeof(double) * nloc, hipMemcpyHostToDevice, st));
    rc = L.op(vl.p, wl.p);
    if (rc) return rc;
    std::vector<double> wh((size_t)std::max(nloc, 1));
    if (nloc > 0) DCORA_HIP(hipMemcpyAsync(wh.data(), wl.p, sizeof(double) * nloc, hipMemcpyDeviceToHost, st));
    DCORA_HIP(hipStreamSynchronize(st));
    double dots[2] = {0, 0};
    for (int i = 0; i < nloc; ++i) {
      dots[0] += vloc[(size_t)i] * wh[(size_t)i];
      dots[1] += vloc[(size_t)i] * vloc[(size_t)i];
    }
    rc = allreduce_sum(dots, 2);
    if (rc) return rc;
    if (theta) *theta = dots[0] / dots[1] - eta;
  }
  if (lambda_min) *lambda_min = res.lambda;
  if (matvecs) *matvecs = mv;
  if (v) std::memcpy(v, vfull.data(), sizeof(double) * ktot);
  return DCORA_OK;
}

// The job-wide pattern and the hosted agents' tables, once per job.  The pattern is dcora_cert_dual_matrix's for the
// job's creation-time Q: kept from the assembly at creation on a rank of a job (SessionCore::job_pat), the central
// problem's in a one-rank job.  The agents' patterns are taken back from the device once: the matrices the kernel will
// read.  No pass over the dataset.
int Exchange::live_cert_build() {
  LiveCertState &cs = live_;
  HostCsr central;
  const HostCsr *Qpat = &s_->job_pat;
  if (Qpat->n == 0) {
    DeviceProblem *cp = s_->central_problem();
    if (!cp) return fail("certify_live: the session kept no pattern of the job's Q", DCORA_ERR_UNSUPPORTED);
    if (s_->robust && s_->robust->central_pat.n == cp->Q.nrows) {
      Qpat = &s_->robust->central_pat;
    } else {
      const int rc = cp->Q.download(&central);
      if (rc) return rc;
      Qpat = &central;
    }
  }
  if (Qpat->n != (int)s_->num_cols()) return fail("certify_live: the job's pattern has another size", DCORA_ERR_BAD_ARG);
  cs.pat = dual_certificate_pattern(s_->global_manifold(), *Qpat);
  const long nnz = cs.pat.nnz();
  cs.agents.clear();
  for (int a = 0; a < s_->R; ++a) {
    AgentCore &core = s_->agent_core(a);
    if (!core.hosted) continue;
    const AgentBlock blk = s_->agent_block(a);
    std::vector<int> own((size_t)blk.k);
    for (int i = 0; i < blk.k; ++i) own[(size_t)i] = (int)blk.global_col(i);
    HostCsr Qaa, C;
    int rc = core.prob->Q.download(&Qaa);
    if (!rc) rc = core.coupling.download(&C);
    if (rc) return rc;
    const ManiDesc &m = core.prob->m;
    const long n_lambda = (long)m.n * m.d * m.d + m.l;
    CertRowTable t;
    rc = build_cert_row_table(cs.pat, own, Qaa, C, m, &t);
    if (!rc) rc = check_cert_row_table(t, nnz, Qaa.nnz(), C.nnz(), n_lambda);
    if (rc) return fail(std::string("certify_live: agent ") + std::to_string(a) + ": " + dcora_last_error(), rc);
    cs.agents.emplace_back();
    LiveCertState::Agent &A = cs.agents.back();
    A.id = a;
    const size_t ne = std::max<size_t>(t.size(), 1);
    DCORA_HIP(A.pos.alloc(ne));
    DCORA_HIP(A.src.alloc(ne));
    DCORA_HIP(A.slot.alloc(ne));
    DCORA_HIP(A.diag.alloc(ne));
    if (t.size()) {
      DCORA_HIP(hipMemcpy(A.pos.p, t.pos.data(), sizeof(int) * t.size(), hipMemcpyHostToDevice));
      DCORA_HIP(hipMemcpy(A.src.p, t.src.data(), sizeof(int) * t.size(), hipMemcpyHostToDevice));
      DCORA_HIP(hipMemcpy(A.slot.p, t.slot.data(), sizeof(int) * t.size(), hipMemcpyHostToDevice));
      DCORA_HIP(hipMemcpy(A.diag.p, t.diag.data(), t.size(), hipMemcpyHostToDevice));
    }
    A.pos_host = std::move(t.pos);
  }
  if (rank == 0) {
    DCORA_HIP(cs.vals.alloc((size_t)nnz));
    DCORA_HIP(hipEventCreateWithFlags(&cs.ready, hipEventDisableTiming));
  }
  cs.built = true;
  return DCORA_OK;
}

int Exchange::certify_live(double eta, int *certified, double *theta, double *lambda_min, double *v, long long *matvecs,
                           int *distributed, double *info10) {
  // refusals, from the arguments alone: no collective step has begun and the job is untouched
  if (!certified) return usage("certify_live: certified is required", DCORA_ERR_BAD_ARG);
  if (!std::isfinite(eta) || eta < 0) return usage("certify_live: eta must be finite and not negative", DCORA_ERR_BAD_ARG);
  // from here on a failure on this rank is the job's: the others leave their waits by the `failed` word
  const int rc = certify_live_run(eta, certified, theta, lambda_min, v, matvecs, distributed, info10);
  if (rc && hdr_) hdr_->failed.store(1);
  return rc;
}

int Exchange::certify_live_run(double eta, int *certified, double *theta, double *lambda_min, double *v,
                               long long *matvecs, int *distributed, double *info10) {
  const auto t0 = std::chrono::steady_clock::now();
  const int device = s_->opt.device;
  hipStream_t st = s_->st;
  DCORA_HIP(hipSetDevice(device));
  *certified = 0;
  if (theta) *theta = 0;
  if (lambda_min) *lambda_min = 0;
  if (matvecs) *matvecs = 0;
  if (distributed) *distributed = 0;
  if (info10) std::fill(info10, info10 + 10, 0.0);
  CertRows rows;
  int rc = cert_rows_begin(&rows);
  if (rc) return rc;
  if (!live_.built) {
    rc = live_cert_build();
    if (rc) return rc;
  }
  LiveCertState &cs = live_;
  if (cs.agents.size() != rows.blocks.size()) return fail("certify_live: the hosted agents changed", DCORA_ERR_BAD_ARG);
  // ---- every rank's rows of M = (Q - Lambda) + eta I, to rank 0 through the X area: round c carries entries
  // [c x_doubles, (c + 1) x_doubles) of the value array.  Kernel end, stream synchronise, barrier: rank 0 reads what
  // every rank's launches have stored; second barrier: nobody stores into the area before rank 0 has copied it ----
  const long nnz = cs.pat.nnz(), xd = (long)lay_.x_doubles;
  if (xd < 1) return fail("certify_live: the segment has no X area", DCORA_ERR_UNSUPPORTED);
  const int rounds = (int)((nnz + xd - 1) / xd);
  double *window = lay_.x(dev_map_);
  for (int c = 0; c < rounds; ++c) {
    const long lo = (long)c * xd, hi = std::min(nnz, lo + xd);
    for (size_t i = 0; i < cs.agents.size(); ++i) {
      const LiveCertState::Agent &A = cs.agents[i];
      const CertBlock &B = rows.blocks[i];
      size_t first = 0, last = 0;
      cert_row_window(A.pos_host, lo, hi, &first, &last);
      if (last == first) continue;
      const int count = (int)(last - first);
      hipLaunchKernelGGL(k_cert_rows, dim3((unsigned)((count + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, count,
                         (const int *)A.pos.p + first, (const int *)A.src.p + first, (const int *)A.slot.p + first,
                         (const unsigned char *)A.diag.p + first, (const double *)B.prob->Q.v.p, B.coupling.v,
                         (const double *)B.L.p, eta, (int)lo, window);
    }
    DCORA_HIP(hipGetLastError());
    DCORA_HIP(hipStreamSynchronize(st));
    rc = barrier();
    if (rc) return rc;
    if (rank == 0) {
      DCORA_HIP(hipMemcpyAsync(cs.vals.p + lo, lay_.x(map_), sizeof(double) * (size_t)(hi - lo), hipMemcpyHostToDevice, st));
      DCORA_HIP(hipStreamSynchronize(st));
    }
    rc = barrier();
    if (rc) return rc;
  }
  // ---- the PSD test on rank 0, on the values where they are; the verdict and info10 to every rank ----
  double out[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // {1 = PSD, 2 = not PSD; error code; info10}
  if (rank == 0) {
    bool psd = false;
    DCORA_HIP(hipEventRecord(cs.ready, st));
    const int c = device_chol_is_pd_dev(cs.pat, cs.vals.p, cs.ready, s_->cert_block(), device, &psd, out + 2);
    out[0] = c ? 0 : (psd ? 1 : 2);
    out[1] = c;
    out[10] = rounds;
    out[11] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  rc = allreduce_sum(out, 12);  // the other ranks add zeros: a broadcast
  if (rc) return rc;
  if (out[1] != 0) return fail("certify_live: the PSD test failed on rank 0", (int)out[1]);
  if (info10) std::copy(out + 2, out + 12, info10);
  if (out[0] == 1) {
    *certified = 1;
    return DCORA_OK;
  }
  // ---- refused: the row-block Lanczos stage.  Rank 0 needs M on its host for the second run's start vector and for
  // the shift-and-invert fallback: one download of the values onto the kept pattern, in this branch only ----
  double got[1] = {0};
  if (rank == 0) {
    cs.pat.v.resize((size_t)nnz);
    got[0] = fetch_values(st, cs.vals.p, (size_t)nnz, cs.pat.v.data());
  }
  rc = allreduce_sum(got, 1);
  if (rc) return rc;
  if (got[0] != 0) return fail("certify_live: the values could not be fetched on rank 0", (int)got[0]);
  return cert_min_eigenpair(rows, cs.pat, eta, true, theta, lambda_min, v, matvecs, distributed);
}

}  // namespace dcora
