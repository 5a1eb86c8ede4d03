// Certification on the device (replaces src/DCORA_utils.cpp:1713-1982):
//   * dual certificate S(X) = Q - Lambda(X): Q X^T by the SpMM kernel, Lambda blocks by a per-pose kernel;
//   * minimum eigenpair: thick-restart Lanczos (nev = 1, ncv = 20, largest magnitude, spectrum shift) whose
//     mat-vecs, re-orthogonalisation GEMVs and basis updates run on the GPU; only the <= 20 x 20 projected
//     eigenproblem is solved on the host (the recurrence: lanczos_restart.h; the plan of its runs: min_eig_plan.h);
//   * PSD test: sparse Cholesky of S + eta I on the host (setup-class code shared with the preconditioner).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <thread>

#include "cert.h"
#include "env.h"
#include "device_chol.h"
#include "device_problem.h"
#include "ra_rbcd.h"

namespace dcora {

namespace {
__global__ __launch_bounds__(kBlock) void k_basis_combine(int n, int m, int keep, const double *__restrict__ V,
                                                          const double *__restrict__ Z /* m x keep, col-major */,
                                                          double *__restrict__ out) {
  for (long t = (long)blockIdx.x * kBlock + threadIdx.x; t < n; t += (long)gridDim.x * kBlock)
    for (int c = 0; c < keep; ++c) {
      double s = 0;
      for (int i = 0; i < m; ++i) s += V[(size_t)i * n + t] * Z[(size_t)c * m + i];
      out[(size_t)c * n + t] = s;
    }
}

inline uint64_t splitmix(uint64_t &s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
inline double u01(uint64_t &s) { return (splitmix(s) >> 11) * (1.0 / 9007199254740992.0); }
}  // namespace

int DeviceLanczos::init(const HostCsr &S, int device_) {
  device = device_;
  n = S.n;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    set_last_error("no HIP device available: libdcora_hip has no CPU fallback");
    return DCORA_ERR_NO_DEVICE;
  }
  DCORA_HIP(hipSetDevice(device));
  DCORA_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  int rc = Sd.upload(S);
  if (rc) return rc;
  DCORA_HIP(V.alloc((size_t)n * (kMaxNcv + 1)));
  DCORA_HIP(Vtmp.alloc((size_t)n * kMaxNcv));
  DCORA_HIP(w.alloc(n));
  DCORA_HIP(part.alloc((size_t)kMaxPartials * 24));
  DCORA_HIP(small.alloc(1024));
  return DCORA_OK;
}
int DeviceLanczos::init_rows(int n_local, int n_global_, int lo_, int device_, hipStream_t stream) {
  device = device_;
  n = n_local;
  ranks.n_global = n_global_;
  ranks.lo = lo_;
  st = stream;
  own_stream = false;
  DCORA_HIP(hipSetDevice(device));
  const size_t nn = (size_t)std::max(n, 1);
  DCORA_HIP(V.alloc(nn * (kMaxNcv + 1)));
  DCORA_HIP(Vtmp.alloc(nn * kMaxNcv));
  DCORA_HIP(w.alloc(nn));
  DCORA_HIP(part.alloc((size_t)kMaxPartials * 24));
  DCORA_HIP(small.alloc(1024));
  return DCORA_OK;
}
DeviceLanczos::~DeviceLanczos() {
  if (st && own_stream) (void)hipStreamDestroy(st);
}

int LanczosRanks::reduce(hipStream_t st, double *dev, int count) const {
  if (!allreduce) return DCORA_OK;
  std::vector<double> tmp((size_t)count);
  DCORA_HIP(hipMemcpyAsync(tmp.data(), dev, sizeof(double) * count, hipMemcpyDeviceToHost, st));
  DCORA_HIP(hipStreamSynchronize(st));
  const int rc = allreduce(tmp.data(), count);
  if (rc) return rc;
  DCORA_HIP(hipMemcpyAsync(dev, tmp.data(), sizeof(double) * count, hipMemcpyHostToDevice, st));
  DCORA_HIP(hipStreamSynchronize(st));  // tmp leaves scope
  return DCORA_OK;
}

// per step 64 coefficients (two passes of 32) and the norm; raised by a step whose direction was dead
struct DeviceLanczos::CycleStore {
  DevBuf<double> h, beta;
  DevBuf<int> dead;
};

double DeviceLanczos::whole_vector(uint64_t s, const double *given) {
  double nn = 0;
  for (double &x : whole_) {
    x = given ? *given++ : (u01(s) - 0.5);
    nn += x * x;
  }
  ranks.slice(whole_.data(), n, local_.data());
  return std::sqrt(nn);
}

int DeviceLanczos::apply(int j) {
  double *vj = V.p + (size_t)j * n;
  const bool inverse = !op && inverse_op;
  if (op) {
    const int rc = op(vj, w.p);
    if (rc) return rc;
  } else if (inverse) {
    inverse_op->apply(st, 1, buf1(vj), w.p, Gate{});
  } else {
    launch_spmm(st, 1, Sd.view(), buf1(vj), 0, nullptr, buf1(w.p), 0, nullptr, Gate{});
  }
  if (!inverse && shift_ != 0) launch_scale_shift(st, n, shift_, vj, w.p);
  ++*matvecs_;
  return DCORA_OK;
}

int DeviceLanczos::orthogonalise(int nv, double *coeff) {
  launch_lanczos_proj(st, n, nv, V.p, w.p, part.p);
  launch_sum_partials(st, part.p, npart_, 24, nv, coeff);
  const int rc = ranks.reduce(st, coeff, nv);
  if (rc) return rc;
  launch_lanczos_sub(st, n, nv, V.p, coeff, w.p);
  return DCORA_OK;
}

int DeviceLanczos::norm2() {
  launch_dot(st, n, w.p, w.p, part.p);
  launch_sum_partials(st, part.p, npart_, 1, 1, small.p + 64);
  return ranks.reduce(st, small.p + 64, 1);
}

int DeviceLanczos::fresh_direction(int j) {
  whole_vector(seed_ + 7919 * (j + 1), nullptr);
  DCORA_HIP(hipMemcpyAsync(w.p, local_.data(), sizeof(double) * n, hipMemcpyHostToDevice, st));
  for (int pass = 0; pass < 2; ++pass) {
    const int rc = orthogonalise(j + 1, small.p);
    if (rc) return rc;
  }
  const int rc = norm2();
  if (rc) return rc;
  launch_scale(st, n, small.p + 64, w.p, V.p + (size_t)(j + 1) * n);
  DCORA_HIP(hipStreamSynchronize(st));
  return DCORA_OK;
}

// One Lanczos step = operator, two passes of projection against the whole basis, the norm, the next vector.  The slow
// form reads the coefficients and the norm back after every step (needed when the sums go over ranks, and to handle a
// vanishing norm); the fast form keeps them on the device -- the subtraction sums the projection's partials in its
// prologue, the next vector is scaled by the kernel that sums <w, w> -- and the host reads a whole restart cycle's
// coefficients at once: 8 launches and no host round trip per step instead of 11 launches, two copies and a wait.
int DeviceLanczos::slow_step(LanczosRestart &T, int j) {
  int rc = apply(j);
  if (rc) return rc;
  for (int pass = 0; pass < 2; ++pass) {
    rc = orthogonalise(j + 1, small.p + 32 * pass);
    if (rc) return rc;
  }
  rc = norm2();
  if (rc) return rc;
  double hbuf[64], b2 = 0;
  DCORA_HIP(hipMemcpyAsync(hbuf, small.p, sizeof(double) * 64, hipMemcpyDeviceToHost, st));
  DCORA_HIP(hipMemcpyAsync(&b2, small.p + 64, sizeof(double), hipMemcpyDeviceToHost, st));
  DCORA_HIP(hipStreamSynchronize(st));
  // a dead direction is an invariant subspace (the remainder is rounding noise of the orthogonalisation, or exactly
  // zero): continue with a fresh random direction orthogonalised against the basis
  if (!T.take_step(j, hbuf, hbuf + 32, b2)) return fresh_direction(j);
  launch_axpby(st, n, 1.0 / T.beta, w.p, 0.0, nullptr, V.p + (size_t)(j + 1) * n);
  return DCORA_OK;
}

int DeviceLanczos::fast_cycle(LanczosRestart &T) {
  CycleStore &c = *cycle_;
  const int m = T.m;
  const bool fused = npart_ <= kLanczosFuseParts;
  // (the dot's partials go behind the projection's in `part`: k_lanczos_sub_sum still reads those)
  double *dotpart = fused ? part.p + (size_t)npart_ * 24 : part.p;
  for (int j = T.k; j < m; ++j) {
    const int rc = apply(j);
    if (rc) return rc;
    const int nv = j + 1;
    double *hrow = c.h.p + (size_t)j * 64;
    for (int pass = 0; pass < 2; ++pass) {
      launch_lanczos_proj(st, n, nv, V.p, w.p, part.p);
      if (fused) {
        launch_lanczos_sub_sum(st, n, nv, V.p, part.p, npart_, hrow + 32 * pass, w.p, pass == 1 ? dotpart : nullptr);
      } else {
        launch_sum_partials(st, part.p, npart_, 24, nv, small.p + 32 * pass);
        launch_lanczos_keep(st, nv, small.p + 32 * pass, hrow + 32 * pass);
        launch_lanczos_sub(st, n, nv, V.p, small.p + 32 * pass, w.p);
      }
    }
    if (!fused) launch_dot(st, n, w.p, w.p, part.p);
    launch_lanczos_next(st, n, dotpart, npart_, c.beta.p + j, c.dead.p, w.p, V.p + (size_t)(j + 1) * n, hrow, nv);
  }
  std::vector<double> hh((size_t)m * 64), bb((size_t)m);
  int dead = 0;
  DCORA_HIP(hipMemcpyAsync(hh.data(), c.h.p, sizeof(double) * hh.size(), hipMemcpyDeviceToHost, st));
  DCORA_HIP(hipMemcpyAsync(bb.data(), c.beta.p, sizeof(double) * bb.size(), hipMemcpyDeviceToHost, st));
  DCORA_HIP(hipMemcpyAsync(&dead, c.dead.p, sizeof(int), hipMemcpyDeviceToHost, st));
  DCORA_HIP(hipStreamSynchronize(st));
  int jdead = m;
  if (dead)
    for (int j = T.k; j < m; ++j)
      if (!(bb[(size_t)j] >= 1e-300)) {
        jdead = j;
        break;
      }
  for (int j = T.k; j < jdead; ++j) T.take_live_step(j, &hh[(size_t)j * 64], &hh[(size_t)j * 64 + 32], bb[(size_t)j]);
  if (jdead < m) {  // a norm vanished at step jdead: that step and the rest of the cycle again, on the slow path
    DCORA_HIP(hipMemsetAsync(c.dead.p, 0, sizeof(int), st));
    *matvecs_ -= m - jdead;
    for (int j = jdead; j < m; ++j) {
      const int rc = slow_step(T, j);
      if (rc) return rc;
    }
  }
  return DCORA_OK;
}

int DeviceLanczos::combine(const std::vector<double> &cols, int count) {
  const int m = (int)cols.size() / count;
  DCORA_HIP(hipMemcpyAsync(small.p + 128, cols.data(), sizeof(double) * cols.size(), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_basis_combine, dim3(vec_grid(n)), dim3(kBlock), 0, st, n, m, count, V.p, small.p + 128, Vtmp.p);
  return DCORA_OK;
}

// Thick-restart Lanczos for the largest-magnitude eigenpair of (S - shift I): the recurrence of lanczos_restart.h over
// a basis on the device.
int DeviceLanczos::largest_magnitude(double shift, int ncv, int maxit, double tol, const double *x0, uint64_t seed,
                                     LanczosResult *out) {
  DCORA_HIP(hipSetDevice(device));
  out->ok = false;
  out->v.assign(n, 0.0);
  out->matvecs = 0;
  const int ng = ranks.order(n);
  if (ng == 0) return DCORA_OK;
  LanczosRestart T(std::min(ncv, kMaxNcv), ng);
  const int m = T.m;
  shift_ = shift;
  seed_ = seed;
  matvecs_ = &out->matvecs;
  npart_ = vec_grid(n);
  whole_.assign((size_t)ng, 0.0);
  local_.assign((size_t)std::max(n, 1), 0.0);
  {
    const double nn = whole_vector(seed ? seed : 1, x0);
    for (double &x : local_) x /= nn;
    DCORA_HIP(hipMemcpyAsync(V.p, local_.data(), sizeof(double) * n, hipMemcpyHostToDevice, st));
    DCORA_HIP(hipStreamSynchronize(st));
  }
  CycleStore cycle;
  cycle_ = !ranks.allreduce && !env::lanczos_sync() ? &cycle : nullptr;
  if (cycle_) {
    DCORA_HIP(cycle.h.alloc((size_t)m * 64));
    DCORA_HIP(cycle.beta.alloc((size_t)m));
    DCORA_HIP(cycle.dead.alloc(1));
    DCORA_HIP(hipMemsetAsync(cycle.dead.p, 0, sizeof(int), st));
  }
  for (int it = 0; it <= maxit; ++it) {
    if (cycle_) {
      const int rc = fast_cycle(T);
      if (rc) return rc;
    } else {
      for (int j = T.k; j < m; ++j) {
        const int rc = slow_step(T, j);
        if (rc) return rc;
      }
    }
    const bool conv = T.solve(tol);
    if (conv || it == maxit || T.spans_everything()) {
      out->ok = conv || T.spans_everything();
      out->lambda = T.theta();
      const std::vector<double> zc = T.ritz_coefficients(1);
      int rc = combine(zc, 1);
      if (rc) return rc;
      DCORA_HIP(hipMemcpyAsync(out->v.data(), Vtmp.p, sizeof(double) * n, hipMemcpyDeviceToHost, st));
      DCORA_HIP(hipStreamSynchronize(st));
      double nn = 0;
      for (double x : out->v) nn += x * x;
      rc = ranks.sum(&nn, 1);
      if (rc) return rc;
      nn = std::sqrt(nn);
      for (double &x : out->v) x /= nn;
      return DCORA_OK;
    }
    // thick restart: V[:, 0:keep] = V Z[:, ord[0:keep]], V[:, keep] = v_{m}
    const std::vector<double> Zk = T.ritz_coefficients(T.keep);
    const int rc = combine(Zk, T.keep);
    if (rc) return rc;
    DCORA_HIP(hipMemcpyAsync(V.p, Vtmp.p, sizeof(double) * (size_t)n * T.keep, hipMemcpyDeviceToDevice, st));
    DCORA_HIP(hipMemcpyAsync(V.p + (size_t)T.keep * n, V.p + (size_t)m * n, sizeof(double) * n,
                             hipMemcpyDeviceToDevice, st));
    DCORA_HIP(hipStreamSynchronize(st));
    T.restart();
  }
  return DCORA_OK;
}

// default when the eigenvalue computation is unsuccessful: ref src/Graph.cpp:1923, 1932-1939
int device_precond_regularization(const HostCsr &Q, int device, double *reg) {
  *reg = 1e-1;
  DeviceLanczos L;
  int rc = L.init(Q, device);
  if (rc) return rc;
  LanczosResult e;
  rc = L.largest_magnitude(0.0, std::min(6, Q.n), 10000, 1e-3, nullptr, 1, &e);
  if (rc) return rc;
  if (e.ok && e.lambda > 0) *reg = e.lambda / (1e6 - 1);
  return DCORA_OK;
}

// start vector of the spectrum-shifted run: the first row of the matrix with a ~3 % random perturbation
// (ref src/DCORA_utils.cpp:1861-1866)
std::vector<double> min_eig_second_start(const HostCsr &S, uint64_t seed) {
  const int k = S.n;
  std::vector<double> x0((size_t)k, 0.0), pert((size_t)k);
  for (int p = S.rp[0]; p < S.rp[1]; ++p) x0[S.ci[p]] = S.v[p];
  uint64_t s = seed + 17;
  double pn = 0, vn = 0;
  for (int i = 0; i < k; ++i) {
    pert[i] = 2 * u01(s) - 1;
    pn += pert[i] * pert[i];
    vn += x0[i] * x0[i];
  }
  pn = std::sqrt(pn);
  vn = std::sqrt(vn);
  for (int i = 0; i < k; ++i) x0[i] += 0.03 * vn * pert[i] / pn;
  return x0;
}

namespace {
// One attempt of the shift-and-invert fallback (ref :1878-1888 -> :1751-1805): Lanczos on (S - sigma I)^-1.  The solve
// per step is the partitioned sparse inverse of the SPD matrix S - sigma I replayed on the device (sparse_precond.h), one
// right-hand side; a matrix that is not positive definite is an outcome, not an error.
int inverse_attempt(DeviceLanczos &L, const HostCsr &S, double sigma, int ncv, uint64_t seed, int nthreads,
                    LanczosResult *si, ShiftLadder::Outcome *outcome) {
  PartInvHost P;
  DeviceWeightSink sink(L.device);  // the stored weights stream to the device while they are formed
  P.sink = &sink;
  const int brc = build_partitioned_inverse_auto(csr_shift_diag(S, -sigma), 1, nthreads, L.device, &P);
  *outcome = ShiftLadder::Outcome::not_pd;
  if (brc) return brc == DCORA_ERR_NOT_PD ? DCORA_OK : brc;
  SparsePrecond inv;
  auto img = std::make_shared<SpImage>();
  int rc = img->upload(P, &sink);
  if (rc) return rc;
  rc = inv.attach(img, 1);
  if (rc) return rc;
  const MinEigPlan::Run run = MinEigPlan::inverse_run(ncv);
  L.inverse_op = &inv;
  rc = L.largest_magnitude(run.shift, run.ncv, run.maxit, run.tol, nullptr, seed, si);
  L.inverse_op = nullptr;
  if (rc) return rc;
  if (env::init_timing())
    fprintf(stderr, "[min_eig] shift-and-invert at sigma %.3g: %ld solves, converged %d\n", sigma, si->matvecs, (int)si->ok);
  *outcome = si->ok ? ShiftLadder::Outcome::converged : ShiftLadder::Outcome::factored_but_not_converged;
  return DCORA_OK;
}
}  // namespace

// min_eig_plan.h with its runs on this device
int device_min_eig(const HostCsr &S, int maxit, double min_eig_tol, int ncv, uint64_t seed, int device,
                   LanczosResult *out) {
  using After = MinEigPlan::AfterFirst;
  const MinEigPlan plan{MinEigPlan::Shortcut::always, MinEigPlan::OnFailedFirst::error};
  DeviceLanczos L;
  int rc = L.init(S, device);
  if (rc) return rc;
  const int k = S.n;
  ncv = std::min(ncv, k);
  auto lanczos = [&](const MinEigPlan::Run &run, const double *x0, LanczosResult *res) {
    return L.largest_magnitude(run.shift, run.ncv, run.maxit, run.tol, x0, seed, res);
  };
  LanczosResult lm;
  rc = lanczos(plan.first_run(ncv, maxit), nullptr, &lm);
  if (rc) return rc;
  const After after = plan.after_first_run(lm.ok, lm.lambda, min_eig_tol, true);
  if (after == After::failed_first) {
    set_last_error("min_eig: could not compute the largest-magnitude eigenvalue of S");
    *out = lm;
    return DCORA_ERR_NO_CONVERGENCE;
  }
  if (after == After::done_negative || after == After::done_zero) {
    *out = lm;
    return DCORA_OK;
  }
  const double lambda_lm = lm.lambda;
  const std::vector<double> x0 = min_eig_second_start(S, seed);
  const MinEigPlan::Run shifted = plan.shifted_run(lambda_lm, min_eig_tol, ncv, maxit);
  LanczosResult sh;  // (the shortcut: the run not made counts as not converged; the eigenpair is the fallback's either way)
  sh.v.assign((size_t)k, 0.0);
  if (after == After::shifted) {
    rc = lanczos(shifted, x0.data(), &sh);
    if (rc) return rc;
  }
  sh.matvecs += lm.matvecs;
  if (env::init_timing())
    fprintf(stderr, "[min_eig] k %d: largest-magnitude run %ld matvecs (lambda %.3e), shifted run %ld matvecs, converged %d\n", k,
            lm.matvecs, lm.lambda, sh.matvecs - lm.matvecs, (int)sh.ok);
  if (sh.ok) {
    sh.lambda = plan.shifted_eigenvalue(sh.lambda, lambda_lm);
    *out = sh;
    return DCORA_OK;
  }
  const int nthreads = std::max(1, std::min(host_cpus_available(), 32));
  ShiftLadder ladder(lambda_lm, min_eig_tol, after == After::fallback_hopeless);
  while (ladder.step() != ShiftLadder::Step::end) {
    LanczosResult res;
    ShiftLadder::Outcome outcome = ShiftLadder::Outcome::factored_but_not_converged;
    if (ladder.step() == ShiftLadder::Step::invert) {
      rc = inverse_attempt(L, S, ladder.sigma(), ncv, seed, nthreads, &res, &outcome);
      if (rc) return rc;
      if (outcome == ShiftLadder::Outcome::converged) {
        res.matvecs += sh.matvecs;
        res.lambda = plan.inverse_eigenvalue(res.lambda, ladder.sigma());
        *out = res;
        return DCORA_OK;
      }
    } else {
      // the shortcut skipped the reference's first attempt and the fallback delivered nothing: make that attempt now
      rc = lanczos(shifted, x0.data(), &res);
      if (rc) return rc;
      res.matvecs += sh.matvecs;
      if (res.ok) {
        res.lambda = plan.shifted_eigenvalue(res.lambda, lambda_lm);
        *out = res;
        return DCORA_OK;
      }
      sh = res;
    }
    ladder.next(outcome);
  }
  set_last_error("min_eig: neither the spectrum-shifted nor the shift-and-invert Lanczos run converged");
  *out = sh;
  out->lambda = plan.shifted_eigenvalue(sh.lambda, lambda_lm);
  return DCORA_ERR_NO_CONVERGENCE;
}

// ref src/DCORA_utils.cpp:1898-1982
// The entries of Lambda(X) in S = Q - Lambda (ref src/DCORA_utils.cpp:1898-1982): the d x d block of every rotation,
// then the diagonal entry of every unit sphere, appended to I (rows) and J (columns).  The q-th entry appended is the
// q-th value launch_lambda_blocks writes (rotation blocks column-major).
void lambda_entries(const ManiDesc &m, std::vector<int> &I, std::vector<int> &J) {
  for (int i = 0; i < m.n; ++i) {
    const int c = m.rot_col(i);
    for (int b = 0; b < m.d; ++b)
      for (int a = 0; a < m.d; ++a) {
        I.push_back(c + a);
        J.push_back(c + b);
      }
  }
  for (int i = 0; i < m.l; ++i) {
    I.push_back(m.sphere_col(i));
    J.push_back(m.sphere_col(i));
  }
}

HostCsr dual_certificate_pattern(const ManiDesc &m, const HostCsr &Q) {
  std::vector<int> I, J;
  I.reserve((size_t)Q.nnz() + (size_t)m.n * m.d * m.d + m.l);
  J.reserve(I.capacity());
  for (int i = 0; i < Q.n; ++i)
    for (int p = Q.rp[i]; p < Q.rp[i + 1]; ++p) {
      I.push_back(i);
      J.push_back(Q.ci[p]);
    }
  lambda_entries(m, I, J);
  return pattern_of(csr_shift_diag(csr_from_coo(Q.n, Q.n, I, J, std::vector<double>(I.size(), 1.0)), 1.0));
}

int device_dual_certificate(const dcora_dims &dims, const double *Xh, const HostCsr &Q, int device, HostCsr *S) {
  if (dims.r < 1 || dims.r > 16 || (dims.d != 2 && dims.d != 3) || dims.n < 0 || dims.l < 0 || dims.b < 0) {
    set_last_error("bad dims (need 1 <= r <= 16, d in {2,3})");
    return DCORA_ERR_BAD_ARG;
  }
  const ManiDesc m = make_mani(dims);
  if (Q.n != m.k) {
    set_last_error("Q dimension does not match (d+1) n + l + b");
    return DCORA_ERR_BAD_ARG;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    set_last_error("no HIP device available: libdcora_hip has no CPU fallback");
    return DCORA_ERR_NO_DEVICE;
  }
  DCORA_HIP(hipSetDevice(device));
  // only what the two kernels need: Q, X, X Q and the Lambda blocks (no solver workspace).  Q without long rows (a
  // pose graph, or a range-aided one whose landmarks are ranged from few poses) goes into ONE recycled scratch block
  // with the vectors: six allocations and six frees per certificate were 3 of its 5 ms at k = 10 000.
  const size_t N = (size_t)m.r * m.k;
  const size_t NL = (size_t)m.n * m.d * m.d + m.l;
  std::vector<double> L(NL + 1);
  bool long_rows = false;
  for (int i = 0; i < Q.n && !long_rows; ++i) long_rows = Q.rp[i + 1] - Q.rp[i] > kLongRow;
  if (!long_rows) {
    auto up8 = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t nnz = (size_t)Q.nnz();
    const size_t o_v = 0, o_x = o_v + up8(nnz * 8), o_xq = o_x + up8(N * 8), o_l = o_xq + up8(N * 8),
                 o_rp = o_l + up8((NL + 1) * 8), o_ci = o_rp + up8((size_t)(Q.n + 1) * 4), total = o_ci + up8(nnz * 4);
    struct Arena {
      int device;
      size_t bytes;
      char *p;
      ~Arena() { scratch_release(device, p, bytes); }
    } ar{device, total, scratch_acquire(device, total)};
    if (!ar.p) {
      set_last_error("dual certificate: device allocation failed");
      return DCORA_ERR_HIP;
    }
    double *dv = (double *)(ar.p + o_v), *dX = (double *)(ar.p + o_x), *dXQ = (double *)(ar.p + o_xq),
           *dL = (double *)(ar.p + o_l);
    int *drp = (int *)(ar.p + o_rp), *dci = (int *)(ar.p + o_ci);
    // the inputs travel through ONE pinned block laid out like the device block (copies from pageable memory stall
    // for tens of milliseconds now and then: device_chol.h), the Lambda blocks come back through its tail
    struct Pin {
      size_t bytes;
      char *p;
      ~Pin() { pinned_release(p, bytes); }
    } pin{total, total <= ((size_t)256 << 20) ? pinned_acquire(total) : nullptr};
    if (pin.p) {
      std::memcpy(pin.p + o_v, Q.v.data(), nnz * 8);
      std::memcpy(pin.p + o_x, Xh, sizeof(double) * N);
      std::memcpy(pin.p + o_rp, Q.rp.data(), (size_t)(Q.n + 1) * 4);
      std::memcpy(pin.p + o_ci, Q.ci.data(), nnz * 4);
      DCORA_HIP(hipMemcpyAsync(dv, pin.p + o_v, o_xq - o_v, hipMemcpyHostToDevice, nullptr));
      DCORA_HIP(hipMemcpyAsync(drp, pin.p + o_rp, total - o_rp, hipMemcpyHostToDevice, nullptr));
    } else {
      DCORA_HIP(hipMemcpyAsync(dv, Q.v.data(), nnz * 8, hipMemcpyHostToDevice, nullptr));
      DCORA_HIP(hipMemcpyAsync(drp, Q.rp.data(), (size_t)(Q.n + 1) * 4, hipMemcpyHostToDevice, nullptr));
      DCORA_HIP(hipMemcpyAsync(dci, Q.ci.data(), nnz * 4, hipMemcpyHostToDevice, nullptr));
      DCORA_HIP(hipMemcpyAsync(dX, Xh, sizeof(double) * N, hipMemcpyHostToDevice, nullptr));
    }
    CsrDev Qv;
    Qv.nrows = Q.n;
    Qv.nnz = (int)nnz;
    Qv.rp = drp;
    Qv.ci = dci;
    Qv.v = dv;
    launch_spmm(nullptr, m.r, Qv, buf1(dX), 0, nullptr, buf1(dXQ), 0, nullptr, Gate{});
    launch_lambda_blocks(nullptr, m, dX, dXQ, dL);
    if (pin.p) {
      DCORA_HIP(hipMemcpyAsync(pin.p + o_l, dL, sizeof(double) * NL, hipMemcpyDeviceToHost, nullptr));
      DCORA_HIP(hipStreamSynchronize(nullptr));
      std::memcpy(L.data(), pin.p + o_l, sizeof(double) * NL);
    } else {
      DCORA_HIP(hipMemcpy(L.data(), dL, sizeof(double) * NL, hipMemcpyDeviceToHost));
    }
  } else {
    DevCsr Qd;
    int rc = Qd.upload(Q);
    if (rc) return rc;
    DevBuf<double> dX, dXQ, dL;
    DCORA_HIP(dX.alloc(N));
    DCORA_HIP(dXQ.alloc(N));
    DCORA_HIP(dL.alloc(NL + 1));
    DCORA_HIP(hipMemcpy(dX.p, Xh, sizeof(double) * N, hipMemcpyHostToDevice));
    launch_spmm(nullptr, m.r, Qd.view(), buf1(dX.p), 0, nullptr, buf1(dXQ.p), 0, nullptr, Gate{});
    launch_lambda_blocks(nullptr, m, dX.p, dXQ.p, dL.p);
    DCORA_HIP(hipMemcpy(L.data(), dL.p, sizeof(double) * NL, hipMemcpyDeviceToHost));
  }
  // S = Q - Lambda.  Lambda is block diagonal on entries that Q's own pattern holds (the d x d rotation blocks
  // and the unit-sphere diagonal): subtract in place on a copy of Q; fall back to a merge when an entry is absent.
  std::vector<int> LI, LJ;
  lambda_entries(m, LI, LJ);
  {
    HostCsr T = Q;
    bool all_found = true;
    for (size_t q = 0; q < LI.size() && all_found; ++q) {
      const int *lo = T.ci.data() + T.rp[LI[q]], *hi = T.ci.data() + T.rp[LI[q] + 1];
      const int *it = std::lower_bound(lo, hi, LJ[q]);
      if (it == hi || *it != LJ[q])
        all_found = false;
      else
        T.v[it - T.ci.data()] -= L[q];
    }
    if (all_found) {
      *S = std::move(T);
      return DCORA_OK;
    }
  }
  std::vector<int> I, J;
  std::vector<double> V;
  I.reserve(Q.nnz() + NL);
  J.reserve(Q.nnz() + NL);
  V.reserve(Q.nnz() + NL);
  for (int i = 0; i < Q.n; ++i)
    for (int p = Q.rp[i]; p < Q.rp[i + 1]; ++p) {
      I.push_back(i);
      J.push_back(Q.ci[p]);
      V.push_back(Q.v[p]);
    }
  I.insert(I.end(), LI.begin(), LI.end());
  J.insert(J.end(), LJ.begin(), LJ.end());
  for (size_t q = 0; q < LI.size(); ++q) V.push_back(-L[q]);
  *S = csr_from_coo(Q.n, Q.n, I, J, V);
  return DCORA_OK;
}

int host_is_psd(const HostCsr &S, int block, bool *psd) {
  SparseChol c;
  *psd = c.factor(S, block);
  return DCORA_OK;
}

// the half of fastVerification that runs when the PSD test has refused (ref src/DCORA_utils.cpp:1725-1733): the minimum
// eigenpair of M = S + eta I and theta = v^T S v.  S is given as A - shift I: (S, 0) by the caller that holds S, (M, eta)
// by the one that holds only M (session_cert.hip).
int device_verification_eigenpair(const HostCsr &M, double eta, const HostCsr &A, double shift, int device, double *theta,
                                  std::vector<double> *x, double *lambda_min, long *matvecs) {
  LanczosResult e;
  const int rc = device_min_eig(M, 1000, eta, 20, 12345, device, &e);
  if (rc && rc != DCORA_ERR_NO_CONVERGENCE) return rc;
  double th = 0, vv = 0;
  for (int i = 0; i < A.n; ++i) {
    double s = 0;
    for (int p = A.rp[i]; p < A.rp[i + 1]; ++p) s += A.v[p] * e.v[A.ci[p]];
    th += e.v[i] * s;
    vv += e.v[i] * e.v[i];
  }
  if (shift != 0) th -= shift * vv;
  if (theta) *theta = th;
  if (x) *x = e.v;
  if (lambda_min) *lambda_min = e.lambda;
  if (matvecs) *matvecs = e.matvecs;
  return rc;
}

// ref src/DCORA_utils.cpp:1713-1735
int device_fast_verification(const HostCsr &S, double eta, int block, int device, bool *psd, double *theta,
                             std::vector<double> *x, double *lambda_min, long *matvecs, double *info8) {
  HostCsr M = csr_shift_diag(S, eta);
  // the PSD test: LL^T of S + eta I succeeds <=> PSD up to eta (ref src/DCORA_utils.cpp:1737-1747), factorised on the
  // device (device_chol.h)
  int rc = device_chol_is_pd(M, block, device, psd, info8);
  if (rc) return rc;
  if (*psd) return DCORA_OK;
  return device_verification_eigenpair(M, eta, S, 0.0, device, theta, x, lambda_min, matvecs);
}

}  // namespace dcora
