// Certification entry points of the product (see cert.hip).
#pragma once
#include <cstdint>
#include <functional>
#include <vector>

#include "device_problem.h"

namespace dcora {

struct LanczosResult {
  bool ok = false;
  double lambda = 0;
  std::vector<double> v;
  long matvecs = 0;
};

class DeviceLanczos {
 public:
  static constexpr int kMaxNcv = 20;
  int device = 0, n = 0;
  hipStream_t st = nullptr;
  bool own_stream = true;
  DevCsr Sd;
  // shift-and-invert mode: when set, a Lanczos step applies (S - sigma I)^-1 through the partitioned sparse inverse
  // instead of S - shift I
  const SparsePrecond *inverse_op = nullptr;
  // Row-block form (one process per GPU, exchange.hip): this object holds rows [lo, lo + n) of a matrix of order
  // n_global.  op applies the row block (it moves the halo entries itself); allreduce sums `count` doubles over the
  // ranks in rank order, the same result on every rank.  Start vectors are generated for the whole problem on every
  // rank (same seed) and sliced, so the run does not depend on how the rows are split.
  std::function<int(const double *v, double *w)> op;
  std::function<int(double *vals, int count)> allreduce;
  int n_global = 0, lo = 0;
  // rows of this rank that are NOT one contiguous range of the whole problem (range-aided sessions: an agent's
  // variables are scattered over the global ordering): global index of every local row; empty = [lo, lo + n)
  std::vector<int> row_map;
  DevBuf<double> V, Vtmp, w, part, small;
  ~DeviceLanczos();
  int init(const HostCsr &S, int device_);
  int init_rows(int n_local, int n_global_, int lo_, int device_, hipStream_t stream);
  int largest_magnitude(double shift, int ncv, int maxit, double tol, const double *x0, uint64_t seed,
                        LanczosResult *out);
};

std::vector<double> min_eig_second_start(const HostCsr &S, uint64_t seed);
// the spectrum-shifted run would have to resolve min_eig_tol on a spectrum of width lambda_lm: below this ratio a
// 20-vector Krylov space is given no chance and the shift-and-invert fallback is taken at once (device_min_eig)
inline bool min_eig_shifted_run_hopeless(double min_eig_tol, double lambda_lm) { return min_eig_tol / lambda_lm < 1e-8; }
int device_min_eig(const HostCsr &S, int maxit, double min_eig_tol, int ncv, uint64_t seed, int device,
                   LanczosResult *out);
// (row, col) of Lambda's entries, in the order of launch_lambda_blocks's values (cert.hip)
void lambda_entries(const ManiDesc &m, std::vector<int> &I, std::vector<int> &J);
// the pattern of S + eta I over the entries Q stores: Q's entries, the entries of Lambda, every diagonal (no values) --
// what the host assembly hands to the PSD test and dcora_cert_prepare analyses
HostCsr dual_certificate_pattern(const ManiDesc &m, const HostCsr &Q);
int device_dual_certificate(const dcora_dims &dims, const double *Xh, const HostCsr &Q, int device, HostCsr *S);
int host_is_psd(const HostCsr &S, int block, bool *psd);
// info8 (may be null): the PSD test's, as device_chol_is_pd fills it
int device_fast_verification(const HostCsr &S, double eta, int block, int device, bool *psd, double *theta,
                             std::vector<double> *x, double *lambda_min, long *matvecs, double *info8 = nullptr);
// its second half (the PSD test has refused M = S + eta I): minimum eigenpair of M, theta = v^T (A - shift I) v
int device_verification_eigenpair(const HostCsr &M, double eta, const HostCsr &A, double shift, int device, double *theta,
                                  std::vector<double> *x, double *lambda_min, long *matvecs);

}  // namespace dcora
