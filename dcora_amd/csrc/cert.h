// Certification entry points of the product (see cert.hip).
#pragma once
#include <cstdint>
#include <functional>
#include <vector>

#include "device_problem.h"
#include "min_eig_plan.h"

namespace dcora {

struct LanczosResult {
  bool ok = false;
  double lambda = 0;
  std::vector<double> v;
  long matvecs = 0;
};

// How a Lanczos run is spread over the ranks of a job (one process per GPU, exchange.hip): this rank holds rows
// [lo, lo + n) of a matrix of order n_global -- or the rows row_map lists, where they are NOT one contiguous range of
// the whole problem (range-aided sessions: an agent's variables are scattered over the global ordering).  allreduce sums
// `count` doubles over the ranks in rank order, the same result on every rank.  Start vectors are generated for the
// whole problem on every rank (same seed) and sliced, so the run does not depend on how the rows are split.  Left as
// constructed it is one process holding everything: the identity in all three answers.
struct LanczosRanks {
  std::function<int(double *vals, int count)> allreduce;
  int n_global = 0, lo = 0;
  std::vector<int> row_map;  // global index of every local row; empty = [lo, lo + n)
  int order(int n) const { return allreduce ? n_global : n; }
  void slice(const double *whole, int n, double *local) const {
    for (int i = 0; i < n; ++i) local[i] = whole[row_map.empty() ? (size_t)lo + i : (size_t)row_map[(size_t)i]];
  }
  int sum(double *vals, int count) const { return allreduce ? allreduce(vals, count) : DCORA_OK; }
  // the sum over the ranks of `count` doubles that sit on the device at dev
  int reduce(hipStream_t st, double *dev, int count) const;
};

struct LanczosRestart;

class DeviceLanczos {
 public:
  static constexpr int kMaxNcv = 20;
  int device = 0, n = 0;
  hipStream_t st = nullptr;
  bool own_stream = true;
  DevCsr Sd;
  // The operator of a step, in this order of precedence: op (the row-block form: it applies this rank's rows and moves
  // the halo entries itself), then inverse_op (shift-and-invert mode: (S - sigma I)^-1 through the partitioned sparse
  // inverse), else Sd; op and Sd are followed by - shift v
  std::function<int(const double *v, double *w)> op;
  const SparsePrecond *inverse_op = nullptr;
  LanczosRanks ranks;
  DevBuf<double> V, Vtmp, w, part, small;
  ~DeviceLanczos();
  int init(const HostCsr &S, int device_);
  int init_rows(int n_local, int n_global_, int lo_, int device_, hipStream_t stream);
  int largest_magnitude(double shift, int ncv, int maxit, double tol, const double *x0, uint64_t seed,
                        LanczosResult *out);

 private:
  struct CycleStore;  // a restart cycle's coefficients kept on the device
  // one run's state
  double shift_ = 0;
  uint64_t seed_ = 0;
  long *matvecs_ = nullptr;
  int npart_ = 0;
  CycleStore *cycle_ = nullptr;
  std::vector<double> whole_, local_;
  // this rank's slice (in local_) of a vector of the whole problem: x0 or the seeded stream; -> its norm
  double whole_vector(uint64_t s, const double *given);
  // the operations on the basis, each stated once; w is the vector in work
  int apply(int j);                                // w = operator (V_j)
  int orthogonalise(int nv, double *coeff);        // coeff = V[:, 0:nv]^T w (summed over the ranks), w -= V coeff
  int norm2();                                     // small[64] = <w, w> (summed over the ranks)
  int fresh_direction(int j);                      // V_{j+1} = a seeded random vector, orthogonal to V_0 .. V_j, unit
  int slow_step(LanczosRestart &T, int j);         // step j with a read-back of its coefficients
  int fast_cycle(LanczosRestart &T);               // steps T.k .. T.m - 1 with one read-back
  int combine(const std::vector<double> &cols, int count);  // Vtmp[:, 0:count] = V[:, 0:m] cols
};

std::vector<double> min_eig_second_start(const HostCsr &S, uint64_t seed);
// the plan of computeMinimumEigenPair (min_eig_plan.h) with its runs on one device
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
