// Certification of a live single-process RBCD session (either kind) on the device: fastVerification (ref
// src/DCORA_utils.cpp:1713-1735) of S = Q - Lambda(X) with the Q the session's central problem holds NOW -- after every
// weight change -- and the mirror X as it stands.  The accepting path stays on the device: X Q by the central problem's
// own Q-apply, the Lambda blocks by k_lambda, the values of S + eta I gathered in the CSR order of S's pattern
// (k_cert_values) and factorised where they are (device_chol_is_pd_dev); only the verdict crosses to the host.  S's
// pattern is Q's wherever Q stores every entry of Lambda and every diagonal; where it does not (sphere2500's Q has six
// structural zeros inside rotation blocks; an isolated pose; a unit sphere without a range) the gather runs over the
// union, which is the pattern the host assembly inserts those entries into: no session is sent back to the host.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "device_problem.h"
#include "host_sparse.h"

namespace dcora {

// what a session keeps between certificates; all of it depends on the central pattern alone, so a re-weight (new
// values on the creation pattern) leaves it valid -- unless the session certifies over the live entries only
// (session_certify's `live`), whose owner calls reset() when they change
struct SessionCertState {
  bool built = false;
  // the pattern of S + eta I: Q's entries, the entries of Lambda, every diagonal (Q's own pattern where Q stores all of
  // them) -- the pattern the host assembly gives, so both find the same analysis in the factorisation's cache; v: where
  // the values land when the PSD test has refused
  HostCsr pat;
  DevBuf<int> qidx;             // per stored entry of pat: index of Q's stored entry, -1 where Q has none
  DevBuf<int> slot;             // ... index into the Lambda values (launch_lambda_blocks's order) or -1
  DevBuf<unsigned char> diag;   // ... 1 on the diagonal
  DevBuf<double> XQ, L, vals;   // X Q, the Lambda values, the values of S + eta I
  hipEvent_t ready = nullptr;   // vals complete (the factorisation runs on a stream of its own)
  SessionCertState() = default;
  SessionCertState(const SessionCertState &) = delete;
  SessionCertState &operator=(const SessionCertState &) = delete;
  ~SessionCertState() {
    if (ready) (void)hipEventDestroy(ready);
  }
  void reset() {  // as never built (no certificate in flight)
    if (ready) (void)hipEventDestroy(ready);
    ready = nullptr;
    built = false;
    pat = HostCsr();
    qidx.release();
    slot.release();
    diag.release();
    XQ.release();
    L.release();
    vals.release();
  }
};

struct CertifyResult {
  bool psd = false;
  double theta = 0, lambda_min = 0;  // (not PSD only) theta = v^T S v, lambda_min of S + eta I
  std::vector<double> v;             // (not PSD only) its unit eigenvector, the central problem's ordering
  long matvecs = 0;
};

// central: the session's central problem (its stream: the session's; nothing else of the session in flight on another
// stream); pattern: the host copy of its CSR pattern where the session keeps one (else taken back from the device once);
// X: the mirror, r x k in the central problem's ordering (device); block: unknowns ordered together by the factorisation.
// live (may be null: all of them): the stored entries the session's current weights give, a sub-pattern of `pattern` --
// a re-weighted session whose creation pattern keeps explicit zeros certifies over these alone, i.e. over the matrix a
// fresh session with its weights would hold, to the same bits (the factorisation and the Lanczos runs see that pattern).
// Writes nothing the session reads.  info8 (may be null): as device_chol_is_pd fills it.
int session_certify(SessionCertState &cs, DeviceProblem &central, const HostCsr *pattern, const HostCsr *live,
                    const double *X, int block, double eta, CertifyResult *out, double *info8);

}  // namespace dcora
