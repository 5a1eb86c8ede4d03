// Certification of a live session on the device (see session_cert.h).
#include "session_cert.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>

#include "cert.h"
#include "device_chol.h"
#include "env.h"

namespace dcora {

namespace {

// The values of S + eta I = Q - Lambda + eta I in the CSR order of S's pattern, one thread per stored entry, gather form:
// entry p reads the Q value qidx names (if Q stores that entry), the Lambda value its slot names (if any) and writes its
// own output -- no atomics, no scatter, the same bits on every call.  The order (Q - Lambda) + eta is the host
// assembly's (device_dual_certificate, then csr_shift_diag).  8 bytes per lane, consecutive lanes on consecutive
// entries (qidx increases with p, skipping nothing: the Q values are read in order too).
__global__ __launch_bounds__(kBlock) void k_cert_values(int nnz, const double *__restrict__ Qv,
                                                        const int *__restrict__ qidx, const int *__restrict__ slot,
                                                        const unsigned char *__restrict__ diag,
                                                        const double *__restrict__ L, double eta,
                                                        double *__restrict__ out) {
  const long p = (long)blockIdx.x * kBlock + threadIdx.x;
  if (p >= nnz) return;
  const int pq = qidx[p], q = slot[p];
  double t = pq >= 0 ? Qv[pq] : 0.0;
  if (q >= 0) t -= L[q];
  if (diag[p]) t += eta;
  out[p] = t;
}

// the pattern of S + eta I and its three tables (host), the buffers of the device path
int build_state(SessionCertState &cs, DeviceProblem &central, const HostCsr *pattern, const HostCsr *live) {
  const ManiDesc &m = central.m;
  const DevCsr &Q = central.Q;
  const int k = Q.nrows, nnzq = Q.nnz;
  HostCsr own;
  if (!(pattern && pattern->n == k && pattern->nnz() == nnzq)) {
    own.n = k;
    own.ncols = Q.ncols;
    own.rp.resize((size_t)k + 1);
    own.ci.resize((size_t)nnzq);
    DCORA_HIP(hipMemcpy(own.rp.data(), Q.rp.p, sizeof(int) * ((size_t)k + 1), hipMemcpyDeviceToHost));
    if (nnzq) DCORA_HIP(hipMemcpy(own.ci.data(), Q.ci.p, sizeof(int) * (size_t)nnzq, hipMemcpyDeviceToHost));
    pattern = &own;
    live = nullptr;
  }
  // the entries of Q that S is built over: all the stored ones, or the live ones among them (a sub-pattern)
  const HostCsr *used = (live && live->n == k) ? live : pattern;
  // what the host assembly hands to the PSD test and dcora_cert_prepare analyses: Q's entries, the entries of Lambda,
  // every diagonal -- Q's own pattern unless Q lacks one of them (a rotation block with a structural zero, an isolated
  // pose, a unit sphere without a range)
  std::vector<int> LI, LJ;
  lambda_entries(m, LI, LJ);
  cs.pat = dual_certificate_pattern(m, *used);
  const HostCsr &P = cs.pat;
  const int nnz = P.nnz();
  auto find = [&](int i, int j) -> int {  // (every entry asked for is there)
    const int *lo = P.ci.data() + P.rp[i], *hi = P.ci.data() + P.rp[i + 1];
    return (int)(std::lower_bound(lo, hi, j) - P.ci.data());
  };
  std::vector<int> qidx((size_t)nnz, -1), slot((size_t)nnz, -1);
  std::vector<unsigned char> diag((size_t)nnz, 0);
  for (int i = 0; i < k; ++i) {
    int p = pattern->rp[i];  // (both rows are sorted: one walk finds every used entry among the stored ones)
    for (int u = used->rp[i]; u < used->rp[i + 1]; ++u) {
      while (p < pattern->rp[i + 1] && pattern->ci[p] < used->ci[u]) ++p;
      if (p == pattern->rp[i + 1] || pattern->ci[p] != used->ci[u]) {
        set_last_error("session certify: the live pattern is not part of the stored one");
        return DCORA_ERR_BAD_ARG;
      }
      qidx[(size_t)find(i, used->ci[u])] = p;
    }
  }
  for (size_t q = 0; q < LI.size(); ++q) slot[(size_t)find(LI[q], LJ[q])] = (int)q;
  for (int i = 0; i < k; ++i) diag[(size_t)find(i, i)] = 1;
  DCORA_HIP(cs.qidx.alloc((size_t)nnz));
  DCORA_HIP(cs.slot.alloc((size_t)nnz));
  DCORA_HIP(cs.diag.alloc((size_t)nnz));
  DCORA_HIP(hipMemcpy(cs.qidx.p, qidx.data(), sizeof(int) * (size_t)nnz, hipMemcpyHostToDevice));
  DCORA_HIP(hipMemcpy(cs.slot.p, slot.data(), sizeof(int) * (size_t)nnz, hipMemcpyHostToDevice));
  DCORA_HIP(hipMemcpy(cs.diag.p, diag.data(), (size_t)nnz, hipMemcpyHostToDevice));
  DCORA_HIP(cs.XQ.alloc((size_t)m.r * m.k));
  DCORA_HIP(cs.L.alloc(LI.size() + 1));
  DCORA_HIP(cs.vals.alloc((size_t)nnz));
  DCORA_HIP(hipEventCreateWithFlags(&cs.ready, hipEventDisableTiming));
  cs.built = true;
  return DCORA_OK;
}

// `count` doubles from the device (stream st) through pinned staging where there is some
int fetch(hipStream_t st, const double *dev, size_t count, double *host) {
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

}  // namespace

int session_certify(SessionCertState &cs, DeviceProblem &central, const HostCsr *pattern, const HostCsr *live,
                    const double *X, int block, double eta, CertifyResult *out, double *info8) {
  const ManiDesc &m = central.m;
  const int device = central.device;
  hipStream_t st = central.st;
  DCORA_HIP(hipSetDevice(device));
  *out = CertifyResult();
  if (!cs.built) {
    const int rc = build_state(cs, central, pattern, live);
    if (rc) return rc;
  }
  const int nnz = cs.pat.nnz();  // k at least: every diagonal is stored
  const auto t0 = std::chrono::steady_clock::now();
  central.enq_qapply(buf1(X), 0, nullptr, buf1(cs.XQ.p), 0, nullptr, Gate{});  // (the central problem has no linear term)
  launch_lambda_blocks(st, m, X, cs.XQ.p, cs.L.p);
  hipLaunchKernelGGL(k_cert_values, dim3((unsigned)((nnz + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, nnz,
                     (const double *)central.Q.v.p, (const int *)cs.qidx.p, (const int *)cs.slot.p,
                     (const unsigned char *)cs.diag.p, (const double *)cs.L.p, eta, cs.vals.p);
  DCORA_HIP(hipGetLastError());
  DCORA_HIP(hipEventRecord(cs.ready, st));
  const auto t1 = std::chrono::steady_clock::now();
  int rc = device_chol_is_pd_dev(cs.pat, cs.vals.p, cs.ready, block, device, &out->psd, info8);
  if (env::init_timing())
    fprintf(stderr, "[session certify] enqueue of X Q, Lambda and the values %.3f ms, PSD test %.3f ms: %s\n",
            std::chrono::duration<double, std::milli>(t1 - t0).count(),
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count(),
            out->psd ? "accepted" : "refused");
  if (rc || out->psd) return rc;
  // refused: the minimum eigenpair needs the matrix on the host (the Lanczos runs' start vector and the shift-and-invert
  // fallback read it).  One download of the values onto the kept pattern: M = S + eta I.
  cs.pat.v.resize((size_t)nnz);
  rc = fetch(st, cs.vals.p, (size_t)nnz, cs.pat.v.data());
  if (rc) return rc;
  return device_verification_eigenpair(cs.pat, eta, cs.pat, eta, device, &out->theta, &out->v, &out->lambda_min,
                                       &out->matvecs);
}

}  // namespace dcora
