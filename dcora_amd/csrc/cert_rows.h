// The addressing of the job-wide certificate (Exchange::certify_live, exchange_cert.hip): which stored entries of
// M = (Q - Lambda) + eta I one agent's rows are, and where each takes its value from.  Host code, built once per job;
// nothing in it depends on r, so it survives lifts, and nothing on the values, so it survives re-weights (the device
// matrices keep their creation patterns).
#pragma once
#include <vector>

#include "host_sparse.h"
#include "kernels.h"

namespace dcora {

// One entry per stored entry of the agent's rows of the job-wide pattern, ascending in `pos`.
struct CertRowTable {
  std::vector<int> pos;             // its place in the job-wide value array (CSR order of the pattern of S + eta I)
  std::vector<int> src;             // >= 0: that value of the agent's Q_aa; <= -2: value -2 - src of its coupling block;
                                    // -1: neither stores the entry
  std::vector<int> slot;            // its Lambda value (launch_lambda_blocks's order on the agent's manifold) or -1
  std::vector<unsigned char> diag;  // 1 on the diagonal
  size_t size() const { return pos.size(); }
};

// P: the job-wide pattern (dual_certificate_pattern of the job's creation-time Q); own: the global column of each of
// the agent's columns; Qaa (square, the agent's ordering) and C (rows: the agent's columns, columns: global) as the
// device holds them; m: the agent's manifold.  DCORA_ERR_BAD_ARG when the agent's matrices, its Lambda entries or a
// diagonal do not lie inside P, or when a column map is not one.
int build_cert_row_table(const HostCsr &P, const std::vector<int> &own, const HostCsr &Qaa, const HostCsr &C,
                         const ManiDesc &m, CertRowTable *out);
// every index against the length of the array it addresses (nnz of P, of Qaa, of C; the Lambda values): a table that
// fails is DCORA_ERR_BAD_ARG and is never launched on
int check_cert_row_table(const CertRowTable &t, long nnz_p, long nnz_q, long nnz_c, long n_lambda);
// entries [*first, *last) of a table's positions lie in the window [lo, hi) of the value array
void cert_row_window(const std::vector<int> &pos, long lo, long hi, size_t *first, size_t *last);
// the kernel's arithmetic by a host loop (dcora_debug_cert_rows): entries [first, last) into window[pos - lo],
// written[pos - lo] counted up
void cert_rows_host(const CertRowTable &t, size_t first, size_t last, const double *Qv, const double *Cv,
                    const double *L, double eta, long lo, double *window, unsigned char *written);

}  // namespace dcora
