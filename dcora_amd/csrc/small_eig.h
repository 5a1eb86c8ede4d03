// The r x r symmetric eigenproblem of a rank-d truncation (r <= 16), on the host: shared by the host-fed
// projectSolutionRASLAM (round.hip) and the projection of a live session (session_project.hip).
#pragma once
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace dcora {

// cyclic Jacobi eigen-decomposition of a small symmetric matrix (host): G = V diag(w) V^T
inline void jacobi_eig(int n, std::vector<double> &G, std::vector<double> &V) {
  V.assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) V[(size_t)i * n + i] = 1.0;
  for (int sweep = 0; sweep < 100; ++sweep) {
    double off = 0;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) off = std::max(off, std::fabs(G[(size_t)q * n + p]));
    double diag = 0;
    for (int i = 0; i < n; ++i) diag = std::max(diag, std::fabs(G[(size_t)i * n + i]));
    if (off <= 1e-16 * std::max(diag, 1e-300)) break;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = G[(size_t)q * n + p];
        if (std::fabs(apq) <= 1e-300) continue;
        const double app = G[(size_t)p * n + p], aqq = G[(size_t)q * n + q];
        const double zeta = (aqq - app) / (2.0 * apq);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
        for (int i = 0; i < n; ++i) {  // columns p, q
          const double x = G[(size_t)p * n + i], y = G[(size_t)q * n + i];
          G[(size_t)p * n + i] = c * x - s * y;
          G[(size_t)q * n + i] = s * x + c * y;
        }
        for (int i = 0; i < n; ++i) {  // rows p, q
          const double x = G[(size_t)i * n + p], y = G[(size_t)i * n + q];
          G[(size_t)i * n + p] = c * x - s * y;
          G[(size_t)i * n + q] = s * x + c * y;
        }
        for (int i = 0; i < n; ++i) {
          const double x = V[(size_t)p * n + i], y = V[(size_t)q * n + i];
          V[(size_t)p * n + i] = c * x - s * y;
          V[(size_t)q * n + i] = s * x + c * y;
        }
      }
  }
}

// The form the certificate's Lanczos recurrence has used since its first version (lanczos_restart.h): A = Z diag(w) Z^T
// with the eigenvectors as the COLUMNS of the row-major Z, the sweeps ended by the off-diagonal's share of the Frobenius
// norm, not by its largest entry.  Kept beside the form above because the two stop after different sweeps: the
// eigensolver's Ritz values, and with them every certificate's bits, follow this one.
inline void jacobi_eig(int m, std::vector<double> A, std::vector<double> &Z, std::vector<double> &w) {
  Z.assign((size_t)m * m, 0.0);
  for (int i = 0; i < m; ++i) Z[(size_t)i * m + i] = 1;
  for (int sweep = 0; sweep < 100; ++sweep) {
    double off = 0, dg = 0;
    for (int i = 0; i < m; ++i) {
      dg += A[(size_t)i * m + i] * A[(size_t)i * m + i];
      for (int j = i + 1; j < m; ++j) off += A[(size_t)i * m + j] * A[(size_t)i * m + j];
    }
    if (off == 0 || off <= 1e-32 * (dg + off)) break;
    for (int p = 0; p < m - 1; ++p)
      for (int q = p + 1; q < m; ++q) {
        const double apq = A[(size_t)p * m + q];
        if (apq == 0) continue;
        const double zeta = (A[(size_t)q * m + q] - A[(size_t)p * m + p]) / (2 * apq);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1 + zeta * zeta));
        const double c = 1 / std::sqrt(1 + t * t), s = c * t;
        for (int k = 0; k < m; ++k) {
          const double akp = A[(size_t)k * m + p], akq = A[(size_t)k * m + q];
          A[(size_t)k * m + p] = c * akp - s * akq;
          A[(size_t)k * m + q] = s * akp + c * akq;
        }
        for (int k = 0; k < m; ++k) {
          const double apk = A[(size_t)p * m + k], aqk = A[(size_t)q * m + k];
          A[(size_t)p * m + k] = c * apk - s * aqk;
          A[(size_t)q * m + k] = s * apk + c * aqk;
          const double zkp = Z[(size_t)k * m + p], zkq = Z[(size_t)k * m + q];
          Z[(size_t)k * m + p] = c * zkp - s * zkq;
          Z[(size_t)k * m + q] = s * zkp + c * zkq;
        }
      }
  }
  w.resize(m);
  for (int i = 0; i < m; ++i) w[i] = A[(size_t)i * m + i];
}

// The eigenvalues of G (n x n, symmetric, column-major) in descending order in w, their eigenvectors as the columns of
// V (n x n, column-major) in that order.  Equal eigenvalues keep the order of their index (a stable sort on the value
// alone), so the choice among ties is the same call after call.
inline void sym_eig_descending(int n, const double *G, std::vector<double> *w, std::vector<double> *V) {
  std::vector<double> A(G, G + (size_t)n * n), U;
  jacobi_eig(n, A, U);
  std::vector<int> order((size_t)n);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(),
                   [&](int a, int b) { return A[(size_t)a * n + a] > A[(size_t)b * n + b]; });
  w->resize((size_t)n);
  V->resize((size_t)n * n);
  for (int j = 0; j < n; ++j) {
    (*w)[(size_t)j] = A[(size_t)order[(size_t)j] * n + order[(size_t)j]];
    std::copy(U.begin() + (size_t)order[(size_t)j] * n, U.begin() + (size_t)(order[(size_t)j] + 1) * n,
              V->begin() + (size_t)j * n);
  }
}

// projectSolutionRASLAM's reflection rule (ref src/DCORA_utils.cpp:2016): most rotation blocks are improper
inline bool reflect_rule(int positive_dets, int n) { return positive_dets < n / 2; }

}  // namespace dcora
