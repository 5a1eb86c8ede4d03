// The thick-restart Lanczos recurrence for one largest-magnitude eigenpair, host only: the projected matrix H of a
// cycle, its eigenproblem, the convergence test and what a restart keeps.  Convergence test and the number of Ritz
// vectors kept per restart follow Spectra's SymEigsSolver for nev = 1:
// |beta_m y_m| < tol max(eps^(2/3), |theta|), keep = ncv / 2.
// It knows nothing of where the basis lives: the owner of the basis (DeviceLanczos in cert.hip, plain arrays in
// tests/cpp/lanczos_restart.cpp) runs step j -- operator on basis vector j, two passes of projection against vectors
// 0 .. j, the norm of the remainder -- hands the coefficients in, and applies the combination coefficients it gets back.
#pragma once
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "small_eig.h"

namespace dcora {

// a new direction whose norm is below this fraction of |S v_j| is rounding noise of the orthogonalisation, not a
// direction: the Krylov space is exhausted (an invariant subspace) and the basis continues with a fresh vector
constexpr double kLanczosDead = 1e-10;

struct LanczosRestart {
  int order = 0;  // of the whole problem
  int m = 0;      // basis vectors of a cycle
  int keep = 0;   // Ritz vectors a restart keeps
  int k = 0;      // first step of the coming cycle: 0, then keep
  double beta = 0;  // norm of the remainder of the last step taken (0: that direction was dead)
  std::vector<double> H, Z, th;  // m x m projected matrix; its eigenvectors (columns of the row-major Z) and values
  std::vector<int> ord;          // Ritz values by decreasing magnitude

  LanczosRestart(int ncv, int order_)
      : order(order_), m(std::min(ncv, order_)), keep(std::max(1, std::min(m - 1, m / 2))), H((size_t)m * m, 0.0),
        ord((size_t)std::max(m, 0)) {}

  // column j of H from the two passes' coefficients against vectors 0 .. j
  void take_coefficients(int j, const double *pass0, const double *pass1) {
    for (int i = 0; i <= j; ++i) {
      const double h = pass0[i] + pass1[i];
      H[(size_t)i * m + j] = h;
      H[(size_t)j * m + i] = h;
    }
  }
  // Step j as its owner measured it: b2 = |remainder|^2.  -> false when the remainder is no direction (relative to
  // |S v_j|^2 = b2 + the squared coefficients taken out, or vanishing outright): beta = 0, the owner continues with a
  // fresh direction as vector j + 1
  bool take_step(int j, const double *pass0, const double *pass1, double b2) {
    take_coefficients(j, pass0, pass1);
    beta = std::sqrt(b2);
    double h2 = 0;
    for (int i = 0; i <= j; ++i) h2 += H[(size_t)i * m + j] * H[(size_t)i * m + j];
    if (!(beta > kLanczosDead * std::sqrt(h2 + b2)) || beta < 1e-300) {
      beta = 0;
      return false;
    }
    return true;
  }
  // Step j whose owner applied the same test itself (k_lanczos_next) and found a direction of norm beta_j
  void take_live_step(int j, const double *pass0, const double *pass1, double beta_j) {
    take_coefficients(j, pass0, pass1);
    beta = beta_j;
  }

  // end of a cycle: the Ritz pairs of H, by magnitude; -> the residual estimate of the first passes Spectra's test
  bool solve(double tol) {
    jacobi_eig(m, H, Z, th);
    std::iota(ord.begin(), ord.end(), 0);
    std::sort(ord.begin(), ord.end(), [&](int a, int b) { return std::fabs(th[a]) > std::fabs(th[b]); });
    const double eps23 = std::pow(2.220446049250313e-16, 2.0 / 3.0);
    const double resid = std::fabs(beta * Z[(size_t)(m - 1) * m + ord[0]]);
    return resid < tol * std::max(eps23, std::fabs(th[ord[0]]));
  }
  double theta() const { return th[ord[0]]; }
  bool spans_everything() const { return m == order; }  // the Ritz pairs are the eigenpairs: nothing to iterate on

  // `count` columns of m coefficients, column-major: basis vectors 0 .. m - 1 combined by column c give Ritz vector
  // ord[c].  count = 1: the eigenvector returned; count = keep: the vectors a restart keeps
  std::vector<double> ritz_coefficients(int count) const {
    std::vector<double> C((size_t)m * count);
    for (int c = 0; c < count; ++c)
      for (int i = 0; i < m; ++i) C[(size_t)c * m + i] = Z[(size_t)i * m + ord[c]];
    return C;
  }
  // thick restart: the kept Ritz vectors become vectors 0 .. keep - 1 (H diagonal on them), vector m becomes vector keep
  void restart() {
    std::fill(H.begin(), H.end(), 0.0);
    for (int c = 0; c < keep; ++c) H[(size_t)c * m + c] = th[ord[c]];
    k = keep;
  }
};

}  // namespace dcora
