// Unit test of dcora_amd/csrc/lanczos_restart.h -- the thick-restart recurrence of the certificate's eigensolver -- with
// a basis in plain arrays: the per-step form of DeviceLanczos (operator, two passes of projection, the norm, a fresh
// seeded direction where the remainder is dead) on diagonal and tridiagonal matrices whose eigenvalues are known; built
// with g++ under ASan + UBSan by tests/test_min_eig_plan_cpu.py.  Prints "ok <n>" per passed case and nothing that says
// FAILED.  Every eigenvalue is held to the known one within 2 tol max(eps^(2/3), |theta|) at tol = 1e-8: the Ritz residual
// the recurrence tests bounds the error by tol |theta|, the factor 2 covers the estimated against the true residual, and
// rounding at these orders is five digits below.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <vector>

#include "lanczos_restart.h"

namespace {

using Matvec = std::function<void(const double *x, double *y)>;

struct Result {
  bool ok = false;
  double lambda = 0;
  std::vector<double> v;
  long matvecs = 0;
  int restarts = 0;
};

double u01(uint64_t &s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(s >> 11) * (1.0 / 9007199254740992.0);
}

double dot(int n, const double *a, const double *b) {
  double s = 0;
  for (int i = 0; i < n; ++i) s += a[i] * b[i];
  return s;
}

// h = V[:, 0:nv]^T w, w -= V h
void orthogonalise(int n, int nv, const std::vector<double> &V, std::vector<double> &w, double *h) {
  for (int i = 0; i < nv; ++i) h[i] = dot(n, &V[(size_t)i * n], w.data());
  for (int i = 0; i < nv; ++i)
    for (int t = 0; t < n; ++t) w[(size_t)t] -= V[(size_t)i * n + t] * h[i];
}

Result largest_magnitude(int n, const Matvec &A, double shift, int ncv, int maxit, double tol, uint64_t seed) {
  Result out;
  dcora::LanczosRestart T(ncv, n);
  const int m = T.m;
  std::vector<double> V((size_t)n * (m + 1)), w((size_t)n), tmp((size_t)n * m);
  double nn = 0;
  for (int t = 0; t < n; ++t) V[(size_t)t] = u01(seed) - 0.5, nn += V[(size_t)t] * V[(size_t)t];
  for (int t = 0; t < n; ++t) V[(size_t)t] /= std::sqrt(nn);
  for (int it = 0; it <= maxit; ++it) {
    for (int j = T.k; j < m; ++j) {
      const double *vj = &V[(size_t)j * n];
      double *next = &V[(size_t)(j + 1) * n];
      A(vj, w.data());
      for (int t = 0; t < n; ++t) w[(size_t)t] -= shift * vj[t];
      ++out.matvecs;
      double h[2][32];
      for (int pass = 0; pass < 2; ++pass) orthogonalise(n, j + 1, V, w, h[pass]);
      if (T.take_step(j, h[0], h[1], dot(n, w.data(), w.data()))) {
        for (int t = 0; t < n; ++t) next[t] = w[(size_t)t] / T.beta;
      } else {  // a fresh direction (in order 1 there is none: the vector is not used, the basis spans everything)
        uint64_t s = seed + 7919 * (uint64_t)(j + 1);
        for (int t = 0; t < n; ++t) w[(size_t)t] = u01(s) - 0.5;
        for (int pass = 0; pass < 2; ++pass) orthogonalise(n, j + 1, V, w, h[0]);
        const double b = std::sqrt(dot(n, w.data(), w.data()));
        for (int t = 0; t < n; ++t) next[t] = b > 0 ? w[(size_t)t] / b : 0.0;
      }
    }
    const bool conv = T.solve(tol);
    const bool last = conv || it == maxit || T.spans_everything();
    const int count = last ? 1 : T.keep;
    const std::vector<double> C = T.ritz_coefficients(count);
    for (int c = 0; c < count; ++c)
      for (int t = 0; t < n; ++t) {
        double s = 0;
        for (int i = 0; i < m; ++i) s += V[(size_t)i * n + t] * C[(size_t)c * m + i];
        tmp[(size_t)c * n + t] = s;
      }
    if (last) {
      out.ok = conv || T.spans_everything();
      out.lambda = T.theta();
      out.v.assign(tmp.begin(), tmp.begin() + n);
      const double vn = std::sqrt(dot(n, out.v.data(), out.v.data()));
      for (double &x : out.v) x /= vn;
      return out;
    }
    std::copy(tmp.begin(), tmp.begin() + (size_t)n * T.keep, V.begin());
    std::copy(V.begin() + (size_t)m * n, V.begin() + (size_t)(m + 1) * n, V.begin() + (size_t)T.keep * n);
    T.restart();
    ++out.restarts;
  }
  return out;
}

Matvec diagonal(const std::vector<double> &d) {
  return [d](const double *x, double *y) {
    for (size_t i = 0; i < d.size(); ++i) y[i] = d[i] * x[i];
  };
}

const double kTol = 1e-8;
const double kEps23 = std::pow(2.220446049250313e-16, 2.0 / 3.0);
int g_failed = 0, g_case = 0;

// `want`: the eigenvalue of (A - shift I) of largest magnitude
void check(const char *name, int n, const Matvec &A, double shift, int ncv, int maxit, double want, int min_restarts = 0) {
  const Result r = largest_magnitude(n, A, shift, ncv, maxit, kTol, 12345);
  const dcora::LanczosRestart T(ncv, n);
  const long budget = T.m + (long)maxit * (T.m - T.keep);
  double vn = 0;
  for (double x : r.v) vn += x * x;
  const double bound = 2 * kTol * std::max(kEps23, std::fabs(want));
  std::printf("%s: converged %d lambda %.17g (want %.17g, |difference| %.3g, bound %.3g) | |v| - 1 | %.3g matvecs %ld (budget %ld) "
              "restarts %d\n", name, (int)r.ok, r.lambda, want, std::fabs(r.lambda - want), bound, std::fabs(std::sqrt(vn) - 1),
              r.matvecs, budget, r.restarts);
  const bool pass = r.ok && std::fabs(r.lambda - want) <= bound && std::fabs(std::sqrt(vn) - 1) <= 1e-12 &&
                    r.matvecs <= budget && r.restarts >= min_restarts;
  if (pass)
    std::printf("ok %d\n", ++g_case);
  else
    std::printf("FAILED %s\n", name), ++g_failed;
}

}  // namespace

int main() {
  std::vector<double> three(401, 1.0);
  three[0] = -2.0;
  for (int i = 201; i < 401; ++i) three[(size_t)i] = 3.0;
  check("three eigenvalues", 401, diagonal(three), 0.0, 20, 1000, 3.0);
  check("three eigenvalues, spectrum shifted by 6", 401, diagonal(three), 6.0, 20, 1000, -8.0);
  // the Krylov space is exhausted at step 1; the remainder is rounding noise and must be called dead by the relative test
  check("2 I", 200, diagonal(std::vector<double>(200, 2.0)), 0.0, 20, 1000, 2.0);
  check("zero", 200, diagonal(std::vector<double>(200, 0.0)), 0.0, 20, 1000, 0.0);
  check("order 1", 1, diagonal({-0.75}), 0.0, 20, 1000, -0.75);
  check("order below ncv", 7, diagonal({1, 2, 3, 4, 5, 6, -7}), 0.0, 20, 1000, -7.0);
  const int n = 300;
  const Matvec laplacian = [n](const double *x, double *y) {
    for (int i = 0; i < n; ++i) y[i] = 2 * x[i] - (i > 0 ? x[i - 1] : 0.0) - (i + 1 < n ? x[i + 1] : 0.0);
  };
  check("1-D Laplacian, ncv 6", n, laplacian, 0.0, 6, 20000, 2.0 - 2.0 * std::cos(n * M_PI / (n + 1)), 3);
  return g_failed ? 1 : 0;
}
