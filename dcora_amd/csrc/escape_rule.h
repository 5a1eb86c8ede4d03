// The line search of escapeSaddle (ref src/QuadraticProblem.cpp:161-233), stated once, without HIP: the first step
// length and its halving, the first trial that lowers f with both gradient norms above their tolerances, else the trial
// of least f if it lowers f, else no escape.  Its callers supply the numbers of each trial: the whole-graph problem
// (DeviceProblem::escape_saddle_dev, SessionCore::lift) and the ranks of a job together (Exchange::lift), where every
// number offered is a sum over the ranks in rank order, so that every rank takes the same branch.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

namespace dcora {

struct EscapeSearch {
  static constexpr double kAlphaMin = 1e-6;
  double gtol, pgtol, FX, alpha;
  std::vector<double> alphas, fvals;
  // ref :165-169: SE-Sync's second-order step when asked for, else Algorithm 7 of the DC2-PGO report
  EscapeSearch(double theta, double gtol_, double pgtol_, bool second_order, double f_of_X_plus)
      : gtol(gtol_), pgtol(pgtol_), FX(f_of_X_plus),
        alpha(second_order ? std::max(16 * kAlphaMin, 100 * gtol_ / std::fabs(theta)) : 1.0) {}
  bool more() const { return alpha >= kAlphaMin; }  // a trial at `alpha` is due
  int trials() const { return (int)alphas.size(); }
  // the trial at `alpha`: f, |rgrad| and |P rgrad| there.  True: accepted (ref :181-204); false: alpha is halved
  bool offer(double f, double gradnorm, double pgradnorm) {
    alphas.push_back(alpha);
    fvals.push_back(f);
    if (f < FX && gradnorm > gtol && pgradnorm > pgtol) return true;
    alpha /= 2;
    return false;
  }
  // no trial was accepted (ref :208-233): the trial of least f (the first of equals) if it lowers f, else -1
  int fallback() const {
    if (fvals.empty()) return -1;
    const size_t idx = std::min_element(fvals.begin(), fvals.end()) - fvals.begin();
    return fvals[idx] < FX ? (int)idx : -1;
  }
};

// what a lift checks of its arguments before anything is touched: the same on a session and on every rank of a job
inline bool lift_args_finite(double theta, const double *v, long k, double gtol, double pgtol) {
  bool finite = v && std::isfinite(theta) && std::isfinite(gtol) && std::isfinite(pgtol);
  for (long j = 0; finite && j < k; ++j) finite = std::isfinite(v[j]);
  return finite;
}

}  // namespace dcora
