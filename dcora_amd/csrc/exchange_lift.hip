// The Riemannian staircase's step across the ranks of a job (see exchange.h, Exchange::lift): escapeSaddle's search
// (ref src/QuadraticProblem.cpp:138-234, stated once in escape_rule.h) over trial points every rank forms for the agents
// it hosts, the level change of examples/MultiRobotExample.cpp:352-366 without leaving the job.
#include "exchange.h"

#include <chrono>
#include <cmath>
#include <numeric>

#include "escape_rule.h"

namespace dcora {

int Exchange::lift(double theta, const double *v, const dcora_lift_params &p, int *escaped, double *info8) {
  using clock = std::chrono::steady_clock;
  const auto t0 = clock::now();
  auto ms_total = [&] { return std::chrono::duration<double, std::milli>(clock::now() - t0).count(); };
  *escaped = 0;
  if (info8) std::fill(info8, info8 + 8, 0.0);
  SessionCore &s = *s_;
  // ---- refusals: the same on every rank (every rank is handed the same arguments), nothing touched ----
  if (s.r + 1 > kMaxRank) return usage("lift: the job is at rank 16, the largest the kernels are built for", DCORA_ERR_BAD_ARG);
  if (!lift_args_finite(theta, v, s.num_cols(), p.gradient_tolerance, p.preconditioned_gradient_tolerance))
    return usage("lift: v must be k finite numbers, theta and the tolerances finite", DCORA_ERR_BAD_ARG);
  if (s.r + 1 > r_cap_)
    return usage("lift: rank " + std::to_string(s.r + 1) + " is beyond what the job's segment and halo slots hold (" +
                     std::to_string(r_cap_) + "); reserve the ranks to come before the exchange is created "
                     "(dcora_rbcd_reserve_rank / dcora_ra_rbcd_reserve_rank, or dcora_rbcd_create_robust_ranks_reserved "
                     "/ dcora_ra_rbcd_create_robust_ranks_reserved)",
                 DCORA_ERR_UNSUPPORTED);
  const int r_new = s.r + 1;
  std::vector<int> all((size_t)R_);
  std::iota(all.begin(), all.end(), 0);
  // a step failed on this rank: its problems go back to r, and the ranks that wait for it learn so (`failed`)
  auto give_up = [&](int rc) {
    s.lift_trial_abort();
    if (hdr_) hdr_->failed.store(1);
    if (info8) info8[7] = ms_total();
    return rc;
  };
  int rc = s.lift_trial_begin(v);
  if (rc) return give_up(rc);
  // one trial point on every rank: the hosted blocks at alpha, then everybody's public columns (r + 1 rows) as in a round
  auto point = [&](double alpha) -> int {
    double *mirror = nullptr;
    int c = s.lift_trial_point(alpha, &mirror);
    if (!c) c = post_arr(all.data(), R_, r_new, mirror);
    if (!c) c = wait_arr(all.data(), R_, r_new, mirror);
    return c;
  };
  // ... and its scalars {2 f, |rgrad|^2, |P grad|^2}: this rank's sums in agent order, then the ranks' in rank order
  auto scalars = [&](double s3[3]) -> int {
    const int c = s.lift_trial_scalars(s3);
    return c ? c : allreduce_sum(s3, 3);
  };
  double s3[3] = {0, 0, 0};
  rc = point(0.0);  // f([X; 0]): the evaluation of the current iterate, through the trials' own path
  if (!rc) rc = scalars(s3);
  if (rc) return give_up(rc);
  const double FX = 0.5 * s3[0];
  if (info8) info8[2] = info8[3] = FX;
  EscapeSearch search(theta, p.gradient_tolerance, p.preconditioned_gradient_tolerance, p.is_second_order != 0, FX);
  bool accepted = false;
  double alpha_acc = 0, f_acc = FX;
  while (search.more()) {
    rc = point(search.alpha);
    if (!rc) rc = scalars(s3);
    if (rc) return give_up(rc);
    const double ft = 0.5 * s3[0];
    accepted = search.offer(ft, std::sqrt(s3[1]), std::sqrt(s3[2]));
    if (info8) info8[0] = (double)search.trials();
    if (accepted) {
      alpha_acc = search.alphas.back();
      f_acc = ft;
      break;
    }
  }
  if (!accepted) {
    const int idx = search.fallback();
    if (idx >= 0) {  // the trial of least f once more: its blocks into the trial mirror, its public columns exchanged
      rc = point(search.alphas[(size_t)idx]);
      if (rc) return give_up(rc);
      accepted = true;
      alpha_acc = search.alphas[(size_t)idx];
      f_acc = search.fvals[(size_t)idx];
    }
  }
  if (!accepted) {  // no escape: the session's mirror, sequences and counters were never touched
    s.lift_trial_abort();
    if (info8) info8[7] = ms_total();
    return DCORA_OK;
  }
  // every rank's mirror becomes the accepted point at once, as Exchange::set_X does
  rc = barrier();
  if (rc) {
    s.lift_trial_abort();
    return rc;
  }
  double redim_ms = 0;
  rc = s.lift_trial_commit(&redim_ms);
  if (rc) return give_up(rc);
  rc = barrier();
  if (rc) return rc;
  *escaped = 1;
  if (info8) info8[1] = alpha_acc, info8[3] = f_acc, info8[6] = redim_ms, info8[7] = ms_total();
  return DCORA_OK;
}

}  // namespace dcora
