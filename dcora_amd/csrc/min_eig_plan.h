// The plan of computeMinimumEigenPair (ref src/DCORA_utils.cpp:1809-1896), host only: which Lanczos runs are made with
// which parameters, what is decided after the first, how a run's eigenvalue becomes the matrix's, and the shifts of the
// shift-and-invert fallback.  Its clients supply the runs: device_min_eig (cert.hip) on one device, with the fallback;
// Exchange::cert_min_eigenpair (exchange_cert.hip) collectively, handing over to rank 0 where the plan says fallback.
#pragma once
#include <algorithm>

namespace dcora {

// the spectrum-shifted run would have to resolve min_eig_tol on a spectrum of width lambda_lm: below this ratio a
// 20-vector Krylov space is given no chance and the shift-and-invert fallback is taken at once
inline bool min_eig_shifted_run_hopeless(double min_eig_tol, double lambda_lm) { return min_eig_tol / lambda_lm < 1e-8; }

struct MinEigPlan {
  // The "hopeless" shortcut past the spectrum-shifted run (tiers.pyfg: the landmark every pose ranges to puts
  // lambda_lm at 2e6, the ratio at 5e-10; the reference's run spends its 1000 restarts -- 10 020 matvecs -- and then
  // takes the fallback anyway): taken whenever the ratio says so, or only when the caller asks for it as well
  enum class Shortcut { always, when_asked };
  // a first run that did not converge: an error, or the fallback's business (it makes that run again, on one device)
  enum class OnFailedFirst { error, fallback };
  Shortcut shortcut;
  OnFailedFirst on_failed_first;

  // one Lanczos run for the largest-magnitude eigenpair of S - shift I
  struct Run {
    double shift, tol;
    int ncv, maxit;
  };
  static Run first_run(int ncv, int maxit) { return {0.0, 1e-4, ncv, maxit}; }
  // started from min_eig_second_start; its eigenvalue + 2 lambda_lm is the smallest of S
  static Run shifted_run(double lambda_lm, double tol, int ncv, int maxit) {
    return {2 * lambda_lm, tol / lambda_lm, ncv, maxit};
  }
  static double shifted_eigenvalue(double lambda, double lambda_lm) { return lambda + 2 * lambda_lm; }
  // on (S - sigma I)^-1 (ref :1751-1805); mu, its largest eigenvalue, gives sigma + 1 / mu
  static Run inverse_run(int ncv) { return {0.0, 1e-10, ncv, 1000}; }
  static double inverse_eigenvalue(double mu, double sigma) { return sigma + 1.0 / mu; }

  enum class AfterFirst {
    done_negative,      // the largest-magnitude eigenvalue is negative: it is the smallest
    done_zero,          // S = 0: every vector is an eigenvector of the eigenvalue 0
    shifted,            // make the spectrum-shifted run
    fallback_hopeless,  // the shortcut: straight to the fallback
    failed_first,       // the first run did not converge: see on_failed_first
  };
  AfterFirst after_first_run(bool ok, double lambda_lm, double tol, bool shortcut_asked) const {
    if (!ok) return AfterFirst::failed_first;
    if (lambda_lm < 0) return AfterFirst::done_negative;
    if (lambda_lm == 0) return AfterFirst::done_zero;
    if ((shortcut == Shortcut::always || shortcut_asked) && min_eig_shifted_run_hopeless(tol, lambda_lm))
      return AfterFirst::fallback_hopeless;
    return AfterFirst::shifted;
  }
  bool goes_to_fallback(AfterFirst a) const {
    return a == AfterFirst::fallback_hopeless || (a == AfterFirst::failed_first && on_failed_first == OnFailedFirst::fallback);
  }
};

// The fallback's attempts, one after the other: sigma = -10, halved after every attempt whose run on the inverse did not
// converge, nine times, the tenth at the floor -2 tol (which also holds earlier).  The factorisation is a Cholesky (the
// reference's Spectra run factors S - sigma I by a sparse LU, which exists for any shift): S - sigma I must be positive
// definite, i.e. sigma < lambda_min.  When the very first shift is refused, lambda_min lies below it: the shift moves
// OUTWARD by factors of ten until the matrix factors -- not beyond 2 lambda_lm + 10, below which nothing of the spectrum
// can lie -- and the first attempt that factors is the last.  A refusal after an inward move is an attempt like any
// other.  Where the shortcut skipped the spectrum-shifted run and the ladder delivered nothing, that run is made last.
class ShiftLadder {
 public:
  enum class Outcome { not_pd, factored_but_not_converged, converged };
  enum class Step { invert, late_shifted, end };

  ShiftLadder(double lambda_lm, double tol, bool shortcut_taken)
      : lambda_lm_(lambda_lm), tol_(tol), late_(shortcut_taken) {}
  Step step() const { return step_; }
  double sigma() const { return sigma_; }
  // what follows the attempt at step() (after late_shifted every outcome ends the ladder)
  Step next(Outcome o) {
    if (step_ != Step::invert || o == Outcome::converged) return step_ = Step::end;
    if (o == Outcome::not_pd && (i_ == 0 || outward_)) {
      outward_ = true;
      if (-sigma_ > 2.0 * lambda_lm_ + 10.0) return leave();  // (cannot happen in exact arithmetic)
      sigma_ *= 10.0;
      return ++i_ < kMaxAttempts ? step_ : leave();
    }
    if (outward_ || i_ >= 9) return leave();
    sigma_ /= 2;
    if (i_ == 8 || sigma_ > -2 * tol_) sigma_ = -2 * tol_;
    ++i_;
    return step_;
  }

 private:
  static constexpr int kMaxAttempts = 24;
  Step leave() { return step_ = late_ ? Step::late_shifted : Step::end; }
  double lambda_lm_, tol_, sigma_ = -10.0;
  bool late_, outward_ = false;
  int i_ = 0;
  Step step_ = Step::invert;
};

}  // namespace dcora
