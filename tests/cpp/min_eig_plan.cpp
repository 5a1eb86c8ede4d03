// Unit test of dcora_amd/csrc/min_eig_plan.h -- the plan of computeMinimumEigenPair: the runs' parameters, the decision
// after the first run under both policies, the eigenvalue corrections and the shift ladder of the fallback; built with
// g++ under ASan + UBSan by tests/test_min_eig_plan_cpu.py.  The ladder's shift sequences are literals derived by hand
// from the loop device_min_eig held before the plan was stated (sigma = -10; a refusal at the first shift or after an
// outward move: stop beyond 2 lambda_lm + 10, else times ten; otherwise stop when outward or after the tenth attempt,
// else halve, with the floor -2 tol, which the tenth attempt takes in any case; 24 attempts at most).  Prints "ok <n>"
// per passed group and nothing that says FAILED.
#include <cstdio>
#include <vector>

#include "min_eig_plan.h"

using dcora::MinEigPlan;
using dcora::ShiftLadder;
using After = MinEigPlan::AfterFirst;
using Outcome = ShiftLadder::Outcome;
using Step = ShiftLadder::Step;

#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                  \
    }                                                            \
  } while (0)

namespace {
// the shifts attempted when attempt i ends with outcomes[i] (the last outcome repeats), and the step that ends them
std::vector<double> shifts(ShiftLadder L, const std::vector<Outcome> &outcomes, Step *last) {
  std::vector<double> s;
  for (size_t i = 0; L.step() == Step::invert && i < 100; ++i) {
    s.push_back(L.sigma());
    L.next(outcomes[std::min(i, outcomes.size() - 1)]);
  }
  *last = L.step();
  return s;
}
}  // namespace

int main() {
  int group = 0;
  const MinEigPlan one{MinEigPlan::Shortcut::always, MinEigPlan::OnFailedFirst::error};         // device_min_eig's
  const MinEigPlan job{MinEigPlan::Shortcut::when_asked, MinEigPlan::OnFailedFirst::fallback};  // cert_min_eigenpair's

  // 1. the runs' parameters and the eigenvalue corrections
  {
    const MinEigPlan::Run a = MinEigPlan::first_run(20, 1000);
    CHECK(a.shift == 0.0 && a.tol == 1e-4 && a.ncv == 20 && a.maxit == 1000);
    const MinEigPlan::Run b = MinEigPlan::shifted_run(250.0, 1e-3, 12, 77);
    CHECK(b.shift == 500.0 && b.tol == 1e-3 / 250.0 && b.ncv == 12 && b.maxit == 77);
    const MinEigPlan::Run c = MinEigPlan::inverse_run(20);
    CHECK(c.shift == 0.0 && c.tol == 1e-10 && c.ncv == 20 && c.maxit == 1000);
    CHECK(MinEigPlan::shifted_eigenvalue(-503.5, 250.0) == -3.5);
    CHECK(MinEigPlan::inverse_eigenvalue(0.125, -10.0) == -2.0);  // mu = 1 / (lambda - sigma)
    std::printf("ok %d\n", ++group);
  }
  // 2. the decision after the first run, both policies, the shortcut asked for and not
  {
    for (const MinEigPlan *p : {&one, &job})
      for (bool asked : {false, true}) {
        CHECK(p->after_first_run(false, 5.0, 1e-3, asked) == After::failed_first);
        CHECK(p->after_first_run(false, -5.0, 1e-3, asked) == After::failed_first);  // (not converged: the sign says nothing)
        CHECK(p->after_first_run(true, -5.0, 1e-3, asked) == After::done_negative);
        CHECK(p->after_first_run(true, -4e9, 1e-3, asked) == After::done_negative);  // (before any ratio is looked at)
        CHECK(p->after_first_run(true, 0.0, 1e-3, asked) == After::done_zero);
        CHECK(p->after_first_run(true, 5.0, 1e-3, asked) == After::shifted);
        CHECK(p->after_first_run(true, 0.99e5, 1e-3, asked) == After::shifted);  // ratio 1.01e-8: not hopeless
      }
    // ratio 5e-10 (tiers.pyfg) and just below 1e-8
    for (double lm : {2e6, 1.01e5}) {
      CHECK(one.after_first_run(true, lm, 1e-3, false) == After::fallback_hopeless);
      CHECK(one.after_first_run(true, lm, 1e-3, true) == After::fallback_hopeless);
      CHECK(job.after_first_run(true, lm, 1e-3, false) == After::shifted);
      CHECK(job.after_first_run(true, lm, 1e-3, true) == After::fallback_hopeless);
    }
    for (After a : {After::done_negative, After::done_zero, After::shifted}) CHECK(!one.goes_to_fallback(a) && !job.goes_to_fallback(a));
    CHECK(one.goes_to_fallback(After::fallback_hopeless) && job.goes_to_fallback(After::fallback_hopeless));
    CHECK(!one.goes_to_fallback(After::failed_first) && job.goes_to_fallback(After::failed_first));
    std::printf("ok %d\n", ++group);
  }
  Step last;
  // 3. never converging at tol = 1e-3: nine halvings, the tenth attempt at the floor, then the end
  {
    const std::vector<double> want = {-10, -5, -2.5, -1.25, -0.625, -0.3125, -0.15625, -0.078125, -0.0390625, -0.002};
    CHECK(shifts(ShiftLadder(100.0, 1e-3, false), {Outcome::factored_but_not_converged}, &last) == want);
    CHECK(last == Step::end);
    // ... after the shortcut the run it skipped comes last, and whatever that gives ends the ladder
    ShiftLadder L(2e6, 1e-3, true);
    for (int i = 0; i < 10; ++i) CHECK(L.step() == Step::invert && L.next(Outcome::factored_but_not_converged) != Step::end);
    CHECK(L.step() == Step::late_shifted && L.next(Outcome::factored_but_not_converged) == Step::end);
    std::printf("ok %d\n", ++group);
  }
  // 4. the floor holds before the tenth attempt where tol is large: -10, -5, then -2 tol until the tenth
  {
    const std::vector<double> want = {-10, -5, -4, -4, -4, -4, -4, -4, -4, -4};
    CHECK(shifts(ShiftLadder(100.0, 2.0, false), {Outcome::factored_but_not_converged}, &last) == want && last == Step::end);
    std::printf("ok %d\n", ++group);
  }
  // 5. refused at the first shift under lambda_lm = 4e6: outward by tens; the first shift that factors is the last
  //    attempt whether or not its run converges; refused throughout, the stop beyond 2 lambda_lm + 10 = 8 000 010
  {
    const std::vector<double> to_1e3 = {-10, -100, -1000};
    CHECK(shifts(ShiftLadder(4e6, 1e-3, false), {Outcome::not_pd, Outcome::not_pd, Outcome::converged}, &last) == to_1e3);
    CHECK(last == Step::end);
    CHECK(shifts(ShiftLadder(4e6, 1e-3, true), {Outcome::not_pd, Outcome::not_pd, Outcome::factored_but_not_converged}, &last) ==
          to_1e3);
    CHECK(last == Step::late_shifted);
    const std::vector<double> all = {-10, -100, -1000, -1e4, -1e5, -1e6, -1e7};
    CHECK(shifts(ShiftLadder(4e6, 1e-3, true), {Outcome::not_pd}, &last) == all && last == Step::late_shifted);
    CHECK(shifts(ShiftLadder(4e6, 1e-3, false), {Outcome::not_pd}, &last) == all && last == Step::end);
    // a spectrum so wide that the bound is never reached: the 24 attempts
    CHECK(shifts(ShiftLadder(1e40, 1e-3, false), {Outcome::not_pd}, &last).size() == 24 && last == Step::end);
    std::printf("ok %d\n", ++group);
  }
  // 6. a refusal after an inward move does not turn outward: it is halved like a run that did not converge
  {
    const std::vector<double> want = {-10, -5, -2.5, -1.25};
    CHECK(shifts(ShiftLadder(100.0, 1e-3, false),
                 {Outcome::factored_but_not_converged, Outcome::not_pd, Outcome::not_pd, Outcome::converged}, &last) == want);
    CHECK(last == Step::end);
    std::printf("ok %d\n", ++group);
  }
  // 7. converged at the first shift: one attempt, and no late run even after the shortcut
  {
    CHECK(shifts(ShiftLadder(2e6, 1e-3, true), {Outcome::converged}, &last) == std::vector<double>{-10} && last == Step::end);
    std::printf("ok %d\n", ++group);
  }
  return 0;
}
