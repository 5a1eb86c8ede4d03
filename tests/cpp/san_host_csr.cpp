// pattern_of / scatter_on_pattern (host_sparse.h) under AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_host_sanitizers.py): identity on the own pattern, explicit zeros on a wider pattern, refusal when an
// entry falls outside the pattern or the shapes differ.  Prints "ok" lines; any failed check ends with status 1.
#include "host_sparse.h"
#include <cstdio>
using namespace dcora;
static int failed = 0;
static void check(bool c, const char *what) {
  printf("%s %s\n", c ? "ok" : "FAILED", what);
  failed += !c;
}
int main() {
  // A = [1 0 2; 0 3 0; 4 0 5], 3 x 4 with an empty last column
  const HostCsr A = csr_from_coo(3, 4, {0, 0, 1, 2, 2}, {0, 2, 1, 0, 2}, {1, 2, 3, 4, 5});
  const HostCsr Pa = pattern_of(A);
  check(Pa.n == 3 && Pa.ncols == 4 && Pa.rp == A.rp && Pa.ci == A.ci && Pa.v.empty(), "pattern_of keeps rp / ci only");
  HostCsr S;
  check(scatter_on_pattern(A, Pa, &S) && S.n == A.n && S.ncols == A.ncols && S.rp == A.rp && S.ci == A.ci && S.v == A.v,
        "identity on the own pattern");
  // a wider pattern: every entry of A and (0, 1), (1, 3), (2, 1)
  const HostCsr W = csr_from_coo(3, 4, {0, 0, 0, 1, 1, 2, 2, 2}, {0, 1, 2, 1, 3, 0, 1, 2}, {9, 9, 9, 9, 9, 9, 9, 9});
  check(scatter_on_pattern(A, pattern_of(W), &S) && S.rp == W.rp && S.ci == W.ci &&
            S.v == std::vector<double>({1, 0, 2, 3, 0, 4, 0, 5}),
        "explicit zeros on a wider pattern");
  // a matrix without entries scatters to all zeros
  const HostCsr Z = csr_from_coo(3, 4, {}, {}, {});
  check(scatter_on_pattern(Z, Pa, &S) && S.v == std::vector<double>(5, 0.0), "empty matrix gives zeros");
  // refusals: an entry outside the pattern (last in its row, first in its row, in an empty row), other shapes
  check(!scatter_on_pattern(W, Pa, &S), "entry outside the pattern refused");
  check(!scatter_on_pattern(csr_from_coo(3, 4, {2}, {3}, {1}), Pa, &S), "entry past the row's last refused");
  check(!scatter_on_pattern(A, pattern_of(Z), &S), "entry in an empty pattern row refused");
  check(!scatter_on_pattern(csr_from_coo(2, 4, {0}, {0}, {1}), Pa, &S), "fewer rows refused");
  check(!scatter_on_pattern(csr_from_coo(3, 3, {0}, {0}, {1}), Pa, &S), "fewer columns refused");
  return failed ? 1 : 0;
}
