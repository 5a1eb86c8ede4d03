// The column-slot map of a workgroup tiling (dcora_amd/csrc/column_slots.h) on the shapes at which it can go wrong,
// as a program of its own (built with -fsanitize=address,undefined by tests/test_column_slots_cpu.py; no device).
// For every case and tiling: the lists are ascending, distinct and hold the workgroup's own poses; every entry's slot
// leads back to its column; overflow is flagged exactly where the poses a workgroup names exceed the cap, counted here
// with a std::set; an overflow workgroup has an empty list and entries without a slot.
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "column_slots.h"

using dcora::ColumnSlots;

namespace {

int g_failed = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      std::printf("FAILED %s: ", #cond);       \
      std::printf(__VA_ARGS__);                \
      std::printf("\n");                       \
      ++g_failed;                              \
    }                                          \
  } while (0)

struct Pattern {
  int n, dh;
  std::vector<int> rp, ci;
};

// SE-layout pattern of a pose graph: the dh rows of a pose name every column of the pose and of its neighbours, except
// that an edge i -> j with i < j leaves the last column of i out of the rows of j (rows of one pose then differ in
// nothing, rows of different poses do: what an entering edge without a translation block looks like)
Pattern pattern_of(int n, int dh, const std::vector<std::pair<int, int>> &edges) {
  std::vector<std::set<int>> nb((size_t)n);
  for (auto [i, j] : edges) {
    nb[(size_t)i].insert(j);
    nb[(size_t)j].insert(i);
  }
  Pattern P{n, dh, {0}, {}};
  for (int i = 0; i < n; ++i) {
    nb[(size_t)i].insert(i);
    for (int a = 0; a < dh; ++a) {
      for (int j : nb[(size_t)i])
        for (int c = 0; c < dh; ++c)
          if (!(j < i && c == dh - 1)) P.ci.push_back(j * dh + c);
      P.rp.push_back((int)P.ci.size());
    }
  }
  return P;
}

std::vector<std::pair<int, int>> chain(int n) {
  std::vector<std::pair<int, int>> e;
  for (int i = 0; i + 1 < n; ++i) e.push_back({i, i + 1});
  return e;
}
// the hub graph of tests/test_run_waits_gpu.py: pose 5 of degree 9, pose 20 of degree 6
std::vector<std::pair<int, int>> hubs(int n) {
  std::vector<std::pair<int, int>> e = chain(n);
  for (int j : {9, 12, 15, 18, 21, 24, 27}) e.push_back({5, j});
  for (int j : {2, 7, 11, 30}) e.push_back({20, j});
  return e;
}
std::vector<std::pair<int, int>> star(int n, int centre) {
  std::vector<std::pair<int, int>> e = chain(n);
  for (int j = 0; j < n; ++j)
    if (j < centre - 1 || j > centre + 1) e.push_back({centre, j});
  return e;
}

int check_map(const char *name, const Pattern &P, int pb, int cap_cols) {
  const int before = g_failed;
  const ColumnSlots cs = dcora::column_slots(P.rp.data(), P.ci.data(), P.n, P.dh, pb, cap_cols);
  const int nwg = (P.n + pb - 1) / pb, cap_poses = cap_cols / P.dh;
  CHECK(cs.nwg == nwg && (int)cs.lp.size() == nwg + 1 && cs.lp[0] == 0, "%s pb %d: %d workgroups", name, pb, cs.nwg);
  CHECK(cs.slot.size() == P.ci.size(), "%s: one slot per entry", name);
  int n_over = 0, max_count = 0;
  for (int w = 0; w < nwg; ++w) {
    const int p0 = w * pb, p1 = std::min(P.n, p0 + pb);
    std::set<int> want;
    for (int p = p0; p < p1; ++p) want.insert(p);
    for (int e = P.rp[(size_t)p0 * P.dh]; e < P.rp[(size_t)p1 * P.dh]; ++e) want.insert(P.ci[(size_t)e] / P.dh);
    const bool over = (int)want.size() > cap_poses;
    n_over += over;
    max_count = std::max(max_count, (int)want.size());
    CHECK(cs.count[(size_t)w] == (int)want.size(), "%s pb %d wg %d: count %d, want %zu", name, pb, w, cs.count[(size_t)w],
          want.size());
    CHECK((cs.overflow[(size_t)w] != 0) == over, "%s pb %d wg %d: overflow %d with %zu poses, cap %d", name, pb, w,
          (int)cs.overflow[(size_t)w], want.size(), cap_poses);
    const int lb = cs.lp[(size_t)w], le = cs.lp[(size_t)w + 1];
    if (over) {
      CHECK(le == lb, "%s pb %d wg %d: an overflow workgroup has no list", name, pb, w);
      for (int e = P.rp[(size_t)p0 * P.dh]; e < P.rp[(size_t)p1 * P.dh]; ++e)
        CHECK(cs.slot[(size_t)e] == dcora::kNoSlot, "%s wg %d entry %d: slot in an overflow workgroup", name, w, e);
      continue;
    }
    CHECK(le - lb == (int)want.size(), "%s pb %d wg %d: list of %d", name, pb, w, le - lb);
    for (int i = lb; i < le; ++i) {
      CHECK(want.count(cs.list[(size_t)i]) == 1, "%s wg %d: pose %d is not named", name, w, cs.list[(size_t)i]);
      if (i > lb) CHECK(cs.list[(size_t)i] > cs.list[(size_t)i - 1], "%s wg %d: not ascending at %d", name, w, i - lb);
    }
    for (int e = P.rp[(size_t)p0 * P.dh]; e < P.rp[(size_t)p1 * P.dh]; ++e) {
      const int s = cs.slot[(size_t)e];
      CHECK(s / P.dh < le - lb, "%s wg %d entry %d: slot %d beyond the list", name, w, e, s);
      if (s / P.dh < le - lb)
        CHECK(cs.list[(size_t)(lb + s / P.dh)] * P.dh + s % P.dh == P.ci[(size_t)e], "%s wg %d entry %d: slot %d, ci %d",
              name, w, e, s, P.ci[(size_t)e]);
    }
  }
  CHECK(cs.n_overflow == n_over && cs.max_count == max_count, "%s pb %d: %d overflow, most %d", name, pb, cs.n_overflow,
        cs.max_count);
  std::printf("%-10s n %3d pb %2d cap %3d: %3d workgroups, %d overflow, most %d poses %s\n", name, P.n, pb, cap_cols, nwg,
              n_over, max_count, g_failed == before ? "ok" : "FAILED");
  return n_over;
}

}  // namespace

int main() {
  const int dh = 4;
  // the two tilings: 2 poses with lists of 64 columns (k_tcg_run), fused_pb = 16 / 12 / 10 poses at r = 4 / 5 / 6 with
  // lists of 256 columns
  const std::pair<int, int> tilings[] = {{2, 64}, {16, 256}, {12, 256}, {10, 256}};
  for (auto [pb, cap] : tilings) {
    for (int n : {2, 3, 33, 161}) {
      const Pattern P = pattern_of(n, dh, n > 30 ? hubs(n) : chain(n));
      CHECK(check_map(n > 30 ? "hubs" : "chain", P, pb, cap) == 0, "no overflow on the hub graph (n %d, pb %d)", n, pb);
    }
    check_map("chain", pattern_of(40, dh, chain(40)), pb, cap);
    check_map("odd", pattern_of(25, dh, chain(25)), pb, cap);  // the last workgroup holds one pose (pb = 2, 16, 12)
    // a star whose centre names more poses than the cap holds: its workgroup overflows, and only workgroups that hold
    // the centre or enough of its spokes do
    const int n = 100, centre = 41;
    const Pattern S = pattern_of(n, dh, star(n, centre));
    const int over = check_map("star", S, pb, cap);
    CHECK(over >= 1, "the centre's workgroup overflows (pb %d)", pb);
    const ColumnSlots cs = dcora::column_slots(S.rp.data(), S.ci.data(), n, dh, pb, cap);
    CHECK(cs.overflow[(size_t)(centre / pb)] == 1, "the centre's workgroup is the one flagged");
    if (pb == 2) CHECK(over == 1, "2-pose tiling: only the centre's workgroup overflows, %d do", over);
    // the same star under a cap that just holds it: nothing overflows
    CHECK(check_map("star-fits", S, pb, n * dh) == 0, "a cap of every column holds every list");
  }
  // a d = 2 layout (dh = 3) and a cap that is no multiple of dh: whole pose blocks only
  check_map("dh3", pattern_of(31, 3, hubs(31)), 2, 10);
  if (g_failed) {
    std::printf("%d checks failed\n", g_failed);
    return 1;
  }
  std::printf("all ok\n");
  return 0;
}
