// Unit test of dcora_amd/csrc/agent_block.h -- the global indices of the poses, unit spheres and landmarks of a hosted
// agent's block -- built with g++ under ASan + UBSan by tests/test_session_blocks_cpu.py.
//   no argument:  column lists built from chosen global indices, d = 2 and 3; prints "ok <case>" per passed case
//   query d n l  n_a l_a b_a  c0 c1 ...:  a listed block's columns (the whole problem's d, n, l first) -> three lines
//                 "pose ...", "sphere ...", "landmark ...": what tests/test_session_blocks_cpu.py holds against the
//                 ownership of the range-aided fixtures
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "agent_block.h"

namespace {

using dcora::AgentBlock;
using dcora::BlockStates;

// the columns of an agent that owns these global poses, unit spheres and landmarks, in its own ordering, out of a
// mirror in the range-aided ordering of n poses and l unit spheres
std::vector<int> columns_of(int d, int n, int l, const std::vector<int> &pose, const std::vector<int> &sphere,
                            const std::vector<int> &landmark) {
  std::vector<int> own;
  if (sphere.empty() && landmark.empty()) {  // SE ordering
    for (int p : pose) {
      for (int c = 0; c < d; ++c) own.push_back(d * p + c);
      own.push_back(d * n + l + p);
    }
    return own;
  }
  for (int p : pose)
    for (int c = 0; c < d; ++c) own.push_back(d * p + c);
  for (int s : sphere) own.push_back(d * n + s);
  for (int p : pose) own.push_back(d * n + l + p);
  for (int q : landmark) own.push_back(d * n + l + n + q);
  return own;
}

AgentBlock listed(const std::vector<int> &own, size_t n, size_t l, size_t b) {
  AgentBlock blk;
  blk.k = (int)own.size();
  blk.n = (int)n, blk.l = (int)l, blk.b = (int)b;
  blk.se = (l == 0 && b == 0) ? 1 : 0;
  blk.cols_host = own.data();
  blk.cols_dev = own.data();  // (never read on the host: only says that the block is listed)
  return blk;
}

bool returns_them(int d, int n, int l, const std::vector<int> &pose, const std::vector<int> &sphere,
                  const std::vector<int> &landmark) {
  const std::vector<int> own = columns_of(d, n, l, pose, sphere, landmark);
  BlockStates got;
  dcora::agent_block_states(listed(own, pose.size(), sphere.size(), landmark.size()), d, n, l, &got);
  return got.pose == pose && got.sphere == sphere && got.landmark == landmark;
}

void print(const char *what, const std::vector<int> &v) {
  std::printf("%s", what);
  for (int x : v) std::printf(" %d", x);
  std::printf("\n");
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1 && !std::strcmp(argv[1], "query")) {
    if (argc < 8) return 2;
    const int d = std::atoi(argv[2]), n = std::atoi(argv[3]), l = std::atoi(argv[4]);
    const int na = std::atoi(argv[5]), la = std::atoi(argv[6]), ba = std::atoi(argv[7]);
    std::vector<int> own;
    for (int i = 8; i < argc; ++i) own.push_back(std::atoi(argv[i]));
    if ((int)own.size() != (d + 1) * na + la + ba) return 2;
    BlockStates got;
    dcora::agent_block_states(listed(own, (size_t)na, (size_t)la, (size_t)ba), d, n, l, &got);
    print("pose", got.pose);
    print("sphere", got.sphere);
    print("landmark", got.landmark);
    return 0;
  }
  int failed = 0;
  auto check = [&](bool ok, const char *what, int d) {
    std::printf("%s %s d=%d\n", ok ? "ok" : "FAILED", what, d);
    failed += !ok;
  };
  for (int d = 2; d <= 3; ++d) {
    const int n = 9, l = 4;  // the whole problem: 9 poses, 4 unit spheres (and landmarks behind them)
    // the SE ordering: neither a unit sphere nor a landmark, the poses neither contiguous nor monotone
    check(returns_them(d, n, l, {5, 1, 8, 3}, {}, {}), "se", d);
    check(returns_them(d, n, 0, {2, 0}, {}, {}), "se-of-a-problem-without-spheres", d);
    // [rotations | unit spheres | translations | landmarks] with l, b > 0
    check(returns_them(d, n, l, {7, 0, 4}, {3, 1}, {2, 0, 5}), "ra", d);
    // a landmark but no unit sphere, a unit sphere but no landmark
    check(returns_them(d, n, l, {6, 2}, {}, {1}), "landmark-without-sphere", d);
    check(returns_them(d, n, l, {4}, {0, 2}, {}), "sphere-without-landmark", d);
    // a contiguous range of a mirror in the SE ordering, from col0
    AgentBlock blk;
    blk.n = 3, blk.k = (d + 1) * 3, blk.col0 = (long)(d + 1) * 4;
    BlockStates got;
    dcora::agent_block_states(blk, d, n, 0, &got);
    check(blk.contiguous() && got.pose == std::vector<int>({4, 5, 6}) && got.sphere.empty() && got.landmark.empty() &&
              blk.global_col(0) == blk.col0 && blk.global_col(blk.k - 1) == blk.col0 + blk.k - 1,
          "contiguous", d);
    const std::vector<int> own = columns_of(d, n, l, {7, 0, 4}, {3, 1}, {2, 0, 5});
    const AgentBlock lb = listed(own, 3, 2, 3);
    check(!lb.contiguous() && lb.global_col(0) == d * 7 && lb.global_col(lb.k - 1) == d * n + l + n + 5, "listed-columns", d);
  }
  return failed ? 1 : 0;
}
