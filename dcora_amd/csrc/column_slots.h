// The column-slot map of a workgroup tiling (host only: no HIP in here).  A kernel whose workgroup holds `pb` poses
// gathers, for every CSR entry of its (d+1) pb matrix rows, the column the entry names.  The rows of one pose name the
// same neighbour poses and a pose's d+1 columns are contiguous, so the distinct columns of a workgroup are a short
// list of whole pose blocks: the kernel fetches each listed block ONCE into LDS and the rows read their operands by
// slot.  Pose blocks are the unit because SE-layout rows never name part of a foreign layout.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace dcora {

constexpr uint16_t kNoSlot = 0xffff;  // entry of an overflow workgroup: it keeps its global column (the kernel reads ci)

struct ColumnSlots {
  int nwg = 0;
  // CSR-style per workgroup: list[lp[w] .. lp[w + 1]) are the distinct poses its rows name, ascending, its own poses
  // among them.  An overflow workgroup's list is EMPTY (the kernels test lp[w + 1] == lp[w]) ...
  std::vector<int> lp, list;
  // ... and count[w] says how many poses it names (> cap_poses exactly where overflow[w])
  std::vector<int> count;
  std::vector<uint8_t> overflow;
  // per CSR entry: (position of its pose in the workgroup's list) * (d+1) + column within the pose; kNoSlot in an
  // overflow workgroup
  std::vector<uint16_t> slot;
  int max_count = 0, n_overflow = 0;
};

// rp, ci: the pattern of an n (d+1) square SE-layout matrix (dh = d + 1); pb: poses per workgroup; cap_cols: the most
// columns a workgroup's list may hold (whole pose blocks: cap_cols / dh poses; at most 0xffff columns).  Columns at or
// beyond n dh (none on the SE layout) make the workgroup an overflow one.
inline ColumnSlots column_slots(const int *rp, const int *ci, int n, int dh, int pb, int cap_cols) {
  ColumnSlots cs;
  if (n <= 0 || dh <= 0 || pb <= 0) {
    cs.lp.assign(1, 0);
    return cs;
  }
  const int cap_poses = std::min(cap_cols, 0xffff) / dh;
  cs.nwg = (n + pb - 1) / pb;
  cs.lp.assign((size_t)cs.nwg + 1, 0);
  cs.count.assign((size_t)cs.nwg, 0);
  cs.overflow.assign((size_t)cs.nwg, 0);
  cs.slot.assign((size_t)rp[(size_t)n * dh], kNoSlot);
  std::vector<int> pos((size_t)n, -1), named;
  for (int w = 0; w < cs.nwg; ++w) {
    const int p0 = w * pb, p1 = std::min(n, p0 + pb);
    const int eb = rp[(size_t)p0 * dh], ee = rp[(size_t)p1 * dh];
    named.clear();
    bool foreign = false;
    auto name = [&](int p) {
      if (pos[(size_t)p] < 0) {
        pos[(size_t)p] = 0;
        named.push_back(p);
      }
    };
    for (int p = p0; p < p1; ++p) name(p);
    for (int e = eb; e < ee; ++e) {
      if (ci[e] < 0 || ci[e] >= n * dh) {
        foreign = true;
        continue;
      }
      name(ci[e] / dh);
    }
    std::sort(named.begin(), named.end());
    cs.count[(size_t)w] = (int)named.size();
    cs.max_count = std::max(cs.max_count, (int)named.size());
    const bool over = foreign || (int)named.size() > cap_poses;
    cs.overflow[(size_t)w] = over ? 1 : 0;
    if (over) {
      ++cs.n_overflow;
    } else {
      for (size_t i = 0; i < named.size(); ++i) pos[(size_t)named[i]] = (int)i;
      for (int e = eb; e < ee; ++e) cs.slot[(size_t)e] = (uint16_t)(pos[(size_t)(ci[e] / dh)] * dh + ci[e] % dh);
      cs.list.insert(cs.list.end(), named.begin(), named.end());
    }
    for (int p : named) pos[(size_t)p] = -1;
    cs.lp[(size_t)w + 1] = (int)cs.list.size();
  }
  return cs;
}

}  // namespace dcora
