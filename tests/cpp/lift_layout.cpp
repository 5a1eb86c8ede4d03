// The room a job keeps for its later ranks (dcora_amd/csrc/exchange_slots.h), as a plain host program without HIP:
//   lift_layout layout world R maxcols r reserve k w   every offset and the total of SegmentLayout::for_job, one line
//   lift_layout plain  world R slot x w                the same line for SegmentLayout(world, R, slot, x, w)
//   lift_layout check  d r r_reserve zero_is_none      the status reserve_rank_check gives (0 = DCORA_OK, 1 = BAD_ARG)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "exchange_slots.h"

using namespace dcora;

static int print_layout(const SegmentLayout &l) {
  std::printf("%d %d %zu %zu %zu | %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", l.world, l.R, l.slot,
              l.x_doubles, l.w_doubles, l.off_ranks, l.off_flags, l.off_evals, l.off_consumed, l.off_red, l.off_status,
              l.off_status_read, l.off_probe_flags, l.off_probe_res, l.off_probe_stage, l.off_staged, l.off_x, l.off_w,
              l.total);
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  auto num = [&](int i) { return std::strtoull(argv[i], nullptr, 10); };
  if (!std::strcmp(argv[1], "layout") && argc == 9)
    return print_layout(SegmentLayout::for_job((int)num(2), (int)num(3), num(4), (int)num(5), (int)num(6), num(7), num(8)));
  if (!std::strcmp(argv[1], "plain") && argc == 7)
    return print_layout(SegmentLayout((int)num(2), (int)num(3), num(4), num(5), num(6)));
  if (!std::strcmp(argv[1], "check") && argc == 6) {
    std::printf("%d\n", reserve_rank_check(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]) != 0));
    return 0;
  }
  return 2;
}
