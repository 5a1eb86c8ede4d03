// The exchange's host protocol (dcora_amd/csrc/exchange_slots.h) under ASan + UBSan, as a plain program.
//   san_host_exchange run world R rounds          exchange_rehearsal in `world` processes over an anonymous mapping
//       laid out like a job's segment: "checksum <rank> <value>" per rank and "ok 1" when all agree
//   san_host_exchange die world R timeout_s       the same with no end, rank 1 leaving after 2000 rounds:
//       "gave_up <rank> <code> <seconds>" for every other rank
//   san_host_exchange layout world R slot x w     the layout's own checks -- every area 64-byte aligned, the link
//       check's stages, the staged poses and X 4096-byte aligned, no two areas overlapping, the last one ending within
//       the total -- then "total <bytes>"
#include <cstring>

#include "san_host_ranks.h"

using namespace dcora;

static int check_layout(const SegmentLayout &l) {
  // the accessors on a real base: a reservation of the whole segment that is never touched
  char *b = (char *)mmap(nullptr, l.total, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
  if (b == MAP_FAILED) return 3;
  struct Area {
    const char *name;
    const void *begin, *end;
    size_t align;
  };
  const int W = l.world;
  const Area areas[] = {
      {"header", l.header(b), l.header(b) + 1, 64},
      {"ranks", l.rank_record(b, 0), l.rank_record(b, W), 64},
      {"flags", l.flag(b, 0, 0), l.flag(b, 2, 0), 64},
      {"evaluation slots", l.eval(b, 0, 0), l.heartbeat(b, 1, W), 64},
      {"consumed", l.consumed(b, 0, 0), l.consumed(b, W, 0), 64},
      {"sums", l.red(b, 0, 0), l.red(b, 2, 0), 64},
      {"statuses", l.status(b, 0, 0), l.status(b, 2, 0), 64},
      {"status read words", l.status_read(b, 0, 0), l.status_read(b, W, 0), 64},
      {"probe flags", l.probe_flag(b, 0, 0), l.probe_flag(b, W, 0), 64},
      {"probe results", l.probe_result(b, 0, 0), l.probe_result(b, W, 0), 64},
      {"probe stages", l.probe_stage(b, 0, 0), l.probe_stage(b, W, 0), 4096},
      {"staged poses", l.staged(b, 0, 0), l.staged(b, 2, 0), 4096},
      {"X", l.x(b), l.x(b) + l.x_doubles, 4096},
      {"weights", l.weights(b), l.weights(b) + l.w_doubles, 64},
  };
  int bad = 0;
  const char *end = b;
  for (const Area &a : areas) {
    const char *lo = (const char *)a.begin, *hi = (const char *)a.end;
    if ((size_t)(lo - b) % a.align || lo < end || hi < lo) {
      std::printf("bad area %s: [%zu, %zu) after %zu\n", a.name, (size_t)(lo - b), (size_t)(hi - b), (size_t)(end - b));
      bad = 1;
    }
    end = hi;
  }
  if ((size_t)(end - b) > l.total) bad = 1;
  munmap(b, l.total);
  std::printf("total %zu\n", l.total);
  return bad;
}

int main(int argc, char **argv) {
  if (argc < 5) return 2;
  const int world = std::atoi(argv[2]), R = std::atoi(argv[3]);
  if (world < 1 || world > kMaxRanks || R < 1 || R > kMaxAgents) return 2;
  if (!std::strcmp(argv[1], "layout") && argc == 7)
    return check_layout(SegmentLayout(world, R, std::strtoull(argv[4], nullptr, 10), std::strtoull(argv[5], nullptr, 10),
                                      std::strtoull(argv[6], nullptr, 10)));
  if (argc != 5) return 2;
  const int per = (R + world - 1) / world;
  const san::Job job(world, R);
  if (!std::strcmp(argv[1], "run")) {
    const int rounds = std::atoi(argv[4]);
    return job.report(job.run([&](int rank, double *checksum) {
      return exchange_rehearsal(job.slots(rank, 20.0), per, rounds, checksum, nullptr);
    }));
  }
  if (std::strcmp(argv[1], "die")) return 2;
  const double timeout_s = std::atof(argv[4]);
  job.run([&](int rank, double *checksum) {
    const int rc = exchange_rehearsal(job.slots(rank, timeout_s), per, rank == 1 ? 2000 : 1 << 30, checksum, nullptr);
    if (rank == 1) _exit(9);  // mid-run, without a word to anybody
    return rc;
  });
  for (int k = 0; k < world; ++k)
    if (k != 1) std::printf("gave_up %d %d %.3f\n", k, job.res->status[k], job.res->seconds[k]);
  return 0;
}
