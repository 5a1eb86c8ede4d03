// What the sanitizer programs of the host protocol share (san_host_team.cpp, san_host_exchange.cpp): `world` forked
// processes over one anonymous shared mapping laid out by SegmentLayout like a job's segment, with a record of what
// every rank returned behind it.
#pragma once
#include <sys/mman.h>
#include <sys/wait.h>

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <new>

#include "exchange_slots.h"

namespace san {

using namespace dcora;

struct Results {
  double checksum[kMaxRanks];
  double seconds[kMaxRanks];
  int status[kMaxRanks];
};

struct Job {
  SegmentLayout lay;
  void *map = nullptr;
  Results *res = nullptr;

  Job(int world, int R) : lay(world, R, 16, 16, 0) {
    map = mmap(nullptr, lay.total + sizeof(Results), PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
    if (map == MAP_FAILED) std::exit(3);
    new (lay.header(map)) ShmHeader{};  // (an anonymous mapping starts zeroed, as rank 0's memset leaves the segment)
    res = new ((char *)map + lay.total) Results{};
  }
  ~Job() { munmap(map, lay.total + sizeof(Results)); }
  ExchangeSlots slots(int rank, double timeout_s) const { return ExchangeSlots{lay, map, rank, timeout_s}; }

  // body(rank, &checksum) in `world` processes (rank 0: this one); a rank that gives up raises `failed`, as
  // Exchange::fail does.  True when every child exited through its body.
  bool run(const std::function<int(int, double *)> &body) const {
    auto one = [&](int rank) {
      const auto t0 = Clock::now();
      const int rc = body(rank, &res->checksum[rank]);
      if (rc) lay.header(map)->failed.store(1);
      res->status[rank] = rc;
      res->seconds[rank] = since(t0);
      return rc;
    };
    std::vector<pid_t> kids;
    for (int k = 1; k < lay.world; ++k) {
      const pid_t pid = fork();
      if (pid < 0) std::exit(4);
      if (pid == 0) _exit(one(k) ? 1 : 0);
      kids.push_back(pid);
    }
    one(0);
    bool clean = true;
    for (pid_t pid : kids) {
      int st = 0;
      waitpid(pid, &st, 0);
      clean = clean && WIFEXITED(st) && WEXITSTATUS(st) <= 1;
    }
    return clean;
  }
  // "checksum <rank> <value>" per rank and "ok 1" when every rank returned 0 with rank 0's checksum
  int report(bool clean) const {
    bool same = clean;
    for (int k = 0; k < lay.world; ++k) {
      std::printf("checksum %d %.17g\n", k, res->checksum[k]);
      same = same && res->status[k] == 0 && res->checksum[k] == res->checksum[0];
    }
    std::printf("ok %d\n", same ? 1 : 0);
    return same ? 0 : 1;
  }
};

}  // namespace san
