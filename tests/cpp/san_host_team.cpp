// The team protocol's host transport (dcora_amd/csrc/team_slots.h) under ASan + UBSan, as a plain program: `world`
// processes share an anonymous mapping laid out like the exchange's status area and run team_rehearsal on it -- the
// slots, the read words, the bounded waits and the rules -- with a heartbeat of their own in the evaluation's place.
// usage: san_host_team world R rounds skew_us.  Prints "checksum <rank> <value>" per rank and "ok 1" when all agree.
#include <sys/mman.h>
#include <sys/wait.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "team_slots.h"

using namespace dcora;

struct alignas(64) Shared {
  std::atomic<uint32_t> failed;
  double checksum[64];
  int status[64];
};

int main(int argc, char **argv) {
  if (argc != 5) return 2;
  const int world = std::atoi(argv[1]), R = std::atoi(argv[2]), rounds = std::atoi(argv[3]), skew = std::atoi(argv[4]);
  if (world < 1 || world > 64 || R < 1 || R > 64 || rounds < 1 || skew < 0) return 2;
  const size_t bytes = sizeof(Shared) + sizeof(ShmFlag) * 2 * world + sizeof(ShmStatus) * 2 * R + sizeof(ShmFlag) * world * R;
  void *map = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
  if (map == MAP_FAILED) return 3;
  std::memset(map, 0, bytes);
  Shared *sh = new (map) Shared;
  ShmFlag *beat = (ShmFlag *)(sh + 1);  // [parity][rank]
  ShmStatus *status = (ShmStatus *)(beat + 2 * world);
  ShmFlag *read = (ShmFlag *)(status + 2 * R);
  auto run = [&](int rank) {
    TeamSlots t;
    t.status = status;
    t.read = read;
    t.failed = &sh->failed;
    t.rank = rank;
    t.world = world;
    t.R = R;
    t.timeout_s = 20.0;
    uint64_t beats = 0;
    auto heartbeat = [&]() -> int {
      const uint64_t want = ++beats;
      ShmFlag *hb = beat + (size_t)(want & 1) * world;
      std::atomic_thread_fence(std::memory_order_release);
      hb[rank].seq = want;
      for (int p = 0; p < world; ++p)
        if (const int rc = t.wait_until([&] { return hb[p].seq >= want; })) return rc;
      return 0;
    };
    double cs = 0;
    const int rc = team_rehearsal(t, (R + world - 1) / world, rounds, skew, heartbeat, &cs);
    if (rc) sh->failed.store(1);
    sh->checksum[rank] = cs;
    sh->status[rank] = rc;
    return rc;
  };
  std::vector<pid_t> kids;
  for (int k = 1; k < world; ++k) {
    const pid_t pid = fork();
    if (pid < 0) return 4;
    if (pid == 0) _exit(run(k));
    kids.push_back(pid);
  }
  int bad = run(0);
  for (pid_t pid : kids) {
    int st = 0;
    waitpid(pid, &st, 0);
    if (!WIFEXITED(st) || WEXITSTATUS(st) != 0) bad = 1;
  }
  bool same = !bad;
  for (int k = 0; k < world; ++k) {
    std::printf("checksum %d %.17g\n", k, sh->checksum[k]);
    same = same && sh->status[k] == 0 && sh->checksum[k] == sh->checksum[0];
  }
  std::printf("ok %d\n", same ? 1 : 0);
  munmap(map, bytes);
  return same ? 0 : 1;
}
