// The team protocol's host transport (dcora_amd/csrc/exchange_slots.h) under ASan + UBSan, as a plain program: `world`
// processes share an anonymous mapping laid out like a job's segment and run team_rehearsal on it -- the slots, the
// read words, the bounded waits, the evaluation's heartbeat and the rules.
// usage: san_host_team world R rounds skew_us.  Prints "checksum <rank> <value>" per rank and "ok 1" when all agree.
#include "san_host_ranks.h"

int main(int argc, char **argv) {
  if (argc != 5) return 2;
  const int world = std::atoi(argv[1]), R = std::atoi(argv[2]), rounds = std::atoi(argv[3]), skew = std::atoi(argv[4]);
  if (world < 1 || world > 64 || R < 1 || R > 64 || rounds < 1 || skew < 0) return 2;
  const san::Job job(world, R);
  return job.report(job.run([&](int rank, double *checksum) {
    return dcora::team_rehearsal(job.slots(rank, 20.0), (R + world - 1) / world, rounds, skew, checksum);
  }));
}
