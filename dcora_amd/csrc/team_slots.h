// The team protocol's transport between the ranks of a job, host side (no HIP): the status slots in the shared segment,
// the words that say how far every rank has read them, and the bounded waits on both.  Exchange (exchange.h) places
// them in its segment and drives them from its collective calls; the rehearsal at the end runs the same slots and waits
// with host stores in the device's place (dcora_exchange_host_selftest_team, and the sanitizer program of the tests).
#pragma once
#include <sched.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <functional>
#include <vector>

#include "team_rules.h"

namespace dcora {

struct alignas(64) ShmFlag {
  volatile uint64_t seq;
  uint64_t pad[7];
};
// one agent's status slot: what only the hosting rank knows of an optimisation
struct alignas(64) ShmStatus {
  volatile double rel;        // LiftedArray::maxTranslationDistance(X, XPrev), stored by the ranked k_rel_change
  volatile uint64_t seq;      // the optimisation of the agent the slot holds (stored last, by the same kernel)
  volatile uint32_t success;  // !last_skipped, stored by the hosting rank's host before the launch
  uint32_t pad32;
  uint64_t pad[5];
};

// host polling with back-off: a burst of pause instructions, then the core is handed over between polls (a rank per
// core is not guaranteed: the four-ranks-on-one-GPU rehearsal runs on whatever cores the container has)
inline void polite_spin(unsigned &spins) {
  ++spins;
  if (spins < 2048u) {
    __builtin_ia32_pause();
  } else if (spins < 8192u) {
    sched_yield();
  } else {
    usleep(50);
  }
}

enum { kTeamWaitOk = 0, kTeamWaitPeerFailed = 1, kTeamWaitTimeout = 2 };

// Optimisation q of agent a (q counts from 1, the same on every rank) lives in slot [q & 1][a], last used by q - 2.
struct TeamSlots {
  ShmStatus *status = nullptr;  // [2][R]
  ShmFlag *read = nullptr;      // [reader rank][R]: the last optimisation of the agent whose status that rank has read
  std::atomic<uint32_t> *failed = nullptr;  // the job's failure word: every wait gives up when it is raised
  int rank = 0, world = 1, R = 0;
  double timeout_s = 120.0;

  ShmStatus *slot(uint64_t q, int a) const { return status + (size_t)(q & 1) * R + a; }

  template <class Ready>
  int wait_until(Ready &&ready) const {
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    while (!ready()) {
      polite_spin(spins);
      if ((spins & 1023u) == 0) {
        if (failed->load()) return kTeamWaitPeerFailed;
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s)
          return kTeamWaitTimeout;
      }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return kTeamWaitOk;
  }
  // the writer's back-pressure: every rank has read optimisation `upto` of the agent (*whom: the rank that has not)
  int read_wait(int agent, uint64_t upto, int *whom) const {
    for (int p = 0; p < world; ++p) {
      const ShmFlag *rf = read + (size_t)p * R + agent;
      const int rc = wait_until([&] { return rf->seq >= upto; });
      if (rc) {
        if (whom) *whom = p;
        return rc;
      }
    }
    return kTeamWaitOk;
  }
  // the reader's wait: the slot holds optimisation q of the agent
  int status_wait(uint64_t q, int agent) const {
    const ShmStatus *s = slot(q, agent);
    return wait_until([&] { return s->seq >= q; });
  }
  void mark_read(uint64_t q, int agent) const {
    std::atomic_thread_fence(std::memory_order_release);
    read[(size_t)rank * R + agent].seq = q;
  }
  // what the hosting rank's host and its ranked k_rel_change store, from the host (the rehearsal only)
  void publish_from_host(uint64_t q, int agent, bool success, double rel) const {
    ShmStatus *s = slot(q, agent);
    s->success = success ? 1u : 0u;
    s->rel = rel;
    std::atomic_thread_fence(std::memory_order_release);
    s->seq = q;
  }
};

// The rehearsal.  Round q = 1 .. rounds: a tick of the agents a with a % 2 == (q / 3) % 2 when q % 3 == 0, else agent
// q % R alone followed by heartbeat() (the evaluation's: nobody leaves it before everybody has entered it).  Agent a
// lives on rank a / per.  Its owner publishes success = (q + a) % 5 != 0 and relative change 0.001 ((7 q + 3 a) % 11).
// Every rank settles the status (robust team, 4 accepted and min(updates, 2) rejected of 6 loop closures, the default
// parameters with 3 weight updates, 7 inner iterations and no iteration cap), decides, and applies an update's
// bookkeeping when the rules ask for one.  Rank k sleeps k * skew_us at the start of a round.
inline int team_rehearsal(const TeamSlots &t, int per, int rounds, int skew_us, const std::function<int()> &heartbeat,
                          double *checksum) {
  const int R = t.R;
  dcora_team_params p = team_params_default();
  p.max_num_iters = 1 << 30;
  p.robust_opt_num_weight_updates = 3;
  p.robust_opt_inner_iters = 7;
  std::vector<dcora_agent_status> status((size_t)R, dcora_agent_status{});
  std::vector<int> have((size_t)R, 0);
  std::vector<uint64_t> seq((size_t)R, 0);
  int updates = 0, inner = 0, latest = 0;
  double sum = 0;
  for (int q = 1; q <= rounds; ++q) {
    if (skew_us) usleep((useconds_t)t.rank * (useconds_t)skew_us);
    const bool tick = q % 3 == 0;
    std::vector<int> set;
    if (tick) {
      for (int a = 0; a < R; ++a)
        if (a % 2 == (q / 3) % 2) set.push_back(a);
    } else {
      set.push_back(q % R);
    }
    ++inner;
    const int rejected = std::min(updates, 2);
    for (int a : set) {
      const uint64_t k = ++seq[(size_t)a];
      if (a / per != t.rank) continue;
      if (k > 2)
        if (const int rc = t.read_wait(a, k - 2, nullptr)) return rc;
      t.publish_from_host(k, a, (q + a) % 5 != 0, 0.001 * (double)((7 * q + 3 * a) % 11));
    }
    for (int a : set) {
      const uint64_t k = seq[(size_t)a];
      if (const int rc = t.status_wait(k, a)) return rc;
      const ShmStatus *slot = t.slot(k, a);
      dcora_agent_status &st = status[(size_t)a];
      st = dcora_agent_status{};
      st.agent_id = a;
      st.state = DCORA_AGENT_INITIALIZED;
      st.iteration_number = q;
      st.relative_change = slot->rel;
      st.ready_to_terminate =
          team_ready_to_terminate(p, true, updates, slot->success != 0, st.relative_change, 4, rejected, 6) ? 1 : 0;
      have[(size_t)a] = 1;
      t.mark_read(k, a);
    }
    if (!tick)
      if (const int rc = heartbeat()) return rc;
    const TeamView v{true, q, updates, inner, latest, status.data(), have.data(), nullptr, R};
    const bool term = team_should_terminate(p, v), upd = team_should_update_weights(p, v);
    for (int a = 0; a < R; ++a)
      if (have[(size_t)a])
        sum += (a + 1) * ((double)status[(size_t)a].iteration_number + 0.5 * status[(size_t)a].ready_to_terminate +
                          status[(size_t)a].relative_change);
    sum += 1000.0 * (term ? 1 : 0) + 2000.0 * (upd ? 1 : 0);
    if (upd) {  // Agent::updateMeasurementWeights' bookkeeping (ref src/Agent.cpp:1417-1424)
      ++updates;
      inner = 0;
      latest = q;
      have.assign((size_t)R, 0);
    }
  }
  if (checksum) *checksum = sum;
  return kTeamWaitOk;
}

}  // namespace dcora
