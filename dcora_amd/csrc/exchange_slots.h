// The host protocol of a multi-rank job, stated once (no HIP: plain C++, also compiled into the sanitizer programs of
// the tests): the records of the POSIX shared segment, where every area of it lies (SegmentLayout), the one bounded
// wait (Wait), and the host steps over both (ExchangeSlots) -- the back-pressure of a post, the consumer's flag wait,
// the evaluation's heartbeat and gather, the barrier, the sum over the ranks, and the team's status slots.  Exchange
// (exchange.h) wraps each step with its error text and its statistics and forms its kernels' arguments with the same
// accessors on the device view of the segment; the two rehearsals at the end drive the same steps with host stores in
// the device's place (dcora_exchange_host_selftest, dcora_exchange_host_selftest_team, tests/cpp/san_host_*.cpp).
#pragma once
#include <sched.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "team_rules.h"

namespace dcora {

constexpr int kMaxRanks = 64;
constexpr int kMaxAgents = 64;
constexpr uint32_t kShmMagic = 0x44434f52u;  // "DCOR"
constexpr int kProbeDoubles = 512;           // the link check's payload: 4 KB

// What dcora_rbcd_reserve_rank / dcora_ra_rbcd_reserve_rank and the *_reserved creators accept for a session of
// dimension d at rank r: 0 (no reserve; the creators only) or d <= r <= r_reserve <= 16, the largest rank the kernels
// are built for.  The codes are DCORA_OK and DCORA_ERR_BAD_ARG, stated as numbers: this header includes no other.
constexpr int kMaxRank = 16;
inline int reserve_rank_check(int d, int r, int r_reserve, bool zero_is_none) {
  if (zero_is_none && r_reserve == 0) return 0;
  return d <= r && r <= r_reserve && r_reserve <= kMaxRank ? 0 : 1;
}

// ---- the records of the segment -------------------------------------------------------------------------------------
struct alignas(64) ShmFlag {
  volatile uint64_t seq;
  uint64_t pad[7];
};
struct alignas(64) ShmEval {
  volatile double g2, xeg;  // |Proj(X_b Q_bb + G_b)|^2, <X_b, X_b Q_bb + G_b>
  volatile uint64_t seq;
  uint64_t pad[5];
};
struct alignas(64) ShmRed {  // one rank's contribution to a sum over the ranks
  volatile uint64_t seq;
  double vals[31];
};
// one agent's status slot: what only the hosting rank knows of an optimisation
struct alignas(64) ShmStatus {
  volatile double rel;        // LiftedArray::maxTranslationDistance(X, XPrev), stored by the ranked k_rel_change
  volatile uint64_t seq;      // the optimisation of the agent the slot holds (stored last, by the same kernel)
  volatile uint32_t success;  // !last_skipped, stored by the hosting rank's host before the launch
  uint32_t pad32;
  uint64_t pad[5];
};
struct alignas(64) ShmRank {
  unsigned char halo[64];  // the rank's hipIpcMemHandle_t, copied in and out as bytes
  std::atomic<int> device, pid, ipc_ok, published;
  std::atomic<uint64_t> bus;  // hash of the device's PCI bus id: two ranks with the same value share a GPU
  std::atomic<int> fine;      // 1: this rank's halo buffer is fine-grained device memory
  std::atomic<int> probe;     // link check: +round passed, -round failed
  uint64_t pad[4];
};
struct ShmHeader {
  std::atomic<uint32_t> magic;
  uint32_t world, R;
  uint64_t slot_doubles, total_bytes, x_doubles;
  std::atomic<uint32_t> bar_count, bar_gen;
  std::atomic<uint32_t> failed;  // a rank gave up: everybody waiting returns an error instead of spinning on
  int32_t creator_pid;           // rank 0's process: a segment whose creator is gone is a stale one (crashed job)
  uint64_t creator_start;        // ... and its start time (/proc/<pid>/stat): a recycled pid is not the creator
};

// ---- where every area lies: header | per-rank records | flags [2][R] | evaluation slots [2][R + world] | consumed
//      words [world][R] | sums [2][world] | statuses [2][R] and their read words [world][R] | link check: flag and
//      result words [world][world], 4 KB stages [world][world] | staged poses [2][R][slot] | X | weights.
//      Every accessor takes the base of a view of the segment: the host mapping, or the device's view of it.
struct SegmentLayout {
  int world = 1, R = 0;
  size_t slot = 0, x_doubles = 0, w_doubles = 0;  // doubles per agent slot, of the X area, of the weights area
  size_t off_ranks = 0, off_flags = 0, off_evals = 0, off_consumed = 0, off_red = 0, off_status = 0, off_status_read = 0,
         off_probe_flags = 0, off_probe_res = 0, off_probe_stage = 0, off_staged = 0, off_x = 0, off_w = 0, total = 0;

  SegmentLayout() = default;
  SegmentLayout(int world_, int R_, size_t slot_doubles, size_t x_doubles_, size_t w_doubles_)
      : world(world_), R(R_), slot(slot_doubles), x_doubles(x_doubles_), w_doubles(w_doubles_) {
    const size_t W = (size_t)world, A = (size_t)R;
    size_t off = sizeof(ShmHeader);
    auto take = [&off](size_t align, size_t bytes) {  // the next area: its offset
      off = (off + align - 1) / align * align;
      const size_t at = off;
      off += bytes;
      return at;
    };
    off_ranks = take(64, sizeof(ShmRank) * W);
    off_flags = take(64, sizeof(ShmFlag) * 2 * A);
    off_evals = take(64, sizeof(ShmEval) * 2 * (A + W));  // R agent slots + one heartbeat slot per rank, per parity
    off_consumed = take(64, sizeof(ShmFlag) * W * A);
    off_red = take(64, sizeof(ShmRed) * 2 * W);
    off_status = take(64, sizeof(ShmStatus) * 2 * A);
    off_status_read = take(64, sizeof(ShmFlag) * W * A);
    off_probe_flags = take(64, sizeof(ShmFlag) * W * W);
    off_probe_res = take(64, sizeof(ShmFlag) * W * W);
    off_probe_stage = take(4096, sizeof(double) * kProbeDoubles * W * W);
    off_staged = take(4096, sizeof(double) * 2 * A * slot);
    off_x = take(4096, sizeof(double) * x_doubles);
    off_w = take(64, sizeof(double) * w_doubles);
    total = take(4096, 0);
  }

  // The segment of a job whose sessions are at rank r and have reserved reserve_r (SessionCore::reserve_r; 0: none):
  // the agent slots (maxcols public columns at the most) and the X area (k columns) are sized by the larger of the
  // two, so that the job can lift up to it without another segment; every other area does not depend on the rank.
  static int rank_capacity(int r, int reserve_r) { return r > reserve_r ? r : reserve_r; }
  static size_t slot_doubles(size_t maxcols, int r, int reserve_r) {
    return (maxcols * (size_t)rank_capacity(r, reserve_r) + 15) / 16 * 16;
  }
  static SegmentLayout for_job(int world_, int R_, size_t maxcols, int r, int reserve_r, size_t k, size_t w_doubles_) {
    return SegmentLayout(world_, R_, slot_doubles(maxcols, r, reserve_r), (size_t)rank_capacity(r, reserve_r) * k,
                         w_doubles_);
  }

  template <class T>
  static T *at(void *base, size_t off, size_t index = 0) {
    return (T *)((char *)base + off) + index;
  }
  ShmHeader *header(void *b) const { return at<ShmHeader>(b, 0); }
  ShmRank *rank_record(void *b, int rank) const { return at<ShmRank>(b, off_ranks, (size_t)rank); }
  ShmFlag *flag(void *b, int parity, int agent) const { return at<ShmFlag>(b, off_flags, (size_t)parity * R + agent); }
  ShmEval *eval(void *b, int parity, int agent) const {
    return at<ShmEval>(b, off_evals, (size_t)parity * ((size_t)R + world) + agent);
  }
  ShmEval *heartbeat(void *b, int parity, int rank) const { return eval(b, parity, R + rank); }
  ShmFlag *consumed(void *b, int reader, int agent) const {  // the last post of the agent that rank has scattered
    return at<ShmFlag>(b, off_consumed, (size_t)reader * R + agent);
  }
  ShmRed *red(void *b, int parity, int rank) const { return at<ShmRed>(b, off_red, (size_t)parity * world + rank); }
  ShmStatus *status(void *b, int parity, int agent) const {
    return at<ShmStatus>(b, off_status, (size_t)parity * R + agent);
  }
  ShmFlag *status_read(void *b, int reader, int agent) const {  // the last status of the agent that rank has read
    return at<ShmFlag>(b, off_status_read, (size_t)reader * R + agent);
  }
  ShmFlag *probe_flag(void *b, int reader, int writer) const {
    return at<ShmFlag>(b, off_probe_flags, (size_t)reader * world + writer);
  }
  ShmFlag *probe_result(void *b, int reader, int writer) const {
    return at<ShmFlag>(b, off_probe_res, (size_t)reader * world + writer);
  }
  double *probe_stage(void *b, int reader, int writer) const {
    return at<double>(b, off_probe_stage, ((size_t)reader * world + writer) * kProbeDoubles);
  }
  double *staged(void *b, int parity, int agent) const {
    return at<double>(b, off_staged, ((size_t)parity * R + agent) * slot);
  }
  double *x(void *b) const { return at<double>(b, off_x); }        // r x (d+1) n
  double *weights(void *b) const { return at<double>(b, off_w); }  // m doubles in dataset order, written by the owners
};

// ---- the one bounded wait -------------------------------------------------------------------------------------------
using Clock = std::chrono::steady_clock;
inline double since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

enum { kWaitOk = 0, kWaitPeerFailed = 1, kWaitTimeout = 2, kRehearsalMismatch = 3 };

// Poll until ready(), giving up when the job's `failed` word is raised or `timeout_s` after `t0` (waits that belong to
// one step share one Wait and with it one clock); the acquire that makes the awaited stores readable comes with kWaitOk.
// The caller turns the other codes into its error text, and decides whether giving up raises `failed`.
struct Wait {
  const std::atomic<uint32_t> *failed;
  double timeout_s;
  Clock::time_point t0 = Clock::now();

  // back-off: a burst of pause instructions, then the core is handed over between polls (a rank per core is not
  // guaranteed: the four-ranks-on-one-GPU rehearsal runs on whatever cores the container has)
  static void polite_spin(unsigned &spins) {
    ++spins;
    if (spins < 2048u) {
      __builtin_ia32_pause();
    } else if (spins < 8192u) {
      sched_yield();
    } else {
      usleep(50);
    }
  }
  template <class Ready>
  int until(Ready &&ready) const {
    unsigned spins = 0;
    while (!ready()) {
      polite_spin(spins);
      if ((spins & 1023u) == 0) {
        if (failed->load()) return kWaitPeerFailed;
        if (since(t0) > timeout_s) return kWaitTimeout;
      }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return kWaitOk;
  }
  int reached(const volatile uint64_t &word, uint64_t want) const {
    return until([&] { return word >= want; });
  }
};

// ---- the host steps, over one rank's host view of the segment -------------------------------------------------------
// A step that waits for several ranks or agents says in *whom (may be null) which one it gave up on.
struct ExchangeSlots {
  SegmentLayout lay;
  void *base = nullptr;
  int rank = 0;
  double timeout_s = 120.0;  // how long a rank waits for another before it gives up

  ShmHeader *header() const { return lay.header(base); }
  Wait wait(double budget_s) const { return Wait{&header()->failed, budget_s}; }
  Wait wait() const { return wait(timeout_s); }

  // -- public poses.  Post q of agent a (q counts from 1, the same on every rank) goes into slot [q & 1][a], last
  // written by post q - 2: before the producer overwrites it, every rank that reads it must have scattered that post
  // (ticks of one set posted again and again and the per-phase C ABI have no evaluation between two posts).
  int consumed_wait(const Wait &w, int agent, uint64_t q, const int *readers, int count, int *whom) const {
    for (int i = 0; q > 2 && i < count; ++i)
      if (const int rc = w.reached(lay.consumed(base, readers[i], agent)->seq, q - 2)) {
        if (whom) *whom = readers[i];
        return rc;
      }
    return kWaitOk;
  }
  int flag_wait(const Wait &w, int agent, uint64_t q) const {
    return w.reached(lay.flag(base, (int)(q & 1), agent)->seq, q);
  }

  // -- the evaluation.  Heartbeat: every rank -- also one that hosts no agent and therefore publishes nothing -- says
  // that it has entered evaluation `want`, and nobody leaves it before all have.  A rank can then never be lapped: the
  // slot of parity `want` is overwritten at evaluation want + 2, which every writer enters only after all ranks have
  // entered want + 1, i.e. after they have finished reading `want`.
  int heartbeat(const Wait &w, uint64_t want, int *whom) const {
    std::atomic_thread_fence(std::memory_order_release);
    lay.heartbeat(base, (int)(want & 1), rank)->seq = want;
    for (int p = 0; p < lay.world; ++p)
      if (const int rc = w.reached(lay.heartbeat(base, (int)(want & 1), p)->seq, want)) {
        if (whom) *whom = p;
        return rc;
      }
    return kWaitOk;
  }
  // the gather: every agent's two scalars, summed in agent order (the same bits on every rank)
  int eval_gather(const Wait &w, uint64_t want, double *cost2, double *gradnorm, double *block_norms, int *next_selected,
                  int *whom) const {
    double g2 = 0, c2 = 0, best = -1;
    int arg = 0;
    for (int a = 0; a < lay.R; ++a) {
      const ShmEval *e = lay.eval(base, (int)(want & 1), a);
      if (const int rc = w.reached(e->seq, want)) {
        if (whom) *whom = a;
        return rc;
      }
      const double ga = e->g2, xa = e->xeg;
      const double nb = std::sqrt(ga);
      if (block_norms) block_norms[a] = nb;
      g2 += ga;
      c2 += xa;  // 2 f = sum_b <X_b, X_b Q_bb + G_b>
      if (nb > best) {
        best = nb;
        arg = a;
      }
    }
    if (cost2) *cost2 = c2;
    if (gradnorm) *gradnorm = std::sqrt(g2);
    if (next_selected) *next_selected = arg;
    return kWaitOk;
  }

  int barrier(double budget_s) const {
    ShmHeader *h = header();
    if (lay.world == 1) return kWaitOk;
    const Wait w = wait(std::min(budget_s, timeout_s));
    const uint32_t gen = h->bar_gen.load(std::memory_order_acquire);
    if (h->bar_count.fetch_add(1, std::memory_order_acq_rel) + 1 == (uint32_t)lay.world) {
      h->bar_count.store(0, std::memory_order_relaxed);
      h->bar_gen.fetch_add(1, std::memory_order_release);
      return kWaitOk;
    }
    return w.until([&] { return h->bar_gen.load(std::memory_order_acquire) != gen; });
  }
  // sum number q of the job: `count` (<= 31) doubles over the ranks, added in rank order (the same bits on every rank)
  int allreduce_sum(const Wait &w, uint64_t q, double *vals, int count, int *whom) const {
    if (lay.world == 1) return kWaitOk;
    ShmRed *mine = lay.red(base, (int)(q & 1), rank);
    for (int i = 0; i < count; ++i) mine->vals[i] = vals[i];
    std::atomic_thread_fence(std::memory_order_release);
    mine->seq = q;
    double acc[31] = {0};
    for (int p = 0; p < lay.world; ++p) {
      const ShmRed *s = lay.red(base, (int)(q & 1), p);
      if (const int rc = w.reached(s->seq, q)) {
        if (whom) *whom = p;
        return rc;
      }
      for (int i = 0; i < count; ++i) acc[i] += s->vals[i];
    }
    for (int i = 0; i < count; ++i) vals[i] = acc[i];
    return kWaitOk;
  }

  // -- the team's statuses.  Optimisation q of agent a goes into slot [q & 1][a], last used by q - 2.  Before the
  // hosting rank touches it, it waits (bounded) until every rank's read word of the agent has reached q - 2: that one
  // wait closes the hazard for ticks, which have no evaluation behind them and whose posts are scattered before the
  // status is read.  Greedy iterations would not need it -- nobody leaves evaluation k before everybody has entered it,
  // and a rank says it has entered only after it has read status k, so even one slot per agent would do there; the
  // word is then always there already and the wait costs one load per rank.  (rbcd_iterate reads the status inside
  // evaluate, after the evaluation's kernels are enqueued and before its heartbeat: read before them, the hosting
  // rank's host waited for its own update and its queue ran dry -- 18 us per iteration instead of the launch's 6.)
  ShmStatus *status_slot(uint64_t q, int agent) const { return lay.status(base, (int)(q & 1), agent); }
  // the writer's back-pressure: every rank has read optimisation `upto` of the agent
  int status_read_wait(int agent, uint64_t upto, int *whom) const {
    for (int p = 0; p < lay.world; ++p)
      if (const int rc = wait().reached(lay.status_read(base, p, agent)->seq, upto)) {
        if (whom) *whom = p;
        return rc;
      }
    return kWaitOk;
  }
  // the reader's wait: the slot holds optimisation q of the agent
  int status_wait(uint64_t q, int agent) const { return wait().reached(status_slot(q, agent)->seq, q); }
  void mark_status_read(uint64_t q, int agent) const {
    std::atomic_thread_fence(std::memory_order_release);
    lay.status_read(base, rank, agent)->seq = q;
  }

  // -- what the device stores, from the host (the rehearsals only): k_post_public's slot and flag, k_wait_scatter's
  // consumed word, k_eval_publish's scalars, the hosting rank's host and its ranked k_rel_change
  static double rehearsal_payload(uint64_t q, int agent, size_t i) { return 1000.0 * (double)q + 16.0 * agent + (double)i; }
  void post_from_host(uint64_t q, int agent) const {
    double *dst = lay.staged(base, (int)(q & 1), agent);
    for (size_t i = 0; i < lay.slot; ++i) dst[i] = rehearsal_payload(q, agent, i);
    std::atomic_thread_fence(std::memory_order_release);
    lay.flag(base, (int)(q & 1), agent)->seq = q;
  }
  bool scatter_from_host(uint64_t q, int agent) const {  // false: the payload is not post q's
    const double *src = lay.staged(base, (int)(q & 1), agent);
    for (size_t i = 0; i < lay.slot; ++i)
      if (src[i] != rehearsal_payload(q, agent, i)) return false;
    std::atomic_thread_fence(std::memory_order_release);
    lay.consumed(base, rank, agent)->seq = q;
    return true;
  }
  void eval_from_host(uint64_t want, int agent, double g2, double xeg) const {
    ShmEval *e = lay.eval(base, (int)(want & 1), agent);
    e->g2 = g2;
    e->xeg = xeg;
    std::atomic_thread_fence(std::memory_order_release);
    e->seq = want;
  }
  void status_from_host(uint64_t q, int agent, bool success, double rel) const {
    ShmStatus *s = status_slot(q, agent);
    s->success = success ? 1u : 0u;
    s->rel = rel;
    std::atomic_thread_fence(std::memory_order_release);
    s->seq = q;
  }
};

// The exchange's rehearsal.  Round q = 1 .. rounds is one iteration's traffic with every agent posting (agent a lives
// on rank a / per): the owners wait until post q - 2 has been read everywhere and post; every rank waits for every
// flag, checks the payload and says so in its consumed word; the owners publish g2 = q + a / 2, xeg = q / 4 - a; then
// the heartbeat, the gather and one sum of {rank + 1, q} over the ranks, all on the round's one clock.  checksum folds
// what the gather returned: sum of (a + 1) g2_a + xeg_a.  *what (may be null): what a result other than kWaitOk means.
inline int exchange_rehearsal(const ExchangeSlots &s, int per, int rounds, double *checksum, const char **what) {
  const int R = s.lay.R, world = s.lay.world;
  std::vector<int> everybody((size_t)world);
  for (int p = 0; p < world; ++p) everybody[(size_t)p] = p;
  std::vector<double> norms((size_t)R);
  const char *unused;
  if (!what) what = &unused;
  double sum = 0;
  for (uint64_t q = 1; q <= (uint64_t)rounds; ++q) {
    const Wait w = s.wait();
    for (int a = 0; a < R; ++a) {
      if (a / per != s.rank) continue;
      *what = "host selftest: a post was never read";
      if (const int rc = s.consumed_wait(w, a, q, everybody.data(), world, nullptr)) return rc;
      s.post_from_host(q, a);
    }
    for (int a = 0; a < R; ++a) {
      *what = "host selftest: a post never arrived";
      if (const int rc = s.flag_wait(w, a, q)) return rc;
      *what = "host selftest: payload mismatch";
      if (!s.scatter_from_host(q, a)) return kRehearsalMismatch;
    }
    for (int a = 0; a < R; ++a)
      if (a / per == s.rank) s.eval_from_host(q, a, (double)q + 0.5 * a, (double)q * 0.25 - a);
    *what = "host selftest: a heartbeat never arrived";
    if (const int rc = s.heartbeat(w, q, nullptr)) return rc;
    double c2 = 0;
    *what = "host selftest: an evaluation never arrived";
    if (const int rc = s.eval_gather(w, q, &c2, nullptr, norms.data(), nullptr, nullptr)) return rc;
    sum += c2;
    for (int a = 0; a < R; ++a) sum += norms[(size_t)a] * norms[(size_t)a] * (a + 1);
    double v[2] = {(double)(s.rank + 1), (double)q};
    *what = "host selftest: a rank never joined a sum";
    if (const int rc = s.allreduce_sum(w, q, v, 2, nullptr)) return rc;
    *what = "host selftest: sum mismatch";
    if (v[0] != 0.5 * world * (world + 1) || v[1] != (double)q * world) return kRehearsalMismatch;
  }
  if (checksum) *checksum = sum;
  return kWaitOk;
}

// The team's rehearsal.  Round q = 1 .. rounds: a tick of the agents a with a % 2 == (q / 3) % 2 when q % 3 == 0, else
// agent q % R alone followed by the evaluation's heartbeat (nobody leaves it before everybody has entered it).  Agent a
// lives on rank a / per.  Its owner publishes success = (q + a) % 5 != 0 and relative change 0.001 ((7 q + 3 a) % 11).
// Every rank settles the status (robust team, 4 accepted and min(updates, 2) rejected of 6 loop closures, the default
// parameters with 3 weight updates, 7 inner iterations and no iteration cap), decides, and applies an update's
// bookkeeping when the rules ask for one.  Rank k sleeps k * skew_us at the start of a round.
inline int team_rehearsal(const ExchangeSlots &t, int per, int rounds, int skew_us, double *checksum) {
  const int R = t.lay.R;
  dcora_team_params p = team_params_default();
  p.max_num_iters = 1 << 30;
  p.robust_opt_num_weight_updates = 3;
  p.robust_opt_inner_iters = 7;
  std::vector<dcora_agent_status> status((size_t)R, dcora_agent_status{});
  std::vector<int> have((size_t)R, 0);
  std::vector<uint64_t> seq((size_t)R, 0);
  int updates = 0, inner = 0, latest = 0;
  uint64_t beats = 0;
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
        if (const int rc = t.status_read_wait(a, k - 2, nullptr)) return rc;
      t.status_from_host(k, a, (q + a) % 5 != 0, 0.001 * (double)((7 * q + 3 * a) % 11));
    }
    for (int a : set) {
      const uint64_t k = seq[(size_t)a];
      if (const int rc = t.status_wait(k, a)) return rc;
      const ShmStatus *slot = t.status_slot(k, a);
      dcora_agent_status &st = status[(size_t)a];
      st = dcora_agent_status{};
      st.agent_id = a;
      st.state = DCORA_AGENT_INITIALIZED;
      st.iteration_number = q;
      st.relative_change = slot->rel;
      st.ready_to_terminate =
          team_ready_to_terminate(p, true, updates, slot->success != 0, st.relative_change, 4, rejected, 6) ? 1 : 0;
      have[(size_t)a] = 1;
      t.mark_status_read(k, a);
    }
    if (!tick)
      if (const int rc = t.heartbeat(t.wait(), ++beats, nullptr)) return rc;
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
  return kWaitOk;
}

}  // namespace dcora
