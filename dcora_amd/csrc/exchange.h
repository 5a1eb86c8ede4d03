// Neighbour exchange of public poses between the ranks of ONE node (one process per GPU), inside the library
// (replaces the transport the reference leaves to its host: Agent::getSharedStateDicts -> updateNeighborStates,
// ref src/Agent.cpp:113-152, 844-906, driven by examples/MultiRobotExample.cpp:236-258).
//
// Transport: every rank owns a halo buffer in its HBM with one slot per agent; the peers map
// it through HIP IPC.  A post is ONE kernel per hosted agent: it gathers the agent's public poses from the mirror of
// X and stores them straight into the halo slot of every rank that hosts a neighbour of that agent (peer stores over
// xGMI), fences at system scope and lets its last workgroup store the agent's sequence number into a flag word.  Flag
// words and the 2R evaluation scalars live in a POSIX shared-memory segment that every rank registers with HIP
// (device-writable, host-readable): a device store there IS the all-gather.  The receiving host spins on the flag
// word and enqueues the scatter into its mirror.  No collective, no ring, no host copy of pose data.
// When IPC mapping (or its self-test) fails on any rank, all ranks fall back to staging the packed poses in the same
// shared host segment (device store over PCIe, device load over PCIe on the consumer).
// The host half of the protocol -- the segment's layout, the bounded wait and every host step -- is stated once in
// exchange_slots.h (no HIP); this class wraps the steps with its error texts and statistics and launches the kernels.
#pragma once
#include <functional>
#include <string>
#include <vector>

#include "cert_rows.h"
#include "exchange_slots.h"
#include "session_core.h"

namespace dcora {

enum ExchangeMode { kExchangeIpc = 1, kExchangeStaged = 2 };

// how long a rank waits for another before it gives up, raises `failed` for everybody and returns an error
// (DCORA_EXCHANGE_TIMEOUT_S, default 120: a rank that died takes the job down within this time, never a hang)
double exchange_timeout_s();
extern std::atomic<int> g_probe_fault_rounds;  // test hook of the link check (dcora_debug_exchange_probe_fault)
// test / measurement hook of Exchange::project (dcora_debug_exchange_project_sums): the per-agent Gram matrices travel
// through allreduce_sum pieces instead of the X area
extern std::atomic<int> g_project_gram_sums;

// What certify_live keeps between certificates: the job-wide pattern of S + eta I and, per hosted agent, the table of
// its rows (cert_rows.h) on the device.  Built by the first call; valid for the life of the job.
struct LiveCertState {
  struct Agent {
    int id = 0;
    std::vector<int> pos_host;  // the table's positions, ascending: which entries a window takes
    DevBuf<int> pos, src, slot;
    DevBuf<unsigned char> diag;
  };
  bool built = false;
  HostCsr pat;                 // v: where the values land on rank 0 when the PSD test has refused
  std::vector<Agent> agents;   // the hosted ones, in agent order
  DevBuf<double> vals;         // rank 0: the values of S + eta I in pat's CSR order
  hipEvent_t ready = nullptr;  // rank 0: vals complete (the factorisation runs on a stream of its own)
  LiveCertState() = default;
  LiveCertState(const LiveCertState &) = delete;
  LiveCertState &operator=(const LiveCertState &) = delete;
  ~LiveCertState() {
    if (ready) (void)hipEventDestroy(ready);
  }
};

class Exchange {
 public:
  ~Exchange();
  // weights: doubles of the segment's weights area (the m weights of a robust job, dcora_rbcd_create_robust_ranks /
  // dcora_ra_rbcd_create_robust_ranks)
  int init(SessionCore *s, const char *job_name, size_t weights = 0);
  int post(const int *agents, int count);
  int wait(const int *agents, int count);
  int post_arr(const int *agents, int count, int r, const double *arr);
  int wait_arr(const int *agents, int count, int r, double *arr);
  // sum of `count` (<= 31) doubles over the ranks, added in rank order: the same bits on every rank
  int allreduce_sum(double *vals, int count);
  // Certification across the ranks ("Collective"): fastVerification (ref src/DCORA_utils.cpp:1713-1735)
  // of the current iterate.  The PSD test runs on rank 0 (it assembles S from the gathered X and the global Q it is
  // given; Qglobal may be null on the other ranks); when it fails, the minimum eigenpair of S + eta I is computed by
  // ALL ranks: each applies its row block of S (its agents' Q_bb and coupling blocks, the Lambda blocks of its poses)
  // to its slice of the Lanczos vectors, the public entries travel like public poses, every inner product is an
  // allreduce_sum.  v (may be null): the eigenvector, (d+1) n doubles, the same on every rank.
  int certify(const HostCsr *Qglobal, double eta, int *certified, double *theta, double *lambda_min, double *v,
              long long *matvecs, int *distributed);
  // The same certificate from the matrices the ranks hold on the device NOW (dcora_exchange_certify_live): no Q is
  // passed in and no X crosses to a host.  Every rank forms the values of its own rows of M = (Q - Lambda) + eta I in
  // the CSR order of the job-wide pattern (k_cert_rows, gather form, no atomics); they reach rank 0 through the X area
  // of the segment in rounds of x_doubles entries (kernel end, stream synchronise, barrier, copy, barrier); rank 0
  // factorises them where they land.  Refused: the row-block Lanczos stage of certify, with M downloaded once on
  // rank 0.  info10 (may be null): the PSD test's eight, the rounds, ms from entry to the verdict on rank 0.
  int certify_live(double eta, int *certified, double *theta, double *lambda_min, double *v, long long *matvecs,
                   int *distributed, double *info10);
  int evaluate(double *cost2, double *gradnorm, double *block_norms, int *next_selected);
  int rbcd_iterate(int selected, double *cost2, double *gradnorm, double *block_norms, int *next_selected);
  int rbcd_tick(const int *set, int count, int allow_adjacent);
  // coloured sweeps across the ranks (run_coloured_sweeps): rbcd_tick per colour of the greedy colouring, then evaluate
  int run_coloured(int max_sweeps, double rgrad_tol, int *sweeps_done, double *cost2_trace, double *gradnorm_trace);
  // Robust jobs (the exchange's session was created by init_robust(..., ranked = true), of either kind: the session's
  // part comes through SessionCore's weight hooks): Agent::updateMeasurementWeights of every agent on every rank.  Each
  // rank weights the edges touching its agents from its mirror, the owners store theirs into the weights area, counts
  // are summed over the ranks.  Weights are in the job's order: the dataset's, or a range-aided one's pose-pose.
  int update_weights(bool reset_to_initial, int counts[3]);
  int set_weights(const double *w);  // all m weights, the same on every rank
  int get_weights(double *w);        // all m weights of the job, from the weights area
  int publish_weights();             // the owned edges' current weights into the area (creation)
  // ---- the team protocol across the ranks (dcora_exchange_team_enable on a pose-graph job, dcora_exchange_team_enable_ra
  // on a range-aided one; everything after the enabling call is the same for both kinds) ----
  // Every rank keeps every agent's status (TeamState, ranked).  Of an optimisation only two facts are not known
  // everywhere: whether it succeeded and its relative change.  The hosting rank stores the first from the host, the
  // ranked k_rel_change behind the agent's update stores the second and then the slot's sequence word; every rank
  // (the hosting one too) collects them inside the collective call and settles the status by the same rule.
  // (Slot re-use and the back-pressure on the read words: exchange_slots.h, at the steps.)
  // range_aided: which of the two entries calls; each serves its own session kind and refuses the other's exchange
  int team_enable(const dcora_team_params &p, bool range_aided);
  bool team_on() const { return s_ && s_->team && s_->team->ranked; }
  SessionCore *team_session() const { return team_on() ? s_ : nullptr; }
  int run_team(int *iters_done, double *cost2_trace, double *gradnorm_trace, int *selected_trace, int *updated_trace,
               int *weight_updates, int *stop_reason);
  // the same slots and waits without a device (host stores stand in for the kernel's): rounds of one agent (round % R)
  // behind an evaluation heartbeat, every third round a tick of non-adjacent agents without one; every rank collects,
  // settles and decides by team_rules.h; checksum folds every status and both decisions of every round
  int host_selftest_team(const char *job_name, int rank, int world, int R, int rounds, int skew_us, double *checksum);
  // The Riemannian staircase's step across the ranks (SessionCore::lift's contract carried over the job; ref
  // examples/MultiRobotExample.cpp:352-366, src/QuadraticProblem.cpp:138-234).  SPMD: every rank calls it with the same
  // theta, v (k doubles, global ordering, as certify returns it) and parameters.  The search is EscapeSearch
  // (escape_rule.h), one statement for this and the single-process lift.  Per trial every rank retracts the blocks of
  // its hosted agents at rank r + 1 (SessionCore::lift_trial_point), the public columns travel with the ordinary post
  // and wait of all agents at r + 1 rows, and the trial's three scalars -- 2 f, |rgrad|^2, |P grad|^2 -- are each
  // rank's sums over its agents in agent order, added over the ranks in rank order (allreduce_sum): the same bits
  // and so the same branch on every rank.  f([X; 0]) is the same evaluation of the current iterate.
  // The preconditioned norm is NOT escapeSaddle's: no rank holds the whole graph, so
  //   |P grad|^2 := sum_a |Proj(rgrad_a M_a^-1)|^2,  M_a^-1 the image agent a's solves use (its own regularisation);
  // p.central_reg is ignored.  A one-rank exchange takes this same path.
  // Escaped: every hosted problem is at r + 1, the kind's buffers are re-dimensioned and the accepted point is adopted
  // on every rank at once, between barriers as set_X does, with set_X's consequences; matrices, preconditioners,
  // weights, mu and its update count, team parameters and counts, and this exchange with its transport stay.  No
  // escape, or an error on any rank: every problem is back at r, the session's mirror was never written (the trials
  // ran in a mirror of their own).  Refused alike on every rank, the job untouched: r = 16, v null or not finite,
  // theta or a tolerance not finite (DCORA_ERR_BAD_ARG); r + 1 beyond max(r at creation, reserve)
  // (DCORA_ERR_UNSUPPORTED).  info8 (may be null): trials, accepted alpha, f before, f after, 0, 0, ms of the
  // re-dimensioning, ms total.
  int lift(double theta, const double *v, const dcora_lift_params &p, int *escaped, double *info8);
  // The last step of a solve across the ranks (ref examples/MultiRobotExample.cpp:341-347,
  // examples/MultiRobotExample_RASLAM.cpp:488-495, src/Agent.cpp:1014-1033): SessionCore::round's rounding, every state
  // by the rank that hosts it (a rank's mirror is current only in its hosted and the neighbours' public columns).  SPMD.
  // An anchor named by anchor_pose travels from its hosting rank through allreduce_sum -- zeros from the others, pieces
  // of at most 31 doubles, added in rank order: x + 0 keeps x's bits, a -0 arrives as +0 and changes no sum --, a passed
  // one (r x (d + 1), host) is every rank's as it is.  The pieces are assembled through the X area as gather_X
  // assembles X (d / r of its room); every rank returns everything.  No rounded cost: no rank holds a central problem.
  // Refused before any collective step, alike on every rank (DCORA_ERR_BAD_ARG): trajectory null, anchor_pose outside
  // 0 .. n - 1, a non-finite anchor.
  int round(int anchor_pose, const double *anchor, double *trajectory, double *unit_spheres, double *landmarks);
  // How CORA ends a certified solve, across the ranks (SessionCore::project's contract carried over the job; ref
  // examples/SingleRobotExample_RASLAM.cpp:220-234, projectSolutionRASLAM src/DCORA_utils.cpp:1984-2031).  SPMD.
  //   a. every rank drains its session;
  //   b. G = X X^T = sum_a G_a: every rank forms G_a of the agents it hosts from their own blocks in one launch pair
  //      (launch_gram_blocks); the matrices reach every rank per agent and unchanged (project_sum_grams) and every rank
  //      adds them in agent order 0 .. R - 1.  A rank never sums its own agents first: G has the same bits on every
  //      rank, for any number of ranks, either transport and a one-rank exchange.  (Not the single-process session's G
  //      bit for bit unless R = 1: that one sums workgroups over the whole mirror's columns.)
  //   c. the r x r eigenproblem on every rank's host: the same input, the same code, the same V_d; no broadcast;
  //   d. r == d: X passes through; sigma and gram are produced, cost2 and |rgrad| are evaluate()'s, the job is untouched;
  //   e. poses with det(V_d^T Y_i) > 0 over the hosted blocks, summed as doubles (allreduce_sum: integers, exact); the
  //      reflection rule on the JOB's n, the same branch everywhere;
  //   f. the hosted blocks projected into a zeroed trial mirror of d rows, everybody's public columns at d rows through
  //      post_arr / wait_arr of all agents, as lift's trial points travel;
  //   g. between barriers, as lift commits: every hosted problem (and a one-rank job's central one) re-ranked to d, the
  //      session re-dimensioned at the trial mirror.  What lift keeps is kept -- r_cap_ too: a projected job can lift
  //      again up to its old capacity; certify_live's tables stay valid;
  //   h. cost2 and info8[3]: evaluate() at the adopted point, what a following evaluate returns bit for bit.
  // An error on any rank before the commit: nothing of its session was written, `failed` is raised for the ranks that
  // wait.  Outputs as SessionCore::project, every one may be null and every one but the three times of info8 has the
  // same bits on every rank; info8[2] counts over the job.
  int project(double *sigma, double *basis, double *gram, double *cost2, double *info8);
  int rank_capacity() const { return r_cap_; }  // the largest rank the job's segment and halo slots hold
  int barrier(double timeout_s = 120.0);
  int gather_X(double *Xh);
  // Agent::setX of every agent on every rank: sequence numbers restart with the Nesterov sequences
  int set_X(const double *Xh);
  // host half of the protocol alone, without a GPU: the bootstrap, then exchange_rehearsal (exchange_slots.h) -- the
  // steps post_arr, wait_arr, evaluate and allreduce_sum make, host stores standing in for the device's
  int host_selftest(const char *job_name, int rank, int world, int R, int rounds, double *checksum);
  // test hook: what a crashed job of this shape leaves behind under the name (initialised, creator gone)
  int debug_leave_stale(const char *job_name, int world, int R);

  int mode = 0;
  int rank = 0, world = 1;
  // link check (init): rounds run, whether the device-side wait / the IPC transport were given up, time of the last round
  int link_rounds = 0, link_gave_up_device_wait = 0, link_gave_up_ipc = 0;
  double link_last_us = 0;
  bool halo_is_finegrained() const { return halo_finegrained_; }
  // statistics since creation (host wall time spent in post / wait / the evaluation all-gather, bytes posted)
  bool waits_on_device() const { return device_wait_; }
  double post_s = 0, wait_s = 0, eval_wait_s = 0;
  long posts = 0, waits = 0, evals = 0;
  double bytes_posted = 0;
  int num_peers() const;

 private:
  SessionCore *s_ = nullptr;
  std::string name_;
  SegmentLayout lay_;        // where every area of the segment lies (exchange_slots.h)
  void *map_ = nullptr;      // host view of the segment
  char *dev_map_ = nullptr;  // device view of it: kernel arguments are lay_'s accessors on this base
  bool registered_ = false;
  ShmHeader *hdr_ = nullptr;
  uint64_t red_seq_ = 0;
  std::vector<double> job_w_;        // the job's weights as of the last weight change (the team's loop-closure counts)
  std::vector<int> team_due_;        // agents whose status the evaluation of this rbcd_iterate has to collect
  int team_clear_to_write(const int *agents, int count);  // before the agents optimise: their slots may be overwritten
  int team_collect(const int *agents, int count);         // after their posts: every rank reads and settles
  ExchangeSlots slots() const { return ExchangeSlots{lay_, map_, rank, exchange_timeout_s()}; }
  ShmRank &rank_record(int q) const { return *lay_.rank_record(map_, q); }
  int wait_failed(int what, const std::string &who);  // a kWait* result as this exchange's failure (`who`: timed out)
  void team_snapshot_weights();
  size_t probe_off_ = 0;  // in a halo buffer: [writer] x (kProbeDoubles payload + 8 doubles of flag)
  size_t devflag_off_ = 0;       // in a halo buffer, behind the slots and the self-test area: [parity][agent] x 64 bytes
  bool device_wait_ = true;      // the scatter kernel polls the flag itself (no host hop between post and scatter)
  DevBuf<unsigned> arrive2_;     // last-workgroup counters of the scatter kernels
  int R_ = 0;
  int r_cap_ = 0;                  // max(the session's rank at creation, its reserve): what slot_ and the X area hold
  size_t slot_ = 0;                // doubles per agent slot
  DevBuf<double> halo_;            // [parity][agent][slot] + self-test area (fine-grained device memory)
  bool halo_finegrained_ = false;
  double *peer_halo_[kMaxRanks]{};  // IPC mappings (null for myself and for ranks I never write to)
  bool opened_[kMaxRanks]{};
  DevBuf<unsigned> arrive_;        // one last-workgroup counter per agent
  DevBuf<double> evalbuf_;         // 2R
  DevBuf<int> hosted_list_;
  int n_hosted_ = 0;
  std::vector<int> owner_;               // rank hosting agent a
  std::vector<std::vector<int>> dests_;  // for a hosted agent: the other ranks hosting one of its neighbours
  std::vector<char> needed_;             // agent a (hosted elsewhere) is a neighbour of an agent hosted here
  std::vector<uint64_t> seq_;            // posts of agent a so far (identical on every rank)
  uint64_t eval_seq_ = 0;

  size_t halo_off(int parity, int agent) const { return ((size_t)parity * R_ + agent) * slot_; }
  int open_segment(const char *job_name);
  int map_segment(const char *job_name, size_t x_doubles, size_t w_doubles = 0);
  int selftest_bootstrap(const char *job_name, int rank, int world, int R, bool args_ok);
  int setup_ipc(bool attempt);
  int link_check();
  bool probe_round(uint64_t seq, std::string *why);
  // the two halves both certificates share (exchange_cert.hip): post and wait of all agents with the Lambda blocks of
  // the hosted ones; the minimum eigenpair of M = S + eta I by all ranks once the PSD test has refused (M: rank 0's).
  // skip_hopeless: the plan's shortcut past the spectrum-shifted run (min_eig_plan.h, Shortcut::when_asked) is asked
  // for -- certify_live's choice; certify keeps making the run.  share_whole_vector: one vector of the whole problem
  // through the segment's X area, to every rank
  struct CertRows;
  int cert_rows_begin(CertRows *rows);
  int cert_min_eigenpair(CertRows &rows, const HostCsr &M, double eta, bool skip_hopeless, double *theta,
                         double *lambda_min, double *v, long long *matvecs, int *distributed);
  int share_whole_vector(const std::function<void(double *x_area)> &store, double *whole);
  int live_cert_build();  // the pattern and the tables, on the first certify_live
  int certify_live_run(double eta, int *certified, double *theta, double *lambda_min, double *v, long long *matvecs,
                       int *distributed, double *info10);  // certify_live behind its refusals
  LiveCertState live_;
  // project's step b (exchange_project.hip): mine = the hosted agents' r x r matrices in agent order -> *G, their sum
  // over all agents in agent order
  int project_sum_grams(const std::vector<int> &hosted, const std::vector<double> &mine, int r, std::vector<double> *G);
  int fail(const std::string &msg, int code);   // a transport / peer failure: raises `failed` for every rank
  int usage(const std::string &msg, int code);  // a refused call (bad argument, unsupported): this call only
};

}  // namespace dcora
