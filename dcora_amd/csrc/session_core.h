// What the pose-graph session (rbcd.h) and the range-aided one (ra_rbcd.h) share, stated once: the agent state every
// RBCD agent has, the Nesterov sequences, the colouring, and the tick (simultaneous updates of a set of agents).  It is
// also all the in-library exchange (exchange.h) needs from a session, so the same transport -- peer stores into
// IPC-mapped halo buffers, flag words and evaluation scalars in the shared segment -- carries both kinds (ref
// src/Agent.cpp:113-152, 844-906: getSharedStateDicts / updateNeighborStates are the same calls on either graph type).
// Where a hosted agent's block lies (agent_block), how a session changes rank (RankChange, redimension) and what "nothing
// of the session is in flight" means (drain) are stated here once, for the session's own calls and for the exchange's.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "agent_block.h"
#include "device_problem.h"
#include "host_robust.h"
#include "rank_change.h"
#include "robust.h"
#include "session_cert.h"
#include "session_project.h"
#include "session_round.h"
#include "team_rules.h"

namespace dcora {

struct AgentCore {
  bool hosted = false;                  // lives on this rank (agent a on rank a / ceil(R / world_size))
  std::unique_ptr<DeviceProblem> prob;  // Q_aa, its preconditioner, solver workspace (hosted agents only)
  DevCsr coupling;                      // rows: my columns (my ordering), cols: global columns (hosted agents only)
  DevBuf<int> public_cols;              // my columns of the mirror that OTHER agents' measurements reach (all agents)
  int n_public_cols = 0;
  std::vector<int> neighbors;           // agents sharing a measurement with me (all agents)
  hipStream_t own_st = nullptr;         // stream of my solve when several agents update at once (hosted agents only;
  hipEvent_t done = nullptr;            // both owned by the session)
};

// Team protocol of a session that called dcora_rbcd_team_enable / dcora_ra_rbcd_team_enable, or whose exchange called
// dcora_exchange_team_enable / _team_enable_ra (ranked, below): every agent's status as Agent::iterate(true) stores it
// (ref src/Agent.cpp:558-586) and the bookkeeping Agent::updateMeasurementWeights does on it (:1417-1424).  The relative
// change comes from k_rel_change, in the session kind's form of it, through host-mapped memory: a status is `pending` from its launch until the host has seen the stream pass it (an evaluation the host has
// waited for, or a synchronisation in the query), then it is settled by team_ready_to_terminate with what the agent
// knew when it optimised.
struct TeamState {
  dcora_team_params params{};
  double *rel_host = nullptr, *rel_dev = nullptr;  // kMaxAgents relative changes, written by k_rel_change
  TeamState() = default;
  TeamState(const TeamState &) = delete;
  TeamState &operator=(const TeamState &) = delete;
  ~TeamState() {
    if (rel_host) (void)hipHostFree((void *)rel_host);
  }
  std::vector<dcora_agent_status> status;          // by agent; have[b] == 0: none since the last clear
  std::vector<int> have;
  struct Pending {
    bool on = false, success = false;
    int updates = 0, lc[3] = {0, 0, 0};
  };
  std::vector<Pending> pending;
  std::vector<int> lc;  // 3 per agent: accepted, rejected, all loop closures (Graph::statistics, ref src/Graph.cpp:475-521)
  int latest_weight_update_iteration = 0, resets_done = 0;
  // Ranked mode (the session is one rank of a job, enabled by Exchange::team_enable): every rank keeps the statuses of
  // all R agents.  What an agent knew when it optimised -- round, weight-update count, loop-closure counts -- every
  // rank knows; whether its update succeeded and its relative change only the hosting rank does, and those two travel
  // through the agent's status slot of the job's segment (the ranked k_rel_change), collected by the exchange inside
  // the collective call.  Nothing is read from rel_host.
  bool ranked = false;
  ShmStatus *slots = nullptr, *slots_dev = nullptr;  // [2][R], host and device view (owned by the exchange)
  std::vector<uint64_t> seq;     // optimisations of agent a since the team was enabled: the same on every rank
  const double *job_w = nullptr; // the job's m weights as of the last weight change (the exchange's copy); null on an
                                 // L2 job, whose counts come from the creation weights
};

// Robust state of a session created by dcora_rbcd_create_robust / dcora_ra_rbcd_create_robust (world_size 1) or by
// dcora_rbcd_create_robust_ranks / dcora_ra_rbcd_create_robust_ranks (one rank of a job, whose updates are collective:
// Exchange::update_weights): the agents' GNC loop inside one live session (Agent::initializeRobustOptimization /
// updateMeasurementWeights, ref src/Agent.cpp:1332-1346, 1397-1441).  The job's measurements are the re-weightable ones
// in the kind's order: the dataset's, or a range-aided one's pose-pose.  A weight change rebuilds the VALUES of every
// agent's matrix, of its coupling block and of the central Q on their creation patterns (a weight of 0 leaves explicit
// zeros), and the preconditioners through the path creation takes.  A rank's matrices hold only the measurements
// touching its hosted agents: the weight it keeps for any other is the last it was told and reaches no device matrix.
struct RobustState {
  explicit RobustState(const dcora_robust_params &p) : cost(p), params(p) {}
  RobustCost cost;
  dcora_robust_params params;
  int updates = 0;
  std::vector<double> w;         // the job's current weights
  std::vector<char> update;      // loop closures whose weight is not fixed: what updateMeasurementWeights rewrites
  std::vector<char> meas_zero;   // weight 0 at creation: the patterns do not hold these measurements
  RobustEdges edges;             // device copy of the measurements and of the weights
  bool ranked = false;           // created by one of the _create_robust_ranks entries
  std::vector<int> edge_ids;     // the measurements in `edges` (job order): all, or those touching a hosted agent
  std::vector<char> owned;       // per measurement: this rank hosts the agent of p1 (every one has one owner in the job)
  DevBuf<double> X_initial;      // the last set_X, laid out like the mirror (robustOptNumResets: setXToInitialGuess)
  std::vector<HostCsr> Qpat, Cpat;  // creation patterns (rp, ci) of every hosted agent's matrix and coupling block
  HostCsr central_pat;
  HostCsr live_pat;  // range-aided: the central Q's entries as the current weights give them (what certify reads)
};

enum class SessionKind { PoseGraph, RangeAided };

class SessionCore {
 public:
  int r = 0, R = 0;  // relaxation rank (rows of the mirror), agents
  dcora_rbcd_options opt{};
  hipStream_t st = nullptr;
  DevBuf<double> Xg;  // the mirror, r x num_cols() column-major: own columns current, the neighbours' public ones after
                      // the exchange's wait
  double gamma = 0, alpha = 0;
  int iteration = 0;
  int inner_rounds = 0;  // rounds since the owner last zeroed it (Agent::mRobustOptInnerIter, ref src/Agent.cpp:537-538)
  DeviceProblem *last_solver = nullptr;
  double setup_ms = 0;

  explicit SessionCore(SessionKind kind) : kind_(kind), tag_(kind == SessionKind::PoseGraph ? "rbcd" : "ra_rbcd") {}
  SessionKind kind() const { return kind_; }
  const char *tag() const { return tag_; }
  virtual ~SessionCore() {}
  virtual AgentCore &agent_core(int a) = 0;
  virtual long num_cols() const = 0;                  // columns of the mirror (the whole problem)
  virtual int phase_nonselected(int selected) = 0;    // Agent::iterate(false) of the hosted non-selected agents
  virtual int phase_selected(int selected) = 0;       // Agent::iterate(true) where the selected agent lives
  // per hosted agent a: out[2a] = |Proj(X_a Q_aa + G_a)|^2, out[2a + 1] = <X_a, X_a Q_aa + G_a> (device, 2 R doubles)
  virtual int phase_evaluate_dev(double *out_dev) = 0;
  virtual int set_X(const double *Xh) = 0;
  // where hosted agent a's block lies now (agent_block.h): a view for the call at hand, void after a rank change
  virtual AgentBlock agent_block(int a) = 0;
  // the hosted agents' columns of the mirror into host_area (laid out like the mirror): a contiguous block is copied
  // straight from the device, listed ones go through one download of the whole mirror; synchronises
  int x_stage_hosted(double *host_area);
  // nothing of the session is in flight: every agent's own stream is synchronised, then (then_session) the session's
  int drain(bool then_session);
  long chain_launches = 0;  // kernel launches of the chain's wrappers enqueued by the iterate() of the session or of its
                            // exchange (debug counter; only the pose-graph kind reports it)

  // greedy colouring of the agent graph in agent order: agents of one colour share no measurement, so their
  // simultaneous updates equal the same updates done one after the other
  int agent_colours(int *colours, int *ncolours);
  // The tick: the agents of `set` run Agent::iterate(true) at the same time, every one of them seeing the mirror as it
  // was when the tick began (what concurrently firing agents of the asynchronous mode see, ref src/Agent.cpp:650-678;
  // non-accelerated like that mode, :651-653).  Every agent's G, start point and XPrev are staged on the session's
  // stream before any block goes back into the mirror, and no solve reads the mirror: for agents that share no
  // measurement the tick equals one-after-the-other updates, for adjacent ones (allow_adjacent) it is well defined.
  int iterate_set(const int *set, int count, int allow_adjacent);

  // fastVerification (ref src/DCORA_utils.cpp:1713-1735) of S = Q - Lambda(X) on the session's current matrices -- the
  // central Q as the last weight change left it -- at the mirror as it stands (session_cert.h).  Single-process sessions
  // only; nothing of the session changes.
  int certify(double eta, CertifyResult *out, double *info8);
  // The Riemannian staircase's step in place (ref examples/MultiRobotExample.cpp:352-366, where a level is a new set of
  // agents; src/QuadraticProblem.cpp:138-234): the session goes from rank r to r + 1 along the certificate's direction
  // (theta, v: what certify returned, v on the host) and keeps everything that does not depend on r -- matrices,
  // preconditioners, regularisations, neighbours, public columns, colours, robust weights with mu and the update count,
  // the team with its parameters and loop-closure counts, the certificate's tables.
  //   a. every stream of the session is synchronised;
  //   b. the central problem gets its preconditioner (escapeSaddle's PreCondition) if it has none, or if a re-weight
  //      changed the central Q since it was built: of the matrix the device holds, with p.central_reg or the kind's
  //      default (lift_default_reg: what the two Python drivers pass);
  //   c. the central problem is re-ranked and runs the device escape from the mirror;
  //   d. no escape: its re-rank is undone, *escaped = 0, nothing of the session has changed;
  //   e. escaped: every hosted agent's problem is re-ranked and the session re-dimensioned (redimension): the kind's
  //      buffers (lift_buffers), the accepted point adopted as set_X adopts one (lift_adopt) -- mirror, agents' blocks,
  //      V = Y = XPrev = X, sequences and round counters restarted, X_initial of a robust session, team statuses
  //      cleared.  Handed neighbour caches
  //      are dropped; device pointers into the session's buffers handed out earlier (X_device_ptr) are void.
  // Refused, the session untouched: a rank of a job, a ranked robust / team session or a session an exchange was created
  // on (DCORA_ERR_UNSUPPORTED: those lift together, through their exchange -- Exchange::lift); r = 16, v null or not
  // finite, theta or a tolerance not finite (DCORA_ERR_BAD_ARG).  info8 (may be null): trials, accepted alpha, f before,
  // f after, 1 if the central preconditioner was built in this call, its ms, ms of the re-dimensioning, ms total.
  int lift(double theta, const double *v, const dcora_lift_params &p, int *escaped, double *info8);
  bool exchange_attached = false;  // an Exchange was created on this session

  // The last step of a solve where the iterate lies (session_round.h): the mirror rounded into the frame of an anchor
  // -- the lifted pose anchor_pose of the current iterate, read on the device (anchor null; 0 is the pose the
  // reference's drivers share), or r x (d + 1) doubles from the host (setGlobalAnchor) -- whose translation is the
  // origin.  trajectory: d x (d+1) n, SE ordering; unit_spheres (d x l, rotated only) and landmarks (d x b) may be null.
  // cost2 (may be null): 2 f of the rounded solution through central_problem()->eval_dev on the lifted rounded point
  // (sphere columns normalised), i.e. on the session's own matrix with its current weights.  info4 (may be null):
  // |rgrad| at that point, ms of the kernels, ms of the evaluation, ms total.  Runs on the session's stream; writes
  // nothing the session reads: a run after the call equals the run without it, bit for bit.  Refused, the session
  // untouched: a rank of a job (DCORA_ERR_UNSUPPORTED: those round through Exchange::round); trajectory null,
  // anchor_pose outside 0 .. n - 1, a non-finite anchor (DCORA_ERR_BAD_ARG).
  int round(int anchor_pose, const double *anchor, double *trajectory, double *unit_spheres, double *landmarks,
            double *cost2, double *info4);
  int round_check_args(int anchor_pose, const double *anchor, const double *trajectory) const;
  // ---- the session's half of the collective rounding (Exchange::round, where the flow stands).  A rank's mirror is
  // current only in its hosted agents' columns and the neighbours' public ones, so every state is rounded by the rank
  // that hosts it, from the agent's own block (agent_block), with the kernel of round.
  //   fetch_anchor: the r x (d + 1) words of global pose anchor_pose into out where this rank hosts it (else out is left
  //                 as it is: the caller's zeros); synchronises
  //   hosted:       the hosted agents' poses, unit spheres and landmarks rounded against the anchor (host, r x (d + 1))
  //                 and stored at their global places of the three host areas (traj: d x (d+1) n in the SE ordering,
  //                 spheres: d x l, landmarks: d x b; the latter two may be null); synchronises
  int round_fetch_anchor(int anchor_pose, double *out);
  int round_hosted(const double *anchor, double *traj_area, double *spheres_area, double *landmarks_area);

  // How CORA ends a certified solve, in place (session_project.h; ref examples/SingleRobotExample_RASLAM.cpp:220-234,
  // projectSolutionRASLAM src/DCORA_utils.cpp:1984-2031): the session goes from rank r to rank d at Proj(V_d^T X), V_d
  // the top-d eigenvectors of G = X X^T with the reflection rule folded in, and keeps everything lift keeps.
  //   a. every stream of the session is synchronised;
  //   b. G on the device in one pass over the mirror, its eigenproblem on the host (stable order among equal values);
  //   c. r == d: the reference passes X through -- sigma, gram and cost2 are produced, nothing of the session changes;
  //   d. the determinant count under V_d, the reflection (npos < n / 2), the projected point in a d x k buffer aside;
  //   e. the central problem and every hosted agent's problem re-ranked to d, the session re-dimensioned (redimension)
  //      at the point.  A failure on the way takes the re-ranks back, as in lift.
  // Every output may be null.  sigma: r singular values of X, descending; basis: r x d column-major, V_d as applied
  // (only where projected); gram: r x r, G as the device formed it; cost2: 2 f of the adopted point through
  // central_problem()->eval_dev (the session's current matrices and weights); info8: projected, reflected, rotation
  // blocks with positive determinant before the reflection, |rgrad| at the adopted point, ms of the projection
  // kernels, ms of the re-dimensioning, ms total, columns per workgroup of the Gram kernel.  Refused, the session
  // untouched, as lift (DCORA_ERR_UNSUPPORTED): the ranks of a job project together, through Exchange::project.
  int project(double *sigma, double *basis, double *gram, double *cost2, double *info8);
  // ---- the session's half of the collective projection (Exchange::project, where the flow stands).  A rank's mirror
  // is current only in its hosted agents' columns and the neighbours' public ones, so every step works on the hosted
  // agents' own blocks (agent_block).  The session itself is not touched before project_trial_commit.
  //   grams:  every stream synchronised; G_a = X_a X_a^T of every hosted agent in one launch pair (launch_gram_blocks);
  //           *hosted: the agents in agent order, *grams: their r x r matrices one after another (host); synchronises
  //   dets:   *npos = the hosted poses with det(basis^T Y_i) > 0 (basis: r x d, host); synchronises
  //   point:  Proj(basis^T X_a) of every hosted block into the trial mirror of d rows, zero elsewhere; *mirror: what the
  //           exchange posts from and waits into; synchronises
  //   commit: every hosted agent's problem, and the central one of a one-rank job, re-ranked to d and the session
  //           re-dimensioned (redimension) at the trial mirror; *redim_ms: what that took
  //   abort:  the trial dropped; a commit that failed before redimension's point of no return has its re-ranks taken
  //           back (the error that led here stays the one reported)
  //   ms:     event time of the trial's kernels so far
  int project_trial_grams(std::vector<int> *hosted, std::vector<double> *grams);
  int project_trial_dets(const double *basis, double *npos);
  int project_trial_point(const double *basis, double **mirror);
  int project_trial_commit(double *redim_ms);
  void project_trial_abort();
  double project_trial_ms() const { return project_trial_ ? project_trial_->kernel_ms : 0.0; }

  // ---- room for the ranks to come: an exchange created on this session sizes its halo slots, its staged slots and its
  // gather_X area by max(r, reserve_r), so that the job can lift up to that rank (Exchange::lift).  0: a job that will
  // never lift, laid out exactly as before.  Legal (d <= r <= r_reserve <= 16, else DCORA_ERR_BAD_ARG) until an
  // exchange exists (then DCORA_ERR_UNSUPPORTED: its segment is mapped and its IPC handles are open).
  int reserve_r = 0;
  int reserve_rank(int r_reserve);
  virtual int dim() const = 0;  // d

  // ---- the session's half of the collective lift (Exchange::lift, where the flow stands): the escape of
  // SessionCore::lift carried by the hosted agents' own problems, each at rank r + 1 on its block of
  // [X; 0] + alpha [0; v^T], against a trial mirror of r + 1 rows that holds the hosted blocks and, after the exchange's
  // post and wait, the neighbours' public columns.  The session itself -- mirror, sequences, counters -- is not
  // touched before lift_trial_commit.
  //   begin:   every stream synchronised, every hosted agent's problem re-ranked, v on the device, the two images of
  //            every hosted block (k_lift_images, agent form) in its problem's X0 / eta
  //   point:   X1 = Retract(X0, alpha eta) of every hosted block and its columns into the trial mirror; *mirror: what
  //            the exchange posts from and waits into.  alpha = 0 is the current iterate through the same kernel: f
  //            before and f of a trial then come from one arithmetic path, and a direction of zeros gives trial
  //            points that equal it bit for bit -- no trial "lowers" f by the rounding of a projection
  //   scalars: G_a from the trial mirror, then per hosted agent <X_a Q_aa, X_a> + <X_a, G_a>, |rgrad_a|^2 and
  //            |Proj(rgrad_a M_a^-1)|^2 with the agent's own preconditioner; ONE host wait; out3: their sums over the
  //            hosted agents in agent order (2 f's share, |rgrad|^2's, |P grad|^2's)
  //   commit:  the central problem of a one-rank job re-ranked, the session re-dimensioned (redimension) at the trial
  //            mirror; *redim_ms: what that took plus the agents' re-ranks of begin -- the re-dimensioning as
  //            SessionCore::lift's info8[6] counts it
  //   abort:   the trial's RankChange rolled back: every re-ranked problem at r again (the error that led here stays the
  //            one reported)
  int lift_trial_begin(const double *v_host);
  int lift_trial_point(double alpha, double **mirror);
  int lift_trial_scalars(double out3[3]);
  int lift_trial_commit(double *redim_ms);
  void lift_trial_abort();
  virtual DeviceProblem *central_problem() = 0;                        // null on a rank of a multi-rank job
  virtual int cert_block() const = 0;  // unknowns the factorisation orders together (d + 1 for poses)
  // A rank of a multi-rank job: the pattern (rp, ci) of the job's whole Q as its creation-time weights give it, kept
  // from the assembly at creation -- what the job-wide certificate (Exchange::certify_live) is laid out on.  Empty in a
  // single-process session, whose central problem holds that pattern.
  HostCsr job_pat;
  virtual ManiDesc global_manifold() const = 0;  // of the whole problem, at the current r

  // ---- robust sessions (session_robust.hip), stated once for both kinds; null on a plain session.  The calls below
  // are a robust session's.
  std::unique_ptr<RobustState> robust;
  bool weights_ranked() const { return robust && robust->ranked; }  // the exchange changes its weights
  size_t weights_count() const { return robust ? robust->w.size() : 0; }  // measurements of the job
  // updateMeasurementWeights on the current iterate; counts (may be null): accepted, rejected, undecided closures
  int update_weights(bool reset_to_initial, int counts[3]);
  // its two halves, which the exchange's collective update calls one by one: the weights of the session's edges on the
  // device from the mirror (ranked: the owned ones also into shared_w, counts over the owned ones), then the matrices
  // rebuilt and the rest of the update
  int compute_weights(double *shared_w, std::vector<double> *w, double counts[3]);
  int apply_weights(const std::vector<double> &w, bool reset_to_initial);
  // all weights_count() of them; refused (session untouched) when one is negative or not finite
  int set_weights(const double *w);
  int get_weights(double *w) const;  // ranked: NaN for the measurements touching no hosted agent
  // whether this rank owns measurement e (hosts the agent of its first pose); *w: the weight the session holds for it
  bool weight_owned(size_t e, double *w) const {
    *w = robust->w[e];
    return robust->owned[e] != 0;
  }

  // ---- the team protocol of a single-process session (dcora_rbcd_team_enable / dcora_ra_rbcd_team_enable): the
  // bookkeeping of Agent::iterate's status block, shouldTerminate, shouldUpdateMeasurementWeights and
  // updateMeasurementWeights (ref src/Agent.cpp:558-586, 1123-1156, 1280-1330, 1417-1424), the same on either graph type
  std::unique_ptr<TeamState> team;
  int team_enable(const dcora_team_params &p);
  int team_agent_status(int agent, dcora_agent_status *status, int *known);
  int team_decide(int *should_terminate, int *should_update_weights);
  bool team_robust() const { return robust && robust->params.cost_type != DCORA_ROBUST_L2; }
  int team_weight_updates() const { return robust ? robust->updates : 0; }  // mWeightUpdateCount
  int team_inner_iter() const { return team_robust() ? inner_rounds : 0; }
  // ---- the half of a rank of a job, of either kind, through its exchange only (Exchange::team_enable): the status area
  // and the job's weights the exchange keeps
  int team_enable_ranked(const dcora_team_params &p, ShmStatus *slots, ShmStatus *slots_dev, const double *job_w);
  // ranked: the bookkeeping of team_note_optimized for those agents of ids that live on another rank, and the two facts
  // the hosting rank published for one agent settled into its status
  void team_note_elsewhere(const int *ids, int count);
  void team_settle_published(int agent, bool success, double relative_change);
  // the agents' own loop: stop and re-weight by the team rules instead of a central gradient norm and fixed counts
  int run_team(int *iters_done, double *cost2_trace, double *gradnorm_trace, int *selected_trace, int *updated_trace,
               int *weight_updates, int *stop_reason);

 protected:
  const SessionKind kind_;
  const char *tag_;  // "rbcd" / "ra_rbcd": the prefix of the messages
  hipEvent_t fork_ev_ = nullptr;
  bool own_stream_ = true;
  SessionCertState cert_;  // built by the first certify
  SessionRoundState round_;  // built by the first round
  int round_buffers(const ManiDesc &m, bool with_lifted);
  SessionProjectState project_;  // built by the first project
  int project_buffers(const ManiDesc &m);

  // updateGamma / updateAlpha (ref src/Agent.cpp:1189-1200) and the round counter; the sequences are data-independent
  // and identical for every agent, so they live on the host
  void advance_sequences();
  bool restart_now() const { return opt.acceleration && ((iteration + 1) % opt.restart_interval == 0); }
  int check_selected(int selected) const;

  // the session's stream (borrowed: the caller's, never released here), an agent's stream and event, the fork event
  int acquire_stream(void *borrowed);
  int acquire_tick_resources(AgentCore &a);
  int create_fork_event();
  void release_tick_resources(AgentCore &a);  // before the agent's problem goes
  void release_stream();  // (with the fork event) after everything that runs on it has gone

  // what a session kind supplies to a rank change (lift, the collective lift, project):
  // the regularisation of the central preconditioner where the caller names none
  virtual int lift_default_reg(const HostCsr &Qc, double *reg) = 0;
  // the buffers the kind owns at rank r_new, allocated aside and swapped in, with r, opt.r and what else the kind
  // derives from r; their contents are undefined until lift_adopt.  On failure nothing has changed.
  virtual int lift_buffers(int r_new) = 0;
  // set_X of a point that lies on the device (r x num_cols(), the mirror's ordering): everything set_X leaves
  virtual int lift_adopt(const double *X_dev) = 0;
  // The re-dimensioning of a rank change whose problems `change` holds, in this order: the certificate's XQ at r_new
  // aside (where a certificate was built), lift_buffers, the swap of XQ, change.commit() -- the point of no return --,
  // lift_adopt of the device point X_dev, the session's stream synchronised.  A failure before the commit leaves the
  // session as it was and `change` to its roll-back; after a failed lift_adopt the session stays at r_new.  what:
  // "lift" / "project", for the message.
  int redimension(const char *what, int r_new, const double *X_dev, RankChange<DeviceProblem> &change);
  // a block of `rows` rows in blk's ordering into blk's columns of a mirror of `rows` rows (enqueued on st)
  int scatter_block(const AgentBlock &blk, int rows, const double *block, double *mirror);
  struct LiftTrial {
    explicit LiftTrial(int r_old) : change(r_old) {}
    double rerank_ms = 0;            // what the hosted agents' re-ranks took in lift_trial_begin
    DevBuf<double> mirror, v, scal;  // (r + 1) x num_cols(), num_cols(), 4 per hosted agent
    std::vector<int> hosted;         // in agent order
    RankChange<DeviceProblem> change;  // (the last member: the re-ranks go back before the buffers go)
  };
  std::unique_ptr<LiftTrial> lift_trial_;  // between lift_trial_begin and commit / abort
  struct ProjectTrial {
    explicit ProjectTrial(int r_old) : change(r_old) {}
    double kernel_ms = 0;
    DevBuf<double> mirror;    // d x num_cols()
    std::vector<int> hosted;  // in agent order
    RankChange<DeviceProblem> change;  // (the last member, as in LiftTrial)
  };
  std::unique_ptr<ProjectTrial> project_trial_;  // between project_trial_grams and commit / abort

  // robust sessions, for the kinds' init_robust.  robust_check_args: what both kinds refuse.  robust_begin: the state,
  // with weight 1 on every loop closure (lc: one flag per measurement) that is not fixed (fixed: one flag per
  // measurement, or null) and the creation weight on the rest; the kind then creates itself from robust->w.
  // robust_finish: the edges on the device, X_initial.
  int robust_check_args(const std::vector<PoseMeas> &meas, int num_poses, const dcora_rbcd_options &o,
                        const dcora_robust_params &p, bool ranked) const;
  void robust_begin(const std::vector<PoseMeas> &meas, const std::vector<char> &lc, const dcora_robust_params &p,
                    const int *fixed, bool ranked);
  int robust_finish();
  // the shared tail of both ways to change weights (w: all of the job's, swapped in when they are adopted)
  int adopt_weights(std::vector<double> &w, bool from_device, bool reset_to_initial);
  // what a session kind supplies to them:
  // edge_ids and owned filled (ranked: the measurements touching a hosted agent; else all) and those measurements
  // uploaded through the kind's entry of RobustEdges
  virtual int robust_upload_edges() = 0;
  // Graph::clearDataMatrices + constructDataMatrices (ref src/Agent.cpp:1416) for the job's weights w on the creation
  // patterns; every stream of the session has been drained
  virtual int robust_rebuild(const std::vector<double> &w) = 0;
  // Agent::initializeAcceleration of every agent (ref src/Agent.cpp:1178-1187): XPrev = V = Y = X, gamma = alpha = 0;
  // the round counter goes on
  virtual int robust_restart_acceleration() = 0;

  // the three things a session kind supplies to the tick
  virtual void tick_begins() {}  // (the set is valid: per-tick resets)
  // G = X_mirror C_a^T, the start point and XPrev of one agent, enqueued on the session's stream
  virtual int stage(AgentCore &a) = 0;
  // the result of a's solve into its X and the mirror, enqueued on run_on
  virtual int write_back(AgentCore &a, hipStream_t run_on) = 0;
  // whether the set's solves run one after the other on the session's stream instead of side by side on the agents' own
  virtual bool serial_set(const std::vector<AgentCore *> &work) = 0;
  // the tick's updates are all enqueued (the session's stream waits for every one of them)
  virtual int tick_done(const std::vector<AgentCore *> &work) { return DCORA_OK; }

  // the team protocol's steps: agents that just ran iterate(true) (one launch of the relative-change kernel behind their
  // updates), pending statuses settled (visible: the host has already seen the stream pass their launch), the
  // loop-closure counts after a weight change, the statuses cleared, the weight update of this round recorded, the
  // bookkeeping restarted with the round counter
  int team_note_optimized(const int *ids, int count);
  void team_mark_optimized(int agent, bool success);
  int team_settle(bool visible);
  void team_refresh_counts();
  void team_clear_statuses();
  void team_weights_updated();
  void team_restart_rounds();
  RelChangePublish team_publish_slots(const std::vector<int> &ids);  // ranked: what team_launch_rel_change publishes
  std::vector<TeamLoopClosure> team_lcs_;  // the session's loop closures, filled at creation
  // what a session kind supplies to the team protocol:
  // its relative-change kernel for these hosted agents, just marked, enqueued on the session's stream
  virtual int team_launch_rel_change(const std::vector<int> &ids) = 0;
  double team_lc_weight(const TeamLoopClosure &q) const;  // the current weight of one of team_lcs_
  virtual bool team_last_success(int agent) const { return true; }    // `success` of the agent's last local update
  virtual int team_iteration_number(int agent) const { return iteration; }
  virtual int team_iterate(int selected, double *cost2, double *gradnorm, int *next_selected) = 0;

 private:
  int solve_block(AgentCore &a, std::string *err, bool serial);
};


// The coloured run loop of dcora_rbcd_run_coloured / dcora_ra_rbcd_run_coloured / dcora_exchange_run_coloured: a sweep is
// one tick per colour (tick(set, count): the agents of that colour, in agent order), colours 0, 1, ... in order, followed
// by one evaluation (evaluate(&cost2, &gradnorm)); it stops after the first sweep whose |rgrad| < rgrad_tol or after
// max_sweeps.  Exactly the calls a caller of iterate_set / rbcd_tick and evaluate makes (the agents that fire together in
// the asynchronous mode, ref src/Agent.cpp:650-678, made a schedule).  Trace entry s: the evaluation after sweep s.
template <class Tick, class Evaluate>
int run_coloured_sweeps(const std::vector<int> &colours, int ncolours, Tick &&tick, Evaluate &&evaluate, int max_sweeps,
                        double rgrad_tol, int *sweeps_done, double *cost2_trace, double *gradnorm_trace) {
  std::vector<std::vector<int>> sets((size_t)ncolours);
  for (size_t a = 0; a < colours.size(); ++a) sets[(size_t)colours[a]].push_back((int)a);
  int s = 0;
  while (s < max_sweeps) {
    for (const std::vector<int> &set : sets) {
      const int rc = tick(set.data(), (int)set.size());
      if (rc) return rc;
    }
    double c2 = 0, gn = 0;
    const int rc = evaluate(&c2, &gn);
    if (rc) return rc;
    if (cost2_trace) cost2_trace[s] = c2;
    if (gradnorm_trace) gradnorm_trace[s] = gn;
    ++s;
    if (gn < rgrad_tol) break;
  }
  if (sweeps_done) *sweeps_done = s;
  return 0;
}

}  // namespace dcora
