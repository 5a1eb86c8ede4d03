/*
 * dcora_hip.h -- C ABI of the MI355X (gfx950) implementation of DCORA's hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.
 * Every entry point names the reference interface it replaces (paths relative
 * to the reference tree).  Conventions shared by all calls:
 *
 *   - dense matrices are column-major double with leading dimension = rows
 *     (Eigen::MatrixXd layout, ref include/DCORA/DCORA_types.h:34);
 *   - sparse matrices are row-major CSR, int32 indices, both triangles stored
 *     (ref include/DCORA/DCORA_types.h:36);
 *   - column ordering of the lifted variable X (r x k): SE ordering
 *     [Y1 p1 ... Yn pn] when l == b == 0, otherwise RA ordering
 *     [Y1..Yn | s1..sl | p1..pn | L1..Lb]
 *     (ref src/manifold/LiftedVariable.cpp:74-106, 257-295);
 *   - host pointers are borrowed for the duration of the call only; handles own
 *     their device memory; *_dev variants take device pointers and enqueue on
 *     the handle's HIP stream without synchronising;
 *   - every function returns a dcora_status (0 = ok); nothing throws across
 *     the ABI.  The library fails loudly (DCORA_ERR_NO_DEVICE / DCORA_ERR_HIP)
 *     when no gfx950 device is usable: there is no CPU fallback;
 *   - a NULL handle or a NULL required pointer (one not documented as optional)
 *     returns DCORA_ERR_BAD_ARG; the *_destroy functions accept NULL.
 */
#ifndef DCORA_HIP_H_
#define DCORA_HIP_H_

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  DCORA_OK = 0,
  DCORA_ERR_BAD_ARG = 1,
  DCORA_ERR_NO_DEVICE = 2,
  DCORA_ERR_HIP = 3,
  DCORA_ERR_NOT_PD = 4,          /* Cholesky hit a non-positive pivot */
  DCORA_ERR_NO_CONVERGENCE = 5,  /* Lanczos did not converge */
  DCORA_ERR_NO_PRECONDITIONER = 6,
  DCORA_ERR_IO = 7,
  DCORA_ERR_UNSUPPORTED = 8,
  DCORA_ERR_EXCHANGE_LINK = 9    /* dcora_exchange_create: no transport between the ranks passed its start-up check */
} dcora_status;

const char *dcora_status_string(int status);
const char *dcora_last_error(void);
/* number of usable HIP devices (0 when there is none; never initialises more than the runtime) */
int dcora_device_count(void);

/* Manifold shape (ref src/manifold/LiftedManifold.cpp:18-89) and column ordering (ref src/manifold/LiftedVariable.cpp:
 * 74-106 SE: pose i = columns [i (d+1), i (d+1) + d]; :257-295 RA: rotations | unit spheres | translations | landmarks).
 * The reference chooses the manifold by GRAPH TYPE (ref src/Graph.cpp:68-75, src/QuadraticProblem.cpp:19-34): a
 * RangeAidedSLAMGraph that happens to hold neither ranges nor landmarks still uses the RA ordering.  `layout` carries that
 * choice; brace-initialising the first five members leaves it at DCORA_LAYOUT_AUTO. */
enum {
  DCORA_LAYOUT_AUTO = 0, /* SE ordering when l = b = 0, RA ordering otherwise */
  DCORA_LAYOUT_SE = 1,   /* pose graph (l and b must be 0) */
  DCORA_LAYOUT_RA = 2    /* range-aided ordering whatever l and b are */
};
typedef struct {
  int r; /* relaxation rank */
  int d; /* 2 or 3 */
  int n; /* poses (Stiefel blocks) */
  int l; /* unit spheres (oblique columns) */
  int b; /* landmarks */
  int layout; /* DCORA_LAYOUT_* */
} dcora_dims;

/* ref include/DCORA/DCORA_types.h:152-168 ROptParameters (same defaults via dcora_ropt_params_default) */
typedef struct {
  int method; /* 0 = RTR, 1 = RGD */
  int verbose;
  double gradnorm_tol;
  double RGD_stepsize;
  int RGD_use_preconditioner;
  int RTR_iterations;
  int RTR_tCG_iterations;
  double RTR_initial_radius;
} dcora_ropt_params;
void dcora_ropt_params_default(dcora_ropt_params *p);

/* ref include/DCORA/DCORA_types.h:203-233 ROPTResult (+ solver counters) */
typedef struct {
  int success;
  double fInit, gradNormInit, fOpt, gradNormOpt, elapsedMs;
  int tCGStatus; /* 0 NEGCURVTURE, 1 EXCREGION, 2 LCON, 3 SCON, 4 MAXITER */
  int outer_iterations, inner_iterations, accepted_steps;
} dcora_ropt_result;

/* ------------------------------------------------------------------------- *
 * QuadraticProblem  (replaces src/QuadraticProblem.cpp)
 * ------------------------------------------------------------------------- */
typedef struct dcora_problem_s *dcora_problem_t;

/* QuadraticProblem(shared_ptr<Graph>) (ref src/QuadraticProblem.cpp:19-34): uploads Q (k x k CSR) and G
 * (r x k, may be NULL = zero) and, when precond_reg >= 0, builds the preconditioner (Q + reg I)^-1
 * (ref src/Graph.cpp:1901-1917; reg = 0.1 for PGO).  device = HIP device ordinal. */
int dcora_problem_create(const dcora_dims *dims, const int *rowptr, const int *colidx, const double *vals,
                         const double *G, double precond_reg, int device, dcora_problem_t *out);
int dcora_problem_destroy(dcora_problem_t p);
/* Graph::linearMatrix() changed (ref src/Graph.cpp:535-540, 685-822) */
int dcora_problem_set_linear_term(dcora_problem_t p, const double *G);
/* f(Y) (ref src/QuadraticProblem.cpp:38-44) */
int dcora_problem_cost(dcora_problem_t p, const double *X, double *f);
/* EucGrad = X Q + G (ref :53-59) */
int dcora_problem_eucgrad(dcora_problem_t p, const double *X, double *out);
/* RieGrad / RieGradNorm (ref :86-123); out may be NULL */
int dcora_problem_riegrad(dcora_problem_t p, const double *X, double *out, double *norm);
/* Riemannian Hessian-vector product: EucHessianEta (ref :61-68) followed by ROPTLIB's EucHvToHv */
int dcora_problem_hessvec(dcora_problem_t p, const double *X, const double *V, double *out);
/* Test hook: the same product as the generic-layout solver loop forms it (delta Q, EucHvToHv and the partial sums of
 * <V, H V> in ONE launch, k_spmm_dir_fix); dots[0] = <V, H V> from that kernel's partials, dots[1] = the same from the
 * two-launch form.  DCORA_ERR_UNSUPPORTED when the one-launch form does not apply (a long row on a manifold column). */
int dcora_debug_hessvec_solver_form(dcora_problem_t p, const double *X, const double *V, double *out, double *dots);
/* How the tCG iteration of the local solver runs on this problem: info[0] = 0 three launches per
 * iteration (or the sparse preconditioner), 1 = two launches (Hessian product; step + dense preconditioner + projection),
 * 2 = the whole tCG run of an RTR iteration in ONE launch (dense preconditioner, n / 2 workgroups co-resident). */
int dcora_problem_solver_info(dcora_problem_t p, double *info);
/* How the one-launch tCG run gathers its neighbours' columns on this problem (DCORA_GATHER):
 * info[0] = 1 a column-slot map of the run's 2-pose workgroups was built, info[1] its workgroups, info[2] those naming
 * more pose blocks than the map holds per workgroup (overflow), info[3] the most pose blocks a workgroup names, info[4] = 1
 * the run form applies here and fetches every neighbour column once per workgroup (a map, no overflow), 0 every row
 * gathers its own entries, or the problem has no run form.
 * info: 5 doubles. */
int dcora_problem_gather_info(dcora_problem_t p, double *info);
/* test hook: the problem at another relaxation rank, in place (what a session's lift and projection do to their agents'
 * problems): Q, the preconditioner and the stream stay, the workspace and the solver forms are those of r_new, G is
 * zero afterwards. */
int dcora_debug_problem_rerank(dcora_problem_t p, int r_new);
/* test hook (host only, no device needed): the column-slot map of a workgroup tiling.  rowptr / colidx: the pattern of
 * an n dh x n dh SE-layout matrix (dh = d + 1); pb poses per workgroup, ceil(n / pb) workgroups; cap_cols: the most
 * columns a workgroup's list may hold.  lp (workgroups + 1) / list (room for list_cap): per workgroup the ascending
 * distinct poses its rows name, its own among them; empty where it overflows.  count, overflow (workgroups): the poses
 * it names, and whether they exceed cap_cols / dh.  slot (one per entry): position of the entry's pose in the list
 * times dh plus its column within the pose; 65535 in an overflow workgroup. */
int dcora_debug_column_slots(const int *rowptr, const int *colidx, int n, int dh, int pb, int cap_cols, int list_cap,
                             int *lp, int *list, int *count, int *overflow, int *slot);
/* test hook: the next `runs` one-launch tCG runs of this process lose a workgroup before their first grid-wide step, as
 * if the grid were not co-resident: the run must give up within milliseconds and the solve continue on the launches */
int dcora_debug_tcg_run_fault(int runs);
/* the same after `skip` launches of the run kernel that pass untouched (to hit the LAST iteration of a solve) */
int dcora_debug_tcg_run_fault_at(int skip, int runs);
/* test hook: one workgroup of 256 threads sums nv values per lane (nv = 33, 41, 49; in[i * 256 + 64 * wave + lane], host)
 * over its 16-lane rows the way the one-launch tCG run does (a reduce-scatter over lane-swap instructions) and with the
 * four-step DPP butterfly.  out (host, 2 * nv * 17 doubles): for each of the two, in that order, the nv x 16 row sums
 * (out[i * 16 + 4 * wave + row]) followed by the nv totals of the serial add over the 16. */
int dcora_debug_wg_sums(int nv, const double *in, double *out);
/* test hook: Retr_X(alpha V) by the 8-lanes-per-pose kernel (k_g_retract) on host arrays in the SE ordering, r x (d+1) n
 * each, r <= 8 (DCORA_ERR_BAD_ARG otherwise).  grad and HV are given together or both NULL.  Given: partials_out (host,
 * room for 2 * 1024 doubles) receives the kernel's pairs {<V, grad>, <V, HV>} of *npartials_out workgroups, in slot order.
 * NULL: the kernel gets no partial buffer, partials_out is not written and *npartials_out = 0. */
int dcora_debug_group_retract(int r, int d, int n, const double *X, const double *V, double alpha, const double *grad,
                              const double *HV, double *out, double *partials_out, int *npartials_out);
/* test hook: one launch of the RBCD++ Nesterov bookkeeping on host arrays (SE ordering, r x (d+1) n each; X, V, Y, XPrev,
 * Yloc in and out).  form 1: k_g_nesterov (r <= 8) with all bits of restart_bits; cur = 0 / 1 builds a control block on
 * the device whose `cur` picks Xloc0 / Xloc1, cur = -1 passes none (Xloc0 is read); inner_Yloc (NULL, or in / out,
 * r x (d+1) (skip_hi - skip_lo)) as in the session's mode-0 launch.  form 0: k_nesterov (r <= 16) with restart_bits & 1
 * and Xloc0, as the session calls it; inner_Yloc must be NULL. */
int dcora_debug_nesterov(int form, int r, int d, int n, int mode, int restart_bits, int skip_lo, int skip_hi,
                         double alpha, double gamma, double *X, double *V, double *Y, double *XPrev, double *Yloc,
                         const double *Xloc0, const double *Xloc1, int cur, double *inner_Yloc);
/* test hook (host only, no device needed): the LDS image of the one-launch tCG run at rank r (4, 5, 6) and k <= 2048
 * columns.  off (ceil(k / 128) * 64 * r ints): the byte offset of every pair of doubles of the column-major residual;
 * lanes (64 ints): the logical lane (columns 2 L, 2 L + 1 of a 128-column step) of each lane of a wave in the product;
 * bytes: the dynamic LDS the launch asks for. */
int dcora_debug_run_image(int r, int k, int *off, int *lanes, int *bytes);
/* PreCondition (ref :70-84, 261-297) */
int dcora_problem_precondition(dcora_problem_t p, const double *X, const double *V, double *out);
/* Retract (ref :125-136, 236-259) */
int dcora_problem_retract(dcora_problem_t p, const double *X, const double *V, double *out);
/* projectToTangentSpace (ref :299-307; src/manifold/LiftedManifold.cpp:37-41, 104-108) */
int dcora_problem_tangent_project(dcora_problem_t p, const double *X, const double *V, double *out);
/* escapeSaddle (ref :138-234): p is the problem at rank r, Xopt is (r-1) x k.  is_second_order selects the first
 * trial step: 0 => 1 (the header's default), 1 => max(16e-6, 100 gradient_tolerance / |theta|) (ref :165-169) */
int dcora_problem_escape_saddle(dcora_problem_t p, const double *Xopt, double theta, const double *v,
                                double gradient_tolerance, double preconditioned_gradient_tolerance,
                                int is_second_order, double *Xout, int *success);
/* LiftedSEManifold::project / LiftedRAManifold::project, projectToSEMatrix / projectToRAMatrix
 * (ref src/manifold/LiftedManifold.cpp:28-35, 91-102; src/DCORA_utils.cpp:2201-2220) */
int dcora_manifold_project(const dcora_dims *dims, const double *M, double *out, int device);

/* ------------------------------------------------------------------------- *
 * QuadraticOptimizer  (replaces src/QuadraticOptimizer.cpp)
 * ------------------------------------------------------------------------- */
/* optimize(Y) (ref src/QuadraticOptimizer.cpp:28-50): RTR (ref :52-108, 234-280) or one RGD step (ref :110-180) */
int dcora_optimizer_optimize(dcora_problem_t p, const dcora_ropt_params *params, const double *X0, double *Xout,
                             dcora_ropt_result *result);

/* ------------------------------------------------------------------------- *
 * Certification  (replaces src/DCORA_utils.cpp:1713-1982)
 * ------------------------------------------------------------------------- */
typedef struct dcora_csr_s *dcora_csr_t; /* host-side CSR returned by the library */
int dcora_csr_info(dcora_csr_t m, int *n, int *nnz);
int dcora_csr_copy(dcora_csr_t m, int *rowptr, int *colidx, double *vals);
int dcora_csr_destroy(dcora_csr_t m);

/* constructDualCertificateMatrixPGO / ...RASLAM (ref :1898-1982): S = Q - Lambda(X) */
int dcora_cert_dual_matrix(const dcora_dims *dims, const double *X, const int *rowptr, const int *colidx,
                           const double *vals, int device, dcora_csr_t *S);
/* isSparseSymmetricMatrixPSD (ref :1737-1747) */
int dcora_cert_is_psd(int k, const int *rowptr, const int *colidx, const double *vals, int block, int *is_psd);
/* the same test with the numeric factorisation on the device (multifrontal LL^T over the nested-dissection pieces,
 * dcora_amd/csrc/device_chol.h; the symbolic analysis is cached on the sparsity pattern).  This is what
 * dcora_cert_fast_verification runs.  info8 (optional): symbolic ms (0 on a cache hit), numeric ms, bytes of the
 * front arena, factorisation flops, tree levels, kernel launches, log det of the matrix (when PD), ms of the pattern
 * hash + cache look-up. */
int dcora_cert_is_psd_device(int k, const int *rowptr, const int *colidx, const double *vals, int block, int device,
                             int *is_psd, double *info8);
/* validation of the symbolic analysis without a GPU: the schedule of dcora_cert_is_psd_device executed by plain host
 * loops; *resid = max |P A P^T - L L^T| (dense check, k <= 4096).  Test utility, not a product path. */
int dcora_chol_host_selftest(int k, const int *rowptr, const int *colidx, const double *vals, int block, int *is_pd,
                             double *resid, double *info4);
int dcora_chol_cache_clear(void);
/* computeMinimumEigenPair(S, max_iterations, min_eig_num_tol, num_Lanczos_vectors) (ref :1809-1896) */
int dcora_cert_min_eig(int k, const int *rowptr, const int *colidx, const double *vals, int max_iterations,
                       double min_eig_num_tol, int num_lanczos_vectors, unsigned long long seed, int device,
                       double *lambda_min, double *v, long *num_matvecs);
/* fastVerification(S, eta, &theta, &x) (ref :1713-1735) */
int dcora_cert_fast_verification(int k, const int *rowptr, const int *colidx, const double *vals, double eta,
                                 int block, int device, int *is_psd, double *theta, double *x, double *lambda_min);

/* Suboptimality bound that goes with the certificate -- an ADDITION of this library: the reference reports the
 * boolean and theta only (ref examples/MultiRobotExample.cpp:321-352).  SE-Sync form: at a first-order critical point
 * X with certificate matrix S = Q - Lambda(X), every feasible Z = X'^T X' satisfies f(X) - f(X') = -1/2 <S, Z>
 * <= -1/2 lambda tr(Z) for any lower bound lambda <= min(lambda_min(S), 0).  tr(Z) is evaluated at X itself with the
 * translation / landmark columns centred (the cost does not see a common shift of them): n_eff = |rotation and
 * sphere columns|_F^2 + sum_i |p_i - mean p|^2, so gap = -1/2 lambda n_eff is exact for the rotation part and an
 * estimate for comparison points whose translations spread more than X's.  Pass lambda = -eta after a positive
 * dcora_cert_fast_verification(S, eta) (then S + eta I >= 0), or lambda_min - eta from its lambda_min output otherwise.
 * gap is in units of f (half of the "cost" the reference driver prints); n_eff may be NULL. */
int dcora_cert_suboptimality_gap(const dcora_dims *dims, const double *X, double lambda_lower_bound, double *gap,
                                 double *n_eff);
/* The eta-test only says lambda_min(S) >= -eta, and eta n_eff can exceed the cost itself when the trajectory is large
 * (n_eff grows with the spread of the translations).  After an accepted certificate this returns a CERTIFIED lower
 * bound of lambda_min(S): Lanczos with full re-orthogonalisation on (S + eta I)^-1 (the matrix the PSD test
 * factorised; sparse Cholesky on the host) until the Ritz value changes by less than 0.1 % (at most max_iterations
 * solves) gives the candidate 1 / (theta + Ritz residual) - eta, which is lowered by 0.1 % and then VERIFIED like the
 * certificate itself: S - lambda I must have a Cholesky factorisation.  The verified shift is returned; when the
 * verification fails, -eta (what the accepted certificate guarantees by itself).  DCORA_ERR_NOT_PD when S + eta I is
 * not positive definite.  An addition of this library.  lambda_lower_bound = min(lambda_min, 0) in
 * dcora_cert_suboptimality_gap gives a certified gap. */
int dcora_cert_lambda_min_certified(int k, const int *rowptr, const int *colidx, const double *vals, double eta,
                                    int block, int max_iterations, double *lambda_min, int *iterations);

/* ------------------------------------------------------------------------- *
 * Data feed  (replaces the parts of src/Graph.cpp / src/DCORA_utils.cpp that
 * produce Q, G and the measurement list)
 * ------------------------------------------------------------------------- */
/* measurement arrays: ids m x 4 int32 (r1, p1, r2, p2); vals m x (d*d + d + 3) double
 * (R column-major, t, kappa, tau, weight)  (ref include/DCORA/Measurements.h RelativePosePoseMeasurement) */
typedef struct dcora_dataset_s *dcora_dataset_t;
/* read_g2o_file (ref src/DCORA_utils.cpp:179-375); .gz not handled here */
int dcora_dataset_load_g2o(const char *path, dcora_dataset_t *out);
int dcora_dataset_create(int d, int n, int m, const int *ids, const double *vals, dcora_dataset_t *out);
int dcora_dataset_info(dcora_dataset_t ds, int *d, int *n, int *m);
int dcora_dataset_copy(dcora_dataset_t ds, int *ids, double *vals);
int dcora_dataset_destroy(dcora_dataset_t ds);
/* chordalInitialization (ref src/DCORA_solver.cpp:218-268): T is d x (d+1) n column-major (SE ordering), the start
 * point of the reference driver's InitializationMethod::Chordal (ref examples/MultiRobotExample.cpp:150-153) */
int dcora_dataset_chordal_init(dcora_dataset_t ds, double *T);
/* the same with the two sparse SPD systems solved on the device (partitioned inverse built from the device
 * factorisation, one replay each): for graphs whose host factorisation takes minutes (the 100k lattice: 237 s on the
 * host).  Same result up to the rounding of the solves. */
int dcora_dataset_chordal_init_device(dcora_dataset_t ds, int device, double *T);
/* Graph::constructQuadraticCostTermPGO (ref src/Graph.cpp:579-683) for agent `agent_id` owning n poses */
int dcora_graph_build_Q_pgo(int d, int n, int agent_id, int m, const int *ids, const double *vals, dcora_csr_t *Q);

/* Range-aided SLAM, centralised agent (CORA flow of examples/SingleRobotExample_RASLAM.cpp:59-130):
 * read_pyfg_file + getGlobalMeasurements (ref src/DCORA_utils.cpp:437-1167, 1169-1365) and
 * Graph::constructQuadraticCostTermRASLAM (ref src/Graph.cpp:824-1188).  Column ordering of X is the RA ordering. */
typedef struct dcora_radataset_s *dcora_radataset_t;
int dcora_radataset_load_pyfg(const char *path, dcora_radataset_t *out);
/* info[7] = {d, n poses, l unit spheres, b landmarks, #pose-pose, #pose-landmark, #range measurements} */
int dcora_radataset_info(dcora_radataset_t ds, int *info);
/* Graph::setMeasurements(const RelativeMeasurements &) of a range-aided graph (ref include/DCORA/Graph.h:57-147,
 * src/Graph.cpp:374-470): the dataset from measurement arrays instead of a file.  States are numbered as the Graph
 * numbers them: poses 0 .. n - 1, unit spheres 0 .. l - 1 (one per range measurement), landmarks 0 .. b - 1, all owned
 * by robot 0 (the centralised agent).
 *   pose-pose:     pp_ids m_pp x 2 (pose i, pose j); pp_vals m_pp x (d d + d + 3): R column-major, t, kappa, tau, weight
 *   pose-landmark: pl_ids m_pl x 2 (pose i, landmark j); pl_vals m_pl x (d + 2): t, tau, weight
 *   range:         rg_ids m_rg x 5 (type1, i, type2, j, unit sphere; type 0 = pose, 1 = landmark); rg_vals m_rg x 3:
 *                  range, precision, weight
 * gt: d x k ground truth in the RA ordering, or NULL.  dcora_radataset_copy writes a dataset's measurements into the
 * same arrays (any of them may be NULL; sizes from dcora_radataset_info). */
int dcora_radataset_create(int d, int n, int l, int b, int m_pp, const int *pp_ids, const double *pp_vals, int m_pl,
                           const int *pl_ids, const double *pl_vals, int m_rg, const int *rg_ids, const double *rg_vals,
                           const double *gt, dcora_radataset_t *out);
int dcora_radataset_copy(dcora_radataset_t ds, int *pp_ids, double *pp_vals, int *pl_ids, double *pl_vals, int *rg_ids,
                         double *rg_vals);
/* ground truth of the VERTEX records in RA ordering, d x k column-major (unit spheres = normalised state1 - state2) */
int dcora_radataset_ground_truth(dcora_radataset_t ds, double *gt);
int dcora_radataset_build_Q(dcora_radataset_t ds, dcora_csr_t *Q);
/* start point of the centralised CORA driver (ref examples/SingleRobotExample_RASLAM.cpp:92-150 with
 * odometryInitialization, ref src/DCORA_solver.cpp:270-302): odometry chains anchored at their ground-truth first
 * pose, ground-truth unit spheres, landmarks uniform in (-1, 1) from a splitmix64 stream seeded with `seed`
 * (the reference draws them with Matrix::Random).  X0 is d x k in the RA ordering. */
int dcora_radataset_odometry_init(dcora_radataset_t ds, unsigned long long seed, double *X0);
/* Ownership of the merged problem's variables, as the reference splits a multi-robot pyfg file
 * (getRobotMeasurements, ref src/DCORA_utils.cpp:1370-1512; landmark symbols, ref src/Graph.cpp:584-616; unit
 * spheres belong to the SOURCE robot of their range measurement, ref :1092-1097).  Robot ids: 'A' = 0, 'B' = 1,
 * ..., 'M' = 12 is the map.  Any output may be NULL. */
int dcora_radataset_ownership(dcora_radataset_t ds, int *pose_robot, int *sphere_robot, int *landmark_robot);
/* Columns of the global RA ordering owned by `robot`, listed in that agent's own RA ordering
 * [rotations | unit spheres | translations | landmarks]; dims3 = {n_a, l_a, b_a}; own (k entries of room) may be NULL */
int dcora_radataset_agent_columns(dcora_radataset_t ds, int robot, int *dims3, int *own, int *k_a);
/* Host only: the colours dcora_ra_rbcd_agent_colours will give, before any session exists (a driver plans its ranks
 * and its ticks with them; the agents that may fire together, ref src/Agent.cpp:650-678).  Agents = the robots that own
 * poses, in id order; two are adjacent when a measurement has endpoints (or, for a range, its unit sphere) owned by
 * both; greedy in agent order: the smallest colour no lower-numbered neighbour holds.  colours: one int per agent. */
int dcora_radataset_agent_colours(dcora_radataset_t ds, int *colours, int *ncolours);
/* An agent's share of a global quadratic form Q (k x k): Qaa = Q[own, own] in the agent's ordering and the coupling
 * C = Q[own, rest] (k_a x k, GLOBAL column indices), so that the agent's linear term is G_a = X_global C^T -- the
 * restriction the reference assembles measurement by measurement (ref src/Graph.cpp:824-1772) */
int dcora_graph_extract_agent_blocks(int k, const int *rowptr, const int *colidx, const double *vals, int k_a,
                                     const int *own, dcora_csr_t *Qaa, dcora_csr_t *C);
int dcora_radataset_destroy(dcora_radataset_t ds);
/* Graph::computePreconditionerRegularization (ref src/Graph.cpp:1921-1960): reg = lambda_max(Q) / (1e6 - 1), lambda_max
 * by Lanczos (nev 1, ncv 6, tol 1e-3) on the device; falls back to 0.1 when the eigensolver does not converge */
int dcora_graph_precond_regularization(int k, const int *rowptr, const int *colidx, const double *vals, int device,
                                       double *reg);

/* ------------------------------------------------------------------------- *
 * RBCD session: Agents + synchronous driver on device
 * (replaces Agent::iterate/updateX/getSharedStateDicts/updateNeighborStates, ref src/Agent.cpp:113-152,
 *  535-596, 844-906, 1158-1278, and the loop body of examples/MultiRobotExample.cpp:223-307)
 * ------------------------------------------------------------------------- */
typedef struct dcora_rbcd_s *dcora_rbcd_t;
typedef struct {
  int num_robots;
  int r;
  int acceleration;     /* AgentParameters::acceleration */
  int restart_interval; /* AgentParameters::restartInterval (30) */
  dcora_ropt_params local; /* AgentParameters::localOptimizationParams */
  int rank, world_size; /* this process hosts the agents a with a / ceil(num_robots / world_size) == rank:
                           consecutive agents share a rank, so the colours of a chain of agents spread evenly */
  int device;
  void *stream; /* hipStream_t the session enqueues on (e.g. the stream the caller's RCCL calls are ordered on, so
                   pack -> collective -> unpack needs no host synchronisation); NULL: the session creates its own */
} dcora_rbcd_options;
void dcora_rbcd_options_default(dcora_rbcd_options *o);

/* partition (ref examples/MultiRobotExample.cpp:56-118), per-agent Q / preconditioner, central Q */
int dcora_rbcd_create(dcora_dataset_t ds, const dcora_rbcd_options *opt, dcora_rbcd_t *out);
int dcora_rbcd_destroy(dcora_rbcd_t s);
/* Agent::setX for every agent from the global r x (d+1)n matrix (ref examples/MultiRobotExample.cpp:209-217) */
int dcora_rbcd_set_X(dcora_rbcd_t s, const double *X);
int dcora_rbcd_get_X(dcora_rbcd_t s, double *X);
/* one pass of the loop body :223-307 with `selected` as the optimising agent: non-selected iterate(false),
 * public-pose pull, selected iterate(true), central evaluation.  Outputs: 2 f, |rgrad|, per-agent |rgrad_b|
 * (num_robots doubles, may be NULL) and the greedy next selection. */
int dcora_rbcd_iterate(dcora_rbcd_t s, int selected, double *cost2, double *gradnorm, double *block_norms,
                       int *next_selected);
/* runs up to max_iters passes, stopping when |rgrad| < rgrad_tol; fills the trace arrays (may be NULL) */
int dcora_rbcd_run(dcora_rbcd_t s, int max_iters, double rgrad_tol, int *iters_done, double *cost2_trace,
                   double *gradnorm_trace, int *selected_trace);
/* One tick in which the `count` agents of `set` run Agent::iterate(true) at the same time, each on its own HIP
 * stream, every one of them reading the neighbour states as they were when the tick began: what agents that fire
 * together see in the asynchronous mode (Agent::runOptimizationLoop, ref src/Agent.cpp:650-678).  Needs
 * acceleration off, as that mode does (:651-653).  Agents of the set that share measurements are refused unless
 * allow_adjacent != 0; for mutually non-adjacent agents (one colour of dcora_rbcd_agent_colours) the tick equals
 * updating them one after the other with dcora_rbcd_iterate.  Multi-process: every rank passes the same set and
 * solves the agents it hosts; the caller exchanges public poses afterwards. */
int dcora_rbcd_iterate_set(dcora_rbcd_t s, const int *set, int count, int allow_adjacent);
/* AgentParameters::acceleration of every agent; restarts the Nesterov sequences (V = Y = X, gamma = alpha = 0) */
int dcora_rbcd_set_acceleration(dcora_rbcd_t s, int acceleration);
/* greedy colouring of the agent graph (agents adjacent when they share a measurement): colours[num_robots] */
int dcora_rbcd_agent_colours(dcora_rbcd_t s, int *colours, int *ncolours);
/* The coloured run loop (the schedule this library gives the agents that fire together in the asynchronous mode, ref
 * src/Agent.cpp:650-678): a sweep is one dcora_rbcd_iterate_set per colour of dcora_rbcd_agent_colours, colours 0, 1, ...
 * in order, followed by one dcora_rbcd_evaluate; it stops after the first sweep whose |rgrad| < rgrad_tol, at most
 * max_sweeps.  Exactly the calls a caller's own loop makes, so traces and X are the same bits.  Trace entry s (arrays
 * of max_sweeps doubles, may be NULL) is the evaluation after sweep s.  Needs acceleration off, as a tick does;
 * world_size 1 (ranks: dcora_exchange_run_coloured). */
int dcora_rbcd_run_coloured(dcora_rbcd_t s, int max_sweeps, double rgrad_tol, int *sweeps_done, double *cost2_trace,
                            double *gradnorm_trace);
/* the central evaluation of dcora_rbcd_iterate alone (ref examples/MultiRobotExample.cpp:264-305); world_size 1 */
int dcora_rbcd_evaluate(dcora_rbcd_t s, double *cost2, double *gradnorm, double *block_norms, int *next_selected);
/* Agent::iterate(doOptimization) of ONE agent (ref src/Agent.cpp:535-596), for callers that keep the reference's
 * per-agent loop (examples/MultiRobotExample.cpp:223-262).  The agents of a session advance in lockstep: one call
 * per hosted agent and round; the first call of a round advances the shared Nesterov sequences. */
int dcora_rbcd_agent_iterate(dcora_rbcd_t s, int agent, int do_optimization);
/* Agent::updateNeighborStates (ref src/Agent.cpp:844-906): `count` public poses of `neighbor` (frames local to it;
 * poses: count blocks of r x (d+1), column-major) handed to `agent`.  From the first such call on the agent optimises
 * against what it was HANDED -- its own cache of neighbour poses, the plain one or (auxiliary != 0) the one used when
 * it starts from Y -- and no longer against the session's shared mirror: stale poses are used as they are, poses it
 * does not require are ignored (Graph::requireNeighborPose), and an iterate(true) whose cache misses a required pose
 * skips the optimisation (ref src/Agent.cpp:1243-1249; dcora_rbcd_agent_last_skipped tells).  Agents that are never
 * handed anything keep reading the mirror (the session-level loop, dcora_rbcd_iterate). */
int dcora_rbcd_agent_update_neighbor(dcora_rbcd_t s, int agent, int neighbor, int count, const int *frames,
                                     const double *poses, int auxiliary);
int dcora_rbcd_agent_last_skipped(dcora_rbcd_t s, int agent, int *skipped);
/* Agent::getX / setX: the agent's own block, r x (d+1) num_poses (ref src/Agent.cpp:64-77, 98-105) */
int dcora_rbcd_agent_get_X(dcora_rbcd_t s, int agent, double *X);
int dcora_rbcd_agent_set_X(dcora_rbcd_t s, int agent, const double *X);
/* num_poses, first global pose index and Agent::iteration_number() of an agent (any of the outputs may be NULL) */
int dcora_rbcd_agent_info(dcora_rbcd_t s, int agent, int *num_poses, int *first_pose, int *iteration_number);
/* statistics of the last selected agent's local solve */
int dcora_rbcd_last_result(dcora_rbcd_t s, dcora_ropt_result *res);

/* --- multi-process pieces (one process per GPU, exchange through RCCL by the caller) --- */
/* device pointer of the session's global lifted variable (r x (d+1)n, column-major, resident in HBM) */
int dcora_rbcd_X_device_ptr(dcora_rbcd_t s, double **X_dev);
/* number of public poses of agent a, and their global pose indices (ref src/Graph.h myPublicPoseIDs) */
int dcora_rbcd_public_count(dcora_rbcd_t s, int agent, int *count);
int dcora_rbcd_public_indices(dcora_rbcd_t s, int agent, int *global_pose_idx);
/* getSharedStateDicts: gather agent's public poses into a packed r x (d+1)count device buffer */
int dcora_rbcd_pack_public_dev(dcora_rbcd_t s, int agent, double *packed_dev);
/* updateNeighborStates: scatter a packed buffer received from agent's owner into the local mirror of X */
int dcora_rbcd_unpack_public_dev(dcora_rbcd_t s, int agent, const double *packed_dev);
/* the three phases of dcora_rbcd_iterate for callers that exchange between them */
int dcora_rbcd_phase_nonselected(dcora_rbcd_t s, int selected);
int dcora_rbcd_phase_selected(dcora_rbcd_t s, int selected);
/* debug counter (read-only): the kernel launches of the RBCD chain -- evaluations, Nesterov steps, G, the RTR
 * bookkeeping and tCG kernels, the evaluation epilogue -- that this session's dcora_rbcd_iterate calls have enqueued
 * since creation.  Meaningful while one session iterates at a time. */
int dcora_debug_rbcd_launches(dcora_rbcd_t s, long long *launches);
/* the same counter of the whole process (every session and exchange of either kind, since the library was loaded) */
int dcora_debug_launch_count(long long *launches);
/* local part of the evaluation: for every hosted agent b, |Proj(X_b Q_bb + G_b)|^2 and <X_b, X_b Q_bb + G_b>
 * written to out_dev[2*b], out_dev[2*b+1] (device, 2*num_robots doubles, entries of non-hosted agents zero) */
int dcora_rbcd_phase_evaluate_dev(dcora_rbcd_t s, double *out_dev);
int dcora_rbcd_synchronize(dcora_rbcd_t s);
/* The certificate of a live single-process session, on the device: fastVerification(S, eta, &theta, &v) (ref
 * src/DCORA_utils.cpp:1713-1735) on S = Q - Lambda(X) with the Q the session's central problem holds NOW -- the weights
 * the last dcora_rbcd_update_weights / _set_weights left -- and the session's current iterate.  X Q, the Lambda blocks,
 * the values of S + eta I (in the CSR order of the central pattern) and the Cholesky factorisation all run where the
 * session's data is; an accepted certificate moves only the verdict to the host.  *certified (required) = 1: S + eta I
 * has a Cholesky factorisation.  Otherwise *lambda_min and v (k doubles, the session's global ordering) are the minimum
 * eigenpair of S + eta I and *theta = v^T S v, as dcora_cert_fast_verification reports them.  theta, lambda_min, v,
 * matvecs (Lanczos products) and info8 (as dcora_cert_is_psd_device) may be NULL.  The factorisation orders d + 1
 * unknowns together (range-aided sessions: 1) and shares its analysis cache with the host-fed calls: after
 * dcora_cert_prepare on Q's pattern it starts with the numeric phase.  Where Q's pattern lacks an entry of Lambda or of
 * the diagonal (a structural zero inside a rotation block, an isolated pose, a unit sphere without a range) the values
 * are gathered on the pattern with those entries added, the one dcora_cert_dual_matrix produces: still on the device.
 * The session is left as it was: a run after the call equals the run without it.
 * world_size > 1: DCORA_ERR_UNSUPPORTED (the ranks certify together: dcora_exchange_certify). */
int dcora_rbcd_certify(dcora_rbcd_t s, double eta, int *certified, double *theta, double *lambda_min, double *v,
                       long long *matvecs, double *info8);
/* The Riemannian staircase's step inside a live single-process session (ref examples/MultiRobotExample.cpp:352-366,
 * examples/MultiRobotExample_RASLAM.cpp, src/QuadraticProblem.cpp:138-234).  The reference makes a new set of agents
 * per level; here the session that dcora_rbcd_certify has refused goes from rank r to r + 1 in place: escapeSaddle of
 * the whole-graph problem along (theta, v) -- what the certificate returned, v: k doubles on the host -- runs on the
 * device from the session's iterate, which never crosses to the host, and the accepted point becomes the session's
 * iterate as dcora_rbcd_set_X would make it (V = Y = XPrev = X, Nesterov sequences and round counters restarted, a
 * robust session's X_initial, team statuses cleared).  Everything that does not depend on r stays: matrices,
 * preconditioners, neighbours, colours, the robust weights with mu and the update count, the team with its parameters
 * and loop-closure counts, the certificate's tables.  Poses handed over with dcora_rbcd_agent_update_neighbor are
 * dropped, and a pointer obtained from dcora_rbcd_X_device_ptr is void after a lift that escaped.
 * The search is src/QuadraticProblem.cpp:161-233's: the first trial step, in order, that lowers f with both gradient
 * norms above their tolerances; else the trial of least f if it lowers f; else *escaped = 0 and the session is as it
 * was.  The whole-graph problem's preconditioner is built on the first call and again after a weight change, of the
 * matrix the session holds, with central_reg or, where that is negative, the kind's default: 0.1 on a pose graph, the
 * reference's lambda_max / (1e6 - 1) rule (dcora_graph_precond_regularization) on a range-aided session.
 * info8 (may be NULL): trials, accepted alpha, f before, f after, 1 if the preconditioner was built in this call, its
 * ms, ms of the re-dimensioning, ms total.
 * DCORA_ERR_UNSUPPORTED: world_size > 1, a ranked robust / team session, a session with an exchange -- those lift
 * together through dcora_exchange_lift (below).
 * DCORA_ERR_BAD_ARG: r = 16; v or params NULL; v, theta or a tolerance not finite. */
typedef struct {
  double gradient_tolerance, preconditioned_gradient_tolerance;
  int is_second_order;
  double central_reg;
} dcora_lift_params;
int dcora_lift_params_default(dcora_lift_params *p); /* 1e-6, 1e-6, 0, -1 (= the kind's default) */
int dcora_rbcd_lift(dcora_rbcd_t s, double theta, const double *v, const dcora_lift_params *p, int *escaped,
                    double *info8);
/* the session's current relaxation rank: the r of the staircase loop after the lifts so far (ref
 * examples/MultiRobotExample.cpp:352-366, examples/MultiRobotExample_RASLAM.cpp, src/QuadraticProblem.cpp:138-234) */
int dcora_rbcd_rank(dcora_rbcd_t s, int *r);
/* Room for the ranks to come (a job that will climb the staircase through dcora_exchange_lift): an exchange created on
 * the session afterwards sizes its halo slots, its staged slots and its gather_X area by max(r, r_reserve) instead of
 * r, so that the job can lift up to r_reserve without another segment; nothing else of the layout, no allocation of
 * the session and no launch depends on it, and a session that never calls this is laid out exactly as before.  Legal
 * between the session's creation and dcora_exchange_create.  Every rank of a job reserves the same rank.
 * DCORA_ERR_BAD_ARG unless d <= r <= r_reserve <= 16; DCORA_ERR_UNSUPPORTED once an exchange exists on the session
 * (its segment is unlinked after creation and its IPC mappings are fixed: an exchange does not grow). */
int dcora_rbcd_reserve_rank(dcora_rbcd_t s, int r_reserve);
/* The last step of a solve, on the device where the iterate lies: the session's current iterate rounded to SE(d) in
 * the frame of an anchor, as the reference's drivers end -- agents[0]->getSharedPose(0, &M), setGlobalAnchor(M) on every
 * agent, then each agent's getTrajectoryInGlobalFrame (ref examples/MultiRobotExample.cpp:341-347,
 * examples/MultiRobotExample_RASLAM.cpp:488-495, src/Agent.cpp:1014-1033; the alignment: src/DCORA_utils.cpp:2262-2289):
 *   T_i = [ Proj_SO(d)(R0^T Y_i) | R0^T p_i - R0^T p_anchor ].
 * anchor NULL: the lifted pose anchor_pose (a global pose index; 0 is what the reference's drivers share) of the current
 * iterate is the anchor, read on the device -- no host round trip precedes the kernel.  anchor given: r x (d+1) doubles
 * on the host, column-major (setGlobalAnchor(M)).  Either way the anchor's translation is the origin.
 * trajectory: d x (d+1) n doubles, the SE ordering (what dcora_round_align_trajectory returns for the same X and anchor,
 * up to rounding: every element here is one sum in index order through fma).
 * cost2 (may be NULL): 2 f of the rounded solution on the matrix the session holds NOW (its current robust weights),
 * evaluated at the lifted rounded point R0 [R_i | t_i], which is feasible at rank r and has the rounded solution's cost:
 * no rank-d problem is created and no Q is uploaded.  This is the number to set against the certified lower bound.
 * info4 (may be NULL): the Riemannian gradient norm at that point, ms of the rounding kernels, ms of the evaluation, ms
 * total.  The session is left as it was: a run after the call equals the run without it, bit for bit.
 * DCORA_ERR_BAD_ARG: trajectory NULL, anchor_pose outside 0 .. n - 1, a non-finite anchor.
 * DCORA_ERR_UNSUPPORTED: world_size > 1 (the ranks round together: dcora_exchange_round). */
int dcora_rbcd_round(dcora_rbcd_t s, int anchor_pose, const double *anchor, double *trajectory, double *cost2,
                     double *info4);
/* How CORA ends a certified solve, on the live session (ref examples/SingleRobotExample_RASLAM.cpp:220-234,
 * projectSolutionRASLAM src/DCORA_utils.cpp:1984-2031): the session goes from rank r to rank d, in place, at
 *   Proj(V_d^T X),   V_d = the top-d eigenvectors of G = X X^T (r x r), its last column negated where fewer than n / 2
 * (integer division) of the blocks V_d^T Y_i have a positive determinant;
 * rotation blocks projected to SO(d), unit-sphere columns normalised (a zero column stays zero), translation and
 * landmark columns truncated only.  G is formed on the device in one pass over X, without floating-point atomics and
 * with a fixed number of columns per workgroup: the same X gives the same G bit for bit, on any device; its r x r
 * eigenproblem is solved on the host (equal eigenvalues keep the order of their index).  Everything dcora_rbcd_lift
 * keeps is kept (matrices, preconditioners, robust weights, mu and the update count, the team and its parameters, a
 * reserved rank); everything dcora_rbcd_set_X resets is reset.  Afterwards dcora_rbcd_rank reports d and the session
 * behaves as a session created at rank d and handed the same point.  (A session created above rank 8 keeps the CSR
 * form of its matrices, as after any re-rank.)
 * r == d: the reference passes X through unprojected; sigma, gram and cost2 are produced, info8[0] = 0 and nothing of
 * the session changes.
 * Every output may be NULL.  sigma: r doubles, the singular values of X, descending (square roots of G's eigenvalues,
 * round-off below zero clamped).  basis: r x d doubles column-major, V_d as applied (written only where the session was
 * projected): the new iterate is exactly Proj(basis^T X).  gram: r x r doubles, G as the device formed it.  cost2: 2 f
 * of the adopted point on the matrix the session holds NOW (its current robust weights).  info8: projected (0 / 1),
 * reflected (0 / 1), rotation blocks with positive determinant before the reflection decision, |rgrad| at the adopted
 * point, ms of the projection kernels, ms of the re-dimensioning, ms total, columns per workgroup of the Gram kernel.
 * DCORA_ERR_UNSUPPORTED, the session untouched: a rank of a job, a ranked robust or team session, a session an exchange
 * was created on (those project together, through dcora_exchange_project below). */
int dcora_rbcd_project(dcora_rbcd_t s, double *sigma, double *basis, double *gram, double *cost2, double *info8);
/* Debug entry of the tests: the one-pass Gram kernel of dcora_rbcd_project on a host array.  X: r x k column-major,
 * 1 <= r <= 16, k >= 1; gram: r x r; *chunk (may be NULL): columns per workgroup. */
int dcora_debug_project_gram(int r, long long k, const double *X, double *gram, int *chunk);
/* Debug entry of the tests: the agent form of the lift's image kernel (k_lift_images).  From Xa (r x ka column-major:
 * one agent's block), the global v (kglobal doubles) and the agent's column map -- cols (ka global column indices) or,
 * with cols NULL, the contiguous range starting at col0 -- Xplus = [Xa; 0] and dir = [0; v_a^T], each (r + 1) x ka.
 * All arrays on the host.  DCORA_ERR_BAD_ARG: r outside 1..15, ka < 1 or a column outside 0..kglobal-1. */
int dcora_debug_lift_images(int r, int ka, const double *Xa, int kglobal, const double *v, const int *cols, int col0,
                            double *Xplus, double *dir);
/* Measurement hook (bench.py's `roofline`): while enabled, HIP events are recorded on the solver's stream around every
 * one-launch tCG run (k_tcg_run) of the session's agents; _read waits for the stream, returns {launches, sum of their
 * event times in us} since the last read and forgets them.  Not for timed regions: an event pair costs a few us. */
int dcora_rbcd_profile_tcg_runs(dcora_rbcd_t s, int enable);
int dcora_rbcd_profile_tcg_read(dcora_rbcd_t s, double *out2);

/* ------------------------------------------------------------------------- *
 * Neighbour exchange between the ranks of one node (one process per GPU): the transport the reference leaves to its
 * host -- Agent::getSharedStateDicts on the sender, Agent::updateNeighborStates on the receiver (ref src/Agent.cpp:
 * 113-152, 844-906), moved by the driver (ref examples/MultiRobotExample.cpp:236-258).  An exchange belongs to a
 * session created with rank / world_size; every rank of the job creates one under the same job name (unique per job
 * on the node: it names a POSIX shared-memory segment that carries the bootstrap, the flag words and the evaluation
 * scalars).  Pose data moves by direct stores into the halo buffer of each rank that hosts a NEIGHBOUR of the posting
 * agent (peer memory mapped through HIP IPC, xGMI between GPUs); there is no collective on the data path.  If the IPC
 * transport is not usable on some rank, all ranks stage the packed poses in the shared host segment instead
 * (dcora_exchange_info reports which).  All calls are SPMD: every rank makes the same calls with the same agent lists.
 * ------------------------------------------------------------------------- */
typedef struct dcora_exchange_s *dcora_exchange_t;
int dcora_exchange_create(dcora_rbcd_t s, const char *job_name, dcora_exchange_t *out);
int dcora_exchange_destroy(dcora_exchange_t ex);
/* info[10] = {transport (1 = IPC peer stores, 2 = shared host segment), ranks this rank stores to, posts, waits,
 * bytes posted so far, host seconds in post, host seconds in wait, host seconds waiting for the evaluation scalars,
 * 1 when this rank's halo buffer is fine-grained device memory (remote stores never served stale from the local L2),
 * 1 when the scatter kernel itself waits for the producer's flag (default where every rank has a GPU of its own and a
 * fine-grained halo buffer; DCORA_EXCHANGE_WAIT=host: the host spins)}.
 * dcora_exchange_create ends with a LINK CHECK when there is more than one rank: every rank stores a 4 KB pattern and a
 * flag into each rank it will write to, through the transport and the form of the wait it is about to use, and every
 * reader waits for the flag (bounded: 3 s) and compares the pattern word for word.  When any rank's check fails all
 * ranks step down together -- device-side wait -> host wait -> shared host segment instead of IPC peer stores -- and
 * check again; when nothing passes, the call returns DCORA_ERR_EXCHANGE_LINK on every rank within seconds instead of
 * hanging in the first post.  dcora_exchange_link_report says what was tried. */
int dcora_exchange_info(dcora_exchange_t ex, double *info10);
/* out[4] = {rounds of the link check run, 1 if the device-side wait was given up, 1 if the IPC transport was given up,
 * microseconds of the last (passed) round} */
int dcora_exchange_link_report(dcora_exchange_t ex, double *out4);
/* getSharedStateDicts of `agents`: each hosted one is written to its neighbours' ranks and flagged (one kernel per
 * agent on the session's stream; returns without synchronising).  A slot is re-used two posts later: the call first
 * waits until every reading rank has scattered that older post (an error after 120 s, never a torn read), so a post
 * may run at most two ahead of the dcora_exchange_wait calls of its readers. */
int dcora_exchange_post(dcora_exchange_t ex, const int *agents, int count);
/* updateNeighborStates: waits until the posts of those of `agents` that neighbour an agent hosted here have
 * arrived and scatters them into the session's mirror of X (enqueued on the session's stream) */
int dcora_exchange_wait(dcora_exchange_t ex, const int *agents, int count);
/* the driver's evaluation (ref examples/MultiRobotExample.cpp:264-305) without a central copy of X: every rank
 * evaluates |Proj(X_b Q_bb + G_b)| and <X_b, X_b Q_bb + G_b> of its agents, 2 R scalars are all-gathered through
 * the shared segment; same outputs as dcora_rbcd_evaluate, identical on every rank */
int dcora_exchange_evaluate(dcora_exchange_t ex, double *cost2, double *gradnorm, double *block_norms,
                            int *next_selected);
/* dcora_rbcd_iterate across the ranks: non-selected updates, post + wait, the selected agent's solve on its rank,
 * post + wait of its new public poses, evaluation */
int dcora_exchange_rbcd_iterate(dcora_exchange_t ex, int selected, double *cost2, double *gradnorm,
                                double *block_norms, int *next_selected);
/* dcora_rbcd_iterate_set across the ranks, followed by post + wait of the updated agents */
int dcora_exchange_rbcd_tick(dcora_exchange_t ex, const int *set, int count, int allow_adjacent);
/* dcora_rbcd_run_coloured / dcora_ra_rbcd_run_coloured across the ranks (ref src/Agent.cpp:650-678): per sweep one
 * dcora_exchange_rbcd_tick per colour of the greedy colouring (every rank computes the same one from the agents'
 * neighbour lists), then dcora_exchange_evaluate.  SPMD; sweeps_done and the traces are identical on every rank. */
int dcora_exchange_run_coloured(dcora_exchange_t ex, int max_sweeps, double rgrad_tol, int *sweeps_done,
                                double *cost2_trace, double *gradnorm_trace);
/* dcora_rbcd_set_X on every rank between two barriers; dcora_rbcd_get_X of the whole X assembled from the ranks that
 * host each block (collective; X is valid on every rank) */
int dcora_exchange_set_X(dcora_exchange_t ex, const double *X);
int dcora_exchange_gather_X(dcora_exchange_t ex, double *X);
/* The Riemannian staircase's step of a whole job (ref examples/MultiRobotExample.cpp:352-366,
 * examples/MultiRobotExample_RASLAM.cpp, src/QuadraticProblem.cpp:138-234): dcora_rbcd_lift's contract carried across
 * the ranks, on the exchange of a pose-graph or a range-aided session.  SPMD: every rank calls it with the same theta,
 * the same v (k doubles on the host, global ordering, as dcora_exchange_certify returns it) and the same params.  The
 * job goes from rank r to r + 1 without leaving the library: no agent's X crosses to the host, no session and no
 * exchange is destroyed, and a robust job keeps mu, its update count and its team.
 * The search is src/QuadraticProblem.cpp:161-233's, the statement dcora_rbcd_lift runs: first step length and halving;
 * the first trial that lowers f with both gradient norms above their tolerances; else the trial of least f if it
 * lowers f; else *escaped = 0.  Per trial each rank retracts the blocks of [X; 0] + alpha [0; v^T] of the agents it
 * hosts at rank r + 1, the public columns travel with the ordinary post and wait of all agents, and every scalar a
 * decision uses is summed over the ranks in rank order, so that all ranks decide alike.
 * ONE DIFFERENCE from the reference and from dcora_rbcd_lift: no rank holds the whole graph, so the third test uses
 * the agents' own preconditioners, |P grad|^2 := sum_a |Proj(rgrad_a M_a^-1)|^2 with the images the agents' solves
 * use (their own regularisation).  params->central_reg is ignored here, at any world_size: the exchange of a
 * one-rank job takes this same path.
 * Escaped: every hosted agent's problem is at r + 1, the sessions' buffers are re-dimensioned and the accepted point is
 * adopted on every rank at once as dcora_exchange_set_X adopts one (V = Y = XPrev = X, Nesterov sequences and round
 * counters restarted, a robust job's X_initial, team statuses cleared on every rank alike); dcora_rbcd_rank /
 * dcora_ra_rbcd_rank report r + 1.  Matrices, preconditioners, weights, mu and its update count, team parameters and
 * loop-closure counts, and the exchange with its transport stay.
 * No escape, or an error on any rank: the job is as it was (the trials ran beside the sessions' mirrors), and its next
 * iterates are those of a job that never called this.  A failure on one rank raises the segment's `failed` word as in
 * every collective call; every wait is bounded by DCORA_EXCHANGE_TIMEOUT_S.
 * Refused on every rank alike, the job untouched: DCORA_ERR_BAD_ARG for r = 16, v or params NULL, v, theta or a
 * tolerance not finite; DCORA_ERR_UNSUPPORTED when r + 1 exceeds max(r at the exchange's creation, the reserve):
 * reserve with dcora_rbcd_reserve_rank / dcora_ra_rbcd_reserve_rank or the *_create_robust_ranks_reserved entries.
 * info8 (may be NULL): trials, accepted alpha, f before, f after, 0, 0, ms of the re-dimensioning, ms total. */
int dcora_exchange_lift(dcora_exchange_t ex, double theta, const double *v, const dcora_lift_params *params,
                        int *escaped, double *info8);
/* dcora_rbcd_round / dcora_ra_rbcd_round across the ranks of a job (ref examples/MultiRobotExample.cpp:341-347,
 * examples/MultiRobotExample_RASLAM.cpp:488-495: every agent rounds its OWN trajectory against the shared anchor;
 * src/Agent.cpp:1014-1033).  Collective and SPMD, every rank with the same arguments.  An anchor named by anchor_pose
 * travels from the rank that hosts it to every rank through the segment's sums (the others add zeros, in rank order: the
 * hosting rank's bits arrive, a -0 as +0, which changes no sum of the kernel); a passed anchor (r x (d+1), host) is used
 * as it is.  Every rank rounds the poses, unit spheres and landmarks of the agents it hosts from those agents' own
 * blocks with the single-process kernel, the pieces are assembled through the segment's X area as dcora_exchange_gather_X
 * assembles X (they need d / r of its room), and every rank returns the whole trajectory (d x (d+1) n) and, on a
 * range-aided job, unit_spheres (d x l) and landmarks (d x b) where those are not NULL: the bits a single-process
 * session at the same iterate returns.  There is no rounded cost across ranks: no rank holds the whole problem.
 * The job is left as it was.  DCORA_ERR_BAD_ARG, decided from the arguments alone before any collective step:
 * trajectory NULL, anchor_pose outside 0 .. n - 1, a non-finite anchor.  A failure on one rank raises `failed` as in
 * every collective call; every wait is bounded by DCORA_EXCHANGE_TIMEOUT_S. */
int dcora_exchange_round(dcora_exchange_t ex, int anchor_pose, const double *anchor, double *trajectory,
                         double *unit_spheres, double *landmarks);
/* dcora_rbcd_project / dcora_ra_rbcd_project across the ranks of a job: how CORA ends a certified solve (ref
 * examples/SingleRobotExample_RASLAM.cpp:220-234, projectSolutionRASLAM src/DCORA_utils.cpp:1984-2031), on the exchange
 * of a pose-graph or a range-aided session -- plain or robust, with or without the ranked team, at any world_size (a
 * one-rank exchange takes this same path).  Collective and SPMD.  The job goes from rank r to rank d at Proj(V_d^T X)
 * without leaving the library: no X crosses to a host and no session or exchange is destroyed.
 *   G = X X^T = sum over the agents of G_a = X_a X_a^T.  Every rank forms G_a of the agents it hosts, from their own
 * blocks, in one launch pair; the matrices reach every rank per agent and unchanged (through the segment) and every rank
 * adds them in agent order 0 .. R - 1.  G therefore has the same bits on every rank, for any number of ranks and either
 * transport; it is the single-process session's G bit for bit only where the job has one agent (that one sums
 * workgroups over the whole mirror).  Every rank solves the same r x r eigenproblem: the same V_d, no broadcast.  The
 * blocks with positive determinant are counted by the hosting ranks and summed over the job (integers: exact); the
 * reflection rule uses the job's n.  Every rank projects its hosted blocks, the public columns travel at d rows with the
 * ordinary post and wait of all agents, and every rank adopts the point at once between barriers, as dcora_exchange_lift
 * does, with what that keeps (matrices, preconditioners, robust weights with mu and the update count, team parameters
 * and loop-closure counts, the exchange, its transport and its rank capacity: a projected job can lift again) and what
 * it resets (statuses, sequences, round counters; X_initial is the adopted point).
 * r == d: nothing of the job changes; sigma and gram are produced, cost2 and info8[3] are dcora_exchange_evaluate's.
 * Outputs as dcora_rbcd_project, every one may be NULL: sigma (r), basis (r x d, where projected), gram (r x r), cost2
 * and info8[3] (dcora_exchange_evaluate at the adopted point, bit for bit what a following call returns), info8 =
 * {projected, reflected, positive determinants before the reflection over the JOB, |rgrad|, ms of the projection kernels
 * on this rank, ms of the re-dimensioning, ms total, columns per workgroup of the Gram kernel}.  Everything but the three
 * times has the same bits on every rank.
 * An error on any rank before the adoption leaves the job as it was (the point was formed beside the sessions'
 * mirrors) and raises the segment's `failed` word as in every collective call; every wait is bounded by
 * DCORA_EXCHANGE_TIMEOUT_S. */
int dcora_exchange_project(dcora_exchange_t ex, double *sigma, double *basis, double *gram, double *cost2,
                           double *info8);
/* Debug entry of the tests: the block-list Gram kernel pair of dcora_exchange_project on host arrays.  X: the blocks one
 * after another, block b r x k[b] column-major (k[b] >= 0); grams: nblocks x r x r, block b's bit for bit what
 * dcora_debug_project_gram gives on that block alone (zeros for k[b] = 0); *chunk (may be NULL): columns per workgroup. */
int dcora_debug_project_gram_blocks(int r, int nblocks, const long long *k, const double *X, double *grams, int *chunk);
/* Measurement entry (tools/project_ranks_cost.py): the block-list pair against a loop of the single-block pair over the
 * same blocks (every k[b] >= 1, zeros as data), alternated `reps` times after one warm-up each; loop_us, pair_us: reps
 * event times in microseconds. */
int dcora_debug_project_gram_time(int r, int nblocks, const long long *k, int reps, double *loop_us, double *pair_us);
/* test / measurement hook: while on, dcora_exchange_project moves the per-agent Gram matrices through the segment's
 * sums (pieces of 31 doubles, zeros from the ranks that do not host the agent) instead of its X area; the same bits
 * either way.  Every rank of the job calls it with the same value. */
int dcora_debug_exchange_project_sums(int on);
/* host barrier over the ranks of the job (does not synchronise the device) */
int dcora_exchange_barrier(dcora_exchange_t ex);
/* Agent::shouldTerminate's team condition (ref src/Agent.cpp:1137-1153: terminate only when EVERY robot reports
 * readyToTerminate): the AND of the ranks' flags through the shared segment.  SPMD; *all_ready is the same everywhere. */
int dcora_exchange_all_ready(dcora_exchange_t ex, int ready, int *all_ready);
/* fastVerification of the current iterate across the ranks (ref src/DCORA_utils.cpp:1713-1735 on the global
 * S = Q - Lambda(X); the driver calls it where examples/MultiRobotExample.cpp:329-330 does).  SPMD.  The global
 * connection Laplacian Q (k = (d+1) n, CSR) is needed on rank 0 only (NULL elsewhere): rank 0 assembles S from the
 * gathered X and runs the PSD test (Cholesky of S + eta I on its device).  When that fails the minimum eigenpair of
 * S + eta I is computed by ALL ranks: each applies the row block of S of the agents it hosts (Q_bb, the coupling
 * blocks, the Lambda blocks of its poses) to its slice of the Lanczos vectors, the public entries travel between
 * neighbouring ranks like public poses, and every inner product is summed over the ranks through the shared segment in
 * rank order (the same bits everywhere).  *certified: 1 = S + eta I >= 0; otherwise *theta = v^T S v (the curvature
 * escapeSaddle takes), *lambda_min = the eigenvalue of S + eta I, v (NULL or k doubles) its unit eigenvector, the same
 * on every rank; *distributed: 1 when the eigenpair came from the row-block Lanczos runs, 0 when they did not
 * converge and rank 0's shift-and-invert fallback (a factorisation of the whole matrix) supplied it. */
int dcora_exchange_certify(dcora_exchange_t ex, int k, const int *rowptr, const int *colidx, const double *vals,
                           double eta, int *certified, double *theta, double *lambda_min, double *v, long long *matvecs,
                           int *distributed);
/* The same certificate of the matrices the job really holds (ref src/DCORA_utils.cpp:1713-1735, 1898-1982, called where
 * examples/MultiRobotExample.cpp:321-335 certifies): no Q is passed in and no X crosses to a host.  SPMD, every rank
 * with the same eta, on the exchange of a pose-graph or a range-aided session, robust or plain, at any world_size, with
 * either transport, after any number of dcora_exchange_lift / _update_weights / _set_weights calls.  Every rank forms
 * the values of ITS rows of M = (Q - Lambda) + eta I from its agents' device matrices as they are now -- the current
 * weights, explicit zeros where a weight is 0 -- and the Lambda blocks of its agents, in the CSR order of the job-wide
 * pattern (the one dcora_cert_dual_matrix gives for the job's creation-time Q: Q's entries, Lambda's, every diagonal),
 * one thread per stored entry, no atomics: the same bits on every call.  The values reach rank 0 through the X area of
 * the segment (max(r at creation, reserve) * k doubles) in as many rounds as they need; rank 0 factorises them on its
 * device (blocks of d + 1 unknowns on a pose graph, 1 on a range-aided job; the analysis cache is the one
 * dcora_cert_prepare fills) and the verdict goes to every rank.  Refused: the row-block Lanczos stage of
 * dcora_exchange_certify, with M downloaded once on rank 0 -- and with dcora_cert_min_eig's rule for a spectrum so wide
 * (eta / lambda_max < 1e-8: tiers.pyfg) that the spectrum-shifted run is not attempted: rank 0's shift-and-invert run
 * on the downloaded values supplies the eigenpair, *distributed = 0; an accepted certificate moves nothing but the verdict.
 * Outputs as dcora_exchange_certify's, the same bits on every rank; certified is required, the others may be NULL.
 * info10 (may be NULL): [0..7] as dcora_cert_is_psd_device reports, [8] the rounds through the X area, [9] ms from entry
 * to the verdict on rank 0.  The job is left as it was: its next iterates are those of a job that never called this.
 * DCORA_ERR_BAD_ARG, decided from the arguments alone before any collective step (the job untouched, the segment's
 * `failed` word not raised): certified NULL, eta not finite or negative.  A failure on one rank raises `failed` as in
 * every collective call; every wait is bounded by DCORA_EXCHANGE_TIMEOUT_S. */
int dcora_exchange_certify_live(dcora_exchange_t ex, double eta, int *certified, double *theta, double *lambda_min,
                                double *v, long long *matvecs, int *distributed, double *info10);
/* Debug entry of the tests, all arrays on the host, no device: the addressing of dcora_exchange_certify_live for ONE
 * agent.  dims and (rowptr, colidx, vals): the job's global Q (k rows); agent_dims and cols: the agent's own dimensions
 * (its n, l, b and layout) and the global column of each of its ka columns, in its ordering; lambda: its Lambda values
 * as the device leaves them (n_a d x d blocks column-major, then l_a scalars).  The agent's Q_aa and coupling block are
 * cut out of Q, the table of its rows is built and checked as the job builds it, and a host loop in the kernel's place
 * writes the entries whose positions lie in [lo, hi) of the value array to window[pos - lo] and counts them up in
 * written[pos - lo] (hi - lo doubles / bytes; the caller zeroes them).  round_size > 0: [lo, hi) is walked as the job
 * walks the value array, in rounds of round_size entries, each round a window of its own.  *nnz_pattern (may be NULL): stored entries of
 * the job-wide pattern.  corrupt_entry >= 0: test hook, the source index of that table entry is pushed past its array
 * before the check.  DCORA_ERR_BAD_ARG: a table that fails its check, a window outside the value array, bad dims. */
int dcora_debug_cert_rows(const dcora_dims *dims, const int *rowptr, const int *colidx, const double *vals,
                          const dcora_dims *agent_dims, const int *cols, const double *lambda, double eta, long long lo,
                          long long hi, long long round_size, double *window, unsigned char *written,
                          long long *nnz_pattern, long long corrupt_entry);
/* the host half of the protocol alone, without a device: bootstrap through the shared segment, barriers, and
 * `rounds` rounds of post -> wait -> evaluation all-gather with host stores in the device's place; every rank of the
 * job calls it, *checksum comes out identical on all of them.  For multi-process tests on machines without a GPU. */
int dcora_exchange_host_selftest(const char *job_name, int rank, int world_size, int num_agents, int rounds,
                                 double *checksum);
/* the team protocol's half of the same rehearsal (dcora_exchange_team_enable's status slots and waits, host stores in
 * the device's place): per round one agent (round % num_agents) "optimises" behind an evaluation heartbeat, every
 * third round a set of non-adjacent agents as a tick without one; the owner publishes a relative change and a success
 * flag that are fixed functions of (round, agent), every rank collects, settles by dcora_team_ready_to_terminate and
 * decides by dcora_team_decide.  Rank q sleeps q * skew_us per round.  *checksum folds every status and both decisions
 * of every round: identical on every rank and for every skew. */
int dcora_exchange_host_selftest_team(const char *job_name, int rank, int world_size, int num_agents, int rounds,
                                      int skew_us, double *checksum);
/* test hook: leaves under the job's name what a crashed job of the same shape would (an initialised segment whose
 * creator is gone); a job started afterwards under that name must not attach to it */
int dcora_debug_exchange_leave_stale(const char *job_name, int world_size, int num_agents);
/* test hook: the link check of exchanges created afterwards in this process reports its first `rounds` rounds as failed
 * on the last rank (every rank of the job calls it with the same value), so the step-down ladder and
 * DCORA_ERR_EXCHANGE_LINK can be exercised on healthy hardware */
int dcora_debug_exchange_probe_fault(int rounds);

/* ------------------------------------------------------------------------- *
 * RBCD session for multi-robot range-aided SLAM (replaces the Agents on a RangeAidedSLAMGraph and the loop body of
 * examples/MultiRobotExample_RASLAM.cpp; ref src/Agent.cpp:535-596, 1158-1278, src/Graph.cpp:824-1772).
 * Agents = the robots of the pyfg file that own poses, in id order; variables are owned as the reference assigns
 * them (dcora_radataset_ownership); X is the merged problem's r x k matrix in the RA ordering.  Files in which the
 * passive map agent would own a landmark or a unit sphere are refused (DCORA_ERR_UNSUPPORTED).  One process.
 * ------------------------------------------------------------------------- */
typedef struct dcora_ra_rbcd_s *dcora_ra_rbcd_t;
/* opt->num_robots is ignored (the file decides); opt->local are the agents' localOptimizationParams */
int dcora_ra_rbcd_create(dcora_radataset_t ds, const dcora_rbcd_options *opt, dcora_ra_rbcd_t *out);
/* the same exchange for the agents of a multi-robot range-aided SLAM problem (ref examples/MultiRobotExample_RASLAM.cpp;
 * ownership by robot symbol, src/DCORA_utils.cpp:1370-1512): the session was created by dcora_ra_rbcd_create with
 * rank / world_size (agent i on rank i / ceil(R / world_size)); an agent's public variables are its poses, unit spheres
 * and landmarks that other agents' measurements reach.  Every dcora_exchange_* call but the team protocol works as for
 * pose graphs: _set_X / _rbcd_iterate / _rbcd_tick / _run_coloured / _evaluate / _gather_X / _post / _wait /
 * _all_ready / _certify (k = the merged problem's columns, Q = dcora_radataset_build_Q on rank 0); the weight updates
 * of a robust job on the exchange dcora_ra_rbcd_create_robust_ranks makes. */
int dcora_exchange_create_ra(dcora_ra_rbcd_t s, const char *job_name, dcora_exchange_t *out);
int dcora_ra_rbcd_destroy(dcora_ra_rbcd_t s);
/* number of agents and (robots != NULL) their robot ids ('A' = 0, ...) */
int dcora_ra_rbcd_info(dcora_ra_rbcd_t s, int *num_agents, int *robots);
int dcora_ra_rbcd_set_X(dcora_ra_rbcd_t s, const double *X);
int dcora_ra_rbcd_get_X(dcora_ra_rbcd_t s, double *X);
/* dcora_rbcd_certify on the merged range-aided problem (v: k doubles in the global RA ordering) */
int dcora_ra_rbcd_certify(dcora_ra_rbcd_t s, double eta, int *certified, double *theta, double *lambda_min, double *v,
                          long long *matvecs, double *info8);
/* dcora_rbcd_lift / dcora_rbcd_rank on a range-aided session (ref examples/MultiRobotExample.cpp:352-366,
 * examples/MultiRobotExample_RASLAM.cpp, src/QuadraticProblem.cpp:138-234): v in the global RA ordering; every agent's
 * X, V, Y, XPrev in its own ordering are re-dimensioned with the mirror */
int dcora_ra_rbcd_lift(dcora_ra_rbcd_t s, double theta, const double *v, const dcora_lift_params *p, int *escaped,
                       double *info8);
int dcora_ra_rbcd_rank(dcora_ra_rbcd_t s, int *r);
/* dcora_rbcd_round on a range-aided session (ref examples/MultiRobotExample_RASLAM.cpp:488-495,
 * src/Agent.cpp:1014-1033): trajectory d x (d+1) n in the SE ordering; unit_spheres (d x l, may be NULL): R0^T s, rotated
 * only, as getStatesInLocalFrame and dcora_round_align_trajectory return them; landmarks (d x b, may be NULL): rotated
 * and shifted.  The point behind cost2 is [T | s / |s| | L]: its sphere columns are NORMALISED, as projectSolutionRASLAM
 * normalises them (ref src/DCORA_utils.cpp:1984-2031) -- the returned unit_spheres are not. */
int dcora_ra_rbcd_round(dcora_ra_rbcd_t s, int anchor_pose, const double *anchor, double *trajectory,
                        double *unit_spheres, double *landmarks, double *cost2, double *info4);
/* dcora_rbcd_project on a range-aided session: X, the projected point and basis^T X in the global RA ordering
 * [rotations | unit spheres | translations | landmarks] */
int dcora_ra_rbcd_project(dcora_ra_rbcd_t s, double *sigma, double *basis, double *gram, double *cost2, double *info8);
/* dcora_rbcd_reserve_rank on a range-aided session: legal until dcora_exchange_create_ra */
int dcora_ra_rbcd_reserve_rank(dcora_ra_rbcd_t s, int r_reserve);
/* as dcora_rbcd_iterate / _evaluate / _run / _last_result; `selected` indexes the agents of dcora_ra_rbcd_info */
int dcora_ra_rbcd_iterate(dcora_ra_rbcd_t s, int selected, double *cost2, double *gradnorm, double *block_norms,
                          int *next_selected);
int dcora_ra_rbcd_evaluate(dcora_ra_rbcd_t s, double *cost2, double *gradnorm, double *block_norms,
                           int *next_selected);
int dcora_ra_rbcd_run(dcora_ra_rbcd_t s, int max_iters, double rgrad_tol, int *iters_done, double *cost2_trace,
                      double *gradnorm_trace, int *selected_trace);
int dcora_ra_rbcd_last_result(dcora_ra_rbcd_t s, dcora_ropt_result *res);
/* as dcora_rbcd_iterate_set / _set_acceleration / _agent_colours / _run_coloured (agents that fire together, ref
 * src/Agent.cpp:650-678; acceleration off as there, :651-653): every agent of the set reads its linear term, its start
 * point and its XPrev from the mirror as it stood when the tick began, each hosted one solves on a HIP stream of its
 * own, and no block returns to the mirror before all are staged.  Agents that share a measurement are refused unless
 * allow_adjacent != 0; a colour of dcora_ra_rbcd_agent_colours ticks to the same result as dcora_ra_rbcd_iterate of
 * its agents one after the other. */
int dcora_ra_rbcd_iterate_set(dcora_ra_rbcd_t s, const int *set, int count, int allow_adjacent);
int dcora_ra_rbcd_set_acceleration(dcora_ra_rbcd_t s, int acceleration);
int dcora_ra_rbcd_agent_colours(dcora_ra_rbcd_t s, int *colours, int *ncolours);
int dcora_ra_rbcd_run_coloured(dcora_ra_rbcd_t s, int max_sweeps, double rgrad_tol, int *sweeps_done,
                               double *cost2_trace, double *gradnorm_trace);

/* ------------------------------------------------------------------------- *
 * Robust estimation (replaces src/DCORA_robust.cpp and the robust parts of src/DCORA_solver.cpp)
 * ------------------------------------------------------------------------- */
/* RobustCostParameters::Type (ref include/DCORA/DCORA_robust.h:28-35) */
typedef enum {
  DCORA_ROBUST_L2 = 0,
  DCORA_ROBUST_L1 = 1,
  DCORA_ROBUST_TLS = 2,
  DCORA_ROBUST_HUBER = 3,
  DCORA_ROBUST_GM = 4,
  DCORA_ROBUST_GNC_TLS = 5
} dcora_robust_type;
/* RobustCostParameters (ref :25-60); defaults: L2, 20 GNC iterations, barc 5, mu step 1.4, mu init 1e-4, Huber 3, TLS 10 */
typedef struct {
  int cost_type;
  int GNCMaxNumIters;
  double GNCBarc, GNCMuStep, GNCInitMu;
  double HuberThreshold, TLSThreshold;
} dcora_robust_params;
void dcora_robust_params_default(dcora_robust_params *p);
/* --- robust sessions: the agents' GNC loop inside one live session (pose-graph sessions; world_size 1 here, any
 *     world_size through dcora_rbcd_create_robust_ranks below) --- */
/* dcora_rbcd_create with Agent::initializeRobustOptimization (ref src/Agent.cpp:1332-1346): weight 1 on every loop
 * closure -- every measurement but odometry (p2 == p1 + 1 inside one agent of the contiguous partition) -- whose
 * fixed_weight flag (m ints, may be NULL) is 0.  The matrices' patterns are those of these weights, the largest any
 * later weights can give.  world_size > 1: DCORA_ERR_UNSUPPORTED (see dcora_rbcd_create_robust_ranks). */
int dcora_rbcd_create_robust(dcora_dataset_t ds, const dcora_rbcd_options *opt, const dcora_robust_params *robust,
                             const int *fixed_weight, dcora_rbcd_t *out);
/* Agent::updateMeasurementWeights (ref src/Agent.cpp:1397-1441): weight = RobustCost::weight(residual) of every
 * non-fixed loop closure on the current iterate (on the device), Q_bb / coupling / central Q / preconditioners rebuilt
 * in place, RobustCost::update(), reset_to_initial != 0: X = the last dcora_rbcd_set_X (robustOptNumResets), then
 * initializeAcceleration (XPrev = V = Y = X, gamma = alpha = 0; the iteration count goes on).  counts (may be NULL):
 * accepted (w > 1 - 1e-8), rejected (w < 1e-8), undecided among the updated closures.  The next three entries and this
 * one return DCORA_ERR_BAD_ARG on a session created without robust state by dcora_rbcd_create (DCORA_ERR_UNSUPPORTED
 * when its world_size > 1). */
int dcora_rbcd_update_weights(dcora_rbcd_t s, int reset_to_initial, int counts[3]);
/* all m weights in dataset order (Agent::setMeasurementWeight of every measurement, ref src/Agent.cpp:1443-1454), then
 * initializeAcceleration.  A weight that is negative or not finite, or a zero weight of creation made nonzero: the call
 * is refused (DCORA_ERR_BAD_ARG) and the session left as it was. */
int dcora_rbcd_set_weights(dcora_rbcd_t s, const double *w);
int dcora_rbcd_get_weights(dcora_rbcd_t s, double *w);
/* RobustCost's current mu (GNC-TLS) and the number of dcora_rbcd_update_weights calls so far (either may be NULL) */
int dcora_rbcd_robust_info(dcora_rbcd_t s, double *mu, int *updates);
/* Robust sessions of a multi-rank job (one process per GPU, the agents spread over the ranks, public poses moved by
 * dcora_exchange_*).  All calls are SPMD: every rank makes the same calls with the same arguments, and each gives on
 * W ranks exactly what the single-process session gives (weights, counts and X bit for bit).
 * dcora_rbcd_create_robust_ranks: the session of rank opt->rank of opt->world_size (world_size 1 included: that session
 * is the one dcora_rbcd_create_robust makes) as dcora_rbcd_create_robust sets it up, together with its exchange
 * (dcora_exchange_create under job_name).  Each rank builds and uploads what its hosted agents need only.  On such a
 * session dcora_rbcd_update_weights and dcora_rbcd_set_weights return DCORA_ERR_UNSUPPORTED (they are not collective);
 * dcora_rbcd_get_weights gives this rank's view: the weights its matrices hold for every measurement touching one of
 * its agents, NaN for all others; dcora_rbcd_robust_info is unchanged.  Destroy the exchange before the session. */
int dcora_rbcd_create_robust_ranks(dcora_dataset_t ds, const dcora_rbcd_options *opt, const dcora_robust_params *robust,
                                   const int *fixed_weight, const char *job_name, dcora_rbcd_t *session,
                                   dcora_exchange_t *ex);
/* The same with room for the ranks to come (dcora_rbcd_reserve_rank between the session and its exchange): r_reserve 0
 * is dcora_rbcd_create_robust_ranks, which calls this with 0; else d <= opt->r <= r_reserve <= 16 (DCORA_ERR_BAD_ARG). */
int dcora_rbcd_create_robust_ranks_reserved(dcora_dataset_t ds, const dcora_rbcd_options *opt,
                                            const dcora_robust_params *robust, const int *fixed_weight, int r_reserve,
                                            const char *job_name, dcora_rbcd_t *session, dcora_exchange_t *ex);
/* dcora_rbcd_update_weights of every agent on every rank, on the iterate that the last dcora_exchange_wait left in each
 * rank's mirror: each rank weights the measurements touching its agents (one launch; a measurement shared by two ranks
 * is weighted on both, to the same bits), the rank hosting p1 publishes the weight in the exchange's shared segment,
 * counts[3] (accepted, rejected, undecided) are summed over the ranks and the same on every rank.  reset_to_initial:
 * every rank's X back to the last dcora_exchange_set_X.  A failure on one rank fails the other ranks' next collective
 * call (within DCORA_EXCHANGE_TIMEOUT_S), never a hang. */
int dcora_exchange_update_weights(dcora_exchange_t ex, int reset_to_initial, int counts[3]);
/* all m weights in dataset order (a range-aided job: m_pp, pose-pose order), the same vector on every rank; checked in
 * full on every rank before anything changes (the refusals of dcora_rbcd_set_weights, DCORA_ERR_BAD_ARG everywhere, the
 * job left as it was) */
int dcora_exchange_set_weights(dcora_exchange_t ex, const double *w);
/* all m current weights of the job, the same on every rank */
int dcora_exchange_get_weights(dcora_exchange_t ex, double *w);
/* --- robust range-aided sessions: the same GNC loop inside a live dcora_ra_rbcd session.  The reference's Agent runs
 *     initializeRobustOptimization / updateMeasurementWeights / setMeasurementWeight (ref src/Agent.cpp:1332-1346,
 *     1397-1441, 1443-1454) on a RangeAidedSLAMGraph as on a pose graph, over the pose-pose loop closures only
 *     (computeMeasurementResidual, :1349-1395, refuses every other type): range and pose-landmark weights never change.
 *     Weights are in pose-pose order (dcora_radataset_copy).  world_size 1 here, any world_size through
 *     dcora_ra_rbcd_create_robust_ranks below. --- */
/* Host only.  mask: one flag per pose-pose measurement, 1 for a loop closure, 0 for odometry -- both poses of one robot
 * (dcora_radataset_ownership) and consecutive in that robot's own numbering.  The RA counterpart of the contiguous
 * partition's rule above. */
int dcora_radataset_loop_closures(dcora_radataset_t ds, int *mask);
/* Host only.  w: m_pp weights, each finite and >= 0 (else DCORA_ERR_BAD_ARG, the dataset left as it was).
 * dcora_radataset_build_Q, dcora_radataset_copy and every session created afterwards see them; a pose-pose measurement
 * of weight 0 contributes no entry to Q. */
int dcora_radataset_set_pose_pose_weights(dcora_radataset_t ds, const double *w);
/* out: m_pp squared errors kappa |Y1 R - Y2|^2 + tau |p2 - p1 - Y1 t|^2 (weights not applied) at X, r x k in the global
 * RA ordering, d <= r <= 16: dcora_measurement_errors with the RA addressing, the same expression bit for bit */
int dcora_ra_measurement_errors(dcora_radataset_t ds, int r, const double *X, double *out, int device);
/* dcora_ra_rbcd_create with Agent::initializeRobustOptimization: weight 1 on every loop closure
 * (dcora_radataset_loop_closures) whose fixed_weight flag (m_pp ints, may be NULL) is 0.  The patterns of every agent's
 * Q_aa, of its coupling block and of the central Q are those of these weights, the largest any later weights can give;
 * neighbours, public columns and colours stay those of creation whatever the weights become (a weight of 0 on the only
 * measurement joining two agents would separate them in a fresh session; the reference, too, keeps a weight-0
 * measurement in its graph).  opt->world_size > 1: DCORA_ERR_UNSUPPORTED (see dcora_ra_rbcd_create_robust_ranks). */
int dcora_ra_rbcd_create_robust(dcora_radataset_t ds, const dcora_rbcd_options *opt, const dcora_robust_params *robust,
                                const int *fixed_weight, dcora_ra_rbcd_t *out);
/* The contracts of dcora_rbcd_update_weights / _set_weights / _get_weights / _robust_info.  The weights come from the
 * mirror (the global iterate); every agent's Q_aa, its regularisation (recomputed as the reference does whenever the
 * data matrices are rebuilt, ref src/Graph.cpp:1906, 1921), its preconditioner, its coupling block and the central Q
 * are rebuilt through the path creation takes; reset_to_initial: X = the last dcora_ra_rbcd_set_X.  On a session of
 * dcora_ra_rbcd_create: DCORA_ERR_BAD_ARG (DCORA_ERR_UNSUPPORTED when its world_size > 1). */
int dcora_ra_rbcd_update_weights(dcora_ra_rbcd_t s, int reset_to_initial, int counts[3]);
int dcora_ra_rbcd_set_weights(dcora_ra_rbcd_t s, const double *w);
int dcora_ra_rbcd_get_weights(dcora_ra_rbcd_t s, double *w);
int dcora_ra_rbcd_robust_info(dcora_ra_rbcd_t s, double *mu, int *updates);
/* Robust sessions of a multi-rank range-aided job: dcora_rbcd_create_robust_ranks' contract on a dcora_ra_rbcd session.
 * The session of rank opt->rank of opt->world_size (world_size 1 included: that session is the one
 * dcora_ra_rbcd_create_robust makes), together with its exchange (dcora_exchange_create_ra under job_name), whose
 * dcora_exchange_update_weights / _set_weights / _get_weights take and give the job's m_pp weights in pose-pose order and
 * give on W ranks exactly what the single-process session gives (weights, counts and X bit for bit).  Each rank weights
 * the pose-pose measurements touching an agent it hosts (dcora_radataset_rank_edges) from its mirror; the rank hosting
 * the owner of p1 publishes the weight.  A rank's matrices hold only the measurements touching its agents: for any other
 * it keeps the last weight it was told (creation, dcora_exchange_set_weights), which reaches none of them.  On such a
 * session dcora_ra_rbcd_update_weights and dcora_ra_rbcd_set_weights return DCORA_ERR_UNSUPPORTED (they are not
 * collective); dcora_ra_rbcd_get_weights gives this rank's view: the weight of every pose-pose measurement touching one
 * of its agents, NaN for all others; dcora_ra_rbcd_robust_info is unchanged.  dcora_exchange_team_enable_ra serves the
 * exchange (below).  Destroy the exchange before the session. */
int dcora_ra_rbcd_create_robust_ranks(dcora_radataset_t ds, const dcora_rbcd_options *opt,
                                      const dcora_robust_params *robust, const int *fixed_weight, const char *job_name,
                                      dcora_ra_rbcd_t *session, dcora_exchange_t *ex);
/* dcora_rbcd_create_robust_ranks_reserved on a range-aided job (r_reserve 0: dcora_ra_rbcd_create_robust_ranks) */
int dcora_ra_rbcd_create_robust_ranks_reserved(dcora_radataset_t ds, const dcora_rbcd_options *opt,
                                               const dcora_robust_params *robust, const int *fixed_weight,
                                               int r_reserve, const char *job_name, dcora_ra_rbcd_t *session,
                                               dcora_exchange_t *ex);
/* Host only.  The rule of dcora_ra_rbcd_create_robust_ranks for rank `rank` of world_size: one flag per pose-pose
 * measurement each.  touches: either pose is owned by an agent the rank hosts (agent i -- position in the sorted list of
 * robots owning poses -- on rank i / ceil(R / world_size)); owns: it hosts the owner of p1.  Every measurement is owned
 * by exactly one rank; a rank beyond the last agent's has none. */
int dcora_radataset_rank_edges(dcora_radataset_t ds, int rank, int world_size, int *touches, int *owns);

/* --- agent status, team termination and weight-update decisions (ref src/Agent.cpp:558-586, 1123-1156, 1280-1330) --- */
/* the fields of AgentParameters the three rules read (ref include/DCORA/Agent.h:113-125); defaults: 500 iterations,
 * relative change 5e-3, 10 weight updates, 0 resets, 30 inner iterations, convergence ratio 0.8 */
typedef struct {
  int max_num_iters;
  double rel_change_tol;
  int robust_opt_num_weight_updates, robust_opt_num_resets, robust_opt_inner_iters;
  double robust_opt_min_convergence_ratio;
} dcora_team_params;
void dcora_team_params_default(dcora_team_params *p);
/* AgentState (ref include/DCORA/Agent.h:149-155) */
typedef enum {
  DCORA_AGENT_WAIT_FOR_DATA = 0,
  DCORA_AGENT_WAIT_FOR_INITIALIZATION = 1,
  DCORA_AGENT_INITIALIZED = 2
} dcora_agent_state;
/* AgentStatus (ref include/DCORA/Agent.h:157-200) */
typedef struct {
  int agent_id, state, instance_number, iteration_number, ready_to_terminate;
  double relative_change;
} dcora_agent_status;
/* The local rule of Agent::iterate (ref src/Agent.cpp:567-585), host only.  robust: cost type != L2.  *ready = 0 when
 * success == 0, when relative_change > tolerance (rel_change_tol; 5 while robust and weight_update_count == 0), or when
 * (accepted + rejected) / total < robust_opt_min_convergence_ratio in doubles, as written there: an agent without loop
 * closures (0 / 0) passes. */
int dcora_team_ready_to_terminate(const dcora_team_params *params, int robust, int weight_update_count, int success,
                                  double relative_change, int accepted, int rejected, int total, int *ready);
/* Agent::shouldTerminate and Agent::shouldUpdateMeasurementWeights (ref src/Agent.cpp:1123-1156, 1280-1330) in the
 * reference's order of tests, host only.  statuses / have: num_robots entries, have[q] == 0: the status of robot q is
 * absent; active (may be NULL: all active): robots with active[q] == 0 are skipped.  Either output may be NULL. */
int dcora_team_decide(const dcora_team_params *params, int robust, int iteration_number, int weight_update_count,
                      int inner_iter, int latest_weight_update_iteration, const dcora_agent_status *statuses,
                      const int *have, const int *active, int num_robots, int *should_terminate,
                      int *should_update_weights);
/* LiftedArray::maxTranslationDistance (ref src/manifold/Elements.cpp:59-69) of two lifted pose arrays r x (d+1) n
 * (column-major, host) on the device, by the kernel that computes the agents' relative change: max over the poses of
 * the 2-norm of the translations' difference.  2 <= r <= 16, d in {2, 3}, d <= r, n >= 1. */
int dcora_max_translation_distance(int r, int d, int n, const double *X, const double *Y, double *out);
/* Opt-in to the team protocol on a pose-graph session of one process (world_size > 1: DCORA_ERR_UNSUPPORTED).  From
 * here on every Agent::iterate(true) of an agent -- dcora_rbcd_iterate, dcora_rbcd_phase_selected,
 * dcora_rbcd_agent_iterate(.., 1), dcora_rbcd_iterate_set and the run loops over them -- stores that agent's status
 * (ref src/Agent.cpp:558-586): one more launch per round, no synchronisation.  The round counter of the robust inner
 * iterations advances with every round (:537-538).  dcora_rbcd_update_weights clears the statuses, records the round as
 * the latest weight update and zeroes that counter (:1417-1424); dcora_rbcd_set_weights only refreshes the loop-closure
 * counts; dcora_rbcd_set_X, which restarts the rounds, restarts this bookkeeping with them.  A session that never
 * calls this launches nothing new.  The entries below return DCORA_ERR_BAD_ARG before it. */
int dcora_rbcd_team_enable(dcora_rbcd_t s, const dcora_team_params *params);
/* the status `agent` stored at its last optimisation since the statuses were cleared (*known = 0: none, *status then
 * holds the agent's id, state and iteration number only) */
int dcora_rbcd_agent_status(dcora_rbcd_t s, int agent, dcora_agent_status *status, int *known);
/* Graph::statistics (ref src/Graph.cpp:475-521) of `agent`: accepted (weight == 1), rejected (weight == 0) and all
 * loop closures -- every measurement but odometry -- with an end at the agent */
int dcora_rbcd_loop_closure_stats(dcora_rbcd_t s, int agent, int counts[3]);
/* dcora_team_decide over the statuses the session holds (an agent that has not optimised since the last clear is
 * absent), the session's round counter as the iteration number */
int dcora_rbcd_should_terminate(dcora_rbcd_t s, int *yes);
int dcora_rbcd_should_update_weights(dcora_rbcd_t s, int *yes);
/* info[4]: robust inner iterations since the latest weight update (0 with the L2 cost), the round of the latest weight
 * update, weight updates so far, trajectory resets dcora_rbcd_run_team has made */
int dcora_rbcd_team_info(dcora_rbcd_t s, int info[4]);
typedef enum { DCORA_TEAM_STOP_ALL_READY = 1, DCORA_TEAM_STOP_MAX_ITERS = 2 } dcora_team_stop_reason;
/* The loop a team without a central evaluator runs, made of exactly these calls: until dcora_rbcd_should_terminate,
 * each pass { if dcora_rbcd_should_update_weights: dcora_rbcd_update_weights(reset = resets made so far <
 * robust_opt_num_resets), updated_trace[it] = 1; dcora_rbcd_iterate(selected) with the greedy next selection, first
 * agent 0 }.  The traces (any may be NULL) hold max_num_iters entries, entry it belonging to pass it. */
int dcora_rbcd_run_team(dcora_rbcd_t s, int *iters_done, double *cost2_trace, double *gradnorm_trace,
                        int *selected_trace, int *updated_trace, int *weight_updates, int *stop_reason);
/* ---- the team protocol on a range-aided session of one process ----
 * The reference's agents run the same three rules on a RangeAidedSLAMGraph as on a pose graph: the status block of
 * Agent::iterate (ref src/Agent.cpp:558-586), shouldTerminate (:1123-1156), shouldUpdateMeasurementWeights (:1280-1330)
 * and the bookkeeping of updateMeasurementWeights (:1417-1424).  The contracts are the dcora_rbcd_* namesakes'.
 * dcora_ra_max_translation_distance: LiftedArray::maxTranslationDistance(*X.GetLiftedPoseArray(), ...) (ref
 * src/Agent.cpp:564-565, src/manifold/Elements.cpp:59-69) of two arrays r x k, k = (d+1) n + l + b, in the RA ordering
 * [rotations | l unit spheres | translations | b landmarks] (column-major, host) by the kernel that computes a
 * range-aided agent's relative change: over the POSES only (translation i is column d n + l + i), unit spheres and
 * landmarks never count.  2 <= r <= 16, d in {2, 3}, d <= r, n >= 1, l >= 0, b >= 0. */
int dcora_ra_max_translation_distance(int r, int d, int n, int l, int b, const double *X, const double *Y,
                                      double *out);
/* Graph::statistics (ref src/Graph.cpp:475-521) of `robot` on the dataset's current weights, host only (no device):
 * accepted (weight == 1), rejected (weight == 0) and all loop closures with an end at the robot.  By
 * Graph::addMeasurement (ref :121-134) a loop closure is every measurement but pose-pose odometry
 * (dcora_radataset_loop_closures' rule): pose-pose loop closures, pose-landmark measurements and ranges, each counted
 * at the owner of either end (a range's ends by their types), once when both are the robot's.  These are the counts a
 * session of this dataset starts with for that robot. */
int dcora_radataset_loop_closure_stats(dcora_radataset_t ds, int robot, int counts[3]);
/* Opt-in (ref src/Agent.cpp:558-586, 1417-1424) on a session of dcora_ra_rbcd_create (an L2 team) or
 * dcora_ra_rbcd_create_robust; world_size > 1: DCORA_ERR_UNSUPPORTED.  From here on every Agent::iterate(true) of an
 * agent -- dcora_ra_rbcd_iterate, _run, _iterate_set, _run_coloured, _run_team -- stores that agent's status (state
 * INITIALIZED, instance 0, the session's round, the relative change over the agent's poses): one more launch per
 * round or tick, no synchronisation.  dcora_ra_rbcd_update_weights clears the statuses, records the round as the
 * latest weight update and zeroes the inner counter; dcora_ra_rbcd_set_weights only refreshes the loop-closure counts
 * (range and pose-landmark weights are the file's, pose-pose weights the session's current ones);
 * dcora_ra_rbcd_set_X and _set_acceleration restart this bookkeeping with the rounds.  A session that never calls
 * this launches nothing new.  The six entries below return DCORA_ERR_BAD_ARG before it. */
int dcora_ra_rbcd_team_enable(dcora_ra_rbcd_t s, const dcora_team_params *params);
/* Agent::getStatus (ref include/DCORA/Agent.h:427-433); `agent`: position in the sorted robot list */
int dcora_ra_rbcd_agent_status(dcora_ra_rbcd_t s, int agent, dcora_agent_status *status, int *known);
/* Graph::statistics (ref src/Graph.cpp:475-521) of the agent, on the session's current weights */
int dcora_ra_rbcd_loop_closure_stats(dcora_ra_rbcd_t s, int agent, int counts[3]);
/* Agent::shouldTerminate (ref src/Agent.cpp:1123-1156), Agent::shouldUpdateMeasurementWeights (ref :1280-1330) */
int dcora_ra_rbcd_should_terminate(dcora_ra_rbcd_t s, int *yes);
int dcora_ra_rbcd_should_update_weights(dcora_ra_rbcd_t s, int *yes);
/* info[4] as dcora_rbcd_team_info (ref include/DCORA/Agent.h:720-735) */
int dcora_ra_rbcd_team_info(dcora_ra_rbcd_t s, int info[4]);
/* dcora_rbcd_run_team's loop (ref src/Agent.cpp:650-678) of dcora_ra_rbcd_update_weights and dcora_ra_rbcd_iterate:
 * traces of max_num_iters entries, greedy selection starting with agent 0, reset = resets made <
 * robust_opt_num_resets */
int dcora_ra_rbcd_run_team(dcora_ra_rbcd_t s, int *iters_done, double *cost2_trace, double *gradnorm_trace,
                           int *selected_trace, int *updated_trace, int *weight_updates, int *stop_reason);
/* ---- the team protocol across the ranks of a job ----
 * The entries above on a multi-rank job of either kind, through its exchange: semantics are their dcora_rbcd_* /
 * dcora_ra_rbcd_* namesakes', every rank holds every agent's status, and the outputs are identical on every rank.  Of an optimisation only its
 * success and its relative change are known to the hosting rank alone: they travel through a status slot of the job's
 * segment (the relative change stored by the kernel that computes it), every rank settles the status by
 * dcora_team_ready_to_terminate.
 * dcora_exchange_team_enable (SPMD): on the exchange of any pose-graph session -- dcora_exchange_create (an L2 team, its
 * loop-closure counts from the creation weights) or dcora_rbcd_create_robust_ranks, world_size 1 included;
 * DCORA_ERR_UNSUPPORTED on a range-aided exchange, as before.
 * dcora_exchange_team_enable_ra (SPMD): the same on the exchange of any range-aided session -- dcora_exchange_create_ra
 * (an L2 team) or dcora_ra_rbcd_create_robust_ranks, world_size 1 included; DCORA_ERR_UNSUPPORTED on a pose-graph
 * exchange.  There `agent` is the position in the sorted robot list, the loop closures of an agent are every measurement
 * but pose-pose odometry (pose-pose closures, pose-landmark measurements, ranges) as for dcora_ra_rbcd_team_*, only the
 * pose-pose ones are re-weighted, and the counts of all agents come from the job's weights (a rank's own session knows
 * only its agents').  The six entries below serve both kinds.
 * Either entry returns DCORA_ERR_UNSUPPORTED, on every rank alike and with the exchange usable afterwards, when the
 * session's own dcora_rbcd_team_enable / dcora_ra_rbcd_team_enable came first or when a robust ranked session is given an
 * exchange it was not created with.  Before it the other six return DCORA_ERR_BAD_ARG
 * (the job goes on).  Once enabled, the session's agents optimise through dcora_exchange_rbcd_iterate / _rbcd_tick /
 * _run_coloured / _run_team only.
 * _agent_status, _loop_closure_stats, _should_terminate, _should_update_weights are LOCAL queries: once a collective
 * call (dcora_exchange_rbcd_iterate, _rbcd_tick, _run_coloured, _update_weights, _set_weights, _set_X) has returned,
 * they answer from this rank's copy without talking to anyone.  _team_info and _run_team are SPMD.
 * dcora_exchange_run_team: dcora_rbcd_run_team's loop of dcora_exchange_update_weights and dcora_exchange_rbcd_iterate. */
int dcora_exchange_team_enable(dcora_exchange_t ex, const dcora_team_params *params);
int dcora_exchange_team_enable_ra(dcora_exchange_t ex, const dcora_team_params *params);
int dcora_exchange_agent_status(dcora_exchange_t ex, int agent, dcora_agent_status *status, int *known);
int dcora_exchange_loop_closure_stats(dcora_exchange_t ex, int agent, int counts[3]);
int dcora_exchange_should_terminate(dcora_exchange_t ex, int *yes);
int dcora_exchange_should_update_weights(dcora_exchange_t ex, int *yes);
int dcora_exchange_team_info(dcora_exchange_t ex, int info[4]);
int dcora_exchange_run_team(dcora_exchange_t ex, int *iters_done, double *cost2_trace, double *gradnorm_trace,
                            int *selected_trace, int *updated_trace, int *weight_updates, int *stop_reason);
/* RobustCost::weight(r) for n residuals after num_updates calls of RobustCost::update() (ref src/DCORA_robust.cpp:56-136) */
int dcora_robust_weights(const dcora_robust_params *p, int num_updates, int n, const double *r, double *w);
/* chi2inv (ref src/DCORA_utils.cpp:2103-2106), RobustCost::computeErrorThresholdAtQuantile (ref src/DCORA_robust.cpp:138-148) */
int dcora_chi2inv(double quantile, int dof, double *out);
int dcora_robust_error_threshold_at_quantile(double quantile, int dimension, double *out);
/* robustSingleRotationAveraging / robustSinglePoseAveraging (ref src/DCORA_solver.cpp:76-216): R holds n rotations
 * d x d column-major back to back, t n translations; kappa / tau may be NULL (1 resp. 10000 / 100 as in the
 * reference); inlier receives n flags */
int dcora_robust_single_rotation_averaging(int d, int n, const double *R, const double *kappa, double error_threshold,
                                           double *Ropt, int *inlier);
int dcora_robust_single_pose_averaging(int d, int n, const double *R, const double *t, const double *kappa,
                                       const double *tau, double error_threshold, double *Ropt, double *topt,
                                       int *inlier);
/* computeMeasurementError of every measurement of the dataset at once (ref src/DCORA_utils.cpp:2095-2101;
 * Agent::computeMeasurementResidual, ref src/Agent.cpp:1342-1389): X is r x (d+1) n (SE ordering, r >= d, lifted or
 * not); out[i] = kappa |Y1 R - Y2|^2 + tau |p2 - p1 - Y1 t|^2, weights not applied */
/* ---- cross-robot frame alignment (ref src/Agent.cpp:460-520, 694-833); poses d x (d+1) column-major [R t] ---- */
/* Agent::computeNeighborTransform for m inter-robot loop closures: incoming[i] != 0 when this robot is the
 * measurement's second pose; nbr_pose[i] the neighbour's pose of the closure in the neighbour's (world2) frame,
 * my_pose[i] my pose of it in my (world1) frame; T_out[i] = T_world2_world1 implied by closure i */
int dcora_agent_neighbor_transforms(int d, int m, const int *incoming, const double *meas_R, const double *meas_t,
                                    const double *nbr_pose, const double *my_pose, double *T_out);
/* Agent::computeRobustNeighborTransform (two_stage = 0) / computeRobustNeighborTransformTwoStage (two_stage != 0)
 * over m candidate transforms; *ok = 0 when fewer than min_inliers (AgentParameters::robustInitMinInliers) agree */
int dcora_agent_robust_neighbor_transform(int d, int m, const double *candidates, int two_stage, int min_inliers,
                                          double *T_world_robot, int *num_inliers, int *ok);
/* Logger::logTrajectory (ref src/Logger.cpp:107-145): "# pose_index x y z qx qy qz qw", one line per pose, 9 decimals;
 * T is d x (d+1) n (SE ordering); planar poses are embedded in 3D (z = 0, rotation about z) */
int dcora_log_trajectory(const char *path, int d, int n, const double *T);
/* fixedStiefelVariable (ref src/DCORA_utils.cpp:2053-2056): the lifting matrix YLift (r x d, orthonormal columns) the
 * agents share; identical on every call and in every process */
int dcora_fixed_stiefel_variable(int r, int d, double *Y);
/* Agent::initializeInGlobalFrame: X (r x k) = YLift (r x d) * T_world_robot applied to the local estimate (d x k,
 * SE ordering when dims.l = dims.b = 0, RA ordering otherwise) */
int dcora_agent_initialize_in_global_frame(const dcora_dims *dims, const double *T_world_robot,
                                           const double *T_local, const double *YLift, double *X);
int dcora_measurement_errors(dcora_dataset_t ds, int r, const double *X, double *out, int device);
/* solvePGO (ref src/DCORA_solver.cpp:304-328): T0 (d x (d+1) n) or NULL for the chordal start; one optimize() at
 * rank d with params */
int dcora_solve_pgo(dcora_dataset_t ds, const dcora_ropt_params *params, const double *T0, double *Tout,
                    dcora_ropt_result *result, int device);
/* solveRobustPGO (ref :330-409): GNC-TLS around solvePGO; fixed_weight: one flag per measurement (NULL = none
 * fixed); the final weights are written into the dataset handle and to weights_out (may be NULL) */
int dcora_solve_robust_pgo(dcora_dataset_t ds, const dcora_ropt_params *params, const dcora_robust_params *robust,
                           const int *fixed_weight, const double *T0, double *Tout, double *weights_out, int device);

/* ------------------------------------------------------------------------- *
 * Rounding / solution recovery
 * ------------------------------------------------------------------------- */
/* alignLiftedTrajectoryToFrame (ref src/DCORA_utils.cpp:2262-2289), Agent::getTrajectoryInGlobalFrame /
 * getStatesInLocalFrame (ref src/Agent.cpp:950-1034).  X is r x k in the layout of dims (SE ordering when
 * l = b = 0, RA ordering otherwise); anchor is the lifted pose [Y0 p0], r x (d+1), or NULL for pose 0 of X.
 * global_alignment != 0: the anchor's translation is the origin; 0: pose 0 of X is the origin.
 * trajectory: d x (d+1) n in the SE ordering, every rotation block projected to SO(d);
 * unit_spheres (d x l, rotated) and landmarks (d x b, rotated and translated) may be NULL. */
int dcora_round_align_trajectory(const dcora_dims *dims, const double *X, const double *anchor, int global_alignment,
                                 double *trajectory, double *unit_spheres, double *landmarks, int device);
/* projectSolutionRASLAM (ref src/DCORA_utils.cpp:1984-2031): rank-d truncation of X (r x k), reflection test,
 * SO(d) / unit-sphere projection; out is d x k in the same column layout.  Defined up to the sign convention of
 * the SVD, i.e. up to a global orthogonal transformation that the caller's refinement / alignment removes. */
int dcora_round_project_solution_raslam(const dcora_dims *dims, const double *X, double *out, int device);

/* ------------------------------------------------------------------------- *
 * Bench / profiling hooks
 * ------------------------------------------------------------------------- */
/* times `reps` launches of the Q-apply kernel Y = X Q + G of a problem with HIP events on the handle's
 * stream; returns average milliseconds per launch and the algorithmic bytes of one launch */
int dcora_problem_time_qapply(dcora_problem_t p, int reps, double *avg_ms, double *algorithmic_bytes);
/* the same kernel over `count` problems in turn on one stream: distinct (Q, X, Y) sets, so that with more than 256 MiB
 * between two uses of a set every launch streams from HBM instead of the Infinity Cache */
int dcora_problem_time_qapply_rotating(const dcora_problem_t *problems, int count, int reps, double *avg_ms);
/* which Q-apply kernel the problem runs: info[0] = 0 k_spmm (CSR), 1 k_spmm_bsr (block-CSR, pose graphs with
 * n >= 8192); info[1] = nnz(Q); info[2] = matrix blocks (block-CSR); info[3] = bytes of the stored matrix form */
int dcora_problem_qapply_info(dcora_problem_t p, double *info4);
/* same for the preconditioner application kernel z = Proj_X(r (Q + reg I)^-1) (dense-inverse streaming part) */
int dcora_problem_time_precond(dcora_problem_t p, int reps, double *avg_ms, double *algorithmic_bytes);
/* how the preconditioner (Q + reg I)^-1 of ref src/Graph.cpp:1901-1917 is held on the device:
 * info[0] = 0 none, 1 dense inverse, 2 partitioned sparse inverse (sparse_precond.h);
 * info[1] = kernel launches per application; info[2] = nnz of the Cholesky factor; info[3] = host setup ms;
 * info[4] = doubles of stored inverse one application streams */
int dcora_problem_precond_info(dcora_problem_t p, double *info5);
/* The preconditioner image (dense inverse or partitioned sparse inverse of Q + reg I) is cached inside the library,
 * keyed on the content of the matrix (rowptr, colidx, vals, reg, device): the reference re-creates its QuadraticProblem
 * on every Agent::updateX (ref src/Agent.cpp:1252) while its Graph keeps Q and the factor (ref src/Graph.cpp:523-533,
 * 1901-1917).  A second dcora_problem_create / dcora_rbcd_create on the same matrix -- the next staircase level, a
 * problem re-created per update -- attaches to the resident image instead of factorising again.
 * info[4] = {hits, misses, entries, device bytes held}.  Budget: DCORA_PRECOND_CACHE_MB (default 8192, 0 = off). */
/* addition of this library: the analysis of a certificate's PSD test ahead of time.  The dual certificate S = Q - Lambda
 * has the sparsity pattern of Q, known before the agents start: a driver calls this on another host thread while they
 * iterate; the symbolic analysis (ordering, fronts), its device image and the arena are left in the library's cache and
 * dcora_cert_fast_verification / dcora_cert_is_psd_device of a matrix with this pattern begin with the numeric phase.
 * dims as for dcora_cert_dual_matrix (r is not used); rp / ci: the CSR pattern of Q, both triangles; block as in the PSD
 * test.  The pattern analysed is the one dcora_cert_dual_matrix produces: Q's, the blocks of Lambda, every diagonal. */
int dcora_cert_prepare(const dcora_dims *dims, const int *rp, const int *ci, int block, int device);
int dcora_precond_cache_info(double *info4);
int dcora_precond_cache_clear(void);

#ifdef __cplusplus
}
#endif
#endif /* DCORA_HIP_H_ */
