// Projection of a live session to rank d on the device (see session_project.h): the kernels and SessionCore::project,
// the flow both session kinds share.
#include "session_project.h"

#include <chrono>
#include <cmath>
#include <cstring>

#include "exchange_slots.h"
#include "round_quad.h"
#include "session_core.h"
#include "small_eig.h"

namespace dcora {

namespace {

typedef double gram_v4f64 __attribute__((ext_vector_type(4)));

constexpr int kGramWaves = kBlock / 64;
constexpr int kGramWaveCols = kGramCols / kGramWaves;  // a wave's contiguous run of columns
constexpr int kGramSteps = kGramWaveCols / 4;          // v_mfma_f64_16x16x4_f64 sums four columns a step
constexpr int kGramUnroll = 8;                         // loads in flight per lane before the first product needs one
static_assert(kGramCols % (4 * kGramWaves) == 0 && kGramSteps % kGramUnroll == 0, "whole steps, whole unrolled groups");

// One pass over X: workgroup w owns columns [w kGramCols, (w + 1) kGramCols), wave v of it the run of kGramWaveCols
// from w kGramCols + v kGramWaveCols.  A step takes four columns c0 .. c0 + 3: lane l loads X(l & 15, c0 + (l >> 4)) --
// zero for a row >= r or a column >= k, which is never read -- and that ONE value is both operands of
// v_mfma_f64_16x16x4_f64 (A(i, j) = X(i, c0 + j), B(j, i) = X(i, c0 + j): device_chol.hip's mma16 map), which adds the
// step's X X^T to the wave's 16 x 16 accumulator: lane l holds D((l >> 4) + 4 v, l & 15) in register v.  The waves'
// accumulators meet in LDS and are added in wave order; partials[256 w + i + 16 j] is the workgroup's share of G(i, j).
// Loads of a group of kGramUnroll steps are issued before its first product.
template <class Ptr, class Sm>
__device__ __forceinline__ void gram_chunk(int r, long k, Ptr X, long chunk, Sm &sm,
                                           double *__restrict__ out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lo = lane & 15, hi = lane >> 4;
  const long c_begin = chunk * kGramCols + (long)wave * kGramWaveCols;
  const bool row = lo < r;
  gram_v4f64 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int s = 0; s < kGramSteps; s += kGramUnroll) {
    if (c_begin + 4L * s >= k) break;  // (uniform in the wave: the rest of its run lies past the last column)
    double x[kGramUnroll];
#pragma unroll
    for (int u = 0; u < kGramUnroll; ++u) {
      const long c = c_begin + 4L * (s + u) + hi;
      x[u] = (row && c < k) ? X[c * r + lo] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kGramUnroll; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x[u], x[u], acc, 0, 0, 0);
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) sm[wave][(hi + 4 * v) + 16 * lo] = acc[v];
  __syncthreads();
  double t = sm[0][threadIdx.x];
#pragma unroll
  for (int w = 1; w < kGramWaves; ++w) t += sm[w][threadIdx.x];
  out[threadIdx.x] = t;
}

// G(a, b) = the partials of (min(a, b), max(a, b)) added in chunk order by ONE thread, so G(a, b) and G(b, a) are the
// same sum and G is symmetric bit for bit
__device__ __forceinline__ void gram_finish_sum(int r, long nwg, const double *__restrict__ partials,
                                                double *__restrict__ G) {
  const int a = threadIdx.x & 15, b = threadIdx.x >> 4;
  if (a >= r || b >= r) return;
  const int e = (a < b ? a : b) + 16 * (a < b ? b : a);
  double t = 0.0;
  for (long w = 0; w < nwg; ++w) t += partials[w * 256 + e];
  G[a + r * b] = t;
}

__global__ __launch_bounds__(kBlock) void k_gram_mfma(int r, long k, const double *__restrict__ X,
                                                      double *__restrict__ partials) {
  __shared__ double sm[kGramWaves][256];
  gram_chunk(r, k, X, (long)blockIdx.x, sm, partials + (long)blockIdx.x * 256);
}

// one workgroup, one thread per entry
__global__ __launch_bounds__(256) void k_gram_finish(int r, long nwg, const double *__restrict__ partials,
                                                     double *__restrict__ G) {
  gram_finish_sum(r, nwg, partials, G);
}

// The block-list form: table[b] = {X, k, first workgroup} of block b, table[nblocks].wg0 the number of workgroups.
// Workgroup w belongs to the block b with table[b].wg0 <= w < table[b + 1].wg0 (a block of no columns owns none) and
// takes that block's chunk w - table[b].wg0: kGramCols columns counted from the BLOCK's first column, through
// gram_chunk, so partials[256 w ...] holds what k_gram_mfma of the block alone writes for that chunk, bit for bit.
__global__ __launch_bounds__(kBlock) void k_gram_blocks_mfma(int r, int nblocks, const GramBlock *__restrict__ table,
                                                             double *__restrict__ partials) {
  __shared__ double sm[kGramWaves][256];
  const long w = blockIdx.x;
  int lo = 0, hi = nblocks;  // (uniform: the search runs on the scalar unit)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (table[mid].wg0 <= w)
      lo = mid;
    else
      hi = mid;
  }
  const GramBlock blk = table[lo];
  // (a pointer read from memory: said to be global, so that the loads are global loads as in k_gram_mfma, not flat ones)
  typedef const __attribute__((address_space(1))) double *GlobalPtr;
  gram_chunk(r, blk.k, (GlobalPtr)blk.X, w - blk.wg0, sm, partials + w * 256);
}

// one workgroup PER BLOCK: its partials in chunk order by k_gram_finish's rule; the blocks' sums run side by side
__global__ __launch_bounds__(256) void k_gram_blocks_finish(int r, const GramBlock *__restrict__ table,
                                                            const double *__restrict__ partials,
                                                            double *__restrict__ grams) {
  const long w0 = table[blockIdx.x].wg0, w1 = table[blockIdx.x + 1].wg0;
  gram_finish_sum(r, w1 - w0, partials + w0 * 256, grams + (size_t)blockIdx.x * r * r);
}

// the frame into LDS: sm[a r + q] = V_d(q, a).  Every workgroup reads the same r D words.
template <int D>
__device__ __forceinline__ void load_basis(int r, const double *__restrict__ basis, double *sm) {
  if ((int)threadIdx.x < r * D) sm[threadIdx.x] = basis[threadIdx.x];
  __syncthreads();
}

template <int D>
__device__ __forceinline__ double det_of(const double *P) {
  if (D == 2) return P[0] * P[3] - P[2] * P[1];
  return P[0] * (P[4] * P[8] - P[7] * P[5]) - P[3] * (P[1] * P[8] - P[7] * P[2]) + P[6] * (P[1] * P[5] - P[4] * P[2]);
}

// the poses of a block whose truncated rotation V_d^T Y_i has a positive determinant, k_round_states' lane map: lane c
// of a quad forms column c (one fma chain per element, in index order), the quad hands the columns round, its lane 0
// votes; one ballot and ONE integer atomicAdd per wave (integers are exact: the count does not depend on the order)
template <int D, class Cols>
__global__ __launch_bounds__(kBlock) void k_project_dets(int r, int n, Cols cols, const double *__restrict__ X,
                                                         const double *__restrict__ basis, int *__restrict__ count) {
  __shared__ double sm[16 * D];
  load_basis<D>(r, basis, sm);
  const long g = (long)blockIdx.x * kBlock + threadIdx.x;
  const int c = threadIdx.x & (kQuad - 1);
  const long il = g / kQuad;
  const bool valid = il < n && c < D;
  const int i = valid ? (int)il : 0;
  double m[D], A[D * D];
  frame_dot<D>(r, sm, X + cols.col(i, valid ? c : 0) * r, valid, m);
  quad_gather<D>(m, A);
  const int pos = (valid && c == 0 && det_of<D>(A) > 0) ? 1 : 0;
  const unsigned long long b = __ballot(pos);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, __popcll(b));
}

// [ Proj_SO(D)(V_d^T Y_i) | V_d^T p_i ] for the n poses of a block: k_round_states with V_d (the reflection folded in)
// in the anchor's place, no shift, and the D-row columns of the new mirror -- the block's own ordering -- as output
template <int D, class Cols>
__global__ __launch_bounds__(kBlock) void k_project_states(int r, int n, Cols cols, const double *__restrict__ X,
                                                           const double *__restrict__ basis, double *__restrict__ out) {
  __shared__ double sm[16 * D];
  load_basis<D>(r, basis, sm);
  const long g = (long)blockIdx.x * kBlock + threadIdx.x;
  const int c = threadIdx.x & (kQuad - 1);
  const long il = g / kQuad;
  const bool valid = il < n && c <= D;  // (a quad is valid or not as a whole but for its idle lane at D = 2)
  const int i = valid ? (int)il : 0;
  const long column = cols.col(i, valid ? c : 0);
  double m[D], v[D];
  frame_dot<D>(r, sm, X + column * r, valid, m);
  quad_so_project<D>(m, c, v);
  if (!valid) return;
  double *__restrict__ o = out + column * D;
#pragma unroll
  for (int a = 0; a < D; ++a) o[a] = v[a];
}

// `count` point columns (X, out: their first column): out(:, j) = V_d^T x_j, normalised where asked (unit spheres; a
// zero column stays zero).  One lane per point, as k_round_points.
template <int D>
__global__ __launch_bounds__(kBlock) void k_project_points(int r, int count, const double *__restrict__ X,
                                                           const double *__restrict__ basis, int normalise,
                                                           double *__restrict__ out) {
  __shared__ double sm[16 * D];
  load_basis<D>(r, basis, sm);
  const long j = (long)blockIdx.x * kBlock + threadIdx.x;
  if (j >= count) return;
  double m[D];
  frame_dot<D>(r, sm, X + j * r, true, m);
  if (normalise) unit_or_zero<D>(m);
#pragma unroll
  for (int a = 0; a < D; ++a) out[j * D + a] = m[a];
}

template <int D>
void launch_project_dets_d(hipStream_t st, int r, const RoundBlock &blk, const double *basis, int *count) {
  if (blk.n <= 0) return;
  const unsigned grid = (unsigned)(((long)blk.n * kQuad + kBlock - 1) / kBlock);
  if (blk.se)
    hipLaunchKernelGGL((k_project_dets<D, SeCols<D>>), dim3(grid), dim3(kBlock), 0, st, r, blk.n, SeCols<D>{}, blk.X,
                       basis, count);
  else
    hipLaunchKernelGGL((k_project_dets<D, RaCols<D>>), dim3(grid), dim3(kBlock), 0, st, r, blk.n,
                       (RaCols<D>{blk.n, blk.l}), blk.X, basis, count);
}

template <int D>
void launch_project_block_d(hipStream_t st, int r, const RoundBlock &blk, const double *basis, double *out) {
  const unsigned grid = (unsigned)(((long)blk.n * kQuad + kBlock - 1) / kBlock);
  if (blk.n > 0) {
    if (blk.se)
      hipLaunchKernelGGL((k_project_states<D, SeCols<D>>), dim3(grid), dim3(kBlock), 0, st, r, blk.n, SeCols<D>{},
                         blk.X, basis, out);
    else
      hipLaunchKernelGGL((k_project_states<D, RaCols<D>>), dim3(grid), dim3(kBlock), 0, st, r, blk.n,
                         (RaCols<D>{blk.n, blk.l}), blk.X, basis, out);
  }
  if (blk.se) return;
  const long s0 = (long)D * blk.n, l0 = s0 + blk.l + blk.n;  // first sphere / landmark column
  if (blk.l > 0)
    hipLaunchKernelGGL(k_project_points<D>, dim3((unsigned)((blk.l + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, r,
                       blk.l, blk.X + s0 * r, basis, 1, out + s0 * D);
  if (blk.b > 0)
    hipLaunchKernelGGL(k_project_points<D>, dim3((unsigned)((blk.b + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, r,
                       blk.b, blk.X + l0 * r, basis, 0, out + l0 * D);
}

}  // namespace

void launch_gram(hipStream_t st, int r, long k, const double *X, double *partials, double *G) {
  const long nwg = gram_workgroups(k);
  hipLaunchKernelGGL(k_gram_mfma, dim3((unsigned)nwg), dim3(kBlock), 0, st, r, k, X, partials);
  hipLaunchKernelGGL(k_gram_finish, dim3(1), dim3(256), 0, st, r, nwg, partials, G);
}

void launch_gram_blocks(hipStream_t st, int r, int nblocks, long nwg, const GramBlock *table, double *partials,
                        double *grams) {
  if (nblocks <= 0) return;
  if (nwg > 0)
    hipLaunchKernelGGL(k_gram_blocks_mfma, dim3((unsigned)nwg), dim3(kBlock), 0, st, r, nblocks, table, partials);
  hipLaunchKernelGGL(k_gram_blocks_finish, dim3((unsigned)nblocks), dim3(256), 0, st, r, table, partials, grams);
}

void launch_project_dets(hipStream_t st, int r, int d, const RoundBlock &blk, const double *basis, int *count) {
  if (d == 3)
    launch_project_dets_d<3>(st, r, blk, basis, count);
  else
    launch_project_dets_d<2>(st, r, blk, basis, count);
}

void launch_project_block(hipStream_t st, int r, int d, const RoundBlock &blk, const double *basis, double *out) {
  if (d == 3)
    launch_project_block_d<3>(st, r, blk, basis, out);
  else
    launch_project_block_d<2>(st, r, blk, basis, out);
}

int SessionCore::project_buffers(const ManiDesc &m) {
  SessionProjectState &ps = project_;
  const size_t np = 256 * (size_t)gram_workgroups(m.k), nx = (size_t)m.d * (size_t)m.k;
  if (ps.partials_cap < np) {
    DCORA_HIP(ps.partials.alloc(np));
    ps.partials_cap = np;
  }
  if (ps.point_cap < nx) {
    DCORA_HIP(ps.point.alloc(nx));
    ps.point_cap = nx;
  }
  if (!ps.gram.p) DCORA_HIP(ps.gram.alloc((size_t)kMaxRank * kMaxRank));
  if (!ps.basis.p) DCORA_HIP(ps.basis.alloc((size_t)kMaxRank * 3));
  if (!ps.count.p) DCORA_HIP(ps.count.alloc(1));
  for (hipEvent_t *e : {&ps.ev0, &ps.ev1, &ps.ev2, &ps.ev3})
    if (!*e) DCORA_HIP(hipEventCreate(e));
  return DCORA_OK;
}

int SessionCore::project(double *sigma, double *basis, double *gram, double *cost2, double *info8) {
  using clock = std::chrono::steady_clock;
  auto ms_since = [](clock::time_point t) { return std::chrono::duration<double, std::milli>(clock::now() - t).count(); };
  const std::string tag = std::string(tag_) + " project: ";
  if (info8) {
    std::fill(info8, info8 + 8, 0.0);
    info8[7] = kGramCols;
  }
  DeviceProblem *central = opt.world_size == 1 ? central_problem() : nullptr;
  if (!central || weights_ranked() || (team && team->ranked) || exchange_attached) {
    set_last_error(tag + "serves single-process sessions without an exchange; the ranks of a job, and a session an "
                   "exchange was created on, project together through dcora_exchange_project");
    return DCORA_ERR_UNSUPPORTED;
  }
  const auto t_begin = clock::now();
  const ManiDesc m = global_manifold();
  const int r_old = m.r, d = m.d;
  const long k = m.k;
  DCORA_HIP(hipSetDevice(opt.device));
  // a. nothing of the session is in flight
  int rc = drain(true);
  if (!rc) rc = project_buffers(m);
  if (rc) return rc;
  SessionProjectState &ps = project_;
  // b. G in one pass, down to the host; its eigenvectors
  std::vector<double> G((size_t)r_old * r_old), w, V;
  DCORA_HIP(hipEventRecord(ps.ev0, st));
  launch_gram(st, r_old, k, Xg.p, ps.partials.p, ps.gram.p);
  DCORA_HIP(hipGetLastError());
  DCORA_HIP(hipEventRecord(ps.ev1, st));
  DCORA_HIP(hipMemcpyAsync(G.data(), ps.gram.p, sizeof(double) * G.size(), hipMemcpyDeviceToHost, st));
  DCORA_HIP(hipStreamSynchronize(st));
  float gram_ms = 0, rest_ms = 0;
  DCORA_HIP(hipEventElapsedTime(&gram_ms, ps.ev0, ps.ev1));
  sym_eig_descending(r_old, G.data(), &w, &V);
  if (gram) std::copy(G.begin(), G.end(), gram);
  if (sigma)
    for (int j = 0; j < r_old; ++j) sigma[j] = std::sqrt(std::max(w[(size_t)j], 0.0));
  double f = 0, gn = 0;
  if (r_old == d) {
    // the reference passes X through unprojected at r == d: the session is not touched
    if (cost2 || info8) {
      rc = central->eval_dev(Xg.p, &f, &gn);
      if (rc) return rc;
    }
    if (cost2) *cost2 = 2.0 * f;
    if (info8) info8[3] = gn, info8[4] = gram_ms, info8[6] = ms_since(t_begin);
    return DCORA_OK;
  }
  // c. the determinant count under V_d, the reflection rule folded into its last column
  RoundBlock blk;
  blk.n = m.n, blk.l = m.l, blk.b = m.b, blk.se = m.se, blk.X = Xg.p;
  const size_t basis_bytes = sizeof(double) * (size_t)r_old * d;
  int npos = 0;
  DCORA_HIP(hipEventRecord(ps.ev2, st));
  DCORA_HIP(hipMemcpyAsync(ps.basis.p, V.data(), basis_bytes, hipMemcpyHostToDevice, st));
  DCORA_HIP(hipMemsetAsync(ps.count.p, 0, sizeof(int), st));
  launch_project_dets(st, r_old, d, blk, ps.basis.p, ps.count.p);
  DCORA_HIP(hipGetLastError());
  DCORA_HIP(hipMemcpyAsync(&npos, ps.count.p, sizeof(int), hipMemcpyDeviceToHost, st));
  DCORA_HIP(hipStreamSynchronize(st));
  const bool reflect = reflect_rule(npos, m.n);
  if (reflect) {
    for (int q = 0; q < r_old; ++q) V[(size_t)(d - 1) * r_old + q] = -V[(size_t)(d - 1) * r_old + q];
    DCORA_HIP(hipMemcpyAsync(ps.basis.p, V.data(), basis_bytes, hipMemcpyHostToDevice, st));
  }
  // d. the projected point, aside
  launch_project_block(st, r_old, d, blk, ps.basis.p, ps.point.p);
  DCORA_HIP(hipGetLastError());
  DCORA_HIP(hipEventRecord(ps.ev3, st));
  DCORA_HIP(hipStreamSynchronize(st));
  DCORA_HIP(hipEventElapsedTime(&rest_ms, ps.ev2, ps.ev3));
  if (basis) std::copy(V.begin(), V.begin() + (size_t)r_old * d, basis);
  // e. the swap: the central problem and every hosted agent's at rank d, then the session re-dimensioned at the point.
  // What has been re-ranked goes back to r_old on every way out before the commit.
  const auto te = clock::now();
  RankChange<DeviceProblem> change(r_old);
  rc = change.add(central, d);
  for (int a = 0; a < R && !rc; ++a)
    if (agent_core(a).hosted) rc = change.add(agent_core(a).prob.get(), d);
  if (rc) return rc;
  double redim_ms = ms_since(te);
  // 2 f and |rgrad| of the point on the session's current matrices and weights
  if (cost2 || info8) {
    rc = central->eval_dev(ps.point.p, &f, &gn);
    if (rc) return rc;
  }
  const auto tf = clock::now();
  rc = redimension("project", d, ps.point.p, change);
  if (rc) return rc;
  redim_ms += ms_since(tf);
  if (cost2) *cost2 = 2.0 * f;
  if (info8) {
    info8[0] = 1, info8[1] = reflect ? 1 : 0, info8[2] = npos, info8[3] = gn;
    info8[4] = (double)gram_ms + (double)rest_ms, info8[5] = redim_ms, info8[6] = ms_since(t_begin);
  }
  return DCORA_OK;
}

// ---- the session's half of the collective projection (session_core.h) ------------------------------------------------
namespace {
RoundBlock round_block_of(const AgentBlock &ab) {
  RoundBlock blk;
  blk.X = ab.X, blk.n = ab.n, blk.l = ab.l, blk.b = ab.b, blk.se = ab.se;
  return blk;
}
}  // namespace

int SessionCore::project_trial_grams(std::vector<int> *hosted, std::vector<double> *grams) {
  const std::string tag = std::string(tag_) + " project: ";
  DCORA_HIP(hipSetDevice(opt.device));
  const ManiDesc m = global_manifold();
  int rc = drain(true);
  if (!rc) rc = project_buffers(m);
  if (rc) return rc;
  std::unique_ptr<ProjectTrial> t(new ProjectTrial(r));
  std::vector<GramBlock> table;
  long nwg = 0;
  for (int a = 0; a < R; ++a) {
    if (!agent_core(a).hosted) continue;
    const AgentBlock ab = agent_block(a);
    t->hosted.push_back(a);
    table.push_back(GramBlock{ab.X, (long)ab.k, nwg});
    nwg += gram_workgroups_of(ab.k);
  }
  const size_t nh = t->hosted.size();
  table.push_back(GramBlock{nullptr, 0, nwg});
  SessionProjectState &ps = project_;
  const size_t np = 256 * (size_t)std::max<long>(nwg, 1), ng = 256 * std::max<size_t>(nh, 1);
  if (ps.partials_cap < np) {
    DCORA_HIP(ps.partials.alloc(np));
    ps.partials_cap = np;
  }
  if (ps.grams_cap < ng) {
    DCORA_HIP(ps.grams.alloc(ng));
    ps.grams_cap = ng;
  }
  if (ps.table_cap < table.size()) {
    DCORA_HIP(ps.table.alloc(table.size()));
    ps.table_cap = table.size();
  }
  const size_t rr = (size_t)r * r;
  grams->assign(nh * rr, 0.0);
  DCORA_HIP(hipMemcpyAsync(ps.table.p, table.data(), sizeof(GramBlock) * table.size(), hipMemcpyHostToDevice, st));
  DCORA_HIP(hipEventRecord(ps.ev0, st));
  launch_gram_blocks(st, r, (int)nh, nwg, ps.table.p, ps.partials.p, ps.grams.p);
  DCORA_HIP(hipGetLastError());
  DCORA_HIP(hipEventRecord(ps.ev1, st));
  if (nh) DCORA_HIP(hipMemcpyAsync(grams->data(), ps.grams.p, sizeof(double) * nh * rr, hipMemcpyDeviceToHost, st));
  DCORA_HIP(hipStreamSynchronize(st));
  float ms = 0;
  DCORA_HIP(hipEventElapsedTime(&ms, ps.ev0, ps.ev1));
  t->kernel_ms = ms;
  *hosted = t->hosted;
  project_trial_ = std::move(t);
  return DCORA_OK;
}

int SessionCore::project_trial_dets(const double *basis, double *npos) {
  ProjectTrial &t = *project_trial_;
  SessionProjectState &ps = project_;
  DCORA_HIP(hipSetDevice(opt.device));
  const int d = dim();
  int count = 0;
  DCORA_HIP(hipEventRecord(ps.ev2, st));
  DCORA_HIP(hipMemcpyAsync(ps.basis.p, basis, sizeof(double) * (size_t)r * d, hipMemcpyHostToDevice, st));
  DCORA_HIP(hipMemsetAsync(ps.count.p, 0, sizeof(int), st));
  for (int id : t.hosted) launch_project_dets(st, r, d, round_block_of(agent_block(id)), ps.basis.p, ps.count.p);
  DCORA_HIP(hipGetLastError());
  DCORA_HIP(hipEventRecord(ps.ev3, st));
  DCORA_HIP(hipMemcpyAsync(&count, ps.count.p, sizeof(int), hipMemcpyDeviceToHost, st));
  DCORA_HIP(hipStreamSynchronize(st));
  float ms = 0;
  DCORA_HIP(hipEventElapsedTime(&ms, ps.ev2, ps.ev3));
  t.kernel_ms += ms;
  *npos = (double)count;
  return DCORA_OK;
}

int SessionCore::project_trial_point(const double *basis, double **mirror) {
  ProjectTrial &t = *project_trial_;
  SessionProjectState &ps = project_;
  DCORA_HIP(hipSetDevice(opt.device));
  const int d = dim();
  const size_t k = (size_t)num_cols();
  if (hipSuccess != t.mirror.alloc((size_t)d * k)) {
    (void)hipGetLastError();
    set_last_error(std::string(tag_) + " project: out of device memory");
    return DCORA_ERR_HIP;
  }
  // (columns no hosted agent owns and no neighbour publishes are read by nobody: zero, as a fresh mirror has them)
  DCORA_HIP(hipMemsetAsync(t.mirror.p, 0, sizeof(double) * (size_t)d * k, st));
  DCORA_HIP(hipEventRecord(ps.ev2, st));
  DCORA_HIP(hipMemcpyAsync(ps.basis.p, basis, sizeof(double) * (size_t)r * d, hipMemcpyHostToDevice, st));
  size_t off = 0;  // the hosted blocks one behind the other in the point buffer (d x num_cols(): room enough)
  for (int id : t.hosted) {
    const AgentBlock ab = agent_block(id);
    launch_project_block(st, r, d, round_block_of(ab), ps.basis.p, ps.point.p + off);
    const int rc = scatter_block(ab, d, ps.point.p + off, t.mirror.p);
    if (rc) return rc;
    off += (size_t)d * ab.k;
  }
  DCORA_HIP(hipGetLastError());
  DCORA_HIP(hipEventRecord(ps.ev3, st));
  DCORA_HIP(hipStreamSynchronize(st));
  float ms = 0;
  DCORA_HIP(hipEventElapsedTime(&ms, ps.ev2, ps.ev3));
  t.kernel_ms += ms;
  *mirror = t.mirror.p;
  return DCORA_OK;
}

int SessionCore::project_trial_commit(double *redim_ms) {
  const auto te = std::chrono::steady_clock::now();
  ProjectTrial &t = *project_trial_;
  const int d = dim();
  DCORA_HIP(hipSetDevice(opt.device));
  int rc = DCORA_OK;
  for (int id : t.hosted)
    if ((rc = t.change.add(agent_core(id).prob.get(), d))) return rc;
  if (DeviceProblem *central = central_problem())  // (a one-rank job keeps its whole-graph evaluation)
    if ((rc = t.change.add(central, d))) return rc;
  // (a failure before redimension's commit leaves the re-ranks to project_trial_abort; after it nothing is left to it)
  rc = redimension("project", d, t.mirror.p, t.change);
  if (rc) return rc;
  if (redim_ms) *redim_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - te).count();
  project_trial_.reset();
  return DCORA_OK;
}

void SessionCore::project_trial_abort() {
  if (!project_trial_) return;
  (void)hipSetDevice(opt.device);
  project_trial_.reset();  // (its RankChange rolls back)
}

}  // namespace dcora
