// Rounding of a live session on the device (see session_round.h): the kernels and SessionCore::round, the flow both
// session kinds and the exchange share.
#include "session_round.h"

#include <chrono>
#include <cmath>
#include <cstring>

#include "device_chol.h"
#include "round_quad.h"
#include "session_core.h"

namespace dcora {

namespace {

// the anchor into LDS: sm[a r + q] = R0(q, a) for a < D, sm[D r + q] = p_anchor(q).  Every workgroup reads the same
// r (D + 1) words, so every one of them forms the same frame.
template <int D>
__device__ __forceinline__ void load_anchor(int r, const double *__restrict__ rot, const double *__restrict__ trans,
                                            double *sm) {
  const int t = threadIdx.x;
  if (t < r * D)
    sm[t] = rot[t];
  else if (t < r * (D + 1))
    sm[t] = trans[t - r * D];
  __syncthreads();
}

// T_i = [ Proj_SO(D)(R0^T Y_i) | R0^T p_i - t0 ] for the n poses of a block, four lanes per pose.  Lane c reads column c
// of its pose (r contiguous doubles; in the SE ordering the 16 poses of a wave are one contiguous run) and forms the D
// elements of R0^T times it, each ONE sum over q = 0 .. r-1 in index order through fma(): neither the schedule nor the
// compiler's contraction decides a bit.  Every lane forms t0 = R0^T p_anchor the same way (LDS broadcasts), lane D
// subtracts it.  The quad then hands its D rotation columns round with quad_perm moves, every lane projects the whole
// block (so_project: the same operations on the same bits in the D lanes that store), lane c keeps column c: D
// contiguous doubles of the trajectory, and -- where asked -- the r doubles R0 (that column) of the lifted point.
// No atomics, no partial sums, nothing but the anchor in LDS.
template <int D, class Cols>
__global__ __launch_bounds__(kBlock) void k_round_states(int r, int n, Cols cols, const double *__restrict__ X,
                                                         const double *__restrict__ arot,
                                                         const double *__restrict__ atrans, double *__restrict__ traj,
                                                         double *__restrict__ lifted) {
  __shared__ double sm[16 * (D + 1)];
  load_anchor<D>(r, arot, atrans, sm);
  const long g = (long)blockIdx.x * kBlock + threadIdx.x;
  const int c = threadIdx.x & (kQuad - 1);
  const long il = g / kQuad;
  const bool valid = il < n && c <= D;  // (a quad is valid or not as a whole but for its idle lane at D = 2)
  const int i = valid ? (int)il : 0;
  const long column = cols.col(i, valid ? c : 0);
  const double *__restrict__ y = X + column * r;
  double m[D], t0[D];
#pragma unroll
  for (int a = 0; a < D; ++a) m[a] = t0[a] = 0.0;
  for (int q = 0; q < r; ++q) {
    const double yq = valid ? y[q] : 0.0;
    const double pq = sm[D * r + q];
#pragma unroll
    for (int a = 0; a < D; ++a) {
      const double R0 = sm[a * r + q];
      m[a] = fma(R0, yq, m[a]);
      t0[a] = fma(R0, pq, t0[a]);
    }
  }
  if (c == D) {
#pragma unroll
    for (int a = 0; a < D; ++a) m[a] -= t0[a];
  }
  double v[D];
  quad_so_project<D>(m, c, v);
  if (!valid) return;
  double *__restrict__ o = traj + ((long)i * (D + 1) + c) * D;
#pragma unroll
  for (int a = 0; a < D; ++a) o[a] = v[a];
  if (lifted) {
    double *__restrict__ z = lifted + column * r;
    for (int q = 0; q < r; ++q) {
      double s = 0.0;
#pragma unroll
      for (int a = 0; a < D; ++a) s = fma(sm[a * r + q], v[a], s);
      z[q] = s;
    }
  }
}

// `count` point columns (X, lifted: their first column): out(:, j) = R0^T x_j - shift t0, the sums as above.  The
// lifted image is R0 out(:, j), of out(:, j) / |out(:, j)| where normalise is set (unit spheres).  One lane per point:
// a block has few of them beside its poses.
template <int D>
__global__ __launch_bounds__(kBlock) void k_round_points(int r, int count, const double *__restrict__ X,
                                                         const double *__restrict__ arot,
                                                         const double *__restrict__ atrans, int shift, int normalise,
                                                         double *__restrict__ out, double *__restrict__ lifted) {
  __shared__ double sm[16 * (D + 1)];
  load_anchor<D>(r, arot, atrans, sm);
  const long j = (long)blockIdx.x * kBlock + threadIdx.x;
  if (j >= count) return;
  const double *__restrict__ x = X + j * r;
  double m[D], t0[D];
#pragma unroll
  for (int a = 0; a < D; ++a) m[a] = t0[a] = 0.0;
  for (int q = 0; q < r; ++q) {
    const double xq = x[q], pq = sm[D * r + q];
#pragma unroll
    for (int a = 0; a < D; ++a) {
      const double R0 = sm[a * r + q];
      m[a] = fma(R0, xq, m[a]);
      t0[a] = fma(R0, pq, t0[a]);
    }
  }
  if (shift) {
#pragma unroll
    for (int a = 0; a < D; ++a) m[a] -= t0[a];
  }
#pragma unroll
  for (int a = 0; a < D; ++a) out[j * D + a] = m[a];
  if (!lifted) return;
  if (normalise) unit_or_zero<D>(m);
  double *__restrict__ z = lifted + j * r;
  for (int q = 0; q < r; ++q) {
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a) s = fma(sm[a * r + q], m[a], s);
    z[q] = s;
  }
}

template <int D>
void launch_round_block_d(hipStream_t st, int r, const RoundBlock &blk, const RoundAnchor &an, const RoundOut &out) {
  const unsigned grid = (unsigned)(((long)blk.n * kQuad + kBlock - 1) / kBlock);
  if (blk.n > 0 && out.traj) {
    if (blk.se)
      hipLaunchKernelGGL((k_round_states<D, SeCols<D>>), dim3(grid), dim3(kBlock), 0, st, r, blk.n, SeCols<D>{}, blk.X,
                         an.rot, an.trans, out.traj, out.lifted);
    else
      hipLaunchKernelGGL((k_round_states<D, RaCols<D>>), dim3(grid), dim3(kBlock), 0, st, r, blk.n,
                         (RaCols<D>{blk.n, blk.l}), blk.X, an.rot, an.trans, out.traj, out.lifted);
  }
  if (blk.se) return;
  const long s0 = (long)D * blk.n, l0 = s0 + blk.l + blk.n;  // first sphere / landmark column
  if (blk.l > 0 && out.spheres)
    hipLaunchKernelGGL(k_round_points<D>, dim3((unsigned)((blk.l + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, r, blk.l,
                       blk.X + s0 * r, an.rot, an.trans, 0, 1, out.spheres, out.lifted ? out.lifted + s0 * r : nullptr);
  if (blk.b > 0 && out.landmarks)
    hipLaunchKernelGGL(k_round_points<D>, dim3((unsigned)((blk.b + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, r, blk.b,
                       blk.X + l0 * r, an.rot, an.trans, 1, 0, out.landmarks,
                       out.lifted ? out.lifted + l0 * r : nullptr);
}

// `count` doubles from the device into host memory: enqueued on st through pinned staging where there is some; the
// caller synchronises st and then calls finish()
struct Fetch {
  char *pin = nullptr;
  size_t bytes = 0;
  double *host = nullptr;
  hipError_t start(hipStream_t st, const double *dev, size_t count, double *host_) {
    host = host_;
    bytes = count * sizeof(double);
    if (!bytes) return hipSuccess;
    pin = pinned_acquire(bytes);
    return hipMemcpyAsync(pin ? (void *)pin : (void *)host, dev, bytes, hipMemcpyDeviceToHost, st);
  }
  void finish(bool ok) {
    if (pin && ok) std::memcpy(host, pin, bytes);
    if (pin) pinned_release(pin, bytes);
    pin = nullptr;
  }
};

}  // namespace

void launch_round_block(hipStream_t st, int r, int d, const RoundBlock &blk, const RoundAnchor &anchor,
                        const RoundOut &out) {
  if (d == 3)
    launch_round_block_d<3>(st, r, blk, anchor, out);
  else
    launch_round_block_d<2>(st, r, blk, anchor, out);
}

int SessionCore::round_check_args(int anchor_pose, const double *anchor, const double *trajectory) const {
  const std::string tag = std::string(tag_) + " round: ";
  const ManiDesc m = global_manifold();
  if (!trajectory) {
    set_last_error(tag + "trajectory is null");
    return DCORA_ERR_BAD_ARG;
  }
  if (anchor_pose < 0 || anchor_pose >= m.n) {
    set_last_error(tag + "anchor_pose must be a pose of the problem, 0 .. n - 1");
    return DCORA_ERR_BAD_ARG;
  }
  if (anchor)
    for (int e = 0; e < m.r * (m.d + 1); ++e)
      if (!std::isfinite(anchor[e])) {
        set_last_error(tag + "the anchor must be r x (d + 1) finite numbers");
        return DCORA_ERR_BAD_ARG;
      }
  return DCORA_OK;
}

int SessionCore::round_buffers(const ManiDesc &m, bool with_lifted) {
  SessionRoundState &rs = round_;
  if (rs.r != m.r || !rs.traj.p) {
    DCORA_HIP(rs.anchor.alloc((size_t)m.r * (m.d + 1)));
    DCORA_HIP(rs.traj.alloc((size_t)m.d * (m.d + 1) * m.n));
    DCORA_HIP(rs.spheres.alloc((size_t)m.d * m.l));
    DCORA_HIP(rs.landmarks.alloc((size_t)m.d * m.b));
    rs.lifted.release();
    rs.r = m.r;
  }
  if (with_lifted && !rs.lifted.p) DCORA_HIP(rs.lifted.alloc((size_t)m.r * m.k));
  if (!rs.ev0) DCORA_HIP(hipEventCreate(&rs.ev0));
  if (!rs.ev1) DCORA_HIP(hipEventCreate(&rs.ev1));
  return DCORA_OK;
}

int SessionCore::round(int anchor_pose, const double *anchor, double *trajectory, double *unit_spheres,
                       double *landmarks, double *cost2, double *info4) {
  using clock = std::chrono::steady_clock;
  auto ms_since = [](clock::time_point t) { return std::chrono::duration<double, std::milli>(clock::now() - t).count(); };
  const std::string tag = std::string(tag_) + " round: ";
  if (info4) std::fill(info4, info4 + 4, 0.0);
  DeviceProblem *central = opt.world_size == 1 ? central_problem() : nullptr;
  if (!central) {
    set_last_error(tag + "serves single-process sessions (world_size 1); the ranks of a job round together through "
                   "dcora_exchange_round");
    return DCORA_ERR_UNSUPPORTED;
  }
  int rc = round_check_args(anchor_pose, anchor, trajectory);
  if (rc) return rc;
  const auto t_begin = clock::now();
  const ManiDesc m = global_manifold();
  DCORA_HIP(hipSetDevice(opt.device));
  // the mirror is complete: nothing of the session is in flight on an agent's own stream
  rc = drain(false);
  if (rc) return rc;
  rc = round_buffers(m, cost2 != nullptr);
  if (rc) return rc;
  SessionRoundState &rs = round_;
  // 1. the anchor: a passed one goes to the device behind the stream; a named pose is read where it lies
  RoundAnchor an;
  if (anchor) {
    DCORA_HIP(hipMemcpyAsync(rs.anchor.p, anchor, sizeof(double) * (size_t)m.r * (m.d + 1), hipMemcpyHostToDevice, st));
    an.rot = rs.anchor.p;
    an.trans = rs.anchor.p + (size_t)m.r * m.d;
  } else {
    an.rot = Xg.p + (size_t)m.rot_col(anchor_pose) * m.r;
    an.trans = Xg.p + (size_t)m.euc_col(anchor_pose) * m.r;
  }
  // 2. the kernels
  RoundBlock blk;
  blk.n = m.n, blk.l = m.l, blk.b = m.b, blk.se = m.se, blk.X = Xg.p;
  RoundOut out;
  out.traj = rs.traj.p;
  out.spheres = (unit_spheres || cost2) ? rs.spheres.p : nullptr;
  out.landmarks = (landmarks || cost2) ? rs.landmarks.p : nullptr;
  out.lifted = cost2 ? rs.lifted.p : nullptr;
  DCORA_HIP(hipEventRecord(rs.ev0, st));
  launch_round_block(st, m.r, m.d, blk, an, out);
  DCORA_HIP(hipGetLastError());
  DCORA_HIP(hipEventRecord(rs.ev1, st));
  // 4. (enqueued ahead of the evaluation, whose wait then covers them) the results on their way out
  Fetch ft, fs, fl;
  hipError_t e = ft.start(st, rs.traj.p, (size_t)m.d * (m.d + 1) * m.n, trajectory);
  if (e == hipSuccess && unit_spheres) e = fs.start(st, rs.spheres.p, (size_t)m.d * m.l, unit_spheres);
  if (e == hipSuccess && landmarks) e = fl.start(st, rs.landmarks.p, (size_t)m.d * m.b, landmarks);
  // 3. 2 f and |rgrad| of the lifted rounded point on the session's current matrices
  double f = 0, gn = 0, eval_ms = 0;
  if (e == hipSuccess && cost2) {
    const auto te = clock::now();
    rc = central->eval_dev(rs.lifted.p, &f, &gn);
    eval_ms = ms_since(te);
  }
  const hipError_t e2 = hipStreamSynchronize(st);
  const bool ok = e == hipSuccess && e2 == hipSuccess && !rc;
  ft.finish(ok), fs.finish(ok), fl.finish(ok);
  DCORA_HIP(e);
  DCORA_HIP(e2);
  if (rc) return rc;
  if (cost2) *cost2 = 2.0 * f;
  if (info4) {
    float kms = 0;
    DCORA_HIP(hipEventElapsedTime(&kms, rs.ev0, rs.ev1));
    info4[0] = gn, info4[1] = kms, info4[2] = eval_ms, info4[3] = ms_since(t_begin);
  }
  return DCORA_OK;
}

// ---- the session's half of the collective rounding (session_core.h) ------------------------------------------------
int SessionCore::round_fetch_anchor(int anchor_pose, double *out) {
  const ManiDesc m = global_manifold();
  const int d = m.d;
  DCORA_HIP(hipSetDevice(opt.device));
  BlockStates states;
  for (int a = 0; a < R; ++a) {
    AgentCore &ac = agent_core(a);
    if (!ac.hosted) continue;
    const AgentBlock blk = agent_block(a);
    agent_block_states(blk, d, m.n, m.l, &states);
    for (int j = 0; j < blk.n; ++j) {
      if (states.pose[(size_t)j] != anchor_pose) continue;
      if (ac.own_st) DCORA_HIP(hipStreamSynchronize(ac.own_st));  // (the one agent that holds the pose)
      const long rot = blk.se ? (long)j * (d + 1) : (long)j * d;
      const long trans = blk.se ? rot + d : (long)d * blk.n + blk.l + j;
      DCORA_HIP(hipMemcpyAsync(out, blk.X + rot * r, sizeof(double) * (size_t)r * d, hipMemcpyDeviceToHost, st));
      DCORA_HIP(hipMemcpyAsync(out + (size_t)r * d, blk.X + trans * r, sizeof(double) * (size_t)r, hipMemcpyDeviceToHost,
                               st));
      DCORA_HIP(hipStreamSynchronize(st));
      return DCORA_OK;
    }
  }
  return DCORA_OK;
}

int SessionCore::round_hosted(const double *anchor, double *traj_area, double *spheres_area, double *landmarks_area) {
  const ManiDesc m = global_manifold();
  const int d = m.d;
  DCORA_HIP(hipSetDevice(opt.device));
  int rc = drain(false);
  if (!rc) rc = round_buffers(m, false);
  if (rc) return rc;
  SessionRoundState &rs = round_;
  DCORA_HIP(hipMemcpyAsync(rs.anchor.p, anchor, sizeof(double) * (size_t)m.r * (d + 1), hipMemcpyHostToDevice, st));
  RoundAnchor an;
  an.rot = rs.anchor.p;
  an.trans = rs.anchor.p + (size_t)m.r * d;
  // the hosted agents one behind the other in the outputs (they hold the whole problem's states: room enough)
  std::vector<BlockStates> maps;
  long np = 0, ns = 0, nl = 0;
  for (int a = 0; a < R; ++a) {
    if (!agent_core(a).hosted) continue;
    const AgentBlock ab = agent_block(a);
    maps.emplace_back();
    agent_block_states(ab, d, m.n, m.l, &maps.back());
    RoundBlock blk;
    blk.X = ab.X, blk.n = ab.n, blk.l = ab.l, blk.b = ab.b, blk.se = ab.se;
    RoundOut out;
    out.traj = rs.traj.p + (size_t)np * d * (d + 1);
    out.spheres = rs.spheres.p + (size_t)ns * d;
    out.landmarks = rs.landmarks.p + (size_t)nl * d;
    launch_round_block(st, m.r, d, blk, an, out);
    np += ab.n, ns += ab.l, nl += ab.b;
  }
  DCORA_HIP(hipGetLastError());
  std::vector<double> ht((size_t)np * d * (d + 1)), hs((size_t)ns * d), hl((size_t)nl * d);
  Fetch ft, fs, fl;
  hipError_t e = ft.start(st, rs.traj.p, ht.size(), ht.data());
  if (e == hipSuccess) e = fs.start(st, rs.spheres.p, hs.size(), hs.data());
  if (e == hipSuccess) e = fl.start(st, rs.landmarks.p, hl.size(), hl.data());
  const hipError_t e2 = hipStreamSynchronize(st);
  const bool ok = e == hipSuccess && e2 == hipSuccess;
  ft.finish(ok), fs.finish(ok), fl.finish(ok);
  DCORA_HIP(e);
  DCORA_HIP(e2);
  np = ns = nl = 0;
  const size_t pose_doubles = (size_t)d * (d + 1);
  for (const BlockStates &map : maps) {
    for (int g : map.pose)
      std::memcpy(traj_area + (size_t)g * pose_doubles, &ht[(size_t)np++ * pose_doubles], sizeof(double) * pose_doubles);
    for (int g : map.sphere)
      if (spheres_area) std::memcpy(spheres_area + (size_t)g * d, &hs[(size_t)ns++ * d], sizeof(double) * d);
    for (int g : map.landmark)
      if (landmarks_area) std::memcpy(landmarks_area + (size_t)g * d, &hl[(size_t)nl++ * d], sizeof(double) * d);
  }
  return DCORA_OK;
}

}  // namespace dcora
