// The relative change of an agent's update on the device: LiftedArray::maxTranslationDistance(X, XPrev) of
// Agent::iterate's status (ref src/Agent.cpp:564-565, src/manifold/Elements.cpp:59-69).
#include "device_problem.h"
#include "kernels.h"

#include <type_traits>

namespace dcora {

// max over the 64 lanes, same value in every lane (the moves of wave_sum_dpp; a maximum does not depend on the order)
__device__ __forceinline__ double wave_max_dpp(double v) {
  v = fmax(v, dpp_move<0xB1>(v));   // quad_perm [1,0,3,2]
  v = fmax(v, dpp_move<0x4E>(v));   // quad_perm [2,3,0,1]
  v = fmax(v, dpp_move<0x141>(v));  // row_half_mirror
  v = fmax(v, dpp_move<0x140>(v));  // row_mirror
  return fmax(fmax(readlane_f64(v, 0), readlane_f64(v, 16)), fmax(readlane_f64(v, 32), readlane_f64(v, 48)));
}

// Where the poses of entry e of the set live, stated once for both layouts (the pattern of SeCols / RaCols, robust.hip).
// SE: the session's mirror and its XPrev, agent b's poses pose_start[b] .. pose_start[b + 1] - 1, translation i at column
// (d+1) i + d.  RA: every agent keeps its own X / XPrev in its own ordering [rotations | unit spheres | translations |
// landmarks] (RaAgentDev, ra_rbcd.h), its pose i's translation at column d n_a + l_a + i: the set carries them by value.
struct SePoses {
  int dh;
  const double *X, *XPrev;
  const int *pose_start;
  RelChangeSet set;
  __device__ __forceinline__ int agent(int e) const { return set.agent[e]; }
  __device__ __forceinline__ const double *x(int) const { return X; }
  __device__ __forceinline__ const double *xprev(int) const { return XPrev; }
  __device__ __forceinline__ int first(int e) const { return pose_start[set.agent[e]]; }
  __device__ __forceinline__ int last(int e) const { return pose_start[set.agent[e] + 1]; }
  __device__ __forceinline__ size_t column(int, int i) const { return (size_t)i * dh + (dh - 1); }
};
struct RaPoses {
  RaRelChangeSet set;
  __device__ __forceinline__ int agent(int e) const { return set.agent[e]; }
  __device__ __forceinline__ const double *x(int e) const { return set.X[e]; }
  __device__ __forceinline__ const double *xprev(int e) const { return set.XPrev[e]; }
  __device__ __forceinline__ int first(int) const { return 0; }
  __device__ __forceinline__ int last(int e) const { return set.n[e]; }
  __device__ __forceinline__ size_t column(int e, int i) const { return (size_t)set.toff[e] + (size_t)i; }
};

// One workgroup per agent of the set, striding over the agent's poses: out[b] = max_i |t_i(X_b) - t_i(XPrev_b)|_2.
// A translation is r contiguous doubles at the column Poses names.  The norm of a pose is the square root of
// its r squares summed in index order by one thread, the maximum of those is exact in any order: the result's bits do
// not depend on the schedule, and nothing is atomic.  `out` may be host-mapped: the store is followed by a system fence,
// so whatever the stream publishes next (the evaluation epilogue's seq) is seen after it.
// Ranked (the team of a multi-rank job): the result is stored into the agent's status slot of the job's shared segment
// and the slot's sequence word after it, as k_eval_publish stores an evaluation: that device store is the all-gather,
// every rank's host reads the slot once the word has arrived.  The reduction is the same code: the same bits.
struct RelNoPublish {};
template <bool Ranked, class Poses>
__global__ __launch_bounds__(kBlock) void k_rel_change(int r, Poses where, double *out,
                                                       std::conditional_t<Ranked, RelChangePublish, RelNoPublish> pub) {
  __shared__ double s_max[kBlock / 64];
  const int e = (int)blockIdx.x;
  const int b = where.agent(e);
  const double *__restrict__ X = where.x(e);
  const double *__restrict__ XPrev = where.xprev(e);
  const int lo = where.first(e), hi = where.last(e);
  double m = 0;
  for (int i = lo + (int)threadIdx.x; i < hi; i += kBlock) {
    const size_t o = where.column(e, i) * r;
    double s = 0;
    for (int k = 0; k < r; ++k) {
      const double e2 = X[o + k] - XPrev[o + k];
      s += e2 * e2;
    }
    m = fmax(m, sqrt(s));
  }
  m = wave_max_dpp(m);
  if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kBlock / 64; ++w) m = fmax(m, s_max[w]);
    if constexpr (Ranked) {
      const uint64_t q = pub.seq[blockIdx.x];
      ShmStatus *slot = pub.slots + (size_t)(q & 1) * pub.R + b;
      __hip_atomic_store((double *)&slot->rel, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __threadfence_system();
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store((uint64_t *)&slot->seq, q, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    } else {
      out[b] = m;
      __threadfence_system();
    }
  }
}

namespace {
// Every (ranked, layout) form of the kernel is launched from here: Pub names the ranked half (RelChangePublish: into the
// status slots; RelNoPublish: into `out`), Poses the layout.  The one-process forms count a launch for an empty set too,
// the ranked ones only a launch that is made (a rank that hosts none of the agents enqueues nothing).
template <class Poses, class Pub>
void launch_rel_change_form(hipStream_t st, int r, const Poses &where, double *out, const Pub &pub) {
  constexpr bool ranked = std::is_same_v<Pub, RelChangePublish>;
  if (!ranked) count_launch();
  if (where.set.count < 1) return;
  if (ranked) count_launch();
  hipLaunchKernelGGL((k_rel_change<ranked, Poses>), dim3(where.set.count), dim3(kBlock), 0, st, r, where, out, pub);
}
}  // namespace

void launch_rel_change(hipStream_t st, int r, int d, const double *X, const double *XPrev, const int *pose_start,
                       const RelChangeSet &set, double *out) {
  launch_rel_change_form(st, r, SePoses{d + 1, X, XPrev, pose_start, set}, out, RelNoPublish{});
}

void launch_rel_change_ranked(hipStream_t st, int r, int d, const double *X, const double *XPrev, const int *pose_start,
                              const RelChangeSet &set, const RelChangePublish &pub) {
  launch_rel_change_form(st, r, SePoses{d + 1, X, XPrev, pose_start, set}, (double *)nullptr, pub);
}

void launch_rel_change_ra(hipStream_t st, int r, const RaRelChangeSet &set, double *out) {
  launch_rel_change_form(st, r, RaPoses{set}, out, RelNoPublish{});
}

void launch_rel_change_ra_ranked(hipStream_t st, int r, const RaRelChangeSet &set, const RelChangePublish &pub) {
  launch_rel_change_form(st, r, RaPoses{set}, (double *)nullptr, pub);
}

namespace {
// two host arrays of N doubles each through one launch of the kernel (launch(dX, dY, dout): one agent, out[0])
template <class Launch>
int host_rel_change(size_t N, const double *X, const double *Y, double *out, Launch &&launch) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    set_last_error("no HIP device available: libdcora_hip has no CPU fallback");
    return DCORA_ERR_NO_DEVICE;
  }
  DevBuf<double> dX, dY, dout;
  DCORA_HIP(dX.alloc(N));
  DCORA_HIP(dY.alloc(N));
  DCORA_HIP(dout.alloc(1));
  DCORA_HIP(hipMemcpy(dX.p, X, sizeof(double) * N, hipMemcpyHostToDevice));
  DCORA_HIP(hipMemcpy(dY.p, Y, sizeof(double) * N, hipMemcpyHostToDevice));
  const int rc = launch(dX.p, dY.p, dout.p);
  if (rc) return rc;
  DCORA_HIP(hipGetLastError());
  DCORA_HIP(hipMemcpy(out, dout.p, sizeof(double), hipMemcpyDeviceToHost));
  return DCORA_OK;
}
}  // namespace

// LiftedArray::maxTranslationDistance of two host arrays through the same kernel (one agent holding all n poses)
int max_translation_distance(int r, int d, int n, const double *X, const double *Y, double *out) {
  if (r < 2 || r > 16 || (d != 2 && d != 3) || d > r || n < 1) {
    set_last_error("max_translation_distance: needs 2 <= r <= 16, d in {2, 3}, d <= r, n >= 1");
    return DCORA_ERR_BAD_ARG;
  }
  return host_rel_change((size_t)r * (d + 1) * n, X, Y, out, [&](const double *dX, const double *dY, double *dout) {
    DevBuf<int> dps;
    DCORA_HIP(dps.alloc(2));
    const int ps[2] = {0, n};
    DCORA_HIP(hipMemcpy(dps.p, ps, sizeof(ps), hipMemcpyHostToDevice));
    RelChangeSet set{};
    set.count = 1;
    launch_rel_change(nullptr, r, d, dX, dY, dps.p, set, dout);
    DCORA_HIP(hipDeviceSynchronize());  // (dps leaves scope)
    return (int)DCORA_OK;
  });
}

// the same of two arrays in the RA ordering [rotations | l unit spheres | translations | b landmarks]: the poses only
int ra_max_translation_distance(int r, int d, int n, int l, int b, const double *X, const double *Y, double *out) {
  if (r < 2 || r > 16 || (d != 2 && d != 3) || d > r || n < 1 || l < 0 || b < 0) {
    set_last_error("ra_max_translation_distance: needs 2 <= r <= 16, d in {2, 3}, d <= r, n >= 1, l >= 0, b >= 0");
    return DCORA_ERR_BAD_ARG;
  }
  const size_t k = (size_t)(d + 1) * n + (size_t)l + (size_t)b;
  return host_rel_change((size_t)r * k, X, Y, out, [&](const double *dX, const double *dY, double *dout) {
    RaRelChangeSet set{};
    set.count = 1;
    set.X[0] = dX;
    set.XPrev[0] = dY;
    set.n[0] = n;
    set.toff[0] = d * n + l;
    launch_rel_change_ra(nullptr, r, set, dout);
    return (int)DCORA_OK;
  });
}

}  // namespace dcora
