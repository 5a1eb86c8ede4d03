// Rounding of a live RBCD session (either kind) where its iterate lies: the last step of a solve, after which the
// reference's drivers read every agent's trajectory in the global frame (getSharedPose(0) -> setGlobalAnchor on every
// agent -> getTrajectoryInGlobalFrame: ref examples/MultiRobotExample.cpp:341-347,
// examples/MultiRobotExample_RASLAM.cpp:488-495, src/Agent.cpp:1014-1033; the alignment itself is
// alignLiftedTrajectoryToFrame, ref src/DCORA_utils.cpp:2262-2289):
//   T_i = [ Proj_SO(d)(R0^T Y_i) | R0^T p_i - t0 ],   R0 = the anchor's rotation columns,  t0 = R0^T p_anchor,
// unit spheres rotated (R0^T s), landmarks rotated and shifted (R0^T L - t0).  The frame is formed on the device, by
// every workgroup from the same r x (d+1) anchor words: no host round trip precedes the launch, and the anchor may be
// the anchor pose's own columns of the mirror.
//
// The lifted rounded point R0 [R_i | t_i] is feasible at the session's rank r, and <R0 Z Q, R0 Z> = <Z Q, Z>: the cost
// of the rounded solution is the central problem's own evaluation of it -- its matrix with the current robust weights,
// its Q-apply -- and no rank-d problem exists anywhere.
// Sphere columns of a range-aided session: the point EVALUATED is [T | s / |s| | L], the sphere columns normalised as
// projectSolutionRASLAM normalises them (ref src/DCORA_utils.cpp:1984-2031); the unit_spheres RETURNED are rotated only
// (R0^T s), as getStatesInLocalFrame and dcora_round_align_trajectory return them.
#pragma once
#include <hip/hip_runtime.h>

#include "device_problem.h"

namespace dcora {

// One run of states in one ordering: a session's whole mirror, or the block of one agent.  se: poses are runs of d + 1
// columns (rotation, translation); else the range-aided ordering [rotations | l unit spheres | translations | b
// landmarks] (rotations at d i, translations at d n + l + i).
struct RoundBlock {
  int n = 0, l = 0, b = 0, se = 1;
  const double *X = nullptr;  // r x ((d + 1) n + l + b), device
};

// The frame's source, device: r x d rotation columns and the r translation words (contiguous behind a passed anchor and
// in the SE ordering, apart in the range-aided one).
struct RoundAnchor {
  const double *rot = nullptr, *trans = nullptr;
};

// Where the rounded states go (device; null: not wanted).  traj: d x (d+1) n in the SE ordering; spheres: d x l;
// landmarks: d x b; lifted: r x (the block's columns) in the block's own ordering, sphere columns normalised.
struct RoundOut {
  double *traj = nullptr, *spheres = nullptr, *landmarks = nullptr, *lifted = nullptr;
};

// k_round_states (and k_round_points where the block has spheres or landmarks) enqueued on st; nothing synchronises.
// d in {2, 3}, d <= r <= 16 (the callers check).
void launch_round_block(hipStream_t st, int r, int d, const RoundBlock &blk, const RoundAnchor &anchor,
                        const RoundOut &out);

// What a session keeps between roundings: the outputs on the device, sized on first use and again after a lift.
struct SessionRoundState {
  int r = 0;
  bool with_lifted = false;
  DevBuf<double> anchor, traj, spheres, landmarks, lifted;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // around the kernels
  SessionRoundState() = default;
  SessionRoundState(const SessionRoundState &) = delete;
  SessionRoundState &operator=(const SessionRoundState &) = delete;
  ~SessionRoundState() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
};

}  // namespace dcora
