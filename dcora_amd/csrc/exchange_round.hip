// The last step of a solve across the ranks of a job (see exchange.h, Exchange::round): every agent's own trajectory
// against the shared anchor, rounded on the rank that hosts it (ref examples/MultiRobotExample.cpp:341-347,
// examples/MultiRobotExample_RASLAM.cpp:488-495, src/Agent.cpp:1014-1033).
#include "exchange.h"

#include <algorithm>
#include <cstring>

namespace dcora {

int Exchange::round(int anchor_pose, const double *anchor, double *trajectory, double *unit_spheres,
                    double *landmarks) {
  SessionCore &s = *s_;
  // ---- refusals: decided from the arguments alone, the same on every rank, nothing touched ----
  int rc = s.round_check_args(anchor_pose, anchor, trajectory);
  if (rc) return rc;
  const ManiDesc m = s.global_manifold();
  const size_t na = (size_t)m.r * (m.d + 1);
  // ---- the anchor: the hosting rank's words, zeros from everybody else, added in rank order ----
  std::vector<double> A(na, 0.0);
  if (anchor) {
    std::copy(anchor, anchor + na, A.begin());
  } else {
    rc = s.round_fetch_anchor(anchor_pose, A.data());
    if (rc) return fail(std::string("round: ") + dcora_last_error(), rc);
    for (size_t off = 0; off < na; off += 31) {
      rc = allreduce_sum(A.data() + off, (int)std::min<size_t>(31, na - off));
      if (rc) return rc;
    }
  }
  // ---- every rank's own states into the X area at their global places, then the whole of it out, as gather_X ----
  const size_t nt = (size_t)m.d * (m.d + 1) * m.n, ns = (size_t)m.d * m.l, nl = (size_t)m.d * m.b;
  double *area = lay_.x(map_);
  rc = s.round_hosted(A.data(), area, area + nt, area + nt + ns);
  if (rc) return fail(std::string("round: ") + dcora_last_error(), rc);
  rc = barrier();
  if (rc) return rc;
  std::memcpy(trajectory, area, sizeof(double) * nt);
  if (unit_spheres && ns) std::memcpy(unit_spheres, area + nt, sizeof(double) * ns);
  if (landmarks && nl) std::memcpy(landmarks, area + nt + ns, sizeof(double) * nl);
  return barrier();
}

}  // namespace dcora
