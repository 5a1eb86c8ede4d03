// How CORA ends a certified solve, across the ranks of a job (see exchange.h, Exchange::project): the projection of the
// rank-r iterate to rank d (projectSolutionRASLAM, ref src/DCORA_utils.cpp:1984-2031, used at
// examples/SingleRobotExample_RASLAM.cpp:220-234) with every step of SessionCore::project made by the rank that hosts
// the agent, from the agent's own block.
#include "exchange.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <numeric>

#include "small_eig.h"

namespace dcora {

std::atomic<int> g_project_gram_sums{0};  // test / measurement hook (dcora_debug_exchange_project_sums)

namespace {
inline size_t tri(int i, int j) { return (size_t)i + (size_t)j * (j + 1) / 2; }  // i <= j: the packed upper triangle
}  // namespace

// G = sum over the agents a = 0 .. R - 1, in that order, of G_a, every G_a unchanged from the rank that formed it:
// the grouping of the sum does not depend on how the agents are spread over the ranks.  mine: the hosted agents'
// r x r matrices in agent order.  Two transports that keep bits:
//   the X area: the hosting ranks store their agents' packed triangles (r (r + 1) / 2 doubles each) side by side,
//     barrier, everybody adds them in agent order, barrier; in rounds of as many agents as the area holds;
//   the segment's sums: per agent, pieces of at most 31 doubles with zeros from the ranks that do not host it
//     (x + 0 keeps x's bits; the kernels' sums start from +0 and never give -0).  Where not even one triangle fits the
//     area, and when the debug hook asks for it.
int Exchange::project_sum_grams(const std::vector<int> &hosted, const std::vector<double> &mine, int r,
                                std::vector<double> *G) {
  const size_t T = (size_t)r * (r + 1) / 2, rr = (size_t)r * r;
  std::vector<double> P(T, 0.0), piece(T);
  auto packed = [&](int a, double *out) {  // the hosted agent a's triangle, or false
    const auto it = std::lower_bound(hosted.begin(), hosted.end(), a);
    if (it == hosted.end() || *it != a) return false;
    const double *Ga = &mine[(size_t)(it - hosted.begin()) * rr];
    for (int j = 0; j < r; ++j)
      for (int i = 0; i <= j; ++i) out[tri(i, j)] = Ga[i + (size_t)r * j];
    return true;
  };
  const size_t per_round = lay_.x_doubles / T;
  if (per_round == 0 || g_project_gram_sums.load()) {
    for (int a = 0; a < R_; ++a) {
      if (!packed(a, piece.data())) std::fill(piece.begin(), piece.end(), 0.0);
      for (size_t off = 0; off < T; off += 31) {
        const int rc = allreduce_sum(piece.data() + off, (int)std::min<size_t>(31, T - off));
        if (rc) return rc;
      }
      for (size_t e = 0; e < T; ++e) P[e] += piece[e];
    }
  } else {
    double *area = lay_.x(map_);
    for (int a0 = 0; a0 < R_; a0 += (int)std::min<size_t>(per_round, (size_t)R_)) {
      const int a1 = (int)std::min<size_t>((size_t)R_, (size_t)a0 + per_round);
      for (int a = a0; a < a1; ++a) (void)packed(a, area + (size_t)(a - a0) * T);
      int rc = barrier();
      if (rc) return rc;
      for (int a = a0; a < a1; ++a)
        for (size_t e = 0; e < T; ++e) P[e] += area[(size_t)(a - a0) * T + e];
      rc = barrier();
      if (rc) return rc;
    }
  }
  G->resize(rr);
  for (int j = 0; j < r; ++j)
    for (int i = 0; i <= j; ++i) (*G)[i + (size_t)r * j] = (*G)[j + (size_t)r * i] = P[tri(i, j)];
  return DCORA_OK;
}

int Exchange::project(double *sigma, double *basis, double *gram, double *cost2, double *info8) {
  using clock = std::chrono::steady_clock;
  const auto t0 = clock::now();
  auto ms_total = [&] { return std::chrono::duration<double, std::milli>(clock::now() - t0).count(); };
  if (info8) {
    std::fill(info8, info8 + 8, 0.0);
    info8[7] = kGramCols;
  }
  SessionCore &s = *s_;
  const ManiDesc m = s.global_manifold();
  const int r_old = m.r, d = m.d;
  std::vector<int> all((size_t)R_);
  std::iota(all.begin(), all.end(), 0);
  // a step failed on this rank: nothing of its session was written, and the ranks that wait for it learn so (`failed`)
  auto give_up = [&](int rc) {
    const double ms = s.project_trial_ms();
    s.project_trial_abort();
    if (hdr_) hdr_->failed.store(1);
    if (info8) info8[4] = ms, info8[6] = ms_total();
    return rc;
  };
  // a. + b. every rank drains its session and forms G_a of the agents it hosts; G = sum_a G_a in agent order
  std::vector<int> hosted;
  std::vector<double> mine, G, w, V;
  int rc = s.project_trial_grams(&hosted, &mine);
  if (!rc) rc = project_sum_grams(hosted, mine, r_old, &G);
  if (rc) return give_up(rc);
  // c. the same bits through the same code on every rank: the same V_d everywhere, nothing to broadcast
  sym_eig_descending(r_old, G.data(), &w, &V);
  if (gram) std::copy(G.begin(), G.end(), gram);
  if (sigma)
    for (int j = 0; j < r_old; ++j) sigma[j] = std::sqrt(std::max(w[(size_t)j], 0.0));
  double c2 = 0, gn = 0;
  if (r_old == d) {
    // d. the reference passes X through unprojected at r == d: nothing of the job changes
    const double ms = s.project_trial_ms();
    s.project_trial_abort();
    rc = evaluate(&c2, &gn, nullptr, nullptr);  // (collective: made whichever outputs this rank asked for)
    if (rc) return rc;
    if (cost2) *cost2 = c2;
    if (info8) info8[3] = gn, info8[4] = ms, info8[6] = ms_total();
    return DCORA_OK;
  }
  // e. the determinant count over the job (integers: their sum as doubles is exact), the reflection rule on the job's n
  double npos = 0;
  rc = s.project_trial_dets(V.data(), &npos);
  if (!rc) rc = allreduce_sum(&npos, 1);
  if (rc) return give_up(rc);
  const bool reflect = reflect_rule((int)npos, m.n);
  if (reflect)
    for (int q = 0; q < r_old; ++q) V[(size_t)(d - 1) * r_old + q] = -V[(size_t)(d - 1) * r_old + q];
  // f. the hosted blocks projected into a trial mirror of d rows, then everybody's public columns at d rows as in a round
  double *mirror = nullptr;
  rc = s.project_trial_point(V.data(), &mirror);
  if (!rc) rc = post_arr(all.data(), R_, d, mirror);
  if (!rc) rc = wait_arr(all.data(), R_, d, mirror);
  if (rc) return give_up(rc);
  if (basis) std::copy(V.begin(), V.begin() + (size_t)r_old * d, basis);
  const double kernel_ms = s.project_trial_ms();
  // g. every rank's mirror becomes the projected point at once, as Exchange::set_X and lift do
  rc = barrier();
  if (rc) {
    s.project_trial_abort();
    return rc;
  }
  double redim_ms = 0;
  rc = s.project_trial_commit(&redim_ms);
  if (rc) return give_up(rc);
  rc = barrier();
  if (rc) return rc;
  // h. 2 f and |rgrad| of the adopted point: the job's own evaluation
  rc = evaluate(&c2, &gn, nullptr, nullptr);
  if (rc) return rc;
  if (cost2) *cost2 = c2;
  if (info8) {
    info8[0] = 1, info8[1] = reflect ? 1 : 0, info8[2] = npos, info8[3] = gn;
    info8[4] = kernel_ms, info8[5] = redim_ms, info8[6] = ms_total();
  }
  return DCORA_OK;
}

}  // namespace dcora
