// Projection of a live RBCD session (either kind) to rank d where its iterate lies: how CORA ends a certified solve (ref
// examples/SingleRobotExample_RASLAM.cpp:220-234, projectSolutionRASLAM src/DCORA_utils.cpp:1984-2031).  With
// X^T = U S V^T the rank-d truncation is (U_d S_d)^T = V_d^T X, V_d the top-d eigenvectors of G = X X^T (r x r):
//   1. G in ONE pass over X on the matrix pipe (k_gram_mfma: a workgroup owns kGramCols columns and writes its
//      16 x 16 partial; k_gram_finish adds the partials in workgroup order -- no floating-point atomics, the same X
//      gives the same G bit for bit, on any device);
//   2. the r x r eigenproblem on the host (small_eig.h), all that crosses: r^2 doubles down, r d doubles up;
//   3. the number of blocks V_d^T Y_i with positive determinant (k_project_dets: four lanes per pose, one integer
//      atomicAdd per wave), the reflection rule npos < n / 2 folded into V_d (its last column negated);
//   4. the point [ Proj_SO(d)(V_d^T Y_i) | V_d^T p_i ], unit spheres normalised, landmarks truncated, written as the
//      d-row columns of the new mirror in its own ordering (k_project_states / k_project_points: the kernels of
//      session_round.hip with V_d in the anchor's place and the mirror as output, round_quad.h).
// SessionCore::project (session_core.h) then takes the session from r to d the way lift takes it from r to r + 1.
#pragma once
#include <hip/hip_runtime.h>

#include "device_problem.h"
#include "session_round.h"

namespace dcora {

// columns of X one workgroup of k_gram_mfma owns: a constant, so that the partial sums -- and with them every bit of
// G -- do not depend on the device (3 * 256 = 4 * 192: whole poses of either dimension; 48 steps of 4 columns per wave)
constexpr int kGramCols = 768;

inline long gram_workgroups(long k) { return k > 0 ? (k + kGramCols - 1) / kGramCols : 1; }

// G = X X^T (r x r column-major, device) of X r x k column-major, 1 <= r <= 16; partials: 256 gram_workgroups(k)
// doubles.  Enqueued on st; nothing synchronises.
void launch_gram(hipStream_t st, int r, long k, const double *X, double *partials, double *G);

// The same for a list of blocks in ONE launch pair (what a rank of a job needs: one matrix per hosted agent, see
// Exchange::project).  table (device): nblocks + 1 entries, entry b = {X of block b (r x k column-major), k >= 0, the
// sum of gram_workgroups_of(k) over the blocks before it}, the last entry's wg0 the total nwg.  partials: 256 nwg
// doubles; grams: nblocks x r x r.  Chunks are counted from each block's first column and every block has a finishing
// workgroup of its own, so grams[b] is bit for bit what launch_gram gives on block b alone -- wherever the block
// stands in the list and whatever stands beside it.  A block with k = 0 owns no workgroup and yields zeros.
struct GramBlock {
  const double *X;
  long k, wg0;
};
inline long gram_workgroups_of(long k) { return (k + kGramCols - 1) / kGramCols; }
void launch_gram_blocks(hipStream_t st, int r, int nblocks, long nwg, const GramBlock *table, double *partials,
                        double *grams);

// *count += the number of poses of blk with det(basis^T Y_i) > 0; basis: r x d column-major, device
void launch_project_dets(hipStream_t st, int r, int d, const RoundBlock &blk, const double *basis, int *count);

// out (d x the block's columns, the block's own ordering) = Proj(basis^T X)
void launch_project_block(hipStream_t st, int r, int d, const RoundBlock &blk, const double *basis, double *out);

// What a session keeps between projections (there is usually one per solve): sized on first use.
struct SessionProjectState {
  DevBuf<double> partials, gram, basis, point;
  DevBuf<int> count;
  size_t partials_cap = 0, point_cap = 0;
  DevBuf<double> grams;    // the collective form: one r x r matrix per hosted agent ...
  DevBuf<GramBlock> table;  // ... and the block list of their launch pair
  size_t grams_cap = 0, table_cap = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;  // around the Gram kernels / the rest
  SessionProjectState() = default;
  SessionProjectState(const SessionProjectState &) = delete;
  SessionProjectState &operator=(const SessionProjectState &) = delete;
  ~SessionProjectState() {
    for (hipEvent_t e : {ev0, ev1, ev2, ev3})
      if (e) (void)hipEventDestroy(e);
  }
};

}  // namespace dcora
