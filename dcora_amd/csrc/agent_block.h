// Where a hosted agent's block lies, stated once for both session kinds (SessionCore::agent_block), and the global
// indices of the states it holds.  Host only (no HIP), so that a CPU program can drive the index rule.
#pragma once
#include <vector>

namespace dcora {

// A hosted agent's block as the session holds it NOW.  A pose-graph agent's block is a contiguous range of the mirror
// (cols_dev null, from col0); a range-aided agent's is a buffer of its own with the list of its global columns.  X of a
// contiguous block points into the mirror, which a rank change replaces: the struct is a view taken where it is used,
// never kept across lift_buffers.
struct AgentBlock {
  const double *X = nullptr;       // device: r x k, the agent's ordering
  int k = 0;                       // its columns
  int n = 0, l = 0, b = 0;         // its poses, unit spheres and landmarks
  int se = 1;                      // its ordering: SE ((d + 1) columns per pose), else [rotations | unit spheres |
                                   // translations | landmarks]
  long col0 = 0;                   // contiguous: its first column of the global ordering
  const int *cols_dev = nullptr;   // listed: the global column of each of its columns, on the device ...
  const int *cols_host = nullptr;  // ... and on the host
  bool contiguous() const { return !cols_dev; }
  long global_col(int c) const { return contiguous() ? col0 + c : (long)cols_host[c]; }
};

// The global indices of a block's poses, unit spheres and landmarks, in the block's order.  d, n, l: of the whole
// problem.  A contiguous block lies in a mirror in the SE ordering; a listed one in a mirror in the range-aided ordering,
// where pose p's rotation starts at column d p, unit sphere s is column d n + s and landmark q column d n + l + n + q.
struct BlockStates {
  std::vector<int> pose, sphere, landmark;
};
inline void agent_block_states(const AgentBlock &blk, int d, int n, int l, BlockStates *out) {
  out->pose.resize((size_t)blk.n);
  out->sphere.resize((size_t)blk.l);
  out->landmark.resize((size_t)blk.b);
  if (blk.contiguous()) {
    for (int j = 0; j < blk.n; ++j) out->pose[(size_t)j] = (int)(blk.col0 / (d + 1)) + j;
    return;
  }
  const int *own = blk.cols_host;
  for (int j = 0; j < blk.n; ++j) out->pose[(size_t)j] = own[(size_t)(blk.se ? (d + 1) * j : d * j)] / d;
  for (int j = 0; j < blk.l; ++j) out->sphere[(size_t)j] = own[(size_t)(d * blk.n + j)] - d * n;
  for (int j = 0; j < blk.b; ++j)
    out->landmark[(size_t)j] = own[(size_t)(d * blk.n + blk.l + blk.n + j)] - (d * n + l + n);
}

}  // namespace dcora
