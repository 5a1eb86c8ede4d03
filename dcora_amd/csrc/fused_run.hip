// The one-launch tCG run of the dense pose-graph path: k_tcg_run, its grid-wide step and its row sums, the test entry
// of the row sums, and the host side with the fault hooks.  The launch forms it replaces are in fused_step.hip.
#include <algorithm>
#include <atomic>
#include <cstdio>

#include "kernels.h"
#include "tcg_rules.h"
#include "pose_group.h"
#include "fused_pc.h"

namespace dcora {

namespace {

// ---- the same 16-lane row sums for NV values per lane as a reduce-scatter (k_tcg_run) ----------------------------
// row16_sum_dpp adds over the lane bits in the order 1, 2, 4, 8 and leaves every sum in all 16 lanes of its row; only
// one lane stores it.  The tree is a tree over LOGICAL lanes (lane L of a wave holds columns 2 L, 2 L + 1 of a
// 128-column step), so a wave may place logical lane L = l5..l0 in physical lane P = p5..p0 as it likes.  With
//   l0 = p5, l1 = p4, l2 = p0, l3 = p1, l4 = p2, l5 = p3
// level 1 (L ^ 1) pairs P ^ 32 and level 2 (L ^ 2) pairs P ^ 16: v_permlane32_swap / v_permlane16_swap exchange the
// halves of TWO registers at once, so one add reduces two values and leaves the first in one half of the lanes, the
// second in the other: NV values become (NV + 1) / 2 registers, then half as many again (an odd count is padded with a
// zero register whose sums nobody stores).  Levels 3 and 4 (L ^ 4, L ^ 8) are the two quad_perm butterflies on what is
// left.  The logical row (l5 l4) is (p3 p2): the lane with p1 = p0 = 0 of every quad holds the row sums of the values
// 4 j + 2 p4 + p5 (register j).  Same pairs, same order, IEEE addition commutes: bitwise the butterfly's row sums.
__host__ __device__ __forceinline__ int wg_sums_logical_lane(int p) { return ((p >> 5) & 1) | ((p >> 3) & 2) | ((p & 15) << 2); }
template <bool HALF32>
__device__ __forceinline__ double wg_sums_swap_add(double x, double y) {
  typedef unsigned u2 __attribute__((ext_vector_type(2)));
  u2 lo, hi;
  if constexpr (HALF32) {  // lanes 32-63 of x <-> lanes 0-31 of y
    lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(x), (unsigned)__double2loint(y), false, false);
    hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(y), false, false);
  } else {                 // the odd 16-lane rows of x <-> the even rows of y
    lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(x), (unsigned)__double2loint(y), false, false);
    hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(y), false, false);
  }
  return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}
// v[NV]: the values of this lane's LOGICAL lane wg_sums_logical_lane(lane).  Fills sP[i][wave * 4 + logical row] for
// every i < NV, exactly what `if ((lane & 15) == 0) sP[i][wave * 4 + (lane >> 4)] = row16_sum_dpp(v[i])` leaves when
// physical and logical lanes coincide.  Every lane of the wave must take part.
template <int NV>
__device__ __forceinline__ void wg_row_sums(const double (&v)[NV], double (*sP)[4 * kPcNW], int wave, int lane) {
  constexpr int N1 = (NV + 1) / 2, N2 = (N1 + 1) / 2;
  double a[N1], b[N2];
#pragma unroll
  for (int j = 0; j < N1; ++j) a[j] = wg_sums_swap_add<true>(v[2 * j], 2 * j + 1 < NV ? v[2 * j + 1] : 0.0);
#pragma unroll
  for (int j = 0; j < N2; ++j) {
    double s = wg_sums_swap_add<false>(a[2 * j], 2 * j + 1 < N1 ? a[2 * j + 1] : 0.0);
    s += dpp_move<0xB1>(s);  // quad_perm [1,0,3,2]
    s += dpp_move<0x4E>(s);  // quad_perm [2,3,0,1]
    b[j] = s;
  }
  if ((lane & 3) == 0) {
    const int sub = ((lane >> 3) & 2) | (lane >> 5), slot = wave * 4 + ((lane >> 2) & 3);
#pragma unroll
    for (int j = 0; j < N2; ++j)
      if (4 * j + sub < NV) sP[4 * j + sub][slot] = b[j];
  }
}

// ------------------------------------------------------------------------------------------------------
// ONE launch per tCG run (round 5): PC in "first" mode, then [A, PC] per iteration and the retraction of the step, all
// inside one kernel of n / 2 workgroups (one per CU at the headline size: 250), with two grid-wide steps per iteration
// instead of two kernel boundaries.  What it buys (tools/tcg_probe.hip, profiles/r05_persistent_tcg.txt): a grid step
// among 250 resident workgroups costs 1.9 us where a kernel boundary costs 2.9 us of launch floor + the prologue's
// round trips; the workgroup's 8 rows of the inverse stay in REGISTERS for the whole run (64 doubles per lane: 32 MB per
// launch were streamed per iteration); the residual image stays in LDS and only H delta is gathered per iteration.
// What it costs: everything the workgroups exchange inside the launch (z, delta, H delta, the partial sums) crosses the
// XCDs' private L2s through the coherent level -- write-through stores and loads with sc1 -- and the grid must be
// co-resident: the form is used only where n / 2 <= the CU count, never by concurrent solves (the coloured mode), and
// every spin is bounded: a workgroup that waits longer than 2 ms raises an abort word, all workgroups leave, the kernels
// queued behind the run become no-ops (outer_done_stamp) and the host repeats the RTR iteration on the launch form.
// The arithmetic is the launch form's, term for term and sum for sum (same lane layouts, same partial-sum trees: the
// <delta, H delta> partials are rebuilt from the workgroups' 16-lane row sums exactly as k_fused_hess's workgroups of
// PB_A poses add them), so a run is bitwise the run of the launches: tests/test_kernel_forms_gpu.py.
// ------------------------------------------------------------------------------------------------------
constexpr int kRunShards = 32, kRunCopies = 64, kRunStride = 32;  // sync words 128 B apart
constexpr int kRunSyncWords = (kRunShards + 1 + kRunCopies + 1) * kRunStride;
constexpr int kRunQCap = 1024;  // CSR entries of a workgroup's 2 (d+1) matrix rows staged in LDS once per run
constexpr int kRunNS = 4;       // 128-column steps per wave held in registers: k <= 4 * 4 * 128 = 2048
// The most columns a workgroup's list of neighbour pose blocks may hold (column_slots.h): 16 pose blocks of d + 1 = 4.
// What the staged nd = beta d_old - z of those columns takes in LDS is kRunColCap * r doubles, 3 KB at r = 6.  The LDS
// free at r = 6, k = 2048: 160 KB - the image (2048 * 6 * 8 + 16 = 98 320 B) - s_P (49 * 16 * 8 = 6 272 B) - s_Z, s_R,
// s_W, s_D, s_H (1 928 B) - s_ci, s_v (12 288 B) - s_red, s_ok (132 B) = 44 900 B, so LDS is not what bounds the cap:
// every listed pair of doubles is loaded by a thread of its own (ONE 16-byte load per thread and vector), and at
// r = 6 sixteen blocks are 16 * 2 r = 192 of the 256 threads.  A map in which a workgroup names more pose blocks sends the
// problem's runs to the other gather (launch_tcg_run): both gathers in one kernel cost it scratch.
constexpr int kRunColCap = 64;
// ---- where the residual image lies in LDS ----
// Pair i (doubles 2 i, 2 i + 1 of the column-major residual) lies at byte run_img_off(i) of the dynamic LDS: every write
// of the image (first staging, zero fill, the update per iteration) and the product's reads go through it, and
// tests/test_run_image_cpu.py enumerates from it which 16-byte slots of the 256-byte bank row a group of 16 lanes
// hits.  The map is the plain one.  With wg_row_sums' lane map the product's ds_read_b128 are 2-way conflicted at
// r = 5 (8-way at r = 4, 4-way at r = 6); one 16-byte pad behind every 160 pairs makes the r = 5 reads and writes
// conflict-free, and was measured slower: the pad's place depends on the thread, so every piece of the update pays for
// its address (profiles/run_image.txt).  Behind the image lies one spare pair (the update's threads without a pair).
__host__ __device__ constexpr int run_img_off(int i) { return 16 * i; }
constexpr size_t run_img_bytes(int r, int cpad) { return (size_t)run_img_off(cpad * r / 2) + 16; }
struct TcgRunArgs {
  ManiDesc m;
  int ldm;
  const double *Minv;
  CsrDev Q;
  Buf2 grad, X, S;
  double *d0, *d1, *Hd, *eta, *Heta, *z, *p1r, *p3, *pC;
  unsigned *sync;  // zeroed by the single-block kernel in front of the run (k_rtr_init / k_rtr_decide)
  SolverCtl *ctl;
  HostFlags *hf;
  int seq;
  int fault;       // test hook (dcora_debug_tcg_run_fault): workgroup 0 leaves before the first grid step
  ColSlotsDev cols;  // the column-slot map of the 2-pose tiling, no workgroup of it overflowing (lp null: the gather goes entry by entry)
#ifdef DCORA_RUN_STAMPS
  long long *stamps;  // profiling build only: wall_clock64 of workgroup 0 at the phase boundaries of a run
#endif
};
#ifdef DCORA_RUN_STAMPS
// (nothing is scheduled across a stamp: the FMAs of a product stay in front of theirs, its sums behind it)
#define RUN_STAMP(i)                                                            \
  do {                                                                          \
    __builtin_amdgcn_sched_barrier(0);                                          \
    if (a.stamps && blockIdx.x == 0 && threadIdx.x == 0 && (i) < 64) a.stamps[(i)] = wall_clock64(); \
    __builtin_amdgcn_sched_barrier(0);                                          \
  } while (0)
#else
#define RUN_STAMP(i) \
  do {                \
  } while (0)
#endif
// stamps 0 .. 3: start, image of grad, first product + projection, grid step; then kRunStampsPerIter per iteration:
// gather returned, A, grid step, own updates, image, FMAs, row sums, sums over the workgroup, projection, grid step
constexpr int kRunStamp0 = 4, kRunStampsPerIter = 10;
__device__ __forceinline__ double ld_coh(const double *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_coh(double *p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double2 pc_ld16_coh(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {
  const pc_v4u v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 16);  // aux bit 4: sc1 (agent scope)
  return __builtin_bit_cast(double2, v);
}
// grid-wide step `step` (0, 1, 2, ...) of this launch: sharded arrival counters, the last arrival replicates the done
// word, workgroup i polls copy i % 64.  false: this workgroup (or another one) gave up.
// Giving up is decided on the SAME word that counts the completed shards (its top bit): a workgroup whose wait ran out
// sets the bit by compare-and-swap only while the count is incomplete, and the arrival that completes the count
// publishes the done word only if its own increment found the bit clear.  So either the step completes for everybody
// or nobody passes it: a workgroup that was descheduled past its 2 ms while the others completed the step does not
// abort a run the others go on to finish (seen with four ranks sharing one GPU, where waits of milliseconds are routine).
constexpr unsigned kRunAbortBit = 0x80000000u;
__device__ __forceinline__ bool run_grid_step(unsigned *sync, unsigned step, int *s_ok) {
  __builtin_amdgcn_s_waitcnt(0);  // this wave's write-through stores are acknowledged
  __syncthreads();
  // wave 0 enters the arrival: lane 0 counts, and where it completed the count with the abort bit clear the wave's 64
  // lanes publish the 64 copies of the done word with ONE store instruction (lane 0 alone stored them one after the
  // other, and the workgroups polling the late copies left that much later); polling and giving up stay on lane 0
  static_assert(kRunCopies == 64, "one copy of the done word per lane of wave 0");
  if (threadIdx.x < 64) {
    unsigned *shard = sync, *top = sync + kRunShards * kRunStride, *done = top + kRunStride;
    const int i = blockIdx.x, G = gridDim.x, sh = i % kRunShards;
    const unsigned in_shard = (unsigned)((G - sh + kRunShards - 1) / kRunShards), want = step + 1;
    const unsigned shards_used = (unsigned)(G < kRunShards ? G : kRunShards);
    int last = 0;
    if (threadIdx.x == 0) {
      const unsigned a = __hip_atomic_fetch_add(shard + sh * kRunStride, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (a + 1 == want * in_shard) {
        const unsigned b = __hip_atomic_fetch_add(top, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = !(b & kRunAbortBit) && b + 1 == want * shards_used;
      }
    }
    if (__builtin_amdgcn_readfirstlane(last))
      __hip_atomic_store(done + threadIdx.x * kRunStride, want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (threadIdx.x == 0) {
    unsigned *top = sync + kRunShards * kRunStride, *done = top + kRunStride, *abort_w = done + kRunCopies * kRunStride;
    const int i = blockIdx.x, G = gridDim.x;
    const unsigned want = step + 1, shards_used = (unsigned)(G < kRunShards ? G : kRunShards);
    long long t0 = wall_clock64();
    const unsigned *p = done + (i % kRunCopies) * kRunStride;
    int ok = 1;
    unsigned spins = 0;
    while (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
      __builtin_amdgcn_s_sleep(1);
      if ((++spins & 63u) == 0) {
        if (__hip_atomic_load(abort_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
          ok = 0;
          break;
        }
        if (wall_clock64() - t0 > 200000) {  // 2 ms at 100 MHz: the grid is not co-resident
          unsigned cur = __hip_atomic_load(top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          bool gave_up = false;
          for (;;) {
            if (cur & kRunAbortBit) {  // somebody else gave up
              gave_up = true;
              break;
            }
            if (cur >= want * shards_used) break;  // everybody has arrived: the done word is on its way
            if (__hip_atomic_compare_exchange_strong(top, &cur, cur | kRunAbortBit, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT)) {
              gave_up = true;
              break;
            }
          }
          if (gave_up) {
            __hip_atomic_store(abort_w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ok = 0;
            break;
          }
          t0 = wall_clock64();
        }
      }
    }
    *s_ok = ok;
  }
  __syncthreads();
  return *s_ok != 0;
}

// COLS: phase A fetches every neighbour column once per workgroup (the launch carries a column-slot map in which no
// workgroup overflows); otherwise every row gathers its entries' columns itself
template <int D, int R, int NS, bool COLS>
__global__ __launch_bounds__(kPcBlock) void k_tcg_run(TcgRunArgs a) {
  constexpr int DH = D + 1, PB = 2, NR = PB * DH, RM = R;
  // pieces of kPcBlock pairs that hold the largest residual of the form (NS * kPcNW * 128 columns of R doubles): 4 R of
  // them; the per-iteration update of the image takes them kImgGroup at a time
  constexpr int kImgGroup = R == 6 ? 1 : 4;
  constexpr int kImgPieces = kImgGroup == 1 ? kPcSB : NS * kPcNW * 128 * R / 2 / kPcBlock;
  static_assert(kImgPieces <= kPcSB && kImgPieces % kImgGroup == 0, "the image's pieces come in whole groups");
  // the residual image, column-major as in memory: cpad * R doubles in pairs of 16 bytes at run_img_off, kept for the
  // run; 16-byte aligned, so the 2 R doubles a lane takes per step are read 16 bytes at a time
  extern __shared__ __align__(16) double s_img[];
  auto img_pair = [&](int i) { return reinterpret_cast<double2 *>(s_img) + run_img_off(i) / 16; };
  __shared__ double s_P[NR * RM + 1][4 * kPcNW];
  __shared__ double s_Z[NR * RM + 1], s_R[NR * RM], s_W[NR * RM], s_D[NR * RM], s_H[NR * RM];
  __shared__ double s_red[16];
  __shared__ int s_ci[kRunQCap];
  __shared__ double s_v[kRunQCap];
  __shared__ int s_ok;
  // nd = beta d_old - z of the workgroup's listed pose blocks, block after block as in memory: column slot s, row t of
  // the vector at s * R + t (column_slots.h); pair i is written by thread i
  static_assert((DH * R) % 2 == 0, "a pose block is a whole number of 16-byte pairs, 16-byte aligned");
  constexpr int kBlkPairs = DH * R / 2;
  static_assert(kRunColCap / DH * kBlkPairs <= kPcBlock, "one thread per listed pair");
  __shared__ double2 s_N[COLS ? kRunColCap * R / 2 : 1];
  SolverCtl *ctl = a.ctl;
  const int seq = a.seq;
  RUN_STAMP(0);
  const int st_o = ctl->outer_done_stamp, cur = ctl->cur & 1;
  if (seq > st_o) return;  // the RTR loop has ended: no-op (uniform over the grid)
  const double c_Delta = ctl->Delta, c_ngf = ctl->ngf;
  const int c_max_inner = ctl->max_inner;
  const ManiDesc m = a.m;
  constexpr int r = R;
  const int k = m.k, ldm = a.ldm;
  const int pose0 = blockIdx.x * PB;
  const int npose = min(PB, m.n - pose0);
  const int j0 = pose0 * DH, nrow = npose * DH;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int e = threadIdx.x;
  const bool own = e < nrow * r;
  const size_t oown = (size_t)j0 * r + e;
  const int lc = e / r, t = e - lc * r;
  const int g = threadIdx.x >> 3, tt = threadIdx.x & (GW - 1);
  const bool pact = (g < npose) && (tt < r);
  const size_t o = (size_t)(pose0 + min(g, npose - 1)) * DH * r;
  const double *__restrict__ grad = a.grad.p[cur];
  const double *__restrict__ X = a.X.p[cur];
  const unsigned vec_bytes = (unsigned)((size_t)r * k * sizeof(double));
  const __amdgpu_buffer_rsrc_t rs_g = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(grad), 0, vec_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_h = __builtin_amdgcn_make_buffer_rsrc(a.Hd, 0, vec_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_m = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<double *>(a.Minv), 0, (unsigned)((size_t)k * ldm * sizeof(double)), 0x00020000);
  // the logical lane of the product: this lane holds columns 2 llane, 2 llane + 1 of a step (wg_row_sums)
#ifdef DCORA_RUN_BUTTERFLY_SUMS
  const int llane = lane;
#else
  const int llane = wg_sums_logical_lane(lane);
#endif
  const unsigned voff_t = threadIdx.x * 16u, voff_l = (unsigned)llane * 16u;
  // ---- once per run: the workgroup's rows of the inverse (registers), its matrix rows of Q (LDS), its poses ----
  // Loads return in the order of their requests.  Everything the first product needs beside the rows -- the gradient
  // image, the CSR entries of the workgroup's matrix rows, X, S, the own gradient element -- is requested AHEAD of the
  // 32 sixteen-byte loads of the rows (128 KB per workgroup) and with no wait among the requests: the image and |r|^2
  // are built while the rows are still in flight, and step u of the first product waits for mreg[u][*] only.  (Rows
  // first, the image reached LDS only behind the rows, and the CSR staging and the row pointers paid three dependent
  // round trips behind that: profiles/run_waits.txt.)  DCORA_RUN_ROWS_FIRST: the order before.
  double2 mreg[NS][NR];
  auto load_rows = [&]() {
#pragma unroll
    for (int u = 0; u < NS; ++u)
#pragma unroll
      for (int q = 0; q < NR; ++q)
        mreg[u][q] = pc_ld16(rs_m, voff_l, (unsigned)(((size_t)(j0 + q) * ldm + (size_t)(wave_u + kPcNW * u) * 128) * 8));
  };
  const int pbeg = a.Q.rp[j0], pend = a.Q.rp[j0 + nrow];
  // COLS: the workgroup's list of neighbour pose blocks.  Thread i loads pair i of the listed blocks; ONE register is
  // kept for the run, coff: the byte offset of this thread's pair in a vector, kNoPair where it loads none
  constexpr unsigned kNoPair = 0xffffffffu;
  [[maybe_unused]] unsigned coff = kNoPair;
  if constexpr (COLS) {
    // (the host launches this form only where no list exceeds the cap: the min is a bound on s_N, not a path)
    const int cl_b = a.cols.lp[blockIdx.x], cl_n = min(a.cols.lp[blockIdx.x + 1] - cl_b, kRunColCap / DH);
    if (e < cl_n * kBlkPairs) coff = (unsigned)((a.cols.list[cl_b + e / kBlkPairs] * kBlkPairs + e % kBlkPairs) * 16);
  }
  // (with a list s_ci holds the entries' column SLOTS: the same loads through another pointer)
  const int *__restrict__ ci_src = COLS ? a.cols.slot : a.Q.ci;
#ifdef DCORA_RUN_ROWS_FIRST
  load_rows();
#endif
  double2 xg[kPcSB];
#pragma unroll
  for (int u = 0; u < kPcSB; ++u) xg[u] = pc_ld16(rs_g, voff_t, (unsigned)u * kPcBlock * 16u);
#ifdef DCORA_RUN_ROWS_FIRST
  for (int i = threadIdx.x; i < pend - pbeg; i += kPcBlock) {
    s_ci[i] = ci_src[pbeg + i];
    s_v[i] = a.Q.v[pbeg + i];
  }
  const int myb = own ? a.Q.rp[j0 + lc] - pbeg : 0, mye = own ? a.Q.rp[j0 + lc + 1] - pbeg : 0;
#else
  // the CSR entries into registers, every thread kRunQCap / kPcBlock of them (a thread beyond the end loads the last
  // entry again and stores nothing); the row pointers of a thread beyond the rows are those of the last row's end.
  // With a list of pose blocks s_ci holds the entries' column SLOTS: the same loads through another pointer
  constexpr int kStage = kRunQCap / kPcBlock;
  int st_ci[kStage];
  double st_v[kStage];
#pragma unroll
  for (int u = 0; u < kStage; ++u) {
    const int i = min(u * kPcBlock + (int)threadIdx.x, pend - pbeg - 1);
    st_ci[u] = ci_src[pbeg + i];
    st_v[u] = a.Q.v[pbeg + i];
  }
  const int rp_b = a.Q.rp[j0 + min(lc, nrow)], rp_e = a.Q.rp[j0 + min(lc + 1, nrow)];
#endif
  Row<D> Y;
  ld_row<D>(X + o, r, tt, pact, Y);
  double S[D][D];
  {
    const double *__restrict__ Sblk = a.S.p[cur];
#pragma unroll
    for (int aa = 0; aa < D; ++aa)
#pragma unroll
      for (int b = 0; b < D; ++b) S[aa][b] = (g < npose) ? Sblk[(size_t)(pose0 + g) * D * D + aa + b * D] : 0.0;
  }
  double o_r = own ? grad[oown] : 0.0, o_eta = 0, o_Heta = 0, o_d = 0, o_h = 0;
#ifndef DCORA_RUN_ROWS_FIRST
  __builtin_amdgcn_sched_barrier(0);  // (no request of the rows moves ahead of the others)
  load_rows();
  __builtin_amdgcn_sched_barrier(0);
  const int myb = own ? rp_b - pbeg : 0, mye = own ? rp_e - pbeg : 0;
#pragma unroll
  for (int u = 0; u < kStage; ++u) {
    const int i = u * kPcBlock + (int)threadIdx.x;
    if (i < pend - pbeg) {
      s_ci[i] = st_ci[u];
      s_v[i] = st_v[u];
    }
  }
#endif
  // image geometry (one chunk: the host admits the form only where the whole residual fits)
  const int cpad = ((k + 127) / 128) * 128;
  const long Nc = (long)k * r;
  const int npair = (int)((Nc + 1) >> 1);
  const int nstep = cpad / 128;
  // tCG scalars (the control block's, kept in registers by every thread: all of them see the same sums)
  double zr = 0, dPd = 0, ePe = 0, ePd = 0, alpha = 0, ePen = 0;
  const double n0 = c_ngf;
  int status = TR_MAXITER, iters_done = 0;
  unsigned gstep = 0;
  double acc[NR * RM + 1];  // [q * RM + tq]: row q of the workgroup, row tq of the residual; the last one: |r|^2
  double nrm2 = 0;
  // product of the workgroup's rows (registers) with the image, sums over the workgroup: s_Z.  sb: the first of its
  // three stamps in the profiling build (>= 64: none)
  auto product = [&](int sb) {
#pragma unroll
    for (int i = 0; i < NR * RM; ++i) acc[i] = 0;
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const int sidx = wave_u + kPcNW * u;
      if (sidx < nstep) {
        const double2 *__restrict__ xs = img_pair((sidx * 64 + llane) * r);
        double x[2 * RM];  // x[tq]: column 2 llane, x[r + tq]: column 2 llane + 1
#pragma unroll
        for (int tq = 0; tq < RM; ++tq) {
          const double2 xx = xs[tq];
          x[2 * tq] = xx.x;
          x[2 * tq + 1] = xx.y;
        }
#pragma unroll
        for (int tq = 0; tq < RM; ++tq)
#pragma unroll
          for (int q = 0; q < NR; ++q)
            acc[q * RM + tq] = fma(x[tq], mreg[u][q].x, fma(x[r + tq], mreg[u][q].y, acc[q * RM + tq]));
      }
    }
    RUN_STAMP(sb);
#ifdef DCORA_RUN_BUTTERFLY_SUMS
    acc[NR * RM] = nrm2;
#pragma unroll
    for (int i = 0; i <= NR * RM; ++i) {
      const double v = row16_sum_dpp(acc[i]);
      if ((lane & 15) == 0) s_P[i][wave * 4 + (lane >> 4)] = v;
    }
#else
    acc[NR * RM] = __shfl(nrm2, llane);  // |r|^2 is summed over the staging's threads: logical lane = thread
    wg_row_sums<NR * RM + 1>(acc, s_P, wave, lane);
#endif
    RUN_STAMP(sb + 1);
    __syncthreads();
    if ((int)threadIdx.x <= NR * RM) {
      double v = 0;
#pragma unroll
      for (int w = 0; w < 4 * kPcNW; ++w) v += s_P[threadIdx.x][w];
      s_Z[threadIdx.x] = v;
    }
    __syncthreads();
    RUN_STAMP(sb + 2);
  };
  // z = Proj_X(columns), partial <z, r> (wave 0 holds the per-pose lanes), published for the other workgroups
  auto project_z = [&]() {
    if (wave == 0) {
      Row<D> Zr, Rr;
#pragma unroll
      for (int aa = 0; aa < DH; ++aa) {
        Zr.e[aa] = pact ? s_Z[(g * DH + aa) * RM + tt] : 0.0;
        Rr.e[aa] = pact ? s_R[(g * DH + aa) * RM + tt] : 0.0;
      }
      row_tangent<D>(Y, Zr);
      if (pact)
#pragma unroll
        for (int aa = 0; aa < DH; ++aa) st_coh(a.z + o + aa * r + tt, Zr.e[aa]);
      double zacc = 0;
#pragma unroll
      for (int aa = 0; aa < DH; ++aa) zacc += Zr.e[aa] * Rr.e[aa];
      const double tot = wave_sum(zacc);
      if (lane == 0) st_coh(a.p3 + blockIdx.x, tot);
    }
  };
  // the end of a run: control block, eta / H eta, the step itself (k_fused_pc's retract_tail)
  auto finish = [&]() {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      ctl->alpha = alpha;
      ctl->e_Pe_n = ePen;
      ctl->norm_r0 = n0;
      ctl->z_r[0] = ctl->z_r[1] = zr;
      ctl->d_Pd[0] = ctl->d_Pd[1] = dPd;
      ctl->e_Pe[0] = ctl->e_Pe[1] = ePe;
      ctl->e_Pd[0] = ctl->e_Pd[1] = ePd;
      tcg_end_run(ctl, a.hf, seq, status, iters_done);
      host_store(&a.hf->last_seq_done, seq);
    }
    __syncthreads();
    double a0 = 0, a1 = 0;
    if (own) {
      a.eta[oown] = o_eta;
      a.Heta[oown] = o_Heta;
      const double gr = grad[oown];
      a0 = o_eta * gr;
      a1 = o_eta * o_Heta;
      s_R[lc * RM + t] = o_eta;
    }
    __syncthreads();
    if (wave == 0) {
      Row<D> Yn = Y;
#pragma unroll
      for (int aa = 0; aa < DH; ++aa) Yn.e[aa] += 1.0 * (pact ? s_R[(g * DH + aa) * RM + tt] : 0.0);
      row_qf<D>(Yn);
      st_row<D>(a.X.p[cur ^ 1] + o, r, tt, pact, Yn);
    }
    const double t0 = block_sum(a0, s_red);
    const double t1 = block_sum(a1, s_red);
    if (threadIdx.x == 0) {
      a.pC[2 * blockIdx.x] = t0;
      a.pC[2 * blockIdx.x + 1] = t1;
    }
  };
  auto give_up = [&]() {  // the grid is not co-resident: later kernels of this solve become no-ops, the host repeats
    if (threadIdx.x == 0) {
      ctl->outer_done_stamp = seq - 1;
      host_store(&a.hf->tcg_abort_seq, seq);
    }
  };
  // ---- PC, first: z0 = Proj_X(grad Minv), res = grad, eta = H eta = 0 ----
#pragma unroll
  for (int u = 0; u < kPcSB; ++u) {
    const int i = u * kPcBlock + (int)threadIdx.x;
    if (i < npair) {
      const double2 x = xg[u];
      nrm2 = fma(x.x, x.x, nrm2);
      nrm2 = fma(x.y, x.y, nrm2);
      *img_pair(i) = x;  // (the upper half of the last pair of an odd count reads as zero: the buffer ends there)
    }
  }
  for (int i = npair + (int)threadIdx.x; i < cpad * r / 2; i += kPcBlock) *img_pair(i) = double2{0.0, 0.0};
  if (own) s_R[lc * RM + t] = o_r;
  __syncthreads();
  RUN_STAMP(1);
  // COLS: the first kColGB entries of this thread's row -- weight and where the entry's nd lies in s_N -- stay in
  // registers for the run (this form has them to spare): an iteration reads s_N only, one LDS round trip behind the
  // staging's barrier where reading s_ci and s_v again made it two
  constexpr int kColGB = 24;
  [[maybe_unused]] int nq[kColGB];
  [[maybe_unused]] double wq[kColGB];
  if constexpr (COLS) {
#pragma unroll
    for (int q = 0; q < kColGB; ++q) {
      const bool ok = myb + q < mye;
      wq[q] = ok ? s_v[myb + q] : 0.0;
      nq[q] = (ok ? s_ci[myb + q] : 0) * r + t;
    }
  }
  product(64);
  project_z();
  RUN_STAMP(2);
  if (c_max_inner <= 0) {  // (no inner iterations allowed: the launch form leaves eta = 0 behind as well)
    status = TR_MAXITER;
    finish();
    return;
  }
  if (a.fault && blockIdx.x == 0) return;  // (test hook: the others wait in vain, give up after 2 ms and say so)
  if (!run_grid_step(a.sync, gstep++, &s_ok)) return give_up();
  RUN_STAMP(3);
  // ---- the iterations ----
  for (int iter = 0;; ++iter) {
    const int par = iter & 1;
    [[maybe_unused]] const int sb0 = kRunStamp0 + kRunStampsPerIter * iter;
    double *__restrict__ d_new = par ? a.d1 : a.d0;
    const double *__restrict__ d_old = par ? a.d0 : a.d1;
    // ======== A: delta = beta delta - z in the gather, H delta = Proj_X(delta Q - delta S), <delta, H delta> ========
    {
      // the gather's loads first (their addresses do not depend on beta): one round trip through the coherent level for
      // up to kRunGB entries of a matrix row, beside the partials' -- in chunks of 8 behind the partials' sum an
      // iteration paid three to four dependent round trips here
      constexpr int kRunGB = 24;
      double z_own = 0, beta = 0, accw = 0, dn = 0;
      // what every thread does between the requests and the products: <z, r> from the workgroups' partials, beta, the
      // tCG scalars of the new direction (once per iteration, in whichever branch below)
      auto direction = [&]() {
        const int np3 = gridDim.x;
        const int l = lane;
        const double pa = (l < np3) ? ld_coh(a.p3 + l) : 0.0, pb = (l + 64 < np3) ? ld_coh(a.p3 + l + 64) : 0.0;
        const double pcc = (l + 128 < np3) ? ld_coh(a.p3 + l + 128) : 0.0, pd = (l + 192 < np3) ? ld_coh(a.p3 + l + 192) : 0.0;
        const double z_r_new = wave_sum((pa + pb) + (pcc + pd));
#ifdef DCORA_RUN_STAMPS
        __builtin_amdgcn_s_waitcnt(0);  // the gather's loads have returned
        RUN_STAMP(sb0);
#endif
        if (iter > 0) beta = tcg_beta(z_r_new, zr);
        const TcgDir dir = iter == 0 ? tcg_dir_start(z_r_new) : tcg_dir_next(z_r_new, beta, alpha, dPd, ePd);
        zr = dir.z_r;
        ePd = dir.e_Pd;
        dPd = dir.d_Pd;
        ePe = iter == 0 ? 0.0 : ePen;
      };
      // Every term of a row's sum is w * nd with nd = beta d_old - z of the entry's column, as ONE fma each (what the
      // compiler contracts `accw += w * (beta * ga - gz)` to, stated so that it does not depend on where nd is formed):
      // the staged nd of a listed column is the nd every row naming it would form itself, bit for bit.
      if (own) z_own = ld_coh(a.z + oown);
      if constexpr (COLS) {
        // ALL threads request the listed blocks of z and d_old, every pair of doubles once (one 16-byte sc1 load per
        // thread and vector: a pose block is 16-byte aligned), instead of every CSR entry's column by every row that
        // names it; in the same trip as the partials
        double2 cz{0.0, 0.0}, cd{0.0, 0.0};
        if (coff != kNoPair) {
          cz = pc_ld16_coh(__builtin_amdgcn_make_buffer_rsrc(a.z, 0, vec_bytes, 0x00020000), coff, 0);
          if (iter > 0)
            cd = pc_ld16_coh(__builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(d_old), 0, vec_bytes, 0x00020000),
                             coff, 0);
        }
        direction();
        if (coff != kNoPair) s_N[e] = double2{fma(beta, cd.x, -cz.x), fma(beta, cd.y, -cz.y)};
        __syncthreads();
        if (own) {
          // the same entries in the same order, the batch of kRunGB and chunks of 8 padded with zero weights as on the
          // other path; a padded term reads s_N[t] (slot 0, always written: the list holds the own poses) where the other
          // path reads element t of column 0 -- either way 0 * a finite value added to the sum
          static_assert(kColGB == kRunGB, "the batch kept in registers is the other gather's batch");
          const double *__restrict__ sN0 = reinterpret_cast<const double *>(s_N), *__restrict__ sN = sN0 + t;
#pragma unroll
          for (int q = 0; q < kRunGB; ++q) accw = fma(wq[q], sN0[nq[q]], accw);
          for (int p = myb + kRunGB; p < mye; p += 8) {
            double n8[8], w8[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
              const bool ok = p + q < mye;
              w8[q] = ok ? s_v[p + q] : 0.0;
              n8[q] = sN[(ok ? s_ci[p + q] : 0) * r];
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) accw = fma(w8[q], n8[q], accw);
          }
        }
      } else {
        double ga[kRunGB], gz[kRunGB];
        if (own) {
#pragma unroll
          for (int q = 0; q < kRunGB; ++q) {
            const bool ok = myb + q < mye;
            const size_t oo = ok ? (size_t)s_ci[myb + q] * r + t : 0;
            gz[q] = ld_coh(a.z + oo);
            ga[q] = (iter > 0) ? ld_coh(d_old + oo) : 0.0;
          }
        }
        direction();
        if (own) {
#pragma unroll
          for (int q = 0; q < kRunGB; ++q) {
            const double w = (myb + q < mye) ? s_v[myb + q] : 0.0;  // (the weights come from LDS when they are used)
            accw = fma(w, fma(beta, ga[q], -gz[q]), accw);
          }
          for (int p = myb + kRunGB; p < mye; p += 8) {
            double a8[8], b8[8], w8[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
              const bool ok = p + q < mye;
              const size_t oo = ok ? (size_t)s_ci[p + q] * r + t : 0;
              w8[q] = ok ? s_v[p + q] : 0.0;
              b8[q] = ld_coh(a.z + oo);
              a8[q] = (iter > 0) ? ld_coh(d_old + oo) : 0.0;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) accw = fma(w8[q], fma(beta, a8[q], -b8[q]), accw);
          }
        }
      }
      if (own) {
        dn = (iter > 0) ? beta * o_d - z_own : -z_own;
        st_coh(d_new + oown, dn);
        o_d = dn;
        s_W[e] = accw;
        s_D[e] = dn;
      }
      __syncthreads();
      if (wave == 0) {
        Row<D> V, W;
#pragma unroll
        for (int aa = 0; aa < DH; ++aa) {
          W.e[aa] = pact ? s_W[(g * DH + aa) * r + tt] : 0.0;
          V.e[aa] = pact ? s_D[(g * DH + aa) * r + tt] : 0.0;
        }
        row_sub_AS<D>(W, V, S);
        row_tangent<D>(Y, W);
        if (pact)
#pragma unroll
          for (int aa = 0; aa < DH; ++aa) {
            st_coh(a.Hd + o + aa * r + tt, W.e[aa]);
            s_H[(g * DH + aa) * r + tt] = W.e[aa];
          }
        double dacc = 0;
#pragma unroll
        for (int aa = 0; aa < DH; ++aa) dacc += V.e[aa] * W.e[aa];
        if (!pact) dacc = 0;
        const double rs = row16_sum_dpp(dacc);  // the 16-lane row sum k_fused_hess's block sum starts from
        if (lane == 0) st_coh(a.p1r + blockIdx.x, rs);
      }
    }
    RUN_STAMP(sb0 + 1);
    if (!run_grid_step(a.sync, gstep++, &s_ok)) return give_up();  // (its barriers also order s_H for the read below)
    RUN_STAMP(sb0 + 2);
    // ======== PC: step length, updates, z = Proj_X(res Minv), stopping rules ========
    // the row sums of <delta, H delta> are requested ahead of the all-gather of H delta: loads return in the order of
    // their requests, so d_Hd, alpha, the boundary test and the own updates are done while the all-gather is still
    // landing, and its pieces go into the image in ascending u as they arrive
    constexpr int rows_per = fused_pb(R, DH) / 2;  // rows of a k_fused_hess workgroup at this r: 8, 6, 5
    static_assert(rows_per <= 8, "the row sums of one k_fused_hess workgroup are loaded as 8 values");
    const int nrows = gridDim.x, nblk = (nrows + rows_per - 1) / rows_per;
    double rs16[16];
    {
      const int b0 = min(lane, nblk - 1) * rows_per;  // (lanes beyond the partials load the last one's and drop it)
#pragma unroll
      for (int ri = 0; ri < 16; ++ri) rs16[ri] = (ri < rows_per && b0 + ri < nrows) ? ld_coh(a.p1r + b0 + ri) : 0.0;
    }
    __builtin_amdgcn_sched_barrier(0);  // (nothing of the all-gather is requested ahead of the row sums)
    double2 xh[kImgPieces];
#pragma unroll
    for (int u = 0; u < kImgPieces; ++u) xh[u] = pc_ld16_coh(rs_h, voff_t, (unsigned)u * kPcBlock * 16u);
    __builtin_amdgcn_sched_barrier(0);
    if (own) o_h = s_H[e];
    double d_Hd;
    {
      // k_fused_hess's partial of workgroup w: rows 2 w' .. of its pbA poses, wave by wave; then the wave sum over them
      double part = 0;
      if (lane < nblk) {
        double wsum[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) wsum[w] = (rs16[4 * w] + rs16[4 * w + 1]) + (rs16[4 * w + 2] + rs16[4 * w + 3]);
        double tsum = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) tsum += wsum[w];
        part = tsum;
      }
      d_Hd = wave_sum(part);
    }
    const double c_zr = zr, c_dPd = dPd, c_ePe = ePe, c_ePd = ePd;
    alpha = tcg_alpha(c_zr, d_Hd);
    const double e_Pe_new = tcg_e_Pe_new(alpha, c_dPd, c_ePe, c_ePd);
    const bool boundary = tcg_boundary(d_Hd, e_Pe_new, c_Delta);
    const double step = boundary ? tcg_tau(c_dPd, c_ePe, c_ePd, c_Delta) : alpha;
    ePen = e_Pe_new;
    if (own) {
      o_eta = o_eta + step * o_d;
      o_Heta = o_Heta + step * o_h;
    }
    if (boundary) {
      status = tcg_boundary_status(d_Hd);
      iters_done = iter + 1;
      finish();
      return;
    }
    if (own) {
      const double rr = fma(alpha, o_h, o_r);
      o_r = rr;
      s_R[lc * RM + t] = rr;
    }
    RUN_STAMP(sb0 + 3);
    // res += alpha H delta, kImgGroup pieces at a time without a branch among them: the LDS reads of a group are in
    // flight together (piece by piece, each behind a test of its own, the update was one LDS round trip per piece).  A
    // thread whose pair lies beyond the residual goes through the spare pair behind the image and adds nothing
    nrm2 = 0;
    if constexpr (kImgGroup == 1) {  // (r = 6: no registers for a group; the pieces one by one, as ever)
#pragma unroll
      for (int u = 0; u < kImgPieces; ++u) {
        const int i = u * kPcBlock + (int)threadIdx.x;
        if (i < npair) {
          double2 x = *img_pair(i);
          x.x = fma(alpha, xh[u].x, x.x);
          x.y = fma(alpha, xh[u].y, x.y);
          nrm2 = fma(x.x, x.x, nrm2);
          nrm2 = fma(x.y, x.y, nrm2);
          *img_pair(i) = x;
        }
      }
    } else {
#pragma unroll
      for (int u0 = 0; u0 < kImgPieces; u0 += kImgGroup) {
        if (u0 * kPcBlock < npair) {
          double2 *pp[kImgGroup];
          double2 x[kImgGroup];
#pragma unroll
          for (int j = 0; j < kImgGroup; ++j) {
            const int i = (u0 + j) * kPcBlock + (int)threadIdx.x;
            pp[j] = i < npair ? img_pair(i) : img_pair(cpad * r / 2);
            x[j] = *pp[j];
          }
          __builtin_amdgcn_sched_barrier(0);  // (every read of the group is requested before the first is waited for)
#pragma unroll
          for (int j = 0; j < kImgGroup; ++j) {
            x[j].x = fma(alpha, xh[u0 + j].x, x[j].x);
            x[j].y = fma(alpha, xh[u0 + j].y, x[j].y);
            const double n2 = fma(x[j].y, x[j].y, fma(x[j].x, x[j].x, nrm2));
            nrm2 = (u0 + j) * kPcBlock + (int)threadIdx.x < npair ? n2 : nrm2;
          }
#pragma unroll
          for (int j = 0; j < kImgGroup; ++j) *pp[j] = x[j];
        }
      }
    }
    __syncthreads();
    RUN_STAMP(sb0 + 4);
    product(sb0 + 5);
    {
      if (tcg_residual_done(sqrt(s_Z[NR * RM]), n0)) {
        status = tcg_residual_status(n0);
        iters_done = iter + 1;
        finish();
        return;
      }
    }
    project_z();
    if (iter + 1 >= c_max_inner) {  // inner loop exhausted: status stays TR_MAXITER
      iters_done = iter + 1;
      finish();
      return;
    }
    RUN_STAMP(sb0 + 8);
    if (!run_grid_step(a.sync, gstep++, &s_ok)) return give_up();
    RUN_STAMP(sb0 + 9);
  }
}

// test entry (dcora_debug_wg_sums): ONE workgroup sums NV values per logical lane (in[i * kPcBlock + wave * 64 + L])
// with wg_row_sums and with row16_sum_dpp; out: per form (the reduce-scatter first) the NV x 16 row sums as k_tcg_run
// keeps them in LDS, then the NV totals of its serial add
template <int NV>
__global__ __launch_bounds__(kPcBlock) void k_debug_wg_sums(const double *__restrict__ in, double *__restrict__ out) {
  __shared__ double s_P[NV][4 * kPcNW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double v[NV];
#pragma unroll
  for (int form = 0; form < 2; ++form) {
    const int src = wave * 64 + (form == 0 ? wg_sums_logical_lane(lane) : lane);
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = in[(size_t)i * kPcBlock + src];
    if (form == 0) {
      wg_row_sums<NV>(v, s_P, wave, lane);
    } else {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const double s = row16_sum_dpp(v[i]);
        if ((lane & 15) == 0) s_P[i][wave * 4 + (lane >> 4)] = s;
      }
    }
    __syncthreads();
    double *__restrict__ o = out + (size_t)form * NV * (4 * kPcNW + 1);
    if ((int)threadIdx.x < NV) {
      double t = 0;
#pragma unroll
      for (int w = 0; w < 4 * kPcNW; ++w) {
        t += s_P[threadIdx.x][w];
        o[threadIdx.x * 4 * kPcNW + w] = s_P[threadIdx.x][w];
      }
      o[NV * 4 * kPcNW + threadIdx.x] = t;
    }
    __syncthreads();
  }
}

}  // namespace

// ---- the one-launch tCG run ------------------------------------------------------------------------------
int tcg_run_sync_words() { return kRunSyncWords; }
int tcg_run_col_cap() { return kRunColCap; }
std::atomic<int> g_tcg_run_fault{0};
std::atomic<int> g_tcg_run_fault_skip{0};
int tcg_run_max_rows_nnz(const ManiDesc &m, const int *rp) {
  const int dh = m.d + 1;
  int worst = 0;
  for (int p0 = 0; p0 < m.n; p0 += 2) {
    const int j0 = p0 * dh, j1 = std::min(m.n, p0 + 2) * dh;
    worst = std::max(worst, rp[j1] - rp[j0]);
  }
  return worst;
}
bool tcg_run_supported(const ManiDesc &m, int ldm, int cus, int max_rows_nnz) {
  if (!m.se || m.d != 3 || m.r < 4 || m.r > 6) return false;    // instantiated ranks; r = 4, 5, 6: fused_pb even
  if (fused_pb(m.r, m.d + 1) % 2 != 0) return false;               // row sums pair up with k_fused_hess's workgroups
  if (!fused_pc_preferred(m, ldm) || fused_pc_pb(m) != 2) return false;
  const int grid = (m.n + 1) / 2;
  if (grid > cus || grid > 256) return false;                      // co-resident, <z, r> partials in one wave load
  if (m.k > kRunNS * kPcNW * 128) return false;                    // the rows of the inverse fit the registers
  const int rows_per = fused_pb(m.r, m.d + 1) / 2;
  if ((grid + rows_per - 1) / rows_per > 64) return false;         // <delta, H delta> partials in one wave
  return max_rows_nnz <= kRunQCap;
}
template <int R, bool COLS>
static int tcg_run_launch(hipStream_t st, const TcgRunArgs &a) {
  static LdsGrant grant;
  const int cpad = ((a.m.k + 127) / 128) * 128;
  const size_t lds = run_img_bytes(R, cpad);
  if (!grant.granted(reinterpret_cast<const void *>(&k_tcg_run<3, R, kRunNS, COLS>), lds, 40 * 1024)) return -1;
  const int grid = (a.m.n + 1) / 2;
  hipLaunchKernelGGL((k_tcg_run<3, R, kRunNS, COLS>), dim3(grid), dim3(kPcBlock), lds, st, a);
  if (hipGetLastError() != hipSuccess) return -1;
  return grid;
}
int launch_tcg_run(hipStream_t st, const TcgOperands &o, int seq) {
  count_launch();
  int fault = 0;
  bool skipped = false;
  for (int sk = g_tcg_run_fault_skip.load(); sk > 0;)
    if (g_tcg_run_fault_skip.compare_exchange_weak(sk, sk - 1)) {
      skipped = true;
      break;
    }
  for (int left = skipped ? 0 : g_tcg_run_fault.load(); left > 0;)
    if (g_tcg_run_fault.compare_exchange_weak(left, left - 1)) {
      fault = 1;
      break;
    }
  const ManiDesc &m = o.m;
  TcgRunArgs a{m, o.ldm, o.Minv, o.Q, o.grad, o.X, o.S, o.d[0], o.d[1], o.Hd, o.eta, o.Heta, o.z, o.p1, o.p3, o.pC,
               o.sync, o.ctl, o.hf, seq, fault, o.cols};
#ifdef DCORA_RUN_STAMPS
  {
    // a ring of stamp blocks: launch c writes block c % kRing, and the host reads a block when it comes round again,
    // kRing launches later (it enqueues ahead of the device: with one block it wiped the stamps of a run in flight,
    // and which stamps it wiped depended on the build)
    constexpr int kRing = 16;
    static long long *ring = nullptr;
    if (!ring && hipHostMalloc((void **)&ring, kRing * 64 * sizeof(long long), hipHostMallocMapped) == hipSuccess)
      for (int i = 0; i < kRing * 64; ++i) ring[i] = 0;
    static int count = 0;
    long long *buf = ring ? ring + (size_t)(count % kRing) * 64 : nullptr;
    if (buf && count >= kRing) {  // the stamps of the run kRing launches back
      static double acc[64];
      static int n = 0;
      long long s0 = buf[0];
      constexpr int kShown = kRunStamp0 + 4 * kRunStampsPerIter;
      bool whole = s0 > 0;
      for (int i = 1; i < kShown; ++i) whole = whole && buf[i] >= buf[i - 1];
      if (whole) {
        for (int i = 0; i < kShown; ++i) acc[i] += (double)(buf[i] - s0) * 0.01;
        ++n;
      }
      for (int i = 0; i < 64; ++i) buf[i] = 0;
      if (n == 500) {
        fprintf(stderr, "k_tcg_run stamps (us from start, workgroup 0, mean of %d runs that went past their fourth iteration):", n);
        for (int i = 0; i < kShown; ++i) fprintf(stderr, " %.2f", acc[i] / n);
        fprintf(stderr, "\n");
        n = -1000000;
      }
    }
    ++count;
    a.stamps = buf;
  }
#endif
  const bool cols = a.cols.lp != nullptr;
  if (m.r == 4) return cols ? tcg_run_launch<4, true>(st, a) : tcg_run_launch<4, false>(st, a);
  if (m.r == 5) return cols ? tcg_run_launch<5, true>(st, a) : tcg_run_launch<5, false>(st, a);
  if (m.r == 6) return cols ? tcg_run_launch<6, true>(st, a) : tcg_run_launch<6, false>(st, a);
  return -1;
}
int launch_debug_wg_sums(hipStream_t st, int nv, const double *in, double *out) {
  if (nv == 33) hipLaunchKernelGGL((k_debug_wg_sums<33>), dim3(1), dim3(kPcBlock), 0, st, in, out);
  else if (nv == 41) hipLaunchKernelGGL((k_debug_wg_sums<41>), dim3(1), dim3(kPcBlock), 0, st, in, out);
  else if (nv == 49) hipLaunchKernelGGL((k_debug_wg_sums<49>), dim3(1), dim3(kPcBlock), 0, st, in, out);
  else return -1;
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
int tcg_run_image_map(int r, int k, int *off, int *lanes) {
  if (r < 4 || r > 6 || k < 1 || k > kRunNS * kPcNW * 128) return -1;
  const int cpad = ((k + 127) / 128) * 128;
  for (int i = 0; i < cpad * r / 2; ++i) off[i] = run_img_off(i);
  for (int p = 0; p < 64; ++p) lanes[p] = wg_sums_logical_lane(p);
  return (int)run_img_bytes(r, cpad);
}

}  // namespace dcora
