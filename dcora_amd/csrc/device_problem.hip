// DeviceProblem: QuadraticProblem / QuadraticOptimizer on the MI355X (see device_problem.h).
#include <atomic>

#include "device_problem.h"
#include "column_slots.h"
#include "env.h"
#include "escape_rule.h"
#include "device_chol.h"
#include "host_threads.h"
#include "precond_cache.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

namespace dcora {

static thread_local std::string g_last_error;
void set_last_error(const std::string &s) { g_last_error = s; }
const std::string &get_last_error() { return g_last_error; }
int hip_fail(hipError_t e, const char *what, const char *file, int line) {
  char buf[512];
  std::snprintf(buf, sizeof buf, "HIP error %d (%s) at %s:%d in %s", (int)e, hipGetErrorString(e), file, line, what);
  set_last_error(buf);
  return (e == hipErrorNoDevice || e == hipErrorInvalidDevice) ? DCORA_ERR_NO_DEVICE : DCORA_ERR_HIP;
}

int DevCsr::upload(int nr, int nc, const int *rph, const int *cih, const double *vh) {
  nrows = nr;
  ncols = nc;
  nnz = rph[nr];
  DCORA_HIP(rp.alloc(nr + 1));
  DCORA_HIP(ci.alloc(std::max(nnz, 1)));
  DCORA_HIP(v.alloc(std::max(nnz, 1)));
  DCORA_HIP(hipMemcpy(rp.p, rph, sizeof(int) * (nr + 1), hipMemcpyHostToDevice));
  if (nnz) {
    DCORA_HIP(hipMemcpy(ci.p, cih, sizeof(int) * nnz, hipMemcpyHostToDevice));
    DCORA_HIP(hipMemcpy(v.p, vh, sizeof(double) * nnz, hipMemcpyHostToDevice));
  }
  std::vector<int> lr;
  for (int i = 0; i < nr; ++i)
    if (rph[i + 1] - rph[i] > kLongRow) lr.push_back(i);
  n_long = (int)lr.size();
  if (n_long > kMaxPartials / 2) {  // not a hub structure any more: let the row-parallel path handle everything
    n_long = 0;
    lr.clear();
  }
  long_host = lr;
  DCORA_HIP(long_rows.alloc(std::max(n_long, 1)));
  if (n_long) DCORA_HIP(hipMemcpy(long_rows.p, lr.data(), sizeof(int) * n_long, hipMemcpyHostToDevice));
  DCORA_HIP(long_part.alloc((size_t)std::max(n_long, 1) * kLongSplit * 16));
  DCORA_HIP(long_cnt.alloc(std::max(n_long, 1)));
  DCORA_HIP(hipMemset(long_cnt.p, 0, sizeof(int) * std::max(n_long, 1)));
  return DCORA_OK;
}
int DevBsr::upload(const HostBsr &B) {
  nbrows = B.nbrows;
  nblocks = B.nblocks();
  DCORA_HIP(bp.alloc(nbrows + 1));
  DCORA_HIP(bc.alloc(std::max(nblocks, 1)));
  DCORA_HIP(bv.alloc(std::max<size_t>(B.bv.size(), 1)));
  DCORA_HIP(hipMemcpy(bp.p, B.bp.data(), sizeof(int) * (nbrows + 1), hipMemcpyHostToDevice));
  if (nblocks) {
    DCORA_HIP(hipMemcpy(bc.p, B.bc.data(), sizeof(int) * nblocks, hipMemcpyHostToDevice));
    DCORA_HIP(hipMemcpy(bv.p, B.bv.data(), sizeof(double) * B.bv.size(), hipMemcpyHostToDevice));
  }
  return DCORA_OK;
}
int DevCsr::upload(const HostCsr &A) { return upload(A.n, A.ncols, A.rp.data(), A.ci.data(), A.v.data()); }
int DevCsr::download(HostCsr *A) const {
  A->n = nrows;
  A->ncols = ncols;
  A->rp.resize((size_t)nrows + 1);
  A->ci.resize((size_t)nnz);
  A->v.resize((size_t)nnz);
  DCORA_HIP(hipMemcpy(A->rp.data(), rp.p, sizeof(int) * ((size_t)nrows + 1), hipMemcpyDeviceToHost));
  if (nnz) {
    DCORA_HIP(hipMemcpy(A->ci.data(), ci.p, sizeof(int) * (size_t)nnz, hipMemcpyDeviceToHost));
    DCORA_HIP(hipMemcpy(A->v.data(), v.p, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToHost));
  }
  return DCORA_OK;
}
int DevCsr::set_values(const HostCsr &A, hipStream_t st) {
  if (A.n != nrows || A.ncols != ncols || A.nnz() != nnz || (int)A.v.size() != nnz) {
    set_last_error("set_values: the matrix does not have the uploaded pattern");
    return DCORA_ERR_BAD_ARG;
  }
  if (nnz) DCORA_HIP(hipMemcpyAsync(v.p, A.v.data(), sizeof(double) * nnz, hipMemcpyHostToDevice, st));
  return DCORA_OK;
}

// HostFlags words live in one host-mapped page per process, handed out slot by slot: hipHostMalloc per problem cost
// more than the rest of a cached creation
namespace {
constexpr int kFlagSlots = 1024;
constexpr size_t kFlagStride = 64;  // one line per problem: the words are written over PCIe by different streams
static_assert(sizeof(HostFlags) <= kFlagStride, "HostFlags slot");
std::mutex g_flag_mu;
HostFlags *g_flag_host = nullptr, *g_flag_dev = nullptr;
std::vector<int> g_flag_free;
}  // namespace
// HIP streams are recycled too: hipStreamCreateWithFlags took 1.7-8.5 ms of a 2-9 ms cached problem creation
// (DCORA_INIT_TIMING), hipStreamDestroy another 1-2 ms.  Idle non-blocking streams are kept per device.
namespace {
std::mutex g_stream_mu;
std::vector<std::pair<int, hipStream_t>> g_idle_streams;
}  // namespace
int stream_acquire(int device, hipStream_t *out) {
  {
    std::lock_guard<std::mutex> lk(g_stream_mu);
    for (size_t i = 0; i < g_idle_streams.size(); ++i)
      if (g_idle_streams[i].first == device) {
        *out = g_idle_streams[i].second;
        g_idle_streams.erase(g_idle_streams.begin() + (long)i);
        return DCORA_OK;
      }
  }
  DCORA_HIP(hipStreamCreateWithFlags(out, hipStreamNonBlocking));
  return DCORA_OK;
}
void stream_release(int device, hipStream_t st) {
  if (!st) return;
  (void)hipStreamSynchronize(st);
  std::lock_guard<std::mutex> lk(g_stream_mu);
  if (g_idle_streams.size() < 256) {
    g_idle_streams.emplace_back(device, st);
    return;
  }
  (void)hipStreamDestroy(st);
}

int host_flags_acquire(HostFlags **host, HostFlags **dev, int *slot) {
  std::lock_guard<std::mutex> lk(g_flag_mu);
  if (!g_flag_host) {
    DCORA_HIP(hipHostMalloc((void **)&g_flag_host, kFlagStride * kFlagSlots, hipHostMallocMapped | hipHostMallocPortable));
    std::memset((void *)g_flag_host, 0, kFlagStride * kFlagSlots);
    DCORA_HIP(hipHostGetDevicePointer((void **)&g_flag_dev, (void *)g_flag_host, 0));
    for (int i = kFlagSlots - 1; i >= 0; --i) g_flag_free.push_back(i);
  }
  if (g_flag_free.empty()) {  // more live problems than slots: a page of its own
    DCORA_HIP(hipHostMalloc((void **)host, sizeof(HostFlags), hipHostMallocMapped | hipHostMallocPortable));
    std::memset((void *)*host, 0, sizeof(HostFlags));
    DCORA_HIP(hipHostGetDevicePointer((void **)dev, (void *)*host, 0));
    *slot = -1;
    return DCORA_OK;
  }
  *slot = g_flag_free.back();
  g_flag_free.pop_back();
  *host = (HostFlags *)((char *)g_flag_host + kFlagStride * (size_t)*slot);
  *dev = (HostFlags *)((char *)g_flag_dev + kFlagStride * (size_t)*slot);
  std::memset((void *)*host, 0, sizeof(HostFlags));
  return DCORA_OK;
}
void host_flags_release(HostFlags *host, int slot) {
  if (!host) return;
  if (slot < 0) {
    (void)hipHostFree((void *)host);
    return;
  }
  std::lock_guard<std::mutex> lk(g_flag_mu);
  g_flag_free.push_back(slot);
}

DeviceProblem::~DeviceProblem() {
  if (st) (void)hipStreamSynchronize(st);  // nothing of this problem is in flight when its flag words are recycled
  for (hipEvent_t e : run_events) (void)hipEventDestroy(e);
  host_flags_release(hf, hf_slot);
  if (own_stream && st) stream_release(device, st);
}

int DeviceProblem::upload(const double *h, double *d, size_t n) {
  DCORA_HIP(hipMemcpyAsync(d, h, n * sizeof(double), hipMemcpyHostToDevice, st));
  return DCORA_OK;
}
int DeviceProblem::download(const double *d, double *h, size_t n) {
  DCORA_HIP(hipMemcpyAsync(h, d, n * sizeof(double), hipMemcpyDeviceToHost, st));
  DCORA_HIP(hipStreamSynchronize(st));
  return DCORA_OK;
}

// (the fused Hessian kernel stages the first matrix tile with clamped, unconditional loads: it needs nnz > 0)
static bool fused_eligible(const ManiDesc &mm, int nnz) {
  return fused_supported(mm) && nnz > 0 && !env::generic_solver();
}

int DeviceProblem::init(const dcora_dims &dims, const HostCsr &Qh, const double *Gh, double reg, int device_,
                        hipStream_t shared) {
  if (dims.r < 1 || dims.r > 16 || (dims.d != 2 && dims.d != 3) || dims.n < 0 || dims.l < 0 || dims.b < 0) {
    set_last_error("bad dims (need 1 <= r <= 16, d in {2,3})");
    return DCORA_ERR_BAD_ARG;
  }
  const bool init_timing = env::init_timing();
  const auto ti0 = std::chrono::steady_clock::now();
  auto lap = [&](const char *what) {
    if (init_timing)
      std::fprintf(stderr, "[init] %-12s %.3f ms\n", what,
                   std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ti0).count());
  };
  m = make_mani(dims);
  if (Qh.n != m.k) {
    set_last_error("Q dimension does not match (d+1) n + l + b");
    return DCORA_ERR_BAD_ARG;
  }
  device = device_;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    set_last_error("no HIP device available: libdcora_hip has no CPU fallback");
    return DCORA_ERR_NO_DEVICE;
  }
  DCORA_HIP(hipSetDevice(device));
  if (shared) {
    st = shared;
    own_stream = false;
  } else {
    const int rcs = stream_acquire(device, &st);
    if (rcs) return rcs;
    own_stream = true;
  }
  lap("stream");
  int rc = Q.upload(Qh);
  if (rc) return rc;
  lap("Q upload");
  // block form of Q for graphs large enough to be bandwidth-bound (the scalar-CSR kernel exposes more parallelism
  // and wins while the launch is latency-bound)
  const bool want_bsr = m.n >= 8192;
  if (m.se && m.r <= 8 && m.n > 0 && want_bsr && !env::generic_solver()) {
    rc = Qb.upload(bsr_from_csr(Qh, m.d + 1));
    if (rc) return rc;
    has_bsr = true;
  }
  fused = fused_eligible(m, Q.nnz);
  group = group_supported(m) && !env::generic_solver();
  run_rows_nnz_ = m.se ? tcg_run_max_rows_nnz(m, Qh.rp.data()) : 0;
  gather_columns_ = env::gather_columns();
  {
    const std::vector<WsSlot> plan = ws_plan(m, fused);
    DevBuf<double> fresh;
    rc = ws_build(plan, &fresh);
    if (rc) return rc;
    ws_adopt(plan, std::move(fresh));
  }
  DCORA_HIP(ctl.alloc(1));
  {
    const int rc2 = host_flags_acquire(&hf, &hf_dev, &hf_slot);
    if (rc2) return rc2;
  }
  DCORA_HIP(hipStreamSynchronize(st));  // the zeroed workspace is visible to every stream before the first upload
  lap("workspace");
  if (Gh) {
    rc = set_G_host(Gh);
    if (rc) return rc;
  }
  if (reg >= 0) {
    rc = build_preconditioner(Qh, reg);
    if (rc) return rc;
  }
  lap("precond");
  rc = run_form(m, fused, has_bsr, &tcg_run_ok, &tcg_sync);
  if (rc || !tcg_run_ok) return rc;
  RunColsBuilt cols;
  rc = build_run_cols(Qh.rp.data(), Qh.ci.data(), Qh.nnz(), &cols);
  if (!rc) adopt_run_cols(std::move(cols));
  return rc;
}

// One allocation for the whole solver workspace, zeroed by one memset: the reference re-creates its problem on
// every Agent::updateX (ref src/Agent.cpp:1252), so creation must cost a fraction of a solve -- thirty hipMalloc
// and ten synchronous hipMemset calls took 4-8 ms.
std::vector<DeviceProblem::WsSlot> DeviceProblem::ws_plan(const ManiDesc &mm, bool fused_) {
  const size_t N = (size_t)mm.r * mm.k;
  const size_t NS = (size_t)mm.n * mm.d * mm.d + mm.l + 1;
  std::vector<WsSlot> slots;
  for (DevBuf<double> *b : {&G, &X0, &X1, &EG0, &EG1, &RG0, &RG1, &delta, &eta, &Heta, &res, &z, &Hd, &W, &Zt})
    slots.push_back({b, N});
  slots.push_back({&delta2, N});
  if (fused_) {
    slots.push_back({&res2, N});
    slots.push_back({&Zpart, (size_t)fused_nsplit(mm) * N});  // slice 0 doubles as Z of the sparse preconditioner
  }
  slots.push_back({&S0, NS});
  slots.push_back({&S1, NS});
  // 2 doubles per slot; the Q-apply may add up to kMaxPartials / 2 long-row blocks to its kMaxPartials row blocks
  for (DevBuf<double> *b : {&pB, &pC, &p1, &p2, &p3}) slots.push_back({b, (size_t)4 * kMaxPartials});
  slots.push_back({&pA, 2 * (size_t)kBsrMaxGrid});  // the block-CSR Q-apply runs up to kBsrMaxGrid workgroups
  slots.push_back({&scal, 64});
  return slots;
}
static size_t ws_pad(size_t n) { return (n + 31) & ~(size_t)31; }  // 256-byte aligned slices
int DeviceProblem::ws_build(const std::vector<WsSlot> &plan, DevBuf<double> *arena_new) {
  size_t total = 0;
  for (const WsSlot &sl : plan) total += ws_pad(sl.n);
  DCORA_HIP(arena_new->alloc(total));
  DCORA_HIP(hipMemsetAsync(arena_new->p, 0, total * sizeof(double), st));
  return DCORA_OK;
}
void DeviceProblem::ws_adopt(const std::vector<WsSlot> &plan, DevBuf<double> &&arena_new) {
  for (DevBuf<double> *b : {&res2, &Zpart}) b->release();  // (not in every plan)
  arena = std::move(arena_new);
  size_t off = 0;
  for (const WsSlot &sl : plan) {
    sl.b->borrow(arena.p + off, sl.n);
    off += ws_pad(sl.n);
  }
}

// the column-slot map of the one-launch run's tiling (init and rerank build it where the run form applies: SE layout,
// d = 3, at most 256 workgroups of 2 poses)
int DeviceProblem::build_run_cols(const int *rp, const int *ci, int nnz, RunColsBuilt *out) const {
  if (!m.se || m.d != 3 || m.n < 1 || (m.n + 1) / 2 > 256 || nnz == 0 || !gather_columns_) return DCORA_OK;
  const ColumnSlots cs = column_slots(rp, ci, m.n, m.d + 1, 2, tcg_run_col_cap());
  std::vector<int> img;
  img.reserve(cs.lp.size() + cs.list.size() + cs.slot.size());
  img.insert(img.end(), cs.lp.begin(), cs.lp.end());
  img.insert(img.end(), cs.list.begin(), cs.list.end());
  for (uint16_t sl : cs.slot) img.push_back((int)sl);
  DCORA_HIP(out->img.alloc(img.size()));
  DCORA_HIP(hipMemcpy(out->img.p, img.data(), sizeof(int) * img.size(), hipMemcpyHostToDevice));
  out->nwg = cs.nwg;
  out->nlist = (int)cs.list.size();
  out->overflow = cs.n_overflow;
  out->max = cs.max_count;
  return DCORA_OK;
}
void DeviceProblem::adopt_run_cols(RunColsBuilt &&b) {
  run_cols = std::move(b.img);
  run_cols_nwg = b.nwg;
  run_cols_nlist = b.nlist;
  run_cols_overflow = b.overflow;
  run_cols_max = b.max;
}

// the one-launch tCG run: dense inverse, the whole residual in one LDS image, n / 2 workgroups co-resident
int DeviceProblem::run_form(const ManiDesc &mm, bool fused_, bool has_bsr_, bool *ok, DevBuf<unsigned> *sync) {
  *ok = false;
  if (!(fused_ && has_precond && !sparse_precond && !has_bsr_ && Q.n_long == 0 && env::solver_tcg() >= 0))
    return DCORA_OK;
  if (cus_ == 0) {
    hipDeviceProp_t prop;
    DCORA_HIP(hipGetDeviceProperties(&prop, device));
    cus_ = prop.multiProcessorCount;
  }
  if (!tcg_run_supported(mm, ldm, cus_, run_rows_nnz_)) return DCORA_OK;
  DCORA_HIP(sync->alloc((size_t)tcg_run_sync_words()));
  DCORA_HIP(hipMemsetAsync(sync->p, 0, sizeof(unsigned) * (size_t)tcg_run_sync_words(), st));
  *ok = true;
  return DCORA_OK;
}

int DeviceProblem::rerank(int r_new) {
  if (r_new < 1 || r_new > 16) {
    set_last_error("rerank: need 1 <= r <= 16");
    return DCORA_ERR_BAD_ARG;
  }
  DCORA_HIP(hipSetDevice(device));
  if (pending_) {
    const int rc = fetch_result(nullptr);
    if (rc) return rc;
  }
  DCORA_HIP(hipStreamSynchronize(st));  // nothing in flight reads the workspace that goes
  ManiDesc mn = m;
  mn.r = r_new;
  const bool fused_n = fused_eligible(mn, Q.nnz);
  const bool group_n = group_supported(mn) && !env::generic_solver();
  const bool bsr_n = Qb.nbrows > 0 && r_new <= 8;  // (the block form was uploaded: every other condition of init held)
  // aside: the arena, the replay vectors of the sparse preconditioner, the counters of the one-launch tCG run
  const std::vector<WsSlot> plan = ws_plan(mn, fused_n);
  DevBuf<double> arena_n;
  int rc = ws_build(plan, &arena_n);
  if (rc) return rc;
  SparsePrecond sp_n;
  if (sparse_precond) {
    rc = sp_n.attach(sp.im, r_new);
    if (rc) return rc;
    DCORA_HIP(hipStreamSynchronize(nullptr));  // (its memsets run on the null stream)
  }
  bool run_n = false;
  DevBuf<unsigned> sync_n;
  rc = run_form(mn, fused_n, bsr_n, &run_n, &sync_n);
  if (rc) return rc;
  RunColsBuilt cols_n;  // the run form applies at this rank first: its map, from the pattern Q holds on the device
  if (run_n && !run_cols.p && gather_columns_) {
    std::vector<int> rp((size_t)Q.nrows + 1), ci((size_t)Q.nnz);
    DCORA_HIP(hipMemcpy(rp.data(), Q.rp.p, sizeof(int) * rp.size(), hipMemcpyDeviceToHost));
    if (Q.nnz) DCORA_HIP(hipMemcpy(ci.data(), Q.ci.p, sizeof(int) * ci.size(), hipMemcpyDeviceToHost));
    rc = build_run_cols(rp.data(), ci.data(), Q.nnz, &cols_n);
    if (rc) return rc;
  }
  DCORA_HIP(hipStreamSynchronize(st));  // the zeroed workspace is visible to every stream
  // the swap: nothing below fails
  m = mn;
  fused = fused_n;
  group = group_n;
  has_bsr = bsr_n;
  ws_adopt(plan, std::move(arena_n));
  if (sparse_precond) sp = std::move(sp_n);
  tcg_run_ok = run_n;
  tcg_sync = std::move(sync_n);
  if (cols_n.img.p) adopt_run_cols(std::move(cols_n));
  has_G = false;
  ride_X_ = nullptr;
  rgd_ = false;
  cur_after_fetch_ = 0;
  return DCORA_OK;
}

int DeviceProblem::set_values(const HostCsr &Q_on_pattern, hipStream_t stream, std::vector<double> *stage) {
  const int rc = Q.set_values(Q_on_pattern, stream);
  if (!rc) precond_stale = has_precond;
  if (rc || Qb.nbrows == 0) return rc;  // (the block form is kept current also while a rank above 8 leaves it unused)
  *stage = std::move(bsr_from_csr(Q_on_pattern, m.d + 1).bv);
  if (stage->size() != Qb.bv.n) {
    set_last_error("set_values: the matrix does not have the uploaded pattern");
    return DCORA_ERR_BAD_ARG;
  }
  DCORA_HIP(hipMemcpyAsync(Qb.bv.p, stage->data(), sizeof(double) * stage->size(), hipMemcpyHostToDevice, stream));
  return DCORA_OK;
}

int DeviceProblem::set_G_host(const double *Gh) {
  DCORA_HIP(hipSetDevice(device));
  if (Gh) {
    DCORA_HIP(hipMemcpy(G.p, Gh, (size_t)nelem() * sizeof(double), hipMemcpyHostToDevice));
    has_G = true;
  } else {
    DCORA_HIP(hipMemset(G.p, 0, (size_t)nelem() * sizeof(double)));
    has_G = false;
  }
  return DCORA_OK;
}

// The dense inverses of SEVERAL matrices (the agents of a session) built in one batch of launches and put into the cache,
// so that the problems created next attach to them: matrices of equal size whose inverse is not cached yet and that would
// take the dense form.  Best effort: whatever is not built here is built by the problem that needs it.
int precond_prebuild_dense(const std::vector<const HostCsr *> &Qs, double reg, int block, int device) {
  if (env::precond_mode() == 2 || env::factor_on_host() || env::precond_cache_mb() <= 0) return DCORA_OK;
  std::map<int, std::vector<size_t>> by_k;
  std::vector<PrecondKey> keys(Qs.size());
  for (size_t i = 0; i < Qs.size(); ++i) {
    const int k = Qs[i]->n;
    const bool want_sparse = env::precond_mode() ? false : (k > kDensePrecondMaxK);
    if (want_sparse || k < 1) continue;
    keys[i] = make_precond_key(*Qs[i], reg, block, device, false);
    PrecondEntry ent;
    if (precond_cache_find(keys[i], &ent, false)) continue;
    bool dup = false;  // (two agents with the same matrix: one build)
    for (size_t j : by_k[k]) dup = dup || keys[j] == keys[i];
    if (!dup) by_k[k].push_back(i);
  }
  DCORA_HIP(hipSetDevice(device));
  for (auto &grp : by_k) {
    const std::vector<size_t> &idx = grp.second;
    if (idx.size() < 2) continue;
    const auto t0 = std::chrono::steady_clock::now();
    const int k = grp.first, ldm = ((k + 127) / 128) * 128;
    std::vector<HostCsr> Ms(idx.size());
    std::vector<const HostCsr *> As;
    std::vector<std::shared_ptr<DevBuf<double>>> bufs;
    std::vector<double *> outs;
    std::vector<long> nnzL(idx.size(), 0);
    // host work per matrix (the shifted copy; nnz(L) of the SPARSE factor from the pattern, what SURVEY 8(d) prices the
    // preconditioner by) on threads of its own (t = 1 .. B), beside the device's batch (t = 0)
    for (size_t q = 0; q < idx.size(); ++q) Ms[q] = csr_shift_diag(*Qs[idx[q]], reg);
    std::vector<char> pd;
    int rc = DCORA_OK;
    auto batch = [&]() -> int {
      for (size_t q = 0; q < idx.size(); ++q) {
        auto buf = std::make_shared<DevBuf<double>>();
        DCORA_HIP(buf->alloc((size_t)k * ldm + 16));
        bufs.push_back(buf);
        outs.push_back(buf->p);
      }
      for (const HostCsr &M : Ms) As.push_back(&M);
      return device_dense_spd_inverse_batch(As, device, outs, ldm, &pd);
    };
    run_threads((int)idx.size() + 1, [&](int t) {
      if (t == 0) {
        rc = batch();
        return;
      }
      const size_t q = (size_t)t - 1;
      CholSymbolic sym;
      chol_symbolic(Ms[q], block, &sym);
      long nz = 0;
      for (const CholPiece &pc : sym.pieces) nz += (long)pc.c * (pc.c + 1) / 2 + (long)pc.m * pc.c;
      nnzL[q] = nz;
    });
    if (rc) return rc;
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (size_t q = 0; q < idx.size(); ++q) {
      if (!pd[q]) continue;  // not positive definite somewhere in the batch: the problems build (and report) one by one
      PrecondEntry ent;
      ent.ldm = ldm;
      ent.dense = bufs[q];
      ent.bytes = bufs[q]->n * sizeof(double);
      ent.build_ms = ms / (double)idx.size();
      ent.nnzL = nnzL[q];
      ent.prebuilt = true;
      precond_cache_insert(keys[idx[q]], ent);
    }
  }
  return DCORA_OK;
}

// (Q + reg I)^-1 as a dense symmetric matrix in HBM: host sparse Cholesky once per Q (Q is reused across all
// RBCD iterations and staircase levels), k independent solves on host threads, one upload.
int DeviceProblem::build_preconditioner(const HostCsr &Qh, double reg) {
  const auto t0 = std::chrono::steady_clock::now();
  const int k = m.k;
  // host threads of the set-up: what the process may really use (host_cpus_available), shared between the problems
  // that are being set up at the same time (the agents of a session are created side by side)
  static std::atomic<int> builders{0};
  struct Builder {
    std::atomic<int> &c;
    int active;
    explicit Builder(std::atomic<int> &c_) : c(c_), active(c_.fetch_add(1) + 1) {}
    ~Builder() { c.fetch_sub(1); }
  } builder(builders);
  const int nthreads = std::max(2, host_cpus_available() / std::max(1, builder.active));
  // Large blocks: partitioned sparse inverse replayed level by level (sparse_precond.h).  Small blocks: the dense
  // inverse streams faster than 2 * depth + 2 dependent launches.  DCORA_PRECOND=dense|sparse overrides.
  const bool want_sparse = env::precond_mode() ? env::precond_mode() == 2 : (k > kDensePrecondMaxK);
  const int block = m.se ? m.d + 1 : 1;
  if (want_sparse && m.r > 16) {
    set_last_error("sparse preconditioner supports r <= 16");
    return DCORA_ERR_UNSUPPORTED;
  }
  if (!want_sparse && (size_t)k > 60000) {
    set_last_error("dense preconditioner limited to k <= 60000");
    return DCORA_ERR_UNSUPPORTED;
  }
  // the inverse depends on Q + reg I only (not on r, not on G): built once per distinct matrix, shared afterwards
  const PrecondKey key = make_precond_key(Qh, reg, block, device, want_sparse);
  PrecondEntry ent;
  const bool found = precond_cache_find(key, &ent);
  precond_cache_hit = found && !ent.prebuilt;  // (an image built ahead for THIS problem is not a hit)
  DCORA_HIP(hipSetDevice(device));
  if (!found) {
    if (env::init_timing())
      fprintf(stderr, "[precond] key + cache look-up %.1f ms\n",
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    HostCsr M = csr_shift_diag(Qh, reg);
    if (want_sparse) {
      PartInvHost P;
      // the stored weights are formed on the device, or stream there while the host's threads form them
      DeviceWeightSink sink(device);
      P.sink = &sink;
      const int brc = build_partitioned_inverse_auto(M, block, nthreads, device, &P);
      if (brc && brc != DCORA_ERR_NOT_PD) return brc;
      const bool ok = brc == DCORA_OK;
      if (!ok) {
        set_last_error("preconditioner: Q + reg I is not positive definite");
        return DCORA_ERR_NOT_PD;
      }
      auto img = std::make_shared<SpImage>();
      const auto tu = std::chrono::steady_clock::now();
      const int rc = img->upload(P, P.sink ? &sink : nullptr);
      if (rc) return rc;
      if (env::init_timing())
        fprintf(stderr, "[precond] image upload %.1f ms (since start %.1f ms)\n",
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tu).count(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
      if (env::init_timing())
        fprintf(stderr, "[precond] host image: %.1f MB wave records, %.1f MB indices, %.1f MB weights\n",
                P.mwaves.size() * sizeof(MWave) / 1e6, P.idxs.size() * 4 / 1e6, P.vals.size() * 8 / 1e6);
      ent.sparse = img;
      ent.nnzL = P.nnzL;
      ent.bytes = img->device_bytes();
    } else {
      // rows padded so every 16-byte column-pair load of a 128-column chunk is in bounds
      ent.ldm = ((k + 127) / 128) * 128;
      auto buf = std::make_shared<DevBuf<double>>();
      DCORA_HIP(buf->alloc((size_t)k * ent.ldm + 16));
      const bool host_factor = env::factor_on_host();
      if (host_factor) {  // A/B measurements: sparse Cholesky and k solves on host threads, one upload
        SparseChol chol;
        if (!chol.factor(M, block)) {
          set_last_error("preconditioner: Q + reg I is not positive definite");
          return DCORA_ERR_NOT_PD;
        }
        ent.nnzL = chol.nnzL();
        std::vector<double> inv((size_t)k * ent.ldm, 0.0);
        chol.dense_inverse(inv.data(), (size_t)ent.ldm, nthreads);
        DCORA_HIP(hipMemcpy(buf->p, inv.data(), (size_t)k * ent.ldm * sizeof(double), hipMemcpyHostToDevice));
      } else {  // dense LL^T, L^-1 and L^-T L^-1 on the device (device_chol.h)
        bool pd = false;
        const int rc = device_dense_spd_inverse(M, device, buf->p, ent.ldm, &pd);
        if (rc) return rc;
        if (!pd) {
          set_last_error("preconditioner: Q + reg I is not positive definite");
          return DCORA_ERR_NOT_PD;
        }
        // nnz(L) of the SPARSE factor of this matrix (what a triangular solve would stream: the quantity SURVEY 8(d)
        // prices the preconditioner by), from the pattern alone -- the dense factor that was formed has k (k + 1) / 2
        CholSymbolic sym;
        chol_symbolic(M, block, &sym);
        long nz = 0;
        for (const CholPiece &pc : sym.pieces) nz += (long)pc.c * (pc.c + 1) / 2 + (long)pc.m * pc.c;
        ent.nnzL = nz;
      }
      ent.dense = buf;
      ent.bytes = buf->n * sizeof(double);
    }
    ent.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (env::init_timing()) fprintf(stderr, "[precond] built after %.1f ms\n", ent.build_ms);
    precond_cache_insert(key, ent);
  }
  if (env::init_timing())
    fprintf(stderr, "[precond] cached after %.1f ms\n",
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  precond_nnzL = ent.nnzL;
  if (want_sparse) {
    const int rc = sp.attach(ent.sparse, m.r);
    if (rc) return rc;
    sparse_precond = true;
  } else {
    ldm = ent.ldm;
    Minv_shared = ent.dense;
    Minv.borrow(ent.dense->p, ent.dense->n);
  }
  has_precond = true;
  precond_stale = false;
  precond_setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (env::init_timing()) fprintf(stderr, "[precond] attached after %.1f ms\n", precond_setup_ms);
  return DCORA_OK;
}

int DeviceProblem::enq_qapply(Buf2 X, int selX, const double *Gp, Buf2 Y, int selY, double *partials, Gate g) {
  if (has_bsr) {
    launch_spmm_bsr(st, m.r, m.d, Qb.view(), X, selX, Gp, Y, selY, partials, g);
    return spmm_bsr_grid(m.n);
  }
  launch_spmm(st, m.r, Q.view(), X, selX, Gp, Y, selY, partials, g);
  return spmm_grid(m.k, m.r) + Q.n_long;
}
void DeviceProblem::enqueue_egrad(const double *X, double *EG, double *partials) {
  enq_qapply(buf1(X), 0, has_G ? G.p : nullptr, buf1(EG), 0, partials, Gate{});
}

int DeviceProblem::enq_rgrad(Buf2 X, Buf2 EG, Buf2 RG, Buf2 S, int sel, double *partials, Gate g,
                             double *posenorm) {
  if (group) return launch_g_rgrad(st, m, X, EG, RG, S, sel, partials, posenorm, g);
  launch_rgrad(st, m, X, EG, RG, S, sel, partials, g);
  return pose_grid(m);
}
int DeviceProblem::enq_retract(Buf2 X, const double *V, double alpha, Buf2 out, int selOut, Buf2 grad,
                               const double *HV, double *partials, Gate g) {
  if (group) return launch_g_retract(st, m, X, V, alpha, out, selOut, grad, HV, partials, g);
  launch_retract(st, m, X, V, alpha, out, selOut, grad, HV, partials, g);
  return pose_grid(m);
}

void DeviceProblem::enq_minv(Buf2 R, double *Z, const double *p2, int np2, Gate g) {
  if (sparse_precond)
    sp.apply(st, m.r, R, Z, g);
  else
    launch_dense_apply(st, m.r, m.k, ldm, Minv.p, R, Z, p2, np2, g);
}
void DeviceProblem::enqueue_precond(const double *X, const double *V, double *out) {
  enq_minv(buf1(V), Zt.p, nullptr, 0, Gate{});
  launch_tangent(st, m, buf1(X), Zt.p, out, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, 0, 0);
}

// ---------------------------------------------------------------------------------------------------------
// host-pointer API
// ---------------------------------------------------------------------------------------------------------
int DeviceProblem::cost(const double *Xh, double *f) {
  DCORA_HIP(hipSetDevice(device));
  int rc = upload(Xh, X0.p, nelem());
  if (rc) return rc;
  enqueue_egrad(X0.p, EG0.p, pA.p);
  launch_sum_partials(st, pA.p, npA(), 2, 2, scal.p);
  double s[2];
  rc = download(scal.p, s, 2);
  if (rc) return rc;
  *f = 0.5 * s[0] + s[1];
  return DCORA_OK;
}
int DeviceProblem::eucgrad(const double *Xh, double *out) {
  DCORA_HIP(hipSetDevice(device));
  int rc = upload(Xh, X0.p, nelem());
  if (rc) return rc;
  enqueue_egrad(X0.p, EG0.p, nullptr);
  return download(EG0.p, out, nelem());
}
int DeviceProblem::riegrad(const double *Xh, double *out, double *norm) {
  DCORA_HIP(hipSetDevice(device));
  int rc = upload(Xh, X0.p, nelem());
  if (rc) return rc;
  enqueue_egrad(X0.p, EG0.p, nullptr);
  launch_rgrad(st, m, buf1(X0.p), buf1(EG0.p), buf1(RG0.p), buf1(S0.p), 0, pB.p, Gate{});
  launch_sum_partials(st, pB.p, npPose(), 1, 1, scal.p);
  double s;
  rc = download(scal.p, &s, 1);
  if (rc) return rc;
  if (norm) *norm = std::sqrt(s);
  if (out) return download(RG0.p, out, nelem());
  return DCORA_OK;
}
int DeviceProblem::hessvec(const double *Xh, const double *Vh, double *out) {
  DCORA_HIP(hipSetDevice(device));
  int rc = upload(Xh, X0.p, nelem());
  if (rc) return rc;
  rc = upload(Vh, delta.p, nelem());
  if (rc) return rc;
  enqueue_egrad(X0.p, EG0.p, nullptr);
  launch_rgrad(st, m, buf1(X0.p), buf1(EG0.p), buf1(RG0.p), buf1(S0.p), 0, pB.p, Gate{});
  launch_spmm(st, m.r, Q.view(), buf1(delta.p), 0, nullptr, buf1(W.p), 0, nullptr, Gate{});
  launch_hessfix(st, m, buf1(X0.p), buf1(S0.p), delta.p, W.p, Hd.p, p1.p, Gate{});
  return download(Hd.p, out, nelem());
}
bool DeviceProblem::hess_one_launch() const {
  const int main_grid = spmm_dir_fix_grid(m, m.k);
  if (main_grid <= 0 || main_grid + Q.n_long > 4 * kMaxPartials) return false;
  for (int jl : Q.long_host) {
    const bool euclid = m.se ? (jl % (m.d + 1) == m.d) : (jl >= m.d * m.n + m.l);
    if (!euclid) return false;
  }
  return true;
}
int DeviceProblem::hessvec_solver_form(const double *Xh, const double *Vh, double *out, double *dots) {
  if (!hess_one_launch()) {
    set_last_error("hessvec_solver_form: the one-launch form does not apply to this problem");
    return DCORA_ERR_UNSUPPORTED;
  }
  DCORA_HIP(hipSetDevice(device));
  int rc = upload(Xh, X0.p, nelem());
  if (rc) return rc;
  std::vector<double> neg(Vh, Vh + nelem());
  for (double &v : neg) v = -v;
  rc = upload(neg.data(), z.p, nelem());  // iteration 0 of the loop: delta = -z
  if (rc) return rc;
  rc = upload(Vh, delta2.p, nelem());
  if (rc) return rc;
  enqueue_egrad(X0.p, EG0.p, nullptr);
  launch_rgrad(st, m, buf1(X0.p), buf1(EG0.p), buf1(RG0.p), buf1(S0.p), 0, pB.p, Gate{});
  DCORA_HIP(hipMemsetAsync(p3.p, 0, sizeof(double), st));
  const int np = launch_spmm_dir_fix(st, m, Q.view(), buf1(X0.p), buf1(S0.p), z.p, delta2.p, delta.p, Hd.p, p3.p, 1, p1.p,
                                     ctl.p, 0, 0);
  std::vector<double> part((size_t)np);
  rc = download(p1.p, part.data(), part.size());
  if (rc) return rc;
  dots[0] = 0;
  for (double v : part) dots[0] += v;
  rc = download(Hd.p, out, nelem());
  if (rc) return rc;
  launch_spmm(st, m.r, Q.view(), buf1(delta.p), 0, nullptr, buf1(W.p), 0, nullptr, Gate{});
  launch_hessfix(st, m, buf1(X0.p), buf1(S0.p), delta.p, W.p, Hd.p, p1.p, Gate{});
  part.assign((size_t)npPose(), 0.0);
  rc = download(p1.p, part.data(), part.size());
  if (rc) return rc;
  dots[1] = 0;
  for (double v : part) dots[1] += v;
  return DCORA_OK;
}
int DeviceProblem::precondition(const double *Xh, const double *Vh, double *out) {
  if (!has_precond) {
    set_last_error("problem has no preconditioner");
    return DCORA_ERR_NO_PRECONDITIONER;
  }
  DCORA_HIP(hipSetDevice(device));
  int rc = upload(Xh, X0.p, nelem());
  if (rc) return rc;
  rc = upload(Vh, res.p, nelem());
  if (rc) return rc;
  enqueue_precond(X0.p, res.p, z.p);
  return download(z.p, out, nelem());
}
int DeviceProblem::retract(const double *Xh, const double *Vh, double *out) {
  DCORA_HIP(hipSetDevice(device));
  int rc = upload(Xh, X0.p, nelem());
  if (rc) return rc;
  rc = upload(Vh, eta.p, nelem());
  if (rc) return rc;
  launch_retract(st, m, buf1(X0.p), eta.p, 1.0, buf1(X1.p), 0, buf1(RG0.p), nullptr, nullptr, Gate{});
  return download(X1.p, out, nelem());
}
int DeviceProblem::tangent_project(const double *Xh, const double *Vh, double *out) {
  DCORA_HIP(hipSetDevice(device));
  int rc = upload(Xh, X0.p, nelem());
  if (rc) return rc;
  rc = upload(Vh, eta.p, nelem());
  if (rc) return rc;
  launch_tangent(st, m, buf1(X0.p), eta.p, z.p, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, 0, 0);
  return download(z.p, out, nelem());
}

int DeviceProblem::eval_dev(const double *Xd, double *f, double *gradnorm) {
  enqueue_egrad(Xd, EG1.p, pA.p);
  launch_rgrad(st, m, buf1(Xd), buf1(EG1.p), Buf2{{nullptr, nullptr}}, Buf2{{nullptr, nullptr}}, 0, pB.p, Gate{});
  launch_sum_partials(st, pA.p, npA(), 2, 2, scal.p);
  launch_sum_partials(st, pB.p, npPose(), 1, 1, scal.p + 2);
  double s[3];
  int rc = download(scal.p, s, 3);
  if (rc) return rc;
  if (f) *f = 0.5 * s[0] + s[1];
  if (gradnorm) *gradnorm = std::sqrt(s[2]);
  return DCORA_OK;
}

// ---------------------------------------------------------------------------------------------------------
// QuadraticOptimizer::optimize
// ---------------------------------------------------------------------------------------------------------
int DeviceProblem::optimize(const dcora_ropt_params &prm, const double *X0h, double *Xout, dcora_ropt_result *res_out) {
  DCORA_HIP(hipSetDevice(device));
  int rc = upload(X0h, X0.p, nelem());
  if (rc) return rc;
  double *X = nullptr;
  if ((rc = optimize_dev(prm)) || (rc = result(&X)) || (rc = fetch_result(res_out))) return rc;
  return download(X, Xout, nelem());
}

int DeviceProblem::optimize_dev(const dcora_ropt_params &prm) {
  pending_ = false;
  rgd_ = prm.method != 0;
  TcgForm form = TcgForm::generic;
  if (fused) form = !use_pc() ? TcgForm::split : (tcg_run_ok && !concurrent_solves) ? TcgForm::run : TcgForm::pc;
  // a G that was to ride in the start-point evaluation where that is not k_fused_grad (RtrForm::gf): its own launch
  if (ride_X_ && (rgd_ || !has_precond || form == TcgForm::generic || has_bsr || Q.n_long != 0)) {
    launch_spmm(st, m.r, ride_C_, buf1(ride_X_), 0, nullptr, buf1(G.p), 0, nullptr, Gate{});
    ride_X_ = nullptr;
  }
  if (rgd_) return rgd_dev(prm);
  if (!has_precond) {
    set_last_error("RTR requires the preconditioner (ref src/QuadraticProblem.cpp:78-82)");
    return DCORA_ERR_NO_PRECONDITIONER;
  }
  return rtr_dev(prm, form);
}

int DeviceProblem::fetch_result(dcora_ropt_result *res_out) {
  if (pending_) {
    SolverCtl h;
    DCORA_HIP(hipMemcpyAsync(&h, ctl.p, sizeof h, hipMemcpyDeviceToHost, st));
    DCORA_HIP(hipStreamSynchronize(st));
    DCORA_HIP(hipGetLastError());
    const double now = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch())
                           .count();
    cur_after_fetch_ = h.cur & 1;
    last_res_.success = 1;
    last_res_.fInit = h.fInit;
    last_res_.gradNormInit = h.gradNormInit;
    last_res_.fOpt = h.f1;
    last_res_.gradNormOpt = h.ngf;
    last_res_.elapsedMs = now - t0_ms_;
    last_res_.tCGStatus = h.tcg_status;
    last_res_.outer_iterations = h.outer_it;
    last_res_.inner_iterations = h.inner_total;
    last_res_.accepted_steps = h.accepted;
    pending_ = false;
  }
  if (res_out) *res_out = last_res_;
  return DCORA_OK;
}

Buf2 DeviceProblem::result_pick(const SolverCtl **c) const {
  *c = rgd_ ? nullptr : ctl.p;
  return rgd_ ? buf1(X1.p) : Xb();
}

int DeviceProblem::result(double **X) {
  const int rc = fetch_result(nullptr);
  if (rc) return rc;
  *X = cur_after_fetch_ ? X1.p : X0.p;
  return DCORA_OK;
}

// one preconditioned Riemannian gradient step (ref src/QuadraticOptimizer.cpp:123-150); the result is X1
int DeviceProblem::rgd_dev(const dcora_ropt_params &prm) {
  const auto t0 = std::chrono::steady_clock::now();
  double f0 = 0, g0 = 0;
  int rc = eval_dev(X0.p, &f0, &g0);
  if (rc) return rc;
  enqueue_egrad(X0.p, EG0.p, nullptr);
  launch_rgrad(st, m, buf1(X0.p), buf1(EG0.p), buf1(RG0.p), buf1(S0.p), 0, pB.p, Gate{});
  const double *dir = RG0.p;
  if (prm.RGD_use_preconditioner) {
    if (!has_precond) {
      set_last_error("RGD with preconditioning requested but the problem has none");
      return DCORA_ERR_NO_PRECONDITIONER;
    }
    enqueue_precond(X0.p, RG0.p, z.p);
    dir = z.p;
  }
  launch_retract(st, m, buf1(X0.p), dir, -prm.RGD_stepsize, buf1(X1.p), 0, buf1(RG0.p), nullptr, nullptr, Gate{});
  double f1 = 0, g1 = 0;
  rc = eval_dev(X1.p, &f1, &g1);
  if (rc) return rc;
  last_res_.success = 1;
  last_res_.fInit = f0;
  last_res_.gradNormInit = g0;
  last_res_.fOpt = f1;
  last_res_.gradNormOpt = g1;
  last_res_.elapsedMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  last_res_.tCGStatus = TR_MAXITER;
  last_res_.outer_iterations = 1;
  last_res_.inner_iterations = 0;
  last_res_.accepted_steps = 1;
  cur_after_fetch_ = 1;
  return DCORA_OK;
}

namespace {
// spin on host-mapped words; never blocks inside the HIP runtime
template <class Pred>
bool spin_until(Pred p, double timeout_s) {
  const auto t0 = std::chrono::steady_clock::now();
  unsigned it = 0;
  while (!p()) {
    if ((++it & 1023u) == 0) {
      if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s) return false;
    }
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
  return true;
}
}  // namespace

// sum of the HIP-event times of the k_tcg_run launches recorded since the last read (gated no-op launches included)
int DeviceProblem::profile_tcg_read(double *launches, double *total_us) {
  DCORA_HIP(hipSetDevice(device));
  DCORA_HIP(hipStreamSynchronize(st));
  double us = 0;
  for (size_t i = 0; i + 1 < run_events_used; i += 2) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, run_events[i], run_events[i + 1]) == hipSuccess) us += 1e3 * ms;
  }
  *launches = (double)(run_events_used / 2);
  *total_us = us;
  run_events_used = 0;
  return DCORA_OK;
}

// the operands of this problem's dense tCG launches (kernels.h), from its workspace
TcgOperands DeviceProblem::tcg_operands() const {
  TcgOperands o;
  o.m = m;  o.ldm = ldm;  o.Minv = sparse_precond ? nullptr : Minv.p;
  o.Q = Q.view();  o.has_bsr = has_bsr;
  if (has_bsr) o.Qb = Qb.view();
  o.grad = RGb();  o.X = Xb();  o.S = Sb();
  o.d[0] = delta.p;  o.d[1] = delta2.p;  o.r[0] = res.p;  o.r[1] = res2.p;
  o.Hd = Hd.p;  o.eta = eta.p;  o.Heta = Heta.p;  o.z = z.p;  o.Zpart = Zpart.p;  o.W = W.p;
  o.p1 = p1.p;  o.p2 = p2.p;  o.p3 = p3.p;  o.pC = pC.p;
  o.ctl = ctl.p;  o.hf = hf_dev;  o.sync = tcg_sync.p;
  if (run_cols_used()) {
    o.cols.lp = run_cols.p;
    o.cols.list = run_cols.p + run_cols_nwg + 1;
    o.cols.slot = o.cols.list + run_cols_nlist;
  }
  // without hubs the sparse preconditioner's two permutations ride in B (scatter of the residual) and C (gather of z)
  if (sparse_precond && sp.foldable()) o.sf = sp.fold();
  return o;
}

bool DeviceProblem::use_pc() const {
  const int forced = env::solver_bc();
  if (sparse_precond || !has_precond) return false;
  if (forced < 0) return false;
  if (!forced && !fused_pc_preferred(m, ldm)) return false;
  // the one-launch form needs more dynamic LDS than the default limit; a device that refuses the attribute keeps B + C
  return fused_pc_ready(m, ldm);
}

// What an RTR solve enqueues in each tCG form; DeviceProblem::rtr_dev paces it.  The forms:
//   generic: the thread-per-variable kernels of manifold.hip, kernels.hip and spmm_csr.hip, any layout -- per tCG iteration the
//            Hessian SpMM with the direction update folded in (k_spmm_dir [+ k_hessfix], or k_spmm_dir_fix),
//            k_tcg_update1, the preconditioner, k_tangent;
//   split:   the fused kernels of fused_step.hip (SE layout, r <= 8) -- per tCG iteration A (direction update +
//            Q-apply + Riemannian Hessian correction + <d,Hd>), B (step length + vector updates + |r|^2 + dense
//            preconditioner slices; with the sparse preconditioner its level replay follows), C (stopping rule + slice
//            sum + tangent projection + <z,r>);
//   pc:      A, then B + C in one launch (k_fused_pc, dense preconditioner) where that form wins; DCORA_SOLVER_BC = pc /
//            split forces one or the other;
//   run:     the whole tCG run of an RTR iteration as ONE launch (k_tcg_run) where the grid is co-resident and no
//            other solve shares the device's launch path.  A run that gives up (tcg_abort_seq) or a launch that is
//            refused switches it off for this problem: the iteration is taken again on the pc launches.
struct DeviceProblem::RtrForm {
  DeviceProblem &p;
  TcgForm form;
  int &seq;
  const int solve_first;
  const TcgOperands o;  // what the fused launches share; the generic form reads its Q and direction buffers too
  SolverCtl *const c;   // o.ctl, for the gates of every form
  const double *const Gp;
  const long N;
  const int nA, nP, nV, nPB;
  const bool sparse;
  // generic: the sparse preconditioner's permutations (and hub correction) ride in k_tcg_update1 / k_tangent; H d in
  // one launch (k_spmm_dir_fix) when every long row is a Euclidean column and the partial slots fit
  const SpFold sfg;
  const bool hess_fused;
  // fused forms
  const int nPG;
  const bool folded;  // the sparse preconditioner's permutations ride in B and C (o.sf)
  const int nZ;  // <z, r> partial slots A sums in its prologue
  // cost + gradient of an evaluation in one launch where the kernel exists (small CSR blocks; large blocks: the same
  // on the block structure, k_spmm_bsrq<.., GRAD>), else Q-apply + rgrad
  const bool gf, gfb;
  unsigned *const sync_p;  // the run form's grid-step counters, zeroed by k_rtr_init / k_rtr_decide
  const int nsync;

  RtrForm(DeviceProblem &p_, TcgForm f, int &seq_)
      : p(p_), form(f), seq(seq_), solve_first(seq_ + 1), o(p.tcg_operands()), c(o.ctl),
        Gp(p.has_G ? p.G.p : nullptr), N(p.nelem()), nA(p.npA()), nP(p.npPose()), nV(p.npVec()),
        nPB(fused_pose_blocks(p.m)), sparse(p.sparse_precond),
        sfg(f == TcgForm::generic && sparse ? p.sp.fold_generic() : SpFold()),
        hess_fused(f == TcgForm::generic && p.hess_one_launch()),
        nPG(sparse ? fused_update_grid(p.m) : fused_precond_grid(p.m)), folded(sparse && p.sp.foldable()),
        nZ(f == TcgForm::pc || f == TcgForm::run ? fused_pc_blocks(p.m) : nPB),
        gf(f != TcgForm::generic && !p.has_bsr && p.Q.n_long == 0), gfb(f != TcgForm::generic && p.has_bsr),
        sync_p(f == TcgForm::run ? p.tcg_sync.p : nullptr), nsync(f == TcgForm::run ? tcg_run_sync_words() : 0) {}

  bool outer_done() const { return p.hf->outer_done_seq >= solve_first; }
  bool stopped(int tcg_first) const { return p.hf->tcg_done_seq >= tcg_first || outer_done(); }
  int nAe() const { return gf ? nPB : nA; }  // {<XQ,X>, <X,G>} partial slots of an evaluation

  // f and the Riemannian gradient at buffer `sel` (the trial point: sel = 1); sel = 0 starts the solve with null gates
  // (its control block is armed by k_rtr_init, which follows).  Returns the |grad|^2 partial slots written.
  int eval(int sel) {
    const auto g = [&] {
      ++seq;
      return sel ? Gate{c, seq, 1} : Gate{};
    };
    const Buf2 kNoBuf{{nullptr, nullptr}};  // EG of the block-structure evaluation: nobody reads it
    if (form == TcgForm::generic) {
      // (enq_qapply, not the CSR kernel directly: the number of partial slots npA() counts follows the Q-apply kernel
      // that runs -- block-CSR for large pose graphs; the thread-per-pose rgrad whatever `group` says)
      p.enq_qapply(p.Xb(), sel, Gp, p.EGb(), sel, p.pA.p, g());
      launch_rgrad(p.st, p.m, p.Xb(), p.EGb(), p.RGb(), p.Sb(), sel, p.pB.p, g());
      return nP;
    }
    if (gf) {
      GradRide ride;
      if (sel == 0 && p.ride_X_) {  // (optimize_dev leaves it only where gf holds)
        ride.c_rp = p.ride_C_.rp;
        ride.c_ci = p.ride_C_.ci;
        ride.c_v = p.ride_C_.v;
        ride.c_X = p.ride_X_;
        ride.G_out = p.G.p;
        p.ride_X_ = nullptr;
      }
      return launch_fused_grad(p.st, p.m, o.Q, p.Xb(), Gp, p.EGb(), p.RGb(), p.Sb(), sel, p.pA.p, p.pB.p, nullptr, g(),
                               ride.c_rp ? &ride : nullptr);
    }
    if (gfb)
      return launch_fused_grad_bsr(p.st, p.m.r, p.m.d, o.Qb, p.Xb(), Gp, kNoBuf, p.RGb(), p.Sb(), sel, p.pA.p, p.pB.p,
                                   nullptr, g());
    p.enq_qapply(p.Xb(), sel, Gp, p.EGb(), sel, p.pA.p, g());
    return p.enq_rgrad(p.Xb(), p.EGb(), p.RGb(), p.Sb(), sel, p.pB.p, g());
  }

  // The first block of an RTR iteration, z0 = P grad (generic: k_tcg_begin, the preconditioner, k_tangent; fused: B in
  // "first" mode, B + C in one launch, or the whole run).  Gated by the RTR loop's own stamp, it picks the accepted
  // iterate's buffers from the control block when it starts.  Returns the seq of its first launch, < 0 when a launch
  // failed (the error is set).
  int first() {
    switch (form) {
      case TcgForm::generic: {
        launch_tcg_begin(p.st, N, p.RGb(), p.eta.p, p.Heta.p, p.res.p, c, ++seq);
        const int s = seq;
        p.enq_minv(buf1(p.res.p), p.Zt.p, nullptr, 0, Gate{c, ++seq, 1});
        launch_tangent(p.st, p.m, p.Xb(), p.Zt.p, p.z.p, p.res.p, p.p3.p, nullptr, 0, c, p.hf_dev, ++seq, 1, 0);
        return s;
      }
      case TcgForm::run: {
        const int s = launch_run();
        if (s != 0) return s;
        // refused: the device does not grant the run its dynamic LDS -- the same fall-back as a run that gave up
        p.tcg_run_ok = false;
        form = TcgForm::pc;
      }
        [[fallthrough]];
      case TcgForm::pc:
        if (launch_fused_pc(p.st, o, ++seq, 0, 1, 0, false) < 0) {
          set_last_error("k_fused_pc could not be launched on this device");
          return -1;
        }
        return seq;
      case TcgForm::split:
        launch_fused_precond(p.st, o, ++seq, 0, 1, 0);
        return seq;
    }
    return -1;
  }
  // k_tcg_run, between HIP events when profiled; returns its seq, 0 when the launch was refused, -1 on a failure
  int launch_run() {
    hipEvent_t e1 = nullptr;
    if (p.profile_tcg_runs) {
      while (p.run_events.size() < p.run_events_used + 2) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) {
          set_last_error("hipEventCreate failed (k_tcg_run profile)");
          return -1;
        }
        p.run_events.push_back(e);
      }
      (void)hipEventRecord(p.run_events[p.run_events_used], p.st);
      e1 = p.run_events[p.run_events_used + 1];
      p.run_events_used += 2;
    }
    if (launch_tcg_run(p.st, o, ++seq) < 0) {
      if (e1) p.run_events_used -= 2;
      return 0;
    }
    if (e1) (void)hipEventRecord(e1, p.st);
    return seq;
  }
  // The rest of the first block in the split form: the sparse replay and C.  A rejected step (k_rtr_decide said so in
  // reject_seq) left the iterate and its gradient where they were: z0 is the one of the iteration before, whose
  // unprojected form the finish kernel kept in W (free on this path) -- one application of the sparse preconditioner
  // less per rejection (0.25 per RBCD iteration on the 100k lattice).
  void rest(bool rejected) {
    if (form != TcgForm::split) return;
    if (sparse && rejected) {
      launch_fused_finish(p.st, o, ++seq, 0, 1, 0, FinishZ::from_raw);
      return;
    }
    if (sparse) p.sp.apply(p.st, p.m.r, buf1(o.res_new(0, 1)), p.Zpart.p, Gate{c, ++seq, 1}, folded);
    launch_fused_finish(p.st, o, ++seq, 0, 1, 0, sparse ? FinishZ::keep_raw : FinishZ::slices);
  }

  // The sparse replay behind the verdict of the step kernel just enqueued (k_tcg_update1 / B), which decides whether
  // the tCG run goes on (boundary, negative curvature).  The replay's launches behind a step that stopped are no-ops of
  // ~4 us each, and runs of one or two iterations are the rule on the large blocks.  So only the replay's FIRST launch
  // is enqueued on speculation: the host reads the verdict while the GPU runs it, and enqueues the rest only behind a
  // step that went on.  (The same pacing on the dense one-launch form measured slower -- 1846 -> 1729-1857 it/s on the
  // headline: its trace holds 69 gated no-op launches among 38 800, and waiting for a verdict there only opens gaps --
  // and is not kept.)  Returns 1: the run goes on, 0: it stopped, -1: spin timeout.
  int replay(Buf2 R, double *Z, bool levels_only, int tcg_first) {
    const int seq_step = seq;
    bool timed = false;
    const std::function<bool()> verdict = [&]() {
      if (!spin_until([&] { return p.hf->go_seq >= seq_step || stopped(tcg_first); }, 20.0)) {
        timed = true;
        return false;
      }
      return !stopped(tcg_first);
    };
    p.sp.apply(p.st, p.m.r, R, Z, Gate{c, ++seq, 2}, levels_only, &verdict);
    if (timed) return -1;
    return stopped(tcg_first) ? 0 : 1;
  }

  // tCG iteration j; the direction ping-pongs between two buffers (the fused forms' residual too).  Returns 1: the
  // run goes on, 0: it stopped, -1: spin timeout.
  int tcg_iter(int j, int max_inner, int tcg_first) {
    const int par = j & 1;
    if (form == TcgForm::generic) {
      // the direction update (the tCG recurrence: iteration 0 starts it, later ones finish iteration j - 1) rides in
      // the Hessian SpMM (k_spmm_dir)
      double *const dcur = o.d[par];
      int nP1 = nP;
      if (hess_fused) {
        nP1 = launch_spmm_dir_fix(p.st, p.m, o.Q, p.Xb(), p.Sb(), p.z.p, o.d[par ^ 1], dcur, p.Hd.p, p.p3.p, nP, p.p1.p,
                                  c, ++seq, j);
      } else {
        launch_spmm_dir(p.st, p.m.r, o.Q, p.z.p, o.d[par ^ 1], dcur, p.W.p, p.p3.p, nP, c, ++seq, j);
        launch_hessfix(p.st, p.m, p.Xb(), p.Sb(), dcur, p.W.p, p.Hd.p, p.p1.p, Gate{c, ++seq, 2});
      }
      launch_tcg_update1(p.st, N, dcur, p.Hd.p, p.eta.p, p.Heta.p, p.res.p, p.p1.p, nP1, p.p2.p, c, p.hf_dev, ++seq, j,
                         p.m.r, sfg);
      if (sfg.y) {
        const int go = replay(buf1(p.res.p), p.Zt.p, true, tcg_first);
        if (go <= 0) return go;
      } else {
        p.enq_minv(buf1(p.res.p), p.Zt.p, p.p2.p, nV, Gate{c, ++seq, 2});
      }
      launch_tangent(p.st, p.m, p.Xb(), p.Zt.p, p.z.p, p.res.p, p.p3.p, p.p2.p, nV, c, p.hf_dev, ++seq, 2, j, sfg);
      // the inner loop exhausted: the bookkeeping of the last direction update (status TR_MAXITER) has no next SpMM
      if (j == max_inner - 1) launch_tcg_update2(p.st, N, p.z.p, dcur, p.p3.p, nP, c, p.hf_dev, ++seq, j);
      return 1;
    }
    const int nP1 = launch_fused_hess(p.st, o, ++seq, j, nZ);
    if (form == TcgForm::pc) {
      launch_fused_pc(p.st, o, ++seq, j, 0, nP1, true);
      return 1;
    }
    launch_fused_precond(p.st, o, ++seq, j, 0, nP1);
    if (sparse) {
      const int go = replay(buf1(o.res_new(j, 0)), p.Zpart.p, folded, tcg_first);
      if (go <= 0) return go;
    }
    launch_fused_finish(p.st, o, ++seq, j, 0, nPG);
    return 1;
  }

  // the trial point; returns the {<eta, grad>, <eta, H eta>} partial slots written
  int trial() {
    switch (form) {
      case TcgForm::generic:
        launch_retract(p.st, p.m, p.Xb(), p.eta.p, 1.0, p.Xb(), 1, p.RGb(), p.Heta.p, p.pC.p, Gate{c, ++seq, 1});
        return nP;
      case TcgForm::split:
        return p.enq_retract(p.Xb(), p.eta.p, 1.0, p.Xb(), 1, p.RGb(), p.Heta.p, p.pC.p, Gate{c, ++seq, 1});
      default:  // the kernel that ended the tCG run has retracted already, one partial pair per workgroup
        return nZ;
    }
  }
};

// RTRNewton with preconditioned Steihaug-Toint tCG, fully device-resident: the host enqueues the kernel sequence of
// the form (RtrForm), stays at most kLookahead tCG iterations ahead of the GPU and learns about terminations from
// host-mapped flags.  Returns without synchronising.  (ref src/QuadraticOptimizer.cpp:52-108, 234-280; ROPTLIB
// semantics: SURVEY.md 3.4)
int DeviceProblem::rtr_dev(const dcora_ropt_params &prm, TcgForm form) {
  constexpr int kLookahead = 2;
  const auto t0 = std::chrono::steady_clock::now();
  t0_ms_ = std::chrono::duration<double, std::milli>(t0.time_since_epoch()).count();
  const bool single = (prm.RTR_iterations == 1);
  const int max_outer = single ? 12 : prm.RTR_iterations;  // ref :254-273 (<= 11 retries)
  const int max_inner = prm.RTR_tCG_iterations;
  if (seq_ > 1500000000) {  // keep the monotonic sequence far from INT_MAX
    DCORA_HIP(hipStreamSynchronize(st));
    hf->last_seq_done = 0;
    hf->tcg_done_seq = 0;
    hf->outer_done_seq = 0;
    hf->go_seq = 0;
    hf->reject_seq = 0;
    seq_ = 0;
  }
  int &seq = seq_;
  RtrForm f(*this, form, seq);
  CtlInit ci;  // written by k_rtr_init, which follows the start point's evaluation (that runs with null gates)
  ci.enable = 1;
  ci.tol = prm.gradnorm_tol;
  ci.Delta = prm.RTR_initial_radius;
  ci.maxDelta = single ? prm.RTR_initial_radius : 5 * prm.RTR_initial_radius;  // :240-241, :259-260
  ci.max_outer = max_outer;
  ci.stop_on_accept = single ? 1 : 0;
  ci.max_inner = max_inner;
  auto timed_out = [&]() {
    set_last_error("rtr_dev: device did not make progress (spin timeout)");
    return DCORA_ERR_HIP;
  };
  auto first_failed = [&]() -> int {
    DCORA_HIP(hipStreamSynchronize(st));
    return DCORA_ERR_HIP;
  };
  auto time_is_up = [&]() {  // TimeBound :252
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 5.0;
  };
  auto run_gave_up = [&]() { return f.form == TcgForm::run && hf->tcg_abort_seq >= f.solve_first; };

  // f(x0), grad(x0) from buffer 0
  int nG = f.eval(0);
  launch_rtr_init(st, pA.p, f.nAe(), pB.p, nG, f.c, hf_dev, ++seq, ci, f.sync_p, f.nsync);
  int last_pace_seq = seq;
  std::vector<int> last_seq((size_t)std::max(1, max_inner));  // of every tCG iteration's last launch
  // The first block of an RTR iteration needs nothing the host has to decide, so it is enqueued BEHIND k_rtr_init /
  // k_rtr_decide at once, before the host has seen their verdict: the GPU runs it while the host reads the flag and
  // enqueues the tCG iteration behind it, instead of idling for that round trip at every iteration (a loop that had
  // ended leaves gated no-ops).  0: the time bound had passed when it was due.
  int next_first_seq = time_is_up() ? 0 : f.first();
  // The host runs ahead of the device by design, but it must not LEAVE while a one-launch run may still give up: the
  // recovery below is the only place that repeats the iteration, and what the caller enqueues next builds on its
  // result.  So with the run form the loop takes one more turn after the last iteration (`tail`), which only waits
  // until that run has ended (its first workgroup raises last_seq_done when the run finishes; a run that finishes has
  // not given up: run_grid_step) or has given up -- then the turn repeats the iteration on the launches like any other.
  // (Round 5: without it a last iteration whose run gave up was lost without a trace -- a flaky bit difference between
  // ranks sharing one GPU, where other ranks' waiting kernels keep the grid from being co-resident.)
  int last_run_seq = 0;
  for (int outer = 0; outer < max_outer || (f.form == TcgForm::run && last_run_seq > 0); ++outer) {
    const bool tail = outer >= max_outer;
    if (!tail && next_first_seq < 0) return first_failed();
    const int need_seq = tail ? last_run_seq : last_pace_seq;
    if (!spin_until([&] { return hf->last_seq_done >= need_seq || f.outer_done() || run_gave_up(); }, 20.0))
      return timed_out();
    if (tail && !run_gave_up()) break;
    if (run_gave_up()) {
      // The one-launch run of iteration `outer` (or the one before: its evaluation and decision were queued behind it)
      // found its grid not co-resident and left; everything queued behind it was a no-op (outer_done_stamp).  Re-arm
      // the control block, drop the form for this problem and take the iteration again on the launches: the run wrote
      // nothing but scratch (eta, H eta, the trial point and the control block are written when a run ENDS).
      DCORA_HIP(hipStreamSynchronize(st));
      const int armed = INT_MAX;
      DCORA_HIP(hipMemcpy(&f.c->outer_done_stamp, &armed, sizeof(int), hipMemcpyHostToDevice));
      if (hf->last_seq_done < last_pace_seq) --outer;  // the decision of iteration outer - 1 never ran
      hf->tcg_abort_seq = 0;
      tcg_run_ok = false;
      f.form = TcgForm::pc;
      next_first_seq = f.first();
      if (next_first_seq < 0) return first_failed();
    }
    if (f.outer_done()) break;
    if (next_first_seq == 0) break;  // the time bound had passed when this iteration's first kernel was due
    const int tcg_first_seq = next_first_seq;
    last_run_seq = f.form == TcgForm::run ? tcg_first_seq : 0;
    f.rest(outer > 0 && hf->reject_seq == last_pace_seq);
    for (int j = 0; j < max_inner && f.form != TcgForm::run; ++j) {
      if (j >= kLookahead) {
        const int need = last_seq[j - kLookahead];
        if (!spin_until([&] { return hf->last_seq_done >= need || f.stopped(tcg_first_seq); }, 20.0))
          return timed_out();
      }
      if (hf->tcg_done_seq >= tcg_first_seq) break;
      const int go = f.tcg_iter(j, max_inner, tcg_first_seq);
      if (go < 0) return timed_out();
      if (go == 0) break;
      last_seq[j] = seq;
    }
    // ---- trial point, model ratio, acceptance ----
    const int nR = f.trial();
    nG = f.eval(1);
    launch_rtr_decide(st, pA.p, f.nAe(), pB.p, nG, pC.p, nR, f.c, hf_dev, ++seq, f.sync_p, f.nsync);
    last_pace_seq = seq;
    if (outer + 1 < max_outer) next_first_seq = time_is_up() ? 0 : f.first();
  }
  pending_ = true;
  return DCORA_OK;
}

// ref src/QuadraticProblem.cpp:138-234 (rare path, host-paced: one scalar read-back per trial step)
int DeviceProblem::escape_saddle(const double *Xopt, double theta, const double *v, double gtol, double pgtol,
                                 bool second_order, double *Xout, int *success) {
  if (!has_precond) {
    set_last_error("escapeSaddle needs the preconditioner");
    return DCORA_ERR_NO_PRECONDITIONER;
  }
  if (m.r < 2) {
    set_last_error("escapeSaddle needs a problem of rank 2 at least (the point has one row less)");
    return DCORA_ERR_BAD_ARG;
  }
  DCORA_HIP(hipSetDevice(device));
  // the point and v staged in two slices the search does not use
  int rc = upload(Xopt, W.p, (size_t)(m.r - 1) * m.k);
  if (rc) return rc;
  rc = upload(v, Hd.p, (size_t)m.k);
  if (rc) return rc;
  DCORA_HIP(hipStreamSynchronize(st));  // (the caller's pageable buffers have been read)
  rc = escape_saddle_dev(W.p, Hd.p, theta, gtol, pgtol, second_order, success, nullptr);
  if (rc || !*success) return rc;
  return download(X1.p, Xout, nelem());
}

int DeviceProblem::escape_saddle_dev(const double *Xprev, const double *v, double theta, double gtol, double pgtol,
                                     bool second_order, int *success, double stats[4]) {
  *success = 0;
  if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
  if (!has_precond) {
    set_last_error("escapeSaddle needs the preconditioner");
    return DCORA_ERR_NO_PRECONDITIONER;
  }
  if (m.r < 2) {
    set_last_error("escapeSaddle needs a problem of rank 2 at least (the point has one row less)");
    return DCORA_ERR_BAD_ARG;
  }
  DCORA_HIP(hipSetDevice(device));
  // X_plus = [X; 0] into X0, the direction [0; v^T] into eta: one launch
  launch_lift_images(st, m.r - 1, m.k, Xprev, v, X0.p, eta.p);
  DCORA_HIP(hipGetLastError());
  double FX = 0;
  int rc = eval_dev(X0.p, &FX, nullptr);
  if (rc) return rc;
  if (stats) stats[2] = stats[3] = FX;
  EscapeSearch search(theta, gtol, pgtol, second_order, FX);
  while (search.more()) {
    escape_trial_point(search.alpha);
    escape_trial_scalars(scal.p);
    double s[4];
    rc = download(scal.p, s, 4);
    if (rc) return rc;
    const double FXt = 0.5 * s[0] + s[1];
    const bool accepted = search.offer(FXt, std::sqrt(s[2]), std::sqrt(s[3]));
    if (stats) stats[0] = (double)search.trials();
    if (accepted) {
      *success = 1;
      if (stats) stats[1] = search.alphas.back(), stats[3] = FXt;
      return DCORA_OK;
    }
  }
  const int idx = search.fallback();
  if (idx >= 0) {
    escape_trial_point(search.alphas[(size_t)idx]);
    *success = 1;
    if (stats) stats[1] = search.alphas[(size_t)idx], stats[3] = search.fvals[(size_t)idx];
  }
  return DCORA_OK;
}

// One trial of the search, in the two halves its callers enqueue (between them the ranks of a job exchange the public
// columns of their trial points and form G): X1 = Retract(X0, alpha eta) ...
void DeviceProblem::escape_trial_point(double alpha) {
  launch_retract(st, m, buf1(X0.p), eta.p, alpha, buf1(X1.p), 0, buf1(RG0.p), nullptr, nullptr, Gate{});
}
// ... and its four scalars into out4 (device): <X1 Q, X1>, <X1, G>, |rgrad(X1)|^2, |Proj(rgrad(X1) M^-1)|^2 -- each
// summed from its partial slots in slot order by one workgroup (no atomics: the same bits whatever the schedule)
void DeviceProblem::escape_trial_scalars(double *out4) {
  enqueue_egrad(X1.p, EG1.p, pA.p);
  launch_rgrad(st, m, buf1(X1.p), buf1(EG1.p), buf1(RG1.p), buf1(S1.p), 0, pB.p, Gate{});
  enqueue_precond(X1.p, RG1.p, z.p);
  launch_dot(st, nelem(), z.p, z.p, p3.p);
  launch_sum_partials(st, pA.p, npA(), 2, 2, out4);
  launch_sum_partials(st, pB.p, npPose(), 1, 1, out4 + 2);
  launch_sum_partials(st, p3.p, npVec(), 1, 1, out4 + 3);
}

int DeviceProblem::time_qapply(int reps, double *avg_ms, double *bytes) {
  DCORA_HIP(hipSetDevice(device));
  hipEvent_t e0, e1;
  DCORA_HIP(hipEventCreate(&e0));
  DCORA_HIP(hipEventCreate(&e1));
  for (int i = 0; i < 3; ++i) enqueue_egrad(X0.p, EG0.p, nullptr);
  DCORA_HIP(hipEventRecord(e0, st));
  for (int i = 0; i < reps; ++i) enqueue_egrad(X0.p, EG0.p, nullptr);
  DCORA_HIP(hipEventRecord(e1, st));
  DCORA_HIP(hipEventSynchronize(e1));
  float ms = 0;
  DCORA_HIP(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *avg_ms = (double)ms / reps;
  // nnz (8+4) + (k+1) 4 + r k 8 (read X) + r k 8 (write Y) [+ r k 8 for G]
  *bytes = 12.0 * Q.nnz + 4.0 * (m.k + 1) + 16.0 * m.r * m.k + (has_G ? 8.0 * m.r * m.k : 0.0);
  return DCORA_OK;
}

}  // namespace dcora

namespace dcora {
// times the dense-preconditioner kernel of the solver (k_fused_precond in its start-of-tCG form: residual = grad,
// no step) with HIP events on the problem's stream
int DeviceProblem::time_precond(int reps, double *avg_ms, double *bytes) {
  if (!has_precond || (!fused && !sparse_precond)) {
    set_last_error("time_precond: needs a preconditioner and the fused solver path or the sparse preconditioner");
    return DCORA_ERR_UNSUPPORTED;
  }
  DCORA_HIP(hipSetDevice(device));
  launch_ctl_init(st, ctl.p, 1e-2, 100, 500, 3, 0, 50);
  hipEvent_t e0, e1;
  DCORA_HIP(hipEventCreate(&e0));
  DCORA_HIP(hipEventCreate(&e1));
  // The dense kernel is timed in its in-loop form (step length from the <d, H d> partials, vector updates, |r|^2),
  // not in the shorter form that opens a tCG run; the partials are set so that the step is a no-op.
  const int nPB = fused_pose_blocks(m);
  if (!sparse_precond) {
    std::vector<double> ones(std::max((size_t)nPB, (size_t)nelem()), 1.0);
    DCORA_HIP(hipMemcpyAsync(p1.p, ones.data(), sizeof(double) * nPB, hipMemcpyHostToDevice, st));
    // a non-zero residual, so that the one-launch form does not leave through its stopping rule
    DCORA_HIP(hipMemcpyAsync(res.p, ones.data(), sizeof(double) * nelem(), hipMemcpyHostToDevice, st));
    DCORA_HIP(hipMemsetAsync(Hd.p, 0, sizeof(double) * nelem(), st));
    DCORA_HIP(hipStreamSynchronize(st));
  }
  const bool bc_split = !use_pc();
  // every launch is iteration 1 (odd: it reads d[1], r[1] and writes r[0]) on delta, res and res2
  TcgOperands o = tcg_operands();
  std::swap(o.d[0], o.d[1]);
  std::swap(o.r[0], o.r[1]);
  auto run = [&]() {
    if (sparse_precond)
      sp.apply(st, m.r, buf1(RG0.p), Zt.p, Gate{});
    else if (!bc_split)  // the one-launch B + C of the dense path, in its in-loop form
      launch_fused_pc(st, o, 1, 1, 0, nPB, false);
    else
      launch_fused_precond(st, o, 1, 1, 0, nPB);
  };
  for (int i = 0; i < 3; ++i) run();
  DCORA_HIP(hipEventRecord(e0, st));
  for (int i = 0; i < reps; ++i) run();
  DCORA_HIP(hipEventRecord(e1, st));
  DCORA_HIP(hipEventSynchronize(e1));
  float ms = 0;
  DCORA_HIP(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *avg_ms = (double)ms / reps;
  // algorithmic bytes: the k x k inverse once, the residual in, the split-K slices out
  // algorithmic bytes, dense form: the k x k inverse once; split form: + the residual in and the split-K slices out;
  // one-launch form: + r_old, H delta in and eta, H eta, r, z through once (7 r k doubles)
  *bytes = sparse_precond ? sp.bytes_per_apply(m.r)
           : !bc_split    ? 8.0 * m.k * (double)m.k + 7.0 * 8.0 * m.r * m.k
                          : 8.0 * m.k * (double)m.k + 8.0 * m.r * m.k + 8.0 * m.r * m.k * fused_nsplit(m);
  return DCORA_OK;
}
}  // namespace dcora
