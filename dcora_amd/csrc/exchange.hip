// Neighbour exchange of public poses between the ranks of one node (see exchange.h).
#include "exchange.h"
#include "env.h"

#include <fcntl.h>
#include <signal.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

namespace dcora {

namespace {

static_assert(sizeof(hipIpcMemHandle_t) == sizeof(ShmRank::halo), "ShmRank stores the IPC handle as 64 bytes");
constexpr int kMaxDst = 8;
struct PostDst {
  double *base[kMaxDst];
  int n;
};

// getSharedStateDicts of one agent, written where its neighbours read it: element i of the packed r x (d+1)count
// block goes to every destination slot (the peers' halo buffers over xGMI, or the shared host segment); the
// workgroup that finishes last publishes the sequence number.  Every storing wave drains its stores and the
// workgroup's lane 0 releases at system scope before it arrives (MI355X_MICROARCH.md, valid producer forms).
__global__ __launch_bounds__(kBlock) void k_post_public(int r, int ncols, const int *__restrict__ src,
                                                        const double *__restrict__ X, PostDst dst, PostDst dflag,
                                                        unsigned *arrive, volatile uint64_t *flag, uint64_t seq) {
  const long N = (long)ncols * r;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < N; i += (long)gridDim.x * kBlock) {
    const int c = (int)(i / r), t = (int)(i - (long)c * r);
    const double v = X[(size_t)src[c] * r + t];
    for (int q = 0; q < dst.n; ++q) dst.base[q][i] = v;
  }
  __threadfence_system();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned prev = atomicAdd(arrive, 1u);
    if (prev == gridDim.x - 1) {
      __hip_atomic_store(arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __threadfence_system();
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      // the flag word next to each destination's slot (what that rank's scatter kernel polls), then the host-visible one
      for (int q = 0; q < dflag.n; ++q)
        __hip_atomic_store((uint64_t *)dflag.base[q], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store((uint64_t *)flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// updateNeighborStates on the consumer's side, with the wait inside: lane 0 of every workgroup polls the flag word
// (system-scope relaxed loads, s_sleep between polls; bounded -- a producer that never arrives raises `failed` and the
// kernel ends), one system-scope acquire, then the slot is read with system-scope loads and scattered into the mirror of
// X.  The workgroup that finishes last tells the producer that the slot has been read (back-pressure of post()).
constexpr long long kWaitBudgetTicks = 20LL * 100000000LL;  // 20 s of the 100 MHz wall clock
__global__ __launch_bounds__(kBlock) void k_wait_scatter(int r, int ncols, const int *__restrict__ cols,
                                                         const double *src, double *__restrict__ X,
                                                         const uint64_t *flag, uint64_t want, unsigned *arrive,
                                                         uint64_t *consumed, uint32_t *failed) {
  __shared__ int s_bad;
  if (threadIdx.x == 0) {
    int bad = 0;
    const long long t0 = wall_clock64();
    while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < want) {
      __builtin_amdgcn_s_sleep(16);
      if (wall_clock64() - t0 > kWaitBudgetTicks ||
          __hip_atomic_load(failed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0) {
        bad = 1;
        break;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_bad = bad;
  }
  __syncthreads();
  if (s_bad) {
    if (threadIdx.x == 0) __hip_atomic_store(failed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  const long N = (long)ncols * r;
  for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < N; i += (long)gridDim.x * kBlock) {
    const int c = (int)(i / r), t = (int)(i - (long)c * r);
    X[(size_t)cols[c] * r + t] = __hip_atomic_load(src + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned prev = atomicAdd(arrive, 1u);
    if (prev == gridDim.x - 1) {
      __hip_atomic_store(arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(consumed, want, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// the hosted agents' two evaluation scalars into the shared segment: the device store is the all-gather
__global__ void k_eval_publish(int nh, const int *__restrict__ hosted, const double *__restrict__ ev, ShmEval *slots,
                               uint64_t seq) {
  const int i = threadIdx.x;
  if (i < nh) {
    const int a = hosted[i];
    ShmEval *e = slots + a;
    __hip_atomic_store((double *)&e->g2, ev[2 * a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store((double *)&e->xeg, ev[2 * a + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store((uint64_t *)&e->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

__global__ void k_selftest_write(double *dst, int count, double base) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) dst[i] = base + i;
  __threadfence_system();
}

// ---- link check (Exchange::link_check): the producer / consumer forms of k_post_public / k_wait_scatter on a 4 KB
//      probe, one workgroup each ----
__global__ __launch_bounds__(256) void k_probe_post(double *dst, uint64_t *dflag, volatile uint64_t *hflag, double base,
                                                    uint64_t seq) {
  for (int i = threadIdx.x; i < kProbeDoubles; i += 256) dst[i] = base + i;
  __threadfence_system();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence_system();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (dflag) __hip_atomic_store(dflag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store((uint64_t *)hflag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
// result: 1 = flag seen and every word equal, 2 = the flag never came (budget), 3 = words differ
__global__ __launch_bounds__(256) void k_probe_wait(const double *src, const uint64_t *flag, uint64_t want,
                                                    long long budget_ticks, int poll, double base, int *result) {
  __shared__ int s_bad, s_diff;
  if (threadIdx.x == 0) {
    int bad = 0;
    s_diff = 0;
    if (poll) {
      const long long t0 = wall_clock64();
      while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < want) {
        __builtin_amdgcn_s_sleep(16);
        if (wall_clock64() - t0 > budget_ticks) {
          bad = 1;
          break;
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    s_bad = bad;
  }
  __syncthreads();
  if (s_bad) {
    if (threadIdx.x == 0) __hip_atomic_store(result, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  int diff = 0;
  for (int i = threadIdx.x; i < kProbeDoubles; i += 256)
    diff += __hip_atomic_load(src + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != base + i;
  if (diff) atomicAdd(&s_diff, diff);
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(result, s_diff ? 3 : 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// start time of a process in clock ticks since boot (field 22 of /proc/<pid>/stat), 0 when it cannot be read
uint64_t proc_start_time(int pid) {
  char path[64], buf[1024];
  std::snprintf(path, sizeof path, "/proc/%d/stat", pid);
  FILE *fp = std::fopen(path, "r");
  if (!fp) return 0;
  const size_t n = std::fread(buf, 1, sizeof buf - 1, fp);
  std::fclose(fp);
  buf[n] = 0;
  const char *p = std::strrchr(buf, ')');  // the command may hold spaces and parentheses: fields resume behind the last ')'
  if (!p) return 0;
  int field = 2;
  for (++p; *p; ++p)
    if (*p == ' ' && ++field == 22) return std::strtoull(p + 1, nullptr, 10);
  return 0;
}
// is the creator of a segment still the process that wrote the header?
bool creator_alive(const ShmHeader *h) {
  if (h->creator_pid <= 0) return false;
  if (!(kill((pid_t)h->creator_pid, 0) == 0 || errno == EPERM)) return false;
  const uint64_t now = proc_start_time(h->creator_pid);
  return now == 0 || h->creator_start == 0 || now == h->creator_start;  // (no /proc: the pid test alone)
}

}  // namespace

double exchange_timeout_s() { return env::exchange_timeout_s(); }

std::atomic<int> g_probe_fault_rounds{0};

int Exchange::usage(const std::string &msg, int code) {
  set_last_error("exchange (rank " + std::to_string(rank) + "): " + msg);
  return code;
}

int Exchange::fail(const std::string &msg, int code) {
  set_last_error("exchange (rank " + std::to_string(rank) + "): " + msg);
  if (hdr_) hdr_->failed.store(1);
  return code;
}

int Exchange::wait_failed(int what, const std::string &who) {
  return fail(what == kWaitPeerFailed ? std::string("another rank failed") : who, DCORA_ERR_HIP);
}

int Exchange::num_peers() const {
  std::set<int> p;
  for (const auto &v : dests_) p.insert(v.begin(), v.end());
  return (int)p.size();
}

Exchange::~Exchange() {
  if (s_) (void)hipSetDevice(s_->opt.device);
  if (team_on()) {  // the team's status area and weights go with the segment: the session goes on without a team
    (void)hipStreamSynchronize(s_->st);
    s_->team.reset();
  }
  for (int q = 0; q < kMaxRanks; ++q)
    if (opened_[q] && peer_halo_[q]) (void)hipIpcCloseMemHandle(peer_halo_[q]);
  if (registered_ && map_) (void)hipHostUnregister(map_);
  if (map_) munmap(map_, lay_.total);
  if (rank == 0 && !name_.empty()) shm_unlink(name_.c_str());
}

// Rank 0 removes whatever carries the name, creates the segment and publishes the magic word last; the others attach
// once it is there.  A rank that opened the name BEFORE rank 0 replaced it holds a stale segment (a crashed job, a reused
// job name): it recognises that by the creator's process being gone or by the name resolving to another inode by now,
// drops the mapping and opens the name again.  Two LIVE jobs under one name on one node remain a caller's error.
int Exchange::open_segment(const char *job_name) {
  const size_t bytes = lay_.total;
  name_ = std::string("/dcora_") + job_name;
  const auto t0 = Clock::now();
  if (rank == 0) {
    shm_unlink(name_.c_str());
    const int fd = shm_open(name_.c_str(), O_CREAT | O_EXCL | O_RDWR, 0600);
    if (fd < 0) return fail("shm_open(create " + name_ + ") failed: " + std::strerror(errno), DCORA_ERR_IO);
    if (ftruncate(fd, (off_t)bytes) != 0) {
      close(fd);
      return fail("ftruncate failed: " + std::string(std::strerror(errno)), DCORA_ERR_IO);
    }
    map_ = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (map_ == MAP_FAILED) {
      map_ = nullptr;
      return fail("mmap failed: " + std::string(std::strerror(errno)), DCORA_ERR_IO);
    }
    hdr_ = (ShmHeader *)map_;
    std::memset(map_, 0, bytes);
    hdr_->world = (uint32_t)world;
    hdr_->R = (uint32_t)R_;
    hdr_->slot_doubles = slot_;
    hdr_->total_bytes = bytes;
    hdr_->creator_pid = (int32_t)getpid();
    hdr_->creator_start = proc_start_time((int)getpid());
    hdr_->magic.store(kShmMagic, std::memory_order_release);
    return DCORA_OK;
  }
  for (;;) {
    if (since(t0) > exchange_timeout_s()) return fail("segment " + name_ + " did not appear", DCORA_ERR_IO);
    const int fd = shm_open(name_.c_str(), O_RDWR, 0600);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0 || (size_t)sb.st_size < bytes) {
      // a segment of another size under the name: a live job of another shape says so in its header (a stale one, or
      // one rank 0 is still creating, is waited out)
      if (fd >= 0 && (size_t)sb.st_size >= sizeof(ShmHeader)) {
        void *hp = mmap(nullptr, sizeof(ShmHeader), PROT_READ, MAP_SHARED, fd, 0);
        if (hp != MAP_FAILED) {
          ShmHeader *h = (ShmHeader *)hp;
          const bool live = h->magic.load(std::memory_order_acquire) == kShmMagic && creator_alive(h);
          const bool other = live && (h->world != (uint32_t)world || h->R != (uint32_t)R_ || h->slot_doubles != slot_ ||
                                      h->total_bytes != bytes);
          if (other && since(t0) > 1.0) {  // (a second: a crashed job's segment is replaced by rank 0 within that)
            // a LOCAL error only: the segment belongs to somebody else's live job and is not written to (raising its
            // `failed` word took that healthy job down); this job's other ranks time out on DCORA_EXCHANGE_TIMEOUT_S
            munmap(hp, sizeof(ShmHeader));
            close(fd);
            return fail("segment " + name_ + " belongs to a job of another shape (a live job under the same name?)",
                        DCORA_ERR_BAD_ARG);
          }
          munmap(hp, sizeof(ShmHeader));
        }
      }
      if (fd >= 0) close(fd);
      usleep(2000);
      continue;
    }
    void *mp = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (mp == MAP_FAILED) return fail("mmap failed: " + std::string(std::strerror(errno)), DCORA_ERR_IO);
    ShmHeader *h = (ShmHeader *)mp;
    bool good = false;
    const auto t1 = Clock::now();
    while (since(t1) < 0.25) {  // a fresh segment is initialised within microseconds of its creation
      if (h->magic.load(std::memory_order_acquire) == kShmMagic) {
        good = true;
        break;
      }
      usleep(500);
    }
    if (good) {
      // still the segment the name stands for, and its creator is alive?
      struct stat now;
      const int fd2 = shm_open(name_.c_str(), O_RDONLY, 0600);
      const bool same = fd2 >= 0 && fstat(fd2, &now) == 0 && now.st_ino == sb.st_ino && now.st_dev == sb.st_dev;
      if (fd2 >= 0) close(fd2);
      good = same && creator_alive(h);
    }
    if (!good) {
      munmap(mp, bytes);
      usleep(2000);
      continue;
    }
    if (h->world != (uint32_t)world || h->R != (uint32_t)R_ || h->slot_doubles != slot_ || h->total_bytes != bytes) {
      h->failed.store(1);  // the job's other ranks give up as well instead of waiting for this one
      munmap(mp, bytes);
      return fail("segment " + name_ + " belongs to a job of another shape (a live job under the same name?)",
                  DCORA_ERR_BAD_ARG);
    }
    map_ = mp;
    hdr_ = h;
    return DCORA_OK;
  }
}

int Exchange::map_segment(const char *job_name, size_t x_doubles, size_t w_doubles) {
  lay_ = SegmentLayout(world, R_, slot_, x_doubles, w_doubles);
  return open_segment(job_name);
}

int Exchange::barrier(double timeout_s) {
  const int rc = slots().barrier(timeout_s);
  return rc ? wait_failed(rc, "barrier timed out") : DCORA_OK;
}

int Exchange::init(SessionCore *s, const char *job_name, size_t weights) {
  s_ = s;
  s->exchange_attached = true;  // (from here on the session lifts through this exchange only, within its reserve)
  rank = s->opt.rank;
  world = s->opt.world_size;
  R_ = s->R;
  const int R = R_;
  if (world > kMaxRanks) return fail("too many ranks", DCORA_ERR_UNSUPPORTED);
  if (!job_name || !*job_name) return fail("empty job name", DCORA_ERR_BAD_ARG);
  DCORA_HIP(hipSetDevice(s->opt.device));
  const int per = (R + world - 1) / world;
  owner_.resize(R);
  size_t maxcols = 1;
  std::vector<int> hosted;
  for (int a = 0; a < R; ++a) {
    const AgentCore &v = s->agent_core(a);
    owner_[a] = a / per;
    maxcols = std::max(maxcols, (size_t)v.n_public_cols);
    if (v.hosted) hosted.push_back(a);
    if (v.hosted != (owner_[a] == rank)) return fail("agent-to-rank map out of step with the session", DCORA_ERR_BAD_ARG);
  }
  n_hosted_ = (int)hosted.size();
  // (slots and the X area by the larger of the session's rank and its reserve: room for Exchange::lift)
  r_cap_ = SegmentLayout::rank_capacity(s->r, s->reserve_r);
  lay_ = SegmentLayout::for_job(world, R, maxcols, s->r, s->reserve_r, (size_t)s->num_cols(), weights);
  slot_ = lay_.slot;
  dests_.assign(R, {});
  needed_.assign(R, 0);
  for (int a = 0; a < R; ++a) {
    const AgentCore &va = s->agent_core(a);
    for (int q : va.neighbors) {
      const AgentCore &vq = s->agent_core(q);
      if (va.hosted && owner_[q] != rank && std::find(dests_[a].begin(), dests_[a].end(), owner_[q]) == dests_[a].end())
        dests_[a].push_back(owner_[q]);
      if (!va.hosted && vq.hosted) needed_[a] = 1;
    }
  }
  for (int a = 0; a < R; ++a)
    if ((int)dests_[a].size() > kMaxDst) return fail("an agent has neighbours on more than 8 other ranks", DCORA_ERR_UNSUPPORTED);
  seq_.assign(R, 0);

  int rc = open_segment(job_name);  // (of lay_: the job's layout, above)
  if (rc) return rc;
  {
    const hipError_t e = hipHostRegister(map_, lay_.total, hipHostRegisterMapped | hipHostRegisterPortable);
    if (e != hipSuccess) return fail(std::string("hipHostRegister of the shared segment failed: ") + hipGetErrorString(e), DCORA_ERR_HIP);
    registered_ = true;
    DCORA_HIP(hipHostGetDevicePointer((void **)&dev_map_, map_, 0));
  }
  DCORA_HIP(arrive_.alloc(R));
  DCORA_HIP(hipMemset(arrive_.p, 0, sizeof(unsigned) * R));
  DCORA_HIP(arrive2_.alloc(R));
  DCORA_HIP(hipMemset(arrive2_.p, 0, sizeof(unsigned) * R));
  {
    char bus[64] = {0};
    uint64_t h = 1469598103934665603ull;
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), s->opt.device) != hipSuccess) {
      (void)hipGetLastError();
      std::snprintf(bus, sizeof(bus), "device-%d", s->opt.device);
    }
    for (const char *c = bus; *c; ++c) h = (h ^ (uint64_t)(unsigned char)*c) * 1099511628211ull;
    rank_record(rank).bus.store(h ? h : 1, std::memory_order_release);
  }
  DCORA_HIP(evalbuf_.alloc(2 * R));
  DCORA_HIP(hipMemset(evalbuf_.p, 0, sizeof(double) * 2 * R));
  DCORA_HIP(hosted_list_.alloc(std::max(1, n_hosted_)));
  if (n_hosted_)
    DCORA_HIP(hipMemcpy(hosted_list_.p, hosted.data(), sizeof(int) * n_hosted_, hipMemcpyHostToDevice));

  const char *force = env::exchange();
  const bool want_ipc = !(force && std::strcmp(force, "staged") == 0);
  int ok = 1;
  if (world > 1) {
    rc = setup_ipc(want_ipc);
    if (rc != DCORA_OK && rc != DCORA_ERR_UNSUPPORTED) return rc;
    ok = rc == DCORA_OK;
  }
  rank_record(rank).ipc_ok.store(ok ? 1 : -1, std::memory_order_release);
  int rc2 = barrier();
  if (rc2) return rc2;
  bool all = true;
  for (int q = 0; q < world; ++q) all = all && rank_record(q).ipc_ok.load(std::memory_order_acquire) == 1;
  mode = all ? kExchangeIpc : kExchangeStaged;
  {
    // Who waits for a producer's flag.  With a GPU of its own the consumer's scatter kernel polls the flag itself: no
    // host hop between the producer's stores and the scatter.  Ranks SHARING a GPU (the rehearsal on one device) keep
    // the host's wait: a kernel that polls occupies the queue the producer's kernels of the other process need --
    // measured with 4 ranks on one MI355X: 875 against 1084 it/s on the headline, 274 against 664 on the 100k lattice.
    // DCORA_EXCHANGE_WAIT=device / host forces one or the other.
    bool shared_gpu = false;
    for (int q = 0; q < world; ++q)
      if (q != rank && rank_record(q).bus.load(std::memory_order_acquire) == rank_record(rank).bus.load()) shared_gpu = true;
    // A peer GPU's stores into a COARSE-grained halo buffer are not guaranteed visible to a kernel of this GPU that is
    // already running (lines may be served from the local L2; the host-wait form relies on the invalidate of the
    // kernel boundary): the kernel polls only where every rank's halo is fine-grained device memory.
    bool all_fine = true;
    for (int q = 0; q < world; ++q) all_fine = all_fine && rank_record(q).fine.load(std::memory_order_acquire) == 1;
    const bool poll_is_safe = mode != kExchangeIpc || all_fine;
    const char *wm = env::exchange_wait();
    device_wait_ = (wm ? std::strcmp(wm, "host") != 0 : !shared_gpu) && poll_is_safe;
  }
  if (force && std::strcmp(force, "ipc") == 0 && !all) return fail("DCORA_EXCHANGE=ipc but the IPC transport is not usable", DCORA_ERR_HIP);
  rc = barrier();
  if (rc) return rc;
  if (world > 1) {
    rc = link_check();
    if (rc) return rc;
  }
  rc = barrier();
  if (rc) return rc;
  if (rank == 0) shm_unlink(name_.c_str());  // every rank has it mapped: nothing is left in /dev/shm after the job
  return DCORA_OK;
}

// Halo buffers mapped into every rank that writes to them, then one round of test stores checked by the owner.
// Every rank passes the same two barriers whatever fails locally; the result is this rank's vote.
int Exchange::setup_ipc(bool attempt) {
  const int R = R_;
  const size_t test_off = 2 * (size_t)R * slot_;
  const int ntest = 64;
  devflag_off_ = align_up(test_off + (size_t)ntest * world, 8);
  probe_off_ = devflag_off_ + 2 * (size_t)R * 8;  // behind one 64-byte flag word per (parity, agent)
  const size_t halo_doubles = probe_off_ + (size_t)world * (kProbeDoubles + 8);  // + the link check's area per writer
  bool ok = attempt;
  std::string why;
  auto no = [&](const std::string &m) {
    if (ok) why = m;
    ok = false;
  };
  // The halo buffer is written by OTHER GPUs while this GPU's kernels read it launch after launch: fine-grained device
  // memory (not cached incoherently in this GPU's L2), so that a slot re-used two posts later is never served stale;
  // plain hipMalloc if the runtime refuses (the self-test below still has to pass).
  if (ok) {
    const size_t bytes = sizeof(double) * halo_doubles;
    void *hp = nullptr;
    if (hipExtMallocWithFlags(&hp, bytes, hipDeviceMallocFinegrained) == hipSuccess && hp) {
      halo_.p = (double *)hp;  // released with hipFree like any DevBuf
      halo_.n = halo_doubles;
      halo_finegrained_ = true;
    } else {
      (void)hipGetLastError();
      if (halo_.alloc(halo_doubles) != hipSuccess) no("hipMalloc of the halo buffer");
    }
  }
  if (ok && hipMemset(halo_.p, 0, sizeof(double) * halo_doubles) != hipSuccess) no("hipMemset");
  hipIpcMemHandle_t mine;
  if (ok && hipIpcGetMemHandle(&mine, halo_.p) != hipSuccess) {
    (void)hipGetLastError();
    if (halo_finegrained_) {  // a runtime that exports no handle for fine-grained memory: once more with plain hipMalloc
      halo_.release();
      halo_finegrained_ = false;
      if (halo_.alloc(halo_doubles) != hipSuccess ||
          hipMemset(halo_.p, 0, sizeof(double) * halo_doubles) != hipSuccess ||
          hipIpcGetMemHandle(&mine, halo_.p) != hipSuccess)
        no("hipIpcGetMemHandle");
    } else {
      no("hipIpcGetMemHandle");
    }
  }
  (void)hipGetLastError();
  if (ok) std::memcpy(rank_record(rank).halo, &mine, sizeof(mine));
  rank_record(rank).device.store(s_->opt.device);
  rank_record(rank).pid.store((int)getpid());
  rank_record(rank).fine.store(ok && halo_finegrained_ ? 1 : 0);
  rank_record(rank).published.store(ok ? 1 : -1, std::memory_order_release);
  int rc = barrier();
  if (rc) return rc;
  // whom do I write to: the owners of my hosted agents' neighbours
  std::set<int> peers;
  for (int a = 0; a < R; ++a) peers.insert(dests_[a].begin(), dests_[a].end());
  for (int q : peers) {
    if (!ok) break;
    if (rank_record(q).published.load(std::memory_order_acquire) != 1) {
      no("rank " + std::to_string(q) + " has no halo handle");
      break;
    }
    const int pd = rank_record(q).device.load();
    if (pd != s_->opt.device) {
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, s_->opt.device, pd) == hipSuccess && can) {
        const hipError_t e = hipDeviceEnablePeerAccess(pd, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) no("hipDeviceEnablePeerAccess");
      }
      (void)hipGetLastError();
    }
    void *p = nullptr;
    hipIpcMemHandle_t h;
    std::memcpy(&h, rank_record(q).halo, sizeof(h));
    if (hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
      (void)hipGetLastError();
      no("hipIpcOpenMemHandle of rank " + std::to_string(q));
      break;
    }
    peer_halo_[q] = (double *)p;
    opened_[q] = true;
  }
  // self-test: a pattern into my strip of every peer's test area, checked by the owner after the barrier
  if (ok) {
    for (int q : peers)
      hipLaunchKernelGGL(k_selftest_write, dim3(1), dim3(64), 0, s_->st,
                         peer_halo_[q] + test_off + (size_t)ntest * rank, ntest, 1000.0 * (rank + 1));
    if (hipStreamSynchronize(s_->st) != hipSuccess) no("self-test stores");
    (void)hipGetLastError();
  }
  rc = barrier();
  if (rc) return rc;
  if (ok) {
    std::vector<double> h((size_t)ntest * world);
    if (hipMemcpy(h.data(), halo_.p + test_off, sizeof(double) * h.size(), hipMemcpyDeviceToHost) != hipSuccess)
      no("reading the self-test area");
    std::set<int> writers;  // ranks hosting an agent whose public poses I need
    for (int a = 0; a < R; ++a)
      if (needed_[a]) writers.insert(owner_[a]);
    for (int q : writers)
      for (int i = 0; i < ntest && ok; ++i)
        if (h[(size_t)ntest * q + i] != 1000.0 * (q + 1) + i) no("self-test pattern of rank " + std::to_string(q) + " did not arrive");
  }
  if (!ok && attempt)
    set_last_error("exchange: IPC transport unavailable (" + why + "), the ranks use the shared host segment");
  return ok ? DCORA_OK : DCORA_ERR_UNSUPPORTED;
}

// One round of the link check: a 4 KB pattern and a flag from every rank into each rank it will write to, through the
// transport (mode) and the form of the wait (device_wait_) in force; true when everything THIS rank reads arrived intact
// within the budget.  Never blocks longer than a few seconds whatever a peer does.
bool Exchange::probe_round(uint64_t seq, std::string *why) {
  const int R = R_;
  const bool ipc = mode == kExchangeIpc;
  std::set<int> peers, writers;
  for (int a = 0; a < R; ++a) {
    peers.insert(dests_[a].begin(), dests_[a].end());
    if (needed_[a]) writers.insert(owner_[a]);
  }
  auto pattern = [&](int writer, int reader) { return 1e6 * (double)seq + 4096.0 * writer + 64.0 * reader; };
  auto hflag_dev = [&](int reader, int writer) { return &lay_.probe_flag(dev_map_, reader, writer)->seq; };
  bool ok = true;
  auto no = [&](const std::string &m) {
    if (ok && why) *why = m;
    ok = false;
  };
  if (hipSetDevice(s_->opt.device) != hipSuccess) no("hipSetDevice");
  hipStream_t st = s_->st;
  for (int q : peers) {
    if (!ok) break;
    double *dst = ipc ? peer_halo_[q] + probe_off_ + (size_t)rank * (kProbeDoubles + 8)
                      : lay_.probe_stage(dev_map_, q, rank);
    uint64_t *dflag = ipc ? (uint64_t *)(peer_halo_[q] + probe_off_ + (size_t)rank * (kProbeDoubles + 8) + kProbeDoubles) : nullptr;
    if (ipc && !peer_halo_[q]) {
      no("no mapping of rank " + std::to_string(q) + "'s halo buffer");
      break;
    }
    hipLaunchKernelGGL(k_probe_post, dim3(1), dim3(256), 0, st, dst, dflag, hflag_dev(q, rank), pattern(rank, q), seq);
  }
  if (hipGetLastError() != hipSuccess) no("probe post launch");
  const double budget_s = 3.0;
  for (int p : writers) {
    if (!ok) break;
    // the host waits for the flag, as wait_arr does; on its own budget, and giving up is this rank's vote only
    if (!device_wait_ && slots().wait(budget_s).reached(lay_.probe_flag(map_, rank, p)->seq, seq)) {
      no("the probe flag of rank " + std::to_string(p) + " never arrived (host wait)");
      break;
    }
    const double *src = ipc ? halo_.p + probe_off_ + (size_t)p * (kProbeDoubles + 8)
                            : lay_.probe_stage(dev_map_, rank, p);
    const uint64_t *flag = ipc ? (const uint64_t *)(halo_.p + probe_off_ + (size_t)p * (kProbeDoubles + 8) + kProbeDoubles)
                               : (const uint64_t *)hflag_dev(rank, p);
    int *res = (int *)lay_.probe_result(dev_map_, rank, p);
    hipLaunchKernelGGL(k_probe_wait, dim3(1), dim3(256), 0, st, src, flag, seq, (long long)(budget_s * 1e8),
                       device_wait_ ? 1 : 0, pattern(p, rank), res);
  }
  if (hipGetLastError() != hipSuccess) no("probe wait launch");
  // the stream drains within the kernels' own budgets; a bounded host wait on top (never hipStreamSynchronize blindly)
  {
    const auto w0 = Clock::now();
    hipError_t e;
    while ((e = hipStreamQuery(st)) == hipErrorNotReady) {
      usleep(200);
      if (since(w0) > 4.0 * budget_s) {
        no("the probe kernels did not finish");
        break;
      }
    }
    if (e != hipSuccess && e != hipErrorNotReady) {
      (void)hipGetLastError();
      no(std::string("probe kernels: ") + hipGetErrorString(e));
    }
  }
  for (int p : writers) {
    if (!ok) break;
    const volatile int *res = (const volatile int *)lay_.probe_result(map_, rank, p);
    if (*res != 1)
      no("probe of rank " + std::to_string(p) + (*res == 2 ? ": the flag never arrived" : *res == 3 ? ": the 4 KB pattern arrived damaged" : ": no result"));
    *(volatile int *)res = 0;
  }
  return ok;
}

// Start-up check of the links this rank will use (dcora_hip.h, dcora_exchange_info): rounds of probe_round, all ranks
// stepping down together -- device-side wait -> host wait -> staged transport -- until a round passes on every rank.
int Exchange::link_check() {
  std::string why, first_why;
  // test hook (dcora_debug_exchange_probe_fault): the last rank reports its first n rounds as failed
  const int fault_rounds = g_probe_fault_rounds.load();
  for (int round = 1; round <= 3; ++round) {
    const auto t0 = Clock::now();
    bool mine = probe_round((uint64_t)round, &why);
    if (mine && rank == world - 1 && round <= fault_rounds) {
      mine = false;
      why = "injected fault (dcora_debug_exchange_probe_fault)";
    }
    if (!mine && first_why.empty()) first_why = why;
    // the vote carries the form of the wait this rank used (device_wait_ is rank-local: only ranks with a GPU of their
    // own poll on the device), so that the step down below is taken from SHARED state and is the same on every rank
    const int vote = 2 * round + (device_wait_ ? 1 : 0);
    rank_record(rank).probe.store(mine ? vote : -vote, std::memory_order_release);
    int rc = barrier(30.0);
    if (rc) return rc;
    bool all = true, any_device_wait = false;
    for (int q = 0; q < world; ++q) {
      const int v = rank_record(q).probe.load(std::memory_order_acquire);
      all = all && v > 0 && v / 2 == round;
      any_device_wait = any_device_wait || ((v < 0 ? -v : v) & 1);
    }
    rc = barrier(30.0);  // nobody overwrites its vote before everybody has read the votes
    if (rc) return rc;
    link_rounds = round;
    link_last_us = 1e6 * since(t0);
    if (all) {
      if (round > 1)
        set_last_error("exchange: link check passed after stepping down (" + first_why + "): " +
                       (mode == kExchangeIpc ? "IPC peer stores, host wait" : "shared host segment"));
      return DCORA_OK;
    }
    // the same step on every rank: it depends on the votes and on `mode` only (identical everywhere), never on this
    // rank's own device_wait_ -- ranks that share a GPU wait on the host from the start while the others poll on the
    // device, and a ladder keyed on the local flag sent them to different rungs (mixed transports, a spurious
    // DCORA_ERR_EXCHANGE_LINK): device wait anywhere -> host wait everywhere -> staged with host wait everywhere
    if (any_device_wait) {
      if (device_wait_) link_gave_up_device_wait = 1;
      device_wait_ = false;
    } else if (mode == kExchangeIpc) {
      const char *force = env::exchange();
      if (force && std::strcmp(force, "ipc") == 0) break;  // (the environment of a job is the same on its ranks)
      mode = kExchangeStaged;
      link_gave_up_ipc = 1;
    } else {
      break;
    }
  }
  return fail("link check: no transport between the ranks works (" + (first_why.empty() ? why : first_why) + ")",
              DCORA_ERR_EXCHANGE_LINK);
}

int Exchange::post(const int *agents, int count) { return post_arr(agents, count, s_->r, s_->Xg.p); }
int Exchange::wait(const int *agents, int count) { return wait_arr(agents, count, s_->r, s_->Xg.p); }

// the same exchange for any r x (d+1)n array laid out like X (the certificate's vectors: r = 1)
int Exchange::post_arr(const int *agents, int count, int r, const double *arr) {
  const auto t0 = Clock::now();
  DCORA_HIP(hipSetDevice(s_->opt.device));
  const int R = R_;
  const ExchangeSlots sl = slots();
  for (int i = 0; i < count; ++i) {
    const int a = agents[i];
    if (a < 0 || a >= R) return usage("post: agent out of range", DCORA_ERR_BAD_ARG);
    const uint64_t q = ++seq_[a];
    const AgentCore &ag = s_->agent_core(a);
    if (!ag.hosted || dests_[a].empty() || ag.n_public_cols == 0) continue;
    const int parity = (int)(q & 1);
    // back-pressure (ExchangeSlots::consumed_wait): post q - 2, the slot's last, has been scattered by all its readers
    int whom = 0;
    if (const int rc = sl.consumed_wait(sl.wait(), a, q, dests_[a].data(), (int)dests_[a].size(), &whom))
      return wait_failed(rc, "rank " + std::to_string(whom) + " never read post " + std::to_string(q - 2) +
                                 " of agent " + std::to_string(a));
    PostDst dst{}, dflag{};
    if (mode == kExchangeIpc) {
      for (int p : dests_[a]) {
        dst.base[dst.n++] = peer_halo_[p] + halo_off(parity, a);
        dflag.base[dflag.n++] = peer_halo_[p] + devflag_off_ + ((size_t)parity * R + a) * 8;
      }
    } else {
      dst.base[dst.n++] = lay_.staged(dev_map_, parity, a);
    }
    const int ncols = ag.n_public_cols;
    const long N = (long)ncols * r;
    const int grid = (int)std::min<long>((N + kBlock - 1) / kBlock, 64);
    volatile uint64_t *flag = &lay_.flag(dev_map_, parity, a)->seq;
    hipLaunchKernelGGL(k_post_public, dim3(grid), dim3(kBlock), 0, s_->st, r, ncols, ag.public_cols.p, arr, dst,
                       dflag, arrive_.p + a, flag, q);
    bytes_posted += 8.0 * N * dst.n;
    ++posts;
  }
  DCORA_HIP(hipGetLastError());
  post_s += since(t0);
  return DCORA_OK;
}

int Exchange::wait_arr(const int *agents, int count, int r, double *arr) {
  const auto t0 = Clock::now();
  DCORA_HIP(hipSetDevice(s_->opt.device));
  const int R = R_;
  const ExchangeSlots sl = slots();
  for (int i = 0; i < count; ++i) {
    const int a = agents[i];
    if (a < 0 || a >= R) return usage("wait: agent out of range", DCORA_ERR_BAD_ARG);
    const AgentCore &ag = s_->agent_core(a);
    if (!needed_[a] || ag.n_public_cols == 0) continue;
    const uint64_t want = seq_[a];
    const int parity = (int)(want & 1);
    // DCORA_EXCHANGE_WAIT=host: the host waits for the flag, the kernel below finds it set
    if (!device_wait_)
      if (const int rc = sl.flag_wait(sl.wait(), a, want))
        return wait_failed(rc, "public poses of agent " + std::to_string(a) + " never arrived");
    const bool ipc = mode == kExchangeIpc;
    const double *src = ipc ? halo_.p + halo_off(parity, a) : lay_.staged(dev_map_, parity, a);
    // the flag the kernel polls: next to the slot in this rank's halo buffer (stored by the producer over xGMI), or the
    // host-visible word when the poses are staged in the shared segment
    const uint64_t *dflag = ipc ? (const uint64_t *)(halo_.p + devflag_off_ + ((size_t)parity * R + a) * 8)
                                : (const uint64_t *)&lay_.flag(dev_map_, parity, a)->seq;
    const int ncols = ag.n_public_cols;
    const long N = (long)ncols * r;
    const int grid = (int)std::min<long>((N + kBlock - 1) / kBlock, 32);
    uint64_t *cons = (uint64_t *)&lay_.consumed(dev_map_, rank, a)->seq;
    uint32_t *failed = (uint32_t *)&lay_.header(dev_map_)->failed;
    // updateNeighborStates: into the local mirror of X
    hipLaunchKernelGGL(k_wait_scatter, dim3(grid), dim3(kBlock), 0, s_->st, r, ncols, ag.public_cols.p, src,
                       arr, dflag, want, arrive2_.p + a, cons, failed);
    ++waits;
  }
  wait_s += since(t0);
  return DCORA_OK;
}

// distributed form of the central evaluation (ref examples/MultiRobotExample.cpp:264-305): every rank evaluates the
// agents it hosts against the neighbours' public poses it holds, publishes two scalars per agent, reads everybody's
int Exchange::evaluate(double *cost2, double *gradnorm, double *block_norms, int *next_selected) {
  int rc = s_->phase_evaluate_dev(evalbuf_.p);
  if (rc) return rc;
  const uint64_t want = ++eval_seq_;
  if (n_hosted_)
    hipLaunchKernelGGL(k_eval_publish, dim3(1), dim3(64), 0, s_->st, n_hosted_, hosted_list_.p, evalbuf_.p,
                       lay_.eval(dev_map_, (int)(want & 1), 0), want);
  DCORA_HIP(hipGetLastError());
  // the team's statuses of the round (rbcd_iterate): read once the evaluation is enqueued behind the agent's update, so
  // that the hosting rank's queue never drains while its host waits for its own kernel's word
  if (!team_due_.empty()) {
    const std::vector<int> due(std::move(team_due_));
    team_due_.clear();
    rc = team_collect(due.data(), (int)due.size());
    if (rc) return rc;
  }
  // the heartbeat and the gather (ExchangeSlots, where the argument for the heartbeat stands), on one clock
  const ExchangeSlots sl = slots();
  const Wait w = sl.wait();
  int whom = 0;
  if ((rc = sl.heartbeat(w, want, &whom)))
    return wait_failed(rc, "rank " + std::to_string(whom) + " never entered the evaluation");
  if ((rc = sl.eval_gather(w, want, cost2, gradnorm, block_norms, next_selected, &whom)))
    return wait_failed(rc, "evaluation of agent " + std::to_string(whom) + " never arrived");
  eval_wait_s += since(w.t0);
  ++evals;
  return DCORA_OK;
}

// one pass of the reference driver's loop body (examples/MultiRobotExample.cpp:223-307) across the ranks
int Exchange::rbcd_iterate(int selected, double *cost2, double *gradnorm, double *block_norms, int *next_selected) {
  const int R = R_;
  if (selected < 0 || selected >= R) return usage("selected agent out of range", DCORA_ERR_BAD_ARG);
  std::vector<int> others;
  for (int a = 0; a < R; ++a)
    if (a != selected) others.push_back(a);
  const bool team = team_on();
  const long launches0 = g_chain_launches.load(std::memory_order_relaxed);
  int rc = s_->phase_nonselected(selected);  // Agent::iterate(false) of the hosted non-selected agents
  if (rc) return rc;
  rc = post(others.data(), (int)others.size());
  if (rc) return rc;
  rc = wait(others.data(), (int)others.size());  // the selected agent's pull (and everybody's for the evaluation)
  if (rc) return rc;
  if (team && (rc = team_clear_to_write(&selected, 1))) return rc;
  rc = s_->phase_selected(selected);  // Agent::iterate(true) where the selected agent lives
  if (rc) return rc;
  if (team) s_->team_note_elsewhere(&selected, 1);
  rc = post(&selected, 1);
  if (rc) return rc;
  rc = wait(&selected, 1);
  if (rc) return rc;
  if (team) team_due_.assign(1, selected);  // collected inside evaluate, before its waits
  int nxt = selected;
  rc = evaluate(cost2, gradnorm, block_norms, &nxt);
  team_due_.clear();
  s_->chain_launches += g_chain_launches.load(std::memory_order_relaxed) - launches0;
  if (rc) return rc;
  if (next_selected) *next_selected = s_->agent_core(selected).neighbors.empty() ? selected : nxt;
  return DCORA_OK;
}

int Exchange::rbcd_tick(const int *set, int count, int allow_adjacent) {
  const bool team = team_on();
  int rc = DCORA_OK;
  // (a set the session is about to refuse touches no slot)
  bool valid = set && count >= 1 && count <= R_;
  for (int i = 0; valid && i < count; ++i) valid = set[i] >= 0 && set[i] < R_;
  if (team && valid && (rc = team_clear_to_write(set, count))) return rc;
  rc = s_->iterate_set(set, count, allow_adjacent);
  if (rc) return rc;
  if (team) s_->team_note_elsewhere(set, count);
  rc = post(set, count);
  if (rc) return rc;
  rc = wait(set, count);
  if (rc || !team) return rc;
  return team_collect(set, count);
}

// ---- the team protocol across the ranks (exchange.h) ----------------------------------------------------------------
void Exchange::team_snapshot_weights() {
  if (!lay_.w_doubles) return;
  std::atomic_thread_fence(std::memory_order_acquire);
  job_w_.resize(lay_.w_doubles);
  std::memcpy(job_w_.data(), lay_.weights(map_), sizeof(double) * lay_.w_doubles);
}

// The job's weights are complete in the area whenever no update is under way; the closing barrier keeps a rank that
// runs ahead from starting one (its kernel stores into the area) while another still copies.
int Exchange::team_enable(const dcora_team_params &p, bool range_aided) {
  const bool pose_graph = s_->kind() == SessionKind::PoseGraph;
  if (!pose_graph && !range_aided)
    return usage("team_enable: dcora_exchange_team_enable serves pose-graph sessions; a range-aided job enables its team "
                 "through dcora_exchange_team_enable_ra", DCORA_ERR_UNSUPPORTED);
  if (pose_graph && range_aided)
    return usage("team_enable: dcora_exchange_team_enable_ra serves range-aided sessions; a pose-graph job enables its "
                 "team through dcora_exchange_team_enable", DCORA_ERR_UNSUPPORTED);
  if (s_->weights_ranked() && lay_.w_doubles != s_->weights_count())
    return usage("team_enable: a robust session needs the exchange it was created with (dcora_rbcd_create_robust_ranks / "
                 "dcora_ra_rbcd_create_robust_ranks)", DCORA_ERR_UNSUPPORTED);
  team_snapshot_weights();
  const int rc = s_->team_enable_ranked(p, lay_.status(map_, 0, 0), lay_.status(dev_map_, 0, 0),
                                           lay_.w_doubles ? job_w_.data() : nullptr);
  if (rc) return rc;
  return barrier();
}

// optimisation q = seq + 1 of a hosted agent will store into slot [q & 1]: every rank has read q - 2 out of it
int Exchange::team_clear_to_write(const int *agents, int count) {
  const TeamState &t = *s_->team;
  const ExchangeSlots sl = slots();
  for (int i = 0; i < count; ++i) {
    const int a = agents[i];
    if (a < 0 || a >= R_ || !s_->agent_core(a).hosted) continue;
    const uint64_t q = t.seq[(size_t)a] + 1;
    if (q <= 2) continue;
    int whom = 0;
    if (const int rc = sl.status_read_wait(a, q - 2, &whom))
      return wait_failed(rc, "rank " + std::to_string(whom) + " never read status " + std::to_string(q - 2) +
                                 " of agent " + std::to_string(a));
  }
  return DCORA_OK;
}

int Exchange::team_collect(const int *agents, int count) {
  const TeamState &t = *s_->team;
  const ExchangeSlots sl = slots();
  for (int i = 0; i < count; ++i) {
    const int a = agents[i];
    const uint64_t q = t.seq[(size_t)a];
    if (const int rc = sl.status_wait(q, a))
      return wait_failed(rc, "the status of agent " + std::to_string(a) + " never arrived");
    const ShmStatus *slot = sl.status_slot(q, a);
    s_->team_settle_published(a, slot->success != 0, slot->rel);
    sl.mark_status_read(q, a);
  }
  return DCORA_OK;
}

// SessionCore::run_team across the ranks: the same loop of the same rules on every rank's copy of the statuses
int Exchange::run_team(int *iters_done, double *cost2_trace, double *gradnorm_trace, int *selected_trace,
                       int *updated_trace, int *weight_updates, int *stop_reason) {
  SessionCore &s = *s_;
  TeamState &t = *s.team;
  const int cap = t.params.max_num_iters;
  int selected = 0, it = 0, nupd = 0;
  for (;;) {
    int stop = 0, upd = 0;
    int rc = s.team_decide(&stop, &upd);
    if (rc) return rc;
    if (stop || it >= cap) break;
    if (updated_trace) updated_trace[it] = upd;
    if (upd) {
      const bool reset = t.resets_done < t.params.robust_opt_num_resets;
      int counts[3];
      rc = update_weights(reset, counts);
      if (rc) return rc;
      if (reset) t.resets_done++;
      nupd++;
    }
    double c2 = 0, gn = 0;
    int nxt = selected;
    rc = rbcd_iterate(selected, &c2, &gn, nullptr, &nxt);
    if (rc) return rc;
    if (cost2_trace) cost2_trace[it] = c2;
    if (gradnorm_trace) gradnorm_trace[it] = gn;
    if (selected_trace) selected_trace[it] = selected;
    selected = nxt;
    ++it;
  }
  if (iters_done) *iters_done = it;
  if (weight_updates) *weight_updates = nupd;
  if (stop_reason) *stop_reason = s.iteration >= cap ? DCORA_TEAM_STOP_MAX_ITERS : DCORA_TEAM_STOP_ALL_READY;
  return DCORA_OK;
}

int Exchange::run_coloured(int max_sweeps, double rgrad_tol, int *sweeps_done, double *cost2_trace,
                           double *gradnorm_trace) {
  std::vector<int> colours((size_t)R_, 0);
  int nc = 0;
  s_->agent_colours(colours.data(), &nc);
  return run_coloured_sweeps(
      colours, nc, [&](const int *set, int count) { return rbcd_tick(set, count, 0); },
      [&](double *c2, double *gn) { return evaluate(c2, gn, nullptr, nullptr); }, max_sweeps, rgrad_tol, sweeps_done,
      cost2_trace, gradnorm_trace);
}

int Exchange::set_X(const double *Xh) {
  int rc = barrier();
  if (rc) return rc;
  rc = s_->set_X(Xh);
  if (rc) return rc;
  return barrier();
}

// every rank's hosted blocks -> the shared segment -> every rank's copy of the whole X
int Exchange::gather_X(double *Xh) {
  int rc = s_->x_stage_hosted(lay_.x(map_));
  if (rc) return rc;
  rc = barrier();
  if (rc) return rc;
  std::memcpy(Xh, lay_.x(map_), sizeof(double) * (size_t)s_->r * (size_t)s_->num_cols());
  return barrier();
}

// Collective weight update (ref src/Agent.cpp:1397-1441 on every agent of every rank), in the single session's order:
// streams drained and the weights computed (compute_weights), the counts summed, the hosted matrices rebuilt,
// RobustCost::update, X back to the last set_X if asked, acceleration re-initialised.  A shared edge is weighted on
// both of its ranks from bitwise-equal mirror columns.  The weights area is written by the kernel while no rank reads
// it: get_weights ends with a barrier, and the allreduce below is passed only once every rank's stores have landed.
int Exchange::update_weights(bool reset_to_initial, int counts[3]) {
  SessionCore &s = *s_;
  if (!s.weights_ranked() || lay_.w_doubles != s.weights_count())
    return usage("update_weights: the exchange's session is not a ranked robust session", DCORA_ERR_BAD_ARG);
  std::vector<double> w;
  double cnt[3] = {0, 0, 0};
  int rc = s.compute_weights(lay_.weights(dev_map_), &w, cnt);
  if (rc) return fail(std::string("update_weights: ") + dcora_last_error(), rc);
  rc = allreduce_sum(cnt, 3);
  if (rc) return rc;
  if (team_on()) {
    // the team's loop-closure counts are of the whole job's weights: a copy of the area, complete now, and nobody
    // starts the next update (whose kernel stores into the area) before every rank has made its copy
    team_snapshot_weights();
    rc = barrier();
    if (rc) return rc;
  }
  if (reset_to_initial) {  // (every rank's mirror becomes the last set_X at once, as Exchange::set_X does)
    rc = barrier();
    if (rc) return rc;
  }
  rc = s.apply_weights(w, reset_to_initial);
  if (rc) return fail(std::string("update_weights: ") + dcora_last_error(), rc);
  if (reset_to_initial) {
    rc = barrier();
    if (rc) return rc;
  }
  for (int c = 0; c < 3; ++c) counts[c] = (int)cnt[c];
  return DCORA_OK;
}

// Every rank receives the same w, and the session's set_weights checks all of them before anything changes (negative
// or not finite, or nonzero where creation had 0): a refusal is the same on every rank and leaves the job as it was,
// with the exchange usable.  The owners then store their edges' weights into the area.
int Exchange::set_weights(const double *w) {
  SessionCore &s = *s_;
  if (!s.weights_ranked() || lay_.w_doubles != s.weights_count())
    return usage("set_weights: the exchange's session is not a ranked robust session", DCORA_ERR_BAD_ARG);
  // (the team's counts are refreshed from the job's weights inside: every rank is handed all m of them)
  std::vector<double> before;
  if (team_on()) {
    before = job_w_;
    std::copy(w, w + lay_.w_doubles, job_w_.begin());
  }
  const int rc = s.set_weights(w);
  if (rc && team_on()) std::copy(before.begin(), before.end(), job_w_.begin());
  if (rc == DCORA_ERR_BAD_ARG) return rc;  // (refused on every rank alike, nothing changed)
  if (rc) return fail(std::string("set_weights: ") + dcora_last_error(), rc);
  return publish_weights();
}

// the weights the session holds for the measurements this rank owns into the area (host stores), then a barrier
int Exchange::publish_weights() {
  if (!s_->weights_ranked() || lay_.w_doubles != s_->weights_count())
    return usage("publish_weights: the exchange's session is not a ranked robust session", DCORA_ERR_BAD_ARG);
  double *area = lay_.weights(map_);
  for (size_t e = 0; e < lay_.w_doubles; ++e) {
    double w = 0;
    if (s_->weight_owned(e, &w)) area[e] = w;
  }
  std::atomic_thread_fence(std::memory_order_release);
  return barrier();
}

int Exchange::get_weights(double *w) {
  if (lay_.w_doubles == 0) return usage("get_weights: the exchange was not created for a robust job", DCORA_ERR_BAD_ARG);
  std::atomic_thread_fence(std::memory_order_acquire);
  std::memcpy(w, lay_.weights(map_), sizeof(double) * lay_.w_doubles);
  return barrier();  // nobody writes the area again before every rank has read it
}

int Exchange::debug_leave_stale(const char *job_name, int world_, int R) {
  rank = 0;
  world = world_;
  R_ = R;
  slot_ = 16;
  const int rc = map_segment(job_name, 16);
  if (rc) return rc;
  hdr_->creator_pid = 0x7ffffff0;  // beyond any pid_max: nobody answers
  hdr_->bar_count.store(1);        // and its barrier stands as the crash left it
  name_.clear();                   // the destructor must not remove it
  return DCORA_OK;
}

// The host half of the protocol on its own (no device): the bootstrap through the segment, then exchange_rehearsal
// (exchange_slots.h) -- `rounds` rounds of back-pressure -> post -> flag wait -> evaluation heartbeat and gather -> sum
// over the ranks, the steps post_arr, wait_arr, evaluate and allreduce_sum make, with host stores in the device's place.
// checksum is identical on every rank.
int Exchange::host_selftest(const char *job_name, int rank_, int world_, int R, int rounds, double *checksum) {
  int rc = selftest_bootstrap(job_name, rank_, world_, R, rounds >= 1);
  if (rc) return rc;
  const char *what = "";
  rc = exchange_rehearsal(slots(), (R + world - 1) / world, rounds, checksum, &what);
  if (rc) return wait_failed(rc, what);
  return barrier();
}

// The team's half of the rehearsal (dcora_hip.h, dcora_exchange_host_selftest_team): team_rehearsal (exchange_slots.h)
// on this segment's status area -- the slots, sequence words, read words and waits of team_clear_to_write /
// team_collect, with host stores where the ranked k_rel_change stores -- behind the same bootstrap and the
// evaluation's heartbeat.
int Exchange::host_selftest_team(const char *job_name, int rank_, int world_, int R, int rounds, int skew_us,
                                 double *checksum) {
  int rc = selftest_bootstrap(job_name, rank_, world_, R, rounds >= 1 && skew_us >= 0);
  if (rc) return rc;
  rc = team_rehearsal(slots(), (R + world - 1) / world, rounds, skew_us, checksum);
  if (rc) return wait_failed(rc, "host selftest: a status, a read word or a heartbeat never arrived");
  return barrier();
}

// what both rehearsals share with init: the segment of a job of this shape, every rank attached, the name removed
int Exchange::selftest_bootstrap(const char *job_name, int rank_, int world_, int R, bool args_ok) {
  rank = rank_;
  world = world_;
  R_ = R;
  if (world < 1 || rank < 0 || rank >= world || world > kMaxRanks || R < 1 || R > kMaxAgents || !args_ok)
    return fail("host selftest: bad arguments", DCORA_ERR_BAD_ARG);
  slot_ = 16;
  int rc = map_segment(job_name, 16);
  if (rc) return rc;
  rc = barrier();
  if (rc) return rc;
  if (rank == 0) shm_unlink(name_.c_str());
  return DCORA_OK;
}

}  // namespace dcora
