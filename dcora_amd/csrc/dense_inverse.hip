// Dense triangular inverses on the device over a job list (dense_tiles.h): the inverses of the pieces of the
// multifrontal factor (device_chol.hip hands its mid and wide pieces here) and the dense preconditioner
// (device_chol.h: device_dense_spd_inverse and its batch), with the recycled scratch arenas the builds carve.
//
// From a factored front [L11; L21] (leading dimension f): YT = (L11^-1)^T right-looking by block rows -- kept
// transposed, upper block triangular, so that every product runs over contiguous rows of both operands --,
// W = -L21 L11^-1 into the piece's packed panel under L11^-1, and M = L11^-T L11^-1 = YT YT^T.  For the dense
// preconditioner (ref src/QuadraticProblem.cpp:70-84 applied as an explicit inverse) the whole matrix is one front
// without rows below, A = L L^T by the panel kernels of device_chol.hip, and M is A^-1.
#include "dense_tiles.h"
#include "env.h"

#include <chrono>
#include <mutex>

namespace dcora {

namespace {

__global__ __launch_bounds__(256) void k_dense_scatter(int k, const int *__restrict__ rp, const int *__restrict__ ci,
                                                       const double *__restrict__ v, double *__restrict__ A) {
  const int i = blockIdx.x;
  for (int p = rp[i] + threadIdx.x; p < rp[i + 1]; p += 256) {
    const int j = ci[p];
    if (j <= i) A[(size_t)i * k + j] = v[p];
  }
}

// inverse of the 64 x 64 diagonal blocks of L11, one workgroup per block (blockIdx.x)
__global__ __launch_bounds__(256) void k_tri_inv64(const InvJob *__restrict__ jobs, const double *__restrict__ F,
                                                   double *__restrict__ Linv) {
  const InvJob J = jobs[blockIdx.z];
  const int b0 = blockIdx.x * NB;
  if (b0 >= J.c) return;  // (the grid is sized for the widest piece)
  __shared__ double T[NB][NB + 1];
  __shared__ double Li[NB][NB + 1];
  const double *__restrict__ L = F + J.l11;
  const int nb = min(NB, J.c - b0);
  const int tid = threadIdx.x;
  for (int e = tid; e < NB * NB; e += 256) {
    const int i = e >> 6, j = e & 63;
    T[i][j] = (i < nb && j <= i) ? L[(long long)(b0 + i) * J.f + b0 + j] : (i == j ? 1.0 : 0.0);
  }
  tri_inv64_lds(T, Li);
  double *__restrict__ O = Linv + J.tinv + (size_t)blockIdx.x * NB * NB;
  for (int e = tid; e < NB * NB; e += 256) O[e] = Li[e >> 6][e & 63];
}

// Y = L^-1 right-looking, one block row of L at a time; Y is kept transposed (YT(j, i) = Y(i, j)^T).  Step ib:
//   finish:  YT(j, ib) = -TT(j, ib) Linv_ib^T for the block rows j < ib (TT accumulated in place), YT(ib, ib) = Linv_ib^T
//   update:  TT(j, i) += YT(j, ib) L(i, ib)^T for every block row i > ib and j <= ib  -- (nb - ib - 1)(ib + 1) tiles
// tstride: 64 x 64 blocks between the inverses of consecutive diagonal blocks -- 1, or the batch size when the potrf of a
// batch of equal matrices stored them panel by panel
__global__ __launch_bounds__(256) void k_dense_trtri_finish(const InvJob *__restrict__ jobs, int ib,
                                                            double *__restrict__ YTs, const double *__restrict__ Linv,
                                                            int tstride) {
  const InvJob J = jobs[blockIdx.z];
  const int k = J.c, i0 = ib * NB;
  if (i0 >= k) return;
  __shared__ double As[NB][NB + 1];
  __shared__ double Bs[NB][NB + 1];
  double *__restrict__ YT = YTs + J.yt;
  const int tid = threadIdx.x;
  const int ni = min(NB, k - i0);
  const double *__restrict__ Li = Linv + J.tinv + (size_t)ib * NB * NB * tstride;
  if ((int)blockIdx.x == ib) {  // diagonal block: the transpose of the inverse of the diagonal block of L
    for (int e = tid; e < NB * NB; e += 256) {
      const int a = e >> 6, b = e & 63;
      if (a < ni && b < ni) YT[(size_t)(i0 + a) * k + i0 + b] = Li[b * NB + a];
    }
    return;
  }
  const int j0 = blockIdx.x * NB;
  for (int e = tid; e < NB * NB; e += 256) {
    const int a = e >> 6, mm = e & 63;
    As[mm][a] = (mm < ni) ? YT[(size_t)(j0 + a) * k + i0 + mm] : 0.0;  // TT(a, m)
    Bs[mm][a] = Li[a * NB + mm];                                       // Linv(b = a, m)
  }
  __syncthreads();
  double acc[4][4];
  zero_acc(acc);
  tile_inner(As, Bs, acc);
  for_each_acc(acc, [&](int a, int b, double s) {
    if (b < ni) YT[(size_t)(j0 + a) * k + i0 + b] = -s;
  });
}
__global__ __launch_bounds__(256) void k_dense_trtri_update(const InvJob *__restrict__ jobs, int ib,
                                                            const double *__restrict__ F, double *__restrict__ YTs) {
  const InvJob J = jobs[blockIdx.z];
  const int k = J.c, i0 = (ib + 1 + blockIdx.x) * NB, j0 = blockIdx.y * NB, l0 = ib * NB;
  if (i0 >= k) return;
  __shared__ double As[NB][NB + 1];
  __shared__ double Bs[NB][NB + 1];
  double *__restrict__ YT = YTs + J.yt;
  const int ni = min(NB, k - i0);
  double acc[4][4];
  zero_acc(acc);
  tile_product_range(YT + (size_t)j0 * k, k, NB, F + J.l11 + (size_t)i0 * J.f, J.f, ni, l0, l0 + NB, As, Bs, acc);
  for_each_acc(acc, [&](int a, int mm, double s) {
    if (mm < ni) YT[(size_t)(j0 + a) * k + i0 + mm] += s;
  });
}

// M = Y^T Y = YT YT^T: tile (ta, tb), tb <= ta, sums over the columns l >= block ta; both triangles are written
__global__ __launch_bounds__(256) void k_dense_lauum(const InvJob *__restrict__ jobs, const double *__restrict__ YTs,
                                                     double *__restrict__ Ms) {
  const InvJob J = jobs[blockIdx.z];
  if (J.mt < 0) return;
  int ta = (int)((sqrtf(8.0f * (float)blockIdx.x + 1.0f) - 1.0f) * 0.5f);
  while ((ta + 1) * (ta + 2) / 2 <= (int)blockIdx.x) ++ta;
  while (ta * (ta + 1) / 2 > (int)blockIdx.x) --ta;
  const int tb = blockIdx.x - ta * (ta + 1) / 2;
  const int k = J.c, ldm = J.ldm, a0 = ta * NB, b0 = tb * NB;
  if (a0 >= k) return;
  __shared__ double As[NB][NB + 1];
  __shared__ double Bs[NB][NB + 1];
  const double *__restrict__ YT = YTs + J.yt;
  double *__restrict__ M = Ms + J.mt;
  const int na = min(NB, k - a0), nb = min(NB, k - b0);
  double acc[4][4];
  zero_acc(acc);
  tile_product_range(YT + (size_t)a0 * k, k, na, YT + (size_t)b0 * k, k, nb, a0, k, As, Bs, acc);
  for_each_acc(acc, [&](int ar, int bc, double s) {
    const int a = a0 + ar, b = b0 + bc;
    if (a < k && b < k) {
      M[(size_t)a * ldm + b] = s;
      M[(size_t)b * ldm + a] = s;
    }
  });
}

// rows [c, c + m) of the piece's packed panel <- W(a, j) = -sum_{l >= j0} L21(a, l) YT(j, l): tile (ta over the m rows
// below, tj over the c columns)
__global__ __launch_bounds__(256) void k_piece_w(const InvJob *__restrict__ jobs, const double *__restrict__ F,
                                                 const double *__restrict__ YTs, double *__restrict__ packed) {
  const InvJob J = jobs[blockIdx.z];
  const int c = J.c, m = J.m, a0 = blockIdx.x * NB, j0 = blockIdx.y * NB;
  if (a0 >= m || j0 >= c) return;
  __shared__ double As[NB][NB + 1];
  __shared__ double Bs[NB][NB + 1];
  const double *__restrict__ B = F + J.l11 + (long long)c * J.f;
  const double *__restrict__ YT = YTs + J.yt;
  double *__restrict__ W = packed + J.pk + (long long)c * c;
  const int na = min(NB, m - a0), nj = min(NB, c - j0);
  double acc[4][4];
  zero_acc(acc);
  tile_product_range(B + (long long)a0 * J.f, J.f, na, YT + (long long)j0 * c, c, nj, j0, c, As, Bs, acc);
  for_each_acc(acc, [&](int ar, int jc, double s) {
    const int a = a0 + ar, j = j0 + jc;
    if (a < m && j < c) W[(long long)a * c + j] = -s;
  });
}
// rows [0, c) of the piece's packed panel <- L11^-1 (lower; = YT transposed)
__global__ __launch_bounds__(256) void k_piece_pack_inverted(const InvJob *__restrict__ jobs,
                                                             const double *__restrict__ YTs,
                                                             double *__restrict__ packed) {
  const InvJob J = jobs[blockIdx.z];
  const int c = J.c;
  const double *__restrict__ YT = YTs + J.yt;
  double *__restrict__ out = packed + J.pk;
  const long long n = (long long)c * c;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    const int i = (int)(e / c), j = (int)(e - (long long)i * c);
    out[e] = j <= i ? YT[(long long)j * c + i] : 0.0;
  }
}

}  // namespace

void enqueue_inverse_jobs(hipStream_t st, const InvBatch &b) {
  if (b.count <= 0) return;
  const unsigned nj = (unsigned)b.count;
  const int nbk = (b.cmax + NB - 1) / NB;
  const dim3 wg(256);
  if (b.diag_inverses) hipLaunchKernelGGL(k_tri_inv64, dim3(nbk, 1, nj), wg, 0, st, b.jobs, b.F, b.tinv);
  // (a failed factorisation leaves garbage behind its flag: the products below are harmless, the caller drops them)
  for (int ib = 0; ib < nbk; ++ib) {
    hipLaunchKernelGGL(k_dense_trtri_finish, dim3(ib + 1, 1, nj), wg, 0, st, b.jobs, ib, b.yt, (const double *)b.tinv,
                       b.tstride);
    if (ib + 1 < nbk)
      hipLaunchKernelGGL(k_dense_trtri_update, dim3(nbk - ib - 1, ib + 1, nj), wg, 0, st, b.jobs, ib, b.F, b.yt);
  }
  if (b.want_panel) {
    if (b.mmax > 0)
      hipLaunchKernelGGL(k_piece_w, dim3((b.mmax + NB - 1) / NB, nbk, nj), wg, 0, st, b.jobs, b.F, (const double *)b.yt,
                         b.packed);
    // about 4096 workgroups in all, at least 64 per piece
    const long long want = ((long long)b.cmax * b.cmax + 255) / 256, cap = std::max(64u, 4096u / nj);
    hipLaunchKernelGGL(k_piece_pack_inverted, dim3((unsigned)std::min(want, cap), 1, nj), wg, 0, st, b.jobs,
                       (const double *)b.yt, b.packed);
  }
  if (b.want_m)
    hipLaunchKernelGGL(k_dense_lauum, dim3(nbk * (nbk + 1) / 2, 1, nj), wg, 0, st, b.jobs, (const double *)b.yt, b.M);
}

// Scratch arenas of the dense builds, recycled process-wide: hipFree of a few hundred MB takes milliseconds (and waits for
// the device), and sessions are created again and again (staircase levels, GNC rounds).  At most two idle arenas per
// process are kept; chol_cache_clear() drops them.
namespace {
std::mutex g_scratch_mu;
struct Scratch {
  int device;
  size_t bytes;
  char *p;
};
std::vector<Scratch> g_scratch_idle;
}  // namespace
char *scratch_acquire(int device, size_t bytes) {
  {
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    for (size_t i = 0; i < g_scratch_idle.size(); ++i)
      if (g_scratch_idle[i].device == device && g_scratch_idle[i].bytes >= bytes &&
          g_scratch_idle[i].bytes <= 4 * bytes + (64u << 20)) {
        char *p = g_scratch_idle[i].p;
        g_scratch_idle.erase(g_scratch_idle.begin() + (long)i);
        return p;
      }
  }
  char *p = nullptr;
  if (hipMalloc((void **)&p, bytes) != hipSuccess) return nullptr;
  return p;
}
void scratch_release(int device, char *p, size_t bytes) {
  if (!p) return;
  {
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    if (g_scratch_idle.size() < 2) {
      g_scratch_idle.push_back(Scratch{device, bytes, p});
      return;
    }
  }
  (void)hipFree(p);
}
void scratch_clear() {
  std::lock_guard<std::mutex> lk(g_scratch_mu);
  for (Scratch &s : g_scratch_idle) (void)hipFree(s.p);
  g_scratch_idle.clear();
}
namespace {
std::mutex g_pinned_mu;
struct Pinned {
  size_t bytes;
  char *p;
};
std::vector<Pinned> g_pinned_idle;
}  // namespace
char *pinned_acquire(size_t bytes) {
  bytes = (bytes + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
  {
    std::lock_guard<std::mutex> lk(g_pinned_mu);
    for (size_t i = 0; i < g_pinned_idle.size(); ++i)
      if (g_pinned_idle[i].bytes >= bytes && g_pinned_idle[i].bytes <= 4 * bytes) {
        char *p = g_pinned_idle[i].p;
        g_pinned_idle.erase(g_pinned_idle.begin() + (long)i);
        return p;
      }
  }
  char *p = nullptr;
  if (hipHostMalloc((void **)&p, bytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return p;
}
void pinned_release(char *p, size_t bytes) {
  if (!p) return;
  bytes = (bytes + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
  {
    std::lock_guard<std::mutex> lk(g_pinned_mu);
    if (bytes <= ((size_t)32 << 20) && g_pinned_idle.size() < 3) {  // (large ones go back: pinned memory is the host's)
      g_pinned_idle.push_back(Pinned{bytes, p});
      return;
    }
  }
  (void)hipHostFree(p);
}

// The dense inverse of a BATCH of matrices of equal size in one set of launches (the agents of a session: five chains of
// ~130 small dependent launches on five streams do not overlap on this part -- the hardware runs two or three queues at a
// time, tools/stream_overlap.hip -- so five builds took 20 ms where one takes 3.5).  Every kernel takes a list / job
// index: potrf one workgroup per matrix, the panel kernels a grid dimension over the matrices.  The arithmetic per
// matrix does not depend on the batch: a matrix built alone (the batch of one) gets the same bits.
int device_dense_spd_inverse_batch(const std::vector<const HostCsr *> &As, int device, const std::vector<double *> &Minv,
                                   int ldm, std::vector<char> *pd) {
  const int B = (int)As.size();
  if (B == 0) return DCORA_OK;
  const int k = As[0]->n;
  for (const HostCsr *A : As)
    if (A->n != k) {
      set_last_error("dense inverse batch: matrices of different sizes");
      return DCORA_ERR_BAD_ARG;
    }
  const auto t_in = std::chrono::steady_clock::now();
  DCORA_HIP(hipSetDevice(device));
  StreamLease lease(device);
  const int rc = lease.acquire();
  if (rc) return rc;
  hipStream_t st = lease.st;
  const int nb = (k + NB - 1) / NB;
  const size_t kk = (size_t)k * k;
  size_t nnz_max = 1;
  for (const HostCsr *A : As) nnz_max = std::max(nnz_max, A->ci.size());
  // one allocation for everything (hipMalloc / hipFree synchronise the device: agents are set up concurrently)
  struct Arena {
    int device;
    size_t bytes = 0;
    char *p = nullptr;
    ~Arena() { scratch_release(device, p, bytes); }
  } arena{device};
  auto carve = [&](size_t bytes) {  // offsets first (p is null), pointers once the arena is there
    const size_t at = arena.bytes;
    arena.bytes += (bytes + 15) & ~(size_t)15;
    return at;
  };
  const size_t o_L = carve(B * kk * 8), o_YT = carve(B * kk * 8), o_tinv = carve((size_t)B * nb * NB * NB * 8),
               o_v = carve(B * nnz_max * 8), o_logdet = carve(8), o_piece = carve(sizeof(PieceDev) * B),
               o_jobs = carve(sizeof(InvJob) * B), o_rp = carve((size_t)B * (k + 1) * 4), o_ci = carve(B * nnz_max * 4),
               o_fail = carve(4), o_list = carve(4 * (size_t)B);
  arena.p = scratch_acquire(device, arena.bytes);
  if (!arena.p) {
    set_last_error("dense inverse: out of device memory");
    return DCORA_ERR_HIP;
  }
  double *L = (double *)(arena.p + o_L), *YT = (double *)(arena.p + o_YT), *tinv = (double *)(arena.p + o_tinv),
         *v = (double *)(arena.p + o_v), *logdet = (double *)(arena.p + o_logdet);
  int *rp = (int *)(arena.p + o_rp), *ci = (int *)(arena.p + o_ci), *fail = (int *)(arena.p + o_fail),
      *list = (int *)(arena.p + o_list);
  PieceDev *piece = (PieceDev *)(arena.p + o_piece);
  InvJob *jobs = (InvJob *)(arena.p + o_jobs);
  std::vector<PieceDev> hp((size_t)B);
  std::vector<InvJob> hj((size_t)B);
  std::vector<int> hl((size_t)B);
  double *Mbase = Minv[0];
  for (double *q : Minv) Mbase = std::min(Mbase, q);
  for (int b = 0; b < B; ++b) {
    hp[(size_t)b] = PieceDev{(long long)(b * kk), k, 0, -1, 0};
    hj[(size_t)b] = InvJob{k, 0, ldm, (long long)(b * kk), (long long)k, (long long)(b * kk), (long long)b * NB * NB, 0,
                          (long long)(Minv[(size_t)b] - Mbase)};
    hl[(size_t)b] = b;
    const HostCsr &A = *As[(size_t)b];
    DCORA_HIP(hipMemcpyAsync(rp + (size_t)b * (k + 1), A.rp.data(), ((size_t)k + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    DCORA_HIP(hipMemcpyAsync(ci + (size_t)b * nnz_max, A.ci.data(), A.ci.size() * sizeof(int), hipMemcpyHostToDevice, st));
    DCORA_HIP(hipMemcpyAsync(v + (size_t)b * nnz_max, A.v.data(), A.ci.size() * sizeof(double), hipMemcpyHostToDevice, st));
    DCORA_HIP(hipMemsetAsync(Minv[(size_t)b], 0, (size_t)k * ldm * sizeof(double), st));
  }
  DCORA_HIP(hipMemcpyAsync(piece, hp.data(), sizeof(PieceDev) * B, hipMemcpyHostToDevice, st));
  DCORA_HIP(hipMemcpyAsync(jobs, hj.data(), sizeof(InvJob) * B, hipMemcpyHostToDevice, st));
  DCORA_HIP(hipMemcpyAsync(list, hl.data(), sizeof(int) * B, hipMemcpyHostToDevice, st));
  DCORA_HIP(hipMemsetAsync(L, 0, o_tinv, st));  // L and YT of every matrix
  DCORA_HIP(hipMemsetAsync(fail, 0, sizeof(int), st));
  DCORA_HIP(hipMemsetAsync(logdet, 0, sizeof(double), st));
  for (int b = 0; b < B; ++b)
    hipLaunchKernelGGL(k_dense_scatter, dim3(k), dim3(256), 0, st, k, rp + (size_t)b * (k + 1), ci + (size_t)b * nnz_max,
                       v + (size_t)b * nnz_max, L + b * kk);
  enqueue_dense_potrf(st, piece, list, B, k, L, tinv, B, fail, logdet);  // panel p of matrix b at (p B + b) blocks
  InvBatch batch;
  batch.jobs = jobs;
  batch.count = B;
  batch.cmax = k;
  batch.F = L;
  batch.yt = YT;
  batch.tinv = tinv;
  batch.M = Mbase;
  batch.tstride = B;
  batch.diag_inverses = false;
  batch.want_panel = false;
  enqueue_inverse_jobs(st, batch);
  DCORA_HIP(hipGetLastError());
  int failed = 0;
  DCORA_HIP(hipMemcpyAsync(&failed, fail, sizeof(int), hipMemcpyDeviceToHost, st));
  DCORA_HIP(hipStreamSynchronize(st));
  // (one flag for the batch: a failure anywhere stops every later launch, the caller then builds one by one)
  pd->assign((size_t)B, failed == 0 ? 1 : 0);
  if (env::init_timing())
    fprintf(stderr, "[dense inverse] batch of %d (k = %d) in %.2f ms\n", B, k,
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_in).count());
  return DCORA_OK;
}

int device_dense_spd_inverse(const HostCsr &A, int device, double *Minv, int ldm, bool *pd) {
  std::vector<char> verdict;
  const int rc = device_dense_spd_inverse_batch({&A}, device, {Minv}, ldm, &verdict);
  if (rc == DCORA_OK) *pd = verdict[0] != 0;
  return rc;
}

}  // namespace dcora
