// What the one-launch B + C (k_fused_pc, fused_step.hip) and the one-launch tCG run (k_tcg_run, fused_run.hip) share:
// the 16-byte buffer load, the 16-lane row sum, the workgroup shape and the LDS sizes of the residual image.  Host
// side, at the end: the sizes both launch functions compute (fused_pc_pb, pc_chunk) and LdsGrant, the per-device grant
// of a kernel's dynamic LDS (hipFuncSetAttribute on the kernel pointer its caller names).
#pragma once
#include <algorithm>
#include <atomic>

#include "kernels.h"

namespace dcora {

namespace {

// 16-byte buffer load: one descriptor (SGPRs) per array, per-lane byte offset in ONE VGPR, the uniform part of the
// address in an SGPR -- instead of a 64-bit VGPR address per load in flight; out-of-range dwords read as zero
typedef unsigned pc_v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ double2 pc_ld16(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {
  const pc_v4u v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0);
  return __builtin_bit_cast(double2, v);
}
// sum over each 16-lane row, same value in the row's lanes (the DPP half of wave_sum_dpp)
__device__ __forceinline__ double row16_sum_dpp(double v) {
  v += dpp_move<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_move<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_move<0x141>(v);  // row_half_mirror
  v += dpp_move<0x140>(v);  // row_mirror
  return v;
}
constexpr int kPcBlock = 256;  // 4 waves: wave w takes the 128-column steps w, w + 4, ... of ALL the workgroup's rows
constexpr int kPcNW = kPcBlock / 64;
constexpr int kPcSB = 25;      // 16-byte loads of each staged operand in flight per thread and batch
constexpr int kPcLoads = 32;   // 16-byte loads of the inverse's rows in flight per lane and batch

// poses per workgroup of the one-launch B + C: about one workgroup per CU at the headline size
inline int fused_pc_pb(const ManiDesc &m) { return m.n <= 768 ? 2 : 4; }
constexpr int kPcLdsCap = 128 * 1024;  // residual chunk in LDS: as many 128-column steps as fit (all of it at k = 2000)
inline int pc_chunk(const ManiDesc &m, int ldm) { return std::min((kPcLdsCap / (8 * m.r)) / 128 * 128, ldm); }

// The dynamic-LDS limit is an attribute of (function, DEVICE): it is set once per device the instantiation runs on
// (one bit per device; a process drives R GPUs from R host threads, SURVEY 8(b) threading).  One LdsGrant per kernel
// instantiation, kept by the launch function that names the kernel.  false: no usable device, or this device refuses
// the attribute and `need` bytes exceed the limit the kernel has without it.
struct LdsGrant {
  std::atomic<unsigned long long> tried{0}, ok{0};
  bool granted(const void *kernel, size_t need, size_t default_limit) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    const unsigned long long bit = 1ull << dev;
    if (!(tried.load(std::memory_order_acquire) & bit)) {
      const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kPcLdsCap);
      if (e == hipSuccess)
        ok.fetch_or(bit, std::memory_order_release);
      else
        (void)hipGetLastError();
      tried.fetch_or(bit, std::memory_order_release);
    }
    return (ok.load(std::memory_order_acquire) & bit) || need <= default_limit;
  }
};

}  // namespace

}  // namespace dcora
