// qvc_launch_util.h -- launch-side helper shared by the .hip translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdint>
#include <type_traits>
#include "../../include/qvc.h"

namespace qvc {

// One-time (per kernel AND per device) opt-in for more than 64 KiB of dynamic LDS.  `done` is a per-kernel static
// bit mask over device ordinals: a process that drives several GPUs must set the attribute on each of them, and
// two host threads racing here just set it twice.  Not a stream operation, so it is legal during graph capture.
inline bool allow_big_lds(std::atomic<uint32_t>& done, const void* kernel) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  const uint32_t bit = 1u << (dev & 31);
  if (done.load(std::memory_order_acquire) & bit) return true;
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return false;
  done.fetch_or(bit, std::memory_order_release);
  return true;
}

// Launch `kern` with `lds` bytes of dynamic LDS: the opt-in above (its per-kernel mask lives here, one instance per
// kernel pointer), the launch and the status check.  Kernels whose usual tile fits the default 64 KiB pass that as
// `optin_above` and take the opt-in for the larger tiles only.
template <auto kern, typename Args>
inline int launch_big_lds(dim3 grid, dim3 block, size_t lds, hipStream_t stream, const Args& args, size_t optin_above = 0) {
  static std::atomic<uint32_t> lds_ok{0};
  if (lds > optin_above && !allow_big_lds(lds_ok, reinterpret_cast<const void*>(kern))) return QVC_ERR_LAUNCH;
  hipLaunchKernelGGL(kern, grid, block, lds, stream, args);
  return hipGetLastError() == hipSuccess ? QVC_OK : QVC_ERR_LAUNCH;
}

// lift<V...>(v, f): f(std::integral_constant<int, V>{}) for the V that equals v -- a run-time integer becomes a template
// argument.  QVC_ERR_BAD_CONFIG when v is none of them.
template <int... V, class F>
inline int lift(int v, F&& f) {
  int st = QVC_ERR_BAD_CONFIG;
  (void)((v == V && ((st = f(std::integral_constant<int, V>{})), true)) || ...);
  return st;
}

}  // namespace qvc
