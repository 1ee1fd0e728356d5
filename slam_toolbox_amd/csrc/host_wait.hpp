// Host-side waiting (host code only): the spin-loop hint, and the wait for a kernel's "result ready" flag in host-coherent memory.
#pragma once

#include <cstdint>

#if defined(__x86_64__) || defined(__i386__)
#define KH_CPU_PAUSE() __builtin_ia32_pause()
#else
#include <thread>
#define KH_CPU_PAUSE() std::this_thread::yield()
#endif

// (host_pool.hpp takes the pause only, and is also built by a plain C++ compiler: the flag wait needs the HIP runtime)
#ifdef __HIPCC__
#include <hip/hip_runtime_api.h>

namespace kh
{

enum class FlagWait {kRaised, kDrained, kFailed};

// Spins until `*flag == value`.  The kernel stores its results and then raises the flag (release, system scope); the acquire load
// here keeps the caller's reads of those results behind it.  The stream is asked every 16384 spins so that a failed launch cannot
// hang the caller: kDrained = it finished without raising the flag, kFailed = it reported an error (`*error`).
inline FlagWait wait_device_flag(const int32_t * flag, int32_t value, hipStream_t stream, hipError_t * error = nullptr)
{
  uint64_t spins = 0;
  while (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != value) {
    KH_CPU_PAUSE();
    if ((++spins & 0x3fff) == 0) {
      const hipError_t e = hipStreamQuery(stream);
      if (e == hipSuccess) {return __atomic_load_n(flag, __ATOMIC_ACQUIRE) == value ? FlagWait::kRaised : FlagWait::kDrained;}
      if (e != hipErrorNotReady) {
        if (error) {*error = e;}
        return FlagWait::kFailed;
      }
    }
  }
  return FlagWait::kRaised;
}

}  // namespace kh
#endif
