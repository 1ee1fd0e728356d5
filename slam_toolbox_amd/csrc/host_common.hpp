// What every host file of libkartohip uses of the others: the last-error text, the persistent host pools and the two device calls
// the HIP-free files make.  Needs no HIP header (spa_symbolic.cpp is also built alone on the CPU).  Not part of the public ABI
// (include/karto_hip.h).
#pragma once
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>

namespace kh
{
void set_error(const std::string & s);                                            // matcher_host.cpp: the thread's kh_last_error text
// the persistent host pools (host_pool.hpp, instantiated by matcher_host.cpp): fn(i) for i in [0, n), back when all are done
void host_parallel_for(size_t n, const std::function<void(size_t)> & fn);
void host_parallel_for_wide(size_t n, const std::function<void(size_t)> & fn);
// matcher_host.cpp: scan points at these poses -- kh_scan_points (n_beams libm sincos) per sensor pose, on the wide pool.  Pose k (3
// doubles) places readings ranges + k * ranges_stride (0: the same readings at every pose) into points + 2 * n_beams * k; sensor_xy,
// unless nullptr, takes the pose's (x, y).
void scan_points_at(const double * ranges, size_t ranges_stride, int32_t n_beams, double min_angle, double angular_resolution, size_t n_poses,
  const double * sensor_poses, double * points, double * sensor_xy);
// comm.cpp: waits for everything queued on the HIP stream
void stream_synchronize(void * hip_stream);
// comm.cpp: KH_OK when `device` can be used, otherwise KH_ERR_NO_DEVICE and its text; require_device(0) asks for any device at all
int require_device(int32_t device);
// wall time in milliseconds: from a to b, and from t to now
inline double ms_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b)
{
  return std::chrono::duration<double, std::milli>(b - a).count();
}
inline double ms_since(std::chrono::steady_clock::time_point t) {return ms_between(t, std::chrono::steady_clock::now());}
}  // namespace kh
