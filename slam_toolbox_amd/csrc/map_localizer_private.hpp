// What map_localizer.cpp (kh_map_localizer_*) shares with map_align.cpp (kh_map_align, section 7m): the handle
// and the fit on its work buffers.  Not part of the public ABI (include/karto_hip.h).
#pragma once
#include "map_localize_plan.hpp"
#include "mapper_private.hpp"

struct kh_map_localizer
{
  kh_mapper_params p;
  kh::mapper::Laser laser;
  int32_t device = 0, max_batch = 1;
  kh_matcher * loop = nullptr;         // MapperGraph's loop matcher (Mapper.cpp:1397-1400)
  kh_matcher * seq = nullptr;          // Mapper::Initialize's sequential matcher (Mapper.cpp:2606-2631)
  kh::MapWork * work = nullptr;
  kh_map_view view;
  bool has_map = false, has_pose = false;
  kh::mapper::Pose robot, odometric;   // the pose the localizer holds, and the odometric pose it belongs to
  kh_map_localizer_stats_t stats;
};

namespace kh
{
// k_map_fit of the readings at n sensor poses against the localizer's map, on its own work buffers: counts takes kFitCounters sums
// per pose
int localizer_fit_counts(kh_map_localizer * loc, const double * ranges, size_t n, const double * poses, uint64_t * counts, double * kernel_ms);
}  // namespace kh
