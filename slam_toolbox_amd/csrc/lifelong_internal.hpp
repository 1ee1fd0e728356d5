// What lifelong.hip offers the mapper besides the public kh_lifelong_* calls.  Not part of the public ABI (include/karto_hip.h).
#pragma once
#include <cstdint>

#include "../../include/karto_hip.h"

namespace kh
{
// kh_lifelong_scores, and the form the mapper's node decay calls (resident != nullptr): candidate k's UNFILTERED readings already
// lie in HBM at resident[k] (n_scan of them) and masks[k] holds one bit per reading, set where the reading passed the range filter
int decay_scores(int32_t device, const kh_scan_box * reference, int32_t n, const kh_scan_box * candidates, const double * const * resident,
  const uint64_t * const * masks, int32_t n_scan, const kh_decay_params * params, int32_t * kept, double * iou, double * area_overlap,
  double * reading_overlap, double * scores);
}  // namespace kh
