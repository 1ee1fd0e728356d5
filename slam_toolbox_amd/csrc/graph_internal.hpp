// What graph.hip offers the mapper besides the public kh_graph_* calls: the forms that work on the caller's vectors.  Not part of
// the public ABI (include/karto_hip.h).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/karto_hip.h"

namespace kh
{
// kh_graph_set without the copies (the mapper's sync_graph): the store takes the caller's arrays and hands its old ones back
int graph_swap(kh_graph * g, int32_t n_scans, std::vector<double> & ref_xy, std::vector<int32_t> & adj_ptr, std::vector<int32_t> & adj_idx,
  std::vector<double> & pose_xy);
// kh_graph_relocalize_candidates with vectors for the answer (kh_mapper_relocalize); the arguments have been checked by the caller
int graph_relocalize_candidates(kh_graph * g, double seed_spacing, double base_radius, int32_t max_base, const double * center_xy, double radius,
  std::vector<int32_t> & seeds, std::vector<int32_t> & base_begin, std::vector<int32_t> & base_idx);
}  // namespace kh
