// The query hook of kh_matcher_match / kh_matcher_match_batch, for callers inside the library that do not see matcher_private.hpp
// (the mapper's Process, the loop-closure batch of matcher_group.cpp).  Not part of the public ABI (include/karto_hip.h).
#pragma once
#include <functional>

namespace kh
{
// A caller inside the library (the mapper's Process) may leave the QUERY scan's readings unfinished when it calls kh_matcher_match
// and hand over the function that finishes them: the fused path runs it behind the rasteriser's launches -- which need the query's
// sensor pose and nothing else of it -- so that LocalizedRangeScan::Update of the new scan (1081 sincos: 15 us) runs while the GPU
// works; every other path runs it before it reads the query.  Per thread; consumed by the next kh_matcher_match_batch on the thread.
struct QueryHook
{
  std::function<void()> fn;
  void run() {if (fn) {std::function<void()> f; f.swap(fn); f();}}
};
QueryHook & pending_query_hook();                            // matcher_seq.cpp
void set_pending_query_hook(std::function<void()> fn);
void run_pending_query_hook();
}  // namespace kh
