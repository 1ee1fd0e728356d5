// The plan of a covariance-column pass as a plain function: which fronts of the assembly tree the forward
// sweep of A X = E_q visits, and which query columns each of them carries.  A query's right-hand side is non-zero in the pivot rows
// of the front that eliminates it; a forward sweep hands non-zeros to ancestors only, so per query exactly the fronts on the path
// from that front to its root are touched -- at most one per level, which is why every (row, column) of the right-hand sides has one
// writer per launch.  Nothing here knows HIP: spa_covariance.cpp plans with this before it queues anything on the device, and
// tests/covariance_columns_plan_check.cpp runs it on the CPU (tests/test_covariance_columns_plan.py).
#pragma once
#include <cstdint>
#include <vector>

namespace kh
{
constexpr int32_t kMaxCovColumns = 64;      // queries per pass: a front's queries are one 64-bit mask (KH_SPA_MAX_COV_COLUMNS)

struct CovColumnsPlan
{
  // per level of the tree (leaves first, as Symbolic::levels): the fronts on the union of the paths, ascending, and per such front
  // the queries it carries (bit k = query k)
  std::vector<std::vector<int32_t>> level_fronts;
  std::vector<std::vector<uint64_t>> level_masks;
  std::vector<uint64_t> front_mask;         // per front: the same mask, 0 for a front on no path
  std::vector<int32_t> query_front;         // per query: the front that eliminates it
  int32_t n_path_fronts = 0;
};

// parent / level / sn_of_elim / elim_of_free as in Symbolic, n_levels = Symbolic::levels.size(); queries: free indices, at most
// kMaxCovColumns of them, each in [0, n_free) or negative (the gauge node: a column of zeros, no front carries it, query_front -1).
// Returns false (an empty plan) on a query beyond n_free or too many.
inline bool plan_covariance_columns(const std::vector<int32_t> & parent, const std::vector<int32_t> & level, int32_t n_levels,
  const std::vector<int32_t> & sn_of_elim, const std::vector<int32_t> & elim_of_free, const std::vector<int32_t> & queries, CovColumnsPlan & plan)
{
  const int32_t n_fronts = static_cast<int32_t>(parent.size());
  plan = CovColumnsPlan{};
  if (static_cast<int32_t>(queries.size()) > kMaxCovColumns) {return false;}
  plan.front_mask.assign(n_fronts, 0);
  for (size_t k = 0; k < queries.size(); ++k) {
    const int32_t f = queries[k];
    if (f >= static_cast<int32_t>(elim_of_free.size())) {plan = CovColumnsPlan{}; return false;}
    int32_t front = f < 0 ? -1 : sn_of_elim[elim_of_free[f]];
    plan.query_front.push_back(front);
    for (; front >= 0; front = parent[front]) {plan.front_mask[front] |= uint64_t{1} << k;}
  }
  plan.level_fronts.assign(n_levels, {});
  plan.level_masks.assign(n_levels, {});
  for (int32_t k = 0; k < n_fronts; ++k) {
    if (plan.front_mask[k]) {
      plan.level_fronts[level[k]].push_back(k);
      plan.level_masks[level[k]].push_back(plan.front_mask[k]);
      ++plan.n_path_fronts;
    }
  }
  return true;
}

}  // namespace kh
