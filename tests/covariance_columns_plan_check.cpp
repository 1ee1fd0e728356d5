// Stand-alone driver of slam_toolbox_amd/csrc/covariance_columns_plan.hpp (tests/test_covariance_columns_plan.py): one case per
// input line,
//   K parent[K] level[K] n_free sn_of_elim[n_free] elim_of_free[n_free] n_queries queries[n_queries]
// and one line back: "fail", or
//   ok n_path_fronts n_levels { count { front mask(hex) }* }* query_front[n_queries] front_mask[K](hex)
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../slam_toolbox_amd/csrc/covariance_columns_plan.hpp"

static bool read_list(std::istringstream & in, std::vector<int32_t> & v, int64_t n)
{
  v.assign(static_cast<size_t>(n), 0);
  for (auto & x : v) {if (!(in >> x)) {return false;}}
  return true;
}

int main()
{
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) {continue;}
    std::istringstream in(line);
    int64_t K = 0, nf = 0, nq = 0;
    std::vector<int32_t> parent, level, sn_of_elim, elim_of_free, queries;
    if (!(in >> K) || K < 0 || !read_list(in, parent, K) || !read_list(in, level, K) || !(in >> nf) || nf < 0 || !read_list(in, sn_of_elim, nf) ||
        !read_list(in, elim_of_free, nf) || !(in >> nq) || nq < 0 || !read_list(in, queries, nq)) {
      std::printf("bad input\n");
      return 2;
    }
    int32_t n_levels = 0;
    for (int32_t l : level) {n_levels = l + 1 > n_levels ? l + 1 : n_levels;}
    kh::CovColumnsPlan plan;
    if (!kh::plan_covariance_columns(parent, level, n_levels, sn_of_elim, elim_of_free, queries, plan)) {
      std::printf("fail\n");
      continue;
    }
    std::printf("ok %d %d", plan.n_path_fronts, n_levels);
    for (int32_t l = 0; l < n_levels; ++l) {
      std::printf(" %zu", plan.level_fronts[l].size());
      for (size_t t = 0; t < plan.level_fronts[l].size(); ++t) {std::printf(" %d %" PRIx64, plan.level_fronts[l][t], plan.level_masks[l][t]);}
    }
    for (int32_t f : plan.query_front) {std::printf(" %d", f);}
    for (uint64_t mk : plan.front_mask) {std::printf(" %" PRIx64, mk);}
    std::printf("\n");
  }
  return 0;
}
