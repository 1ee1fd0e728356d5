// CPU probe of the solver's problem plan and symbolic analysis (no GPU): reads a binary edge list (int32 pairs of node ids; the
// nodes are 0..N-1 in that order unless SYM_PROBE_IDS names a file of N int32 ids in insertion order; the first node is the gauge),
// builds the problem with the library's own stages (csrc/spa_problem_plan.hpp) and prints the assembly tree level by level.
// Build: g++ -O2 -std=c++17 -pthread tools/sym_probe.cpp slam_toolbox_amd/csrc/spa_symbolic.cpp -o /tmp/sym_probe
//   python -c "from slam_toolbox_amd import synth; import numpy as np; synth.make_pose_graph(10000,30000)['edges'].astype(np.int32).tofile('/tmp/edges.bin')"
//   /tmp/sym_probe /tmp/edges.bin 10000 [leaf] [pmax] [cands]
// SYM_PROBE_DUMP=file: the analysis and every array of the plan, for tests/test_spa_symbolic.py.  SYM_PROBE_CACHED=file (int32:
// per supernode its length, then its node ids): an earlier dissection's supernodes, mapped onto this problem and dumped as well.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <thread>
#include <vector>
#include "../slam_toolbox_amd/csrc/spa_problem_plan.hpp"
#include "../slam_toolbox_amd/csrc/host_pool.hpp"
namespace kh {static std::string g_err; void set_error(const std::string & s) {g_err = s;}}

static std::vector<int32_t> read_ints(const char * path)
{
  std::vector<int32_t> v;
  FILE * f = std::fopen(path, "rb");
  if (!f) {std::fprintf(stderr, "sym_probe: cannot read %s\n", path); std::exit(2);}
  int32_t buf[4096]; size_t n;
  while ((n = std::fread(buf, 4, 4096, f)) > 0) {v.insert(v.end(), buf, buf + n);}
  std::fclose(f);
  return v;
}

int main(int argc, char ** argv)
{
  if (argc < 3) {std::fprintf(stderr, "usage: sym_probe edges.bin n_nodes [leaf] [pmax] [cands]\n"); return 2;}
  const std::vector<int32_t> e = read_ints(argv[1]);
  const int E = static_cast<int>(e.size() / 2), N = std::atoi(argv[2]);
  std::vector<int32_t> ids(N);
  for (int i = 0; i < N; ++i) {ids[i] = i;}
  if (const char * path = std::getenv("SYM_PROBE_IDS")) {ids = read_ints(path);}
  if (static_cast<int>(ids.size()) != N) {std::fprintf(stderr, "sym_probe: %zu ids for %d nodes\n", ids.size(), N); return 2;}
  std::unordered_map<int32_t, int32_t> index_of;
  for (int i = 0; i < N; ++i) {index_of[ids[i]] = i;}
  for (int32_t id : e) {if (!index_of.count(id)) {std::fprintf(stderr, "sym_probe: edge to unknown node %d\n", id); return 2;}}
  kh::SymbolicOptions opt;
  if (argc > 3) {opt.leaf_nodes = std::atoi(argv[3]);}
  if (argc > 4) {opt.max_pivot_nodes = std::atoi(argv[4]);}
  if (argc > 5) {opt.separator_candidates = std::atoi(argv[5]);}
  if (argc > 6) {opt.balance_lo = std::atof(argv[6]); opt.balance_hi = 1.0 - opt.balance_lo;}
  if (std::getenv("SYM_PROBE_THREADS")) {
    // the parallel loops on plain threads (the library passes its persistent pool)
    const int nt = std::max(1, std::atoi(std::getenv("SYM_PROBE_THREADS")));
    opt.parallel_for = [nt](size_t n, const std::function<void(size_t)> & fn) {
      std::atomic<size_t> next{0};
      std::vector<std::thread> team;
      auto work = [&] {for (size_t i; (i = next.fetch_add(1)) < n;) {fn(i);}};
      for (int t = 1; t < nt; ++t) {team.emplace_back(work);}
      work();
      for (auto & t : team) {t.join();}
    };
  }
  if (std::getenv("SYM_PROBE_POOL")) {
    // ... or on the library's persistent pool (KH_HOST_THREADS), as kh_spa_compute passes it
    opt.parallel_for = [](size_t n, const std::function<void(size_t)> & fn) {kh::HostPool::instance().run(n, fn);};
  }
  // the problem, stage by stage as prepare_problem builds it
  std::vector<int32_t> ea, eb, free_of_node, node_of_free;
  std::vector<uint8_t> used;
  kh::spa::edge_endpoints(N, E, [&](int32_t i) {return ids[i];}, [&](int32_t k) {return std::pair<int32_t, int32_t>(e[2 * k], e[2 * k + 1]);}, index_of,
    ea, eb, used);
  kh::spa::number_free_nodes(used, 0, free_of_node, node_of_free);
  const int32_t nf = static_cast<int32_t>(node_of_free.size());
  if (nf == 0) {std::fprintf(stderr, "sym_probe: no free node\n"); return 2;}
  kh::spa::Pattern pat;
  kh::spa::build_pattern(ea, eb, free_of_node, nf, opt.parallel_for, pat);
  kh::Symbolic sym;
  double best = 1e30;
  int rc = 0;
  const int reps = std::getenv("SYM_PROBE_REPS") ? std::atoi(std::getenv("SYM_PROBE_REPS")) : 5;
  for (int rep = 0; rep < reps; ++rep) {
    const auto t0 = std::chrono::steady_clock::now();
    rc = kh::build_symbolic(sym, nf, pat.adj_ptr, pat.adj_idx, opt);
    best = std::min(best, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  std::printf("rc %d (%s) fronts %d levels %zu nnz(L) %.2fM flops %.0fM front storage %.0f MB winv %.0f MB max m %d max ns %d  best: %.2f ms\n", rc,
    kh::g_err.c_str(), sym.n_fronts, sym.levels.size(), sym.nnz_factor / 1e6, sym.factor_flops / 1e6, sym.fronts_size * 8e-6, sym.winv_size * 8e-6,
    sym.max_m, sym.max_ns, best);
  int sum_ns = 0;
  for (size_t l = 0; l < sym.levels.size(); ++l) {
    int mm = 0, mns = 0; double work = 0;
    for (int k : sym.levels[l]) {
      mm = std::max(mm, sym.front_m[k]); mns = std::max(mns, sym.front_ns[k]);
      for (int j = 0; j < sym.front_ns[k]; ++j) {work += double(sym.front_m[k] - j) * (sym.front_m[k] - j);}
    }
    sum_ns += mns;
    std::printf("level %2zu: %4zu fronts, max m %3d, max ns %3d, %.1fM mult-adds\n", l, sym.levels[l].size(), mm, mns, work / 1e6);
  }
  std::printf("sum of the levels' largest pivot counts: %d\n", sum_ns);
  const char * dump = std::getenv("SYM_PROBE_DUMP");
  if (dump && rc == 0) {
    kh::spa::Contributions lists;
    kh::spa::build_contributions(ea, eb, free_of_node, nf, pat, lists);
    std::vector<int64_t> slot_dest;
    std::vector<int32_t> slot_ld;
    if (!kh::spa::place_slots(sym, pat, opt.parallel_for, slot_dest, slot_ld)) {std::fprintf(stderr, "sym_probe: matrix entry outside its front\n"); return 3;}
    std::vector<int32_t> reuse_ptr(1, 0), reuse_idx, reuse_placed;
    if (const char * path = std::getenv("SYM_PROBE_CACHED")) {
      const std::vector<int32_t> raw = read_ints(path);
      std::vector<std::vector<int32_t>> cached, sn;
      for (size_t p = 0; p < raw.size(); p += 1 + static_cast<size_t>(raw[p])) {cached.emplace_back(raw.begin() + p + 1, raw.begin() + p + 1 + raw[p]);}
      std::vector<uint8_t> placed;
      const int32_t kept = kh::spa::map_cached_supernodes(cached, nf, [&](int32_t f) {return ids[node_of_free[f]];}, sn, placed);
      for (const auto & g : sn) {reuse_idx.insert(reuse_idx.end(), g.begin(), g.end()); reuse_ptr.push_back(static_cast<int32_t>(reuse_idx.size()));}
      reuse_placed.assign(placed.begin(), placed.end());
      reuse_placed.push_back(kept);
    }
    // arrays, each preceded by its length in int32 units (the int64 arrays count twice), in the order of the test's list of names
    FILE * o = std::fopen(dump, "wb");
    auto put = [&](const std::vector<int32_t> & v) {
      const int32_t n32 = static_cast<int32_t>(v.size());
      std::fwrite(&n32, 4, 1, o);
      if (n32 > 0) {std::fwrite(v.data(), 4, v.size(), o);}
    };
    auto put64 = [&](const std::vector<int64_t> & v) {
      const int32_t n32 = static_cast<int32_t>(2 * v.size());
      std::fwrite(&n32, 4, 1, o);
      if (n32 > 0) {std::fwrite(v.data(), 8, v.size(), o);}
    };
    put(sym.free_of_elim); put(sym.front_first); put(sym.front_ns); put(sym.front_m); put(sym.level); put(sym.parent);
    put(sym.rows_ptr); put(sym.rows); put(sym.child_ptr); put(sym.child_list); put(sym.relpos_ptr); put(sym.relpos);
    put(sym.cinv_ptr); put(sym.cinv);
    put(free_of_node); put(ea); put(eb);
    put(pat.row_ptr); put(pat.col); put(pat.slot_row); put(pat.diag);
    put(lists.slot_ptr); put(lists.slot_list); put(lists.node_ptr); put(lists.node_list);
    put64(slot_dest); put(slot_ld); put64(sym.front_off); put(sym.sn_of_elim);
    put(reuse_ptr); put(reuse_idx); put(reuse_placed);
    std::fclose(o);
  }
  return rc;
}
