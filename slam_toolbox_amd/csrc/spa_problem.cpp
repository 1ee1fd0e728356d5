// Problem setup of the pose-graph SPA solver (hot path B): from the graph store of the handle to the device view of one
// linear-algebra problem (SpaDev), stage by stage.  The stages that need neither HIP nor the handle are spa_problem_plan.hpp's;
// the symbolic analysis is spa_symbolic.cpp's.
//
// Reference: solvers/ceres_solver.cpp:214-269 (Compute: the gauge, then Ceres' own problem setup -- a third-party dependency that is
// not in the reference tree, see spa_symbolic.hpp).
#include <chrono>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <type_traits>

#include "spa_private.hpp"
#include "spa_problem_plan.hpp"

using namespace kh;
using namespace kh::spa;

namespace
{
const ParallelFor kHostPool = [](size_t n, const std::function<void(size_t)> & fn) {host_parallel_for(n, fn);};

// ---- stage 1: edge endpoints and gauge ----
// the first inserted node is constant once it has parameter blocks (ceres_solver.cpp:228-241); returns its position, -1: none
int32_t endpoints_and_gauge(kh_spa * s, std::vector<int32_t> & ea, std::vector<int32_t> & eb, std::vector<uint8_t> & used)
{
  edge_endpoints(static_cast<int32_t>(s->nodes.size()), static_cast<int32_t>(s->cons.size()), [s](int32_t i) {return s->nodes[i].id;},
    [s](int32_t e) {return std::pair<int32_t, int32_t>(s->cons[e].a, s->cons[e].b);}, s->index_of, ea, eb, used);
  if (!s->was_constant_set && s->has_first) {
    auto it = s->index_of.find(s->first_id);
    if (it != s->index_of.end() && used[it->second]) {s->was_constant_set = true;}
  }
  int32_t fixed = -1;
  if (s->was_constant_set) {
    auto it = s->index_of.find(s->first_id);
    if (it != s->index_of.end()) {fixed = it->second;}
  }
  return fixed;
}

// ---- stage 2: the cached-topology test ----
// same nodes, same edges in the same order, same gauge: the cached analysis holds
bool topology_is_cached(const kh_spa * s, int32_t fixed, const std::vector<int32_t> & ea, const std::vector<int32_t> & eb)
{
  return fixed == s->cached_fixed && static_cast<int32_t>(s->nodes.size()) == s->cached_n && ea == s->cached_ea && eb == s->cached_eb &&
         !s->node_of_free.empty();
}

// ---- stage 5: the analysis ----
// Ordering + fronts of the adjacency, into s->sym.
// INCREMENTAL re-analysis: a loop closure adds a few dozen nodes and edges to a graph that was dissected milliseconds
// ago (and lifelong mode removes a few).  The supernodes of the last dissection, kept by node id, are reused -- the
// nodes that have left drop out, the new ones become leading leaf supernodes (eliminated first: no extra levels; their
// old neighbours become mutually adjacent, which the structure pass accounts for like any fill) -- and only the structure
// is rebuilt.  A full dissection again when the new nodes pass a quarter of the graph, when the factorisation's flops have tripled relative to the graph's growth,
// or after kMaxReuse re-analyses.  kh_spa_reset() forgets the supernodes (a reloaded graph is analysed from scratch).
struct Analysis
{
  int rc = KH_OK;
  bool incremental = false;
  std::string error;                 // the analysing thread's error text (kh_last_error is per thread)
};

void analyse(kh_spa * s, const Pattern & pat, const SymbolicOptions & sopt, int extra_levels, Analysis & out)
{
  constexpr int kMaxReuse = 24;
  const int32_t nf = static_cast<int32_t>(s->node_of_free.size());
  auto id_of_free = [s](int32_t f) {return s->nodes[s->node_of_free[f]].id;};
  if (!s->cached_sn_ids.empty() && s->reuse_count < kMaxReuse) {
    std::vector<std::vector<int32_t>> sn;
    std::vector<uint8_t> placed;
    const int32_t kept = map_cached_supernodes(s->cached_sn_ids, nf, id_of_free, sn, placed);
    if (nf - kept <= std::max(64, nf / 4)) {
      std::vector<int32_t> fresh;
      for (int32_t f = 0; f < nf; ++f) {if (!placed[f]) {fresh.push_back(f);}}
      if (!fresh.empty()) {sn.insert(sn.begin(), std::move(fresh));}          // build_structure splits it into a chain when long
      out.rc = build_structure(s->sym, nf, pat.adj_ptr, pat.adj_idx, sopt, sn);
      // fill guard: the factorisation may cost three times the last full dissection's, scaled by how much the graph has
      // grown since (flops grow at least linearly with the free nodes).  Three, not one and a half: the leading leaves of a
      // closure's few dozen new nodes add little fill, but a bound of 1.5 sent most closures of the 50 000-scan replay back
      // to a full dissection (5 ms each: the replay's solver time went from 4.1 to 7.5 s)
      const double allowed = 3.0 * static_cast<double>(s->cached_full_flops) * static_cast<double>(nf) / static_cast<double>(std::max(1, s->cached_full_nf));
      // level guard (round 6): the leading leaf's update matrix reaches into every supernode its nodes touch and strings those up
      // as ancestors of one another -- on a connected graph (the non-lifelong replay) every re-analysis added one to three levels of
      // ONE front each to the top of the tree (8 levels after a full dissection, 26 sixteen closures later), and a level is three
      // launches of 10-27 us per factorisation whatever it holds.  Back to a full dissection once the tree is extra_levels taller
      // than the last one left it.  Measured (solver ms of the 3000-scan non-lifelong / the 20 000-scan lifelong replay): no guard
      // 499 / 810, 5 levels 418 / 647, 3: 384 / 642, 2: 364-377 / 508, 1: 366 / 518, 0: 370 / 602, never incremental 358 / 621.
      // On the 50 000-scan lifelong replay (12 000 free nodes in thousands of components: a dissection costs 5-7 ms, the tree
      // grows slowly) 2 / 6 / no guard gave 2772 / 2576 / 2606 ms (medians of three alternating runs): 6 from 6000 free nodes on.
      const bool levels_ok = static_cast<int>(s->sym.levels.size()) <= s->cached_full_levels + extra_levels;
      if (out.rc == KH_OK && static_cast<double>(s->sym.factor_flops) <= allowed && levels_ok) {
        out.incremental = true;
        return;
      }
    }
  }
  std::vector<std::vector<int32_t>> dissected;
  out.rc = nested_dissection(nf, pat.adj_ptr, pat.adj_idx, sopt, dissected);
  if (out.rc == KH_OK) {
    s->cached_sn_ids.assign(dissected.size(), {});
    for (size_t k = 0; k < dissected.size(); ++k) {
      for (int32_t f : dissected[k]) {s->cached_sn_ids[k].push_back(id_of_free(f));}
    }
    out.rc = build_structure(s->sym, nf, pat.adj_ptr, pat.adj_idx, sopt, dissected);
    s->cached_full_flops = s->sym.factor_flops; s->cached_full_nf = nf; s->reuse_count = 0;
    s->cached_full_levels = static_cast<int32_t>(s->sym.levels.size());
  }
  if (out.rc != KH_OK) {out.error = kh_last_error();}
}

// KH_SPA_DEBUG: what the analysis left
void print_analysis(const Symbolic & sym, int32_t nf)
{
  int32_t max_m = 0, max_ns = 0;
  for (int32_t k = 0; k < sym.n_fronts; ++k) {max_m = std::max(max_m, sym.front_m[k]); max_ns = std::max(max_ns, sym.front_ns[k]);}
  std::fprintf(stderr, "[kh_spa] free nodes %d, fronts %d, levels %zu, max front m %d, max ns %d, front storage %.1f MB, nnz(L) %lld\n",
    nf, sym.n_fronts, sym.levels.size(), max_m, max_ns, sym.fronts_size * 8.0 / 1e6, static_cast<long long>(sym.nnz_factor));
  for (size_t l = 0; l < sym.levels.size(); ++l) {
    int32_t mm = 0; int64_t work = 0;
    for (int32_t k : sym.levels[l]) {mm = std::max(mm, sym.front_m[k]); work += static_cast<int64_t>(sym.front_m[k]) * sym.front_m[k] * sym.front_ns[k];}
    std::fprintf(stderr, "[kh_spa]   level %zu: %zu fronts, max m %d, flops~%.2fM\n", l, sym.levels[l].size(), mm, work / 1e6);
  }
}

// ---- stage 8: the level plan ----
// the level lists, concatenated, and what the launches of a level are sized by (kh_spa::level_*)
void plan_levels(kh_spa * s, std::vector<int32_t> & level_fronts)
{
  const Symbolic & sym = s->sym;
  level_fronts.clear();
  s->level_offsets.assign(1, 0);
  s->level_max_m.clear(); s->level_max_ns.clear(); s->level_split.clear(); s->level_fused_lds.clear(); s->level_max_nu.clear();
  for (auto & lv : sym.levels) {
    level_fronts.insert(level_fronts.end(), lv.begin(), lv.end());
    s->level_offsets.push_back(static_cast<int32_t>(level_fronts.size()));
    int32_t mm = 0, mns = 0;
    for (int32_t k : lv) {mm = std::max(mm, sym.front_m[k]); mns = std::max(mns, sym.front_ns[k]);}
    s->level_max_m.push_back(mm); s->level_max_ns.push_back(mns);
    // the fronts of a level are numbered largest first: the ones that do not fit k_front_update are (nearly) a prefix
    constexpr int kFuseMin = 256;         // fronts of a level from which k_front_update takes the ones that fit it
    int32_t split = 0;
    size_t lds = 0;
    for (size_t q = 0; q < lv.size(); ++q) {
      const size_t b = spa_front_update_lds(sym.front_m[lv[q]], sym.front_ns[lv[q]]);
      if (b == 0 && sym.front_m[lv[q]] > sym.front_ns[lv[q]]) {split = static_cast<int32_t>(q) + 1; lds = 0;} else {lds = std::max(lds, b);}
    }
    if (static_cast<int32_t>(lv.size()) - split < kFuseMin) {split = static_cast<int32_t>(lv.size());}
    s->level_split.push_back(split); s->level_fused_lds.push_back(lds);
    int32_t mnu = 0;
    for (int32_t k : lv) {mnu = std::max(mnu, sym.front_m[k] - sym.front_ns[k]);}
    s->level_max_nu.push_back(mnu);
  }
}

// ---- stage 9: FrontDesc records and the deferred list ----
void describe_fronts(kh_spa * s, std::vector<FrontDesc> & desc, std::vector<int32_t> & deferred)
{
  const Symbolic & sym = s->sym;
  deferred.clear();
  s->deferred_max_m = 0;
  for (int32_t k = 0; k < sym.n_fronts; ++k) {
    if (sym.scatter_mode[k] == 0 && sym.parent[k] >= 0 && sym.front_m[k] > sym.front_ns[k]) {
      deferred.push_back(k); s->deferred_max_m = std::max(s->deferred_max_m, sym.front_m[k]);
    }
  }
  s->n_deferred_fronts = static_cast<int32_t>(deferred.size());
  if (deferred.empty()) {deferred.push_back(0);}
  desc.resize(sym.n_fronts);
  for (int32_t k = 0; k < sym.n_fronts; ++k) {
    FrontDesc & fd = desc[k];
    std::memset(&fd, 0, sizeof(fd));
    fd.off = sym.front_off[k]; fd.woff = sym.winv_off[k]; fd.m = sym.front_m[k]; fd.ns = sym.front_ns[k]; fd.first = sym.front_first[k];
    fd.rows_ptr = sym.rows_ptr[k]; fd.child_ptr = sym.child_ptr[k]; fd.child_end = sym.child_ptr[k + 1];
    fd.relpos_ptr = sym.relpos_ptr[k]; fd.parent = sym.parent[k]; fd.cinv_ptr = sym.cinv_ptr[k];
    fd.flags = sym.scatter_mode[k] | (sym.has_b[k] ? 4 : 0) | (sym.n_deferred[k] << 8);
    for (int32_t q = 0; q < 3 && fd.child_ptr + q < fd.child_end; ++q) {
      const int32_t c = sym.child_list[fd.child_ptr + q];
      fd.ch[q].off = sym.front_off[c]; fd.ch[q].m = sym.front_m[c]; fd.ch[q].ns = sym.front_ns[c]; fd.ch[q].rows_ptr = sym.rows_ptr[c];
    }
  }
}

// ---- stage 10: pack into the pinned block, one upload, alias the slices ----
// Every array is copied into ONE pinned block and travels to ONE device block in ONE copy; the device buffers of the arrays are
// slices of that block (round 5: one pinned block, ~35 asynchronous copies -- 3-4 us of the caller's time each, on every
// closure of a mapper; before that ~35 copies out of pageable vectors, each staged and waited for on its own).
struct PackedUpload
{
  struct Item {std::function<void(char *)> bind; const void * src; size_t bytes; size_t off;};
  std::vector<Item> items;
  size_t bytes = 0;
  // `buf` becomes the slice that holds `vec` (which has to stay where it is until send_packed)
  template <class Buf, class Vec>
  void add(Buf & buf, const Vec & vec)
  {
    typedef typename Buf::value_type T;
    const size_t n = std::max<size_t>(vec.size(), 1);
    Buf * bp = &buf;
    items.push_back({[bp, n](char * base) {bp->alias(reinterpret_cast<T *>(base), n);}, vec.empty() ? nullptr : vec.data(), vec.size() * sizeof(T), bytes});
    bytes += (n * sizeof(T) + 63) & ~static_cast<size_t>(63);
  }
};

int send_packed(kh_spa * s, const PackedUpload & up)
{
  hipStream_t st = s->stream;
  const size_t total = std::max<size_t>(up.bytes, 64);
  if (total > s->h_upload_cap) {
    KS_HIP(hipStreamSynchronize(st));          // (an earlier copy may still read the old block)
    if (s->h_upload) {KS_HIP(hipHostFree(s->h_upload)); s->h_upload = nullptr; s->h_upload_cap = 0;}
    const size_t cap = total + total / 2;
    KS_HIP(hipHostMalloc(reinterpret_cast<void **>(&s->h_upload), cap, hipHostMallocDefault));
    s->h_upload_cap = cap;
  }
  if (total > s->d_pack.cap) {KS_HIP(hipStreamSynchronize(st));}       // (kernels of the last solve read slices of the old block)
  if (s->d_pack.ensure(total)) {return KH_ERR_HIP;}
  for (const PackedUpload::Item & q : up.items) {
    if (q.bytes) {std::memcpy(s->h_upload + q.off, q.src, q.bytes);}
    q.bind(s->d_pack.p + q.off);
  }
  if (hipMemcpyAsync(s->d_pack.p, s->h_upload, total, hipMemcpyHostToDevice, st) != hipSuccess) {
    (void)hipStreamSynchronize(st);
    set_error("hipMemcpyAsync: upload of the analysis");
    return KH_ERR_HIP;
  }
  return KH_OK;
}

// ---- stage 11: work buffers ----
int grow_work_buffers(kh_spa * s, int32_t E, int32_t nf, int32_t n_slots)
{
  const Symbolic & sym = s->sym;
  hipStream_t st = s->stream;
  int rc = s->d_winv.ensure(static_cast<size_t>(sym.winv_size) + 16);
  if (rc) {(void)hipStreamSynchronize(st); return KH_ERR_HIP;}
  s->n_slots = n_slots;
  const size_t scratch = std::max<size_t>(static_cast<size_t>(21) * E, static_cast<size_t>(9) * nf + 16);
  rc |= s->d_edge_lin.ensure(scratch); rc |= s->d_edge_cost.ensure(std::max(E, 1));
  // H and g share one buffer so that a sharded run sums them across ranks with ONE all-reduce
  rc |= s->d_Hg.ensure(static_cast<size_t>(n_slots) * 9 + static_cast<size_t>(nf) * 3 + 8);
  rc |= s->d_Hg_alt.ensure(static_cast<size_t>(n_slots) * 9 + static_cast<size_t>(nf) * 3 + 8);
  // (a buffer that grows is a NEW allocation, and the allocator may hand the old address back: "clean" is a fact about the
  // contents, so it ends with the allocation -- a mapper that asks for a covariance pass per scan grows the fronts between passes)
  const size_t fronts_cap = s->d_fronts.cap, fronts_b_cap = s->d_fronts_b.cap;
  rc |= s->d_fronts.ensure(static_cast<size_t>(sym.fronts_size) + 16);
  rc |= s->d_fronts_b.ensure(static_cast<size_t>(sym.fronts_size) + 16);
  if (s->d_fronts.cap != fronts_cap || s->d_fronts_b.cap != fronts_b_cap) {s->clean_a = nullptr;}
  rc |= s->d_scale.ensure(3 * nf); rc |= s->d_diag.ensure(3 * nf); rc |= s->d_rhs.ensure(3 * nf);
  rc |= s->d_step.ensure(3 * nf); rc |= s->d_delta.ensure(3 * nf);
  rc |= s->d_fail.ensure(4);
  rc |= s->d_upd.ensure(static_cast<size_t>(3) * sym.rows_ptr[sym.n_fronts] + 16);
  rc |= s->d_partial.ensure(static_cast<size_t>(5) * ((4 * nf + 255) / 256) + (E + 255) / 256 + static_cast<size_t>(2) * ((3 * nf + 255) / 256) + 32);
  if (rc) {(void)hipStreamSynchronize(st); return KH_ERR_HIP;}
  return KH_OK;
}

// ---- stages 3 to 11: a new topology (or gauge) from the free numbering to the device ----
// (no free node or no edge: nothing is in the problem, and the topology stays dirty)
int analyse_topology(kh_spa * s, int32_t fixed, const std::vector<int32_t> & ea, const std::vector<int32_t> & eb, const std::vector<uint8_t> & used,
                     std::chrono::steady_clock::time_point t_prep0)
{
  const int32_t N = static_cast<int32_t>(s->nodes.size()), E = static_cast<int32_t>(s->cons.size());
  s->fixed_index = fixed;
  number_free_nodes(used, fixed, s->free_of_node, s->node_of_free);
  const int32_t nf = static_cast<int32_t>(s->node_of_free.size());
  if (nf == 0 || E == 0) {s->topology_dirty = true; return KH_OK;}
  Pattern pat;
  build_pattern(ea, eb, s->free_of_node, nf, kHostPool, pat);
  const int32_t n_slots = pat.n_slots();
  // Ordering + fronts on a thread of their own, beside the contribution lists below (both only read the adjacency).
  const auto t_sym0 = std::chrono::steady_clock::now();
  SymbolicOptions sopt;
  // the independent subsets of a dissection level run on the library's persistent host pool
  sopt.parallel_for = kHostPool;
  if (const char * e = std::getenv("KH_SPA_LEAF")) {sopt.leaf_nodes = std::max(1, std::atoi(e));}
  // how many levels taller than the last full dissection left it an incremental analysis may make the tree (the level guard
  // of analyse()).  Read here, on the caller's thread, before the analysis may start on a thread of its own: tests/test_spa_gpu.py
  // switches the guard off around one Compute().
  const char * guard_env = std::getenv("KH_SPA_EXTRA_LEVELS");
  const int extra_levels = guard_env ? std::atoi(guard_env) : (nf <= 6000 ? 2 : 6);
  Analysis an;
  // (a thread of its own only where there is something to win: the lists below take 0.6 ms on the 10 000-node graph and 0.08 ms on
  // a mapper's 2000 nodes, creating and joining a thread 0.1 ms)
  const bool analysis_beside = nf >= 4000;
  std::thread sym_thread;
  if (analysis_beside) {sym_thread = std::thread([&]() {analyse(s, pat, sopt, extra_levels, an);});}
  struct Joiner {std::thread & t; ~Joiner() {if (t.joinable()) {t.join();}}} sym_joiner{sym_thread};
  Contributions lists;
  build_contributions(ea, eb, s->free_of_node, nf, pat, lists);
  const auto t_lists = std::chrono::steady_clock::now();
  if (analysis_beside) {sym_thread.join();} else {analyse(s, pat, sopt, extra_levels, an);}
  if (an.rc) {set_error(an.error); return an.rc;}
  if (an.incremental) {++s->reuse_count;}
  s->last_analysis_incremental = an.incremental ? 1 : 0;
  if (std::getenv("KH_SPA_DEBUG")) {
    std::fprintf(stderr, "[kh_spa] host: adjacency %.2f ms, lists %.2f ms beside the %s analysis (%.2f ms)\n",
      ms_between(t_prep0, t_sym0), ms_between(t_sym0, t_lists), an.incremental ? "incremental" : "full", ms_since(t_sym0));
  }
  if (std::getenv("KH_SPA_DEBUG")) {print_analysis(s->sym, nf);}
  const Symbolic & sym = s->sym;
  std::vector<int64_t> slot_dest;
  std::vector<int32_t> slot_ld;
  if (!place_slots(sym, pat, kHostPool, slot_dest, slot_ld)) {set_error("symbolic: matrix entry outside its front"); return KH_ERR_SOLVER;}
  std::vector<int32_t> level_fronts, deferred;
  std::vector<FrontDesc> desc;
  plan_levels(s, level_fronts);
  describe_fronts(s, desc, deferred);
  // uploads
  std::vector<int32_t> col_and_row = pat.col;
  col_and_row.insert(col_and_row.end(), pat.slot_row.begin(), pat.slot_row.end());
  PackedUpload up;
  up.add(s->d_edge_a, ea); up.add(s->d_edge_b, eb);
  up.add(s->d_free_of_node, s->free_of_node); up.add(s->d_node_of_free, s->node_of_free);
  up.add(s->d_slot_contrib_ptr, lists.slot_ptr); up.add(s->d_slot_contrib, lists.slot_list);
  up.add(s->d_bsr_row_ptr, pat.row_ptr); up.add(s->d_bsr_col, col_and_row); up.add(s->d_bsr_diag, pat.diag);
  up.add(s->d_node_contrib_ptr, lists.node_ptr); up.add(s->d_node_contrib, lists.node_list);
  up.add(s->d_front_off, sym.front_off); up.add(s->d_front_m, sym.front_m);
  up.add(s->d_front_ns, sym.front_ns); up.add(s->d_front_first, sym.front_first);
  up.add(s->d_rows_ptr, sym.rows_ptr); up.add(s->d_rows, sym.rows);
  up.add(s->d_child_ptr, sym.child_ptr); up.add(s->d_child_list, sym.child_list);
  up.add(s->d_relpos_ptr, sym.relpos_ptr); up.add(s->d_relpos, sym.relpos);
  up.add(s->d_slot_dest, slot_dest); up.add(s->d_slot_ld, slot_ld);
  up.add(s->d_elim_of_free, sym.elim_of_free); up.add(s->d_free_of_elim, sym.free_of_elim);
  up.add(s->d_level_fronts, level_fronts);
  up.add(s->d_deferred, deferred);
  up.add(s->d_winv_off, sym.winv_off);
  up.add(s->d_cinv, sym.cinv);
  up.add(s->d_desc, desc);
  int rc = send_packed(s, up);
  if (rc) {return rc;}
  rc = grow_work_buffers(s, E, nf, n_slots);
  if (rc) {return rc;}
  // the uploads above read host memory of this call: they must have landed before it ends
  KS_HIP(hipStreamSynchronize(s->stream));
  s->topology_dirty = false;
  s->cached_ea = ea; s->cached_eb = eb; s->cached_n = N; s->cached_fixed = fixed;
  s->last_symbolic_ms = ms_since(t_prep0);
  return KH_OK;
}

// ---- stage 12: values that change between calls without touching the topology ----
int upload_values(kh_spa * s)
{
  const int32_t N = static_cast<int32_t>(s->nodes.size()), E = static_cast<int32_t>(s->cons.size());
  std::vector<double> z(static_cast<size_t>(E) * 3), u(static_cast<size_t>(E) * 9), x(static_cast<size_t>(N) * 3);
  for (int32_t e = 0; e < E; ++e) {
    std::copy(s->cons[e].z, s->cons[e].z + 3, z.begin() + 3 * e);
    std::copy(s->cons[e].u, s->cons[e].u + 9, u.begin() + 9 * e);
  }
  for (int32_t i = 0; i < N; ++i) {std::copy(s->nodes[i].pose, s->nodes[i].pose + 3, x.begin() + 3 * i);}
  int rc = 0;
  rc |= s->d_edge_z.upload(z, s->stream); rc |= s->d_edge_u.upload(u, s->stream);
  rc |= s->d_x.upload(x, s->stream); rc |= s->d_cand.ensure(x.size()); rc |= s->d_best.ensure(x.size()); rc |= s->d_scal.ensure(32);
  if (rc) {return KH_ERR_HIP;}
  KS_HIP(hipStreamSynchronize(s->stream));   // the staging vectors above go out of scope
  return KH_OK;
}

// ---- stage 13: the device view ----
void fill_device_view(const kh_spa * s, SpaDev & dev)
{
  const Symbolic & sym = s->sym;
  dev.n_nodes = static_cast<int32_t>(s->nodes.size()); dev.n_free = static_cast<int32_t>(s->node_of_free.size());
  dev.n_edges = static_cast<int32_t>(s->cons.size());
  dev.edge_a = s->d_edge_a.p; dev.edge_b = s->d_edge_b.p; dev.edge_z = s->d_edge_z.p; dev.edge_u = s->d_edge_u.p;
  dev.free_of_node = s->d_free_of_node.p; dev.node_of_free = s->d_node_of_free.p;
  dev.edge_lin = s->d_edge_lin.p; dev.edge_cost = s->d_edge_cost.p;
  dev.n_slots = s->n_slots; dev.slot_contrib_ptr = s->d_slot_contrib_ptr.p; dev.slot_contrib = s->d_slot_contrib.p;
  dev.bsr_row_ptr = s->d_bsr_row_ptr.p; dev.bsr_col = s->d_bsr_col.p; dev.bsr_diag_slot = s->d_bsr_diag.p;
  dev.H = s->d_Hg.p; dev.node_contrib_ptr = s->d_node_contrib_ptr.p; dev.node_contrib = s->d_node_contrib.p;
  dev.g = s->d_Hg.p + static_cast<size_t>(s->n_slots) * 9;
  dev.n_fronts = sym.n_fronts; dev.front_off = s->d_front_off.p; dev.front_m = s->d_front_m.p; dev.front_ns = s->d_front_ns.p;
  dev.front_first = s->d_front_first.p; dev.front_rows_ptr = s->d_rows_ptr.p; dev.front_rows = s->d_rows.p;
  dev.child_ptr = s->d_child_ptr.p; dev.child_list = s->d_child_list.p; dev.relpos_ptr = s->d_relpos_ptr.p; dev.relpos = s->d_relpos.p;
  dev.slot_dest = s->d_slot_dest.p; dev.slot_ld = s->d_slot_ld.p;
  dev.elim_of_free = s->d_elim_of_free.p; dev.free_of_elim = s->d_free_of_elim.p;
  dev.fronts = s->d_fronts.p; dev.fronts_size = sym.fronts_size; dev.fronts_b = s->d_fronts_b.p;
  dev.winv = s->d_winv.p; dev.winv_off = s->d_winv_off.p; dev.desc = s->d_desc.p; dev.cinv = s->d_cinv.p;
}
}  // namespace

int kh::spa::prepare_problem(kh_spa * s, SpaDev & dev, bool & has_work)
{
  has_work = false;
  s->last_symbolic_ms = 0.0;
  const auto t_prep0 = std::chrono::steady_clock::now();
  std::vector<uint8_t> used;
  std::vector<int32_t> ea, eb;
  const int32_t fixed = endpoints_and_gauge(s, ea, eb, used);
  if (s->topology_dirty && topology_is_cached(s, fixed, ea, eb)) {
    s->topology_dirty = false;
    s->fixed_index = fixed;
  }
  if (s->topology_dirty || fixed != s->fixed_index) {
    const int rc = analyse_topology(s, fixed, ea, eb, used, t_prep0);
    if (rc) {return rc;}
  }
  if (s->node_of_free.empty() || s->cons.empty()) {return KH_OK;}
  const int rc = upload_values(s);
  if (rc) {return rc;}
  if (std::getenv("KH_SPA_DEBUG")) {std::fprintf(stderr, "[kh_spa] host: prepare_problem total %.2f ms\n", ms_since(t_prep0));}
  fill_device_view(s, dev);
  has_work = true;
  return KH_OK;
}
