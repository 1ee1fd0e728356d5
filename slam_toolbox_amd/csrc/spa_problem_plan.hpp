// The device-free stages of the solver's problem setup (spa_problem.cpp: prepare_problem): edge endpoints as node positions, the
// numbering of the free nodes, adjacency and BSR pattern, the contribution lists of the gather kernels, where every block of the
// pattern lands in its front, and the supernodes of an earlier dissection mapped onto this problem.  Pure functions of the edge
// endpoints, free_of_node and a Symbolic: nothing here knows HIP or the solver handle, so tools/sym_probe.cpp builds with this header
// alone and tests/test_spa_symbolic.py checks every array against a plain restatement.  The parallel loop is an argument, the way
// SymbolicOptions::parallel_for is (the library passes its persistent host pool); empty = serial.
#pragma once
#include <algorithm>
#include <atomic>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <unordered_map>
#include <vector>

#include "spa_symbolic.hpp"

namespace kh
{
namespace spa
{
typedef std::function<void(size_t, const std::function<void(size_t)> &)> ParallelFor;

// body(first, end) for every block of `block` consecutive indices of [0, n)
template <class Body>
void for_blocks(const ParallelFor & parallel_for, int32_t n, int32_t block, Body body)
{
  const size_t n_blocks = static_cast<size_t>((n + block - 1) / block);
  const std::function<void(size_t)> one = [&](size_t blk) {
    body(static_cast<int32_t>(blk) * block, std::min(n, static_cast<int32_t>(blk + 1) * block));
  };
  if (parallel_for) {parallel_for(n_blocks, one);} else {for (size_t blk = 0; blk < n_blocks; ++blk) {one(blk);}}
}

// ea[e], eb[e]: the positions (insertion order) of the nodes edge e joins; used[i]: an edge touches node i.  node_id(i) is the id
// of node i, edge_ids(e) the pair of ids of edge e, index_of the id -> position map.
// Node ids are scan ids: small and dense, so the 2 E lookups go through a table (a hash lookup each was 2 ms of every
// Compute on a 57 000-edge graph); sparse or negative ids keep the map.
template <class NodeId, class EdgeIds>
void edge_endpoints(int32_t N, int32_t E, NodeId node_id, EdgeIds edge_ids, const std::unordered_map<int32_t, int32_t> & index_of,
                    std::vector<int32_t> & ea, std::vector<int32_t> & eb, std::vector<uint8_t> & used)
{
  used.assign(N, 0); ea.resize(E); eb.resize(E);
  int32_t lo = 0, hi = -1;
  for (int32_t i = 0; i < N; ++i) {lo = std::min(lo, node_id(i)); hi = std::max(hi, node_id(i));}
  std::vector<int32_t> pos_of_id;
  if (lo >= 0 && hi >= 0 && static_cast<int64_t>(hi) < 8ll * N + 4096) {
    pos_of_id.assign(static_cast<size_t>(hi) + 1, -1);
    for (int32_t i = 0; i < N; ++i) {pos_of_id[node_id(i)] = i;}
  }
  for (int32_t e = 0; e < E; ++e) {
    const auto ab = edge_ids(e);
    if (!pos_of_id.empty()) {
      ea[e] = pos_of_id[ab.first]; eb[e] = pos_of_id[ab.second];
    } else {
      ea[e] = index_of.at(ab.first); eb[e] = index_of.at(ab.second);
    }
    used[ea[e]] = 1; used[eb[e]] = 1;
  }
}

// the free nodes: every used node but the gauge (`fixed`, -1: none), numbered in insertion order
inline void number_free_nodes(const std::vector<uint8_t> & used, int32_t fixed, std::vector<int32_t> & free_of_node, std::vector<int32_t> & node_of_free)
{
  const int32_t N = static_cast<int32_t>(used.size());
  free_of_node.assign(N, -1);
  node_of_free.clear();
  for (int32_t i = 0; i < N; ++i) {
    if (used[i] && i != fixed) {free_of_node[i] = static_cast<int32_t>(node_of_free.size()); node_of_free.push_back(i);}
  }
}

// Adjacency of the free nodes (CSR: sorted, duplicate-free, no self loops) and the BSR pattern of H: a row's neighbours with the
// diagonal block in its sorted place; slot_row[k] is the row of slot k, diag[i] the slot of block (i, i).
struct Pattern
{
  std::vector<int32_t> adj_ptr, adj_idx, row_ptr, col, slot_row, diag;
  int32_t n_slots() const {return static_cast<int32_t>(col.size());}
};
constexpr int32_t kRowBlock = 1024;

inline void build_pattern(const std::vector<int32_t> & ea, const std::vector<int32_t> & eb, const std::vector<int32_t> & free_of_node, int32_t nf,
                          const ParallelFor & parallel_for, Pattern & p)
{
  const int32_t E = static_cast<int32_t>(ea.size());
  // flat CSR arrays, counting passes: no per-row vectors
  std::vector<int32_t> deg(nf + 1, 0);
  for (int32_t e = 0; e < E; ++e) {
    const int32_t fa = free_of_node[ea[e]], fb = free_of_node[eb[e]];
    if (fa >= 0 && fb >= 0 && fa != fb) {++deg[fa + 1]; ++deg[fb + 1];}
  }
  for (int32_t i = 0; i < nf; ++i) {deg[i + 1] += deg[i];}
  std::vector<int32_t> nbr(deg[nf]), fill(deg.begin(), deg.end() - 1);
  for (int32_t e = 0; e < E; ++e) {
    const int32_t fa = free_of_node[ea[e]], fb = free_of_node[eb[e]];
    if (fa >= 0 && fb >= 0 && fa != fb) {nbr[fill[fa]++] = fb; nbr[fill[fb]++] = fa;}
  }
  // Rows are independent: blocks of rows on the host pool sort their lists in place, a serial prefix sum places the rows, the
  // blocks write them out.
  std::vector<int32_t> ucount(nf, 0);
  p.adj_ptr.assign(nf + 1, 0); p.row_ptr.assign(nf + 1, 0); p.diag.resize(nf);
  for_blocks(parallel_for, nf, kRowBlock, [&](int32_t i_begin, int32_t i_end) {
    for (int32_t i = i_begin; i < i_end; ++i) {
      int32_t * b = nbr.data() + deg[i], * e2 = nbr.data() + deg[i + 1];
      std::sort(b, e2);
      ucount[i] = static_cast<int32_t>(std::unique(b, e2) - b);
    }
  });
  for (int32_t i = 0; i < nf; ++i) {p.adj_ptr[i + 1] = p.adj_ptr[i] + ucount[i]; p.row_ptr[i + 1] = p.row_ptr[i] + ucount[i] + 1;}
  p.adj_idx.resize(p.adj_ptr[nf]); p.col.resize(p.row_ptr[nf]); p.slot_row.resize(p.row_ptr[nf]);
  for_blocks(parallel_for, nf, kRowBlock, [&](int32_t i_begin, int32_t i_end) {
    for (int32_t i = i_begin; i < i_end; ++i) {
      const int32_t * b = nbr.data() + deg[i], * e2 = b + ucount[i];
      std::copy(b, e2, p.adj_idx.begin() + p.adj_ptr[i]);
      int32_t at = p.row_ptr[i];
      bool placed = false;
      for (const int32_t * q = b; q < e2; ++q) {
        if (!placed && *q > i) {p.diag[i] = at; p.col[at] = i; p.slot_row[at] = i; ++at; placed = true;}
        p.col[at] = *q; p.slot_row[at] = i; ++at;
      }
      if (!placed) {p.diag[i] = at; p.col[at] = i; p.slot_row[at] = i; ++at;}
    }
  });
}

// Contribution lists of the gather kernels, CSR: slot k sums the entries e * 4 + kind of slot_list[slot_ptr[k] .. slot_ptr[k + 1])
// (kind 0 / 1: the diagonal block of edge e's first / second node, 2 / 3: block (a, b) / (b, a)), free node i the entries
// e * 2 + role of node_list.  Two counting passes in edge order: ascending edge index within every slot / node.
struct Contributions
{
  std::vector<int32_t> slot_ptr, slot_list, node_ptr, node_list;
};

inline void build_contributions(const std::vector<int32_t> & ea, const std::vector<int32_t> & eb, const std::vector<int32_t> & free_of_node, int32_t nf,
                                const Pattern & p, Contributions & c)
{
  const int32_t E = static_cast<int32_t>(ea.size()), n_slots = p.n_slots();
  auto slot_of = [&](int32_t i, int32_t j) {
    const auto b = p.col.begin() + p.row_ptr[i], e2 = p.col.begin() + p.row_ptr[i + 1];
    return static_cast<int32_t>(std::lower_bound(b, e2, j) - p.col.begin());
  };
  std::vector<int32_t> & scp = c.slot_ptr, & ncp = c.node_ptr, & scl = c.slot_list, & ncl = c.node_list;
  scp.assign(n_slots + 1, 0); ncp.assign(nf + 1, 0);
  std::vector<int32_t> e_slots(static_cast<size_t>(E) * 4, -1);
  for (int32_t e = 0; e < E; ++e) {
    const int32_t fa = free_of_node[ea[e]], fb = free_of_node[eb[e]];
    if (fa >= 0) {e_slots[4 * e + 0] = p.diag[fa]; ++scp[p.diag[fa] + 1]; ++ncp[fa + 1];}
    if (fb >= 0) {e_slots[4 * e + 1] = p.diag[fb]; ++scp[p.diag[fb] + 1]; ++ncp[fb + 1];}
    if (fa >= 0 && fb >= 0 && fa != fb) {
      e_slots[4 * e + 2] = slot_of(fa, fb); e_slots[4 * e + 3] = slot_of(fb, fa);
      ++scp[e_slots[4 * e + 2] + 1]; ++scp[e_slots[4 * e + 3] + 1];
    }
  }
  for (int32_t k = 0; k < n_slots; ++k) {scp[k + 1] += scp[k];}
  for (int32_t i = 0; i < nf; ++i) {ncp[i + 1] += ncp[i];}
  scl.resize(scp[n_slots]); ncl.resize(ncp[nf]);
  std::vector<int32_t> sfill(scp.begin(), scp.end() - 1), nfill(ncp.begin(), ncp.end() - 1);
  for (int32_t e = 0; e < E; ++e) {
    const int32_t fa = free_of_node[ea[e]], fb = free_of_node[eb[e]];
    for (int kind = 0; kind < 4; ++kind) {
      const int32_t sl = e_slots[4 * e + kind];
      if (sl >= 0) {scl[sfill[sl]++] = e * 4 + kind;}
    }
    if (fa >= 0) {ncl[nfill[fa]++] = e * 2 + 0;}
    if (fb >= 0) {ncl[nfill[fb]++] = e * 2 + 1;}
  }
}

// Where every block of the pattern lands in its front: slot_dest[k] the offset (doubles) of its first entry in the fronts, slot_ld[k]
// the front's leading dimension; -1 / 0 for a block above the diagonal in elimination order.  Independent per slot, blocks of
// slots on the host pool.  False: an entry of the matrix lies outside its front (the analysis does not fit the pattern).
constexpr int32_t kSlotBlock = 8192;

inline bool place_slots(const Symbolic & sym, const Pattern & p, const ParallelFor & parallel_for, std::vector<int64_t> & slot_dest,
                        std::vector<int32_t> & slot_ld)
{
  const int32_t n_slots = p.n_slots();
  slot_dest.assign(n_slots, -1); slot_ld.assign(n_slots, 0);
  std::atomic<int> outside{0};
  for_blocks(parallel_for, n_slots, kSlotBlock, [&](int32_t k_begin, int32_t k_end) {
    for (int32_t k = k_begin; k < k_end; ++k) {
      const int32_t ei = sym.elim_of_free[p.slot_row[k]], ej = sym.elim_of_free[p.col[k]];
      if (ei < ej) {continue;}
      const int32_t f = sym.sn_of_elim[ej];
      const int32_t ncols = sym.front_ns[f] / 3;
      const int32_t colpos = ej - sym.front_first[f];
      int32_t rowpos;
      if (ei < sym.front_first[f] + ncols) {
        rowpos = ei - sym.front_first[f];
      } else {
        const auto b = sym.rows.begin() + sym.rows_ptr[f], e2 = sym.rows.begin() + sym.rows_ptr[f + 1];
        auto it = std::lower_bound(b, e2, ei);
        if (it == e2 || *it != ei) {outside.store(1); continue;}
        rowpos = ncols + static_cast<int32_t>(it - b);
      }
      slot_dest[k] = sym.front_off[f] + 3 * rowpos + static_cast<int64_t>(3 * colpos) * sym.front_m[f];
      slot_ld[k] = sym.front_m[f];
    }
  });
  return outside.load() == 0;
}

// The supernodes of an earlier dissection, kept by node id, as supernodes of this problem: every list with its ids replaced by
// their free indices (ascending), the ids that have left dropped and emptied lists with them.  id_of_free(f) is the id of free node
// f; placed[f] says whether a list holds f.  Returns how many free nodes were placed.
// node id -> free index: a table when the ids are dense (a mapper's scan ids are), a hash map otherwise
template <class IdOfFree>
int32_t map_cached_supernodes(const std::vector<std::vector<int32_t>> & cached_sn_ids, int32_t nf, IdOfFree id_of_free,
                              std::vector<std::vector<int32_t>> & sn, std::vector<uint8_t> & placed)
{
  int32_t id_lo = INT32_MAX, id_hi = INT32_MIN;
  for (int32_t f = 0; f < nf; ++f) {const int32_t id = id_of_free(f); id_lo = std::min(id_lo, id); id_hi = std::max(id_hi, id);}
  const bool dense_ids = nf > 0 && static_cast<int64_t>(id_hi) - id_lo < 8 * static_cast<int64_t>(nf) + 1024;
  std::vector<int32_t> free_of_dense;
  std::unordered_map<int32_t, int32_t> free_of_id;
  if (dense_ids) {
    free_of_dense.assign(static_cast<size_t>(id_hi - id_lo) + 1, -1);
    for (int32_t f = 0; f < nf; ++f) {free_of_dense[static_cast<size_t>(id_of_free(f) - id_lo)] = f;}
  } else {
    free_of_id.reserve(static_cast<size_t>(nf) * 2);
    for (int32_t f = 0; f < nf; ++f) {free_of_id[id_of_free(f)] = f;}
  }
  auto free_index = [&](int32_t id) -> int32_t {
    if (dense_ids) {return (id >= id_lo && id <= id_hi) ? free_of_dense[static_cast<size_t>(id - id_lo)] : -1;}
    const auto it = free_of_id.find(id);
    return it != free_of_id.end() ? it->second : -1;
  };
  placed.assign(nf, 0);
  int32_t kept = 0;
  sn.clear();
  sn.reserve(cached_sn_ids.size() + 1);
  for (const auto & ids : cached_sn_ids) {
    std::vector<int32_t> g;
    g.reserve(ids.size());
    for (int32_t id : ids) {
      const int32_t f = free_index(id);
      if (f >= 0) {g.push_back(f); placed[f] = 1; ++kept;}
    }
    if (!g.empty()) {std::sort(g.begin(), g.end()); sn.push_back(std::move(g));}
  }
  return kept;
}

}  // namespace spa
}  // namespace kh
