// One round of marginalizing node removal (kh_spa_marginalize_nodes): what spa_marginalize.cpp packs and marginalize.hip reads.
#pragma once
#include <cstdint>

namespace kh
{

constexpr int32_t kMargMaxDegree = 64;     // one lane per neighbour entry, one wave per node

// Device view of a round.  All pointers are device pointers into the round's upload (inputs) and download (outputs).
// A constraint travels as 9 doubles: z (3) and the upper triangle of its information (00 01 02 11 12 22).
struct MargDev
{
  int32_t n_nodes;               // nodes of the round with 2 .. 64 neighbour entries
  const int32_t * ent_ptr;       // n_nodes + 1: a node's entries, in the order of its first constraint to each neighbour
  const int32_t * ent_id;        // per entry: the neighbour's id (ties of the hub choice go to the lowest)
  const int32_t * con_ptr;       // entries + 1: an entry's constraints, in constraint order (more than one: parallel constraints)
  const int32_t * con_dir;       // per such constraint: 0 stored node -> neighbour, 1 stored neighbour -> node
  const double * con_d;          // 9 per such constraint
  const int32_t * pair_ptr;      // n_nodes + 1: the first existing constraint of every pair of the node's neighbours that has one
  const int32_t * pair_ent;      // per pair: lo | hi << 8 | dir << 16, lo < hi entry numbers within the node; dir 0: stored lo -> hi
  const double * pair_d;         // 9 per pair
  const int32_t * out_ptr;       // n_nodes + 1: prefix over (entries - 1): where the node's new constraints go
  double * out_d;                // 9 per output slot: the constraint hub -> neighbour, or the existing constraint with it fused in
  int32_t * out_i;               // 2 per output slot: the hub's entry number; the pair it was fused into (-1: none, it is new)
};

void marginalize_launch_round(const MargDev & d, void * stream);

// one edit of the last kh_spa_marginalize_nodes, in the order it was made (the mapper mirrors them): kind 0: constraint a -> b
// appended (a = the hub of node `via`); 1: the existing constraint a -> b took a new one in; 2: node `via` left (after its 0 / 1 edits)
struct MargEdit {int32_t kind, via, a, b; double z[3], omega[6];};

}  // namespace kh
