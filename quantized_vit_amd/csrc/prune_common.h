// The device tables of the declared row groups, shared by prune_step.hip (the pruning stages) and group_lasso.hip
// (the penalty over the same groups): one definition of the descriptors, of the 16-byte rule and of the item check.
#pragma once
#include "reduce_common.h"

namespace {

struct PruneMember {    // 48 B
  float* p;
  const float* grad;    // NULL: no update (pruned rows are still zeroed), no part in the sums
  float* m;
  float* v;
  int64_t width;        // elements per row
  int32_t quantized;    // 1: the group's layer's weight (clip, res and quantize by its weight quantizer)
  int32_t flags;        // bit 0: this tensor's first step
};
struct PruneGroup {     // 64 B
  float* d;             // weight quantizer scalars of the group's layer; t NULL: the linear type
  const float* qm;
  const float* t;
  int32_t member_begin, member_count;
  int32_t rows;
  int32_t joint;        // 1: the joint stage (active redundant rows); 0: the stage path
  int32_t red_begin, red_count;   // its redundant rows' partials
  int64_t elems;        // elements per unit over all members
  int32_t sections, unit_rows;    // 0 as 1; both 1: a unit is one row
};
struct PruneItem {      // 16 B
  int32_t group, row;
  int32_t state;        // 0 important, 1 active redundant, 2 pruned
  int32_t link;         // a row item: the row's unit (0 where a unit is one row); a unit entry of the fold (row = the
                        // unit): the index in the row items of row 0 of its group
};
QVIT_DEV int64_t rows_per_unit(const PruneGroup& G) {
  return (int64_t)(G.sections > 1 ? G.sections : 1) * (G.unit_rows > 1 ? G.unit_rows : 1);
}

QVIT_DEV bool member_vec(const PruneMember& t) {
  return ((((uintptr_t)t.p | (uintptr_t)t.grad | (uintptr_t)t.m | (uintptr_t)t.v) & 15) == 0) && (t.width & 3) == 0;
}

// an item's group, checked against the tables; false: the item is skipped
QVIT_DEV bool item_group(const PruneItem& it, const PruneGroup* groups, int ngroups, int nmembers, PruneGroup& G) {
  if ((uint32_t)it.group >= (uint32_t)ngroups) return false;
  G = groups[it.group];
  return (uint32_t)it.row < (uint32_t)G.rows && G.member_begin >= 0 && G.member_count >= 0 &&
         (int64_t)G.member_begin + G.member_count <= nmembers;
}

}  // namespace
