// adamw_groups.hpp -- the range table of spa3d_adamw_step_groups (include/spa3d.h): its validation, and the map element -> range.
// Plain C++, host- and device-callable: the entry point validates the caller's table with adamw_groups_check, the grouped optimizer kernels
// of loss.hip resolve elements with adamw_group_find / adamw_group_at, and the g++ host test (tests/host/adamw_groups_check.cpp) runs both.
//
// A table is `num` ranges [begin, end) of the n elements handed to the call, sorted ascending and disjoint, each with a learning-rate and a
// weight-decay multiplier; an element in no range has both multipliers 1; lr_scale == 0 freezes a range.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ADAMW_G_HD __host__ __device__ __forceinline__
#else
#define ADAMW_G_HD inline
#endif

constexpr int ADAMW_MAX_GROUPS = 4096;

// the table as the kernels read it (and as spa3d_param_group lays it out): 24 bytes, six 32-bit words
struct AdamwGroup { int64_t begin, end; float lr_scale, wd_scale; };
constexpr int ADAMW_GROUP_WORDS = 6;
static_assert(sizeof(AdamwGroup) == 4 * ADAMW_GROUP_WORDS, "AdamwGroup is six 32-bit words");

enum AdamwGroupsError {
  ADAMW_G_OK = 0,
  ADAMW_G_COUNT,     // num outside [0, 4096]
  ADAMW_G_NULL,      // num > 0 without a table
  ADAMW_G_BOUNDS,    // begin < 0 or end > n
  ADAMW_G_EMPTY,     // begin >= end
  ADAMW_G_ORDER,     // begins before the previous range ends: unsorted or overlapping
  ADAMW_G_SCALE,     // a multiplier that is negative or not finite
};

// G: anything with begin, end, lr_scale, wd_scale.  *bad (optional) = the first offending range.
template <typename G> inline AdamwGroupsError adamw_groups_check(const G* g, int64_t num, int64_t n, int* bad = nullptr) {
  if (bad) *bad = -1;
  if (num < 0 || num > ADAMW_MAX_GROUPS) return ADAMW_G_COUNT;
  if (num > 0 && !g) return ADAMW_G_NULL;
  int64_t prev_end = 0;
  for (int k = 0; k < (int)num; ++k) {
    if (bad) *bad = k;
    if (g[k].begin < 0 || g[k].end > n) return ADAMW_G_BOUNDS;
    if (g[k].begin >= g[k].end) return ADAMW_G_EMPTY;
    if (g[k].begin < prev_end) return ADAMW_G_ORDER;
    // !(x >= 0) is true for a negative number and for NaN; x > FLT_MAX only for +inf
    if (!(g[k].lr_scale >= 0.f) || !(g[k].wd_scale >= 0.f) || g[k].lr_scale > 3.4028234664e38f || g[k].wd_scale > 3.4028234664e38f) return ADAMW_G_SCALE;
    prev_end = g[k].end;
  }
  if (bad) *bad = -1;
  return ADAMW_G_OK;
}
template <typename G> inline bool adamw_groups_any_frozen(const G* g, int num) {
  for (int k = 0; k < num; ++k) if (g[k].lr_scale == 0.f) return true;
  return false;
}

// The first range that ends beyond element i (num when there is none): a binary search over the sorted ends.  Range k holds i exactly when
// k < num and g[k].begin <= i; otherwise i lies in the gap before range k (or behind the last range).
template <typename G> ADAMW_G_HD int adamw_group_find(const G* g, int num, int64_t i) {
  int lo = 0, hi = num;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (g[mid].end <= i) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// The multipliers of element i >= the element k was found for: walks forward from k (elements are visited in ascending order, so the walk is
// short) and leaves k at the first range that ends beyond i.
template <typename G> ADAMW_G_HD void adamw_group_at(const G* g, int num, int& k, int64_t i, float& lr_scale, float& wd_scale) {
  while (k < num && g[k].end <= i) ++k;
  if (k < num && g[k].begin <= i) { lr_scale = g[k].lr_scale; wd_scale = g[k].wd_scale; }
  else { lr_scale = 1.f; wd_scale = 1.f; }
}
