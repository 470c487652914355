// The segment table of the flat parameter buffer as the kernels take it, by value in their arguments, and its two tests
// (csrc/misc.hip's `_seg` kernels, csrc/tensor_walk.h) -- gfx950.  Segments are sorted, disjoint unions of whole tensors
// with bounds that are multiples of 4.  In an unnamed namespace, as the kernels that take a SegTable are.
#pragma once
#include "common.h"
#include "../../include/svit_hip.h"

namespace {
struct SegTable {
  int64_t v[SVIT_MAX_SEGS][2];
  int32_t S;
};

// is the position inside a segment?  S == 0: every position is.  A tensor is trainable when its begin is (segments are
// unions of whole slots, so every position of the tensor then is)
__device__ __forceinline__ bool trainable(const SegTable& T, int64_t i) {
  if (T.S == 0) return true;
  bool in = false;
  for (int j = 0; j < T.S; ++j) in |= (i >= T.v[j][0]) & (i < T.v[j][1]);
  return in;
}

// is the quad at float index i, which lies in the window [lo, hi), inside a segment?  k: first segment that ends past lo,
// a cursor that only moves forward.  S == 0: no -- or, for the caller to whom no table means the whole buffer, yes
template <bool EMPTY_IS_ALL = false>
__device__ __forceinline__ bool seg_inside(const SegTable& t, int& k, int64_t lo, int64_t hi, int64_t i) {
  if (EMPTY_IS_ALL && t.S == 0) return true;
  while (k < t.S && t.v[k][1] <= lo) ++k;
  bool in = false;
  for (int j = k; j < t.S && t.v[j][0] < hi; ++j) in |= (i >= t.v[j][0]) & (i < t.v[j][1]);
  return in;
}
}  // namespace
