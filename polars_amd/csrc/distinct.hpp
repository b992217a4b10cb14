// distinct.hpp -- the arithmetic of n_unique / unique(), one body for the kernels and for the host (the idiom of quantile.hpp and variance.hpp: PLX_HD functions
// compiled into segment_distinct_kernel / distinct_keep_kernel, into the host side of the routes and into a host program that tests/emu/distinct_main.cpp drives
// under ASan + UBSan).
//
// Both operators are runs of equal values in a sorted order.  A run starts where the head mask has a bit; the distinct values of the sorted
// positions [a, b) are the bits of that mask in [a, b), which two ranks give in O(1): rank_before(b) - rank_before(a).
#pragma once
#include <stdint.h>

#include "../../include/polars_amd.h"

#ifndef PLX_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define PLX_HD __host__ __device__
#else
#define PLX_HD
#endif
#endif

namespace plx {
namespace distinct {

PLX_HD inline int popcount64(uint64_t x) { return __builtin_popcountll(x); }

// set bits of `mask` at positions below i.  prefix[w] = set bits of the words before word w (an exclusive prefix with one entry per word and one more for the total,
// so i may be the number of bits itself).  The word of i is read only when i is not at its first bit: i == 64 * words reads nothing past the mask.
PLX_HD inline uint64_t rank_before(const uint64_t* prefix, const uint64_t* mask, uint64_t i) {
  const uint64_t w = i >> 6;
  const unsigned b = (unsigned)(i & 63);
  uint64_t r = prefix[w];
  if (b) r += (uint64_t)popcount64(mask[w] & ((1ull << b) - 1));
  return r;
}

// ---- unique(keep=) ----
PLX_HD inline bool keep_ok(int keep) { return keep >= PLX_UNIQUE_ANY && keep <= PLX_UNIQUE_NONE; }
// the strategy that runs: "any" is served as "first"
PLX_HD inline int keep_served(int keep) { return keep == PLX_UNIQUE_ANY ? PLX_UNIQUE_FIRST : keep; }
inline const char* keep_name(int keep) {
  switch (keep) {
    case PLX_UNIQUE_ANY: return "any";
    case PLX_UNIQUE_FIRST: return "first";
    case PLX_UNIQUE_LAST: return "last";
    case PLX_UNIQUE_NONE: return "none";
    default: return "?";
  }
}
// a row of a class of equal rows, sorted stably: is_head = it is the class's first row in row order, is_tail = its last
PLX_HD inline bool keep_row(bool is_head, bool is_tail, int keep) {
  switch (keep) {
    case PLX_UNIQUE_LAST: return is_tail;
    case PLX_UNIQUE_NONE: return is_head && is_tail;
    default: return is_head;      // first, any
  }
}

// ---- the bitmap route of a whole column ----
// one bit per value of the range [min, max]: legal when the bitmap is at most 8 B a row or 128 KB, whichever is larger -- its memset and popcount then move no more
// than one read of a 64-bit column
constexpr uint64_t kBitmapFloorBits = 128ull * 1024 * 8;
PLX_HD inline bool bitmap_route_ok(uint64_t range, uint64_t n) {
  const uint64_t by_rows = n > (~0ull >> 6) ? ~0ull : n * 64;
  return range >= 1 && range <= (by_rows > kBitmapFloorBits ? by_rows : kBitmapFloorBits);
}

}  // namespace distinct
}  // namespace plx
