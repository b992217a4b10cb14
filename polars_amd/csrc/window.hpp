// window.hpp -- the arithmetic of `expr.over(keys)`, one body for the kernels and for the host (the idiom of distinct.hpp and quantile.hpp: PLX_HD functions compiled
// into window_slots_kernel / window_group_ids_kernel / window_broadcast_kernel, into the host side of the routes and into a host program that
// tests/emu/window_main.cpp drives under ASan + UBSan).
//
// A window is a group-by whose G-row result goes back to the N rows.  The way back is a map row -> group: on the direct route the row's keys become a
// dense code that indexes a table of group ids, on the sorted route the rank of the row's segment in the sorted order does.
#pragma once
#include <stdint.h>

#include "../../include/polars_amd.h"
#include "distinct.hpp"

namespace plx {
namespace window {

constexpr int kMaxKeys = 8;        // key parts of one window (sort::kSegmentMaxKeys)
constexpr int kMaxOutputs = 8;     // output columns of one broadcast launch (k::kGatherMultiMax)

// ---- the route rule ----
// The direct route keeps one u32 slot per code of the keys' joint range R.  It is legal when the table costs no more than one read of a 64-bit column (4 R <= 8 n)
// or fits the L2 of one XCD (4 MiB), whichever is larger: the random slot reads then stay row-proportional or L2-sized.
constexpr uint64_t kSlotFloorBytes = 4ull << 20;
PLX_HD inline bool direct_route_ok(uint64_t range, uint64_t n) {
  const uint64_t by_rows = n > (~0ull >> 3) ? ~0ull : n * 8;
  const uint64_t bytes = by_rows > kSlotFloorBytes ? by_rows : kSlotFloorBytes;
  return range >= 1 && range <= bytes / 4;
}
// the product of the part ranges, 0 once it passes `cap` (or a part range is 0): no u64 overflow whatever the parts are
PLX_HD inline uint64_t joint_range(const uint64_t* part_ranges, int n_parts, uint64_t cap) {
  uint64_t r = 1;
  for (int j = 0; j < n_parts; j++) {
    const uint64_t p = part_ranges[j];
    if (p == 0 || r > cap / p) return 0;
    r *= p;
  }
  return r;
}

// ---- the key code of the direct route ----
// One key part: code = value - min in [0, span); a null is the one extra code `span` (only a column with a validity bitmap has it).  The joint code is
// sum(code_j * stride_j) with stride_0 = 1 and stride_j = stride_(j-1) * range_(j-1), range_j = span_j + (nullable ? 1 : 0).
struct KeyPart {
  const void* values;          // PLX_BOOL: the bitmap
  const uint64_t* validity;    // null: no nulls
  int64_t min;
  uint64_t span;               // max - min + 1 over the valid values (0: no valid value)
  uint64_t stride;
  int32_t dtype;
  int32_t nullable;            // the part range holds the null code
};
struct Keys {
  KeyPart part[kMaxKeys];
  int32_t n_parts;
  uint64_t range;              // the joint range R
};

PLX_HD inline bool bit_at(const uint64_t* words, int64_t i) { return (words[i >> 6] >> (i & 63)) & 1; }

// the value of row r of an integer or Boolean key as i64 (every integer dtype but U64, which the direct route never takes)
PLX_HD inline int64_t part_value(int dtype, const void* v, int64_t r) {
  switch (dtype) {
    case PLX_BOOL: return bit_at(reinterpret_cast<const uint64_t*>(v), r) ? 1 : 0;
    case PLX_I8: return reinterpret_cast<const int8_t*>(v)[r];
    case PLX_I16: return reinterpret_cast<const int16_t*>(v)[r];
    case PLX_I32: return reinterpret_cast<const int32_t*>(v)[r];
    case PLX_I64: return reinterpret_cast<const int64_t*>(v)[r];
    case PLX_U8: return reinterpret_cast<const uint8_t*>(v)[r];
    case PLX_U16: return reinterpret_cast<const uint16_t*>(v)[r];
    case PLX_U32: return reinterpret_cast<const uint32_t*>(v)[r];
    default: return 0;
  }
}
PLX_HD inline bool part_ok(int dtype) { return dtype == PLX_BOOL || (dtype >= PLX_I8 && dtype <= PLX_U32); }

// the joint code of row r; false when a part lies outside its range (bounds a caller declared and the data does not keep) or is null without a null code: the
// code is then no index of the table
PLX_HD inline bool row_code(const Keys& k, int64_t r, uint64_t* code) {
  uint64_t c = 0;
  for (int j = 0; j < kMaxKeys; j++) {
    if (j >= k.n_parts) break;
    const KeyPart& p = k.part[j];
    uint64_t off;
    if (p.validity && !bit_at(p.validity, r)) {
      if (!p.nullable) return false;
      off = p.span;
    } else {
      off = (uint64_t)part_value(p.dtype, p.values, r) - (uint64_t)p.min;
      if (off >= p.span) return false;
    }
    c += off * p.stride;
  }
  *code = c;
  return c < k.range;
}

// ---- the two maps ----
// direct: one lane per group g of the group frame, `gk` = the group frame's key columns under the ROW columns' min / span / stride
PLX_HD inline bool slot_store(const Keys& gk, int64_t g, uint32_t* slot) {
  uint64_t code;
  if (!row_code(gk, g, &code)) return false;
  slot[code] = (uint32_t)g;
  return true;
}
// sorted: position i of the rows' sorted order lies in segment rank_before(i + 1) - 1 (heads has bit 0 whenever n > 0); order[s] = the group of the s-th segment.
// The caller stores the result at gid[perm[i]].  n_groups as the answer: the segment has no group
PLX_HD inline uint32_t sorted_group(const uint64_t* prefix, const uint64_t* heads, const uint32_t* order, uint64_t n_groups, uint64_t i) {
  const uint64_t s = distinct::rank_before(prefix, heads, i + 1);
  return s >= 1 && s <= n_groups ? order[s - 1] : (uint32_t)n_groups;
}

// ---- the broadcast ----
// one output column of a launch: the G-row group column and the N-row result.  width 0: a Boolean column, values are bitmaps
struct Output {
  const void* src;
  const uint64_t* src_valid;   // null: the group column has no nulls, the result gets no validity
  void* dst;
  uint64_t* dst_valid;
  int32_t width;               // 0, 1, 2, 4, 8
};
struct Outputs { Output o[kMaxOutputs]; int32_t n; };

PLX_HD inline void copy_value(int width, const void* src, uint64_t g, void* dst, int64_t r) {
  switch (width) {
    case 1: reinterpret_cast<uint8_t*>(dst)[r] = reinterpret_cast<const uint8_t*>(src)[g]; break;
    case 2: reinterpret_cast<uint16_t*>(dst)[r] = reinterpret_cast<const uint16_t*>(src)[g]; break;
    case 4: reinterpret_cast<uint32_t*>(dst)[r] = reinterpret_cast<const uint32_t*>(src)[g]; break;
    case 8: reinterpret_cast<uint64_t*>(dst)[r] = reinterpret_cast<const uint64_t*>(src)[g]; break;
    default: break;
  }
}
// what lane `r` of a wave contributes to the ballots of one output: bit 0 = the group's value is valid, bit 1 = a Boolean group value is true.  `ok` = the row
// has a group (rows past n and rows without one contribute nothing: the tail wave's ballots are masked by it)
PLX_HD inline unsigned lane_bits(const Output& o, bool ok, uint64_t g) {
  if (!ok) return 0u;
  unsigned b = (!o.src_valid || bit_at(o.src_valid, (int64_t)g)) ? 1u : 0u;
  if (o.width == 0 && bit_at(reinterpret_cast<const uint64_t*>(o.src), (int64_t)g)) b |= 2u;
  return b;
}

}  // namespace window
}  // namespace plx
