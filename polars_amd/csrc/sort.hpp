// sort.hpp -- stable multi-key arg-sort and top-k selection (kernels_sort.hip).
// Replaces, for primitive key columns,
//   arg_sort / arg_sort_multiple   polars-core/src/chunked_array/ops/sort/{mod.rs, arg_sort_multiple.rs, arg_sort.rs}
//   SortExec                       polars-mem-engine/src/executors/sort.rs
//   sort + slice -> top-k          polars-plan/src/plans/optimizer/slice_pushdown_lp.rs, polars-stream/src/nodes/top_k.rs
// Order (arg_sort.rs / total_ord.rs): nulls first unless nulls_last (an absolute position, not flipped by
// `descending`); floats in total order with NaN greatest and -0.0 == +0.0; ties keep input order.
#pragma once
#include <string>
#include <vector>

#include "core.hpp"

namespace plx {
namespace sort {

struct SortKey {
  ColumnPtr col;
  bool descending = false;
  bool nulls_last = false;
};

// PLX_U32 row indices of the first `limit` rows (limit < 0: all rows) of the stable sort by `keys`.
ColumnPtr sort_indices(const std::vector<SortKey>& keys, int64_t limit, std::string* desc);

// Key-only stable LSD radix sort of m 64-bit codes (a device buffer of m * 8 bytes) by their digits first_digit .. 7, least significant first (first_digit = 4:
// by the high 32 bits only, rows with equal high halves keep their input order).  Digits on which every key agrees cost no pass.  Returns the buffer that holds the
// sorted codes (`keys` itself or a scratch buffer of the same size; the other one is released); *passes / *skipped (may be null) = digit passes run / skipped.
Buf sort_keys_u64(Buf keys, int64_t m, int first_digit, int* passes, int* skipped);

// ---- median / quantile (quantile.hpp holds the arithmetic and the inverse of the value codes) ----
// The value codes at ranks lo and hi (hi == lo or lo + 1, both below n_valid >= 1) among the valid rows of `col` in the sort's order: an MSD radix select, the
// column is never sorted.  *desc = "quantile_select[rows=, valid=, rounds=R, next=none|same|min_pass]": R digit rounds ran (digits on which every valid row agrees
// cost none); the code at hi is the one at lo when its multiplicity covers hi, the smallest greater code (one min pass) otherwise.
struct SelectedRanks { uint64_t code_lo = 0, code_hi = 0; };
SelectedRanks select_ranks(const ColumnPtr& col, int64_t n_valid, uint64_t lo, uint64_t hi, std::string* desc);

// Quantiles per group over sorted segments: one sort_indices(keys..., value; ascending, nulls last) whatever the number of (q, interpolation) pairs, the segment
// heads found through the permutation (segment_heads_kernel) and compacted into starts[G], one lane per group picking two values (segment_quantile_kernel).  One
// column per spec (Float64; Float32 for a Float32 value column; null for a group without a valid value), G rows in KEY-SORTED order -- the order of
// sort_indices(group keys; ascending, nulls last).  G must equal expect_groups (PLX_ERR_INVALID naming both otherwise).
constexpr int kSegmentMaxKeys = 8;
struct QuantileSpec { double q; int interpolation; };
std::vector<ColumnPtr> segment_quantiles(const std::vector<ColumnPtr>& keys, const ColumnPtr& value, const std::vector<QuantileSpec>& specs, int64_t expect_groups, std::string* sort_desc);
// inv[perm[i]] = i
ColumnPtr invert_permutation(const ColumnPtr& perm);

}  // namespace sort
}  // namespace plx
