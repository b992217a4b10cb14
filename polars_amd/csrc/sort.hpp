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

}  // namespace sort
}  // namespace plx
