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
#include "window.hpp"

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

// ---- sorted segments: what the grouped order statistics and the grouped distinct counts share ----
// The sorted order of ONE source column under the group keys: one sort_indices(keys..., value; ascending, nulls last), the segment heads found through the
// permutation (segment_heads_kernel) and compacted into starts[G].  The rows of a group are the positions [starts[g], starts[g + 1]) (the last segment ends at n),
// its valid values in order in front of its nulls; the G segments come in KEY-SORTED order -- the order of sort_indices(group keys; ascending, nulls last).  G must
// equal expect_groups (PLX_ERR_INVALID naming both otherwise).  Built once per distinct source column: `x.median(), x.n_unique()` run one sort.
constexpr int kSegmentMaxKeys = 8;
struct SortedSegments {
  ColumnPtr value;        // the source column
  ColumnPtr perm;         // PLX_U32[n]
  Buf heads;              // the segment-head mask, bitmap_bytes(n) (null when n == 0)
  Buf starts;             // u32[max(G, 1)]
  int64_t n = 0, n_groups = 0;
  std::string sort_desc;
};
// descending: the value sorts descending inside every segment (nulls stay last, ties keep row order); the keys never do.  No key at all: the whole column is one
// segment.  expect_groups < 0: no expectation.
SortedSegments sort_segments(const std::vector<ColumnPtr>& keys, const ColumnPtr& value, int64_t expect_groups, bool descending = false);
// The runs of equal values inside the segments of a sorted order: distinct_heads_kernel's mask (a position starts a segment, or its value differs from the position
// before; a null and a value differ, two nulls do not), its per-word prefix and its compacted positions starts[n_runs].  What rank reads beside the segments.
struct ValueRuns { Buf heads, prefix, starts; int64_t n_runs = 0; };
ValueRuns value_runs(const SortedSegments& seg);
// the exclusive prefix of a mask's per-word popcounts (words + 1 entries, the last the total): what distinct::rank_before reads
Buf mask_rank_prefix(const Buf& mask, int64_t n_bits);
// Quantiles per group: one lane per group picking two values (segment_quantile_kernel).  One column per spec (Float64; Float32 for a Float32 value column; null for
// a group without a valid value), G rows in the segments' order.
struct QuantileSpec { double q; int interpolation; };
std::vector<ColumnPtr> segment_quantiles(const SortedSegments& seg, const std::vector<QuantileSpec>& specs);
// Distinct values per group, a null counting as one: distinct_heads_kernel marks the positions that start a segment or whose value differs from the position before
// (null and value differ, two nulls do not), a per-word exclusive prefix of that mask's popcounts, and one lane per group taking the difference of two ranks
// (segment_distinct_kernel: O(1) per group).  PLX_U32 without validity, G rows in the segments' order.
ColumnPtr segment_distinct(const SortedSegments& seg);

// ---- n_unique of a whole column / distinct rows (distinct.hpp holds the arithmetic) ----
// The number of distinct values of `col` (integer, float or Boolean), a null counting as one.  *desc names the route: "n_unique[boolean]",
// "n_unique[bitmap range=R]" or "n_unique[sorted codes: passes=P, skipped=S]".  The rule takes the bitmap route wherever it is legal, so the only route there is
// to force is the sort's: force_sort sends an integer column that would take the bitmap through the sorted codes (Boolean and empty columns have one route).
uint32_t n_unique_column(const ColumnPtr& col, bool force_sort, std::string* desc);
// Row-order Boolean mask (no validity) of the rows unique(keep) keeps over 1..kSegmentMaxKeys key columns: one stable sort_indices over the keys, segment_heads_kernel,
// distinct_keep_kernel.  *kept (may be null: no count, no synchronisation) = the number of set bits; *sort_desc = the sort's description.
ColumnPtr distinct_rows(const std::vector<ColumnPtr>& keys, int keep, int64_t* kept, std::string* sort_desc);
// inv[perm[i]] = i
ColumnPtr invert_permutation(const ColumnPtr& perm);
// The segments of a sorted order by themselves: the head mask of `perm` (a sort_indices of all rows by `keys`; segment_heads_kernel), the exclusive prefix of its
// per-word popcounts (words + 1 entries: what distinct::rank_before reads) and the number of segments (one small download).  At least one row.
struct HeadRanks { Buf heads, prefix; int64_t n_segments = 0; };
HeadRanks segment_head_ranks(const std::vector<ColumnPtr>& keys, const ColumnPtr& perm);

}  // namespace sort

// ---- window expressions: the way back from a group frame to the rows (kernels_window.hip; window.hpp holds the arithmetic) ----
namespace window {
// The map row -> group of `keys` (N rows) against the keys of their group frame (G rows, any order).  direct: `table` = slot[R], read at the row's key code;
// sorted: `table` = gid[N].  desc = "window[direct range=R]" | "window[sorted rows: <sort description>]" | "window[empty]".  PLX_WINDOW_ROUTE=sort in the environment
// forces the sorted route.  On the sorted route the number of segments must be G (PLX_ERR_INVALID naming both otherwise).
struct RowMap {
  bool direct = false;
  int64_t n = 0, n_groups = 0;
  Keys keys{};                       // direct: the key parts of the rows
  std::vector<ColumnPtr> key_cols;   // ... and the columns they point into
  Buf table, flag;
  unsigned int* flag_ptr = nullptr;  // raised by a row or group without a place; read once by broadcast()
  std::string desc;
};
RowMap map_rows(const std::vector<ColumnPtr>& keys, const std::vector<ColumnPtr>& group_keys);
// One N-row column per G-row group column: row r holds the value and validity of its group (window_broadcast_kernel, one launch per kMaxOutputs columns).  A result
// has a validity bitmap only when its group column holds a null.  PLX_ERR_INVALID when a row has no group.
std::vector<ColumnPtr> broadcast(const RowMap& m, const std::vector<ColumnPtr>& group_cols);
}  // namespace window

// ---- cumulative and ranking functions (kernels_cumulative.hip; cumulative.hpp holds the arithmetic) ----
namespace cumulative {
// The order a partitioned scan walks: one stable sort_indices of the rows by the keys (rows of a partition stay in row order) and its segment-head mask.  Shared by
// every cumulative node of one key list.  No key: perm and heads stay null, the rows themselves are the order.
struct ScanOrder { ColumnPtr perm; Buf heads; int64_t n = 0; std::string desc; };      // desc: "cumulative[whole column]" | "cumulative[sorted rows: <sort>]"
ScanOrder scan_order(const std::vector<ColumnPtr>& keys, int64_t n);
// One cumulative function of `value` (any column dtype for PLX_CUM_COUNT; integer, float, Boolean otherwise) along `order`: a segmented inclusive scan in three
// launches (tile aggregates; their scan, recursive above one tile of tiles; the tiles with their carry).  The result shares the validity of `value`.
ColumnPtr scan_column(const ScanOrder& order, const ColumnPtr& value, int op, bool reverse);
// The sorted order rank reads: sort_segments(keys, value; descending as asked, nulls last), the prefix of its segment heads and the runs of equal values.
struct RankOrder { sort::SortedSegments seg; Buf seg_prefix; sort::ValueRuns runs; std::string desc; };      // desc: "rank[sorted segments: <sort>]"
RankOrder rank_order(const std::vector<ColumnPtr>& keys, const ColumnPtr& value, bool descending);
// One ranking method over `order`: O(1) per sorted position.  PLX_F64 ("average") or PLX_U32, the validity of the ranked column
ColumnPtr rank_column(const RankOrder& order, int method);
}  // namespace cumulative

// ---- shift / diff and the rolling functions (kernels_rolling.hip; rolling.hpp holds the arithmetic) ----
namespace rolling {
struct Params;
// What finds the segment of a sorted position in O(1) beside the order's head mask: the mask's per-word prefix and its compacted starts (cumulative::run_of).
// Built once per key list and shared by every shift / diff / rolling function over it; empty for the whole column.
struct Segments { Buf prefix, starts; int64_t n_segments = 0; };
Segments segments_of(const cumulative::ScanOrder& order);
// shift(n) / diff(n) of `value` along `order`: one launch.  fill (shift only): the value of the vacated rows, which are then valid; null: they are null.
// shift(0) returns `value` itself.
ColumnPtr shift_column(const cumulative::ScanOrder& order, const Segments& segs, const ColumnPtr& value, int64_t n, const plx_scalar* fill, bool diff);
// One rolling function (a plx_rolling_op) along `order`.  *route = "rolling[tile halo: w=.., lds=..]" | "rolling[two scans: w=.., launches=7]" | "rolling[empty]".
// tile_route_for(w): the route a window of w rows takes now (PLX_ROLLING_ROUTE=scans in the environment forces the two scans, read per call).
bool tile_route_for(int64_t w);
ColumnPtr rolling_column(const cumulative::ScanOrder& order, const Segments& segs, const ColumnPtr& value, int op, const Params& p, std::string* route);
}  // namespace rolling

// ---- join_asof (kernels_asof.hip; asof.hpp holds the arithmetic and the contract) ----
namespace asof {
// The matched right row of every left row: PLX_U32, len(left_on) rows in left order, a validity bitmap only when some row is unmatched.  how: a plx_asof_strategy,
// OR'd with PLX_ASOF_STRICT; left_by / right_by: 0..7 parts, part j of one dtype on both sides; tolerance: null, or .u for an integer `on`, .f64 for a float one.
// The right rows with a null key part are compacted away, the rest checked for order and sorted (sort::sort_indices by the parts then `on`) only when that fails;
// then one encode launch and one search launch.  Empty sides launch nothing.  *desc = "asof[backward, by=2, right=in order, rows=N x M, samples=S]" |
// "asof[..., right=sorted: <sort description>, dropped null keys=K, ...]" | "asof[empty]"; PLX_ASOF_ROUTE=global in the environment (read per call) searches
// without the LDS sample stage: samples=0.
ColumnPtr match(int how, const std::vector<ColumnPtr>& left_by, const std::vector<ColumnPtr>& right_by, const ColumnPtr& left_on, const ColumnPtr& right_on, const plx_scalar* tolerance,
                std::string* desc);
}  // namespace asof
}  // namespace plx
