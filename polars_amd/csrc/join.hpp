// join.hpp -- hash join on one key column pair (kernels_join.hip) or on a key of several columns (kernels_join_wide.hip); both are one driver and one set of row loops
// (join_driver.hpp) under a key policy per route.
// Replaces polars-ops/src/frame/join/hash_join/{single_keys.rs:16-167 (build_tables),
// single_keys_inner.rs:11-149 (probe_inner / hash_join_tuples_inner),
// single_keys_left.rs:106-195, single_keys_dispatch.rs:234-357,476-553}.
#pragma once
#include <string>
#include <vector>

#include "core.hpp"
#include "fused.hpp"

namespace plx {
namespace join {

// (left_idx, right_idx) as PLX_U32 columns; LEFT join: right_idx nullable.  Pairs come out in probe order (the probe side is the left one unless an inner join's
// left side is not the larger one); *dup_build_keys (may be null; inner / left) = the build side repeats a key, so the pairs of one probe row are in chain order.
// RIGHT join: the left join with the sides exchanged (the probe side is the right one, left_idx nullable).  FULL join: the build side is the shorter one as for an
// inner join; the pairs of the probe side's left join come first, in probe order, then one pair (no probe row, build row) per build row that no probe row
// matched -- null-key build rows among them -- in build row order; both index columns are nullable, *unmatched_build (may be null) = the length of that tail,
// *desc = "hash_full_join[build=<side> ..., unmatched build rows=N]".
void join_indices(int how, const ColumnPtr& left_key, const ColumnPtr& right_key, ColumnPtr& left_idx, ColumnPtr& right_idx, std::string* desc, bool* dup_build_keys = nullptr,
                  int64_t* unmatched_build = nullptr);
// The same contract on a key of 2..8 columns of any integer / Boolean / float dtype (kernels_join_wide.hip; column j has one dtype on both sides, a null in any part makes
// the row's key null).  The table holds row ids, the key words are compared at the build columns; *desc = "wide_hash_join[words=N, ...]" / wide_hash_semi_join / wide_hash_anti_join /
// wide_hash_full_join; `why` (may be empty) = the caller's reason for this route, written behind the word count: "wide_hash_join[words=N (why), ...]".
void join_indices_wide(int how, const std::vector<ColumnPtr>& left_keys, const std::vector<ColumnPtr>& right_keys, ColumnPtr& left_idx, ColumnPtr& right_idx, std::string* desc,
                       bool* dup_build_keys = nullptr, int64_t* unmatched_build = nullptr, const std::string& why = std::string());
// The coalesced key column of a full join: lkey at left_idx where the pair has a left row, rkey at right_idx otherwise; validity from the side that was read.
// Key columns of one dtype, 1 / 2 / 4 / 8 bytes wide.
ColumnPtr coalesce_keys(const ColumnPtr& lkey, const ColumnPtr& rkey, const ColumnPtr& left_idx, const ColumnPtr& right_idx);

// Pairs of an inner / left join from a build table the fused build scan filled (fused::JoinAggTable: unique keys, or chains of rows per key) over a candidate
// list of probe rows (`cand`: PLX_U32, null = every row of probe_key).  Pair order = candidate order; a left join keeps every candidate (build_idx nullable).
void join_pairs(int how, const ColumnPtr& probe_key, const ColumnPtr& cand, const fused::JoinAggTable& t, ColumnPtr& probe_idx, ColumnPtr& build_idx, std::string* desc);

// the same against a direct-address build table (unique build keys over a dense range: bitmap + rank, fused::DirectJoinTable) and its slot -> build row map
void join_pairs_direct(int how, const ColumnPtr& probe_key, const ColumnPtr& cand, const fused::DirectJoinTable& dt, const uint32_t* slot_row, ColumnPtr& probe_idx, ColumnPtr& build_idx,
                       std::string* desc);

// ---- the order of the pair list (kernels_join_order.hip; plx_ir.maintain_order of a PLX_IR_JOIN node, plx_join_order) ----
// What the producer of a pair list guarantees: probe_ordered = probe index non-decreasing (join_indices; join_pairs over a candidate list in row order);
// runs_ordered = inside one probe row the build index increases (unique build keys; not chains).
// build_tail (full joins; -1: not a full join) = the last build_tail pairs are (no probe row, unmatched build row) in build row order, the pairs before them have a probe row.
struct PairProps { bool probe_ordered = false, runs_ordered = false; int64_t build_tail = -1; };
// Puts (probe_idx, build_idx) into `order` (plx_join_order; NONE: untouched, *desc left empty).  probe_is_left: the probe side is the join's left input.  A left / right
// join's nullable build_idx keeps its nulls (kNoRow -> validity is rebuilt when rows moved).  A full join (props.build_tail >= 0): the rows that carry an index of the
// primary side come first, in the order asked; the rows without one follow in increasing row index of the other side.  *desc = "order=<name>: <what was done>".
void order_pairs(int order, bool probe_is_left, PairProps props, ColumnPtr& probe_idx, ColumnPtr& build_idx, std::string* desc);
// A candidate list that is in partition order (k::partitioned_probe_hits / k::partitioned_hash_probe_hits) back into row order: key-only radix of the u32 row ids.
void restore_candidate_order(ColumnPtr& cand, std::string* desc);
// does `order` need the pair list in probe order to take a cheap branch of order_pairs (primary = probe side, or a secondary order is asked)?
bool join_order_needs_probe_order(int order, bool probe_is_left);
const char* join_order_name(int order);

// HashPartitioner (polars-utils/src/hashing.rs:72-121): rows grouped by partition.
void hash_partition(const ColumnPtr& key, int n_partitions, uint64_t seed, ColumnPtr& perm, int64_t* counts_out);
// same, the per-partition row counts stay on the device ([n_partitions] u64): no host round trip (the exchange all-gathers them)
void hash_partition_dev(const ColumnPtr& key, int n_partitions, uint64_t seed, ColumnPtr& perm, Buf& counts_dev);

}  // namespace join
}  // namespace plx
