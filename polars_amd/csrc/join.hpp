// join.hpp -- hash join on one key column pair (kernels_join.hip) or on a key of several columns (kernels_join_wide.hip).
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
void join_indices(int how, const ColumnPtr& left_key, const ColumnPtr& right_key, ColumnPtr& left_idx, ColumnPtr& right_idx, std::string* desc, bool* dup_build_keys = nullptr);
// The same contract on a key of 2..8 columns of any integer / Boolean / float dtype (kernels_join_wide.hip; column j has one dtype on both sides, a null in any part makes
// the row's key null).  The table holds row ids, the key words are compared at the build columns; *desc = "wide_hash_join[words=N, ...]" / wide_hash_semi_join / wide_hash_anti_join.
void join_indices_wide(int how, const std::vector<ColumnPtr>& left_keys, const std::vector<ColumnPtr>& right_keys, ColumnPtr& left_idx, ColumnPtr& right_idx, std::string* desc,
                       bool* dup_build_keys = nullptr);

// Pairs of an inner / left join from a build table the fused build scan filled (fused::JoinAggTable: unique keys, or chains of rows per key) over a candidate
// list of probe rows (`cand`: PLX_U32, null = every row of probe_key).  Pair order = candidate order; a left join keeps every candidate (build_idx nullable).
void join_pairs(int how, const ColumnPtr& probe_key, const ColumnPtr& cand, const fused::JoinAggTable& t, ColumnPtr& probe_idx, ColumnPtr& build_idx, std::string* desc);

// the same against a direct-address build table (unique build keys over a dense range: bitmap + rank, fused::DirectJoinTable) and its slot -> build row map
void join_pairs_direct(int how, const ColumnPtr& probe_key, const ColumnPtr& cand, const fused::DirectJoinTable& dt, const uint32_t* slot_row, ColumnPtr& probe_idx, ColumnPtr& build_idx,
                       std::string* desc);

// ---- the order of the pair list (kernels_join_order.hip; plx_ir.maintain_order of a PLX_IR_JOIN node, plx_join_order) ----
// What the producer of a pair list guarantees: probe_ordered = probe index non-decreasing (join_indices; join_pairs over a candidate list in row order);
// runs_ordered = inside one probe row the build index increases (unique build keys; not chains).
struct PairProps { bool probe_ordered = false, runs_ordered = false; };
// Puts (probe_idx, build_idx) into `order` (plx_join_order; NONE: untouched, *desc left empty).  probe_is_left: the probe side is the join's left input.  A left join's
// nullable build_idx keeps its nulls (kNoRow -> validity is rebuilt when rows moved).  *desc = "order=<name>: <what was done>".
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
