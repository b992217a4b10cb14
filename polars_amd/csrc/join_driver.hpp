// join_driver.hpp -- the hash join that kernels_join.hip (one key word: a single key column, or several packed into one Int64) and kernels_join_wide.hip (a key of
// 2..8 columns) share: the chain part of the table, the three row loops (build, count, emit) and the host driver behind join_indices / join_indices_wide.
// A KEY POLICY per route (SingleKey in kernels_join.hip, WideKey in kernels_join_wide.hip) says what differs.  Device side: Keys (how a side's key is read) and Table (the slot
// storage next to the Chains); hash_row(keys, i, &h) -> false when row i's key is null; find_or_claim(table, build, i, h) -> the slot of build row i's key, claimed when the key is
// new; find(table, probe, i, build, h) -> the slot of probe row i's key or -1.  Host side: HostKeys and rows(); prepare() (the slot storage; wide: descriptor upload, tag bits); the
// three launches (the __global__ kernels keep their names and stay in their files as wrappers of the row loops); the plan-name prefix and bracket lead, the ProfileScope names and
// declared bytes; kSlotsBeyondCap and kRefuseLargeOutputAlways.
#pragma once
#include <algorithm>
#include <string>

#include "dev.hpp"
#include "join.hpp"
#include "join_keys.hpp"
#include "kernels.hpp"
#include "scan.hpp"

namespace plx {
namespace join {

// duplicates of a key form a chain: head[slot] = newest build row (atomicExch), next[row] = the previous head
struct Chains {
  unsigned int* head;        // [cap + P::kSlotsBeyondCap]
  unsigned int* next;        // [build rows]
  unsigned int* flags;       // [0] = a chain longer than 1 exists (build keys not unique)
  uint32_t log2_cap;
};

// ---------------------------------------------------------------------------------------------------------------- row loops ---
template <class P>
__device__ __forceinline__ void join_build_rows(const typename P::Keys& build, const typename P::Table& t) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < build.n; i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t h;
    const int64_t slot = P::hash_row(build, i, &h) ? P::find_or_claim(t, build, i, h) : -1;
    if (slot < 0) { t.ch.next[i] = kNoRow; continue; }
    const unsigned int old = atomicExch(&t.ch.head[slot], (unsigned int)i);
    t.ch.next[i] = old;
    if (old != kNoRow) t.ch.flags[0] = 1u;
  }
}

// counts[i] = number of build matches of probe row i (left join: at least 1).  kFlag (full join): matched[r] = 1 for every build row r on the chain -- several probe
// rows that hit one build row store the same byte, so no atomic is needed; the other join kinds run the instantiation without the store.
template <class P, bool kFlag>
__device__ __forceinline__ void join_count_rows(const typename P::Keys& probe, const typename P::Keys& build, const typename P::Table& t, int how, uint32_t* __restrict__ counts,
                                                uint8_t* __restrict__ matched) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < probe.n; i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t c = 0;
    uint64_t h;
    if (P::hash_row(probe, i, &h)) {
      const int64_t slot = P::find(t, probe, i, build, h);
      if (slot >= 0) { for (unsigned int r = t.ch.head[slot]; r != kNoRow; r = t.ch.next[r]) { c++; if constexpr (kFlag) matched[r] = 1; } }
    }
    // how: 0 inner, 1 left (unmatched rows emit one pair), 2 semi (row kept once if matched), 3 anti (kept if unmatched; null keys never match)
    counts[i] = how == 2 ? (c ? 1u : 0u) : how == 3 ? (c ? 0u : 1u) : (how == 1 && c == 0) ? 1u : c;
  }
}

// the pairs of probe row i at offsets[i], in chain order.  No write reaches offsets[i + 1], whatever the chains say; a row that counted no pair is not looked up again
template <class P>
__device__ __forceinline__ void join_emit_rows(const typename P::Keys& probe, const typename P::Keys& build, const typename P::Table& t, int left_join, const uint64_t* __restrict__ offsets,
                                               uint32_t* __restrict__ out_probe, uint32_t* __restrict__ out_build) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < probe.n; i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t o = offsets[i];
    const uint64_t end = offsets[i + 1];
    bool any = false;
    uint64_t h;
    if (o < end && P::hash_row(probe, i, &h)) {
      const int64_t slot = P::find(t, probe, i, build, h);
      if (slot >= 0) {
        for (unsigned int r = t.ch.head[slot]; r != kNoRow && o < end; r = t.ch.next[r]) { out_probe[o] = (uint32_t)i; out_build[o] = r; o++; any = true; }
      }
    }
    if (left_join && !any && o < end) { out_probe[o] = (uint32_t)i; out_build[o] = kNoRow; }
  }
}

// ------------------------------------------------------------------------------------------------------------- host driver ---
// join_indices / join_indices_wide behind their input checks (the contract: join.hpp).  `p` is the route's policy object; it owns the slot storage until the driver returns.
template <class P>
void join_indices_driver(P& p, int how, const typename P::HostKeys& left, const typename P::HostKeys& right, ColumnPtr& left_idx, ColumnPtr& right_idx, std::string* desc,
                         bool* dup_build_keys, int64_t* unmatched_build, bool exchanged = false) {
  // a right join is the left join with the sides exchanged: the left input is the build side, left_idx the nullable index (`exchanged` is set by this call alone, never by a caller: the side names in *desc are swapped back)
  if (how == PLX_JOIN_RIGHT) return join_indices_driver(p, PLX_JOIN_LEFT, right, left, right_idx, left_idx, desc, dup_build_keys, unmatched_build, true);
  if (dup_build_keys) *dup_build_keys = false;
  if (unmatched_build) *unmatched_build = 0;
  PLX_REQUIRE(how == PLX_JOIN_INNER || how == PLX_JOIN_LEFT || how == PLX_JOIN_SEMI || how == PLX_JOIN_ANTI || how == PLX_JOIN_FULL, PLX_ERR_UNSUPPORTED, "join type outside the hot path");
  const int64_t nl = P::rows(left), nr = P::rows(right);
  PLX_REQUIRE(nl < 0xffffffffll && nr < 0xffffffffll, PLX_ERR_UNSUPPORTED, "join side exceeds u32 IdxSize");
  const bool left_join = how == PLX_JOIN_LEFT;
  const bool full = how == PLX_JOIN_FULL;
  const bool semi_anti = how == PLX_JOIN_SEMI || how == PLX_JOIN_ANTI;
  // det_hash_prone_order (hash_join/mod.rs:41-50): build on the shorter relation (inner and full joins); left / semi / anti joins build on the right
  const bool swapped = !left_join && !semi_anti && !(nl > nr);
  const typename P::HostKeys& probe = swapped ? right : left;
  const typename P::HostKeys& build = swapped ? left : right;
  const int64_t np = P::rows(probe), nb = P::rows(build);
  const int log2_cap = std::max(4, ceil_log2((uint64_t)std::max<int64_t>(nb, 1) * 2));
  const uint64_t cap = 1ull << log2_cap;
  Buf head = dev_alloc(sizeof(uint32_t) * (cap + P::kSlotsBeyondCap));
  Buf next = dev_alloc(sizeof(uint32_t) * (size_t)std::max<int64_t>(nb, 1));
  Buf flags = dev_alloc_zero(16);
  PLX_HIP(hipMemsetAsync(head->ptr, 0xff, sizeof(uint32_t) * (cap + P::kSlotsBeyondCap), stream()));
  p.prepare(probe, build, Chains{head->as<unsigned int>(), next->as<unsigned int>(), flags->as<unsigned int>(), (uint32_t)log2_cap});
  if (nb) {
    ProfileScope ps(P::kBuildScope, (uint64_t)nb * (p.key_bytes + P::kBuildSlotBytes), (uint64_t)nb);
    p.launch_build(k::grid_for(nb, k::kBlock * 2));
    PLX_HIP(hipGetLastError());
  }
  Buf counts = dev_alloc(sizeof(uint32_t) * (size_t)std::max<int64_t>(np, 1));
  Buf offsets = dev_alloc(sizeof(uint64_t) * (size_t)(np + 1));
  Buf matched = full ? dev_alloc_zero((size_t)std::max<int64_t>(nb, 1)) : nullptr;               // full join: one byte per build row, set by the count pass
  if (np) {
    ProfileScope ps(P::kCountScope, (uint64_t)np * (p.key_bytes + P::kCountSlotBytes), (uint64_t)np);
    p.launch_count(k::grid_for(np, k::kBlock * 2), how, counts->as<uint32_t>(), full ? matched->as<uint8_t>() : nullptr);
    PLX_HIP(hipGetLastError());
  }
  k::exclusive_scan_u32(counts->as<uint32_t>(), offsets->as<uint64_t>(), np);
  uint64_t total = 0;
  d2h_sync(&total, offsets->as<uint64_t>() + np, 8);
  // full join: the unflagged build rows, known before the pair list is allocated
  int64_t tail = 0;
  Buf tail_rows = full ? unmatched_build_rows(matched->as<uint8_t>(), nb, &tail) : nullptr;
  PLX_REQUIRE(!(full || P::kRefuseLargeOutputAlways) || total + (uint64_t)tail < 0xffffffffull, PLX_ERR_UNSUPPORTED, "join output exceeds u32 IdxSize");
  if (unmatched_build) *unmatched_build = tail;
  const std::string sides = " rows=" + std::to_string(nb) + " cap=2^" + std::to_string(log2_cap);
  if (semi_anti) {
    ColumnPtr kept = make_idx_column((int64_t)total);
    if (total) {
      ProfileScope ps("join_emit_kept", (uint64_t)np * 12 + total * 4, (uint64_t)np);
      emit_kept_rows(counts->as<uint32_t>(), offsets->as<uint64_t>(), np, kept->values->as<uint32_t>());
    }
    if (desc) *desc = std::string(P::kPlanPrefix) + (how == PLX_JOIN_SEMI ? "hash_semi_join[" : "hash_anti_join[") + p.plan_lead() + "build=right" + sides + ", probe rows=" + std::to_string(np) +
                      ", kept=" + std::to_string(total) + "]";
    left_idx = kept; right_idx = nullptr;
    return;
  }
  ColumnPtr pidx = make_idx_column((int64_t)total + tail), bidx = make_idx_column((int64_t)total + tail);
  if (total) {
    ProfileScope ps(P::kEmitScope, (uint64_t)np * (p.key_bytes + P::kEmitSlotBytes) + total * 8, (uint64_t)np);
    p.launch_emit(k::grid_for(np, k::kBlock * 2), (left_join || full) ? 1 : 0, offsets->as<uint64_t>(), pidx->values->as<uint32_t>(), bidx->values->as<uint32_t>());
    PLX_HIP(hipGetLastError());
  }
  if (full) append_unmatched(tail_rows, tail, (int64_t)total, pidx, bidx);
  // unmatched rows carry the kNoRow sentinel -> validity bitmap
  if (left_join || full) null_out_no_row(bidx);
  if (full) null_out_no_row(pidx);
  if (desc || dup_build_keys) {                                // (the flag costs a sync: read only when someone asks)
    uint32_t f = 0; d2h_sync(&f, flags->ptr, 4);
    if (dup_build_keys) *dup_build_keys = f != 0;
    if (desc) *desc = std::string(P::kPlanPrefix) + (full ? "hash_full_join[" : "hash_join[") + p.plan_lead() + "build=" + (swapped != exchanged ? "left" : "right") + sides +
                      (f ? " dup-keys" : " unique-keys") + ", probe rows=" + std::to_string(np) + ", pairs=" + std::to_string(total) +
                      (full ? ", unmatched build rows=" + std::to_string(tail) : std::string()) + "]";
  }
  if (!swapped) { left_idx = pidx; right_idx = bidx; }
  else { left_idx = bidx; right_idx = pidx; }
}

}  // namespace join
}  // namespace plx
