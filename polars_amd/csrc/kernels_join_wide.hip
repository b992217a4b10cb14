// kernels_join_wide.hip -- hash join on a key of 2..8 columns of any integer / Boolean / float dtype and any value range.
//
// The reference row-encodes such keys and joins on the encoded rows (crates/polars-row via polars-ops/src/frame/join/mod.rs:367-370).  Here the key columns stay
// where they are and the table holds ROW IDS, not key words:
//   entries[cap] : 64 bit = tag32 << 32 | representative build row of the key in this slot; all ones = empty (no row is 0xffffffff = kNoRow)
//   head[cap]    : newest build row of the slot's key (atomicExch);  next[build rows] : the previous head -- the chains of kernels_join.hip
// cap = 2^ceil(log2(2 * build rows)) >= 16 (load <= 0.5), 12 B per slot whatever the key width.  hash = WideAggSink::mix over the words * kRandomOdd; slot = its
// top log2_cap bits, tag = its low 32 bits.
// Insert of build row i: an empty slot is claimed with ONE 64-bit CAS (empty -> tag | i); a slot whose tag equals the row's tag is this key's slot when the key
// columns at its representative row equal the row's own words (the columns are the immutable input: ordinary loads), otherwise the walk goes to the next slot.
// There is no busy state, no publish step and no lane waiting for another: an entry is complete the moment it exists.  A walk ends after at most cap steps.
// Probe: the same walk without the claim; count -> k::exclusive_scan_u32 -> emit at the scanned offsets (pairs in probe order, a probe row's pairs in chain
// order: newest build row first).  A null in any key part makes the row's key null: it matches nothing (nulls_equal = false).
// No per-lane array of key words exists: the hash is one pass over the columns, the compare a second pass that reloads the row's own words (cache hits); the
// column descriptors are read with wave-uniform loads from a small device array (dev::uniform_ld), so nothing is indexed at run time in registers.
// This file holds the WIDE-KEY POLICY (WideKeys, WideTable, WideKey: the descriptor reads, the hash, the two walks, the descriptor upload) and the __global__ wrappers
// join_wide_build_kernel / join_wide_count_kernel / join_wide_full_count_kernel / join_wide_emit_kernel; the row loops and the host driver are join_driver.hpp.
// Right and full joins as in kernels_join.hip: a right join is the left join with the sides exchanged; a full join's count pass (its own kernel, so that the other
// kinds do not pay for the store) flags the build rows it walks over, the unflagged ones are compacted in row order and appended as (kNoRow, row).
#include "dev.hpp"
#include "fused_sinks.hpp"
#include "join.hpp"
#include "join_driver.hpp"
#include "join_keys.hpp"
#include "kernels.hpp"
#include "ops.hpp"
#include "scan.hpp"

namespace plx {
namespace join {

using namespace dev;
using k::kBlock;

constexpr int kMaxWideKeyCols = 8;
constexpr int kDescWords = 3;            // per key column: values pointer, validity pointer, dtype

struct WideKeys {
  const uint64_t* desc;                  // [n_cols][kDescWords], device memory no kernel writes
  int n_cols;
  int64_t n;                             // rows
};
struct WideTable {
  unsigned long long* entries;           // [cap]
  Chains ch;                             // head[cap]
  uint32_t tag_mask;                     // PLX_JOIN_WIDE_TAG_BITS (tests): fewer tag bits -> the word compare decides
};

__device__ __forceinline__ KeyCol wide_col(const WideKeys& ks, int j) {
  KeyCol kc;
  // the loaded integers are made GLOBAL-address-space pointers first: a pointer made from a plain integer is generic to the compiler and every access through it a flat instruction
  kc.values = (const void*)(const __attribute__((address_space(1))) char*)uniform_ld(ks.desc, (uint64_t)j * kDescWords);
  kc.validity = (const uint64_t*)(const __attribute__((address_space(1))) uint64_t*)uniform_ld(ks.desc, (uint64_t)j * kDescWords + 1);
  kc.dtype = (int)uniform_ld(ks.desc, (uint64_t)j * kDescWords + 2);
  kc.n = ks.n;
  return kc;
}
__device__ __forceinline__ bool wide_rows_equal(const WideKeys& a, int64_t i, const WideKeys& b, int64_t r) {
  bool eq = true;
  for (int j = 0; j < a.n_cols; j++) eq = eq && load_key(wide_col(a, j), i) == load_key(wide_col(b, j), r);
  return eq;
}
__device__ __forceinline__ unsigned long long wide_ld(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

static int wide_tag_bits() { const char* e = getenv("PLX_JOIN_WIDE_TAG_BITS"); const int v = e && e[0] ? atoi(e) : 32; return v >= 0 && v <= 32 ? v : 32; }   // (read at every call: the tests switch it)

// The wide-key policy of join_driver.hpp.  The all-ones key takes no special path: the entries hold row ids, and no row is kNoRow.
struct WideKey {
  using Keys = WideKeys;
  using Table = WideTable;
  // hash of row i's key words; false when a key part is null
  static __device__ __forceinline__ bool hash_row(const WideKeys& ks, int64_t i, uint64_t* hash) {
    uint64_t h = 0x9e3779b97f4a7c15ull;
    bool valid = true;
    for (int j = 0; j < ks.n_cols; j++) {
      const KeyCol kc = wide_col(ks, j);
      valid = valid && key_valid(kc, i);
      h = k::WideAggSink::mix(h, load_key(kc, i));
    }
    *hash = h * kRandomOdd;
    return valid;
  }
  // the slot of row i's key or -1; kClaim (build side, `keys` = `build`): an empty slot is claimed for row i, which becomes the key's representative.  A walk ends after at
  // most cap steps (cap >= 2 * build rows: a claim never fails)
  template <bool kClaim>
  static __device__ __forceinline__ int64_t walk(const WideTable& t, const WideKeys& keys, int64_t i, const WideKeys& build, uint64_t hash) {
    const uint64_t cap = 1ull << t.ch.log2_cap;
    const uint32_t tag = (uint32_t)hash & t.tag_mask;
    uint64_t slot = hash >> (64 - t.ch.log2_cap);
    for (uint64_t step = 0; step < cap; step++) {
      unsigned long long cur = kClaim ? wide_ld(&t.entries[slot]) : t.entries[slot];
      if (cur == kEmpty) {
        if constexpr (!kClaim) return -1;
        cur = atomicCAS(&t.entries[slot], (unsigned long long)kEmpty, ((unsigned long long)tag << 32) | (unsigned long long)(uint32_t)i);
        if (cur == kEmpty) return (int64_t)slot;
      }
      if ((uint32_t)(cur >> 32) == tag && wide_rows_equal(keys, i, build, (int64_t)(uint32_t)cur)) return (int64_t)slot;
      slot = (slot + 1) & (cap - 1);
    }
    return -1;
  }
  static __device__ __forceinline__ int64_t find_or_claim(const WideTable& t, const WideKeys& build, int64_t i, uint64_t hash) { return walk<true>(t, build, i, build, hash); }
  static __device__ __forceinline__ int64_t find(const WideTable& t, const WideKeys& probe, int64_t i, const WideKeys& build, uint64_t hash) { return walk<false>(t, probe, i, build, hash); }

  // host side
  using HostKeys = std::vector<ColumnPtr>;
  static int64_t rows(const std::vector<ColumnPtr>& ks) { return ks[0]->len; }
  static constexpr uint64_t kSlotsBeyondCap = 0;
  static constexpr bool kRefuseLargeOutputAlways = true;      // a pair list beyond the u32 IdxSize is refused for every kind (the single-key route: full joins only)
  static constexpr const char* kPlanPrefix = "wide_";
  static constexpr const char *kBuildScope = "join_wide_build", *kCountScope = "join_wide_probe_count", *kEmitScope = "join_wide_probe_emit";
  // declared bytes per row next to the key words: 12 B per slot touched (entry + head), the chain link / the count / the two offsets
  static constexpr uint64_t kBuildSlotBytes = 16, kCountSlotBytes = 12 + 4, kEmitSlotBytes = 12 + 16;
  std::string plan_lead() const { return "words=" + std::to_string(probe.n_cols) + (why.empty() ? "" : " (" + why + ")") + ", "; }
  std::string why;                       // why the key did not pack (the caller's words; may be empty)
  uint64_t key_bytes = 0;
  Buf ddesc, entries;
  WideKeys probe, build;
  WideTable table;
  void prepare(const std::vector<ColumnPtr>& probe_keys, const std::vector<ColumnPtr>& build_keys, const Chains& ch) {
    const int nc = (int)probe_keys.size();
    // column descriptors of both sides: probe columns, then build columns
    uint64_t hdesc[2 * kMaxWideKeyCols * kDescWords];
    for (int s = 0; s < 2; s++)
      for (int j = 0; j < nc; j++) {
        const KeyCol kc = key_col((s ? build_keys : probe_keys)[j]);
        uint64_t* d = hdesc + ((size_t)s * nc + j) * kDescWords;
        d[0] = (uint64_t)reinterpret_cast<uintptr_t>(kc.values); d[1] = (uint64_t)reinterpret_cast<uintptr_t>(kc.validity); d[2] = (uint64_t)kc.dtype;
        if (s) key_bytes += dtype_width(kc.dtype) ? dtype_width(kc.dtype) : 1;
      }
    const size_t desc_bytes = sizeof(uint64_t) * (size_t)(2 * nc * kDescWords);
    ddesc = dev_alloc(desc_bytes);
    h2d_async(ddesc->ptr, hdesc, desc_bytes);
    PLX_HIP(hipStreamSynchronize(stream()));                   // hdesc lives on this frame: copied before anything below can throw
    probe = WideKeys{ddesc->as<uint64_t>(), nc, probe_keys[0]->len};
    build = WideKeys{ddesc->as<uint64_t>() + (size_t)nc * kDescWords, nc, build_keys[0]->len};
    const uint64_t cap = 1ull << ch.log2_cap;
    entries = dev_alloc(sizeof(uint64_t) * cap);
    PLX_HIP(hipMemsetAsync(entries->ptr, 0xff, sizeof(uint64_t) * cap, stream()));
    const int tag_bits = wide_tag_bits();
    table.entries = entries->as<unsigned long long>(); table.ch = ch; table.tag_mask = tag_bits >= 32 ? 0xffffffffu : ((1u << tag_bits) - 1u);
  }
  void launch_build(int grid);
  void launch_count(int grid, int how, uint32_t* counts, uint8_t* matched);
  void launch_emit(int grid, int left_join, const uint64_t* offsets, uint32_t* out_probe, uint32_t* out_build);
};

__global__ __launch_bounds__(kBlock) void join_wide_build_kernel(WideKeys build, WideTable t) { join_build_rows<WideKey>(build, t); }
__global__ __launch_bounds__(kBlock) void join_wide_count_kernel(WideKeys probe, WideKeys build, WideTable t, int how, uint32_t* __restrict__ counts) {
  join_count_rows<WideKey, false>(probe, build, t, how, counts, nullptr);
}
__global__ __launch_bounds__(kBlock) void join_wide_full_count_kernel(WideKeys probe, WideKeys build, WideTable t, uint32_t* __restrict__ counts, uint8_t* __restrict__ matched) {
  join_count_rows<WideKey, true>(probe, build, t, 1, counts, matched);
}
__global__ __launch_bounds__(kBlock) void join_wide_emit_kernel(WideKeys probe, WideKeys build, WideTable t, int left_join, const uint64_t* __restrict__ offsets,
                                                                uint32_t* __restrict__ out_probe, uint32_t* __restrict__ out_build) {
  join_emit_rows<WideKey>(probe, build, t, left_join, offsets, out_probe, out_build);
}
void WideKey::launch_build(int grid) { hipLaunchKernelGGL(join_wide_build_kernel, dim3(grid), dim3(kBlock), 0, stream(), build, table); }
void WideKey::launch_count(int grid, int how, uint32_t* counts, uint8_t* matched) {
  if (matched) hipLaunchKernelGGL(join_wide_full_count_kernel, dim3(grid), dim3(kBlock), 0, stream(), probe, build, table, counts, matched);
  else hipLaunchKernelGGL(join_wide_count_kernel, dim3(grid), dim3(kBlock), 0, stream(), probe, build, table, how, counts);
}
void WideKey::launch_emit(int grid, int left_join, const uint64_t* offsets, uint32_t* out_probe, uint32_t* out_build) {
  hipLaunchKernelGGL(join_wide_emit_kernel, dim3(grid), dim3(kBlock), 0, stream(), probe, build, table, left_join, offsets, out_probe, out_build);
}

void join_indices_wide(int how, const std::vector<ColumnPtr>& left_keys, const std::vector<ColumnPtr>& right_keys, ColumnPtr& left_idx, ColumnPtr& right_idx, std::string* desc,
                       bool* dup_build_keys, int64_t* unmatched_build, const std::string& why) {
  PLX_REQUIRE(left_keys.size() == right_keys.size() && left_keys.size() >= 2, PLX_ERR_INVALID, "wide-key join: 2 or more key columns per side, the same number on both");
  PLX_REQUIRE(left_keys.size() <= (size_t)kMaxWideKeyCols, PLX_ERR_UNSUPPORTED,
              "join on " + std::to_string(left_keys.size()) + " key columns: at most " + std::to_string(kMaxWideKeyCols) + " key columns are supported");
  for (size_t j = 0; j < left_keys.size(); j++) {
    PLX_REQUIRE(left_keys[j]->dtype == right_keys[j]->dtype, PLX_ERR_INVALID,
                std::string("join keys have different dtypes (") + dtype_name(left_keys[j]->dtype) + ", " + dtype_name(right_keys[j]->dtype) + ")");
    PLX_REQUIRE(left_keys[j]->len == left_keys[0]->len && right_keys[j]->len == right_keys[0]->len, PLX_ERR_INVALID, "join key columns of one side differ in length");
  }
  WideKey p;
  p.why = why;
  join_indices_driver(p, how, left_keys, right_keys, left_idx, right_idx, desc, dup_build_keys, unmatched_build);
}

}  // namespace join
}  // namespace plx
