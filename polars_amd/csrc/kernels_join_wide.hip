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
// Right and full joins as in kernels_join.hip: a right join is the left join with the sides exchanged; a full join's count pass (its own kernel, so that the other
// kinds do not pay for the store) flags the build rows it walks over, the unflagged ones are compacted in row order and appended as (kNoRow, row).
#include "dev.hpp"
#include "fused_sinks.hpp"
#include "join.hpp"
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
  unsigned int* head;                    // [cap]
  unsigned int* next;                    // [build rows]
  unsigned int* flags;                   // [0] = a chain longer than 1 exists (build keys not unique)
  uint32_t log2_cap;
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
// hash of row i's key words; false when a key part is null
__device__ __forceinline__ bool wide_hash(const WideKeys& ks, int64_t i, uint64_t* hash) {
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
__device__ __forceinline__ bool wide_rows_equal(const WideKeys& a, int64_t i, const WideKeys& b, int64_t r) {
  bool eq = true;
  for (int j = 0; j < a.n_cols; j++) eq = eq && load_key(wide_col(a, j), i) == load_key(wide_col(b, j), r);
  return eq;
}
__device__ __forceinline__ unsigned long long wide_ld(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the slot of build row i's key, claimed for it when the key is new; -1 only if the table were full (cap >= 2 * build rows: never)
__device__ __forceinline__ int64_t wide_find_or_claim(const WideTable& t, const WideKeys& build, int64_t i, uint64_t hash) {
  const uint64_t cap = 1ull << t.log2_cap;
  const uint32_t tag = (uint32_t)hash & t.tag_mask;
  const unsigned long long mine = ((unsigned long long)tag << 32) | (unsigned long long)(uint32_t)i;
  uint64_t slot = hash >> (64 - t.log2_cap);
  for (uint64_t step = 0; step < cap; step++) {
    unsigned long long cur = wide_ld(&t.entries[slot]);
    if (cur == kEmpty) {
      cur = atomicCAS(&t.entries[slot], (unsigned long long)kEmpty, mine);
      if (cur == kEmpty) return (int64_t)slot;               // row i is the key's representative
    }
    if ((uint32_t)(cur >> 32) == tag && wide_rows_equal(build, i, build, (int64_t)(uint32_t)cur)) return (int64_t)slot;
    slot = (slot + 1) & (cap - 1);
  }
  return -1;
}
__device__ __forceinline__ int64_t wide_find(const WideTable& t, const WideKeys& probe, int64_t i, const WideKeys& build, uint64_t hash) {
  const uint64_t cap = 1ull << t.log2_cap;
  const uint32_t tag = (uint32_t)hash & t.tag_mask;
  uint64_t slot = hash >> (64 - t.log2_cap);
  for (uint64_t step = 0; step < cap; step++) {
    const unsigned long long cur = t.entries[slot];
    if (cur == kEmpty) return -1;
    if ((uint32_t)(cur >> 32) == tag && wide_rows_equal(probe, i, build, (int64_t)(uint32_t)cur)) return (int64_t)slot;
    slot = (slot + 1) & (cap - 1);
  }
  return -1;
}

__global__ __launch_bounds__(kBlock) void join_wide_build_kernel(WideKeys build, WideTable t) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < build.n; i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t h;
    const int64_t slot = wide_hash(build, i, &h) ? wide_find_or_claim(t, build, i, h) : -1;
    if (slot < 0) { t.next[i] = kNoRow; continue; }
    const unsigned int old = atomicExch(&t.head[slot], (unsigned int)i);
    t.next[i] = old;
    if (old != kNoRow) t.flags[0] = 1u;
  }
}

// counts[i] = pairs of probe row i; the `how` rules of join_count_kernel (kernels_join.hip).  kFlag (full join): matched[r] = 1 for every build row on the chain.
template <bool kFlag>
__device__ __forceinline__ void join_wide_count_rows(const WideKeys& probe, const WideKeys& build, const WideTable& t, int how, uint32_t* __restrict__ counts, uint8_t* __restrict__ matched) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < probe.n; i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t c = 0;
    uint64_t h;
    if (wide_hash(probe, i, &h)) {
      const int64_t slot = wide_find(t, probe, i, build, h);
      if (slot >= 0) { for (unsigned int r = t.head[slot]; r != kNoRow; r = t.next[r]) { c++; if constexpr (kFlag) matched[r] = 1; } }
    }
    counts[i] = how == 2 ? (c ? 1u : 0u) : how == 3 ? (c ? 0u : 1u) : (how == 1 && c == 0) ? 1u : c;
  }
}
__global__ __launch_bounds__(kBlock) void join_wide_count_kernel(WideKeys probe, WideKeys build, WideTable t, int how, uint32_t* __restrict__ counts) {
  join_wide_count_rows<false>(probe, build, t, how, counts, nullptr);
}
__global__ __launch_bounds__(kBlock) void join_wide_full_count_kernel(WideKeys probe, WideKeys build, WideTable t, uint32_t* __restrict__ counts, uint8_t* __restrict__ matched) {
  join_wide_count_rows<true>(probe, build, t, 1, counts, matched);
}

__global__ __launch_bounds__(kBlock) void join_wide_emit_kernel(WideKeys probe, WideKeys build, WideTable t, int left_join, const uint64_t* __restrict__ offsets,
                                                                uint32_t* __restrict__ out_probe, uint32_t* __restrict__ out_build) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < probe.n; i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t o = offsets[i];
    const uint64_t end = offsets[i + 1];
    bool any = false;
    uint64_t h;
    if (o < end && wide_hash(probe, i, &h)) {
      const int64_t slot = wide_find(t, probe, i, build, h);
      if (slot >= 0) {
        for (unsigned int r = t.head[slot]; r != kNoRow && o < end; r = t.next[r]) { out_probe[o] = (uint32_t)i; out_build[o] = r; o++; any = true; }
      }
    }
    if (left_join && !any && o < end) { out_probe[o] = (uint32_t)i; out_build[o] = kNoRow; }
  }
}

static int wide_tag_bits() { const char* e = getenv("PLX_JOIN_WIDE_TAG_BITS"); const int v = e && e[0] ? atoi(e) : 32; return v >= 0 && v <= 32 ? v : 32; }   // (read at every call: the tests switch it)

static void join_indices_wide_sides(int how, bool exchanged, const std::vector<ColumnPtr>& left_keys, const std::vector<ColumnPtr>& right_keys, ColumnPtr& left_idx, ColumnPtr& right_idx,
                                    std::string* desc, bool* dup_build_keys, int64_t* unmatched_build);
void join_indices_wide(int how, const std::vector<ColumnPtr>& left_keys, const std::vector<ColumnPtr>& right_keys, ColumnPtr& left_idx, ColumnPtr& right_idx, std::string* desc,
                       bool* dup_build_keys, int64_t* unmatched_build) {
  // a right join is the left join with the sides exchanged: the left input is the build side, left_idx the nullable index
  if (how == PLX_JOIN_RIGHT) join_indices_wide_sides(PLX_JOIN_LEFT, true, right_keys, left_keys, right_idx, left_idx, desc, dup_build_keys, unmatched_build);
  else join_indices_wide_sides(how, false, left_keys, right_keys, left_idx, right_idx, desc, dup_build_keys, unmatched_build);
}
// `exchanged`: the caller swapped the inputs (right join), so the side names in *desc are swapped back
static void join_indices_wide_sides(int how, bool exchanged, const std::vector<ColumnPtr>& left_keys, const std::vector<ColumnPtr>& right_keys, ColumnPtr& left_idx, ColumnPtr& right_idx,
                                    std::string* desc, bool* dup_build_keys, int64_t* unmatched_build) {
  if (dup_build_keys) *dup_build_keys = false;
  if (unmatched_build) *unmatched_build = 0;
  PLX_REQUIRE(left_keys.size() == right_keys.size() && left_keys.size() >= 2, PLX_ERR_INVALID, "wide-key join: 2 or more key columns per side, the same number on both");
  PLX_REQUIRE(left_keys.size() <= (size_t)kMaxWideKeyCols, PLX_ERR_UNSUPPORTED,
              "join on " + std::to_string(left_keys.size()) + " key columns: at most " + std::to_string(kMaxWideKeyCols) + " key columns are supported");
  const int nc = (int)left_keys.size();
  for (int j = 0; j < nc; j++) {
    PLX_REQUIRE(left_keys[j]->dtype == right_keys[j]->dtype, PLX_ERR_INVALID,
                std::string("join keys have different dtypes (") + dtype_name(left_keys[j]->dtype) + ", " + dtype_name(right_keys[j]->dtype) + ")");
    PLX_REQUIRE(left_keys[j]->len == left_keys[0]->len && right_keys[j]->len == right_keys[0]->len, PLX_ERR_INVALID, "join key columns of one side differ in length");
  }
  PLX_REQUIRE(how == PLX_JOIN_INNER || how == PLX_JOIN_LEFT || how == PLX_JOIN_SEMI || how == PLX_JOIN_ANTI || how == PLX_JOIN_FULL, PLX_ERR_UNSUPPORTED, "join type outside the hot path");
  const int64_t nl = left_keys[0]->len, nr = right_keys[0]->len;
  PLX_REQUIRE(nl < 0xffffffffll && nr < 0xffffffffll, PLX_ERR_UNSUPPORTED, "join side exceeds u32 IdxSize");
  const bool left_join = how == PLX_JOIN_LEFT;
  const bool full = how == PLX_JOIN_FULL;
  const bool semi_anti = how == PLX_JOIN_SEMI || how == PLX_JOIN_ANTI;
  // det_hash_prone_order, as in join_indices: left / semi / anti joins build on the right, an inner or full join on the right only when the left side is the larger one
  const bool swapped = !left_join && !semi_anti && !(nl > nr);
  const std::vector<ColumnPtr>& probe = swapped ? right_keys : left_keys;
  const std::vector<ColumnPtr>& build = swapped ? left_keys : right_keys;
  const int64_t np = probe[0]->len, nb = build[0]->len;
  const int log2_cap = std::max(4, ceil_log2((uint64_t)std::max<int64_t>(nb, 1) * 2));
  const uint64_t cap = 1ull << log2_cap;
  const int tag_bits = wide_tag_bits();

  // column descriptors of both sides: probe columns, then build columns
  uint64_t hdesc[2 * kMaxWideKeyCols * kDescWords];
  uint64_t row_bytes = 0;
  for (int s = 0; s < 2; s++)
    for (int j = 0; j < nc; j++) {
      const KeyCol kc = key_col((s ? build : probe)[j]);
      uint64_t* d = hdesc + ((size_t)s * nc + j) * kDescWords;
      d[0] = (uint64_t)reinterpret_cast<uintptr_t>(kc.values); d[1] = (uint64_t)reinterpret_cast<uintptr_t>(kc.validity); d[2] = (uint64_t)kc.dtype;
      if (s) row_bytes += dtype_width(kc.dtype) ? dtype_width(kc.dtype) : 1;
    }
  const size_t desc_bytes = sizeof(uint64_t) * (size_t)(2 * nc * kDescWords);
  Buf ddesc = dev_alloc(desc_bytes);
  h2d_async(ddesc->ptr, hdesc, desc_bytes);
  PLX_HIP(hipStreamSynchronize(stream()));                   // hdesc lives on this frame: copied before anything below can throw
  WideKeys pk{ddesc->as<uint64_t>(), nc, np}, bk{ddesc->as<uint64_t>() + (size_t)nc * kDescWords, nc, nb};

  Buf entries = dev_alloc(sizeof(uint64_t) * cap);
  Buf head = dev_alloc(sizeof(uint32_t) * cap);
  Buf next = dev_alloc(sizeof(uint32_t) * (size_t)std::max<int64_t>(nb, 1));
  Buf flags = dev_alloc_zero(16);
  PLX_HIP(hipMemsetAsync(entries->ptr, 0xff, sizeof(uint64_t) * cap, stream()));
  PLX_HIP(hipMemsetAsync(head->ptr, 0xff, sizeof(uint32_t) * cap, stream()));
  WideTable t;
  t.entries = entries->as<unsigned long long>(); t.head = head->as<unsigned int>(); t.next = next->as<unsigned int>(); t.flags = flags->as<unsigned int>();
  t.log2_cap = (uint32_t)log2_cap; t.tag_mask = tag_bits >= 32 ? 0xffffffffu : ((1u << tag_bits) - 1u);
  if (nb) {
    ProfileScope ps("join_wide_build", (uint64_t)nb * (row_bytes + 16), (uint64_t)nb);
    hipLaunchKernelGGL(join_wide_build_kernel, dim3(k::grid_for(nb, kBlock * 2)), dim3(kBlock), 0, stream(), bk, t);
    PLX_HIP(hipGetLastError());
  }
  Buf counts = dev_alloc(sizeof(uint32_t) * (size_t)std::max<int64_t>(np, 1));
  Buf offsets = dev_alloc(sizeof(uint64_t) * (size_t)(np + 1));
  Buf matched = full ? dev_alloc_zero((size_t)std::max<int64_t>(nb, 1)) : nullptr;               // full join: one byte per build row, set by the count pass
  if (np) {
    ProfileScope ps("join_wide_probe_count", (uint64_t)np * (row_bytes + 12 + 4), (uint64_t)np);
    if (full) hipLaunchKernelGGL(join_wide_full_count_kernel, dim3(k::grid_for(np, kBlock * 2)), dim3(kBlock), 0, stream(), pk, bk, t, counts->as<uint32_t>(), matched->as<uint8_t>());
    else hipLaunchKernelGGL(join_wide_count_kernel, dim3(k::grid_for(np, kBlock * 2)), dim3(kBlock), 0, stream(), pk, bk, t, how, counts->as<uint32_t>());
    PLX_HIP(hipGetLastError());
  }
  k::exclusive_scan_u32(counts->as<uint32_t>(), offsets->as<uint64_t>(), np);
  uint64_t total = 0;
  d2h_sync(&total, offsets->as<uint64_t>() + np, 8);
  // full join: the unflagged build rows, known before the pair list is allocated
  int64_t tail = 0;
  Buf tail_rows = full ? unmatched_build_rows(matched->as<uint8_t>(), nb, &tail) : nullptr;
  PLX_REQUIRE(total + (uint64_t)tail < 0xffffffffull, PLX_ERR_UNSUPPORTED, "join output exceeds u32 IdxSize");
  if (unmatched_build) *unmatched_build = tail;
  auto mk_idx = [&](int64_t n) { auto c = std::make_shared<Column>(); c->dtype = PLX_U32; c->len = n; c->values = dev_alloc(values_bytes(PLX_U32, n)); c->null_count = 0; return c; };
  const std::string words = "words=" + std::to_string(nc);
  if (semi_anti) {
    ColumnPtr kept = mk_idx((int64_t)total);
    if (total) {
      ProfileScope ps("join_emit_kept", (uint64_t)np * 12 + total * 4, (uint64_t)np);
      emit_kept_rows(counts->as<uint32_t>(), offsets->as<uint64_t>(), np, kept->values->as<uint32_t>());
    }
    if (desc) *desc = std::string(how == PLX_JOIN_SEMI ? "wide_hash_semi_join" : "wide_hash_anti_join") + "[" + words + ", build=right rows=" + std::to_string(nb) + " cap=2^" + std::to_string(log2_cap) +
                      ", probe rows=" + std::to_string(np) + ", kept=" + std::to_string(total) + "]";
    left_idx = kept; right_idx = nullptr;
    return;
  }
  ColumnPtr pidx = mk_idx((int64_t)total + tail), bidx = mk_idx((int64_t)total + tail);
  if (total) {
    ProfileScope ps("join_wide_probe_emit", (uint64_t)np * (row_bytes + 12 + 16) + total * 8, (uint64_t)np);
    hipLaunchKernelGGL(join_wide_emit_kernel, dim3(k::grid_for(np, kBlock * 2)), dim3(kBlock), 0, stream(), pk, bk, t, (left_join || full) ? 1 : 0, offsets->as<uint64_t>(),
                       pidx->values->as<uint32_t>(), bidx->values->as<uint32_t>());
    PLX_HIP(hipGetLastError());
  }
  if (full) append_unmatched(tail_rows, tail, (int64_t)total, pidx, bidx);
  // unmatched rows carry the kNoRow sentinel -> validity bitmap
  if (left_join || full) null_out_no_row(bidx);
  if (full) null_out_no_row(pidx);
  uint32_t f = 0; d2h_sync(&f, flags->ptr, 4);
  if (dup_build_keys) *dup_build_keys = f != 0;
  if (desc) *desc = std::string(full ? "wide_hash_full_join[" : "wide_hash_join[") + words + ", build=" + (swapped != exchanged ? "left" : "right") + " rows=" + std::to_string(nb) + " cap=2^" +
                    std::to_string(log2_cap) + (f ? " dup-keys" : " unique-keys") + ", probe rows=" + std::to_string(np) + ", pairs=" + std::to_string(total) +
                    (full ? ", unmatched build rows=" + std::to_string(tail) : std::string()) + "]";
  if (!swapped) { left_idx = pidx; right_idx = bidx; }
  else { left_idx = bidx; right_idx = pidx; }
}

}  // namespace join
}  // namespace plx
