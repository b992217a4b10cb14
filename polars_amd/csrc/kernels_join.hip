// kernels_join.hip -- hash join build / probe / emit and key-hash partitioning.
//
// Reference algorithm (restated, not ported): build_tables makes 3 passes and one
// hashbrown map per partition (polars-ops/src/frame/join/hash_join/single_keys.rs:16-167);
// probe_inner looks every probe key up and emits (idx_a, idx_b) per build duplicate
// (single_keys_inner.rs:11-38).  GPU shape:
//   build  : one open-addressing table in HBM (keys[cap] claimed with 64-bit CAS, slot =
//            top bits of key * RANDOM_ODD like DirtyHash); duplicates form a chain:
//            head[slot] = newest row (atomicExch), next[row] = previous head.
//   probe 1: per probe row, find the slot and count the chain -> counts[i]
//   scan   : device exclusive scan -> output offsets (kernels_scan.hip)
//   probe 2: walk the chain again and write the pairs at offsets[i] (coalesced per row run)
// Keys are read in their physical dtype and widened in registers (no materialised
// 64-bit key copy); floats are canonicalised (-0 -> +0, one NaN: total_ord.rs:40-48).
// Null keys never match (nulls_equal = false).
// This file holds the SINGLE-KEY POLICY (Table, SingleKey: the key-word table and its two walks) and the __global__ wrappers join_build_kernel / join_count_kernel /
// join_full_count_kernel / join_emit_kernel; the row loops they wrap and the host driver behind join_indices are join_driver.hpp, shared with kernels_join_wide.hip.
// The helpers both routes call (index columns, kNoRow -> validity, the kept rows of semi / anti joins, a full join's unmatched tail) are here too.
// Right join: the left join with the sides exchanged (the left input is the build side, left_idx the nullable index).  Full join: the probe side is joined as a
// left join; the count pass also flags every build row it walks over (one byte per row, plain stores of the constant 1), the unflagged rows -- null keys were
// never inserted, so they stay unflagged -- are ballotted into selection words and compacted in row order (kernels_filter.hip), and (kNoRow, row) is appended for
// them behind the left-join pairs.  The reference tree is not at hand for these two kinds: their contract (include/polars_amd.h) is the maintainers' reading of
// polars >= 1.0 and is what the tests pin.
#include "dev.hpp"
#include "fused.hpp"
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

// The single-key policy of join_driver.hpp (a key packed from several columns is one Int64 column here).  The table holds the key words and the row's "hash" is the key word
// itself, so the `build` column is not read on the probe side (the single-key kernels have no such argument: their wrappers pass the probe column).
struct Table {
  unsigned long long* keys;  // [cap + 1]; slot cap = the key whose bits equal kEmpty
  Chains ch;                 // head[cap + 1]
};
struct SingleKey {
  using Keys = KeyCol;
  using Table = join::Table;
  static __device__ __forceinline__ bool hash_row(const KeyCol& kc, int64_t i, uint64_t* key) {
    if (!key_valid(kc, i)) return false;
    *key = load_key(kc, i);
    return true;
  }
  // the walk both sides make; kClaim (build side): an empty slot is claimed for the key with one 64-bit CAS
  template <bool kClaim>
  static __device__ __forceinline__ int64_t walk(const Table& t, uint64_t key) {
    const uint64_t cap = 1ull << t.ch.log2_cap;
    if (key == kEmpty) return (int64_t)cap;
    uint64_t slot = (key * kRandomOdd) >> (64 - t.ch.log2_cap);
    for (;;) {
      unsigned long long cur = t.keys[slot];
      if (cur == key) return (int64_t)slot;
      if (cur == kEmpty) {
        if constexpr (!kClaim) return -1;
        unsigned long long old = atomicCAS(&t.keys[slot], (unsigned long long)kEmpty, (unsigned long long)key);
        if (old == kEmpty || old == key) return (int64_t)slot;
      }
      slot = (slot + 1) & (cap - 1);
    }
  }
  static __device__ __forceinline__ int64_t find_or_claim(const Table& t, const KeyCol&, int64_t, uint64_t key) { return walk<true>(t, key); }
  static __device__ __forceinline__ int64_t find(const Table& t, const KeyCol&, int64_t, const KeyCol&, uint64_t key) { return walk<false>(t, key); }

  // host side
  using HostKeys = ColumnPtr;
  static int64_t rows(const ColumnPtr& c) { return c->len; }
  static constexpr uint64_t kSlotsBeyondCap = 1;
  // a pair list beyond the u32 IdxSize is refused for full joins only (their tail is appended at a u32-checked place); an inner join with more pairs runs, as it always has
  static constexpr bool kRefuseLargeOutputAlways = false;
  static constexpr const char* kPlanPrefix = "";
  static constexpr const char *kBuildScope = "join_build", *kCountScope = "join_probe_count", *kEmitScope = "join_probe_emit";
  static constexpr uint64_t kBuildSlotBytes = 0, kCountSlotBytes = 4, kEmitSlotBytes = 8;       // declared bytes per row next to the key: the count / the two offsets
  std::string plan_lead() const { return std::string(); }
  uint64_t key_bytes = 0;
  Buf keys;
  KeyCol probe, build;
  Table table;
  void prepare(const ColumnPtr& probe_key, const ColumnPtr& build_key, const Chains& ch) {
    const uint64_t slots = (1ull << ch.log2_cap) + kSlotsBeyondCap;
    keys = dev_alloc(sizeof(uint64_t) * slots);
    PLX_HIP(hipMemsetAsync(keys->ptr, 0xff, sizeof(uint64_t) * slots, stream()));
    table.keys = keys->as<unsigned long long>(); table.ch = ch;
    probe = key_col(probe_key); build = key_col(build_key);
    key_bytes = dtype_width(build_key->dtype) ? dtype_width(build_key->dtype) : 1;
  }
  void launch_build(int grid);
  void launch_count(int grid, int how, uint32_t* counts, uint8_t* matched);
  void launch_emit(int grid, int left_join, const uint64_t* offsets, uint32_t* out_probe, uint32_t* out_build);
};

__global__ __launch_bounds__(kBlock) void join_build_kernel(KeyCol build, Table t) { join_build_rows<SingleKey>(build, t); }
__global__ __launch_bounds__(kBlock) void join_count_kernel(KeyCol probe, Table t, int how, uint32_t* __restrict__ counts) { join_count_rows<SingleKey, false>(probe, probe, t, how, counts, nullptr); }
__global__ __launch_bounds__(kBlock) void join_full_count_kernel(KeyCol probe, Table t, uint32_t* __restrict__ counts, uint8_t* __restrict__ matched) {
  join_count_rows<SingleKey, true>(probe, probe, t, 1, counts, matched);
}
__global__ __launch_bounds__(kBlock) void join_emit_kernel(KeyCol probe, Table t, int left_join, const uint64_t* __restrict__ offsets, uint32_t* __restrict__ out_probe,
                                                           uint32_t* __restrict__ out_build) {
  join_emit_rows<SingleKey>(probe, probe, t, left_join, offsets, out_probe, out_build);
}
void SingleKey::launch_build(int grid) { hipLaunchKernelGGL(join_build_kernel, dim3(grid), dim3(kBlock), 0, stream(), build, table); }
void SingleKey::launch_count(int grid, int how, uint32_t* counts, uint8_t* matched) {
  if (matched) hipLaunchKernelGGL(join_full_count_kernel, dim3(grid), dim3(kBlock), 0, stream(), probe, table, counts, matched);
  else hipLaunchKernelGGL(join_count_kernel, dim3(grid), dim3(kBlock), 0, stream(), probe, table, how, counts);
}
void SingleKey::launch_emit(int grid, int left_join, const uint64_t* offsets, uint32_t* out_probe, uint32_t* out_build) {
  hipLaunchKernelGGL(join_emit_kernel, dim3(grid), dim3(kBlock), 0, stream(), probe, table, left_join, offsets, out_probe, out_build);
}

// full join, after the count pass: bit i of mask = build row i was flagged by no probe row (one ballot per 64 rows; the pad bits of the last word are cleared)
__global__ __launch_bounds__(kBlock) void join_unmatched_mask_kernel(const uint8_t* __restrict__ matched, int64_t n, unsigned long long* __restrict__ mask) {
  const int lane = lane_id();
  const int64_t nwords = (n + 63) >> 6;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t w = wave; w < nwords; w += nwaves) {
    const int64_t i = w * 64 + lane;
    const uint64_t m = ballot(i < n && matched[i] == 0);
    if (lane == 0) mask[w] = m;
  }
}
// ... and behind the left-join pairs: (kNoRow, unmatched build row), in build row order
__global__ __launch_bounds__(kBlock) void join_append_unmatched_kernel(const uint32_t* __restrict__ rows, int64_t n, uint32_t* __restrict__ out_probe, uint32_t* __restrict__ out_build) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) { out_probe[i] = kNoRow; out_build[i] = rows[i]; }
}

// semi / anti: the kept probe rows, in probe order (single_keys_semi_anti.rs keeps left order the same way)
__global__ __launch_bounds__(kBlock) void join_emit_kept_kernel(const uint32_t* __restrict__ counts, const uint64_t* __restrict__ offsets, int64_t n, uint32_t* __restrict__ out_probe) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    if (counts[i]) out_probe[offsets[i]] = (uint32_t)i;
}

void emit_kept_rows(const uint32_t* counts, const uint64_t* offsets, int64_t n, uint32_t* out_probe) {
  hipLaunchKernelGGL(join_emit_kept_kernel, dim3(k::grid_for(n, kBlock * 2)), dim3(kBlock), 0, stream(), counts, offsets, n, out_probe);
  PLX_HIP(hipGetLastError());
}

ColumnPtr make_idx_column(int64_t n, int64_t min_alloc_rows) {
  auto c = std::make_shared<Column>();
  c->dtype = PLX_U32; c->len = n; c->values = dev_alloc(values_bytes(PLX_U32, std::max(n, min_alloc_rows))); c->null_count = 0;
  return c;
}
void null_out_no_row(ColumnPtr& idx) {
  if (!idx->len) return;
  plx_scalar s; s.u = kNoRow;
  ColumnPtr ok = ops::cmp_scalar(PLX_NE, idx, s);
  drop_host_mirror(*idx);
  idx->validity = ok->values; idx->null_count = -1;
  if (column_null_count(idx) == 0) { idx->validity = nullptr; idx->null_count = 0; }
}

Buf unmatched_build_rows(const uint8_t* matched, int64_t nb, int64_t* n_out) {
  *n_out = 0;
  if (nb == 0) return nullptr;
  const int64_t nwords = (nb + 63) >> 6;
  Buf mask = dev_alloc(sizeof(uint64_t) * (size_t)nwords);
  {
    ProfileScope ps("join_unmatched_mask", (uint64_t)nb + (uint64_t)nwords * 8, (uint64_t)nb);
    hipLaunchKernelGGL(join_unmatched_mask_kernel, dim3(k::grid_for(nb, kBlock * 4)), dim3(kBlock), 0, stream(), matched, nb, mask->as<unsigned long long>());
    PLX_HIP(hipGetLastError());
  }
  const k::FilterPlan fp = k::filter_prepare(mask->as<uint64_t>(), nb);
  *n_out = fp.n_out;
  Buf rows = dev_alloc(sizeof(uint32_t) * (size_t)std::max<int64_t>(fp.n_out, 1));
  k::filter_rowids(fp, rows->as<uint32_t>());
  PLX_HIP(hipStreamSynchronize(stream()));               // `mask` / the plan's offsets are read by the compaction
  return rows;
}
void append_unmatched(const Buf& rows, int64_t n, int64_t at, const ColumnPtr& probe_idx, const ColumnPtr& build_idx) {
  if (n == 0) return;
  PLX_REQUIRE(at >= 0 && at + n <= probe_idx->len && probe_idx->len == build_idx->len, PLX_ERR_SHAPE, "full join: the unmatched build rows do not fit the pair list");
  ProfileScope ps("join_append_unmatched", (uint64_t)n * 12, (uint64_t)n);
  hipLaunchKernelGGL(join_append_unmatched_kernel, dim3(k::grid_for(n, kBlock * 4)), dim3(kBlock), 0, stream(), rows->as<uint32_t>(), n, probe_idx->values->as<uint32_t>() + at,
                     build_idx->values->as<uint32_t>() + at);
  PLX_HIP(hipGetLastError());
  PLX_HIP(hipStreamSynchronize(stream()));               // `rows` is released by the caller
}

// out[i] = li[i] != kNoRow ? lkey[li[i]] : rkey[ri[i]], validity from the side that was read (the coalesced key column of a full join); one wave per 64 rows
template <class W>
__global__ __launch_bounds__(kBlock) void coalesce_key_kernel(const W* __restrict__ lkey, const uint64_t* __restrict__ lvalid, const W* __restrict__ rkey, const uint64_t* __restrict__ rvalid,
                                                              const uint32_t* __restrict__ li, const uint32_t* __restrict__ ri, int64_t n, W* __restrict__ out,
                                                              unsigned long long* __restrict__ out_validity) {
  const int lane = lane_id();
  const int64_t nwords = (n + 63) >> 6;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t w = wave; w < nwords; w += nwaves) {
    const int64_t i = w * 64 + lane;
    bool ok = false;
    if (i < n) {
      const uint32_t l = li[i];
      const bool from_left = l != kNoRow;
      const uint32_t j = from_left ? l : ri[i];
      ok = j != kNoRow;                                  // (a pair has at least one side)
      const W* src = from_left ? lkey : rkey;
      const uint64_t* val = from_left ? lvalid : rvalid;
      out[i] = ok ? src[j] : (W)0;
      if (ok && val) ok = (val[j >> 6] >> (j & 63)) & 1;
    }
    if (out_validity) { const uint64_t m = ballot(ok); if (lane == 0) out_validity[w] = m; }
  }
}
ColumnPtr coalesce_keys(const ColumnPtr& lkey, const ColumnPtr& rkey, const ColumnPtr& left_idx, const ColumnPtr& right_idx) {
  PLX_REQUIRE(lkey->dtype == rkey->dtype, PLX_ERR_INVALID, std::string("coalesced join key: the key columns have different dtypes (") + dtype_name(lkey->dtype) + ", " + dtype_name(rkey->dtype) + ")");
  const int w = lkey->dtype == PLX_BOOL ? 0 : dtype_width(lkey->dtype);
  PLX_REQUIRE(w == 1 || w == 2 || w == 4 || w == 8, PLX_ERR_UNSUPPORTED, std::string("full join with coalesce on a ") + dtype_name(lkey->dtype) + " key: keys of 1, 2, 4 or 8 bytes coalesce");
  PLX_REQUIRE(left_idx->dtype == PLX_U32 && right_idx->dtype == PLX_U32 && left_idx->len == right_idx->len, PLX_ERR_INVALID, "coalesced join key: two u32 index columns of one length");
  const int64_t n = left_idx->len;
  const bool need_valid = lkey->validity || rkey->validity;
  ColumnPtr out = make_column(lkey->dtype, n, need_valid);
  if (n == 0) return out;
  if (need_valid) out->null_count = -1;
  ProfileScope ps("join_coalesce_key", (uint64_t)n * (8 + 2 * (uint64_t)w), (uint64_t)n);
  const int grid = k::grid_for(n, kBlock * 2);
  unsigned long long* ov = need_valid ? out->validity->as<unsigned long long>() : nullptr;
#define C(W) hipLaunchKernelGGL((coalesce_key_kernel<W>), dim3(grid), dim3(kBlock), 0, stream(), (const W*)lkey->data(), lkey->valid_words(), (const W*)rkey->data(), rkey->valid_words(), \
                                left_idx->values->as<uint32_t>(), right_idx->values->as<uint32_t>(), n, (W*)out->values->ptr, ov)
  switch (w) {
    case 1: C(uint8_t); break;
    case 2: C(uint16_t); break;
    case 4: C(uint32_t); break;
    default: C(uint64_t); break;
  }
#undef C
  PLX_HIP(hipGetLastError());
  return out;
}

void join_indices(int how, const ColumnPtr& left_key, const ColumnPtr& right_key, ColumnPtr& left_idx, ColumnPtr& right_idx, std::string* desc, bool* dup_build_keys, int64_t* unmatched_build) {
  PLX_REQUIRE(left_key->dtype == right_key->dtype, PLX_ERR_INVALID,
              std::string("join keys have different dtypes (") + dtype_name(left_key->dtype) + ", " + dtype_name(right_key->dtype) + ")");
  SingleKey p;
  join_indices_driver(p, how, left_key, right_key, left_idx, right_idx, desc, dup_build_keys, unmatched_build);
}

// ------------------------------------------------ materialising join: pairs over a candidate list ---
// The frame-returning join of the reference (polars-ops/src/frame/join/mod.rs:564-652 _inner_join_from_series: pairs from hash_join/single_keys_inner.rs:40-149,
// then one gather per side) on the machinery of the fused join -> group-by: the build side is the fused::JoinAggTable its build scan fills (16-byte {key, row}
// slots; duplicate build keys: chains through links[]), the probe side arrives as a CANDIDATE list -- the rows that passed the probe side's predicate and the
// partitioned LDS filters of kernels_partition.hip (probe_hits_impl), a few per cent of the probe side for a selective build -- so the only random walk through
// HBM is one slot lookup per candidate, once: pass 1 leaves the build row (or chain head) and the pair count of every candidate, the pairs are then laid out by a
// device scan (duplicate keys / left joins) or by the selection-bitmap compaction of kernels_filter.hip (unique keys: 0 / 1 pairs per candidate) -- no second probe.
struct PairTable {
  const unsigned long long* slots; const unsigned long long* links; uint32_t log2_cap, log2_window;
  // direct-address variant (bits != null; unique build keys): bitmap over the key range + rank per word + slot -> build row (fused::DirectJoinTable, k::direct_slot_rows)
  const unsigned long long* bits; const unsigned int* rank; const unsigned int* slot_row; long long kmin; unsigned long long range;
};
__device__ __forceinline__ unsigned int pair_lookup(const PairTable& t, uint64_t key) {
  if (t.bits) {                                   // wave-uniform
    const uint64_t idx = key - (uint64_t)t.kmin;
    if (idx >= t.range) return kNoRow;
    const unsigned long long w = t.bits[idx >> 6];
    if (!((w >> (idx & 63)) & 1ull)) return kNoRow;
    return t.slot_row[(unsigned long long)t.rank[idx >> 6] + (unsigned long long)__popcll(w & ((1ull << (idx & 63)) - 1ull))];
  }
  const uint64_t cap = 1ull << t.log2_cap;
  if (key == fused::kEmptyKey) return (unsigned int)t.slots[cap * 2 + 1];                   // the key equal to the EMPTY pattern lives in slot `cap` (row kNoRow when absent)
  uint64_t slot = (key * fused::kP2HashMult) >> (64 - t.log2_cap);
  for (uint64_t n = 0; n <= cap; n++) {
    const unsigned long long cur = t.slots[slot * 2];
    if (cur == key) return (unsigned int)t.slots[slot * 2 + 1];
    if (cur == fused::kEmptyKey) return kNoRow;
    const uint64_t wmask = (1ull << (t.log2_window ? t.log2_window : t.log2_cap)) - 1ull;      // probe sequences wrap inside the table's windows (fused::jt_next)
    slot = (slot & ~wmask) | ((slot + 1) & wmask);
  }
  return kNoRow;
}
// head[i] = build row (multi-value: head of the chain) of candidate i or kNoRow; cnt[i] (may be null) = pairs it emits; mask (may be null) bit i = it has a match
__global__ __launch_bounds__(kBlock) void join_match_kernel(KeyCol probe, const uint32_t* __restrict__ cand, int64_t n, PairTable t, int left_join, uint32_t* __restrict__ head,
                                                            uint32_t* __restrict__ cnt, unsigned long long* __restrict__ mask) {
  const int lane = lane_id();
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t base = wave * 64; base < n; base += nwaves * 64) {
    const int64_t i = base + lane;
    unsigned int h = kNoRow, c = 0;
    if (i < n) {
      const int64_t row = cand ? (int64_t)cand[i] : i;
      if (key_valid(probe, row)) h = pair_lookup(t, load_key(probe, row));
      if (h != kNoRow) {
        c = 1;
        if (t.links) { unsigned int r = (unsigned int)t.links[h]; for (uint32_t g = 0; r != kNoRow && g < (1u << 24); g++) { c++; r = (unsigned int)t.links[r]; } }
      } else if (left_join) c = 1;
      head[i] = h;
      if (cnt) cnt[i] = c;
    }
    if (mask) { const uint64_t m = ballot(h != kNoRow); if (lane == 0) mask[base >> 6] = m; }
  }
}
__global__ __launch_bounds__(kBlock) void join_pairs_emit_kernel(const uint32_t* __restrict__ cand, int64_t n, const unsigned long long* __restrict__ links, const uint32_t* __restrict__ head,
                                                                 const uint64_t* __restrict__ off, uint32_t* __restrict__ out_probe, uint32_t* __restrict__ out_build) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t o = off[i];
    const uint64_t end = off[i + 1];
    if (o == end) continue;
    const uint32_t row = cand ? cand[i] : (uint32_t)i;
    unsigned int r = head[i];
    if (r == kNoRow) { out_probe[o] = row; out_build[o] = kNoRow; continue; }               // left join: no match
    for (; o < end && r != kNoRow; o++) { out_probe[o] = row; out_build[o] = r; r = links ? (unsigned int)links[r] : kNoRow; }
  }
}
__global__ __launch_bounds__(kBlock) void iota_u32_kernel(uint32_t* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = (uint32_t)i;
}

static void join_pairs_impl(int how, const ColumnPtr& probe_key, const ColumnPtr& cand, const PairTable& t, ColumnPtr& probe_idx, ColumnPtr& build_idx, std::string* desc);
void join_pairs(int how, const ColumnPtr& probe_key, const ColumnPtr& cand, const fused::JoinAggTable& jt, ColumnPtr& probe_idx, ColumnPtr& build_idx, std::string* desc) {
  PairTable t{}; t.slots = jt.slots; t.links = jt.links; t.log2_cap = jt.log2_cap; t.log2_window = jt.log2_window;
  join_pairs_impl(how, probe_key, cand, t, probe_idx, build_idx, desc);
}
void join_pairs_direct(int how, const ColumnPtr& probe_key, const ColumnPtr& cand, const fused::DirectJoinTable& dt, const uint32_t* slot_row, ColumnPtr& probe_idx, ColumnPtr& build_idx,
                       std::string* desc) {
  PairTable t{}; t.bits = dt.bits; t.rank = dt.rank; t.slot_row = slot_row; t.kmin = dt.kmin; t.range = dt.range;
  join_pairs_impl(how, probe_key, cand, t, probe_idx, build_idx, desc);
}
static void join_pairs_impl(int how, const ColumnPtr& probe_key, const ColumnPtr& cand, const PairTable& t, ColumnPtr& probe_idx, ColumnPtr& build_idx, std::string* desc) {
  PLX_REQUIRE(how == PLX_JOIN_INNER || how == PLX_JOIN_LEFT, PLX_ERR_UNSUPPORTED, "join_pairs: inner and left joins");
  PLX_REQUIRE(probe_key->len < 0xffffffffll, PLX_ERR_UNSUPPORTED, "join side exceeds u32 IdxSize");
  const bool left = how == PLX_JOIN_LEFT, multi = t.links != nullptr;
  const int64_t n = cand ? cand->len : probe_key->len;
  if (n == 0) { probe_idx = make_idx_column(0, 1); build_idx = make_idx_column(0, 1); if (desc) *desc = "join_pairs[no candidates]"; return; }
  const uint32_t* cp = cand ? cand->values->as<uint32_t>() : nullptr;
  const int kw = dtype_width(probe_key->dtype) ? dtype_width(probe_key->dtype) : 1;
  ColumnPtr head = make_idx_column(n, 1);
  const bool counted = multi;                           // unique build keys: 0 / 1 pairs per candidate (left join: exactly 1), no scan
  Buf cnt = counted ? dev_alloc(sizeof(uint32_t) * (size_t)n) : nullptr;
  const int64_t nwords = (n + 63) >> 6;
  Buf mask = (!counted && !left) ? dev_alloc(sizeof(uint64_t) * (size_t)nwords) : nullptr;
  {
    ProfileScope ps("join_match", (uint64_t)n * (kw + 16 + (cand ? 4 : 0) + 4), (uint64_t)n);
    hipLaunchKernelGGL(join_match_kernel, dim3(k::grid_for(n, kBlock * 2)), dim3(kBlock), 0, stream(), key_col(probe_key), cp, n, t, left ? 1 : 0, head->values->as<uint32_t>(),
                       cnt ? cnt->as<uint32_t>() : nullptr, mask ? mask->as<unsigned long long>() : nullptr);
    PLX_HIP(hipGetLastError());
  }
  uint64_t total = 0;
  if (!counted && left) {
    // one pair per candidate: the candidate list IS the probe index, the heads are the build index
    if (cand) probe_idx = cand;
    else { probe_idx = make_idx_column(n, 1); hipLaunchKernelGGL(iota_u32_kernel, dim3(k::grid_for(n, kBlock * 4)), dim3(kBlock), 0, stream(), probe_idx->values->as<uint32_t>(), n); PLX_HIP(hipGetLastError()); }
    build_idx = head;
    null_out_no_row(build_idx);
    total = (uint64_t)n;
  } else if (!counted) {
    const k::FilterPlan fp = k::filter_prepare(mask->as<uint64_t>(), n);
    total = (uint64_t)fp.n_out;
    probe_idx = make_idx_column(fp.n_out, 1); build_idx = make_idx_column(fp.n_out, 1);
    if (cand) k::filter_apply(fp, 4, cp, nullptr, probe_idx->values->ptr, nullptr);
    else k::filter_rowids(fp, probe_idx->values->as<uint32_t>());
    k::filter_apply(fp, 4, head->values->ptr, nullptr, build_idx->values->ptr, nullptr);
    PLX_HIP(hipStreamSynchronize(stream()));             // `mask` / the plan's offsets are read by the compactions
  } else {
    Buf off = dev_alloc(sizeof(uint64_t) * (size_t)(n + 1));
    k::exclusive_scan_u32(cnt->as<uint32_t>(), off->as<uint64_t>(), n);
    d2h_sync(&total, off->as<uint64_t>() + n, 8);
    PLX_REQUIRE(total < 0xffffffffull, PLX_ERR_UNSUPPORTED, "join output exceeds u32 IdxSize");
    probe_idx = make_idx_column((int64_t)total, 1); build_idx = make_idx_column((int64_t)total, 1);
    if (total) {
      ProfileScope ps("join_pairs_emit", (uint64_t)n * 24 + total * 8, (uint64_t)n);
      hipLaunchKernelGGL(join_pairs_emit_kernel, dim3(k::grid_for(n, kBlock * 2)), dim3(kBlock), 0, stream(), cp, n, t.links, head->values->as<uint32_t>(), off->as<uint64_t>(),
                         probe_idx->values->as<uint32_t>(), build_idx->values->as<uint32_t>());
      PLX_HIP(hipGetLastError());
    }
    if (left) null_out_no_row(build_idx);
    PLX_HIP(hipStreamSynchronize(stream()));
  }
  if (desc) *desc = std::string("join_pairs[") + (cand ? "candidates=" : "rows=") + std::to_string(n) + (multi ? ", multi-value chains" : t.bits ? ", direct-address table" : ", unique build keys") + " -> match" +
                    (counted ? "+scan+emit" : left ? "" : "+bitmap compaction") + ", pairs=" + std::to_string(total) + "]";
}

// -------------------------------------------------------------- partitioning ---
__device__ __forceinline__ uint32_t partition_of(const KeyCol& kc, int64_t i, uint64_t seed, uint32_t n_parts) {
  if (!key_valid(kc, i)) return 0;  // null_partition() == 0
  const uint64_t h = load_key(kc, i) * kRandomOdd;  // dirty_hash
  return (uint32_t)__umul64hi(h * seed, (uint64_t)n_parts);
}
// Two passes, no device atomics on the row path (a wave-aggregated bump of 8 global cursors took 32 ms for 3.2e8 rows: a few hot addresses serialise):
// every workgroup owns a contiguous slab of rows; pass 1 leaves its per-partition counts, a scan over (partition, workgroup) turns them into the start of every
// (workgroup, partition) run, pass 2 ranks its rows with LDS cursors and writes the permutation.  Rows of a partition keep their workgroup order (slabs ascend).
__global__ __launch_bounds__(kBlock) void partition_count_kernel(KeyCol kc, uint64_t seed, uint32_t n_parts, int64_t per_block, unsigned long long* __restrict__ block_counts /* [n_parts][grid] */,
                                                                 unsigned long long* __restrict__ counts) {
  extern __shared__ unsigned int lcount[];
  for (uint32_t p = threadIdx.x; p < n_parts; p += blockDim.x) lcount[p] = 0;
  __syncthreads();
  const int64_t beg = (int64_t)blockIdx.x * per_block, end = beg + per_block < kc.n ? beg + per_block : kc.n;
  for (int64_t i = beg + threadIdx.x; i < end; i += blockDim.x) atomicAdd(&lcount[partition_of(kc, i, seed, n_parts)], 1u);
  __syncthreads();
  for (uint32_t p = threadIdx.x; p < n_parts; p += blockDim.x) {
    block_counts[(size_t)p * gridDim.x + blockIdx.x] = lcount[p];
    if (lcount[p]) atomicAdd(&counts[p], (unsigned long long)lcount[p]);
  }
}
__global__ __launch_bounds__(kBlock) void partition_scatter_kernel(KeyCol kc, uint64_t seed, uint32_t n_parts, int64_t per_block, const unsigned long long* __restrict__ block_starts /* [n_parts][grid] */,
                                                                   uint32_t* __restrict__ perm) {
  extern __shared__ unsigned long long lcur[];       // [n_parts] next output position of this workgroup's run in each partition
  for (uint32_t p = threadIdx.x; p < n_parts; p += blockDim.x) lcur[p] = block_starts[(size_t)p * gridDim.x + blockIdx.x];
  __syncthreads();
  const int lane = lane_id();
  const int64_t beg = (int64_t)blockIdx.x * per_block, end = beg + per_block < kc.n ? beg + per_block : kc.n;
  for (int64_t base = beg + (threadIdx.x - lane); base < end; base += blockDim.x) {
    const int64_t i = base + lane;
    const bool active = i < end;
    const uint32_t p = active ? partition_of(kc, i, seed, n_parts) : 0xffffffffu;
    if (n_parts <= 64) {
      // few partitions: one LDS atomic per (wave, partition present), lanes take consecutive positions
      uint64_t todo = ballot(active);
      while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t lp = __shfl(p, leader, 64);
        const uint64_t same = ballot(active && p == lp);
        unsigned long long o = 0;
        if (lane == leader) o = atomicAdd(&lcur[lp], (unsigned long long)popc64(same));
        o = shfl_u64(o, leader);
        if (active && p == lp) perm[o + (uint64_t)prefix_rank(same)] = (uint32_t)i;
        todo &= ~same;
      }
    } else if (active) {
      perm[atomicAdd(&lcur[p], 1ull)] = (uint32_t)i;
    }
  }
}

void hash_partition_dev(const ColumnPtr& key, int n_partitions, uint64_t seed, ColumnPtr& perm, Buf& counts) {
  PLX_REQUIRE(n_partitions >= 1 && n_partitions <= 4096, PLX_ERR_INVALID, "hash_partition: 1..4096 partitions");
  // HashPartitioner::new seed mixing (hashing.rs:81-96)
  auto fold = [](uint64_t a, uint64_t b) { unsigned __int128 r = (unsigned __int128)a * b; return (uint64_t)r ^ (uint64_t)(r >> 64); };
  uint64_t s = fold(seed ^ 0x85921e81c41226a0ull, 0x3bc1d0faba166294ull);
  s = fold(s, 0xfbde893e21a73756ull) | 1;
  const int64_t n = key->len;
  perm = make_idx_column(n);
  counts = dev_alloc_zero(sizeof(uint64_t) * (size_t)n_partitions);
  if (n) {
    ProfileScope ps("hash_partition", (uint64_t)n * (dtype_width(key->dtype) * 2 + 4), (uint64_t)n);
    // slabs of whole waves; enough workgroups to fill the chip, few enough that the (partition x workgroup) table stays small
    const int64_t max_blocks = std::max<int64_t>(1, std::min<int64_t>(2048, ((int64_t)1 << 22) / n_partitions));
    int64_t per_block = (n + max_blocks - 1) / max_blocks;
    per_block = std::max<int64_t>(kBlock, (per_block + kBlock - 1) / kBlock * kBlock);
    const int grid = (int)((n + per_block - 1) / per_block);
    const size_t cells = (size_t)n_partitions * (size_t)grid;
    Buf block_counts = dev_alloc(sizeof(uint64_t) * (cells + 1)), block_starts = dev_alloc(sizeof(uint64_t) * (cells + 1));
    hipLaunchKernelGGL(partition_count_kernel, dim3(grid), dim3(kBlock), sizeof(unsigned int) * (size_t)n_partitions, stream(), key_col(key), s, (uint32_t)n_partitions, per_block,
                       block_counts->as<unsigned long long>(), counts->as<unsigned long long>());
    PLX_HIP(hipGetLastError());
    k::exclusive_scan_u64(block_counts->as<uint64_t>(), block_starts->as<uint64_t>(), (int64_t)cells);
    hipLaunchKernelGGL(partition_scatter_kernel, dim3(grid), dim3(kBlock), sizeof(unsigned long long) * (size_t)n_partitions, stream(), key_col(key), s, (uint32_t)n_partitions, per_block,
                       block_starts->as<unsigned long long>(), perm->values->as<uint32_t>());
    PLX_HIP(hipGetLastError());
  }
}

void hash_partition(const ColumnPtr& key, int n_partitions, uint64_t seed, ColumnPtr& perm, int64_t* counts_out) {
  Buf counts;
  hash_partition_dev(key, n_partitions, seed, perm, counts);
  std::vector<uint64_t> h((size_t)n_partitions, 0);
  if (key->len) d2h_sync(h.data(), counts->ptr, sizeof(uint64_t) * (size_t)n_partitions);
  for (int p = 0; p < n_partitions; p++) counts_out[p] = (int64_t)h[p];
}

}  // namespace join
}  // namespace plx
