// kernels_sort.hip -- stable multi-key arg-sort (LSD radix) and top-k selection (MSD radix select).
//
// Reference behaviour (restated, not ported): arg_sort_multiple compares row-encoded keys with a stable
// comparison sort on the CPU thread pool (polars-core/src/chunked_array/ops/sort/arg_sort_multiple.rs,
// arg_sort.rs); sort followed by a slice keeps only the first rows (slice_pushdown_lp.rs -> SortExec slice /
// streaming top_k.rs).  GPU shape:
//   encode : every key column is turned into an order-preserving u64 (sign flip for ints, the IEEE total-order
//            flip for floats with NaN canonicalised to the greatest value and -0 -> +0, bitwise NOT for
//            descending) read THROUGH the current permutation, so narrow dtypes are never widened in HBM twice.
//   rounds : keys are processed last to first (LSD over keys); within a key, 8-bit digits least significant
//            first.  One pass over the encoded keys builds all 8 digit histograms; digits on which every row
//            agrees are skipped (an i32-range key costs 4 passes, a dictionary code 1-3).
//   pass   : per-workgroup digit histogram -> device exclusive scan (digit-major) -> stable scatter.  The scatter
//            ranks the 256 keys of a sub-tile with wave64 ballots (8 ballots = match-any on the digit), per-wave
//            digit counts meet in LDS, so ties keep input order without any atomics.
//   nulls  : one extra 1-bit pass per nullable key (null rank is an absolute position: nulls_last is not flipped
//            by `descending`, arg_sort.rs).
//   top-k  : `limit` << n: MSD radix select on the first key finds the smallest prefix bucket that contains the
//            limit-th row; rows at or below it (ties included) are compacted in row order and only those are
//            sorted -- same result as the full stable sort followed by head(limit).
//   quantile: a whole column never sorts: the same MSD select finds the codes at two neighbouring ranks (select_ranks); a group-by sorts (keys, value) once per
//            source, finds the segment heads through the permutation and picks two values per group (segment_quantiles).  The arithmetic is quantile.hpp's.
//   distinct: n_unique of a whole column is two popcounts (Boolean), a bitmap over the value range (integers of a small range) or a key-only sort of the value
//            codes and a count of the run heads; per group it is the difference of two ranks in a mask of run heads over the quantiles' sorted segments; unique()
//            is one stable sort of the subset, the segment heads and a row-order mask (n_unique_column, segment_distinct, distinct_rows; distinct.hpp).
// Everything is HBM-streaming integer work: 12 B read + 12 B written per row and pass.
#include <algorithm>

#include "dev.hpp"
#include "distinct.hpp"
#include "kernels.hpp"
#include "ops.hpp"
#include "quantile.hpp"
#include "scan.hpp"
#include "sort.hpp"

namespace plx {
namespace sort {

using namespace dev;
using k::kBlock;

constexpr int kItems = 16;                 // sub-tiles of kBlock keys per workgroup
constexpr int kTile = kBlock * kItems;     // 4096 keys per workgroup and pass
constexpr int kWaves = kBlock / kWave;

struct KeyCol {
  const void* values;
  const uint64_t* validity;
  int dtype;
};

enum EncodeMode { ENC_VALUE = 0, ENC_NULL_RANK = 1, ENC_SELECT = 2 };

// the value code itself lives in quantile.hpp: the host decodes selected codes with its inverse
__device__ __forceinline__ uint64_t encode_value(const KeyCol& kc, int64_t r) { return quantile::encode_value(kc.dtype, kc.values, r); }

__global__ __launch_bounds__(kBlock) void encode_kernel(KeyCol kc, const uint32_t* __restrict__ perm, int64_t n, int descending, int nulls_last, int mode,
                                                        uint64_t* __restrict__ enc) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = perm ? (int64_t)perm[i] : i;
    const bool valid = !kc.validity || ((kc.validity[r >> 6] >> (r & 63)) & 1);
    uint64_t e;
    if (mode == ENC_NULL_RANK) e = (valid == (nulls_last != 0)) ? 0ull : 1ull;   // nulls_last: valid rows rank 0; nulls first: nulls rank 0
    else if (!valid) e = (mode == ENC_SELECT && nulls_last) ? ~0ull : 0ull;       // all nulls tie within a key
    else { e = encode_value(kc, r); if (descending) e = ~e; }
    enc[i] = e;
  }
}

// hist[d * 256 + v] = rows whose digit d (bits 8d..8d+7) equals v
__global__ __launch_bounds__(kBlock) void digit_hist_kernel(const uint64_t* __restrict__ enc, int64_t n, unsigned int* __restrict__ hist) {
  __shared__ unsigned int h[8 * 256];
  for (int j = threadIdx.x; j < 8 * 256; j += kBlock) h[j] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t e = enc[i];
#pragma unroll
    for (int d = 0; d < 8; d++) atomicAdd(&h[d * 256 + (int)((e >> (8 * d)) & 255)], 1u);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < 8 * 256; j += kBlock) if (h[j]) atomicAdd(&hist[j], h[j]);
}

// block_hist[v * nblocks + b] = keys of tile b with digit v
__global__ __launch_bounds__(kBlock) void radix_count_kernel(const uint64_t* __restrict__ enc, int64_t n, int shift, unsigned int* __restrict__ block_hist, uint32_t nblocks) {
  __shared__ unsigned int h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * kTile;
#pragma unroll 4
  for (int r = 0; r < kItems; r++) {
    const int64_t i = base + (int64_t)r * kBlock + threadIdx.x;
    if (i < n) atomicAdd(&h[(int)((enc[i] >> shift) & 255)], 1u);
  }
  __syncthreads();
  block_hist[(uint64_t)threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];
}

// Stable scatter of one tile, staged through LDS so that HBM sees whole runs instead of 12-byte fragments:
//   0. the tile's keys are loaded once into registers and histogrammed (LDS atomics) -> local start of every digit value;
//   1. ranking rounds of kIPT * kBlock keys (key j of lane t = tile_base + round * kIPT * kBlock + j * kBlock + t): every
//      (item j, wave w) pair ranks its 64 keys with ballots (match-any on the digit) and publishes one count per digit;
//      after ONE barrier thread d turns the kIPT * kWaves counts of digit d into exclusive prefixes (item-major, then
//      wave = input order) and advances the digit's running position; after a second barrier every key knows its slot
//      in the LDS copy of the tile, which ends up sorted by digit with ties in input order;
//   2. the LDS copy is written out linearly: neighbouring lanes hold neighbouring keys of the same digit run, so the
//      stores of a run (4096 / 256 = 16 keys = 128 B of codes on average) coalesce.
constexpr int kIPT = 4;                          // keys per thread and ranking round
constexpr int kGroups = kIPT * kWaves;           // (item, wave) pairs of a round, in input order
static_assert(kItems % kIPT == 0, "a tile is a whole number of rounds");
// kPayload = false: key-only instantiation (sort_keys_u64: the whole record is the 64-bit code -- 8 B read + 8 B written per key and pass, 34 KB of LDS, no index staging)
template <bool kPayload>
__global__ __launch_bounds__(kBlock) void radix_scatter_kernel(const uint64_t* __restrict__ enc_in, const uint32_t* __restrict__ idx_in, int64_t n, int shift,
                                                               const uint64_t* __restrict__ offsets, uint32_t nblocks, uint64_t* __restrict__ enc_out,
                                                               uint32_t* __restrict__ idx_out) {
  __shared__ uint64_t s_enc[kTile];              // the tile, sorted by digit (32 KB)
  __shared__ uint32_t s_idx[kPayload ? kTile : 1];   // 16 KB
  __shared__ uint64_t gbase[256];                // global slot of the digit's first key of this tile minus its local start
  __shared__ unsigned int hist[256];             // tile histogram, then the running local position of every digit value
  __shared__ unsigned int round_base[256];       // hist[] as it was at the start of the round
  __shared__ uint8_t cnt[kGroups][256];          // keys of (item, wave) with the digit (<= 64; zero between rounds)
  __shared__ uint16_t pre[kGroups][256];         // exclusive prefix of cnt over the (item, wave) pairs (<= kIPT * kBlock)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t base = (int64_t)blockIdx.x * kTile;
  uint64_t e[kItems]; uint32_t idx[kPayload ? kItems : 1];
  hist[tid] = 0;
#pragma unroll
  for (int q = 0; q < kGroups; q++) cnt[q][tid] = 0;
#pragma unroll
  for (int k = 0; k < kItems; k++) {
    const int64_t i = base + (int64_t)k * kBlock + tid;
    e[k] = i < n ? enc_in[i] : 0ull;
    if constexpr (kPayload) idx[k] = i < n ? (idx_in ? idx_in[i] : (uint32_t)i) : 0u;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kItems; k++) if (base + (int64_t)k * kBlock + tid < n) atomicAdd(&hist[(int)((e[k] >> shift) & 255)], 1u);
  __syncthreads();
  if (wave == 0) {   // exclusive scan of the 256 counts: 4 per lane + a wave scan of the lane totals
    unsigned int v[4], tot = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) { v[c] = hist[lane * 4 + c]; tot += v[c]; }
    unsigned int incl = tot;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const unsigned int t = __shfl_up(incl, off, 64); if (lane >= off) incl += t; }
    unsigned int run = incl - tot;
#pragma unroll
    for (int c = 0; c < 4; c++) { hist[lane * 4 + c] = run; run += v[c]; }
  }
  __syncthreads();
  gbase[tid] = offsets[(uint64_t)tid * nblocks + blockIdx.x] - hist[tid];
#pragma unroll
  for (int r = 0; r < kItems / kIPT; r++) {
    uint32_t d[kIPT], rank[kIPT]; bool valid[kIPT];
#pragma unroll
    for (int j = 0; j < kIPT; j++) {
      const int k = r * kIPT + j;
      valid[j] = base + (int64_t)k * kBlock + tid < n;
      d[j] = (uint32_t)((e[k] >> shift) & 255);
      uint64_t same = ballot(valid[j]);            // lanes of this wave holding the same digit
#pragma unroll
      for (int b = 0; b < 8; b++) {
        const bool bit = (d[j] >> b) & 1;
        const uint64_t bal = ballot(bit);
        same &= bit ? bal : ~bal;
      }
      rank[j] = (uint32_t)prefix_rank(same);
      if (valid[j] && rank[j] == 0) cnt[j * kWaves + wave][d[j]] = (uint8_t)popc64(same);
    }
    __syncthreads();
    {
      uint32_t run = 0;
#pragma unroll
      for (int q = 0; q < kGroups; q++) { const uint32_t c = cnt[q][tid]; cnt[q][tid] = 0; pre[q][tid] = (uint16_t)run; run += c; }
      const unsigned int rb = hist[tid];
      round_base[tid] = rb;
      hist[tid] = rb + run;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kIPT; j++) {
      if (!valid[j]) continue;
      const uint32_t pos = round_base[d[j]] + pre[j * kWaves + wave][d[j]] + rank[j];
      s_enc[pos] = e[r * kIPT + j];
      if constexpr (kPayload) s_idx[pos] = idx[r * kIPT + j];
    }
    // no third barrier: the next round's leaders write cnt (already zeroed); pre / round_base are rewritten only after the next
    // round's first barrier, which every lane reaches after the reads above
  }
  __syncthreads();
  const int64_t tile_n = n - base < kTile ? n - base : kTile;
#pragma unroll 4
  for (int k = 0; k < kItems; k++) {
    const int p = k * kBlock + tid;
    if (p >= tile_n) break;
    const uint64_t ev = s_enc[p];
    const uint64_t out = gbase[(int)((ev >> shift) & 255)] + (uint64_t)p;
    enc_out[out] = ev;
    if constexpr (kPayload) idx_out[out] = s_idx[p];
  }
}

// top-k: histogram of the digit at `shift` among rows whose higher bits equal `prefix`
__global__ __launch_bounds__(kBlock) void select_hist_kernel(const uint64_t* __restrict__ enc, int64_t n, int shift, uint64_t prefix, int have_prefix,
                                                             unsigned int* __restrict__ hist) {
  __shared__ unsigned int h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t e = enc[i];
    if (!have_prefix || (e >> (shift + 8)) == prefix) atomicAdd(&h[(int)((e >> shift) & 255)], 1u);
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}
// mask bit i = (enc[i] >> shift) <= bound
__global__ __launch_bounds__(kBlock) void select_mask_kernel(const uint64_t* __restrict__ enc, int64_t n, int shift, uint64_t bound, uint64_t* __restrict__ mask) {
  const int64_t n_round = (n + 63) & ~63ll;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_round; i += (int64_t)gridDim.x * blockDim.x) {
    const bool keep = i < n && (enc[i] >> shift) <= bound;
    const uint64_t m = ballot(keep);
    if ((threadIdx.x & 63) == 0) mask[i >> 6] = m;
  }
}

// ---- small inputs (a group-by result, top-k candidates): ONE workgroup, comparison rank sort, no host round trips ----
// enc[j * m + i] = order-preserving code of key j for row i, with the null rank folded into nr (bit j of nr[i] set =
// the row sorts AFTER every non-flagged row on key j ... see rank_before).  out[rank(i)] = perm ? perm[i] : i.
constexpr int kSmallBlock = 1024;
constexpr int kSmallMax = 2048;
constexpr int kSmallMaxKeys = 8;

// per key two codes: hi = null rank (0 / 1), lo = value code (0 for nulls); row a sorts before row b iff the
// (hi, lo) sequence over the keys is lexicographically smaller, ties broken by the row position (stable)
__global__ __launch_bounds__(kSmallBlock) void small_rank_sort_kernel(const uint64_t* __restrict__ enc, const uint8_t* __restrict__ nr, int n_keys, int m,
                                                                      const uint32_t* __restrict__ perm, uint32_t* __restrict__ out) {
  for (int i = threadIdx.x; i < m; i += kSmallBlock) {
    uint64_t mine[kSmallMaxKeys]; uint8_t mnr[kSmallMaxKeys];
#pragma unroll
    for (int j = 0; j < kSmallMaxKeys; j++) if (j < n_keys) { mine[j] = enc[(size_t)j * m + i]; mnr[j] = nr[(size_t)j * m + i]; }
    uint32_t rank = 0;
    for (int o = 0; o < m; o++) {          // o is wave-uniform: the loads below are scalar / broadcast
      int c = 0;                           // <0: row o sorts before row i
#pragma unroll
      for (int j = 0; j < kSmallMaxKeys; j++) {
        if (j < n_keys && c == 0) {
          const uint8_t onr = nr[(size_t)j * m + o];
          const uint64_t oe = enc[(size_t)j * m + o];
          c = onr != mnr[j] ? (onr < mnr[j] ? -1 : 1) : (oe != mine[j] ? (oe < mine[j] ? -1 : 1) : 0);
        }
      }
      rank += (c < 0 || (c == 0 && o < i)) ? 1u : 0u;
    }
    out[rank] = perm ? perm[i] : (uint32_t)i;
  }
}

__global__ __launch_bounds__(kBlock) void encode_small_kernel(KeyCol kc, const uint32_t* __restrict__ perm, int m, int descending, int nulls_last,
                                                              uint64_t* __restrict__ enc, uint8_t* __restrict__ nr) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const int64_t r = perm ? (int64_t)perm[i] : i;
  const bool valid = !kc.validity || ((kc.validity[r >> 6] >> (r & 63)) & 1);
  uint64_t e = 0;
  if (valid) { e = encode_value(kc, r); if (descending) e = ~e; }
  enc[i] = e;
  nr[i] = (valid == (nulls_last != 0)) ? 0 : 1;
}

// ---------------------------------------------------------------------------------------------- host side ---
static KeyCol key_col(const ColumnPtr& c) { KeyCol kc; kc.values = c->data(); kc.validity = c->valid_words(); kc.dtype = c->dtype; return kc; }

struct Work {
  int64_t m = 0;                 // rows being sorted
  bool keys_only = false;        // sort_keys_u64: enc[] is the whole record, no permutation travels with it
  Buf enc[2], idx[2];            // ping-pong buffers
  int cur = 0;                   // idx[cur] holds the current permutation (when have_perm)
  bool have_perm = false;        // false: identity
  Buf hist, block_hist, offsets;
  uint32_t nblocks = 0;
  int passes = 0, skipped = 0;
};

static void encode(const SortKey& key, const uint32_t* perm, int64_t m, int mode, uint64_t* out) {
  if (!m) return;
  ProfileScope ps("sort_encode", (uint64_t)m * ((dtype_width(key.col->dtype) ? dtype_width(key.col->dtype) : 1) + 8 + (perm ? 4 : 0)), (uint64_t)m);
  hipLaunchKernelGGL(encode_kernel, dim3(k::grid_for(m, kBlock * 4)), dim3(kBlock), 0, stream(), key_col(key.col), perm, m, key.descending ? 1 : 0,
                     key.nulls_last ? 1 : 0, mode, out);
  PLX_HIP(hipGetLastError());
}

static void radix_pass(Work& w, int shift) {
  const int64_t m = w.m;
  {
    ProfileScope ps("sort_radix_count", (uint64_t)m * 8, (uint64_t)m);
    hipLaunchKernelGGL(radix_count_kernel, dim3(w.nblocks), dim3(kBlock), 0, stream(), w.enc[w.cur]->as<uint64_t>(), m, shift, w.block_hist->as<unsigned int>(), w.nblocks);
    PLX_HIP(hipGetLastError());
  }
  k::exclusive_scan_u32(w.block_hist->as<uint32_t>(), w.offsets->as<uint64_t>(), (int64_t)w.nblocks * 256);
  if (w.keys_only) {
    ProfileScope ps("sort_radix_scatter_keys", (uint64_t)m * 16, (uint64_t)m);
    hipLaunchKernelGGL(radix_scatter_kernel<false>, dim3(w.nblocks), dim3(kBlock), 0, stream(), w.enc[w.cur]->as<uint64_t>(), (const uint32_t*)nullptr, m, shift, w.offsets->as<uint64_t>(),
                       w.nblocks, w.enc[w.cur ^ 1]->as<uint64_t>(), (uint32_t*)nullptr);
    PLX_HIP(hipGetLastError());
    w.cur ^= 1;
    w.passes++;
    return;
  }
  {
    ProfileScope ps("sort_radix_scatter", (uint64_t)m * 24, (uint64_t)m);
    hipLaunchKernelGGL(radix_scatter_kernel<true>, dim3(w.nblocks), dim3(kBlock), 0, stream(), w.enc[w.cur]->as<uint64_t>(),
                       w.have_perm ? w.idx[w.cur]->as<uint32_t>() : (const uint32_t*)nullptr, m, shift, w.offsets->as<uint64_t>(), w.nblocks,
                       w.enc[w.cur ^ 1]->as<uint64_t>(), w.idx[w.cur ^ 1]->as<uint32_t>());
    PLX_HIP(hipGetLastError());
  }
  w.cur ^= 1;
  w.have_perm = true;
  w.passes++;
}

// stable sort of the current permutation by the digits of enc[cur] on which rows differ (digits first_digit .. max_digits - 1, least significant first)
static void sort_encoded(Work& w, int max_digits, int first_digit = 0) {
  PLX_HIP(hipMemsetAsync(w.hist->ptr, 0, 8 * 256 * sizeof(unsigned int), stream()));
  hipLaunchKernelGGL(digit_hist_kernel, dim3(k::grid_for(w.m, kBlock * 8, 4)), dim3(kBlock), 0, stream(), w.enc[w.cur]->as<uint64_t>(), w.m, w.hist->as<unsigned int>());
  PLX_HIP(hipGetLastError());
  std::vector<unsigned int> h(8 * 256);
  d2h_sync(h.data(), w.hist->ptr, h.size() * sizeof(unsigned int));
  for (int d = first_digit; d < max_digits; d++) {
    bool uniform = false;
    for (int v = 0; v < 256; v++) if ((int64_t)h[d * 256 + v] == w.m) { uniform = true; break; }
    if (uniform) { w.skipped++; continue; }
    // the next pass reads enc[cur]; enc must travel with the permutation, which radix_pass does
    radix_pass(w, 8 * d);
  }
}

static void sort_by_key(Work& w, const SortKey& key) {
  const uint32_t* perm = w.have_perm ? w.idx[w.cur]->as<uint32_t>() : nullptr;
  encode(key, perm, w.m, ENC_VALUE, w.enc[w.cur]->as<uint64_t>());
  const int wd = dtype_width(key.col->dtype);
  // unsigned / bool keys only populate their own width; signed and float keys use all 8 bytes (the histogram skips the uniform ones)
  const int digits = key.descending ? 8 : (key.col->dtype == PLX_BOOL ? 1 : (dtype_is_unsigned(key.col->dtype) ? wd : 8));
  sort_encoded(w, digits);
  if (key.col->validity && column_null_count(key.col) > 0) {
    perm = w.have_perm ? w.idx[w.cur]->as<uint32_t>() : nullptr;
    encode(key, perm, w.m, ENC_NULL_RANK, w.enc[w.cur]->as<uint64_t>());
    sort_encoded(w, 1);
  }
}

static void init_work(Work& w, int64_t m, Buf initial_perm) {
  w.m = m;
  const size_t m1 = (size_t)std::max<int64_t>(m, 1);
  for (int i = 0; i < 2; i++) { w.enc[i] = dev_alloc(m1 * 8); w.idx[i] = dev_alloc(m1 * 4); }
  if (initial_perm) { w.idx[0] = initial_perm; w.have_perm = true; }
  w.nblocks = (uint32_t)((m + kTile - 1) / kTile);
  if (!w.nblocks) w.nblocks = 1;
  w.hist = dev_alloc(8 * 256 * sizeof(unsigned int));
  w.block_hist = dev_alloc((size_t)w.nblocks * 256 * sizeof(unsigned int));
  w.offsets = dev_alloc(((size_t)w.nblocks * 256 + 1) * sizeof(uint64_t));
}

// Key-only stable LSD radix of m 64-bit codes on their digits first_digit .. 7 (sort.hpp): the count / scan / scatter pass of the arg-sort without the permutation.
Buf sort_keys_u64(Buf keys, int64_t m, int first_digit, int* passes, int* skipped) {
  PLX_REQUIRE(first_digit >= 0 && first_digit < 8, PLX_ERR_INVALID, "sort_keys_u64: first digit outside 0..7");
  PLX_REQUIRE(m >= 0 && m < 0xffffffffll, PLX_ERR_UNSUPPORTED, "sort_keys_u64: more keys than u32 IdxSize");
  if (passes) *passes = 0;
  if (skipped) *skipped = 0;
  if (m <= 1) return keys;
  Work w;
  w.m = m; w.keys_only = true;
  w.enc[0] = keys; w.enc[1] = dev_alloc((size_t)m * 8);
  w.nblocks = (uint32_t)((m + kTile - 1) / kTile);
  w.hist = dev_alloc(8 * 256 * sizeof(unsigned int));
  w.block_hist = dev_alloc((size_t)w.nblocks * 256 * sizeof(unsigned int));
  w.offsets = dev_alloc(((size_t)w.nblocks * 256 + 1) * sizeof(uint64_t));
  sort_encoded(w, 8, first_digit);
  if (passes) *passes = w.passes;
  if (skipped) *skipped = w.skipped;
  return w.enc[w.cur];
}

static ColumnPtr make_idx(int64_t n) {
  auto c = std::make_shared<Column>();
  c->dtype = PLX_U32; c->len = n; c->values = dev_alloc(values_bytes(PLX_U32, std::max<int64_t>(n, 1))); c->null_count = 0;
  return c;
}

ColumnPtr sort_indices(const std::vector<SortKey>& keys, int64_t limit, std::string* desc) {
  PLX_REQUIRE(!keys.empty(), PLX_ERR_INVALID, "sort needs at least one key");
  const int64_t n = keys[0].col->len;
  for (auto& kx : keys) PLX_REQUIRE(kx.col->len == n, PLX_ERR_SHAPE, "sort: key columns have different lengths");
  PLX_REQUIRE(n < 0xffffffffll, PLX_ERR_UNSUPPORTED, "sort: more rows than u32 IdxSize");
  const int64_t n_out = limit < 0 ? n : std::min(limit, n);
  ColumnPtr out = make_idx(n_out);
  if (n_out == 0) { if (desc) *desc = "sort[empty]"; return out; }
  std::string d;
  Buf cand;            // candidate rows of the top-k selection (row order)
  int64_t m = n;
  if (limit >= 0 && limit < n / 4 && n > 65536) {
    // ---- MSD radix select on the first key: smallest prefix bucket holding the limit-th row
    Buf enc0 = dev_alloc((size_t)n * 8);
    encode(keys[0], nullptr, n, ENC_SELECT, enc0->as<uint64_t>());
    Buf hist = dev_alloc(256 * sizeof(unsigned int));
    std::vector<unsigned int> h(256);
    uint64_t prefix = 0, need = (uint64_t)limit, below = 0, cand_rows = (uint64_t)n;
    int shift = 56, rounds = 0;
    bool have = false;
    const uint64_t good_enough = std::max<uint64_t>(2 * (uint64_t)limit, (uint64_t)kSmallMax);   // small enough for the one-workgroup sort
    for (;; shift -= 8) {
      PLX_HIP(hipMemsetAsync(hist->ptr, 0, 256 * sizeof(unsigned int), stream()));
      {
        ProfileScope ps("topk_select_hist", (uint64_t)n * 8, (uint64_t)n);
        hipLaunchKernelGGL(select_hist_kernel, dim3(k::grid_for(n, kBlock * 8, 4)), dim3(kBlock), 0, stream(), enc0->as<uint64_t>(), n, shift, prefix, have ? 1 : 0, hist->as<unsigned int>());
        PLX_HIP(hipGetLastError());
      }
      d2h_sync(h.data(), hist->ptr, 256 * sizeof(unsigned int));
      rounds++;
      uint64_t c = 0; int b = 0;
      for (; b < 255; b++) { if (c + h[b] >= need) break; c += h[b]; }
      below += c; need -= c;
      prefix = (prefix << 8) | (uint64_t)b; have = true;
      cand_rows = below + h[b];
      if (cand_rows <= good_enough || shift == 0) break;
    }
    if (cand_rows < (uint64_t)n / 2) {
      Buf mask = dev_alloc(bitmap_bytes(n));
      {
        ProfileScope ps("topk_select_mask", (uint64_t)n * 8 + (uint64_t)n / 8, (uint64_t)n);
        hipLaunchKernelGGL(select_mask_kernel, dim3(k::grid_for(n, kBlock * 8, 4)), dim3(kBlock), 0, stream(), enc0->as<uint64_t>(), n, shift, prefix, mask->as<uint64_t>());
        PLX_HIP(hipGetLastError());
      }
      k::FilterPlan fp = k::filter_prepare(mask->as<uint64_t>(), n);
      PLX_REQUIRE((uint64_t)fp.n_out == cand_rows, PLX_ERR_INVALID, "top-k: candidate count mismatch");
      Buf iota = dev_alloc((size_t)n * 4);
      k::fill_iota_u32(iota->as<uint32_t>(), n);
      cand = dev_alloc((size_t)std::max<int64_t>(fp.n_out, 1) * 4);
      k::filter_apply(fp, 4, iota->ptr, nullptr, cand->ptr, nullptr);
      m = fp.n_out;
      d += "top_k_select[" + std::to_string(rounds) + " digit rounds, candidates=" + std::to_string(m) + "] -> ";
    }
  }
  if (m <= kSmallMax && (int)keys.size() <= kSmallMaxKeys) {
    const int nk = (int)keys.size();
    Buf enc = dev_alloc((size_t)nk * m * 8), nr = dev_alloc((size_t)nk * m);
    const uint32_t* perm = cand ? cand->as<uint32_t>() : nullptr;
    ProfileScope ps("sort_small", (uint64_t)m * nk * 9, (uint64_t)m);
    for (int j = 0; j < nk; j++) {
      hipLaunchKernelGGL(encode_small_kernel, dim3((unsigned)((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream(), key_col(keys[j].col), perm, (int)m,
                         keys[j].descending ? 1 : 0, keys[j].nulls_last ? 1 : 0, enc->as<uint64_t>() + (size_t)j * m, nr->as<uint8_t>() + (size_t)j * m);
      PLX_HIP(hipGetLastError());
    }
    Buf sorted = dev_alloc((size_t)m * 4);
    hipLaunchKernelGGL(small_rank_sort_kernel, dim3(1), dim3(kSmallBlock), 0, stream(), enc->as<uint64_t>(), nr->as<uint8_t>(), nk, (int)m, perm, sorted->as<uint32_t>());
    PLX_HIP(hipGetLastError());
    PLX_HIP(hipMemcpyAsync(out->values->ptr, sorted->ptr, (size_t)n_out * 4, hipMemcpyDeviceToDevice, stream()));
    d += "rank_sort[rows=" + std::to_string(m) + ", keys=" + std::to_string(nk) + ", one workgroup]";
    if (desc) *desc = d;
    return out;
  }
  Work w;
  init_work(w, m, cand);
  for (size_t j = keys.size(); j-- > 0;) sort_by_key(w, keys[j]);
  if (w.have_perm) PLX_HIP(hipMemcpyAsync(out->values->ptr, w.idx[w.cur]->ptr, (size_t)n_out * 4, hipMemcpyDeviceToDevice, stream()));
  else k::fill_iota_u32(out->values->as<uint32_t>(), n_out);   // every digit of every key was uniform
  d += "radix_sort[rows=" + std::to_string(m) + ", keys=" + std::to_string(keys.size()) + ", passes=" + std::to_string(w.passes) + ", uniform digits skipped=" + std::to_string(w.skipped) + "]";
  if (desc) *desc = d;
  return out;
}

// ------------------------------------------------------------------------------ median / quantile ---
// Whole column: MSD radix select.  The codes are ENC_SELECT's (nulls = ~0, after every valid row; a valid ~0 ties with them, which moves no valid rank).  The first
// round histograms the top digit and reduces AND / OR over the valid codes: a digit on which AND == OR is the same in every valid row and costs no round, as in the
// sort.  Every other digit is one select_hist_kernel pass under the prefix chosen so far.  8 B read per row and round.
__global__ __launch_bounds__(kBlock) void select_first_kernel(const uint64_t* __restrict__ enc, const uint64_t* __restrict__ validity, int64_t n, unsigned int* __restrict__ hist,
                                                              unsigned long long* __restrict__ and_or) {
  __shared__ unsigned int h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  uint64_t a = ~0ull, o = 0ull;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t e = enc[i];
    atomicAdd(&h[(int)(e >> 56)], 1u);
    if (!validity || ((validity[i >> 6] >> (i & 63)) & 1)) { a &= e; o |= e; }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { a &= shfl_xor_u64(a, m); o |= shfl_xor_u64(o, m); }
  if ((threadIdx.x & 63) == 0) { atomicAnd(&and_or[0], (unsigned long long)a); atomicOr(&and_or[1], (unsigned long long)o); }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}
// *out = the smallest code greater than `code` (~0 when there is none; *out starts as ~0)
__global__ __launch_bounds__(kBlock) void select_next_kernel(const uint64_t* __restrict__ enc, int64_t n, uint64_t code, unsigned long long* __restrict__ out) {
  uint64_t m = ~0ull;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t e = enc[i];
    if (e > code && e < m) m = e;
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) { const uint64_t t = shfl_xor_u64(m, s); m = t < m ? t : m; }
  if ((threadIdx.x & 63) == 0 && m != ~0ull) atomicMin(out, (unsigned long long)m);
}

SelectedRanks select_ranks(const ColumnPtr& col, int64_t n_valid, uint64_t lo, uint64_t hi, std::string* desc) {
  const int64_t n = col->len;
  PLX_REQUIRE(n < 0xffffffffll, PLX_ERR_UNSUPPORTED, "quantile: more rows than u32 IdxSize");
  PLX_REQUIRE(n_valid >= 1 && n_valid <= n && lo <= hi && hi <= lo + 1 && hi < (uint64_t)n_valid, PLX_ERR_INVALID, "quantile select: ranks outside the valid rows");
  Buf enc = dev_alloc((size_t)n * 8);
  SortKey key; key.col = col; key.descending = false; key.nulls_last = true;
  encode(key, nullptr, n, ENC_SELECT, enc->as<uint64_t>());
  constexpr size_t kHistBytes = 256 * sizeof(unsigned int);
  Buf hist = dev_alloc(kHistBytes + 16);            // 256 counts, then AND and OR of the valid codes
  unsigned long long* and_or = reinterpret_cast<unsigned long long*>(hist->as<unsigned char>() + kHistBytes);
  struct { unsigned int h[256]; unsigned long long and_or[2]; } host;
  static_assert(sizeof(host) == kHistBytes + 16, "histogram and the AND / OR pair are one copy");
  const int grid = k::grid_for(n, kBlock * 8, 4);
  uint64_t prefix = 0, need = lo + 1, below = 0, mult = 0;
  auto pick = [&]() {      // the bucket that holds the need-th smallest row under the prefix
    uint64_t c = 0; int b = 0;
    for (; b < 255; b++) { if (c + host.h[b] >= need) break; c += host.h[b]; }
    below += c; need -= c; mult = host.h[b];
    prefix = (prefix << 8) | (uint64_t)b;
  };
  PLX_HIP(hipMemsetAsync(hist->ptr, 0, kHistBytes + 16, stream()));
  PLX_HIP(hipMemsetAsync(and_or, 0xff, 8, stream()));
  {
    ProfileScope ps("quantile_select_first", (uint64_t)n * 8 + (uint64_t)n / 8, (uint64_t)n);
    hipLaunchKernelGGL(select_first_kernel, dim3(grid), dim3(kBlock), 0, stream(), enc->as<uint64_t>(), col->valid_words(), n, hist->as<unsigned int>(), and_or);
    PLX_HIP(hipGetLastError());
  }
  d2h_sync(&host, hist->ptr, sizeof(host));
  pick();
  int rounds = 1;
  const uint64_t differs = host.and_or[0] ^ host.and_or[1];
  const uint64_t common = host.and_or[0];
  for (int shift = 48; shift >= 0; shift -= 8) {
    if (((differs >> shift) & 255) == 0) { prefix = (prefix << 8) | ((common >> shift) & 255); continue; }      // every valid row agrees on this digit
    PLX_HIP(hipMemsetAsync(hist->ptr, 0, kHistBytes, stream()));
    {
      ProfileScope ps("quantile_select_hist", (uint64_t)n * 8, (uint64_t)n);
      hipLaunchKernelGGL(select_hist_kernel, dim3(grid), dim3(kBlock), 0, stream(), enc->as<uint64_t>(), n, shift, prefix, 1, hist->as<unsigned int>());
      PLX_HIP(hipGetLastError());
    }
    d2h_sync(host.h, hist->ptr, kHistBytes);
    pick();
    rounds++;
  }
  mult = std::min<uint64_t>(mult, (uint64_t)n_valid - below);      // nulls share the last bucket of an all-ones prefix
  SelectedRanks r;
  r.code_lo = r.code_hi = prefix;
  const char* next = "none";
  if (hi != lo) {
    if (below + mult > hi) next = "same";
    else {
      next = "min_pass";
      PLX_HIP(hipMemsetAsync(and_or, 0xff, 8, stream()));
      {
        ProfileScope ps("quantile_select_next", (uint64_t)n * 8, (uint64_t)n);
        hipLaunchKernelGGL(select_next_kernel, dim3(grid), dim3(kBlock), 0, stream(), enc->as<uint64_t>(), n, r.code_lo, and_or);
        PLX_HIP(hipGetLastError());
      }
      unsigned long long nx = 0;
      d2h_sync(&nx, and_or, 8);
      r.code_hi = nx;
    }
  }
  if (desc) *desc = "quantile_select[rows=" + std::to_string(n) + ", valid=" + std::to_string(n_valid) + ", rounds=" + std::to_string(rounds) + ", next=" + next + "]";
  return r;
}

// Grouped: the rows sorted by (keys..., value asc nulls last) fall into one segment per group, the valid values of a segment in order in front of its nulls.
struct SegKeys { KeyCol k[kSegmentMaxKeys]; int n; };

__device__ __forceinline__ bool row_valid(const KeyCol& kc, int64_t r) { return !kc.validity || ((kc.validity[r >> 6] >> (r & 63)) & 1); }

// mask bit i = row i of the sorted order starts a segment: i == 0, or a key differs from row i - 1 (the sort's equality: null == null, NaN == NaN, -0 == +0)
__global__ __launch_bounds__(kBlock) void segment_heads_kernel(SegKeys keys, const uint32_t* __restrict__ perm, int64_t n, uint64_t* __restrict__ mask) {
  const int64_t n_round = (n + 63) & ~63ll;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_round; i += (int64_t)gridDim.x * blockDim.x) {
    bool head = false;
    if (i < n) {
      head = i == 0;
      if (!head) {
        const int64_t r = (int64_t)perm[i], p = (int64_t)perm[i - 1];
#pragma unroll
        for (int j = 0; j < kSegmentMaxKeys; j++) {
          if (j < keys.n && !head) {
            const bool vr = row_valid(keys.k[j], r), vp = row_valid(keys.k[j], p);
            head = vr != vp || (vr && encode_value(keys.k[j], r) != encode_value(keys.k[j], p));
          }
        }
      }
    }
    const uint64_t m = ballot(head);
    if ((threadIdx.x & 63) == 0) mask[i >> 6] = m;
  }
}

// one group per lane: the segment [starts[g], starts[g + 1]) (the last one ends at n), its valid rows by a binary search for the first null, two gathered values
__global__ __launch_bounds__(kBlock) void segment_quantile_kernel(KeyCol v, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ starts, int64_t n_groups, int64_t n,
                                                                  double q, int interpolation, int out_f32, void* __restrict__ out, uint64_t* __restrict__ out_valid) {
  const int64_t g_round = (n_groups + 63) & ~63ll;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < g_round; g += (int64_t)gridDim.x * blockDim.x) {
    bool ok = false;
    double res = 0.0;
    if (g < n_groups) {
      const int64_t s = (int64_t)starts[g], e = g + 1 < n_groups ? (int64_t)starts[g + 1] : n;
      int64_t nv = e - s;
      if (v.validity) {
        int64_t lo = s, hi = e;
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (row_valid(v, (int64_t)perm[mid])) lo = mid + 1; else hi = mid; }
        nv = lo - s;
      }
      if (nv > 0) {
        const quantile::Rank rk = quantile::rank_of((uint64_t)nv, q, interpolation);
        const double a = quantile::decode(v.dtype, encode_value(v, (int64_t)perm[s + (int64_t)rk.lo]));
        const double b = rk.hi == rk.lo ? a : quantile::decode(v.dtype, encode_value(v, (int64_t)perm[s + (int64_t)rk.hi]));
        res = quantile::combine(a, b, rk.frac, interpolation);
        ok = true;
      }
      if (out_f32) reinterpret_cast<float*>(out)[g] = (float)res; else reinterpret_cast<double*>(out)[g] = res;
    }
    const uint64_t m = ballot(ok);
    if ((threadIdx.x & 63) == 0) out_valid[g >> 6] = m;
  }
}

// the segment-head mask of a sorted order (`perm`: a sort_indices of n >= 1 rows by `keys`): what sort_segments, distinct_rows and segment_head_ranks start from
static Buf segment_heads_of(const std::vector<ColumnPtr>& keys, const ColumnPtr& perm, int64_t n) {
  SegKeys segk{};
  segk.n = (int)keys.size();
  for (size_t j = 0; j < keys.size(); j++) segk.k[j] = key_col(keys[j]);
  Buf heads = dev_alloc(bitmap_bytes(n));
  ProfileScope ps("segment_heads", (uint64_t)n * 4 + (uint64_t)n / 8, (uint64_t)n);
  hipLaunchKernelGGL(segment_heads_kernel, dim3(k::grid_for(n, kBlock * 4)), dim3(kBlock), 0, stream(), segk, perm->values->as<uint32_t>(), n, heads->as<uint64_t>());
  PLX_HIP(hipGetLastError());
  return heads;
}

__global__ __launch_bounds__(kBlock) void invert_permutation_kernel(const uint32_t* __restrict__ perm, int64_t n, uint32_t* __restrict__ inv) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t p = perm[i];
    if ((int64_t)p < n) inv[p] = (uint32_t)i;
  }
}

ColumnPtr invert_permutation(const ColumnPtr& perm) {
  PLX_REQUIRE(perm->dtype == PLX_U32 && !perm->validity, PLX_ERR_INVALID, "invert_permutation: a u32 permutation without nulls");
  ColumnPtr out = make_idx(perm->len);
  if (!perm->len) return out;
  ProfileScope ps("invert_permutation", (uint64_t)perm->len * 8, (uint64_t)perm->len);
  hipLaunchKernelGGL(invert_permutation_kernel, dim3(k::grid_for(perm->len, kBlock * 4)), dim3(kBlock), 0, stream(), perm->values->as<uint32_t>(), perm->len, out->values->as<uint32_t>());
  PLX_HIP(hipGetLastError());
  return out;
}

SortedSegments sort_segments(const std::vector<ColumnPtr>& keys, const ColumnPtr& value, int64_t expect_groups, bool descending) {
  PLX_REQUIRE((int)keys.size() <= kSegmentMaxKeys, PLX_ERR_UNSUPPORTED, "sorted segments: 1.." + std::to_string(kSegmentMaxKeys) + " key columns, got " + std::to_string(keys.size()));
  SortedSegments seg;
  seg.value = value;
  const int64_t n = seg.n = value->len;
  std::vector<SortKey> sk;
  for (const ColumnPtr& kc : keys) { SortKey s; s.col = kc; s.nulls_last = true; sk.push_back(s); }
  { SortKey s; s.col = value; s.nulls_last = true; s.descending = descending; sk.push_back(s); }
  seg.perm = sort_indices(sk, -1, &seg.sort_desc);
  seg.starts = dev_alloc(4);
  if (n) {
    seg.heads = segment_heads_of(keys, seg.perm, n);      // (no key: position 0 alone)
    k::FilterPlan fp = k::filter_prepare(seg.heads->as<uint64_t>(), n);
    seg.n_groups = fp.n_out;
    PLX_REQUIRE(expect_groups < 0 || seg.n_groups == expect_groups, PLX_ERR_INVALID, "sorted segments: segment count mismatch (" + std::to_string(seg.n_groups) + " segments, " + std::to_string(expect_groups) + " groups)");
    Buf iota = dev_alloc((size_t)n * 4);
    k::fill_iota_u32(iota->as<uint32_t>(), n);
    seg.starts = dev_alloc((size_t)std::max<int64_t>(seg.n_groups, 1) * 4);
    k::filter_apply(fp, 4, iota->ptr, nullptr, seg.starts->ptr, nullptr);
  } else {
    PLX_REQUIRE(expect_groups <= 0, PLX_ERR_INVALID, "sorted segments: segment count mismatch (0 segments, " + std::to_string(expect_groups) + " groups)");
  }
  return seg;
}

std::vector<ColumnPtr> segment_quantiles(const SortedSegments& seg, const std::vector<QuantileSpec>& specs) {
  const bool f32 = seg.value->dtype == PLX_F32;
  const int64_t n_groups = seg.n_groups;
  std::vector<ColumnPtr> out;
  for (const QuantileSpec& sp : specs) {
    auto c = std::make_shared<Column>();
    c->dtype = f32 ? PLX_F32 : PLX_F64; c->len = n_groups;
    c->values = dev_alloc(values_bytes(c->dtype, std::max<int64_t>(n_groups, 1)));
    c->validity = dev_alloc_zero(bitmap_bytes(n_groups));
    c->null_count = -1;
    if (n_groups) {
      ProfileScope ps("segment_quantile", (uint64_t)n_groups * 32, (uint64_t)n_groups);
      hipLaunchKernelGGL(segment_quantile_kernel, dim3(k::grid_for(n_groups, kBlock)), dim3(kBlock), 0, stream(), key_col(seg.value), seg.perm->values->as<uint32_t>(), seg.starts->as<uint32_t>(), n_groups, seg.n,
                         sp.q, sp.interpolation, f32 ? 1 : 0, c->values->ptr, c->validity->as<uint64_t>());
      PLX_HIP(hipGetLastError());
    }
    out.push_back(c);
  }
  return out;
}

// ------------------------------------------------------------------------------ n_unique / unique() ---
// Both are runs of equal values in a sorted order; the arithmetic on the run-head masks is distinct.hpp's.  All atomics are vector atomics on integers (OR, ADD):
// the same input gives the same bits every time.
__device__ __forceinline__ bool mask_bit(const uint64_t* __restrict__ m, int64_t i) { return (m[i >> 6] >> (i & 63)) & 1; }
// the value of row r of an integer column as i64 (every integer dtype but U64, whose range no i64 pair holds: the host never sends one)
__device__ __forceinline__ int64_t int_value(const KeyCol& kc, int64_t r) {
  const uint64_t e = encode_value(kc, r);
  switch (kc.dtype) {
    case PLX_I8: case PLX_I16: case PLX_I32: case PLX_I64: return (int64_t)(e ^ quantile::kSign);
    default: return (int64_t)e;
  }
}

// Whole column, bitmap route: bit (v - mn) of bits[] for every valid row; bits[] holds `range` zeroed bits (a row outside [mn, mn + range) sets nothing).  A lane
// whose bit already shows in a plain load of the word issues no atomic (a stale load only costs a redundant OR); among the lanes left, one per distinct bit does --
// the lowest, found by a readlane / ballot round per distinct value still pending, so a wave of equal values is one atomic and a wave of 64 new values 64 rounds.
// 1..8 B read per row; the atomics land in L2.
__global__ __launch_bounds__(kBlock) void distinct_bitmap_kernel(KeyCol kc, int64_t n, int64_t mn, uint64_t range, unsigned int* __restrict__ bits) {
  const int64_t n_round = (n + 63) & ~63ll;
  const int lane = threadIdx.x & 63;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_round; i += (int64_t)gridDim.x * blockDim.x) {
    bool need = false;
    uint64_t off = 0;
    if (i < n && row_valid(kc, i)) {
      off = (uint64_t)int_value(kc, i) - (uint64_t)mn;
      need = off < range && !((bits[off >> 5] >> (off & 31)) & 1u);
    }
    uint64_t todo = ballot(need);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;      // wave-uniform
      const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)off, leader), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(off >> 32), leader);
      const uint64_t same = ballot(need && off == (((uint64_t)hi << 32) | lo));
      if (lane == leader) atomicOr(&bits[off >> 5], 1u << (off & 31));
      todo &= ~same;
    }
  }
}

// Whole column, sorted-codes route: *out += positions i < m of the sorted codes that start a run (i == 0, or codes[i] != codes[i - 1]).  A ballot and a popcount per
// wave and step, one LDS add per wave, one integer atomicAdd per block.  8 B read per position (the predecessor is the neighbouring lane's line).
__global__ __launch_bounds__(kBlock) void run_heads_count_kernel(const uint64_t* __restrict__ codes, int64_t m, unsigned int* __restrict__ out) {
  __shared__ unsigned int total;
  if (threadIdx.x == 0) total = 0;
  __syncthreads();
  unsigned int c = 0;
  const int64_t m_round = (m + 63) & ~63ll;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m_round; i += (int64_t)gridDim.x * blockDim.x) {
    const bool head = i < m && (i == 0 || codes[i] != codes[i - 1]);
    c += (unsigned int)popc64(ballot(head));
  }
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&total, c);
  __syncthreads();
  if (threadIdx.x == 0 && total) atomicAdd(out, total);
}

// Grouped: mask bit i = position i of the sorted order starts a segment (the segment-head mask) or its value differs from position i - 1 through the permutation: a
// null and a value differ, two nulls do not, values by the sort's equality.  4 B of perm + a gathered value per position.
__global__ __launch_bounds__(kBlock) void distinct_heads_kernel(KeyCol v, const uint32_t* __restrict__ perm, const uint64_t* __restrict__ seg_heads, int64_t n, uint64_t* __restrict__ mask) {
  const int64_t n_round = (n + 63) & ~63ll;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_round; i += (int64_t)gridDim.x * blockDim.x) {
    bool head = false;
    if (i < n) {
      head = i == 0 || mask_bit(seg_heads, i);
      if (!head) {
        const int64_t r = (int64_t)perm[i], p = (int64_t)perm[i - 1];
        const bool vr = row_valid(v, r), vp = row_valid(v, p);
        head = vr != vp || (vr && encode_value(v, r) != encode_value(v, p));
      }
    }
    const uint64_t m = ballot(head);
    if ((threadIdx.x & 63) == 0) mask[i >> 6] = m;
  }
}
// counts[w] = set bits of word w of a mask of n_bits bits (the input of the exclusive scan that gives distinct::rank_before its prefix)
__global__ __launch_bounds__(kBlock) void mask_word_counts_kernel(const uint64_t* __restrict__ mask, int64_t n_bits, uint32_t* __restrict__ counts) {
  const int64_t nwords = (n_bits + 63) >> 6;
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nwords; w += (int64_t)gridDim.x * blockDim.x) {
    uint64_t x = mask[w];
    if (w == nwords - 1 && (n_bits & 63)) x &= (~0ull) >> (64 - (n_bits & 63));
    counts[w] = (uint32_t)popc64(x);
  }
}
// one group per lane: the distinct values of the segment [starts[g], starts[g + 1]) (the last one ends at n) = the difference of two ranks in the mask of
// distinct_heads_kernel.  O(1) per group whatever its size.
__global__ __launch_bounds__(kBlock) void segment_distinct_kernel(const uint64_t* __restrict__ mask, const uint64_t* __restrict__ prefix, const uint32_t* __restrict__ starts, int64_t n_groups,
                                                                  int64_t n, uint32_t* __restrict__ out) {
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n_groups; g += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t s = starts[g], e = g + 1 < n_groups ? (uint64_t)starts[g + 1] : (uint64_t)n;
    out[g] = (s <= e && e <= (uint64_t)n) ? (uint32_t)(distinct::rank_before(prefix, mask, e) - distinct::rank_before(prefix, mask, s)) : 0u;
  }
}

// Distinct rows: position i of the stable sorted order is the first row of its class when the segment-head mask has bit i, the last when it has bit i + 1 (or
// i + 1 == n); a kept position sets bit perm[i] of the ROW-ORDER mask out_bits (n zeroed bits) with a u32 atomic OR.  Only kept rows issue one.
__global__ __launch_bounds__(kBlock) void distinct_keep_kernel(const uint64_t* __restrict__ heads, const uint32_t* __restrict__ perm, int64_t n, int keep, unsigned int* __restrict__ out_bits) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const bool is_head = mask_bit(heads, i), is_tail = i + 1 == n || mask_bit(heads, i + 1);
    if (!distinct::keep_row(is_head, is_tail, keep)) continue;
    const uint32_t r = perm[i];
    if ((int64_t)r < n) atomicOr(&out_bits[r >> 5], 1u << (r & 31));
  }
}

// the exclusive prefix of a mask's per-word popcounts (words + 1 entries, the last the total): what distinct::rank_before reads
Buf mask_rank_prefix(const Buf& mask, int64_t n_bits) {
  const int64_t nwords = (n_bits + 63) >> 6;
  Buf counts = dev_alloc((size_t)nwords * 4), prefix = dev_alloc(((size_t)nwords + 1) * 8);
  hipLaunchKernelGGL(mask_word_counts_kernel, dim3(k::grid_for(nwords, kBlock * 4)), dim3(kBlock), 0, stream(), mask->as<uint64_t>(), n_bits, counts->as<uint32_t>());
  PLX_HIP(hipGetLastError());
  k::exclusive_scan_u32(counts->as<uint32_t>(), prefix->as<uint64_t>(), nwords);
  return prefix;
}

static Buf distinct_heads_of(const SortedSegments& seg) {
  const int64_t n = seg.n;
  Buf mask = dev_alloc(bitmap_bytes(n));
  ProfileScope ps("distinct_heads", (uint64_t)n * (4 + (dtype_width(seg.value->dtype) ? dtype_width(seg.value->dtype) : 1)) + (uint64_t)n / 4, (uint64_t)n);
  hipLaunchKernelGGL(distinct_heads_kernel, dim3(k::grid_for(n, kBlock * 4)), dim3(kBlock), 0, stream(), key_col(seg.value), seg.perm->values->as<uint32_t>(), seg.heads->as<uint64_t>(), n, mask->as<uint64_t>());
  PLX_HIP(hipGetLastError());
  return mask;
}

ColumnPtr segment_distinct(const SortedSegments& seg) {
  const int64_t n = seg.n, n_groups = seg.n_groups;
  ColumnPtr out = make_idx(n_groups);
  if (!n_groups) return out;
  Buf mask = distinct_heads_of(seg);
  Buf prefix = mask_rank_prefix(mask, n);
  {
    ProfileScope ps("segment_distinct", (uint64_t)n_groups * 44, (uint64_t)n_groups);
    hipLaunchKernelGGL(segment_distinct_kernel, dim3(k::grid_for(n_groups, kBlock)), dim3(kBlock), 0, stream(), mask->as<uint64_t>(), prefix->as<uint64_t>(), seg.starts->as<uint32_t>(), n_groups, n,
                       out->values->as<uint32_t>());
    PLX_HIP(hipGetLastError());
  }
  return out;
}

ValueRuns value_runs(const SortedSegments& seg) {
  ValueRuns r;
  const int64_t n = seg.n;
  PLX_REQUIRE(n > 0 && seg.heads, PLX_ERR_INVALID, "value runs: sorted segments of at least one row");
  r.heads = distinct_heads_of(seg);
  r.prefix = mask_rank_prefix(r.heads, n);
  k::FilterPlan fp = k::filter_prepare(r.heads->as<uint64_t>(), n);
  r.n_runs = fp.n_out;
  Buf iota = dev_alloc((size_t)n * 4);
  k::fill_iota_u32(iota->as<uint32_t>(), n);
  r.starts = dev_alloc((size_t)std::max<int64_t>(r.n_runs, 1) * 4);
  k::filter_apply(fp, 4, iota->ptr, nullptr, r.starts->ptr, nullptr);
  return r;
}

uint32_t n_unique_column(const ColumnPtr& c, bool force_sort, std::string* desc) {
  const int64_t n = c->len;
  PLX_REQUIRE(n < 0xffffffffll, PLX_ERR_UNSUPPORTED, "n_unique: more rows than u32 IdxSize");
  if (!(dtype_is_int(c->dtype) || dtype_is_float(c->dtype) || c->dtype == PLX_BOOL)) fail(PLX_ERR_UNSUPPORTED, std::string("n_unique of a ") + dtype_name(c->dtype) + " column: integer, float and Boolean columns only");
  PLX_REQUIRE(c->values || n == 0, PLX_ERR_INVALID, "placeholder column has no data");
  if (n == 0) { if (desc) *desc = "n_unique[empty]"; return 0; }
  const int64_t nulls = column_null_count(c), n_valid = n - nulls;
  const uint32_t null_class = nulls > 0 ? 1u : 0u;
  if (c->dtype == PLX_BOOL) {
    // two popcounts (true-and-valid, valid) and the null count
    int64_t trues;
    if (c->validity) {
      Buf t = dev_alloc_zero(bitmap_bytes(n));
      k::bitmap_op(0, c->values->as<uint64_t>(), c->validity->as<uint64_t>(), n, t->as<uint64_t>());
      trues = k::bitmap_popcount(t->as<uint64_t>(), n);
    } else trues = k::bitmap_popcount(c->values->as<uint64_t>(), n);
    if (desc) *desc = "n_unique[boolean]";
    return (trues > 0 ? 1u : 0u) + (n_valid - trues > 0 ? 1u : 0u) + null_class;
  }
  int64_t mn = 0, mx = 0;
  uint64_t range = 0;
  bool bitmap = false;
  if (!force_sort && dtype_is_int(c->dtype) && c->dtype != PLX_U64 && ops::int_range(c, &mn, &mx)) {
    range = (uint64_t)mx - (uint64_t)mn + 1;      // 0 when the column spans all of i64: no bitmap
    bitmap = mx >= mn && distinct::bitmap_route_ok(range, (uint64_t)n);
  }
  if (bitmap) {
    Buf bits = dev_alloc_zero((size_t)((range + 63) / 64) * 8 + 8);
    {
      ProfileScope ps("distinct_bitmap", (uint64_t)n * dtype_width(c->dtype) + range / 4, (uint64_t)n);
      hipLaunchKernelGGL(distinct_bitmap_kernel, dim3(k::grid_for(n, kBlock * 4)), dim3(kBlock), 0, stream(), key_col(c), n, mn, range, bits->as<unsigned int>());
      PLX_HIP(hipGetLastError());
    }
    const int64_t values = k::bitmap_popcount(bits->as<uint64_t>(), (int64_t)range);
    if (desc) *desc = "n_unique[bitmap range=" + std::to_string(range) + "]";
    return (uint32_t)values + null_class;
  }
  // the select's codes: nulls = ~0 behind every valid row.  A valid ~0 (INT64_MAX, UINT64_MAX) has the code of a null and sorts among them; the first n_valid sorted
  // positions still hold every valid row's code, so the heads are counted there and the nulls added as one class of their own.
  Buf enc = dev_alloc((size_t)n * 8);
  SortKey key; key.col = c; key.descending = false; key.nulls_last = true;
  encode(key, nullptr, n, ENC_SELECT, enc->as<uint64_t>());
  int passes = 0, skipped = 0;
  Buf sorted = sort_keys_u64(enc, n, 0, &passes, &skipped);
  if (n <= 1) skipped = 8;      // (nothing to sort)
  uint32_t values = 0;
  if (n_valid > 0) {
    Buf cnt = dev_alloc_zero(4);
    {
      ProfileScope ps("run_heads_count", (uint64_t)n_valid * 8, (uint64_t)n_valid);
      hipLaunchKernelGGL(run_heads_count_kernel, dim3(k::grid_for(n_valid, kBlock * 8, 4)), dim3(kBlock), 0, stream(), sorted->as<uint64_t>(), n_valid, cnt->as<unsigned int>());
      PLX_HIP(hipGetLastError());
    }
    d2h_sync(&values, cnt->ptr, 4);
  }
  if (desc) *desc = "n_unique[sorted codes: passes=" + std::to_string(passes) + ", skipped=" + std::to_string(skipped) + "]";
  return values + null_class;
}

ColumnPtr distinct_rows(const std::vector<ColumnPtr>& keys, int keep, int64_t* kept, std::string* sort_desc) {
  PLX_REQUIRE(distinct::keep_ok(keep), PLX_ERR_INVALID, "unique: keep " + std::to_string(keep) + " is no plx_unique_keep (0..3)");
  PLX_REQUIRE(!keys.empty() && (int)keys.size() <= kSegmentMaxKeys, PLX_ERR_UNSUPPORTED, "unique: the subset takes 1.." + std::to_string(kSegmentMaxKeys) + " columns, got " + std::to_string(keys.size()));
  const int64_t n = keys[0]->len;
  for (const ColumnPtr& kc : keys) {
    PLX_REQUIRE(kc->len == n, PLX_ERR_SHAPE, "unique: subset columns have different lengths");
    if (!(dtype_is_int(kc->dtype) || dtype_is_float(kc->dtype) || kc->dtype == PLX_BOOL)) fail(PLX_ERR_UNSUPPORTED, std::string("unique over a ") + dtype_name(kc->dtype) + " column: integer, float and Boolean columns only");
    PLX_REQUIRE(kc->values || n == 0, PLX_ERR_INVALID, "placeholder column has no data");
  }
  auto out = std::make_shared<Column>();
  out->dtype = PLX_BOOL; out->len = n; out->values = dev_alloc_zero(bitmap_bytes(n)); out->null_count = 0;
  if (kept) *kept = 0;
  if (n == 0) { if (sort_desc) *sort_desc = "sort[empty]"; return out; }
  std::vector<SortKey> sk;
  for (const ColumnPtr& kc : keys) { SortKey s; s.col = kc; s.nulls_last = true; sk.push_back(s); }
  ColumnPtr perm = sort_indices(sk, -1, sort_desc);      // stable: the head of a segment is its first occurrence, the tail its last
  Buf heads = segment_heads_of(keys, perm, n);
  {
    ProfileScope ps("distinct_keep", (uint64_t)n * 4 + (uint64_t)n / 4, (uint64_t)n);
    hipLaunchKernelGGL(distinct_keep_kernel, dim3(k::grid_for(n, kBlock * 4)), dim3(kBlock), 0, stream(), heads->as<uint64_t>(), perm->values->as<uint32_t>(), n, distinct::keep_served(keep),
                       out->values->as<unsigned int>());
    PLX_HIP(hipGetLastError());
  }
  if (kept) *kept = k::bitmap_popcount(out->values->as<uint64_t>(), n);
  return out;
}

HeadRanks segment_head_ranks(const std::vector<ColumnPtr>& keys, const ColumnPtr& perm) {
  PLX_REQUIRE(!keys.empty() && (int)keys.size() <= kSegmentMaxKeys, PLX_ERR_UNSUPPORTED, "sorted segments: 1.." + std::to_string(kSegmentMaxKeys) + " key columns, got " + std::to_string(keys.size()));
  const int64_t n = perm->len;
  PLX_REQUIRE(n > 0 && perm->dtype == PLX_U32 && !perm->validity, PLX_ERR_INVALID, "segment heads: a u32 permutation of at least one row");
  for (const ColumnPtr& kc : keys) PLX_REQUIRE(kc->len == n, PLX_ERR_SHAPE, "segment heads: key length mismatch");
  HeadRanks hr;
  const int64_t nwords = (n + 63) >> 6;
  hr.heads = segment_heads_of(keys, perm, n);
  hr.prefix = mask_rank_prefix(hr.heads, n);
  uint64_t total = 0;
  d2h_sync(&total, hr.prefix->as<uint64_t>() + nwords, 8);
  hr.n_segments = (int64_t)total;
  return hr;
}

}  // namespace sort
}  // namespace plx
