// kernels_cumulative.hip -- cum_sum / cum_min / cum_max / cum_count and rank on the device (the arithmetic: cumulative.hpp).
//
// Reference behaviour (restated, not ported): cum_* walk a column once and keep a running value, nulls staying null (polars-ops/src/series/ops/cum_agg.rs); rank
// sorts, then counts inside runs of ties (polars-ops/src/series/ops/rank.rs); under `.over` both run per group of the window.
//
// GPU shape of the cumulative functions: a SEGMENTED INCLUSIVE SCAN of (flag, value) pairs, reduce-then-scan, three launches and NO waiting between workgroups (no
// look-back, no flag another workgroup spins on):
//   1. cum_reduce_kernel : per tile of 2048 positions (256 lanes x 8) the tile's aggregate (has a head, value).
//   2. the scan of the tile aggregates under the same combine -- the same two kernels over the pair arrays: one workgroup while they fit one tile, recursive above.
//   3. cum_scan_kernel   : per tile the lanes fold their 8 positions, a wave64 scan of the lane aggregates with __shfl_up, the four wave totals through LDS, the
//      tile's carry-in (the scanned aggregate of the tile before it), then every position's result is stored.
// The price against a single-pass scan is one more read of the input.  An exclusive value is never derived by subtracting.
//   whole column (kPermuted = false): loads and stores are coalesced, 16 bytes per lane where the width allows; there is no head mask.
//   partitions   (kPermuted = true) : position i of the key-sorted order reads x[perm[i]], validity bit perm[i] and head bit i, and stores out[perm[i]].
// The output's validity IS the input's bitmap (cum_count has none), so no bitmap is scattered or read-modify-written.
//
// rank needs no scan: over sort_segments(keys, value) two head masks (segments, runs of ties), their per-word prefixes and their compacted starts give every sorted
// position its segment start and its run's start and end in O(1) (cumulative::run_of); the position writes out[perm[i]].  Positions of the trailing null run of a
// segment write nothing.
#include <algorithm>

#include "cumulative.hpp"
#include "dev.hpp"
#include "kernels.hpp"
#include "ops.hpp"
#include "sort.hpp"

namespace plx {
namespace cumulative {

using namespace dev;
using k::kBlock;
static_assert(kBlock == kThreads, "the scan's tile is kBlock lanes x kPerThread positions");

// ---- shuffles of a pair ----
template <class A> __device__ __forceinline__ A shfl_up_value(A v, int s) {
  if constexpr (sizeof(A) == 8) {
    uint64_t b;
    __builtin_memcpy(&b, &v, 8);
    uint32_t lo = __shfl_up((uint32_t)b, s, 64), hi = __shfl_up((uint32_t)(b >> 32), s, 64);
    b = ((uint64_t)hi << 32) | lo;
    A r;
    __builtin_memcpy(&r, &b, 8);
    return r;
  } else {
    uint32_t b;
    __builtin_memcpy(&b, &v, 4);
    b = __shfl_up(b, s, 64);
    A r;
    __builtin_memcpy(&r, &b, 4);
    return r;
  }
}
template <class A> __device__ __forceinline__ Pair<A> shfl_up_pair(const Pair<A>& p, int s) { return Pair<A>{shfl_up_value<A>(p.v, s), __shfl_up(p.f, s, 64)}; }

// inclusive scan of one pair per lane across the wave
template <int OP, class A> __device__ __forceinline__ Pair<A> wave_inclusive(Pair<A> t, int lane) {
#pragma unroll
  for (int s = 1; s < kWaveLanes; s <<= 1) t = wave_step<OP, A>(t, shfl_up_pair<A>(t, s), lane, s);
  return t;
}

// ---- sources and sinks of a tile's positions ----
// A column along the scan's order.  T: the stored type, A: the accumulator.  kCount: the value is 1 for a valid row and the column's values are never read.
template <class T, class A, int OP, bool kPermuted>
struct ColSrc {
  const T* x;
  const uint64_t* valid;      // null: no nulls
  const uint64_t* heads;      // kPermuted: the segment-head mask of the sorted order
  const uint32_t* perm;       // kPermuted: the sorted order
  int reverse;
  int vec;                    // x is 16-byte aligned (a borrowed column may not be): the vector loads are legal
  static constexpr bool kCount = OP == PLX_CUM_COUNT;
  __device__ __forceinline__ void load(int64_t base, int64_t n, Pair<A>* e) const {
    if constexpr (!kPermuted) {
      if (vec && !reverse && base + kPerThread <= n) {      // a full lane of a forward scan: vector loads, one validity byte (base is a multiple of 8)
        const unsigned vb = valid ? reinterpret_cast<const uint8_t*>(valid)[base >> 3] : 0xffu;
        if constexpr (kCount) {
#pragma unroll
          for (int j = 0; j < kPerThread; j++) e[j] = Pair<A>{(A)((vb >> j) & 1u), 0u};
        } else {
          constexpr int V = sizeof(T) >= 2 ? 16 / (int)sizeof(T) > kPerThread ? kPerThread : 16 / (int)sizeof(T) : kPerThread;
#pragma unroll
          for (int q = 0; q < kPerThread / V; q++) {
            const Pack<T, V> pk = load_pack<T, V>(x + base + q * V);
#pragma unroll
            for (int j = 0; j < V; j++) e[q * V + j] = Pair<A>{((vb >> (q * V + j)) & 1u) ? (A)pk.v[j] : identity<OP, A>(), 0u};
          }
        }
        return;
      }
    }
#pragma unroll
    for (int j = 0; j < kPerThread; j++) {
      const int64_t p = base + j;
      Pair<A> r = neutral<OP, A>();
      if (p < n) {
        const int64_t i = physical_index(p, n, reverse != 0);
        int64_t row = i;
        if constexpr (kPermuted) { row = (int64_t)perm[i]; r.f = flag_at(heads, i, n, reverse != 0) ? 1u : 0u; }
        if (row < n && (!valid || ((valid[row >> 6] >> (row & 63)) & 1))) {
          if constexpr (kCount) r.v = (A)1; else r.v = (A)x[row];
        }
      }
      e[j] = r;
    }
  }
};
template <class O, class A, bool kPermuted>
struct ColDst {
  O* out;
  const uint32_t* perm;
  int reverse;
  int vec;
  __device__ __forceinline__ void store(int64_t base, int64_t n, const Pair<A>* e) const {
    if constexpr (!kPermuted) {
      if (vec && !reverse && base + kPerThread <= n) {
        constexpr int V = sizeof(O) >= 2 ? 16 / (int)sizeof(O) > kPerThread ? kPerThread : 16 / (int)sizeof(O) : kPerThread;
#pragma unroll
        for (int q = 0; q < kPerThread / V; q++) {
          Pack<O, V> pk;
#pragma unroll
          for (int j = 0; j < V; j++) pk.v[j] = (O)e[q * V + j].v;
          store_pack<O, V>(out + base + q * V, pk);
        }
        return;
      }
    }
#pragma unroll
    for (int j = 0; j < kPerThread; j++) {
      const int64_t p = base + j;
      if (p >= n) continue;
      const int64_t i = physical_index(p, n, reverse != 0);
      int64_t row = i;
      if constexpr (kPermuted) row = (int64_t)perm[i];
      if (row < n) out[row] = (O)e[j].v;
    }
  }
};
// the tile aggregates of the level below: plain arrays of flags and values, scanned in place
template <class A, int OP>
struct PairSrc {
  const uint32_t* f;
  const A* v;
  __device__ __forceinline__ void load(int64_t base, int64_t n, Pair<A>* e) const {
#pragma unroll
    for (int j = 0; j < kPerThread; j++) { const int64_t p = base + j; e[j] = p < n ? Pair<A>{v[p], f[p]} : neutral<OP, A>(); }
  }
};
template <class A>
struct PairDst {
  uint32_t* f;
  A* v;
  __device__ __forceinline__ void store(int64_t base, int64_t n, const Pair<A>* e) const {
#pragma unroll
    for (int j = 0; j < kPerThread; j++) { const int64_t p = base + j; if (p < n) { v[p] = e[j].v; f[p] = e[j].f; } }
  }
};

// ---- launch 1: the aggregate of every tile ----
template <int OP, class A, class Src>
__global__ __launch_bounds__(kBlock) void cum_reduce_kernel(Src src, int64_t n, uint32_t* __restrict__ agg_f, A* __restrict__ agg_v) {
  __shared__ Pair<A> wave_tot[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n_tiles = (n + kTile - 1) / kTile;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    Pair<A> e[kPerThread];
    src.load(tile * kTile + (int64_t)threadIdx.x * kPerThread, n, e);
    const Pair<A> t = wave_inclusive<OP, A>(fold_thread<OP, A>(e), lane);
    if (lane == kWaveLanes - 1) wave_tot[wave] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
      const Pair<A> tot = fold_waves<OP, A>(wave_tot, kWaves);
      agg_f[tile] = tot.f;
      agg_v[tile] = tot.v;
    }
    __syncthreads();      // wave_tot is written again by the next tile of the stride loop
  }
}

// ---- launch 3 (and the scan of the aggregates themselves): every position of every tile ----
// carry_f / carry_v: the INCLUSIVE scan of the tile aggregates (tile t starts from entry t - 1); null: there is one tile
template <int OP, class A, class Src, class Dst>
__global__ __launch_bounds__(kBlock) void cum_scan_kernel(Src src, Dst dst, int64_t n, const uint32_t* __restrict__ carry_f, const A* __restrict__ carry_v) {
  __shared__ Pair<A> wave_tot[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n_tiles = (n + kTile - 1) / kTile;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t base = tile * kTile + (int64_t)threadIdx.x * kPerThread;
    Pair<A> e[kPerThread];
    src.load(base, n, e);
    const Pair<A> incl = wave_inclusive<OP, A>(fold_thread<OP, A>(e), lane);
    Pair<A> excl = shfl_up_pair<A>(incl, 1);      // what the lanes in front of this one hold together
    if (lane == 0) excl = neutral<OP, A>();
    if (lane == kWaveLanes - 1) wave_tot[wave] = incl;
    __syncthreads();
    Pair<A> carry = neutral<OP, A>();
    if (carry_f && tile > 0) carry = Pair<A>{carry_v[tile - 1], carry_f[tile - 1]};
    carry = combine<OP, A>(combine<OP, A>(carry, fold_waves<OP, A>(wave_tot, wave)), excl);
    scan_thread<OP, A>(carry, e);
    dst.store(base, n, e);
    __syncthreads();
  }
}

// ---- the host side of the scan ----
template <int OP, class A>
static void scan_pairs(uint32_t* f, A* v, int64_t m) {      // in place, inclusive
  const PairSrc<A, OP> src{f, v};
  const PairDst<A> dst{f, v};
  if (m <= kTile) {
    hipLaunchKernelGGL((cum_scan_kernel<OP, A, PairSrc<A, OP>, PairDst<A>>), dim3(1), dim3(kBlock), 0, stream(), src, dst, m, (const uint32_t*)nullptr, (const A*)nullptr);
    PLX_HIP(hipGetLastError());
    return;
  }
  const int64_t tiles = (m + kTile - 1) / kTile;
  Buf f1 = dev_alloc((size_t)tiles * 4), v1 = dev_alloc((size_t)tiles * sizeof(A));
  hipLaunchKernelGGL((cum_reduce_kernel<OP, A, PairSrc<A, OP>>), dim3(k::grid_for(m, kTile)), dim3(kBlock), 0, stream(), src, m, f1->as<uint32_t>(), v1->as<A>());
  PLX_HIP(hipGetLastError());
  scan_pairs<OP, A>(f1->as<uint32_t>(), v1->as<A>(), tiles);
  hipLaunchKernelGGL((cum_scan_kernel<OP, A, PairSrc<A, OP>, PairDst<A>>), dim3(k::grid_for(m, kTile)), dim3(kBlock), 0, stream(), src, dst, m, (const uint32_t*)f1->as<uint32_t>(), (const A*)v1->as<A>());
  PLX_HIP(hipGetLastError());
  PLX_HIP(hipStreamSynchronize(stream()));      // f1 / v1 live until the kernel that reads them is done
}

template <int OP, class T, class A, class O, bool kPermuted>
static void scan_typed(const ScanOrder& order, const void* x, const uint64_t* valid, void* out, int64_t n, bool reverse) {
  using Src = ColSrc<T, A, OP, kPermuted>;
  using Dst = ColDst<O, A, kPermuted>;
  const Src src{reinterpret_cast<const T*>(x), valid, kPermuted ? order.heads->as<uint64_t>() : nullptr, kPermuted ? order.perm->values->as<uint32_t>() : nullptr, reverse ? 1 : 0,
                (reinterpret_cast<uintptr_t>(x) & 15) == 0 ? 1 : 0};
  const Dst dst{reinterpret_cast<O*>(out), kPermuted ? order.perm->values->as<uint32_t>() : nullptr, reverse ? 1 : 0, (reinterpret_cast<uintptr_t>(out) & 15) == 0 ? 1 : 0};
  const int64_t tiles = (n + kTile - 1) / kTile;
  const int grid = k::grid_for(n, kTile);
  Buf af = dev_alloc((size_t)tiles * 4), av = dev_alloc((size_t)tiles * sizeof(A));
  const uint64_t w_in = OP == PLX_CUM_COUNT ? 0 : sizeof(T), extra = (valid ? 1 : 0) + (kPermuted ? 9 : 0);      // + validity bits, + perm twice and the head bit
  ProfileScope ps(kPermuted ? "cumulative_scan_sorted" : "cumulative_scan", (uint64_t)n * (2 * w_in + sizeof(O)) + (uint64_t)n * extra / 4, (uint64_t)n);
  hipLaunchKernelGGL((cum_reduce_kernel<OP, A, Src>), dim3(grid), dim3(kBlock), 0, stream(), src, n, af->as<uint32_t>(), av->as<A>());
  PLX_HIP(hipGetLastError());
  scan_pairs<OP, A>(af->as<uint32_t>(), av->as<A>(), tiles);
  hipLaunchKernelGGL((cum_scan_kernel<OP, A, Src, Dst>), dim3(grid), dim3(kBlock), 0, stream(), src, dst, n, (const uint32_t*)af->as<uint32_t>(), (const A*)av->as<A>());
  PLX_HIP(hipGetLastError());
  PLX_HIP(hipStreamSynchronize(stream()));      // the aggregates live until the kernel that reads them is done
}
template <int OP, class T, class A, class O>
static void scan_route(const ScanOrder& order, const void* x, const uint64_t* valid, void* out, int64_t n, bool reverse) {
  if (order.perm) scan_typed<OP, T, A, O, true>(order, x, valid, out, n, reverse);
  else scan_typed<OP, T, A, O, false>(order, x, valid, out, n, reverse);
}
// min / max keep the dtype; narrow integers ride in a 32-bit accumulator (a shuffle moves 32 bits)
template <int OP>
static void scan_minmax(const ScanOrder& order, int dtype, const void* x, const uint64_t* valid, void* out, int64_t n, bool reverse) {
  switch (dtype) {
    case PLX_I8: scan_route<OP, int8_t, int32_t, int8_t>(order, x, valid, out, n, reverse); break;
    case PLX_I16: scan_route<OP, int16_t, int32_t, int16_t>(order, x, valid, out, n, reverse); break;
    case PLX_I32: scan_route<OP, int32_t, int32_t, int32_t>(order, x, valid, out, n, reverse); break;
    case PLX_I64: scan_route<OP, int64_t, int64_t, int64_t>(order, x, valid, out, n, reverse); break;
    case PLX_U8: scan_route<OP, uint8_t, uint32_t, uint8_t>(order, x, valid, out, n, reverse); break;
    case PLX_U16: scan_route<OP, uint16_t, uint32_t, uint16_t>(order, x, valid, out, n, reverse); break;
    case PLX_U32: scan_route<OP, uint32_t, uint32_t, uint32_t>(order, x, valid, out, n, reverse); break;
    case PLX_U64: scan_route<OP, uint64_t, uint64_t, uint64_t>(order, x, valid, out, n, reverse); break;
    case PLX_F32: scan_route<OP, float, float, float>(order, x, valid, out, n, reverse); break;
    case PLX_F64: scan_route<OP, double, double, double>(order, x, valid, out, n, reverse); break;
    default: fail(PLX_ERR_UNSUPPORTED, std::string(op_name(OP)) + " of a " + dtype_name(dtype) + " column");
  }
}
// sum: the sum aggregate's dtypes; Float32 accumulates in f64 and rounds once per row, as that aggregate rounds once per group
static void scan_sum(const ScanOrder& order, int dtype, const void* x, const uint64_t* valid, void* out, int64_t n, bool reverse) {
  constexpr int OP = PLX_CUM_SUM;
  switch (dtype) {
    case PLX_I8: scan_route<OP, int8_t, int64_t, int64_t>(order, x, valid, out, n, reverse); break;
    case PLX_I16: scan_route<OP, int16_t, int64_t, int64_t>(order, x, valid, out, n, reverse); break;
    case PLX_I32: scan_route<OP, int32_t, int32_t, int32_t>(order, x, valid, out, n, reverse); break;
    case PLX_I64: scan_route<OP, int64_t, int64_t, int64_t>(order, x, valid, out, n, reverse); break;
    case PLX_U8: scan_route<OP, uint8_t, int64_t, int64_t>(order, x, valid, out, n, reverse); break;
    case PLX_U16: scan_route<OP, uint16_t, int64_t, int64_t>(order, x, valid, out, n, reverse); break;
    case PLX_U32: scan_route<OP, uint32_t, uint32_t, uint32_t>(order, x, valid, out, n, reverse); break;
    case PLX_U64: scan_route<OP, uint64_t, uint64_t, uint64_t>(order, x, valid, out, n, reverse); break;
    case PLX_F32: scan_route<OP, float, double, float>(order, x, valid, out, n, reverse); break;
    case PLX_F64: scan_route<OP, double, double, double>(order, x, valid, out, n, reverse); break;
    default: fail(PLX_ERR_UNSUPPORTED, std::string("cum_sum of a ") + dtype_name(dtype) + " column");
  }
}

ScanOrder scan_order(const std::vector<ColumnPtr>& keys, int64_t n) {
  PLX_REQUIRE((int)keys.size() <= sort::kSegmentMaxKeys, PLX_ERR_UNSUPPORTED, "cumulative: " + std::to_string(keys.size()) + " keys; a window takes 1.." + std::to_string(sort::kSegmentMaxKeys) + " keys on this path");
  PLX_REQUIRE(n < 0xffffffffll - 1, PLX_ERR_UNSUPPORTED, "cumulative: more rows than u32 IdxSize");
  ScanOrder o;
  o.n = n;
  for (const ColumnPtr& kc : keys) {
    PLX_REQUIRE(kc->len == n, PLX_ERR_SHAPE, "cumulative: key columns have different lengths");
    PLX_REQUIRE(kc->values || n == 0, PLX_ERR_INVALID, "placeholder column has no data");
  }
  if (n == 0) { o.desc = "cumulative[empty]"; return o; }
  if (keys.empty()) { o.desc = "cumulative[whole column]"; return o; }
  std::vector<sort::SortKey> sk;
  for (const ColumnPtr& kc : keys) { sort::SortKey s; s.col = kc; s.nulls_last = true; sk.push_back(s); }
  std::string sd;
  o.perm = sort::sort_indices(sk, -1, &sd);      // stable: the rows of a partition stay in row order
  o.heads = sort::segment_head_ranks(keys, o.perm).heads;
  o.desc = "cumulative[sorted rows: " + sd + "]";
  return o;
}

ColumnPtr scan_column(const ScanOrder& order, const ColumnPtr& value, int op, bool reverse) {
  PLX_REQUIRE(op_ok(op), PLX_ERR_INVALID, "cumulative: op " + std::to_string(op) + " is no plx_cum_op (0 = sum, 1 = min, 2 = max, 3 = count)");
  const int64_t n = value->len;
  PLX_REQUIRE(n == order.n, PLX_ERR_SHAPE, "cumulative: a value column of " + std::to_string(n) + " rows for an order of " + std::to_string(order.n));
  PLX_REQUIRE(value->values || n == 0, PLX_ERR_INVALID, "placeholder column has no data");
  const int out_dt = op == PLX_CUM_COUNT ? PLX_U32 : result_dtype(op, value->dtype);
  if (out_dt < 0) fail(PLX_ERR_UNSUPPORTED, std::string(op_name(op)) + " of a " + dtype_name(value->dtype) + " column: integer, float and Boolean columns only");
  auto out = std::make_shared<Column>();
  out->dtype = out_dt; out->len = n;
  out->values = dev_alloc(values_bytes(out_dt, std::max<int64_t>(n, 1)) + 8);
  if (op == PLX_CUM_COUNT) out->null_count = 0;
  else { out->validity = value->validity; out->null_count = value->validity ? value->null_count : 0; }      // the input's bitmap, shared
  if (n == 0) return out;
  const uint64_t* valid = value->valid_words();
  if (op == PLX_CUM_COUNT) {
    scan_route<PLX_CUM_COUNT, uint32_t, uint32_t, uint32_t>(order, nullptr, valid, out->values->ptr, n, reverse);
    return out;
  }
  // a Boolean column is widened first (cum_sum: to its UInt32 result dtype; cum_min / cum_max: to bytes, the result narrowed back to bits)
  const void* x = value->data();
  int dt = value->dtype;
  Buf wide, narrow;
  if (dt == PLX_BOOL) {
    dt = op == PLX_CUM_SUM ? PLX_U32 : PLX_U8;
    wide = dev_alloc((size_t)n * dtype_width(dt) + 16);
    k::cast_from_bool(value->values->as<uint64_t>(), dt, n, wide->ptr);
    x = wide->ptr;
  }
  void* dst = out->values->ptr;
  if (value->dtype == PLX_BOOL && op != PLX_CUM_SUM) { narrow = dev_alloc((size_t)n + 16); dst = narrow->ptr; }
  switch (op) {
    case PLX_CUM_SUM: scan_sum(order, dt, x, valid, dst, n, reverse); break;
    case PLX_CUM_MIN: scan_minmax<PLX_CUM_MIN>(order, dt, x, valid, dst, n, reverse); break;
    default: scan_minmax<PLX_CUM_MAX>(order, dt, x, valid, dst, n, reverse); break;
  }
  if (narrow) {
    plx_scalar zero; zero.u = 0;
    k::cmp(PLX_U8, PLX_NE, narrow->ptr, nullptr, zero, n, out->values->as<uint64_t>());
    PLX_HIP(hipStreamSynchronize(stream()));
  }
  return out;
}

// ---- rank ----
struct RankArgs {
  const uint32_t* perm;
  const uint64_t* valid;       // of the ranked column; null: no nulls
  const uint64_t *seg_heads, *seg_prefix, *run_heads, *run_prefix;
  const uint32_t *seg_starts, *run_starts;
  int64_t n, n_segs, n_runs;
  int method;
};
__global__ __launch_bounds__(kBlock) void rank_kernel(RankArgs a, void* __restrict__ out, unsigned int* __restrict__ flag) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = (int64_t)a.perm[i];
    if (row >= a.n) { *flag = 1u; continue; }
    if (a.valid && !((a.valid[row >> 6] >> (row & 63)) & 1)) continue;      // the trailing null run of a segment: nothing is written, the validity says so
    const RunOf seg = run_of(a.seg_prefix, a.seg_heads, a.seg_starts, (uint64_t)a.n_segs, (uint64_t)a.n, (uint64_t)i);
    const RunOf run = run_of(a.run_prefix, a.run_heads, a.run_starts, (uint64_t)a.n_runs, (uint64_t)a.n, (uint64_t)i);
    if (!seg.ok || !run.ok || run.start < seg.start) { *flag = 1u; continue; }
    if (a.method == PLX_RANK_AVERAGE) reinterpret_cast<double*>(out)[row] = rank_average(seg.start, run.start, run.end);
    else {
      const uint64_t first = a.method == PLX_RANK_DENSE ? distinct::rank_before(a.run_prefix, a.run_heads, seg.start + 1) : 0;
      reinterpret_cast<uint32_t*>(out)[row] = rank_value(a.method, (uint64_t)i, seg.start, run.start, run.end, run.rank, first);
    }
  }
}

RankOrder rank_order(const std::vector<ColumnPtr>& keys, const ColumnPtr& value, bool descending) {
  PLX_REQUIRE((int)keys.size() <= sort::kSegmentMaxKeys, PLX_ERR_UNSUPPORTED, "rank: " + std::to_string(keys.size()) + " keys; a window takes 1.." + std::to_string(sort::kSegmentMaxKeys) + " keys on this path");
  const int64_t n = value->len;
  PLX_REQUIRE(n < 0xffffffffll - 1, PLX_ERR_UNSUPPORTED, "rank: more rows than u32 IdxSize");
  if (!(dtype_is_int(value->dtype) || dtype_is_float(value->dtype) || value->dtype == PLX_BOOL)) fail(PLX_ERR_UNSUPPORTED, std::string("rank of a ") + dtype_name(value->dtype) + " column: integer, float and Boolean columns only");
  PLX_REQUIRE(value->values || n == 0, PLX_ERR_INVALID, "placeholder column has no data");
  for (const ColumnPtr& kc : keys) {
    PLX_REQUIRE(kc->len == n, PLX_ERR_SHAPE, "rank: key columns have different lengths");
    PLX_REQUIRE(kc->values || n == 0, PLX_ERR_INVALID, "placeholder column has no data");
  }
  RankOrder o;
  if (n == 0) { o.seg.value = value; o.desc = "rank[empty]"; return o; }
  o.seg = sort::sort_segments(keys, value, -1, descending);
  o.seg_prefix = sort::mask_rank_prefix(o.seg.heads, n);
  o.runs = sort::value_runs(o.seg);
  o.desc = "rank[sorted segments: " + o.seg.sort_desc + "]";
  return o;
}

ColumnPtr rank_column(const RankOrder& order, int method) {
  PLX_REQUIRE(method_ok(method), PLX_ERR_INVALID, "rank: method " + std::to_string(method) + " is no plx_rank_method (0 = average, 1 = min, 2 = max, 3 = dense, 4 = ordinal)");
  const ColumnPtr& value = order.seg.value;
  const int64_t n = value->len;
  auto out = std::make_shared<Column>();
  out->dtype = rank_dtype(method); out->len = n;
  out->values = dev_alloc(values_bytes(out->dtype, std::max<int64_t>(n, 1)) + 8);
  out->validity = value->validity; out->null_count = value->validity ? value->null_count : 0;
  if (n == 0) return out;
  if (value->validity) PLX_HIP(hipMemsetAsync(out->values->ptr, 0, (size_t)n * dtype_width(out->dtype), stream()));      // null rows are never written: they read as 0 under their cleared bit
  RankArgs a{};
  a.perm = order.seg.perm->values->as<uint32_t>(); a.valid = value->valid_words();
  a.seg_heads = order.seg.heads->as<uint64_t>(); a.seg_prefix = order.seg_prefix->as<uint64_t>(); a.seg_starts = order.seg.starts->as<uint32_t>();
  a.run_heads = order.runs.heads->as<uint64_t>(); a.run_prefix = order.runs.prefix->as<uint64_t>(); a.run_starts = order.runs.starts->as<uint32_t>();
  a.n = n; a.n_segs = order.seg.n_groups; a.n_runs = order.runs.n_runs; a.method = method;
  Buf flag = dev_alloc_zero(8);
  {
    ProfileScope ps("rank", (uint64_t)n * (4 + dtype_width(out->dtype)) + (uint64_t)n, (uint64_t)n);
    hipLaunchKernelGGL(rank_kernel, dim3(k::grid_for(n, kBlock * 4)), dim3(kBlock), 0, stream(), a, out->values->ptr, flag->as<unsigned int>());
    PLX_HIP(hipGetLastError());
  }
  unsigned int bad = 0;
  d2h_sync(&bad, flag->ptr, 4);
  PLX_REQUIRE(!bad, PLX_ERR_INVALID, "rank: a sorted position without a segment or a run (an inconsistent sorted order)");
  return out;
}

}  // namespace cumulative
}  // namespace plx
