// kernels_rolling.hip -- shift / diff and rolling_sum / rolling_mean / rolling_min / rolling_max on the device (the arithmetic: rolling.hpp).
//
// Reference behaviour (restated, not ported): shift moves a column by n rows and leaves nulls (or a fill value) behind, diff subtracts the row n before
// (polars-ops/src/series/ops/diff.rs); the fixed-window rolling functions walk a window of w rows over the column, null below min_samples non-null values
// (polars-compute/src/rolling); under `.over` all of them run per group of the window, in the frame's row order.
//
// The order and the segment bounds are those of the cumulative functions: the rows themselves (whole column: bounds 0 and n, no mask read), or the stable key-sorted
// order of cumulative::scan_order, where the segment holding sorted position i comes from cumulative::run_of on the head mask, its per-word prefix and its compacted
// starts -- the way rank_kernel finds it.  Position i reads x[perm[i]] and writes out[perm[i]].
//
// shift / diff: ONE launch.  Whole column: a copy at an offset, 16 bytes per lane where source and destination are both aligned, and the lane that owns bit 0 of a
// validity word writes that word: the input's bitmap shifted by n bits (a funnel shift of two words), fill bits set for fill_value, ANDed with the input's word for diff.
//
// rolling: the two-scan identity of rolling.hpp, never a difference of prefixes.
//   tile halo (w <= kMaxWindow): ONE launch.  A workgroup loads its tile of outputs plus the w - 1 halo positions once (12 consecutive positions per lane), scans
//     them forward and backward in registers (lane fold, __shfl_up / __shfl_down wave scan, four wave totals through LDS), keeps the P of the tile's window ends and
//     the S of its window starts in LDS, then every lane combines and stores its 8 consecutive outputs.  Both scans lie inside the region: a block start is at most
//     w - 1 positions before a window's end, so no workgroup carries anything to another.
//   two scans (any w): the three-launch segmented scan (tile aggregates, their scan, the tiles with their carry) forward and mirrored, under the combined restart
//     flags, leaves P and S in memory; one combine launch reads S[a] and P[b] per row.
// The result's validity is a new bitmap.  Whole column: a lane owns 8 consecutive outputs and stores whole bytes.  Under the permutation the rows of one bitmap word
// belong to lanes anywhere in the grid, so valid rows atomicOr their bit into zeroed words: one launch and no byte-per-row staging buffer, and the atomics go to L2
// lines the scattered value stores touch anyway.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "dev.hpp"
#include "kernels.hpp"
#include "ops.hpp"
#include "rolling.hpp"
#include "sort.hpp"

namespace plx {
namespace rolling {

using namespace dev;
using cumulative::ScanOrder;
using k::kBlock;
static_assert(kBlock == kThreads, "a workgroup is kBlock lanes");

// ---- values by runtime dtype: the kernels are instantiated per (op, accumulator), not per column dtype ----
template <class A> __device__ __forceinline__ A load_as(const void* x, int dt, int64_t row) {
  switch (dt) {
    case PLX_I8: return (A) reinterpret_cast<const int8_t*>(x)[row];
    case PLX_I16: return (A) reinterpret_cast<const int16_t*>(x)[row];
    case PLX_I32: return (A) reinterpret_cast<const int32_t*>(x)[row];
    case PLX_I64: return (A) reinterpret_cast<const int64_t*>(x)[row];
    case PLX_U8: return (A) reinterpret_cast<const uint8_t*>(x)[row];
    case PLX_U16: return (A) reinterpret_cast<const uint16_t*>(x)[row];
    case PLX_U32: return (A) reinterpret_cast<const uint32_t*>(x)[row];
    case PLX_U64: return (A) reinterpret_cast<const uint64_t*>(x)[row];
    case PLX_F32: return (A) reinterpret_cast<const float*>(x)[row];
    default: return (A) reinterpret_cast<const double*>(x)[row];
  }
}
template <class A> __device__ __forceinline__ void store_as(void* out, int dt, int64_t row, A v) {
  switch (dt) {
    case PLX_I8: reinterpret_cast<int8_t*>(out)[row] = (int8_t)v; break;
    case PLX_I16: reinterpret_cast<int16_t*>(out)[row] = (int16_t)v; break;
    case PLX_I32: reinterpret_cast<int32_t*>(out)[row] = (int32_t)v; break;
    case PLX_I64: reinterpret_cast<int64_t*>(out)[row] = (int64_t)v; break;
    case PLX_U8: reinterpret_cast<uint8_t*>(out)[row] = (uint8_t)v; break;
    case PLX_U16: reinterpret_cast<uint16_t*>(out)[row] = (uint16_t)v; break;
    case PLX_U32: reinterpret_cast<uint32_t*>(out)[row] = (uint32_t)v; break;
    case PLX_U64: reinterpret_cast<uint64_t*>(out)[row] = (uint64_t)v; break;
    case PLX_F32: reinterpret_cast<float*>(out)[row] = (float)v; break;
    default: reinterpret_cast<double*>(out)[row] = (double)v; break;
  }
}
__device__ __forceinline__ bool bit_at(const uint64_t* m, int64_t i) { return (m[i >> 6] >> (i & 63)) & 1; }

// ---- the segment of a position ----
struct SegArgs {
  const uint32_t* perm;         // null: the whole column, bounds 0 and n
  const uint64_t *heads, *prefix;
  const uint32_t* starts;
  int64_t n_segs;
};
__device__ __forceinline__ bool segment_of(const SegArgs& g, int64_t n, int64_t i, int64_t* s0, int64_t* s1) {
  if (!g.perm) { *s0 = 0; *s1 = n; return true; }
  const cumulative::RunOf r = cumulative::run_of(g.prefix, g.heads, g.starts, (uint64_t)g.n_segs, (uint64_t)n, (uint64_t)i);
  if (!r.ok) { *s0 = i; *s1 = i + 1; return false; }
  *s0 = (int64_t)r.start; *s1 = (int64_t)r.end;
  return true;
}

// ============================================================ shift / diff ====
template <class T, class O>
struct ShiftArgs {
  const T* x;
  const uint64_t* valid;        // null: no nulls
  O* out;
  uint64_t* out_valid;          // null: the result has no nulls; zeroed before the launch
  SegArgs seg;
  int64_t n, shift;
  O fill;
  int has_fill, vec;
  unsigned int* flag;
};
template <class T, class O, bool DIFF>
__global__ __launch_bounds__(kBlock) void shift_kernel(ShiftArgs<T, O> a) {
  constexpr int V = 16 / (int)sizeof(T);
  const int64_t n = a.n, gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gsize = (int64_t)gridDim.x * blockDim.x;
  if (!a.seg.perm) {
    const int64_t chunks = (n + V - 1) / V;
    for (int64_t c = gtid; c < chunks; c += gsize) {
      const int64_t base = c * V;
      if (a.out_valid && (base & 63) == 0) {
        uint64_t word = shifted_word(a.valid, n, base >> 6, a.shift, a.has_fill != 0);
        if constexpr (DIFF) word &= clean_word(a.valid, n, base >> 6);
        a.out_valid[base >> 6] = word;
      }
      if constexpr (!DIFF) {
        if (a.vec && a.shift % V == 0 && base - a.shift >= 0 && base + V - a.shift <= n && base + V <= n) {
          store_pack<O, V>(a.out + base, load_pack<O, V>(reinterpret_cast<const O*>(a.x) + (base - a.shift)));
          continue;
        }
      }
#pragma unroll
      for (int j = 0; j < V; j++) {
        const int64_t i = base + j;
        if (i >= n) break;
        int64_t src;
        const bool in = shift_source(i, a.shift, 0, n, &src);
        if constexpr (DIFF) a.out[i] = in ? diff_value<O, T>(a.x[i], a.x[src]) : (O)0;
        else a.out[i] = in ? (O)a.x[src] : a.fill;
      }
    }
    return;
  }
  for (int64_t i = gtid; i < n; i += gsize) {
    const int64_t row = (int64_t)a.seg.perm[i];
    int64_t s0, s1, src;
    if (row >= n || !segment_of(a.seg, n, i, &s0, &s1)) { *a.flag = 1u; continue; }
    const bool in = shift_source(i, a.shift, s0, s1, &src);
    const int64_t srow = in ? (int64_t)a.seg.perm[src] : row;
    if (srow >= n) { *a.flag = 1u; continue; }
    bool ok = in ? (!a.valid || bit_at(a.valid, srow)) : a.has_fill != 0;
    if constexpr (DIFF) {
      ok = ok && (!a.valid || bit_at(a.valid, row));
      a.out[row] = in ? diff_value<O, T>(a.x[row], a.x[srow]) : (O)0;
    } else {
      a.out[row] = in ? (O)a.x[srow] : a.fill;
    }
    if (a.out_valid && ok) atomicOr(reinterpret_cast<unsigned long long*>(a.out_valid) + (row >> 6), 1ull << (row & 63));
  }
}

template <class T, class O, bool DIFF>
static void shift_typed(const ScanOrder& order, const Segments& segs, const void* x, const uint64_t* valid, void* out, uint64_t* out_valid, int64_t n, int64_t shift, const plx_scalar* fill) {
  ShiftArgs<T, O> a{};
  a.x = reinterpret_cast<const T*>(x); a.valid = valid; a.out = reinterpret_cast<O*>(out); a.out_valid = out_valid;
  a.seg = SegArgs{nullptr, nullptr, nullptr, nullptr, 0};
  if (order.perm) a.seg = SegArgs{order.perm->values->as<uint32_t>(), order.heads->as<uint64_t>(), segs.prefix->as<uint64_t>(), segs.starts->as<uint32_t>(), segs.n_segments};
  a.n = n; a.shift = shift;
  a.fill = (O)0; a.has_fill = fill ? 1 : 0;
  if (fill) std::memcpy(&a.fill, fill, sizeof(O));      // (little endian: the low bytes of the 64-bit scalar)
  a.vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0 ? 1 : 0;
  Buf flag = dev_alloc_zero(8);
  a.flag = flag->as<unsigned int>();
  {
    ProfileScope ps(order.perm ? "shift_sorted" : "shift", (uint64_t)n * (sizeof(T) * (DIFF ? 2 : 1) + sizeof(O)) + (uint64_t)n / 4 + (order.perm ? (uint64_t)n * 8 : 0), (uint64_t)n);
    const int64_t items = order.perm ? n : (n + 16 / (int64_t)sizeof(T) - 1) / (16 / (int64_t)sizeof(T));
    hipLaunchKernelGGL((shift_kernel<T, O, DIFF>), dim3(k::grid_for(items, kBlock * 4)), dim3(kBlock), 0, stream(), a);
    PLX_HIP(hipGetLastError());
  }
  unsigned int bad = 0;
  d2h_sync(&bad, flag->ptr, 4);
  PLX_REQUIRE(!bad, PLX_ERR_INVALID, "shift: a sorted position without a segment (an inconsistent sorted order)");
}

Segments segments_of(const ScanOrder& order) {
  Segments s;
  if (!order.perm || order.n == 0) return s;
  const int64_t n = order.n;
  s.prefix = sort::mask_rank_prefix(order.heads, n);
  k::FilterPlan fp = k::filter_prepare(order.heads->as<uint64_t>(), n);
  s.n_segments = fp.n_out;
  Buf iota = dev_alloc((size_t)n * 4);
  k::fill_iota_u32(iota->as<uint32_t>(), n);
  s.starts = dev_alloc((size_t)std::max<int64_t>(s.n_segments, 1) * 4);
  k::filter_apply(fp, 4, iota->ptr, nullptr, s.starts->ptr, nullptr);
  PLX_HIP(hipStreamSynchronize(stream()));      // iota lives until the compaction is done
  return s;
}

static void check_order(const char* what, const ScanOrder& order, const Segments& segs, const ColumnPtr& value) {
  const int64_t n = value->len;
  PLX_REQUIRE(n == order.n, PLX_ERR_SHAPE, std::string(what) + ": a value column of " + std::to_string(n) + " rows for an order of " + std::to_string(order.n));
  PLX_REQUIRE(n < 0xffffffffll - 1, PLX_ERR_UNSUPPORTED, std::string(what) + ": more rows than u32 IdxSize");
  PLX_REQUIRE(value->values || n == 0, PLX_ERR_INVALID, "placeholder column has no data");
  PLX_REQUIRE(!order.perm || n == 0 || (order.heads && segs.prefix && segs.starts && segs.n_segments >= 1), PLX_ERR_INVALID, std::string(what) + ": a sorted order without its segments");
}

ColumnPtr shift_column(const ScanOrder& order, const Segments& segs, const ColumnPtr& value, int64_t shift, const plx_scalar* fill, bool diff) {
  const char* what = diff ? "diff" : "shift";
  check_order(what, order, segs, value);
  const int64_t n = value->len;
  const int in_dt = value->dtype;
  const int out_dt = diff ? diff_dtype(in_dt) : (in_dt >= PLX_BOOL && in_dt <= PLX_F64 ? in_dt : -1);
  if (out_dt < 0) fail(PLX_ERR_UNSUPPORTED, std::string(what) + " of a " + dtype_name(in_dt) + " column: " + (diff ? "integer and float columns only" : "integer, float and Boolean columns only"));
  PLX_REQUIRE(!(diff && fill), PLX_ERR_INVALID, "diff: fill must be NULL (a fill value belongs to shift)");
  shift = std::max<int64_t>(-n, std::min<int64_t>(n, shift));      // |n| >= the rows vacates every row: the same result, and i - n cannot overflow
  if (!diff && shift == 0) return value;                           // shift(0) is the operand itself
  auto out = std::make_shared<Column>();
  out->dtype = out_dt; out->len = n;
  out->values = out_dt == PLX_BOOL ? dev_alloc_zero(bitmap_bytes(std::max<int64_t>(n, 1))) : dev_alloc(values_bytes(out_dt, std::max<int64_t>(n, 1)) + 16);
  const bool nullable = value->validity || (shift != 0 && !fill);
  if (nullable) { out->validity = dev_alloc_zero(bitmap_bytes(std::max<int64_t>(n, 1))); out->null_count = -1; } else out->null_count = 0;
  if (n == 0) { out->null_count = 0; return out; }
  const uint64_t* valid = value->valid_words();
  uint64_t* ov = nullable ? out->validity->as<uint64_t>() : nullptr;
  // a Boolean column travels as bytes: widened, shifted, narrowed back to bits
  const void* x = value->data();
  void* dst = out->values->ptr;
  Buf wide, narrow;
  int dt = in_dt;
  if (in_dt == PLX_BOOL) {
    dt = PLX_U8;
    wide = dev_alloc((size_t)n + 16); narrow = dev_alloc((size_t)n + 16);
    k::cast_from_bool(value->values->as<uint64_t>(), PLX_U8, n, wide->ptr);
    x = wide->ptr; dst = narrow->ptr;
  }
  plx_scalar f; f.u = 0;
  if (fill) f = *fill;
  if (in_dt == PLX_BOOL && fill) f.u = fill->u & 1;
  const plx_scalar* fp = fill ? &f : nullptr;
  if (!diff) {
    switch (dtype_width(dt)) {
      case 1: shift_typed<uint8_t, uint8_t, false>(order, segs, x, valid, dst, ov, n, shift, fp); break;
      case 2: shift_typed<uint16_t, uint16_t, false>(order, segs, x, valid, dst, ov, n, shift, fp); break;
      case 4: shift_typed<uint32_t, uint32_t, false>(order, segs, x, valid, dst, ov, n, shift, fp); break;
      default: shift_typed<uint64_t, uint64_t, false>(order, segs, x, valid, dst, ov, n, shift, fp); break;
    }
  } else {
    switch (dt) {
      case PLX_I8: shift_typed<int8_t, int8_t, true>(order, segs, x, valid, dst, ov, n, shift, nullptr); break;
      case PLX_I16: shift_typed<int16_t, int16_t, true>(order, segs, x, valid, dst, ov, n, shift, nullptr); break;
      case PLX_I32: shift_typed<int32_t, int32_t, true>(order, segs, x, valid, dst, ov, n, shift, nullptr); break;
      case PLX_I64: shift_typed<int64_t, int64_t, true>(order, segs, x, valid, dst, ov, n, shift, nullptr); break;
      case PLX_U8: shift_typed<uint8_t, int16_t, true>(order, segs, x, valid, dst, ov, n, shift, nullptr); break;
      case PLX_U16: shift_typed<uint16_t, int32_t, true>(order, segs, x, valid, dst, ov, n, shift, nullptr); break;
      case PLX_U32: shift_typed<uint32_t, int64_t, true>(order, segs, x, valid, dst, ov, n, shift, nullptr); break;
      case PLX_U64: shift_typed<uint64_t, int64_t, true>(order, segs, x, valid, dst, ov, n, shift, nullptr); break;
      case PLX_F32: shift_typed<float, float, true>(order, segs, x, valid, dst, ov, n, shift, nullptr); break;
      default: shift_typed<double, double, true>(order, segs, x, valid, dst, ov, n, shift, nullptr); break;
    }
  }
  if (narrow) {
    plx_scalar zero; zero.u = 0;
    k::cmp(PLX_U8, PLX_NE, narrow->ptr, nullptr, zero, n, out->values->as<uint64_t>());
    PLX_HIP(hipStreamSynchronize(stream()));
  }
  return out;
}

// ================================================================ rolling ====
struct Src {
  const void* x;
  int dt;
  const uint64_t* valid;        // null: no nulls
  const uint64_t* heads;        // null: the whole column
  const uint32_t* perm;
  int64_t n, w;
};
struct Dst {
  void* out;
  int out_dt;
  uint64_t* out_valid;          // zeroed before the launch
  SegArgs seg;
  uint32_t min_samples;
  int mean;
  unsigned int* flag;
};
// the element at position pos of the scanned order; f bit 0: the forward scan restarts here, bit 1: the backward scan does
template <int OP, class A> __device__ __forceinline__ Elem<A> elem_at(const Src& s, int64_t pos) {
  Elem<A> e = neutral<OP, A>();
  const int64_t row = s.perm ? (int64_t)s.perm[pos] : pos;
  if (row < s.n && (!s.valid || bit_at(s.valid, row))) { e.v = load_as<A>(s.x, s.dt, row); e.c = 1u; }
  const bool head = s.heads ? bit_at(s.heads, pos) : pos == 0;
  const bool next_head = s.heads && pos + 1 < s.n && bit_at(s.heads, pos + 1);
  e.f = (forward_flag(pos, s.w, head) ? 1u : 0u) | (backward_flag(pos, s.n, s.w, next_head) ? 2u : 0u);
  return e;
}

// ---- shuffles of an element ----
template <bool DOWN> __device__ __forceinline__ uint32_t shfl32(uint32_t v, int s) { return DOWN ? __shfl_down(v, s, 64) : __shfl_up(v, s, 64); }
template <class A, bool DOWN> __device__ __forceinline__ A shfl_value(A v, int s) {
  if constexpr (sizeof(A) == 8) {
    uint64_t b;
    __builtin_memcpy(&b, &v, 8);
    const uint32_t lo = shfl32<DOWN>((uint32_t)b, s), hi = shfl32<DOWN>((uint32_t)(b >> 32), s);
    b = ((uint64_t)hi << 32) | lo;
    A r;
    __builtin_memcpy(&r, &b, 8);
    return r;
  } else {
    uint32_t b;
    __builtin_memcpy(&b, &v, 4);
    b = shfl32<DOWN>(b, s);
    A r;
    __builtin_memcpy(&r, &b, 4);
    return r;
  }
}
template <class A, bool DOWN> __device__ __forceinline__ Elem<A> shfl_elem(const Elem<A>& e, int s) { return Elem<A>{shfl_value<A, DOWN>(e.v, s), shfl32<DOWN>(e.c, s), shfl32<DOWN>(e.f, s)}; }

// the workgroup's inclusive scan of N consecutive positions per lane, in place; REV: from the last position to the first.  Returns what precedes the workgroup's
// positions combined with them all (carry (+) total).  Every lane of the workgroup calls it
template <int OP, class A, int N, bool REV>
__device__ __forceinline__ Elem<A> block_scan(Elem<A>* e, const Elem<A>& carry_in, Elem<A>* wave_tot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Elem<A> incl = fold_thread<OP, A, N, REV>(e);
#pragma unroll
  for (int s = 1; s < kWaveLanes; s <<= 1) incl = wave_step<OP, A, REV>(incl, shfl_elem<A, REV>(incl, s), lane, s);
  Elem<A> excl = shfl_elem<A, REV>(incl, 1);
  if (lane == (REV ? kWaveLanes - 1 : 0)) excl = neutral<OP, A>();
  if (lane == (REV ? 0 : kWaveLanes - 1)) wave_tot[wave] = incl;
  __syncthreads();
  const Elem<A> carry = combine<OP, A>(combine<OP, A>(carry_in, fold_waves<OP, A, REV>(wave_tot, wave)), excl);
  const Elem<A> total = combine<OP, A>(carry_in, fold_waves<OP, A, REV>(wave_tot, REV ? -1 : kWaves));
  scan_thread<OP, A, N, REV>(carry, e);
  __syncthreads();      // wave_tot is written again by the next scan
  return total;
}

// ---- one row's window from S[a] and P[b], and the 8 consecutive outputs of a lane ----
template <int OP, class A, class Lookup>
__device__ __forceinline__ void emit_outputs(const Dst& d, const Lookup& look, int64_t base, int64_t n, int64_t w, int64_t h) {
  unsigned bits = 0;
#pragma unroll 1
  for (int j = 0; j < kOutPerThread; j++) {
    const int64_t i = base + j;
    if (i >= n) break;
    const int64_t row = d.seg.perm ? (int64_t)d.seg.perm[i] : i;
    int64_t s0, s1;
    if (row >= n || !segment_of(d.seg, n, i, &s0, &s1)) { *d.flag = 1u; continue; }
    const Window win = window_of(i, s0, s1, w, h);
    Elem<A> r;
    if (win.use == (kUseP | kUseS)) r = join<OP, A>(look.S(win.a), look.P(win.b));
    else if (win.use == kUseP) r = look.P(win.b);
    else r = look.S(win.a);
    const bool ok = r.c >= d.min_samples;
    if (d.mean) store_as<double>(d.out, d.out_dt, row, ok ? (double)r.v / (double)r.c : 0.0);
    else store_as<A>(d.out, d.out_dt, row, ok ? r.v : (A)0);
    if (ok) {
      if (d.seg.perm) atomicOr(reinterpret_cast<unsigned long long*>(d.out_valid) + (row >> 6), 1ull << (row & 63));
      else bits |= 1u << j;
    }
  }
  if (!d.seg.perm && base < n) reinterpret_cast<uint8_t*>(d.out_valid)[base >> 3] = (uint8_t)bits;      // base is a multiple of 8: the lane owns the byte
}

// ---- the tile-halo route ----
template <class A> struct LdsLookup {
  const A* v;
  const uint32_t* c;
  int64_t t0, w, h;
  __device__ __forceinline__ Elem<A> S(int64_t pos) const { const int k = s_slot(pos, t0, w, h); return Elem<A>{v[k < 0 ? 0 : k], c[k < 0 ? 0 : k], 0u}; }
  __device__ __forceinline__ Elem<A> P(int64_t pos) const { const int k = p_slot(pos, t0, w, h); return Elem<A>{v[k < 0 ? 0 : k], c[k < 0 ? 0 : k], 0u}; }
};
template <int OP, class A>
__global__ __launch_bounds__(kBlock) void rolling_tile_kernel(Src s, Dst d, int64_t h) {
  __shared__ A lds_v[kLdsEntries];
  __shared__ uint32_t lds_c[kLdsEntries];
  __shared__ Elem<A> wave_tot[kWaves];
  const int64_t n = s.n, w = s.w;
  const int T = tile_rows(w);
  const int region_n = T + (int)w - 1;
  const int64_t n_tiles = (n + T - 1) / T;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t t0 = tile * T, r0 = region_start(t0, w, h);
    Elem<A> e[kRegionPerThread], sc[kRegionPerThread];
#pragma unroll
    for (int j = 0; j < kRegionPerThread; j++) {
      const int rp = (int)threadIdx.x * kRegionPerThread + j;
      const int64_t pos = r0 + rp;
      e[j] = (rp < region_n && pos >= 0 && pos < n) ? elem_at<OP, A>(s, pos) : neutral<OP, A>();
    }
#pragma unroll
    for (int j = 0; j < kRegionPerThread; j++) { sc[j] = e[j]; sc[j].f = e[j].f & 1u; }
    block_scan<OP, A, kRegionPerThread, false>(sc, neutral<OP, A>(), wave_tot);
#pragma unroll
    for (int j = 0; j < kRegionPerThread; j++) {
      const int rp = (int)threadIdx.x * kRegionPerThread + j;
      const int slot = rp < region_n ? p_slot(r0 + rp, t0, w, h) : -1;
      if (slot >= 0 && slot < kLdsEntries) { lds_v[slot] = sc[j].v; lds_c[slot] = sc[j].c; }
    }
#pragma unroll
    for (int j = 0; j < kRegionPerThread; j++) { sc[j] = e[j]; sc[j].f = (e[j].f >> 1) & 1u; }
    block_scan<OP, A, kRegionPerThread, true>(sc, neutral<OP, A>(), wave_tot);
#pragma unroll
    for (int j = 0; j < kRegionPerThread; j++) {
      const int rp = (int)threadIdx.x * kRegionPerThread + j;
      const int slot = rp < region_n ? s_slot(r0 + rp, t0, w, h) : -1;
      if (slot >= 0 && slot < kLdsEntries) { lds_v[slot] = sc[j].v; lds_c[slot] = sc[j].c; }
    }
    __syncthreads();
    const int o = (int)threadIdx.x * kOutPerThread;
    if (o < T) emit_outputs<OP, A>(d, LdsLookup<A>{lds_v, lds_c, t0, w, h}, t0 + o, n, w, h);
    __syncthreads();      // the LDS arrays are written again by the next tile of the stride loop
  }
}

// ---- the two-scan route ----
// logical position p of a scan is physical position p (forward) or n - 1 - p (backward) of the scanned order: cumulative's mirrored index
template <int OP, class A> __device__ __forceinline__ void load_scan_tile(const Src& s, int backward, int64_t base, Elem<A>* e) {
#pragma unroll
  for (int j = 0; j < kScanPerThread; j++) {
    const int64_t p = base + j;
    e[j] = neutral<OP, A>();
    if (p < s.n) { e[j] = elem_at<OP, A>(s, cumulative::physical_index(p, s.n, backward != 0)); e[j].f = backward ? (e[j].f >> 1) & 1u : e[j].f & 1u; }
  }
}
template <int OP, class A>
__global__ __launch_bounds__(kBlock) void rolling_reduce_kernel(Src s, int backward, A* __restrict__ agg_v, uint32_t* __restrict__ agg_c, uint32_t* __restrict__ agg_f) {
  __shared__ Elem<A> wave_tot[kWaves];
  const int64_t n_tiles = (s.n + kScanTile - 1) / kScanTile;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    Elem<A> e[kScanPerThread];
    load_scan_tile<OP, A>(s, backward, tile * kScanTile + (int64_t)threadIdx.x * kScanPerThread, e);
    const Elem<A> tot = block_scan<OP, A, kScanPerThread, false>(e, neutral<OP, A>(), wave_tot);
    if (threadIdx.x == 0) { agg_v[tile] = tot.v; agg_c[tile] = tot.c; agg_f[tile] = tot.f; }
  }
}
// the inclusive scan of the m tile aggregates, in place: one workgroup walks them 2048 at a time and carries its running element
template <int OP, class A>
__global__ __launch_bounds__(kBlock) void rolling_aggscan_kernel(A* __restrict__ agg_v, uint32_t* __restrict__ agg_c, uint32_t* __restrict__ agg_f, int64_t m) {
  __shared__ Elem<A> wave_tot[kWaves];
  Elem<A> carry = neutral<OP, A>();
  for (int64_t chunk = 0; chunk < m; chunk += kScanTile) {
    const int64_t base = chunk + (int64_t)threadIdx.x * kScanPerThread;
    Elem<A> e[kScanPerThread];
#pragma unroll
    for (int j = 0; j < kScanPerThread; j++) { const int64_t p = base + j; e[j] = p < m ? Elem<A>{agg_v[p], agg_c[p], agg_f[p]} : neutral<OP, A>(); }
    carry = block_scan<OP, A, kScanPerThread, false>(e, carry, wave_tot);
#pragma unroll
    for (int j = 0; j < kScanPerThread; j++) { const int64_t p = base + j; if (p < m) { agg_v[p] = e[j].v; agg_c[p] = e[j].c; agg_f[p] = e[j].f; } }
  }
}
template <int OP, class A>
__global__ __launch_bounds__(kBlock) void rolling_scan_kernel(Src s, int backward, const A* __restrict__ agg_v, const uint32_t* __restrict__ agg_c, const uint32_t* __restrict__ agg_f,
                                                              A* __restrict__ out_v, uint32_t* __restrict__ out_c) {
  __shared__ Elem<A> wave_tot[kWaves];
  const int64_t n_tiles = (s.n + kScanTile - 1) / kScanTile;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t base = tile * kScanTile + (int64_t)threadIdx.x * kScanPerThread;
    Elem<A> e[kScanPerThread];
    load_scan_tile<OP, A>(s, backward, base, e);
    const Elem<A> carry = tile > 0 ? Elem<A>{agg_v[tile - 1], agg_c[tile - 1], agg_f[tile - 1]} : neutral<OP, A>();
    block_scan<OP, A, kScanPerThread, false>(e, carry, wave_tot);
#pragma unroll
    for (int j = 0; j < kScanPerThread; j++) {
      const int64_t p = base + j;
      if (p < s.n) { const int64_t i = cumulative::physical_index(p, s.n, backward != 0); out_v[i] = e[j].v; out_c[i] = e[j].c; }
    }
  }
}
template <class A> struct GlobalLookup {
  const A *pv, *sv;
  const uint32_t *pc, *sc;
  __device__ __forceinline__ Elem<A> S(int64_t pos) const { return Elem<A>{sv[pos], sc[pos], 0u}; }
  __device__ __forceinline__ Elem<A> P(int64_t pos) const { return Elem<A>{pv[pos], pc[pos], 0u}; }
};
template <int OP, class A>
__global__ __launch_bounds__(kBlock) void rolling_combine_kernel(Dst d, GlobalLookup<A> look, int64_t n, int64_t w, int64_t h) {
  const int64_t lanes = (n + kOutPerThread - 1) / kOutPerThread;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < lanes; t += (int64_t)gridDim.x * blockDim.x) emit_outputs<OP, A>(d, look, t * kOutPerThread, n, w, h);
}

// the scanned elements of one direction in memory (the entry beside scan_column that takes the combined flags and builds no column)
template <int OP, class A>
static void scan_elements(const Src& s, bool backward, A* out_v, uint32_t* out_c) {
  const int64_t n = s.n, tiles = (n + kScanTile - 1) / kScanTile;
  const int grid = k::grid_for(n, kScanTile);
  Buf av = dev_alloc((size_t)tiles * sizeof(A)), ac = dev_alloc((size_t)tiles * 4), af = dev_alloc((size_t)tiles * 4);
  hipLaunchKernelGGL((rolling_reduce_kernel<OP, A>), dim3(grid), dim3(kBlock), 0, stream(), s, backward ? 1 : 0, av->as<A>(), ac->as<uint32_t>(), af->as<uint32_t>());
  PLX_HIP(hipGetLastError());
  hipLaunchKernelGGL((rolling_aggscan_kernel<OP, A>), dim3(1), dim3(kBlock), 0, stream(), av->as<A>(), ac->as<uint32_t>(), af->as<uint32_t>(), tiles);
  PLX_HIP(hipGetLastError());
  hipLaunchKernelGGL((rolling_scan_kernel<OP, A>), dim3(grid), dim3(kBlock), 0, stream(), s, backward ? 1 : 0, (const A*)av->as<A>(), (const uint32_t*)ac->as<uint32_t>(), (const uint32_t*)af->as<uint32_t>(), out_v, out_c);
  PLX_HIP(hipGetLastError());
  PLX_HIP(hipStreamSynchronize(stream()));      // the aggregates live until the kernel that reads them is done
}

template <int OP, class A>
static void rolling_typed(const Src& s, const Dst& d, int64_t h, bool tile_route) {
  const int64_t n = s.n;
  const uint64_t in_w = (uint64_t)dtype_width(s.dt), out_w = (uint64_t)dtype_width(d.out_dt), extra = (s.valid ? 1 : 0) + 1 + (s.perm ? 9 : 0);
  if (tile_route) {
    const int T = tile_rows(s.w);
    ProfileScope ps(s.perm ? "rolling_tile_sorted" : "rolling_tile", (uint64_t)n * (in_w + out_w) + (uint64_t)n * extra / 4, (uint64_t)n);
    hipLaunchKernelGGL((rolling_tile_kernel<OP, A>), dim3(k::grid_for(n, T)), dim3(kBlock), 0, stream(), s, d, h);
    PLX_HIP(hipGetLastError());
    return;
  }
  Buf pv = dev_alloc((size_t)n * sizeof(A)), sv = dev_alloc((size_t)n * sizeof(A)), pc = dev_alloc((size_t)n * 4), sc = dev_alloc((size_t)n * 4);
  ProfileScope ps(s.perm ? "rolling_scans_sorted" : "rolling_scans", (uint64_t)n * (4 * in_w + 4 * (sizeof(A) + 4) + out_w) + (uint64_t)n * extra, (uint64_t)n);
  scan_elements<OP, A>(s, false, pv->as<A>(), pc->as<uint32_t>());
  scan_elements<OP, A>(s, true, sv->as<A>(), sc->as<uint32_t>());
  const GlobalLookup<A> look{pv->as<A>(), sv->as<A>(), pc->as<uint32_t>(), sc->as<uint32_t>()};
  hipLaunchKernelGGL((rolling_combine_kernel<OP, A>), dim3(k::grid_for(n, kBlock * kOutPerThread)), dim3(kBlock), 0, stream(), d, look, n, s.w, h);
  PLX_HIP(hipGetLastError());
  PLX_HIP(hipStreamSynchronize(stream()));      // P and S live until the combine is done
}

bool tile_route_for(int64_t w) {
  const char* r = std::getenv("PLX_ROLLING_ROUTE");      // read per call: "scans" forces the two-scan route, "tile" (or nothing) names the default rule
  if (r && std::strcmp(r, "scans") == 0) return false;
  return lds_fits(w);
}

ColumnPtr rolling_column(const ScanOrder& order, const Segments& segs, const ColumnPtr& value, int op, const Params& p, std::string* route) {
  PLX_REQUIRE(op_ok(op), PLX_ERR_INVALID, "rolling: op " + std::to_string(op) + " is no plx_rolling_op (0 = sum, 1 = mean, 2 = min, 3 = max)");
  PLX_REQUIRE(p.window >= 1 && p.window <= 0x7fffffffull, PLX_ERR_INVALID, "rolling: window_size must be at least 1 (and below 2^31), got " + std::to_string((long long)p.window));
  PLX_REQUIRE(p.min_samples >= 1 && p.min_samples <= p.window, PLX_ERR_INVALID, "rolling: min_samples must lie in 1..window_size, got " + std::to_string((long long)p.min_samples));
  check_order(op_name(op), order, segs, value);
  const int64_t n = value->len;
  const int out_dt = result_dtype(op, value->dtype);
  if (out_dt < 0) fail(PLX_ERR_UNSUPPORTED, std::string(op_name(op)) + " of a " + dtype_name(value->dtype) + " column: integer, float and Boolean columns only");
  const int64_t w = (int64_t)p.window, h = half_of(w, p.center);
  const bool tile_route = tile_route_for(w);
  if (route) {
    if (n == 0) *route = "rolling[empty]";
    else if (tile_route) *route = "rolling[tile halo: w=" + std::to_string(w) + ", lds=" + std::to_string((size_t)kLdsEntries * 12 + (size_t)kWaves * 16) + "]";
    else *route = "rolling[two scans: w=" + std::to_string(w) + ", launches=7]";
  }
  auto out = std::make_shared<Column>();
  out->dtype = out_dt; out->len = n;
  out->values = out_dt == PLX_BOOL ? dev_alloc_zero(bitmap_bytes(std::max<int64_t>(n, 1))) : dev_alloc(values_bytes(out_dt, std::max<int64_t>(n, 1)) + 16);
  out->validity = dev_alloc_zero(bitmap_bytes(std::max<int64_t>(n, 1)));
  out->null_count = n == 0 ? 0 : -1;
  if (n == 0) return out;
  // a Boolean column is widened first (sum / mean: to UInt32; min / max: to bytes, the result narrowed back to bits)
  const void* x = value->data();
  int dt = value->dtype;
  Buf wide, narrow;
  void* dst = out->values->ptr;
  int dst_dt = out_dt;
  if (dt == PLX_BOOL) {
    dt = (op == PLX_ROLLING_SUM || op == PLX_ROLLING_MEAN) ? PLX_U32 : PLX_U8;
    wide = dev_alloc((size_t)n * dtype_width(dt) + 16);
    k::cast_from_bool(value->values->as<uint64_t>(), dt, n, wide->ptr);
    x = wide->ptr;
    if (dt == PLX_U8) { narrow = dev_alloc((size_t)n + 16); dst = narrow->ptr; dst_dt = PLX_U8; }
  }
  Src s{x, dt, value->valid_words(), nullptr, nullptr, n, w};
  Buf flag = dev_alloc_zero(8);
  Dst d{dst, dst_dt, out->validity->as<uint64_t>(), SegArgs{nullptr, nullptr, nullptr, nullptr, 0}, (uint32_t)p.min_samples, op == PLX_ROLLING_MEAN ? 1 : 0, flag->as<unsigned int>()};
  if (order.perm) {
    s.heads = order.heads->as<uint64_t>(); s.perm = order.perm->values->as<uint32_t>();
    d.seg = SegArgs{s.perm, s.heads, segs.prefix->as<uint64_t>(), segs.starts->as<uint32_t>(), segs.n_segments};
  }
  constexpr int SUM = PLX_CUM_SUM, MIN = PLX_CUM_MIN, MAX = PLX_CUM_MAX;
  const bool wide_int = dt == PLX_I8 || dt == PLX_I16 || dt == PLX_U8 || dt == PLX_U16 || dt == PLX_I64;
  if (op == PLX_ROLLING_MEAN || ((op == PLX_ROLLING_SUM) && (dt == PLX_F32 || dt == PLX_F64))) rolling_typed<SUM, double>(s, d, h, tile_route);
  else if (op == PLX_ROLLING_SUM) {
    if (wide_int) rolling_typed<SUM, int64_t>(s, d, h, tile_route);
    else if (dt == PLX_I32) rolling_typed<SUM, int32_t>(s, d, h, tile_route);
    else if (dt == PLX_U32) rolling_typed<SUM, uint32_t>(s, d, h, tile_route);
    else rolling_typed<SUM, uint64_t>(s, d, h, tile_route);
  } else {
    const bool mn = op == PLX_ROLLING_MIN;
    switch (dt) {
      case PLX_I8: case PLX_I16: case PLX_I32: mn ? rolling_typed<MIN, int32_t>(s, d, h, tile_route) : rolling_typed<MAX, int32_t>(s, d, h, tile_route); break;
      case PLX_U8: case PLX_U16: case PLX_U32: mn ? rolling_typed<MIN, uint32_t>(s, d, h, tile_route) : rolling_typed<MAX, uint32_t>(s, d, h, tile_route); break;
      case PLX_I64: mn ? rolling_typed<MIN, int64_t>(s, d, h, tile_route) : rolling_typed<MAX, int64_t>(s, d, h, tile_route); break;
      case PLX_U64: mn ? rolling_typed<MIN, uint64_t>(s, d, h, tile_route) : rolling_typed<MAX, uint64_t>(s, d, h, tile_route); break;
      case PLX_F32: mn ? rolling_typed<MIN, float>(s, d, h, tile_route) : rolling_typed<MAX, float>(s, d, h, tile_route); break;
      default: mn ? rolling_typed<MIN, double>(s, d, h, tile_route) : rolling_typed<MAX, double>(s, d, h, tile_route); break;
    }
  }
  unsigned int bad = 0;
  d2h_sync(&bad, flag->ptr, 4);
  PLX_REQUIRE(!bad, PLX_ERR_INVALID, "rolling: a sorted position without a segment (an inconsistent sorted order)");
  if (narrow) {
    plx_scalar zero; zero.u = 0;
    k::cmp(PLX_U8, PLX_NE, narrow->ptr, nullptr, zero, n, out->values->as<uint64_t>());
    PLX_HIP(hipStreamSynchronize(stream()));
  }
  return out;
}

}  // namespace rolling
}  // namespace plx
