// rolling.hpp -- the arithmetic of shift / diff and of rolling_sum / rolling_mean / rolling_min / rolling_max, one body for the kernels and for the host (the idiom
// of cumulative.hpp: PLX_HD functions compiled into the kernels of kernels_rolling.hip, into the host side of the routes and into a host program that
// tests/emu/rolling_main.cpp drives under ASan + UBSan).
//
// A rolling function over a window of w positions is TWO SEGMENTED SCANS and one combine per row (van Herk / Gil-Werman).  The scanned order is cut
// into blocks of w positions aligned at multiples of w.  P is the inclusive forward scan that restarts at every segment head and every block start, S the backward
// scan that restarts at every segment end and every block end.  A window [a, b] with b - a < w inside one segment holds at most one block start c in (a, b], and
//     value(a, b) = S[a] (+) P[b]   if such a c exists        (S[a] covers a .. c - 1, P[b] covers c .. b)
//                 = P[b]            if a starts a run         (a is the segment head or a block start)
//                 = S[a]            otherwise                 (then b is the segment's last position: the window was clipped on the right only)
// The element is (value or identity, count of valid values); the count decides the validity.  Nothing is derived by subtracting prefixes: min / max have no
// inverse, and a float sum would keep an infinity that has left the window.
#pragma once
#include <stdint.h>

#include "cumulative.hpp"

namespace plx {
namespace rolling {

// ---- geometry ----
// tile-halo route: a workgroup of kThreads lanes scans a region of kRegion positions, kRegionPerThread consecutive ones per lane: a tile of output positions plus
// its w - 1 halo positions.  The tile is kTile outputs (8 consecutive per lane: whole validity bytes) while the region holds it, and shrinks to the multiple of 8
// that fits above that: tile_rows(w).  kMaxWindow is the largest w served; there the tile is 1024 outputs.
constexpr int kThreads = cumulative::kThreads;
constexpr int kWaveLanes = cumulative::kWaveLanes;
constexpr int kWaves = cumulative::kWaves;
constexpr int kOutPerThread = 8;
constexpr int kTile = kThreads * kOutPerThread;               // at most 2048 outputs per workgroup
constexpr int kRegionPerThread = 12;
constexpr int kRegion = kThreads * kRegionPerThread;          // 3072 scanned positions per workgroup
constexpr int kMaxWindow = 2048;                              // kRollingMaxWindow of DESIGN.md 4.19
PLX_HD inline int tile_rows(int64_t w) { const int64_t fit = (kRegion + 1 - w) & ~(int64_t)7; return (int)(fit < kTile ? fit : kTile); }
// LDS of the tile route: the S of the tile's window starts (T + w - 1 - h entries) and the P of its window ends (T + h entries) in one array of 2 T + w - 1 entries
// of (value, count), 8 + 4 bytes at the widest accumulator.  T = 2048 up to w = 1025 (5120 entries), and above that 2 T + w - 1 <= 6145 - w stays below
constexpr int kLdsEntries = 2 * kTile + 1024;
constexpr int kScanPerThread = cumulative::kPerThread;        // the two-scan route walks cumulative's 2048-position tiles
constexpr int kScanTile = kThreads * kScanPerThread;

// ---- parameters ----
PLX_HD inline bool op_ok(int op) { return op >= PLX_ROLLING_SUM && op <= PLX_ROLLING_MAX; }
inline const char* op_name(int op) {
  switch (op) {
    case PLX_ROLLING_SUM: return "rolling_sum";
    case PLX_ROLLING_MEAN: return "rolling_mean";
    case PLX_ROLLING_MIN: return "rolling_min";
    case PLX_ROLLING_MAX: return "rolling_max";
    default: return "?";
  }
}
// the three parameters of a PLX_AE_ROLLING node in one literal: window_size in bits 0..31, min_samples in bits 32..62, center in bit 63
struct Params { uint64_t window, min_samples; bool center; };
PLX_HD inline uint64_t pack_params(uint64_t window, uint64_t min_samples, bool center) { return (window & 0xffffffffull) | ((min_samples & 0x7fffffffull) << 32) | ((uint64_t)(center ? 1 : 0) << 63); }
PLX_HD inline Params unpack_params(uint64_t u) { return Params{u & 0xffffffffull, (u >> 32) & 0x7fffffffull, (u >> 63) != 0}; }
PLX_HD inline bool params_ok(const Params& p) { return p.window >= 1 && p.window <= 0x7fffffffull && p.min_samples >= 1 && p.min_samples <= p.window; }
// the window of row i is [i + h - w + 1, i + h]
PLX_HD inline int64_t half_of(int64_t w, bool center) { return center ? (w - 1) / 2 : 0; }

// ---- result dtypes (-1: the operand dtype is not accepted) ----
PLX_HD inline int result_dtype(int op, int in) {
  if (in < PLX_BOOL || in > PLX_F64) return -1;
  switch (op) {
    case PLX_ROLLING_SUM: return cumulative::result_dtype(PLX_CUM_SUM, in);
    case PLX_ROLLING_MEAN: return in == PLX_F32 ? PLX_F32 : PLX_F64;
    case PLX_ROLLING_MIN: case PLX_ROLLING_MAX: return in;
    default: return -1;
  }
}
// diff: an unsigned operand widens to the next signed width (UInt32 and UInt64 to Int64), everything else keeps its dtype; Boolean has no difference
PLX_HD inline int diff_dtype(int in) {
  switch (in) {
    case PLX_U8: return PLX_I16;
    case PLX_U16: return PLX_I32;
    case PLX_U32: case PLX_U64: return PLX_I64;
    case PLX_I8: case PLX_I16: case PLX_I32: case PLX_I64: case PLX_F32: case PLX_F64: return in;
    default: return -1;
  }
}
// x[i] - x[i - n] in the result type; integers wrap (the subtraction runs on the unsigned type)
template <class O, class T> PLX_HD inline O diff_value(T a, T b) {
  if constexpr (std::is_integral<O>::value) { using U = typename std::make_unsigned<O>::type; return (O)(U)((U)(O)a - (U)(O)b); }
  else return (O)a - (O)b;
}

// ---- the element and its combine ----
// v: the op over the valid values (the identity when there is none), c: how many valid values, f: a restart flag inside (as cumulative::Pair's)
template <class A> struct Elem { A v; uint32_t c; uint32_t f; };
// OP is a plx_cum_op: SUM (rolling_sum and rolling_mean), MIN, MAX; `a` precedes `b` in the scan's direction
template <int OP, class A> PLX_HD inline Elem<A> neutral() { return Elem<A>{cumulative::identity<OP, A>(), 0u, 0u}; }
template <int OP, class A> PLX_HD inline Elem<A> combine(const Elem<A>& a, const Elem<A>& b) {
  return Elem<A>{b.f ? b.v : cumulative::apply<OP, A>(a.v, b.v), b.f ? b.c : a.c + b.c, a.f | b.f};
}
// the value of a window from two scanned elements, no flag involved
template <int OP, class A> PLX_HD inline Elem<A> join(const Elem<A>& s, const Elem<A>& p) { return Elem<A>{cumulative::apply<OP, A>(s.v, p.v), s.c + p.c, 0u}; }

// ---- the restart flags of the two scans at position i of the scanned order ----
// head / next_head: the segment-head bit of i / of i + 1 (whole column: i == 0 / never)
PLX_HD inline bool forward_flag(int64_t i, int64_t w, bool head) { return head || i % w == 0; }
PLX_HD inline bool backward_flag(int64_t i, int64_t n, int64_t w, bool next_head) { return i + 1 >= n || next_head || (i + 1) % w == 0; }

// ---- which scanned elements a row's window reads ----
// Row at position i of the segment [s0, s1): the clipped window [a, b], and which of S[a], P[b] give its value
enum { kUseP = 1, kUseS = 2 };
struct Window { int64_t a, b; int use; };
PLX_HD inline Window window_of(int64_t i, int64_t s0, int64_t s1, int64_t w, int64_t h) {
  Window r;
  r.a = i + h - w + 1 < s0 ? s0 : i + h - w + 1;
  r.b = i + h > s1 - 1 ? s1 - 1 : i + h;
  const int64_t c = (r.b / w) * w;      // the last block start at or below b
  r.use = c > r.a ? (kUseP | kUseS) : (r.a == s0 || r.a % w == 0) ? kUseP : kUseS;
  return r;
}

// ---- the pieces of a scan, one body for the lanes of the kernels and for the host program that walks them lane by lane ----
// REV: the scan runs from the last position to the first (the backward scan of the tile route; the two-scan route mirrors its index instead)
template <int OP, class A, int N, bool REV> PLX_HD inline Elem<A> fold_thread(const Elem<A>* e) {
  Elem<A> t = e[REV ? N - 1 : 0];
  for (int j = 1; j < N; j++) t = combine<OP, A>(t, e[REV ? N - 1 - j : j]);
  return t;
}
// one step of the wave's inclusive scan: `other` comes from lane - s (forward, __shfl_up) or lane + s (backward, __shfl_down)
template <int OP, class A, bool REV> PLX_HD inline Elem<A> wave_step(const Elem<A>& mine, const Elem<A>& other, int lane, int s) {
  return (REV ? lane + s < kWaveLanes : lane >= s) ? combine<OP, A>(other, mine) : mine;
}
// what the waves that precede `wave` in the scan's direction carry into it
template <int OP, class A, bool REV> PLX_HD inline Elem<A> fold_waves(const Elem<A>* wave_tot, int wave) {
  Elem<A> c = neutral<OP, A>();
  for (int k = 0; k < kWaves; k++) {
    const int w = REV ? kWaves - 1 - k : k;
    if (REV ? w > wave : w < wave) c = combine<OP, A>(c, wave_tot[w]);
  }
  return c;
}
template <int OP, class A, int N, bool REV> PLX_HD inline void scan_thread(Elem<A> carry, Elem<A>* e) {
  for (int j = 0; j < N; j++) { const int q = REV ? N - 1 - j : j; carry = combine<OP, A>(carry, e[q]); e[q] = carry; }
}

// ---- the tile route's LDS layout ----
// Tile t owns the outputs [t0, t0 + T), t0 = t * T, T = tile_rows(w); its region starts at r0 = t0 + h - (w - 1) and holds T + w - 1 positions.  The S of the
// positions [r0, t0 + T) sits at slot (pos - r0), the P of the positions [t0, t0 + T + h) behind it at slot s_len + (pos - t0)
PLX_HD inline int64_t region_start(int64_t t0, int64_t w, int64_t h) { return t0 + h - (w - 1); }
PLX_HD inline int s_len(int64_t w, int64_t h) { return (int)(tile_rows(w) + w - 1 - h); }
PLX_HD inline int s_slot(int64_t pos, int64_t t0, int64_t w, int64_t h) { const int64_t k = pos - region_start(t0, w, h); return k >= 0 && k < s_len(w, h) ? (int)k : -1; }
PLX_HD inline int p_slot(int64_t pos, int64_t t0, int64_t w, int64_t h) { const int64_t k = pos - t0; return k >= 0 && k < tile_rows(w) + h ? s_len(w, h) + (int)k : -1; }
PLX_HD inline bool lds_fits(int64_t w) { return w >= 1 && w <= kMaxWindow && tile_rows(w) >= 8 && tile_rows(w) + w - 1 <= kRegion && 2 * tile_rows(w) + w - 1 <= kLdsEntries; }

// ---- shift / diff: where row i reads from ----
// sorted position i of the segment [s0, s1) reads position i - n when that lies inside the segment
PLX_HD inline bool shift_source(int64_t i, int64_t n, int64_t s0, int64_t s1, int64_t* src) {
  const int64_t s = i - n;
  *src = s;
  return s >= s0 && s < s1;
}
// word k of a bitmap of n_bits bits with everything outside [0, n_bits) clear; valid == null: every row is valid
PLX_HD inline uint64_t clean_word(const uint64_t* valid, int64_t n_bits, int64_t k) {
  const int64_t words = (n_bits + 63) >> 6;
  if (k < 0 || k >= words) return 0;
  uint64_t v = valid ? valid[k] : ~0ull;
  if (k == words - 1 && (n_bits & 63)) v &= (1ull << (n_bits & 63)) - 1;
  return v;
}
// word `wi` of the whole-column validity of shift(n): bit j = bit (64 * wi + j - n) of the input where that lies in [0, n_bits) -- a funnel shift of two input
// words -- and `fill` (vacated rows are valid) elsewhere below n_bits
PLX_HD inline uint64_t shifted_word(const uint64_t* valid, int64_t n_bits, int64_t wi, int64_t n, bool fill) {
  const int64_t first = wi * 64 - n;                           // the source bit of bit 0
  const int64_t q = first >= 0 ? first >> 6 : -((-first + 63) >> 6);
  const unsigned r = (unsigned)(first - q * 64);
  auto funnel = [&](const uint64_t* m) {
    const uint64_t lo = clean_word(m, n_bits, q), hi = clean_word(m, n_bits, q + 1);
    return r ? (lo >> r) | (hi << (64 - r)) : lo;
  };
  uint64_t out = funnel(valid);
  if (fill) out |= ~funnel(nullptr);
  return out & clean_word(nullptr, n_bits, wi);      // nothing above the last row
}

}  // namespace rolling
}  // namespace plx
