// cumulative.hpp -- the arithmetic of cum_sum / cum_min / cum_max / cum_count and rank, one body for the kernels and for the host (the idiom of window.hpp and
// distinct.hpp: PLX_HD functions compiled into the kernels of kernels_cumulative.hip, into the host side of the routes and into a host program that
// tests/emu/cumulative_main.cpp drives under ASan + UBSan).
//
// A cumulative function is a SEGMENTED INCLUSIVE SCAN of one column: the elements are pairs (flag, value), flag = "this position starts a
// partition", and the combine
//     (f1, v1) (+) (f2, v2) = (f1 | f2, f2 ? v2 : v1 op v2)
// is associative for every associative op, so the scan may be cut into tiles, waves and lanes in any way.  A null row contributes the op's identity and keeps its
// own flag; a valid row always includes itself, so the identity never shows at a valid row.  Nothing here derives an exclusive value by subtracting: there is no
// inverse for min / max, and none for a float sum once an infinity is in the prefix.
#pragma once
#include <stdint.h>

#include <limits>
#include <type_traits>

#include "../../include/polars_amd.h"
#include "distinct.hpp"

namespace plx {
namespace cumulative {

// ---- the scan's geometry (kernels_scan.hip's: 256 lanes x 8 positions) ----
constexpr int kPerThread = 8;
constexpr int kThreads = 256;
constexpr int kWaveLanes = 64;
constexpr int kWaves = kThreads / kWaveLanes;
constexpr int kTile = kThreads * kPerThread;      // 2048 positions per tile

// ---- parameters ----
PLX_HD inline bool op_ok(int op) { return op >= PLX_CUM_SUM && op <= PLX_CUM_COUNT; }
PLX_HD inline bool method_ok(int m) { return m >= PLX_RANK_AVERAGE && m <= PLX_RANK_ORDINAL; }
inline const char* op_name(int op) {
  switch (op) {
    case PLX_CUM_SUM: return "cum_sum";
    case PLX_CUM_MIN: return "cum_min";
    case PLX_CUM_MAX: return "cum_max";
    case PLX_CUM_COUNT: return "cum_count";
    default: return "?";
  }
}
inline const char* method_name(int m) {
  switch (m) {
    case PLX_RANK_AVERAGE: return "average";
    case PLX_RANK_MIN: return "min";
    case PLX_RANK_MAX: return "max";
    case PLX_RANK_DENSE: return "dense";
    case PLX_RANK_ORDINAL: return "ordinal";
    default: return "?";
  }
}

// ---- result dtypes (-1: the operand dtype is not accepted) ----
// cum_sum: the sum aggregate's rule (narrow integers -> Int64, Boolean -> UInt32, everything else keeps its dtype); cum_min / cum_max keep the dtype; cum_count is
// UInt32 whatever it counts
PLX_HD inline int result_dtype(int op, int in) {
  if (in < PLX_BOOL || in > PLX_F64) return -1;
  switch (op) {
    case PLX_CUM_SUM:
      if (in == PLX_BOOL) return PLX_U32;
      if (in == PLX_I8 || in == PLX_I16 || in == PLX_U8 || in == PLX_U16) return PLX_I64;
      return in;
    case PLX_CUM_MIN: case PLX_CUM_MAX: return in;
    case PLX_CUM_COUNT: return PLX_U32;
    default: return -1;
  }
}
// rank: "average" is Float64, the other four are UInt32
PLX_HD inline int rank_dtype(int method) { return method == PLX_RANK_AVERAGE ? PLX_F64 : PLX_U32; }

// ---- the pair and its combine ----
template <class A> struct Pair { A v; uint32_t f; };

// sum wraps for integers (two's complement: the addition runs on the unsigned type, a signed overflow is no undefined behaviour here); min / max of floats ignore a
// NaN unless both sides are NaN (the min / max aggregate's rule, np.fmin / np.fmax); cum_count is a sum of 0 / 1
template <int OP, class A> PLX_HD inline A apply(A a, A b) {
  if constexpr (OP == PLX_CUM_SUM || OP == PLX_CUM_COUNT) {
    if constexpr (std::is_integral<A>::value) { using U = typename std::make_unsigned<A>::type; return (A)(U)((U)a + (U)b); }
    else return a + b;
  } else {
    if constexpr (std::is_floating_point<A>::value) { if (a != a) return b; if (b != b) return a; }
    if constexpr (OP == PLX_CUM_MIN) return b < a ? b : a;
    else return b > a ? b : a;
  }
}
// what a null row (and a position past the end) contributes: a op identity == a.  For the float min / max that ignore NaN, NaN is that value
template <int OP, class A> PLX_HD inline A identity() {
  if constexpr (OP == PLX_CUM_SUM || OP == PLX_CUM_COUNT) return (A)0;
  else if constexpr (std::is_floating_point<A>::value) return std::numeric_limits<A>::quiet_NaN();
  else if constexpr (OP == PLX_CUM_MIN) return std::numeric_limits<A>::max();
  else return std::numeric_limits<A>::lowest();
}
template <int OP, class A> PLX_HD inline Pair<A> neutral() { return Pair<A>{identity<OP, A>(), 0u}; }
template <int OP, class A> PLX_HD inline Pair<A> combine(const Pair<A>& a, const Pair<A>& b) {
  return Pair<A>{b.f ? b.v : apply<OP, A>(a.v, b.v), a.f | b.f};
}

// ---- the mirrored index of reverse=True ----
// Logical position p of the scan is physical position p (forward) or n - 1 - p (reverse) of the order scanned: the rows themselves, or the key-sorted order
PLX_HD inline int64_t physical_index(int64_t p, int64_t n, bool reverse) { return reverse ? n - 1 - p : p; }
// the flag of physical position i under a segment-head mask: forward "i starts its segment"; reverse "i is the last of its segment", i.e. the head bit of the
// position after it, or the end
PLX_HD inline bool flag_at(const uint64_t* heads, int64_t i, int64_t n, bool reverse) {
  if (!reverse) return (heads[i >> 6] >> (i & 63)) & 1;
  return i + 1 >= n || ((heads[(i + 1) >> 6] >> ((i + 1) & 63)) & 1);
}

// ---- the pieces of a tile, one body for the lanes of the kernels and for the host program that walks them lane by lane ----
// the aggregate of a lane's kPerThread consecutive positions
template <int OP, class A> PLX_HD inline Pair<A> fold_thread(const Pair<A>* e) {
  Pair<A> t = e[0];
  for (int j = 1; j < kPerThread; j++) t = combine<OP, A>(t, e[j]);
  return t;
}
// one step of the wave's inclusive scan: lane `lane` holds `mine` and receives `below` from lane - s (__shfl_up); lanes below s keep what they hold
template <int OP, class A> PLX_HD inline Pair<A> wave_step(const Pair<A>& mine, const Pair<A>& below, int lane, int s) {
  return lane >= s ? combine<OP, A>(below, mine) : mine;
}
// what the waves in front of `wave` carry into it (wave_tot: the kWaves wave totals of the tile, through LDS); wave == kWaves: the tile's aggregate
template <int OP, class A> PLX_HD inline Pair<A> fold_waves(const Pair<A>* wave_tot, int wave) {
  Pair<A> c = neutral<OP, A>();
  for (int w = 0; w < kWaves; w++) if (w < wave) c = combine<OP, A>(c, wave_tot[w]);
  return c;
}
// the lane's positions, scanned in place from what precedes them (the tile's carry-in, the waves in front, the lanes in front)
template <int OP, class A> PLX_HD inline void scan_thread(Pair<A> carry, Pair<A>* e) {
  for (int j = 0; j < kPerThread; j++) { carry = combine<OP, A>(carry, e[j]); e[j] = carry; }
}

// ---- rank: the formulas from two ranks and two starts ----
// Sorted position i (0-based) of a segment that starts at seg_start lies in a run of equal values [run_start, run_end); run_rank = the number of run heads at
// positions <= i, seg_first_run = the same count at the segment's first position.  All results are 1-based within the segment
PLX_HD inline uint32_t rank_value(int method, uint64_t i, uint64_t seg_start, uint64_t run_start, uint64_t run_end, uint64_t run_rank, uint64_t seg_first_run) {
  switch (method) {
    case PLX_RANK_ORDINAL: return (uint32_t)(i - seg_start + 1);
    case PLX_RANK_MIN: return (uint32_t)(run_start - seg_start + 1);
    case PLX_RANK_MAX: return (uint32_t)(run_end - seg_start);
    case PLX_RANK_DENSE: return (uint32_t)(run_rank - seg_first_run + 1);
    default: return 0u;
  }
}
// "average": the mean of the min and the max rank, exact in f64 (both below 2^32)
PLX_HD inline double rank_average(uint64_t seg_start, uint64_t run_start, uint64_t run_end) {
  return 0.5 * ((double)(run_start - seg_start + 1) + (double)(run_end - seg_start));
}
// the start of the k-th (1-based) set bit's run and friends come from a mask's per-word prefix (distinct::rank_before) and its compacted positions `starts`:
// position i lies in the run number rank_before(i + 1), which starts at starts[that - 1] and ends at starts[that] (or n for the last run)
struct RunOf { uint64_t rank, start, end; bool ok; };
PLX_HD inline RunOf run_of(const uint64_t* prefix, const uint64_t* mask, const uint32_t* starts, uint64_t n_runs, uint64_t n, uint64_t i) {
  RunOf r{0, 0, 0, false};
  r.rank = distinct::rank_before(prefix, mask, i + 1);
  if (r.rank < 1 || r.rank > n_runs) return r;
  r.start = starts[r.rank - 1];
  r.end = r.rank < n_runs ? (uint64_t)starts[r.rank] : n;
  r.ok = r.start <= i && i < r.end && r.end <= n;
  return r;
}

}  // namespace cumulative
}  // namespace plx
