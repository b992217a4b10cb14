// asof.hpp -- the arithmetic of join_asof, one body for the kernels and for the host (the idiom of rolling.hpp: PLX_HD functions compiled into the kernels of
// kernels_asof.hip and into a host program that tests/emu/asof_main.cpp drives under ASan + UBSan).
//
// Reference behaviour (restated, not ported): py-polars join_asof, polars-ops/src/frame/join/asof/.  Every left row gets at most one right row.  The candidates of
// a left row are the right rows whose `by` parts all equal its own (the sort's equality: NaN == NaN, -0 == +0), taken in (on, right row) order:
//   backward   the last candidate with on_r <= on_l            (allow_exact_matches = false: on_r < on_l)
//   forward    the first candidate with on_r >= on_l           (strict: on_r > on_l)
//   nearest    the candidate at the smallest distance; among several at that distance the LAST one in candidate order.  So an equidistant pair goes to the
//              forward value, a duplicated forward value to its last row, an exact match to the last of its duplicates (strict: exact matches are no candidates)
// A tolerance keeps the match found without it only if its distance is at most the tolerance: there is no fallback to another candidate.
//
// The key of a row is a tuple of W = n_by + 1 words of quantile::encode_value codes, the by parts first, `on` last.  Codes preserve the order, so the usable right
// rows sorted by tuple hold every group as one run in candidate order, and the rules above are positions around the lower and the upper bound of the left tuple:
//   lo = the first position whose tuple is >= t,  hi = the first position whose tuple is > t      (positions [lo, hi) hold the exact matches)
//   backward: hi - 1 (strict: lo - 1);  forward: lo (strict: hi);  nearest: hi - 1 (strict: lo - 1) against hi, the winner moved to the last of its duplicates
// each taken only if it lies in [0, M) and its by parts equal the left row's.  Integer codes differ by exactly the distance of their values, in 64 unsigned bits.
#pragma once
#include <stdint.h>

#include "quantile.hpp"

namespace plx {
namespace asof {

// ---- geometry ----
constexpr int kMaxBy = 7;
constexpr int kMaxWords = kMaxBy + 1;
constexpr int kThreads = 256;                  // T: the left rows a workgroup serves per step of its stride loop, one lane each
constexpr int kWaveLanes = 64;
constexpr int kLdsBytes = 64 * 1024;           // the sample stage: two workgroups share a CU's 160 KiB
constexpr int kLdsWords = kLdsBytes / 8;
// The sorted right side is code[w][M]; the sample stage holds every stride-th tuple as sample[w][ns], ns <= samples_for(W), and a hit among the samples narrows
// the search of the global arrays to less than one stride.
PLX_HD inline int samples_for(int W) { return W >= 1 && W <= kMaxWords ? kLdsWords / W : 0; }
PLX_HD inline int64_t stride_for(int64_t M, int64_t samples) { return samples <= 0 || M <= 0 ? 0 : (M + samples - 1) / samples; }      // 0: no sample stage
PLX_HD inline int64_t sample_count(int64_t M, int64_t stride) { return stride <= 0 ? 0 : (M + stride - 1) / stride; }                   // sample j is position j * stride
struct Range { int64_t lo, hi; };
// j = the bound of t among the ns samples (the first sample >= t, or > t): the same bound among the M positions lies in [lo, hi], and is hi when no position of
// [lo, hi) qualifies -- position (j - 1) * stride is known to fail, position j * stride (or M) to qualify
PLX_HD inline Range narrow(int64_t j, int64_t ns, int64_t stride, int64_t M) {
  Range r;
  r.lo = j == 0 ? 0 : (j - 1) * stride + 1;
  r.hi = j >= ns ? M : j * stride;
  return r;
}

// ---- the `how` slot of a PLX_IR_JOIN_ASOF node: a plx_asof_strategy, OR'd with PLX_ASOF_STRICT for allow_exact_matches = false ----
PLX_HD inline int pack_how(int strategy, bool strict) { return strategy | (strict ? PLX_ASOF_STRICT : 0); }
PLX_HD inline int strategy_of(int how) { return how & 3; }
PLX_HD inline bool strict_of(int how) { return (how & PLX_ASOF_STRICT) != 0; }
PLX_HD inline bool how_ok(int how) { return how >= 0 && (how & ~(3 | PLX_ASOF_STRICT)) == 0 && strategy_of(how) <= PLX_ASOF_NEAREST; }
inline const char* strategy_name(int how) {
  switch (strategy_of(how)) {
    case PLX_ASOF_BACKWARD: return "backward";
    case PLX_ASOF_FORWARD: return "forward";
    case PLX_ASOF_NEAREST: return "nearest";
    default: return "?";
  }
}
// which of the two bounds a strategy reads
PLX_HD inline bool needs_lower(int how) { return strict_of(how) ? strategy_of(how) != PLX_ASOF_FORWARD : strategy_of(how) == PLX_ASOF_FORWARD; }
PLX_HD inline bool needs_upper(int how) { return strict_of(how) ? strategy_of(how) != PLX_ASOF_BACKWARD : strategy_of(how) != PLX_ASOF_FORWARD; }

// ---- tuples ----
template <int W> struct Tuple { uint64_t w[W]; };
template <int W> PLX_HD inline bool tuple_less(const Tuple<W>& a, const Tuple<W>& b) {
#pragma unroll
  for (int i = 0; i < W; i++) if (a.w[i] != b.w[i]) return a.w[i] < b.w[i];
  return false;
}
template <int W> PLX_HD inline bool by_equal(const Tuple<W>& a, const Tuple<W>& b) {
#pragma unroll
  for (int i = 0; i + 1 < W; i++) if (a.w[i] != b.w[i]) return false;
  return true;
}
// An array of tuples, one word array after the other: word w of position p is base[w * pitch + p].  The LDS samples and the global codes are both of this shape,
// so one search body serves both stages.
struct Words {
  const uint64_t* base;
  int64_t pitch;
  PLX_HD uint64_t at(int w, int64_t p) const { return base[(int64_t)w * pitch + p]; }
};
template <int W, class A> PLX_HD inline Tuple<W> tuple_at(const A& arr, int64_t p) {
  Tuple<W> t;
#pragma unroll
  for (int i = 0; i < W; i++) t.w[i] = arr.at(i, p);
  return t;
}
// -1 / 0 / +1: the tuple at position p against t.  A word is read only when the words before it are equal.
template <int W, class A> PLX_HD inline int compare_at(const A& arr, int64_t p, const Tuple<W>& t) {
#pragma unroll
  for (int i = 0; i < W; i++) {
    const uint64_t x = arr.at(i, p);
    if (x != t.w[i]) return x < t.w[i] ? -1 : 1;
  }
  return 0;
}
template <int W, class A> PLX_HD inline bool by_equal_at(const A& arr, int64_t p, const Tuple<W>& t) {
#pragma unroll
  for (int i = 0; i + 1 < W; i++) if (arr.at(i, p) != t.w[i]) return false;
  return true;
}

// ---- the bound search ----
// the first position of [lo, hi) whose tuple is >= t (UPPER: > t); hi when there is none.  The array is sorted over [lo, hi).
template <int W, bool UPPER, class A> PLX_HD inline int64_t bound(const A& arr, int64_t lo, int64_t hi, const Tuple<W>& t) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    const int c = compare_at<W>(arr, mid, t);
    if (UPPER ? c <= 0 : c < 0) lo = mid + 1; else hi = mid;
  }
  return lo;
}
template <int W, class A> PLX_HD inline int64_t lower_bound(const A& arr, int64_t lo, int64_t hi, const Tuple<W>& t) { return bound<W, false>(arr, lo, hi, t); }
template <int W, class A> PLX_HD inline int64_t upper_bound(const A& arr, int64_t lo, int64_t hi, const Tuple<W>& t) { return bound<W, true>(arr, lo, hi, t); }
// both stages: the ns samples (ns == 0: none), then less than one stride of the M positions
template <int W, bool UPPER, class AS, class AG> PLX_HD inline int64_t search(const AS& samples, int64_t ns, int64_t stride, const AG& codes, int64_t M, const Tuple<W>& t) {
  Range r{0, M};
  if (ns > 0) r = narrow(bound<W, UPPER>(samples, 0, ns, t), ns, stride, M);
  return bound<W, UPPER>(codes, r.lo, r.hi, t);
}

// ---- distances and the tolerance ----
// integer family (integers, Date, Datetime): the codes differ by the distance of the values, exact in 64 unsigned bits (Int64.min against Int64.max: 2^64 - 1)
PLX_HD inline uint64_t distance_int(uint64_t a, uint64_t b) { return a > b ? a - b : b - a; }
// floats: |a - b| in f64; equal codes are distance 0 (NaN against NaN, inf against inf); a NaN against a number is a NaN distance
PLX_HD inline double distance_f64(uint64_t a, uint64_t b) {
  if (a == b) return 0.0;
  return __builtin_fabs(quantile::unflip_f64(a) - quantile::unflip_f64(b));
}
enum { kNoTolerance = 0, kIntTolerance = 1, kFloatTolerance = 2 };
struct Tolerance { int kind; uint64_t u; double f; };
PLX_HD inline bool within(const Tolerance& tol, uint64_t a, uint64_t b) {
  if (tol.kind == kIntTolerance) return distance_int(a, b) <= tol.u;
  if (tol.kind == kFloatTolerance) return distance_f64(a, b) <= tol.f;      // false for a NaN distance
  return true;
}
// nearest: the forward candidate (later in candidate order) wins unless the backward one is strictly closer; a NaN distance loses against any number
PLX_HD inline bool forward_wins(bool is_float, uint64_t t_on, uint64_t back_on, uint64_t fwd_on) {
  if (!is_float) return distance_int(fwd_on, t_on) <= distance_int(t_on, back_on);
  const double db = distance_f64(t_on, back_on), df = distance_f64(fwd_on, t_on);
  return df <= db || db != db;
}

// ---- the match of one left row ----
constexpr int64_t kNone = -1;
// lo / hi: the lower / upper bound of t among the M sorted positions (only the one(s) needs_lower / needs_upper name are read).  Returns the matched position or
// kNone; for `nearest` this includes the third search, for the last duplicate of a winning forward value.
template <int W, class A> PLX_HD inline int64_t pick(int how, int64_t lo, int64_t hi, const A& codes, int64_t M, const Tuple<W>& t, bool is_float) {
  const bool strict = strict_of(how);
  const int strategy = strategy_of(how);
  if (strategy == PLX_ASOF_BACKWARD) {
    const int64_t p = (strict ? lo : hi) - 1;
    return p >= 0 && p < M && by_equal_at<W>(codes, p, t) ? p : kNone;
  }
  if (strategy == PLX_ASOF_FORWARD) {
    const int64_t p = strict ? hi : lo;
    return p >= 0 && p < M && by_equal_at<W>(codes, p, t) ? p : kNone;
  }
  int64_t b = (strict ? lo : hi) - 1, f = hi;
  if (!(b >= 0 && b < M && by_equal_at<W>(codes, b, t))) b = kNone;
  if (!(f >= 0 && f < M && by_equal_at<W>(codes, f, t))) f = kNone;
  if (f == kNone) return b;
  if (b != kNone && !forward_wins(is_float, t.w[W - 1], codes.at(W - 1, b), codes.at(W - 1, f))) return b;
  if (f + 1 < M) {
    Tuple<W> tf = tuple_at<W>(codes, f);
    if (is_float && distance_f64(tf.w[W - 1], t.w[W - 1]) == __builtin_inf()) {
      // an infinite distance is shared by every later candidate that is no NaN (on_l is -inf, or the candidates are +inf): the last of those
      tf.w[W - 1] = quantile::flip_f64(__builtin_nan(""));
      return bound<W, false>(codes, f + 1, M, tf) - 1;
    }
    if (compare_at<W>(codes, f + 1, tf) == 0) f = bound<W, true>(codes, f + 2, M, tf) - 1;
  }
  return f;
}
// the whole walk of one left row with every key part valid: search, pick, tolerance
template <int W, class AS, class AG> PLX_HD inline int64_t match_row(int how, const AS& samples, int64_t ns, int64_t stride, const AG& codes, int64_t M, const Tuple<W>& t, bool is_float,
                                                                     const Tolerance& tol) {
  int64_t lo = 0, hi = 0;
  if (needs_lower(how)) lo = search<W, false>(samples, ns, stride, codes, M, t);
  if (needs_upper(how)) hi = search<W, true>(samples, ns, stride, codes, M, t);
  const int64_t p = pick<W>(how, lo, hi, codes, M, t, is_float);
  if (p == kNone) return kNone;
  return within(tol, t.w[W - 1], codes.at(W - 1, p)) ? p : kNone;
}

// ---- dtypes ----
PLX_HD inline bool on_dtype_ok(int dt) { return dt >= PLX_I8 && dt <= PLX_F64; }
PLX_HD inline bool by_dtype_ok(int dt) { return dt >= PLX_BOOL && dt <= PLX_F64; }
PLX_HD inline bool dtype_is_float(int dt) { return dt == PLX_F32 || dt == PLX_F64; }

}  // namespace asof
}  // namespace plx
