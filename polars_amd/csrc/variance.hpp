// variance.hpp -- the arithmetic of var / std, one body for the kernels and for the host (the idiom of temporal.hpp / decimal.hpp: PLX_HD functions compiled into
// var_kernel, finalize_batch_kernel and into a host twin that tests/emu/variance_main.cpp drives under ASan + UBSan).
//
// Two states describe the valid rows of a set:
//   * Moments {n, mean, m2}: m2 = sum (x - mean)^2.  merge() is Chan's pairwise update (Chan, Golub, LeVeque 1979): associative up to rounding.  The per-node kernel
//     (kernels_reduce.hip var_kernel) combines lanes, waves and workgroups with it.  merge only ever subtracts the two means, so both sides may carry them relative
//     to any common origin: the kernel keeps them relative to the column's first valid value, which is what makes it robust to a common offset of any size (an
//     absolute mean near 1e15 is representable to 0.06, and the difference of two such means no better).
//   * shifted sums s1 = sum (x - p), s2 = sum (x - p)^2 about a pivot p: plain sums, so they can live in the aggregate cells of the fused sinks (commutative atomics).
//     from_shifted() turns them into m2 = s2 - s1^2 / n.  The cancellation in that difference is what DESIGN.md 4.14's accuracy contract bounds.
// n is a double everywhere: counts stay exact up to 2^53 rows.
#pragma once
#include <stdint.h>

#ifndef PLX_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define PLX_HD __host__ __device__
#else
#define PLX_HD
#endif
#endif

namespace plx {
namespace variance {

struct Moments { double n, mean, m2; };

// m2 of n rows from their sums about any pivot; a difference that rounding made negative is 0.  (NaN stays NaN: both comparisons are false for it.)
PLX_HD inline double from_shifted(double n, double s1, double s2) {
  if (!(n > 0.0)) return 0.0;
  const double m2 = s2 - s1 * (s1 / n);
  return m2 < 0.0 ? 0.0 : m2;
}

// Chan's pairwise combination.  An empty side is the identity: no 0/0 is ever formed.
PLX_HD inline Moments merge(Moments a, Moments b) {
  if (!(b.n > 0.0)) return a;
  if (!(a.n > 0.0)) return b;
  const double n = a.n + b.n;
  const double delta = b.mean - a.mean;
  Moments r;
  r.n = n;
  r.mean = a.mean + delta * (b.n / n);
  r.m2 = a.m2 + b.m2 + delta * delta * (a.n * (b.n / n));
  return r;
}

// var (or std) of n valid rows with the centred sum of squares m2; *valid = 0 (and 0.0) when n <= ddof.  An infinite or NaN m2 (a NaN or an infinity among the values:
// inf - inf inside the sums) gives NaN, which is not null.
PLX_HD inline double finalize(double n, double m2, int ddof, bool want_std, bool* valid) {
  if (!(n > (double)ddof)) { *valid = false; return 0.0; }
  *valid = true;
  double v = m2 / (n - (double)ddof);
  if (v != v || v - v != 0.0) return v - v;      // NaN and +-inf -> NaN
  if (v < 0.0) v = 0.0;
  return want_std ? __builtin_sqrt(v) : v;
}

}  // namespace variance
}  // namespace plx
