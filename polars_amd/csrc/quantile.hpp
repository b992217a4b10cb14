// quantile.hpp -- the arithmetic of median / quantile, one body for the kernels and for the host (the idiom of variance.hpp: PLX_HD functions compiled into
// segment_quantile_kernel, into ops::reduce_quantile and into a host program that tests/emu/quantile_main.cpp drives under ASan + UBSan).
//
// Reference behaviour (restated, not ported): polars-core/src/chunked_array/ops/aggregate/quantile.rs (quantile_idx, linear_interpol, midpoint_interpol).  With n valid
// values in the sort's total order (NaN greatest, -0 == +0):
//   pos = (double)(n - 1) * q; lo = floor(pos), hi = ceil(pos), both clamped to n - 1; a, b = the values at ranks lo and hi as f64
//   lower -> a; higher -> b; nearest -> the value at rank floor(pos + 0.5) (a tie goes up); midpoint -> a == b ? a : (a + b) / 2;
//   linear -> (a == b or lo == hi) ? a : (pos - lo) * (b - a) + a
// The value codes are the sort's (kernels_sort.hip encodes through encode_value below): an order-preserving u64 per value, so that an integer above 2^53 is selected
// exactly and rounded only by decode().
#pragma once
#include <stdint.h>

#include "../../include/polars_amd.h"

#ifndef PLX_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define PLX_HD __host__ __device__
#else
#define PLX_HD
#endif
#endif

namespace plx {
namespace quantile {

constexpr uint64_t kSign = 0x8000000000000000ull;

PLX_HD inline bool q_ok(double q) { return q >= 0.0 && q <= 1.0; }      // false for NaN
PLX_HD inline bool interpolation_ok(int interpolation) { return interpolation >= PLX_QUANTILE_NEAREST && interpolation <= PLX_QUANTILE_LINEAR; }

// ---- the sort's value code and its inverse ----
PLX_HD inline uint64_t flip_f64(double d) {
  const uint64_t b = (d != d) ? 0x7ff8000000000000ull : __builtin_bit_cast(uint64_t, d + 0.0);   // one NaN, -0 -> +0
  return (b >> 63) ? ~b : (b | kSign);
}
PLX_HD inline double unflip_f64(uint64_t code) { return __builtin_bit_cast(double, (code >> 63) ? (code ^ kSign) : ~code); }

// order-preserving code of row r of a column of `dtype` (Boolean columns are bitmaps)
PLX_HD inline uint64_t encode_value(int dtype, const void* values, int64_t r) {
  switch (dtype) {
    case PLX_I8: return (uint64_t)(long long)reinterpret_cast<const int8_t*>(values)[r] ^ kSign;
    case PLX_I16: return (uint64_t)(long long)reinterpret_cast<const int16_t*>(values)[r] ^ kSign;
    case PLX_I32: return (uint64_t)(long long)reinterpret_cast<const int32_t*>(values)[r] ^ kSign;
    case PLX_I64: return reinterpret_cast<const uint64_t*>(values)[r] ^ kSign;
    case PLX_U8: return reinterpret_cast<const uint8_t*>(values)[r];
    case PLX_U16: return reinterpret_cast<const uint16_t*>(values)[r];
    case PLX_U32: return reinterpret_cast<const uint32_t*>(values)[r];
    case PLX_F32: return flip_f64((double)reinterpret_cast<const float*>(values)[r]);
    case PLX_F64: return flip_f64(reinterpret_cast<const double*>(values)[r]);
    case PLX_BOOL: return (reinterpret_cast<const uint64_t*>(values)[r >> 6] >> (r & 63)) & 1;
    default: return reinterpret_cast<const uint64_t*>(values)[r];
  }
}
// the value behind a code as f64: exact for floats (a Float32 value is an f64), for integers up to 2^53; one rounding above
PLX_HD inline double decode(int dtype, uint64_t code) {
  switch (dtype) {
    case PLX_I8: case PLX_I16: case PLX_I32: case PLX_I64: return (double)(int64_t)(code ^ kSign);
    case PLX_F32: case PLX_F64: return unflip_f64(code);
    default: return (double)code;
  }
}

// ---- ranks ----
struct Rank { uint64_t lo, hi; double frac; };      // the two ranks to read (equal when one value decides) and pos - lo

// n >= 1 valid values, q in [0, 1]
PLX_HD inline Rank rank_of(uint64_t n, double q, int interpolation) {
  const double pos = (double)(n - 1) * q;
  const double fl = __builtin_floor(pos);
  uint64_t lo = (uint64_t)fl, hi = (uint64_t)__builtin_ceil(pos);
  if (lo > n - 1) lo = n - 1;
  if (hi > n - 1) hi = n - 1;
  Rank r;
  r.frac = pos - fl;
  switch (interpolation) {
    case PLX_QUANTILE_LOWER: hi = lo; break;
    case PLX_QUANTILE_HIGHER: lo = hi; break;
    case PLX_QUANTILE_NEAREST: { uint64_t k = (uint64_t)__builtin_floor(pos + 0.5); if (k > n - 1) k = n - 1; lo = hi = k; break; }
    default: break;
  }
  r.lo = lo; r.hi = hi;
  return r;
}

// a, b = the values at ranks lo, hi
PLX_HD inline double combine(double a, double b, double frac, int interpolation) {
  switch (interpolation) {
    case PLX_QUANTILE_HIGHER: return b;
    case PLX_QUANTILE_MIDPOINT: return a == b ? a : (a + b) / 2.0;
    case PLX_QUANTILE_LINEAR: return (a == b || frac == 0.0) ? a : frac * (b - a) + a;      // frac == 0: lo == hi
    default: return a;      // lower, nearest: rank_of made lo the rank
  }
}

}  // namespace quantile
}  // namespace plx
