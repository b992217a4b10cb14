// decimal.hpp -- the arithmetic of the decimal shadow of an f64 column (encoded_inputs.hpp, DESIGN.md "Encoded shadows"): prices, rates and quantities are decimals
// with a few fractional digits kept in 64 bits.  Such a column is held a second time as u32 codes,
//     value = div10((double)(int64)(base + code), e),        e in 0..9,
// and the scan reads the codes.  div10(n, e) is n / 10^e in the three-FMA form for a constant divisor: q = n * r, rem = fma(-q, d, n), q' = fma(rem, r, q) with
// d = 10^e and r = RN(1 / d).  (r is within half an ulp of 1 / d and q within an ulp of n / d, so q' is the correctly rounded quotient -- Markstein's theorem -- and
// the tests compare it with the IEEE division bit for bit; the encoder does not rely on that: it keeps a code only when div10 gives back the row's bits.)  The IEEE
// division in its place (v_div_scale, v_rcp, eight FMAs, v_div_fmas, v_div_fixup per row) took the 11-byte Q1 scan off its memory limit: profiles/decimal_shadow.
// No device dependency.  ONE body for all of these: OP_DEC10 of the fused programs (fused_device.hpp: interpreter, ahead-of-time and run-time compiled kernels), the
// encoder's per-row check (kernels_encode.hip), the host twins (plx_encoding_decimal_decode / _encode, plx_encoding_choose_decimal) and the stand-alone sanitizer
// build (tests/emu/decimal_main.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifndef PLX_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define PLX_HD __host__ __device__
#else
#define PLX_HD
#endif
#endif

namespace plx {
namespace decimal {

constexpr int kMaxExp = 9;
constexpr int kNumExp = kMaxExp + 1;
constexpr double kIntLimit = 9007199254740992.0;      // 2^53: integers below it are exact doubles

PLX_HD inline double pow10(int e) {      // exact doubles, every one of them
  switch (e) {
    case 0: return 1.0; case 1: return 10.0; case 2: return 100.0; case 3: return 1000.0; case 4: return 10000.0;
    case 5: return 100000.0; case 6: return 1000000.0; case 7: return 10000000.0; case 8: return 100000000.0; default: return 1000000000.0;
  }
}
PLX_HD inline double recip10(int e) {    // RN(1 / 10^e): constant-folded, correctly rounded divisions
  switch (e) {
    case 0: return 1.0; case 1: return 1.0 / 10.0; case 2: return 1.0 / 100.0; case 3: return 1.0 / 1000.0; case 4: return 1.0 / 10000.0;
    case 5: return 1.0 / 100000.0; case 6: return 1.0 / 1000000.0; case 7: return 1.0 / 10000000.0; case 8: return 1.0 / 100000000.0; default: return 1.0 / 1000000000.0;
  }
}
PLX_HD inline uint64_t bits_of(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }

// n / 10^e for an integer-valued n, |n| < 2^53: a multiplication and two FMAs (the body of OP_DEC10)
PLX_HD inline double div10(double n, int e) {
  const double d = pow10(e), r = recip10(e);
  const double q = n * r;
  const double rem = fma(-q, d, n);
  return fma(rem, r, q);
}
// THE decode: one integer add, one conversion, div10
PLX_HD inline double decode(int64_t base, uint32_t code, int e) { return div10((double)(int64_t)((uint64_t)base + (uint64_t)code), e); }

// The integer `v` is stored as at exponent e: k = rint(v * 10^e), kept only when div10(k, e) gives back the bits of v.  False for NaN, +-inf, -0.0 (it would come back
// as +0.0), |k| >= 2^53 and every value that is no e-digit decimal.
PLX_HD inline bool quantize(double v, int e, int64_t* k) {
  const double s = v * pow10(e);
  if (!(s > -kIntLimit && s < kIntLimit)) return false;
  const int64_t q = (int64_t)rint(s);
  if (bits_of(div10((double)q, e)) != bits_of(v)) return false;
  *k = q;
  return true;
}

// What one pass over (a sample of) the valid rows learns: per exponent, whether every row seen is a decimal at it, and the range of the integers.
struct Stats {
  uint32_t fail;              // bit e: some row does not round-trip at exponent e
  uint32_t any;               // a valid row was seen
  int64_t mn[kNumExp], mx[kNumExp];
};
PLX_HD inline void stats_init(Stats& s) {
  s.fail = 0; s.any = 0;
  for (int e = 0; e < kNumExp; e++) { s.mn[e] = INT64_MAX; s.mx[e] = INT64_MIN; }
}
// exponents e_lo .. e_hi only (the full pass that follows a sample looks at the chosen one)
PLX_HD inline void stats_row(Stats& s, double v, int e_lo = 0, int e_hi = kMaxExp) {
  s.any = 1;
  for (int e = 0; e < kNumExp; e++) {      // (constant bounds: the kernel keeps mn / mx in registers)
    if (e < e_lo || e > e_hi || ((s.fail >> e) & 1u)) continue;
    int64_t k;
    if (!quantize(v, e, &k)) { s.fail |= 1u << e; continue; }
    if (k < s.mn[e]) s.mn[e] = k;
    if (k > s.mx[e]) s.mx[e] = k;
  }
}
PLX_HD inline void stats_merge(Stats& s, const Stats& o) {
  s.fail |= o.fail; s.any |= o.any;
  for (int e = 0; e < kNumExp; e++) { if (o.mn[e] < s.mn[e]) s.mn[e] = o.mn[e]; if (o.mx[e] > s.mx[e]) s.mx[e] = o.mx[e]; }
}

// The chooser: the smallest exponent e_lo <= e <= e_hi every row seen round-trips at; base 0 when the integers lie in [0, 2^32) (the scan then decodes in one op),
// else their minimum; nothing when no exponent does, no valid row was seen or the integers span 2^32 or more.
struct Choice { bool ok; int e; int64_t base; };
PLX_HD inline Choice choose(const Stats& s, int e_lo = 0, int e_hi = kMaxExp) {
  Choice c{false, 0, 0};
  if (!s.any) return c;
  for (int e = e_lo; e <= e_hi; e++) {
    if ((s.fail >> e) & 1u) continue;
    const int64_t mn = s.mn[e], mx = s.mx[e];
    if (mx < mn) return c;
    c.e = e;
    if (mn >= 0 && mx <= (int64_t)0xffffffffll) { c.ok = true; c.base = 0; return c; }
    if ((uint64_t)mx - (uint64_t)mn > 0xffffffffull) return c;      // (|k| < 2^53: the difference cannot wrap)
    c.ok = true; c.base = mn;
    return c;
  }
  return c;
}

// the code of one row under a choice, or false (the encoder's mismatch): not a decimal at e, or outside [base, base + 2^32)
PLX_HD inline bool encode_row(double v, int64_t base, int e, uint32_t* code) {
  int64_t k;
  if (!quantize(v, e, &k)) return false;
  const uint64_t d = (uint64_t)k - (uint64_t)base;
  if (k < base || d > 0xffffffffull) return false;
  *code = (uint32_t)d;
  return bits_of(decode(base, (uint32_t)d, e)) == bits_of(v);
}

}  // namespace decimal
}  // namespace plx
