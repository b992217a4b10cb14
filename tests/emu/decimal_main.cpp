// decimal_main.cpp -- stand-alone driver of the decimal-shadow arithmetic (polars_amd/csrc/decimal.hpp: quantize, decode, the chooser and the encoder's per-row
// check), built with -fsanitize=address,undefined by the tests: an overflow or an out-of-range float -> integer conversion anywhere in the header aborts the process.
// (TEST INFRASTRUCTURE: never linked into libpolars_amd.so.)
//
// The edge values: NaN, +-inf, -0.0, the 2^53 limit on both sides, a span of exactly 2^32, negative ranges, subnormals and the extremes of f64, the non-decimal
// 0.1 + 0.2, a value that needs ten digits; then decode against a long-double division, an encode / decode round trip over random integers at every exponent, and div10 (the
// three-FMA form) against the IEEE division.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../polars_amd/csrc/decimal.hpp"

using namespace plx::decimal;

static long long bad = 0, checked = 0;
static void expect(bool cond, const char* what, double v = 0.0) {
  checked++;
  if (!cond && bad++ < 20) fprintf(stderr, "FAILED: %s (%.17g)\n", what, v);
}

static Choice choose_rows(const std::vector<double>& rows) {
  std::vector<double> heap(rows);      // a heap block of exactly the rows' size
  Stats st;
  stats_init(st);
  for (double v : heap) stats_row(st, v);
  return choose(st);
}

static uint64_t rng_state = 0x243f6a8885a308d3ull;
static uint64_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double two53 = 9007199254740992.0;
  // ---- the chooser -------------------------------------------------------------------------------------------------------------------------------------------------
  { const Choice c = choose_rows({1.25, 3.5, 100.0}); expect(c.ok && c.e == 2 && c.base == 0, "smallest exponent 2, base 0"); }
  { const Choice c = choose_rows({7.0, 0.0, 4294967295.0}); expect(c.ok && c.e == 0 && c.base == 0, "integers up to 2^32 - 1: exponent 0, base 0"); }
  { const Choice c = choose_rows({0.0, 4294967296.0}); expect(!c.ok, "a span of 2^32 does not encode"); }
  { const Choice c = choose_rows({1.0, 4294967296.0}); expect(c.ok && c.e == 0 && c.base == 1, "past 2^32 with a base"); }
  { const Choice c = choose_rows({-12.5, 3.0}); expect(c.ok && c.e == 1 && c.base == -125, "negative values: base = min"); }
  { const Choice c = choose_rows({-two53 + 1.0, -two53 + 100.0}); expect(c.ok && c.e == 0 && c.base == -9007199254740991ll, "the most negative integers that encode"); }
  { const Choice c = choose_rows({two53}); expect(!c.ok, "|k| = 2^53 does not encode", two53); }
  { const Choice c = choose_rows({-two53}); expect(!c.ok, "|k| = 2^53 does not encode", -two53); }
  { const Choice c = choose_rows({two53 - 1.0}); expect(c.ok && c.e == 0 && c.base == 9007199254740991ll, "2^53 - 1 encodes"); }
  { const Choice c = choose_rows({1.5, nan}); expect(!c.ok, "NaN"); }
  { const Choice c = choose_rows({1.5, inf}); expect(!c.ok, "+inf"); }
  { const Choice c = choose_rows({-inf}); expect(!c.ok, "-inf"); }
  { const Choice c = choose_rows({1.5, -0.0}); expect(!c.ok, "-0.0 would decode to +0.0"); }
  { const Choice c = choose_rows({0.0}); expect(c.ok && c.e == 0 && c.base == 0, "+0.0"); }
  { const Choice c = choose_rows({0.1 + 0.2}); expect(!c.ok, "0.1 + 0.2 is no decimal of nine digits", 0.1 + 0.2); }
  { const Choice c = choose_rows({0.3}); expect(c.ok && c.e == 1, "0.3 is one"); }
  { const Choice c = choose_rows({1e-10}); expect(!c.ok, "ten digits"); }
  { const Choice c = choose_rows({1e-9, 0.5}); expect(c.ok && c.e == 9 && c.base == 0, "nine digits"); }
  { const Choice c = choose_rows({std::numeric_limits<double>::denorm_min()}); expect(!c.ok, "a subnormal"); }
  { const Choice c = choose_rows({std::numeric_limits<double>::max()}); expect(!c.ok, "the largest double"); }
  { const Choice c = choose_rows({-std::numeric_limits<double>::max()}); expect(!c.ok, "the smallest double"); }
  { const Choice c = choose_rows({}); expect(!c.ok, "no valid row"); }
  // exponents restricted to the chosen one (the full pass after a sample)
  {
    Stats st;
    stats_init(st);
    for (double v : {-1.25, 7.5}) stats_row(st, v, 2, 2);
    const Choice c = choose(st, 2, 2);
    expect(c.ok && c.e == 2 && c.base == -125, "one exponent only");
  }
  // ---- the per-row encoder -------------------------------------------------------------------------------------------------------------------------------------------
  {
    uint32_t code = 77;
    expect(encode_row(12.34, 0, 2, &code) && code == 1234, "12.34 at exponent 2");
    expect(!encode_row(-0.01, 0, 2, &code), "below the base");
    expect(encode_row(-0.01, -1, 2, &code) && code == 0, "the base itself");
    expect(encode_row(42949672.95, 0, 2, &code) && code == 0xffffffffu, "the last code");
    expect(!encode_row(42949672.96, 0, 2, &code), "one past the last code");
    expect(!encode_row(nan, 0, 2, &code) && !encode_row(inf, 0, 2, &code) && !encode_row(-0.0, 0, 2, &code) && !encode_row(0.1 + 0.2, 0, 9, &code), "NaN, inf, -0.0, a non-decimal");
    expect(!encode_row(1e300, 0, 9, &code) && !encode_row(-1e300, INT64_MIN, 9, &code), "far outside");
    expect(encode_row(-9007199254740991.0, -9007199254740991ll, 0, &code) && code == 0, "the most negative integer");
  }
  // ---- decode against a long-double division; encode / decode round trip ---------------------------------------------------------------------------------------------
  for (int e = 0; e <= kMaxExp; e++) {
    long double p = 1.0L;
    for (int i = 0; i < e; i++) p *= 10.0L;
    for (int i = 0; i < 200000; i++) {
      const uint32_t code = (uint32_t)rng();
      const int64_t base = (i & 1) ? 0 : (int64_t)(rng() % (1ull << 51)) - (int64_t)(1ull << 50);      // |k| < 2^51: rint(v * 10^e) finds k again whatever the two roundings did
      const double got = decode(base, code, e);
      const double want = (double)((long double)(base + (int64_t)code) / p);      // 64-bit mantissa, then one more rounding: equal unless that double-rounds
      const double alt = std::nextafter(want, got);
      expect(got == want || got == alt, "decode against the long-double quotient", got);
      uint32_t back = 0;
      const bool ok = encode_row(got, base, e, &back);
      // a decoded value always has a code that decodes to the same bits: the one it came from, or the one of a smaller integer that divides to the same double
      expect(ok && bits_of(decode(base, back, e)) == bits_of(got), "round trip", got);
    }
  }
  // ---- div10 is the IEEE division: every price of the benchmark's range in cents, and 4e6 random integers below 2^53 at every exponent --------------------------------
  for (int64_t k = 0; k < 10500000; k++) expect(bits_of(div10((double)k, 2)) == bits_of((double)k / 100.0), "div10 against the division, cents", (double)k);
  for (int e = 0; e <= kMaxExp; e++)
    for (int i = 0; i < 400000; i++) {
      const double n = (double)((int64_t)(rng() >> 11) - ((i & 1) ? (int64_t)1 << 52 : 0));
      expect(bits_of(div10(n, e)) == bits_of(n / pow10(e)), "div10 against the division", n);
    }
  printf("checked=%lld bad=%lld\n", checked, bad);
  return bad ? 1 : 0;
}
