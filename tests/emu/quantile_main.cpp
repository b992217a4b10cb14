// quantile_main.cpp -- stand-alone driver of the median / quantile arithmetic (polars_amd/csrc/quantile.hpp: rank_of, combine, the sort's value code and its
// inverse -- the one body of segment_quantile_kernel, of the encode kernels and of ops::reduce_quantile), built with -fsanitize=address,undefined by the tests.
// (TEST INFRASTRUCTURE: never linked into libpolars_amd.so.)
//
// What it is checked against is a straightforward sort-and-index computation written out here from the contract, not from the header:
//   (1) random sizes 0..70 (0: nothing to rank, the callers' null), all five interpolations, q in {0, 1, 0.5, 0.25, 1/3, 0.999}: std::sort, then the rule;
//       results compared bit for bit (the same operations in the same order).
//   (2) the ranks stay inside [0, n) and lo <= hi <= lo + 1 for every n up to 70 and a few large n (2^32 - 2 among them).
//   (3) nearest: a tie goes up (n = 2, 6 at q = 0.5; n = 3 at q = 0.25).
//   (4) encode -> decode round trips at the edges: INT64_MIN / INT64_MAX, UINT64_MAX, +-0.0 (one code, decoded as +0.0), +-inf, NaN (one code, the greatest),
//       f32 denormals; the codes are ordered like the values, every narrow dtype included.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../../polars_amd/csrc/quantile.hpp"

using namespace plx::quantile;

static long long bad = 0, checked = 0;
static void expect(bool ok, const char* what, double got, double want) {
  checked++;
  if (!ok && bad++ < 20) fprintf(stderr, "%s: got %.17g, want %.17g\n", what, got, want);
}
static bool same_bits(double a, double b) { return !memcmp(&a, &b, 8) || (a != a && b != b); }

// the contract, from its text
static double reference(std::vector<double> v, double q, int interpolation) {
  std::sort(v.begin(), v.end());
  const size_t n = v.size();
  const double pos = (double)(n - 1) * q;
  size_t lo = (size_t)std::floor(pos), hi = (size_t)std::ceil(pos);
  lo = std::min(lo, n - 1); hi = std::min(hi, n - 1);
  const double a = v[lo], b = v[hi];
  switch (interpolation) {
    case PLX_QUANTILE_LOWER: return a;
    case PLX_QUANTILE_HIGHER: return b;
    case PLX_QUANTILE_NEAREST: return v[std::min((size_t)std::floor(pos + 0.5), n - 1)];
    case PLX_QUANTILE_MIDPOINT: return a == b ? a : (a + b) / 2.0;
    default: return (a == b || lo == hi) ? a : (pos - (double)lo) * (b - a) + a;
  }
}

template <typename T>
static uint64_t code_of(int dtype, T v) { return encode_value(dtype, &v, 0); }

template <typename T>
static void ordered_round_trip(int dtype, std::vector<T> vals, const char* what) {
  std::sort(vals.begin(), vals.end());
  for (size_t i = 0; i < vals.size(); i++) {
    const uint64_t c = code_of(dtype, vals[i]);
    expect(decode(dtype, c) == (double)vals[i], what, decode(dtype, c), (double)vals[i]);
    if (i) expect(vals[i - 1] == vals[i] ? code_of(dtype, vals[i - 1]) == c : code_of(dtype, vals[i - 1]) < c, what, (double)i, (double)vals[i]);
  }
}

int main() {
  std::mt19937_64 rng(415);
  const double qs[6] = {0.0, 1.0, 0.5, 0.25, 1.0 / 3.0, 0.999};
  // (1) + (2)
  for (int rep = 0; rep < 40; rep++) {
    for (size_t n = 0; n <= 70; n++) {
      std::vector<double> v(n);
      for (auto& x : v) x = (rng() % 4 == 0) ? (double)(int)(rng() % 7) : std::ldexp((double)(int64_t)rng(), -40);      // ties and spread values
      if (n == 0) { expect(v.empty(), "empty", 0, 0); continue; }
      std::vector<double> s = v;
      std::sort(s.begin(), s.end());
      for (int it = 0; it < 5; it++)
        for (double q : qs) {
          const Rank r = rank_of((uint64_t)n, q, it);
          expect(r.lo < n && r.hi < n && r.lo <= r.hi && r.hi <= r.lo + 1 && r.frac >= 0.0 && r.frac < 1.0, "rank bounds", (double)r.lo, (double)r.hi);
          const double got = combine(s[r.lo], s[r.hi], r.frac, it), want = reference(v, q, it);
          expect(same_bits(got, want), "quantile", got, want);
        }
    }
  }
  for (uint64_t n : {(uint64_t)1 << 20, ((uint64_t)1 << 31) + 7, ((uint64_t)1 << 32) - 2})
    for (int it = 0; it < 5; it++)
      for (double q : qs) {
        const Rank r = rank_of(n, q, it);
        expect(r.lo < n && r.hi < n && r.lo <= r.hi && r.hi <= r.lo + 1, "rank bounds (large n)", (double)r.lo, (double)r.hi);
      }
  // (3)
  expect(rank_of(2, 0.5, PLX_QUANTILE_NEAREST).lo == 1, "nearest n=2", (double)rank_of(2, 0.5, PLX_QUANTILE_NEAREST).lo, 1);
  expect(rank_of(6, 0.5, PLX_QUANTILE_NEAREST).lo == 3, "nearest n=6", (double)rank_of(6, 0.5, PLX_QUANTILE_NEAREST).lo, 3);
  expect(rank_of(3, 0.25, PLX_QUANTILE_NEAREST).lo == 1, "nearest n=3", (double)rank_of(3, 0.25, PLX_QUANTILE_NEAREST).lo, 1);
  expect(!q_ok(std::nan("")) && !q_ok(-0.1) && !q_ok(1.0000001) && q_ok(0.0) && q_ok(1.0), "q_ok", 0, 0);
  expect(!interpolation_ok(-1) && !interpolation_ok(5) && interpolation_ok(0) && interpolation_ok(4), "interpolation_ok", 0, 0);
  // NaN is an ordinary, largest element; infinities of both signs make a NaN midpoint, as the rule says
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  expect(combine(1.0, nan, 0.5, PLX_QUANTILE_HIGHER) != combine(1.0, nan, 0.5, PLX_QUANTILE_HIGHER), "higher NaN", 0, 0);
  expect(combine(nan, nan, 0.0, PLX_QUANTILE_LINEAR) != combine(nan, nan, 0.0, PLX_QUANTILE_LINEAR), "linear NaN", 0, 0);
  expect(combine(1.0, 3.0, 0.0, PLX_QUANTILE_LINEAR) == 1.0 && combine(1.0, inf, 0.0, PLX_QUANTILE_LINEAR) == 1.0, "linear lo == hi", 0, 0);
  expect(std::isnan(combine(-inf, inf, 0.5, PLX_QUANTILE_MIDPOINT)) && combine(inf, inf, 0.5, PLX_QUANTILE_MIDPOINT) == inf, "midpoint inf", 0, 0);
  // (4)
  const int64_t i64min = std::numeric_limits<int64_t>::min(), i64max = std::numeric_limits<int64_t>::max();
  expect(code_of<int64_t>(PLX_I64, i64min) == 0 && code_of<int64_t>(PLX_I64, i64max) == ~0ull, "i64 code ends", 0, 0);
  expect(decode(PLX_I64, code_of<int64_t>(PLX_I64, i64min)) == -9223372036854775808.0 && decode(PLX_I64, code_of<int64_t>(PLX_I64, i64max)) == 9223372036854775808.0, "i64 ends decode", 0, 0);
  expect(code_of<int64_t>(PLX_I64, ((int64_t)1 << 53) + 1) == code_of<int64_t>(PLX_I64, (int64_t)1 << 53) + 1, "i64 above 2^53 stays exact as a code", 0, 0);
  expect(code_of<uint64_t>(PLX_U64, ~0ull) == ~0ull && decode(PLX_U64, ~0ull) == 18446744073709551616.0, "u64 max", decode(PLX_U64, ~0ull), 18446744073709551616.0);
  ordered_round_trip<int8_t>(PLX_I8, {-128, -1, 0, 1, 127}, "i8");
  ordered_round_trip<int16_t>(PLX_I16, {-32768, -1, 0, 1, 32767}, "i16");
  ordered_round_trip<int32_t>(PLX_I32, {std::numeric_limits<int32_t>::min(), -1, 0, 1, std::numeric_limits<int32_t>::max()}, "i32");
  ordered_round_trip<int64_t>(PLX_I64, {i64min, -((int64_t)1 << 53), -1, 0, 1, (int64_t)1 << 53, i64max}, "i64");
  ordered_round_trip<uint8_t>(PLX_U8, {0, 1, 255}, "u8");
  ordered_round_trip<uint16_t>(PLX_U16, {0, 1, 65535}, "u16");
  ordered_round_trip<uint32_t>(PLX_U32, {0u, 1u, 0xffffffffu}, "u32");
  ordered_round_trip<uint64_t>(PLX_U64, {0ull, 1ull, 1ull << 63, ~0ull}, "u64");
  const float fden = std::numeric_limits<float>::denorm_min();
  ordered_round_trip<float>(PLX_F32, {-std::numeric_limits<float>::infinity(), -1.5f, -fden, 0.0f, fden, std::numeric_limits<float>::min(), 1.5f, std::numeric_limits<float>::infinity()}, "f32");
  ordered_round_trip<double>(PLX_F64, {-inf, -1e300, -std::numeric_limits<double>::denorm_min(), 0.0, std::numeric_limits<double>::denorm_min(), 1e300, inf}, "f64");
  expect(code_of<double>(PLX_F64, -0.0) == code_of<double>(PLX_F64, 0.0) && !std::signbit(decode(PLX_F64, code_of<double>(PLX_F64, -0.0))), "-0 == +0", 0, 0);
  expect(code_of<float>(PLX_F32, -0.0f) == code_of<float>(PLX_F32, 0.0f), "-0f == +0f", 0, 0);
  expect(code_of<double>(PLX_F64, nan) == code_of<double>(PLX_F64, -nan) && code_of<double>(PLX_F64, nan) > code_of<double>(PLX_F64, inf) && std::isnan(decode(PLX_F64, code_of<double>(PLX_F64, nan))), "NaN greatest, one code", 0, 0);
  expect(code_of<float>(PLX_F32, std::nanf("")) == code_of<double>(PLX_F64, nan), "f32 NaN is the same code", 0, 0);
  expect((float)decode(PLX_F32, code_of<float>(PLX_F32, fden)) == fden && decode(PLX_F32, code_of<float>(PLX_F32, -fden)) == -(double)fden, "f32 denormal round trip", 0, 0);
  printf("checked=%lld bad=%lld\n", checked, bad);
  return bad ? 1 : 0;
}
