// temporal_main.cpp -- stand-alone driver of the date-part arithmetic (polars_amd/csrc/temporal.hpp: temporal::part, the one body of OP_DATEPART, of the per-node
// kernel and of plx_temporal_part_host), built with -fsanitize=undefined,address by the tests: a signed overflow anywhere in the header aborts the process.
// (TEST INFRASTRUCTURE: never linked into libpolars_amd.so.)
//
// What it is checked against shares nothing with the era formulas: a calendar WALKED day by day with plain counters (days per month, leap years by the 4 / 100 / 400
// rule, a weekday counter).  (1) every day of the years 1..4000 is walked directly; (2) any other day count is reduced by whole 400-year cycles (146097 days, a multiple
// of 7) into a table of one walked cycle; the day count and the time of day of a tick count come from 128-bit floor division.
// Inputs: the corpus file of the tests (per unit: u64 n, then n i64 values), 1e6 strided values per unit over the unit's whole range, and walk (1) in every unit.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../polars_amd/csrc/temporal.hpp"

using namespace plx::temporal;

struct Civil { int32_t year; int8_t month, day, weekday; int16_t ordinal; };

static bool is_leap(int64_t y) { return (y % 4 == 0 && y % 100 != 0) || y % 400 == 0; }
static int month_len(int64_t y, int m) { static const int len[12] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31}; return m == 2 && is_leap(y) ? 29 : len[m - 1]; }
static void step(Civil& c) {
  c.weekday = (int8_t)(c.weekday % 7 + 1);
  if (c.day < month_len(c.year, c.month)) { c.day++; c.ordinal++; return; }
  c.day = 1;
  if (c.month < 12) { c.month++; c.ordinal++; return; }
  c.month = 1; c.ordinal = 1; c.year++;
}

static std::vector<Civil> cycle;                 // the 146097 days from 2000-01-01 (a Saturday, day 10957 of the epoch)
static const int64_t kCycleStart = 10957;

static __int128 floor_div128(__int128 a, __int128 b) { __int128 q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }

static Civil civil_of_days(int64_t days) {
  const __int128 k = floor_div128((__int128)days - kCycleStart, 146097);
  Civil c = cycle[(size_t)((__int128)days - kCycleStart - k * 146097)];
  c.year = (int32_t)(c.year + 400 * k);
  return c;
}

static long long bad = 0, checked = 0;
static void expect(int unit, int part, int64_t v, int64_t got, int64_t want) {
  checked++;
  if (got != want && bad++ < 20) fprintf(stderr, "unit %d part %d value %lld: got %lld, want %lld\n", unit, part, (long long)v, (long long)got, (long long)want);
}

static void check_value(int unit, int64_t v, const Civil* known = nullptr) {
  const __int128 tpd = ticks_per_day(unit);
  const __int128 days128 = unit == kUnitDate ? (__int128)v : floor_div128(v, tpd);
  const int64_t days = (int64_t)days128;
  const Civil c = known ? *known : civil_of_days(days);
  expect(unit, kYear, v, part(v, unit, kYear), c.year);
  expect(unit, kMonth, v, part(v, unit, kMonth), c.month);
  expect(unit, kDay, v, part(v, unit, kDay), c.day);
  expect(unit, kQuarter, v, part(v, unit, kQuarter), (c.month - 1) / 3 + 1);
  expect(unit, kWeekday, v, part(v, unit, kWeekday), c.weekday);
  expect(unit, kOrdinalDay, v, part(v, unit, kOrdinalDay), c.ordinal);
  if (unit == kUnitDate) return;
  const __int128 tod = (__int128)v - days128 * tpd, tps = ticks_per_second(unit);
  const int64_t s = (int64_t)(tod / tps);
  expect(unit, kHour, v, part(v, unit, kHour), s / 3600);
  expect(unit, kMinute, v, part(v, unit, kMinute), s / 60 % 60);
  expect(unit, kSecond, v, part(v, unit, kSecond), s % 60);
  expect(unit, kDatePart, v, part(v, unit, kDatePart), (int64_t)(int32_t)(uint32_t)(uint64_t)days);
}

int main(int argc, char** argv) {
  // one walked 400-year cycle
  {
    Civil c{2000, 1, 1, 6, 1};
    cycle.reserve(146097);
    for (int i = 0; i < 146097; i++) { cycle.push_back(c); step(c); }
    if (c.year != 2400 || c.month != 1 || c.day != 1 || c.weekday != 6) { fprintf(stderr, "the walked cycle does not close\n"); return 3; }
  }
  // (1) every day of the years 1..4000, walked; 0001-01-01 is day -719162, a Monday.  Datetimes: midnight, and the last tick of the day
  {
    Civil c{1, 1, 1, 1, 1};
    for (int64_t d = -719162; c.year <= 4000; d++, step(c)) {
      if (d == 0 && !(c.year == 1970 && c.month == 1 && c.day == 1 && c.weekday == 4)) { fprintf(stderr, "the walk misses the epoch\n"); return 3; }
      check_value(kUnitDate, d, &c);
      for (int unit = kUnitMs; unit <= kUnitNs; unit++) {
        const int64_t tpd = ticks_per_day(unit);
        if (unit == kUnitNs && (d < -106751 || d > 106750)) continue;      // (beyond i64 nanoseconds)
        check_value(unit, d * tpd, &c);
        check_value(unit, d * tpd + (tpd - 1), &c);
      }
    }
  }
  // (2) 1e6 strided values over the whole range of each unit, both ends included
  for (int unit = 0; unit < kNumUnits; unit++) {
    const int n = 1000000;
    if (unit == kUnitDate) {
      for (int i = 0; i < n; i++) check_value(unit, (int64_t)INT32_MIN + (int64_t)i * 4294);
      check_value(unit, INT32_MAX); check_value(unit, INT32_MIN);
    } else {
      const uint64_t stride = 18446744073709ull;      // 2^64 / 1e6
      for (int i = 0; i < n; i++) check_value(unit, (int64_t)((uint64_t)INT64_MIN + (uint64_t)i * stride));
      check_value(unit, INT64_MAX); check_value(unit, INT64_MIN);
    }
  }
  // (3) the corpus of the tests
  if (argc == 2) {
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    for (int unit = 0; unit < kNumUnits; unit++) {
      uint64_t n = 0;
      if (fread(&n, 8, 1, f) != 1) return 3;
      std::vector<int64_t> v(n);
      if (n && fread(v.data(), 8, n, f) != n) return 3;
      for (uint64_t i = 0; i < n; i++) check_value(unit, v[i]);
    }
    fclose(f);
  }
  printf("checked=%lld bad=%lld\n", checked, bad);
  return bad ? 1 : 0;
}
