// temporal.hpp -- the parts of a Date / Datetime value (dt.year, month, day, quarter, weekday, ordinal_day, hour, minute, second, date), ONE body for the fused
// programs' OP_DATEPART (interpreter, ahead-of-time and run-time compiled kernels), the per-node kernel (kernels_temporal.hip) and the host entry
// (plx_temporal_part_host), so that a CPU test of the host entry is a test of the kernels' arithmetic.
//
// A Date is i32 days since 1970-01-01, a Datetime i64 ticks (ms / us / ns) since 1970-01-01T00:00 (crates/polars-core/src/datatypes/time_unit.rs).  days =
// floor(ticks / ticks_per_day) -- a floor, so an instant before the epoch lands on its own day -- and the time of day is ticks - days * ticks_per_day.  The calendar is
// the proleptic Gregorian one, days -> (year, month, day) by the era decomposition (an era is 400 years = 146097 days, counted from 0000-03-01).  Defined for EVERY
// input: no signed operation here can overflow (years of a ms Datetime run to about +-2.9e8; only `date` of a ms Datetime can leave i32, and wraps like the cast it is).
//
// Cost: the unit and the part are compile-time constants wherever a program is (Op::c travels in Shape), so every divisor is a constant and a division is a
// multiply-high sequence; a 64-bit division by a RUN-TIME value is a ~100-instruction routine on gfx950 and appears nowhere.  At most two 64-bit constant divisions are
// paid (ticks -> days, days -> era; a Date pays the second only, us / ns Datetimes keep the second in 32 bits); everything after the era is 32-bit (doe < 146097).
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
namespace temporal {

// plx_time_unit
constexpr int kUnitDate = 0, kUnitMs = 1, kUnitUs = 2, kUnitNs = 3;
constexpr int kNumUnits = 4;
// plx_temporal_part
constexpr int kYear = 0, kMonth = 1, kDay = 2, kQuarter = 3, kWeekday = 4, kOrdinalDay = 5, kHour = 6, kMinute = 7, kSecond = 8, kDatePart = 9;
constexpr int kNumParts = 10;

// Op::c of OP_DATEPART: part in the low four bits, unit in the two bits above
PLX_HD constexpr uint8_t pack(int part, int unit) { return (uint8_t)((part & 15) | ((unit & 3) << 4)); }
PLX_HD constexpr int part_of(uint8_t c) { return c & 15; }
PLX_HD constexpr int unit_of(uint8_t c) { return (c >> 4) & 3; }

PLX_HD constexpr bool unit_ok(int unit) { return unit >= 0 && unit < kNumUnits; }
// the time-of-day parts and `date` exist for a Datetime only
PLX_HD constexpr bool part_ok(int part, int unit) { return unit_ok(unit) && part >= 0 && part < kNumParts && (unit != kUnitDate || part < kHour); }
PLX_HD constexpr int64_t ticks_per_second(int unit) { return unit == kUnitMs ? 1000ll : unit == kUnitUs ? 1000000ll : unit == kUnitNs ? 1000000000ll : 0ll; }
PLX_HD constexpr int64_t ticks_per_day(int unit) { return unit == kUnitDate ? 1ll : 86400ll * ticks_per_second(unit); }
// width in bytes of a part's output (year Int32, ordinal_day Int16, date = Date = i32, the rest Int8)
PLX_HD constexpr int part_width(int part) { return (part == kYear || part == kDatePart) ? 4 : part == kOrdinalDay ? 2 : 1; }
constexpr int64_t kI32Min = -2147483647ll - 1, kI32Max = 2147483647ll;
// smallest / largest value a part can take, whatever the data (year and date: the whole i32)
PLX_HD constexpr int64_t part_min(int part) { return (part == kYear || part == kDatePart) ? kI32Min : (part >= kHour && part <= kSecond) ? 0 : 1; }
PLX_HD constexpr int64_t part_max(int part) {
  switch (part) {
    case kMonth: return 12; case kDay: return 31; case kQuarter: return 4; case kWeekday: return 7; case kOrdinalDay: return 366;
    case kHour: return 23; case kMinute: case kSecond: return 59;
    default: return kI32Max;
  }
}

constexpr int64_t kDaysPerEra = 146097;      // 400 years; a multiple of 7
constexpr int64_t kEpochShift = 719468;      // days from 0000-03-01 to 1970-01-01

// floor(x / D) for a constant D > 0: the truncating quotient (a multiply-high sequence), one less when the remainder is negative.  q * D never leaves [x, 0].
template <int64_t D> PLX_HD inline int64_t floor_div(int64_t x) {
  const int64_t q = x / D;
  return q - ((x - q * D) < 0 ? 1 : 0);
}

#if defined(__GNUC__) || defined(__clang__)
#define PLX_TEMPORAL_INLINE inline __attribute__((always_inline))
#else
#define PLX_TEMPORAL_INLINE inline
#endif

// THE function: part `part` of value `v` in unit `unit`, as the 64-bit widening of the part's output dtype.
//
// ONE body, written over run-time `unit` and `part` and always inlined.  Where they are constants (Op::c of a compiled program's Shape, the template arguments of
// the per-node kernels) every branch below folds and one part's chain with its constant divisors is left; where they are run-time values (the generic interpreter,
// the host entry) the branches are wave-uniform and the body holds each division ONCE -- three ticks -> days, three time of day -> seconds, two days -> era, one
// calendar chain -- not once per (unit, part) pair: 40 specialised chains inside the interpreter's switch cost its kernels scratch and hundreds of spilled SGPRs
// (the divisors' magic numbers are hoisted out of the row loop).
// A time-of-day part or `date` of a Date is refused upstream (part_ok) and evaluates as if the Date were a Datetime at midnight (0, 0, 0, the day itself).
PLX_HD PLX_TEMPORAL_INLINE int64_t part(int64_t v, int unit, int part) {
  int64_t days;
  switch (unit) {
    case kUnitMs: days = floor_div<ticks_per_day(kUnitMs)>(v); break;
    case kUnitUs: days = floor_div<ticks_per_day(kUnitUs)>(v); break;
    case kUnitNs: days = floor_div<ticks_per_day(kUnitNs)>(v); break;
    default: days = (int64_t)(int32_t)v; break;      // (a Date slot holds the sign extension of its 32 bits: the truncation only states the range)
  }
  if (part == kDatePart) return (int64_t)(int32_t)(uint32_t)(uint64_t)days;      // the day count as a Date: its low 32 bits (all of it but for a ms Datetime beyond +-5.8e6 years)
  if (part >= kHour) {      // kHour, kMinute, kSecond: seconds since midnight, 0..86399, first
    const uint64_t tod = (uint64_t)v - (uint64_t)days * (uint64_t)ticks_per_day(unit);      // 0 <= tod < ticks_per_day, exact in wrapping arithmetic
    uint32_t s;
    switch (unit) {
      case kUnitMs: s = (uint32_t)tod / 1000u; break;      // tod < 8.64e7: 32 bits
      case kUnitUs: s = (uint32_t)(tod / 1000000ull); break;
      case kUnitNs: s = (uint32_t)(tod / 1000000000ull); break;
      default: s = 0u; break;
    }
    return part == kHour ? (int64_t)(s / 3600u) : part == kMinute ? (int64_t)((s / 60u) % 60u) : (int64_t)(s % 60u);
  }
  // The calendar parts of the day count.  It is biased by a whole number of eras into the non-negative numbers first, so the era split is one UNSIGNED division and doe
  // is its remainder; 146097 = 7 * 20871, so the bias leaves the weekday alone too.  The day count of a Date (33 bits with the bias) and of a ms Datetime (|days| <
  // 1.07e11: 2^20 eras = 1.53e11 days cover it) divide in 64 bits; for us (|days| < 1.07e8) and ns (|days| < 1.07e5) 1024 eras = 1.5e8 days keep the biased count
  // inside 32 bits.
  uint32_t doe;
  int32_t era;
  if (unit == kUnitUs || unit == kUnitNs) {
    constexpr int32_t kBiasEras = 1 << 10;
    const uint32_t z = (uint32_t)((int32_t)days + (int32_t)kEpochShift + kBiasEras * (int32_t)kDaysPerEra);
    const uint32_t e = z / (uint32_t)kDaysPerEra;
    doe = z - e * (uint32_t)kDaysPerEra;
    era = (int32_t)e - kBiasEras;
  } else {
    constexpr int64_t kBiasEras = 1 << 20;
    const uint64_t z = (uint64_t)(days + kEpochShift + kBiasEras * kDaysPerEra);
    const uint64_t e = z / (uint64_t)kDaysPerEra;
    doe = (uint32_t)(z - e * (uint64_t)kDaysPerEra);
    era = (int32_t)e - (int32_t)kBiasEras;
  }
  // ISO weekday, Monday = 1: floormod(days + 3, 7) + 1, and days + 3 = doe + 2 (mod 7) because kEpochShift = 1 and kDaysPerEra = 0 (mod 7)
  if (part == kWeekday) return (int64_t)((doe + 2u) % 7u) + 1;
  const uint32_t yoe = (doe - doe / 1460u + doe / 36524u - doe / 146096u) / 365u;      // 0..399
  const uint32_t doy = doe - (365u * yoe + yoe / 4u - yoe / 100u);                       // 0..365, counted from 1 March
  const uint32_t mp = (5u * doy + 2u) / 153u;                                            // 0..11, March = 0
  if (part == kDay) return (int64_t)(doy - (153u * mp + 2u) / 5u) + 1;
  const uint32_t m = mp < 10u ? mp + 3u : mp - 9u;
  if (part == kMonth) return (int64_t)m;
  if (part == kQuarter) return (int64_t)((m + 2u) / 3u);
  if (part == kOrdinalDay) {
    // January and February belong to the civil year AFTER the March-based one: 1 January is doy 306.  From March on the civil year is yoe's, and it is a leap
    // year when yoe is (yoe = 0 is a multiple of 400)
    const bool leap = (yoe & 3u) == 0u && (yoe % 100u != 0u || yoe == 0u);
    return mp >= 10u ? (int64_t)doy - 305 : (int64_t)doy + 60 + (leap ? 1 : 0);
  }
  return (int64_t)((int32_t)yoe + era * 400 + (m <= 2u ? 1 : 0));      // kYear: |era| < 7.4e5 (ms), so |year| < 2.95e8
}

// the same with unit and part as template arguments (the per-node kernels)
template <int UNIT, int PART> PLX_HD PLX_TEMPORAL_INLINE int64_t part_static(int64_t v) { return part(v, UNIT, PART); }

}  // namespace temporal
}  // namespace plx
