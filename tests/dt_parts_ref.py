"""The reference of every dt-part check, and the corpus they run over.  (TEST INFRASTRUCTURE.)

Reference: days = floor(ticks / ticks_per_day) and the time of day by numpy integer floor division; (year, month, day) by the civil-from-days formulas (the era
decomposition of a proleptic Gregorian day count) on int64 arrays.  The formulas are the reference -- not numpy's datetime64 casts, which overflow within one day of
INT64_MIN -- and `self_check` validates them on the CPU against numpy's casts (|ticks| < 2^62) and pyarrow.compute (years 1..9999).

Corpus: about 300 boundary values per unit plus random fill (see `corpus`).
"""
import numpy as np

UNITS = ("date", "ms", "us", "ns")                       # plx_time_unit 0..3
PARTS = ("year", "month", "day", "quarter", "weekday", "ordinal_day", "hour", "minute", "second", "date")      # plx_temporal_part_kind 0..9
DATETIME_ONLY = ("hour", "minute", "second", "date")
TICKS_PER_DAY = {"date": 1, "ms": 86_400_000, "us": 86_400_000_000, "ns": 86_400_000_000_000}
OUT_NP = {"year": np.int32, "ordinal_day": np.int16, "date": np.int32}      # every other part: int8
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def out_dtype(part):
    return OUT_NP.get(part, np.int8)


def parts_of(unit, part):
    return part not in DATETIME_ONLY or unit != "date"


def civil_from_days(days):
    """(year, month, day, day of the March-based year) of int64 day counts since 1970-01-01; no intermediate leaves int64 for |days| < 2^62."""
    z = days.astype(np.int64) + 719468
    era = z // 146097                                    # numpy // is a floor
    doe = z - era * 146097                               # [0, 146096]
    yoe = (doe - doe // 1460 + doe // 36524 - doe // 146096) // 365      # [0, 399]
    doy = doe - (365 * yoe + yoe // 4 - yoe // 100)      # [0, 365]
    mp = (5 * doy + 2) // 153                            # [0, 11]
    d = doy - (153 * mp + 2) // 5 + 1
    m = np.where(mp < 10, mp + 3, mp - 9)
    y = yoe + era * 400 + (m <= 2)
    return y, m, d


def days_from_civil(y, m, d):
    """The inverse, for building the corpus (python ints)."""
    y -= m <= 2
    era = y // 400
    yoe = y - era * 400
    doy = (153 * (m + (-3 if m > 2 else 9)) + 2) // 5 + d - 1
    doe = yoe * 365 + yoe // 4 - yoe // 100 + doy
    return era * 146097 + doe - 719468


def part(values, unit, name):
    """The reference: part `name` of `values` (int32 days for unit "date", int64 ticks otherwise), in the part's output dtype."""
    v = np.asarray(values).astype(np.int64)
    tpd = TICKS_PER_DAY[unit]
    days = v // tpd
    tod = v - days * tpd
    if name in ("hour", "minute", "second"):
        s = tod // (tpd // 86400) if unit != "date" else np.zeros_like(v)
        r = {"hour": s // 3600, "minute": s // 60 % 60, "second": s % 60}[name]
    elif name == "date":
        r = days
    elif name == "weekday":
        r = (days + 3) % 7 + 1                           # numpy % is a floor-mod; ISO Monday = 1
    else:
        y, m, d = civil_from_days(days)
        if name == "year":
            r = y
        elif name == "month":
            r = m
        elif name == "day":
            r = d
        elif name == "quarter":
            r = (m - 1) // 3 + 1
        else:                                            # ordinal_day: days since 1 January of the civil year, by the cumulative month lengths
            leap = ((y % 4 == 0) & (y % 100 != 0)) | (y % 400 == 0)
            cum = np.array([0, 31, 59, 90, 120, 151, 181, 212, 243, 273, 304, 334])
            r = cum[m - 1] + d + (leap & (m > 2))
    return r.astype(out_dtype(name))                     # (date of a ms Datetime beyond +-5.8e6 years: the low 32 bits, as the cast)


def self_check():
    """The formulas against numpy's datetime64 casts and pyarrow.compute; raises AssertionError."""
    import pyarrow as pa
    import pyarrow.compute as pc
    rng = np.random.default_rng(7)
    d = np.concatenate([corpus("date")[0].astype(np.int64), rng.integers(-(1 << 31), 1 << 31, 200_000)])
    y, m, dd = civil_from_days(d)
    D = d.astype("M8[D]")
    M, Y = D.astype("M8[M]"), D.astype("M8[Y]")
    assert np.array_equal(y, Y.astype(np.int64) + 1970) and np.array_equal(m, M.astype(np.int64) - Y.astype("M8[M]").astype(np.int64) + 1)
    assert np.array_equal(dd, (D - M.astype("M8[D]")).astype(np.int64) + 1)
    assert np.array_equal(part(d, "date", "ordinal_day"), ((D - Y.astype("M8[D]")).astype(np.int64) + 1).astype(np.int16))
    # the floor and the time of day, every Datetime unit, away from numpy's own overflow
    for unit in ("ms", "us", "ns"):
        t = np.concatenate([corpus(unit)[0], rng.integers(-(1 << 62), 1 << 62, 50_000)])
        t = t[np.abs(t.astype(np.float64)) < 2.0 ** 62]
        T = t.astype(f"M8[{unit}]")
        assert np.array_equal(part(t, unit, "date").astype(np.int64) if unit != "ms" else t // TICKS_PER_DAY[unit], T.astype("M8[D]").astype(np.int64))
        secs = (T - T.astype("M8[D]")).astype("m8[s]").astype(np.int64)
        assert np.array_equal(part(t, unit, "hour"), (secs // 3600).astype(np.int8)) and np.array_equal(part(t, unit, "second"), (secs % 60).astype(np.int8))
        assert np.array_equal(part(t, unit, "minute"), (secs // 60 % 60).astype(np.int8))
    # pyarrow over its own domain, years 1..9999
    d = d[(d >= -719162) & (d <= 2932896)].astype(np.int32)
    a = pa.array(d, pa.int32()).cast(pa.date32())
    for name, fn in (("year", pc.year), ("month", pc.month), ("day", pc.day), ("quarter", pc.quarter), ("ordinal_day", pc.day_of_year),
                     ("weekday", lambda x: pc.day_of_week(x, count_from_zero=False, week_start=1))):
        assert np.array_equal(part(d, "date", name).astype(np.int64), fn(a).to_numpy().astype(np.int64)), name
    t = d.astype(np.int64) * TICKS_PER_DAY["us"] + rng.integers(0, TICKS_PER_DAY["us"], len(d))
    a = pa.array(t, pa.int64()).cast(pa.timestamp("us"))
    for name, fn in (("year", pc.year), ("hour", pc.hour), ("minute", pc.minute), ("second", pc.second),
                     ("weekday", lambda x: pc.day_of_week(x, count_from_zero=False, week_start=1))):
        assert np.array_equal(part(t, "us", name).astype(np.int64), fn(a).to_numpy().astype(np.int64)), name


_corpus_cache = {}


def boundary_days():
    """The day counts at which the calendar arithmetic turns: python ints, some beyond i32 (the Datetime units need them)."""
    days = {0, 1, -1, 58, 59, 60, -719162, 2932896, -719468, -719469, -719467}      # the epoch, 1970's Feb / Mar edge, 0001-01-01, 9999-12-31, the start of era 0
    for y in (1896, 1900, 1904, 1996, 2000, 2004, 2096, 2100, 2104):                # 28 Feb, 29 Feb where there is one, 1 Mar: leap years and century years that are not
        mar1 = days_from_civil(y, 3, 1)
        days |= {mar1, mar1 - 1, days_from_civil(y, 2, 28)}
        assert (mar1 - 1 != days_from_civil(y, 2, 28)) == ((y % 4 == 0 and y % 100 != 0) or y % 400 == 0)
    for y in (2000, 2001):                                                           # a leap and a non-leap year: the year's ends and every month's
        days |= {days_from_civil(y, 12, 31), days_from_civil(y, 1, 1)}
        for mth in range(2, 13):
            days |= {days_from_civil(y, mth, 1), days_from_civil(y, mth, 1) - 1}
    for k in (1, -1):
        for off in (-1, 0, 1):
            days |= {k * 146097 + off, -719468 + k * 146097 + off}
    for y in (-5877641, 5881580, -292275055, 292278994, -290308, 294247, 1677, 2262):      # the years in which the units' ranges end
        days |= {days_from_civil(y, 6, 15), days_from_civil(y, 1, 1), days_from_civil(y, 12, 31)}
    return sorted(days)


def corpus(unit, nullable=False, n_random=60, seed=3):
    """(values, valid) of one unit: int32 days for "date", int64 ticks otherwise; valid is None, or a bool mask with a third of the rows null, boundary rows included.
    Boundary days; for a Datetime the same days as ticks at d * tpd - 1, d * tpd and d * tpd + tpd - 1; the ends of the dtype's range; random fill."""
    key = (unit, nullable, n_random, seed)
    if key not in _corpus_cache:
        rng = np.random.default_rng(seed + UNITS.index(unit))
        if unit == "date":
            lo, hi = -(1 << 31), (1 << 31) - 1
            near = {d + o for d in boundary_days() for o in (-1, 0, 1)}          # a Date has one value per day: the days on either side of each boundary as well
            vals = sorted(d for d in near if lo <= d <= hi) + [lo, hi, lo + 1, hi - 1]
            rnd = np.concatenate([rng.integers(lo, hi, n_random // 2), rng.integers(-20000, 40000, n_random - n_random // 2)])
            v = np.concatenate([np.array(vals, dtype=np.int64), rnd]).astype(np.int32)
        else:
            tpd = TICKS_PER_DAY[unit]
            vals = [I64_MIN, I64_MIN + 1, I64_MAX, I64_MAX - 1, -1, 0, 1]
            for d in boundary_days():
                vals += [t for t in (d * tpd - 1, d * tpd, d * tpd + tpd - 1) if I64_MIN <= t <= I64_MAX]
            rnd = np.concatenate([rng.integers(I64_MIN, I64_MAX, n_random // 2), rng.integers(-20000 * tpd, 40000 * tpd, n_random - n_random // 2)])
            v = np.concatenate([np.array(sorted(set(vals)), dtype=np.int64), rnd])
        valid = None
        if nullable:
            valid = np.random.default_rng(seed + 100).random(len(v)) >= 1 / 3
            valid[:: 7] = False                           # boundary rows among the nulls, whatever the draw
        _corpus_cache[key] = (v, valid)
    v, valid = _corpus_cache[key]
    return v.copy(), None if valid is None else valid.copy()


def padded(unit, n, nullable=False, seed=11):
    """The corpus cut or padded with random values to exactly n rows (boundary values first)."""
    v, valid = corpus(unit, nullable)
    if len(v) < n:
        rng = np.random.default_rng(seed)
        lo, hi = ((-(1 << 31), (1 << 31) - 1) if unit == "date" else (I64_MIN, I64_MAX))
        v = np.concatenate([v, rng.integers(lo, hi, n - len(v)).astype(v.dtype)])
        if valid is not None:
            valid = np.concatenate([valid, rng.random(n - len(valid)) >= 1 / 3])
    return v[:n], None if valid is None else valid[:n]


def write_corpus_file(path):
    """The file tests/emu/temporal_main.cpp reads: per unit a u64 count, then the values as i64."""
    with open(path, "wb") as f:
        for unit in UNITS:
            v = corpus(unit)[0].astype(np.int64)
            f.write(np.uint64(len(v)).tobytes()); f.write(v.tobytes())
