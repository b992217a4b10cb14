"""Tables and references for the stable arg-sort and the top-k selection (polars_amd/csrc/kernels_sort.hip) at the tile, digit, null and value edges that random
keys do not reach.  numpy only: the reference is the oracle's sort_indices (oracle/pyoracle.py, pinned by tests/test_oracle_golden.py); tests/test_sort_edges_cpu.py
pins the tables and the reference without a GPU and tests/test_gpu_sort_edges.py runs the tables through arg_sort_by and the frame front ends.

A key is the oracle's tuple (values, valid or None, descending, nulls_last)."""
import functools

import numpy as np

from oracle import pyoracle

# ---- the geometry the tables are built around, restated (tests/test_sort_edges_cpu.py compares them with the source) ----
BLOCK = 256               # kernels_sort.hip:41  `using k::kBlock` (kconfig.hpp:5): lanes of a workgroup, keys of a sub-tile
ITEMS = 16                # kernels_sort.hip:43  kItems: sub-tiles per workgroup
TILE = 4096               # kernels_sort.hip:44  kTile = kBlock * kItems: keys per workgroup and pass
IPT = 4                   # kernels_sort.hip:109 kIPT: keys per thread and ranking round
ROUND = 1024              # kernels_sort.hip:102 a ranking round is kIPT * kBlock keys
SMALL_BLOCK = 1024        # kernels_sort.hip:230 kSmallBlock: the one workgroup of the rank sort
SMALL_MAX = 2048          # kernels_sort.hip:231 kSmallMax: most rows the rank sort takes
SMALL_MAX_KEYS = 8        # kernels_sort.hip:232 kSmallMaxKeys: most keys the rank sort takes
SELECT_MIN_ROWS = 65536   # kernels_sort.hip:401 the selection needs n > 65536 ...
SELECT_LIMIT_DIV = 4      # kernels_sort.hip:401 ... and limit < n / 4
SELECT_KEEP_DIV = 2       # kernels_sort.hip:427 ... and keeps its candidates only when there are fewer than n / 2


def selects(n, limit):
    """the condition under which sort_indices starts the radix select"""
    return 0 <= limit < n // SELECT_LIMIT_DIV and n > SELECT_MIN_ROWS


NP = {"bool": np.bool_, "i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64, "u8": np.uint8, "u16": np.uint16, "u32": np.uint32, "u64": np.uint64,
      "f32": np.float32, "f64": np.float64}
PLDT = {"bool": "Boolean", "i8": "Int8", "i16": "Int16", "i32": "Int32", "i64": "Int64", "u8": "UInt8", "u16": "UInt16", "u32": "UInt32", "u64": "UInt64",
        "f32": "Float32", "f64": "Float64"}
DTYPES = list(NP)
FLOATS = ["f32", "f64"]
UNSIGNED = ["u8", "u16", "u32", "u64"]
NAN_BITS = {"f64": (0x7ff8000000000000, 0xfff8000000000001, 0x7ff0000000000001), "f32": (0x7fc00000, 0xffc00001, 0x7f800001)}     # quiet, negative with a payload, signalling
F32_DENORM = 2.0 ** -149


def width(dt):
    return 1 if dt == "bool" else np.dtype(NP[dt]).itemsize


def _uint_of(dt):
    return {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[width(dt)]


def from_bits(dt, bits):
    """values of dtype dt with exactly these bit patterns (no conversion ever touches them: a signalling NaN stays one)"""
    return np.array(bits, dtype=_uint_of(dt)).view(NP[dt])


def bits_of(a):
    return np.ascontiguousarray(a).view(_uint_of([k for k, t in NP.items() if np.dtype(t) == a.dtype][0]))


def byte_pairs(dt):
    """for every byte d of the dtype, two values whose bit patterns differ in byte d only (as floats: two finite normal numbers)"""
    w = width(dt)
    base = 0x3ff8111111111111 >> (8 * (8 - w)) if dt == "f64" else (0x3fc11111 if dt == "f32" else int.from_bytes(b"\x21" * w, "little"))
    flip = 0x04 if dt in FLOATS else 0x80          # the integer pairs also flip the sign bit in the top byte
    out = []
    for d in range(w):
        out += [base, base ^ (flip << (8 * d))]
    return from_bits(dt, out)


@functools.lru_cache(maxsize=None)
def base_values(dt):
    """the value edges of one dtype, every one once except the zeros of a float, which appear twice each"""
    if dt == "bool":
        return np.array([False, True])
    t = NP[dt]
    if dt in FLOATS:
        fi = np.finfo(t)
        up, down = t(np.inf), t(-np.inf)
        denorm = np.nextafter(t(0), up)
        vals = [-fi.max, np.nextafter(-fi.max, up), t(-1), t(0), t(1), np.nextafter(fi.max, down), fi.max,                   # min, min + 1, -1, 0, 1, max - 1, max
                up, down, fi.tiny, -fi.tiny, denorm, -denorm, t(F32_DENORM), t(-F32_DENORM), t(-0.0), t(-0.0), t(0.0), t(0.0)]
        return np.concatenate([np.array(vals, dtype=t), from_bits(dt, list(NAN_BITS[dt])), byte_pairs(dt)])
    ii = np.iinfo(t)
    vals = [ii.min, ii.min + 1, 0, 1, ii.max - 1, ii.max] + ([-1] if ii.min < 0 else [])
    return np.concatenate([np.array(vals, dtype=t), byte_pairs(dt)])


def value_table(dt, n):
    """base_values(dt) stretched to n rows: row i holds base value (i * step) % m for a step coprime with m, so neighbouring rows differ, every value returns every m
    rows (ties: the index vector that is compared shows whether they kept their row order) and any cut of the table holds the edges"""
    base = base_values(dt)
    m = len(base)
    step = next(s for s in range(max(m // 2, 1) | 1, 4 * m + 3, 2) if np.gcd(s, m) == 1)
    return base[(np.arange(n, dtype=np.int64) * step) % m]


# --------------------------------------------------------------------------------------------------------------- validity patterns
def _none(n): return None
def _third(n): v = np.ones(n, bool); v[2::3] = False; return v
def _all_null(n): return np.zeros(n, bool)
def _one_valid(n): v = np.zeros(n, bool); v[n // 2] = True; return v
def _words(n): return ((np.arange(n) >> 6) & 1) == 0


def _walk(n):
    """one valid bit per 64-row word: bit (7 w) % 64 of word w"""
    v = np.zeros(n, bool)
    w = np.arange((n + 63) // 64)
    rows = w * 64 + (7 * w) % 64
    v[rows[rows < n]] = True
    return v


VALIDITY = {"none": _none, "third": _third, "walk": _walk, "all_null": _all_null, "one_valid": _one_valid, "words": _words}


# ------------------------------------------------------------------------------------------------------------------------ digits
DIGIT_BASE = 0x4141414141414141
DIGIT_VARIANTS = ["all256", "two"]


def digit_keys(d, n, variant, signed=False):
    """n u64 (signed: i64, the same bits) keys that agree on every byte but byte d.  "all256": byte d takes all 256 values, scrambled; "two": 255 rows scattered over
    the table hold one value and the rest another, so the digit is nearly uniform and still has to be sorted."""
    i = np.arange(n, dtype=np.uint64)
    if variant == "all256":
        b = (i * np.uint64(97) + np.uint64(13)) % np.uint64(256)
    else:
        b = np.full(n, 0x9c, dtype=np.uint64)
        b[(np.arange(255) * (n - 1)) // 254] = 0x1b          # 255 distinct rows, row 0 and row n - 1 among them (n >= 255)
    k = (np.uint64(DIGIT_BASE) & ~(np.uint64(0xff) << np.uint64(8 * d))) | (b << np.uint64(8 * d))
    return k.view(np.int64) if signed else k


# ------------------------------------------------------------------------------------------------------------------------- tiles
SAW_PERIODS = [63, 64, 65, 255, 256, 257]


def tile_patterns(n):
    """{name: one digit value (u8) per row}, to be placed in any byte of a key"""
    i = np.arange(n, dtype=np.int64)
    out = {"sorted": i * 256 // n, "reversed": 255 - i * 256 // n}
    for p in SAW_PERIODS:                        # a wave of 64 keys then holds a value once or twice, at every offset
        out["saw%d" % p] = (i % p) % 256
    w, slot = i // 64, (i % 64) * 13 % 64        # wave w holds one value in w % 64 + 1 scattered lanes and a value of its own in every other lane:
    out["groups"] = np.where(slot < w % 64 + 1, w * 3, w * 3 + 1 + slot) % 256      # match-any groups of every size from 1 to 64, singletons beside them
    const = i % 251                              # tile 0 constant, tile 1 mixed, tile 2 constant on another value, the rest mixed
    const[:TILE] = 200
    const[2 * TILE:3 * TILE] = 3
    out["tile_constant"] = const
    j = i % TILE                                 # every value 16 times per whole tile: sub-tile k holds the 16 values 16 a + k, each 16 times
    out["sixteen_each"] = (j * 16 + j // BLOCK) % 256
    return {k: v.astype(np.uint8) for k, v in out.items()}


def place_digit(pattern, d, signed=False):
    k = (np.uint64(DIGIT_BASE) & ~(np.uint64(0xff) << np.uint64(8 * d))) | (pattern.astype(np.uint64) << np.uint64(8 * d))
    return k.view(np.int64) if signed else k


# ------------------------------------------------------------------------------------------------------------------------- top-k
N1 = SELECT_MIN_ROWS + 1
N3 = 3 * SELECT_MIN_ROWS + 1
KEY2_MOD = 1013


def second_key(n):
    """a low-cardinality u32 with ties, used after the first key"""
    return ((np.arange(n, dtype=np.int64) * 7919) % KEY2_MOD).astype(np.uint32)


def spread(n, c):
    """c distinct rows at an even stride, row 0 and row n - 1 among them"""
    return (np.arange(c, dtype=np.int64) * (n - 1)) // (c - 1)


def value_codes(v, desc):
    """encode_value restated in numpy (quantile.hpp): the order-preserving u64 code of every value, complemented for a descending key"""
    v = np.asarray(v)
    if v.dtype.kind == "f":
        with np.errstate(invalid="ignore"):                           # the signalling NaN
            f = v.astype(np.float64) + 0.0                            # -0 -> +0; a float32 widens exactly
        b = f.view(np.uint64).copy()
        b[np.isnan(f)] = np.uint64(0x7ff8000000000000)
        e = np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))
    elif v.dtype.kind == "i":
        e = v.astype(np.int64).view(np.uint64) ^ np.uint64(1 << 63)
    else:
        e = v.astype(np.uint64)
    return ~e if desc else e


def select_codes(key):
    """ENC_SELECT restated (kernels_sort.hip:58-68): the first key's code the selection walks, a null as 0 (nulls first) or all ones (nulls last).  The CPU tests count
    the candidate class of a top-k table with it; the tables state their counts from how they were built."""
    v, m, desc, nl = key
    e = value_codes(v, desc)
    if m is not None:
        e = np.where(m, e, np.uint64(0xffffffffffffffff) if nl else np.uint64(0))
    return e


def radix_route(keys, rows=None):
    """the text sort_indices reports for a radix sort of these keys (over the candidate rows `rows` of a selection): per key one pass for every digit of its range on
    which the rows differ (a null's value code is 0; an ascending unsigned key has `width` digits, an ascending Boolean one, every other key eight) and one more
    where nulls and valid rows meet; the digits on which every row agrees are skipped"""
    passes = skipped = 0
    for v, m, desc, nl in keys:
        v = np.asarray(v)
        e = value_codes(v, desc)
        if m is not None:
            e = np.where(m, e, np.uint64(0))
        if rows is not None:
            e = e[rows]
        digits = 8 if desc else (1 if v.dtype.kind == "b" else (v.dtype.itemsize if v.dtype.kind == "u" else 8))
        for d in range(digits):
            b = (e >> np.uint64(8 * d)) & np.uint64(255)
            if (b == b[0]).all():
                skipped += 1
            else:
                passes += 1
        if m is not None and not m.all():            # the null-rank pass runs whenever the column has a null, wherever it is
            mm = m if rows is None else m[rows]
            if mm.all() or not mm.any():
                skipped += 1
            else:
                passes += 1
    n = len(keys[0][0]) if rows is None else len(rows)
    return "radix_sort[rows=%d, keys=%d, passes=%d, uniform digits skipped=%d]" % (n, len(keys), passes, skipped)


def rank_route(rows, n_keys):
    return "rank_sort[rows=%d, keys=%d, one workgroup]" % (rows, n_keys)


def sort_route(keys, rows=None):
    """the route sort_indices takes for this many rows and keys"""
    n = len(keys[0][0]) if rows is None else len(rows)
    return rank_route(n, len(keys)) if n <= SMALL_MAX and len(keys) <= SMALL_MAX_KEYS else radix_route(keys, rows)


def select_route(rounds, candidates):
    return "top_k_select[%d digit rounds, candidates=%d] -> " % (rounds, candidates)


def _case(name, keys, picks):
    """picks: [(limit, digit rounds, candidates or None when the plan must show no selection)]"""
    return {"name": name, "keys": keys, "picks": picks}


def _one_round_keys(n, c):
    """c rows (spread) hold the distinct values 0 .. c - 1, scrambled; every other row holds 2^56 + (its number among the others) % 5000: the c rows are the whole of
    the lowest top-digit bucket"""
    k = np.zeros(n, dtype=np.int64)
    rows = spread(n, c)
    other = np.ones(n, bool)
    other[rows] = False
    k[other] = (1 << 56) + np.arange(n - c, dtype=np.int64) % 5000
    k[rows] = (np.arange(c, dtype=np.int64) * 1237) % c           # 1237 is prime and divides neither 2048 nor 2049
    return k


def _tied_min_keys(n, t, low=-3):
    """t rows (spread) hold `low`; the others distinct values from 0 up"""
    k = np.zeros(n, dtype=np.int64)
    rows = spread(n, t)
    other = np.ones(n, bool)
    other[rows] = False
    k[other] = (np.arange(n - t, dtype=np.int64) * 40503) % (n - t)
    k[rows] = low
    return k


EXTREME_REPEAT = 7
FILL_ROWS = 3600          # two thirds of it (a nullable key) are still > max(2 * limit, SMALL_MAX): the selection cannot stop before its last digit


def dtype_first_key(dt, n):
    """(values, rows below the low fill class, rows above the high fill class): the dtype's extremes EXTREME_REPEAT times each, then a class of FILL_ROWS rows next to
    them at either end, the rest in between.  Ascending, the limit-th row (limit = 100) lies in the low fill class; descending, in the high one."""
    t = NP[dt]
    if dt == "bool":
        v = np.ones(n, bool)
        v[spread(n, FILL_ROWS)] = False
        return v, 0, None                 # descending is built by the caller (True has to be the small class then)
    if dt in FLOATS:
        fi = np.finfo(t)
        low = [t(-np.inf), -fi.max]
        high = [t(np.inf), fi.max] + list(from_bits(dt, list(NAN_BITS[dt])))
        lo_fill, hi_fill = np.nextafter(-fi.max, t(0)), np.nextafter(fi.max, t(0))
        mid = np.array([-1.5, -0.0, 0.0, fi.tiny, -fi.tiny, np.nextafter(t(0), t(1)), -np.nextafter(t(0), t(1)), F32_DENORM, -F32_DENORM, 1.0, 2.5, -1e30, 1e30], dtype=t)
    else:
        ii = np.iinfo(t)
        low, high = [ii.min, ii.min + 1], [ii.max, ii.max - 1]
        lo_fill, hi_fill = ii.min + 2, ii.max - 2
        mid = np.array([ii.min + 3, ii.max - 3, ii.max // 2, ii.max // 2 + 1] + ([-1, 0, 1] if ii.min < 0 else [3, 4, 5]), dtype=t)
    v = mid[np.arange(n) % len(mid)]
    rows = spread(n, 2 * FILL_ROWS + EXTREME_REPEAT * (len(low) + len(high)))
    r = 0
    for x in low + high:
        v[rows[r:r + 2 * EXTREME_REPEAT:2]] = x          # every other slot of the spread, so extremes and fill rows interleave
        r += 2 * EXTREME_REPEAT
    rest = np.concatenate([rows[1:r:2], rows[r:]])
    assert len(rest) == 2 * FILL_ROWS
    v[rest[0::2]] = lo_fill
    v[rest[1::2]] = hi_fill
    return v, EXTREME_REPEAT * len(low), EXTREME_REPEAT * len(high)


@functools.lru_cache(maxsize=None)
def topk_tables():
    """Every case: the keys, and per limit the digit rounds and the candidate count that follow from how the first key was built (None: the plan shows no selection,
    because it never starts or because its candidates are not fewer than n / 2).  Nothing here runs the selection."""
    n = N1
    k2 = second_key(n)
    out = []
    # one round: the c small rows are the whole lowest bucket of the top digit
    k = _one_round_keys(n, SMALL_MAX)
    spill = SMALL_MAX + -(-(n - SMALL_MAX) // 5000)            # limit = c + 1: down to the last digit of the next bucket, whose lowest value 2^56 + 0 is held by every 5000th other row
    out.append(_case("one_round_2048", [(k, None, False, False)], [(1, 1, SMALL_MAX), (1000, 1, SMALL_MAX), (SMALL_MAX - 1, 1, SMALL_MAX), (SMALL_MAX, 1, SMALL_MAX), (SMALL_MAX + 1, 8, spill)]))
    out.append(_case("one_round_2049", [(_one_round_keys(n, SMALL_MAX + 1), None, False, False), (k2, None, True, False)], [(1500, 1, SMALL_MAX + 1)]))
    out.append(_case("one_round_2048_three_strides", [(_one_round_keys(N3, SMALL_MAX), None, False, False)], [(1000, 1, SMALL_MAX)]))
    # ties at the bound: 5000 rows equal the minimum
    k = _tied_min_keys(n, 5000)
    out.append(_case("tied_5000", [(k, None, False, False)], [(10, 8, 5000)]))
    out.append(_case("tied_5000_second_key", [(k, None, False, False), (k2, None, True, False)], [(10, 8, 5000)]))
    # the candidates have to be fewer than n / 2
    for t, kept in ((n // 2 + 1, False), (n // 2, False), (n // 2 - 1, True)):
        out.append(_case("tied_%d" % t, [(_tied_min_keys(n, t), None, False, False), (k2, None, False, False)], [(10, 8, t if kept else None)]))
    # nulls first: the null code 0 ties with i64.min's
    imin = np.iinfo(np.int64).min
    for z, mins, picks in ((3000, 0, [(100, 8, 3000)]), (50, 30, [(60, 1, 80)]), (3000, 30, [(100, 8, 3030), (3010, 1, 3030)])):
        k = (np.arange(n, dtype=np.int64) * 40503) % n + 1
        rows = spread(n, z + mins)
        min_rows = rows[1:2 * mins:2]                           # the i64.min rows lie between null rows
        null_rows = np.setdiff1d(rows, min_rows)
        valid = np.ones(n, bool)
        valid[null_rows] = False
        k[min_rows] = imin
        k[null_rows] = 77                                       # what a null row holds must not matter
        out.append(_case("nulls_first_z%d_min%d" % (z, mins), [(k, valid, False, False), (k2, None, True, False)], picks))
    # nulls last with fewer valid rows than the limit: the result runs into the nulls, every row is a candidate and the full sort answers
    for name, dt, edge, desc in (("u64_max", "u64", np.iinfo(np.uint64).max, False), ("u8_255", "u8", 255, False), ("u32_zero_desc", "u32", 0, True)):
        t = NP[dt]
        rows = spread(n, 40)
        valid = np.zeros(n, bool)
        valid[rows] = True
        k = np.full(n, 9, dtype=t)
        k[rows] = (np.arange(40) % 11 + 1).astype(t)
        k[rows[3::8]] = edge                                    # five valid rows at the valid end of the order (u64.max and a descending 0: the nulls' own code, all ones)
        out.append(_case("nulls_last_" + name, [(k, valid, desc, True), (k2, None, False, False)], [(100, 8, None)]))
    # every dtype first, both directions
    for dt in DTYPES:
        v, below, above = dtype_first_key(dt, n)
        valid = _third(n) if dt in ("i16", "f32") else None     # two of them nullable, nulls last: the nulls are no candidates
        out.append(_case("dtype_%s_asc" % dt, [(v, valid, False, True), (k2, None, True, False)], [(100, 8, _count(v, valid, below, dt, False))]))
        if dt == "bool":
            v = ~v
        out.append(_case("dtype_%s_desc" % dt, [(v, valid, True, True), (k2, None, True, False)], [(100, 8, _count(v, valid, above, dt, True))]))
    # Boolean first key with nulls first: the null code ties with False
    v, _, _ = dtype_first_key("bool", n)
    valid = np.ones(n, bool)
    valid[spread(n, 40)[1::2]] = False                          # 20 nulls; the False rows left valid are counted below
    n_false = int((~v & valid).sum())
    out.append(_case("bool_nulls_first", [(v, valid, False, False), (k2, None, False, False)], [(100, 8, 20 + n_false)]))
    # thresholds
    perm = (np.arange(SELECT_MIN_ROWS, dtype=np.int64) * 40503) % SELECT_MIN_ROWS
    out.append(_case("rows_65536", [(perm, None, False, False)], [(10, 0, None)]))
    perm = (np.arange(n, dtype=np.int64) * 40503) % n           # distinct 0 .. n - 1: the walk stops at digit 1, on a whole bucket of 256 values
    q = n // SELECT_LIMIT_DIV
    out.append(_case("limit_thresholds", [(perm, None, False, False)], [(q - 1, 7, -(-(q - 1) // 256) * 256), (q, 0, None), (n - 1, 0, None), (n, 0, None), (n + 5, 0, None)]))
    return out


def _count(v, valid, extremes, dt, desc):
    """candidates of a dtype_first_key table: the extreme rows in front of the fill class and the fill class, counted over the valid rows as they were placed"""
    ok = np.ones(len(v), bool) if valid is None else valid
    if dt == "bool":
        return int(((v if desc else ~v) & ok).sum())
    t = NP[dt]
    if dt in FLOATS:
        fill = np.nextafter(np.finfo(t).max, t(0)) if desc else np.nextafter(-np.finfo(t).max, t(0))
    else:
        fill = np.iinfo(t).max - 2 if desc else np.iinfo(t).min + 2
    if valid is None:
        return extremes + FILL_ROWS
    # nullable: the same classes, less the rows the validity pattern took out of them
    in_front = (np.isnan(v) | (v > fill)) if desc else (v < fill)
    return int(((in_front | (v == fill)) & ok).sum())


def topk_case(name):
    return next(c for c in topk_tables() if c["name"] == name)


# ----------------------------------------------------------------------------------------------------------------------- reference
def reference(keys, limit=None):
    """the oracle's stable multi-key arg-sort, cut to the first `limit` rows"""
    return pyoracle.sort_indices(keys, None if limit is None or limit < 0 else limit)
