"""Tables and references for the column kernels behind the C ABI (plx_cast, plx_reduce, plx_cmp on Booleans, plx_bitmap_*, plx_if_then_else,
plx_frame_concat, the filter -> frame compaction), at the value, word and pointer edges that random data does not reach.  Plain Python / numpy: the
references are exact (Python ints, Fractions, math.fsum) and independent of the CPU oracle; tests/test_column_edges_cpu.py pins them without a GPU and
tests/test_gpu_column_edges.py runs the tables through the Series / DataFrame operators."""
import math
from fractions import Fraction

import numpy as np

NP = {"i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64, "u8": np.uint8, "u16": np.uint16, "u32": np.uint32, "u64": np.uint64,
      "f32": np.float32, "f64": np.float64}
PLDT = {"i8": "Int8", "i16": "Int16", "i32": "Int32", "i64": "Int64", "u8": "UInt8", "u16": "UInt16", "u32": "UInt32", "u64": "UInt64",
        "f32": "Float32", "f64": "Float64"}
DTYPES = list(NP)
INTS = [d for d in DTYPES if d[0] != "f"]
FLOATS = ["f32", "f64"]
CUTS = [1, 63, 64, 65]          # every table is also run cut to these lengths


def int_range(dt):
    info = np.iinfo(NP[dt])
    return int(info.min), int(info.max)


def is_float(dt):
    return dt[0] == "f"


def bits_of(a):
    """the bit patterns of a float array, every NaN folded onto one pattern (a NaN for a NaN)"""
    a = np.ascontiguousarray(a)
    u = a.view(np.uint32 if a.dtype == np.float32 else np.uint64).copy()
    u[np.isnan(a)] = 0
    return u, np.isnan(a)


def same_values(got, want):
    """exact: integers and Booleans equal, floats bit for bit (so -0.0 is not 0.0), a NaN for a NaN"""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind == "f":
        (g, gn), (w, wn) = bits_of(got), bits_of(want)
        return bool(np.array_equal(g, w) and np.array_equal(gn, wn))
    return bool(np.array_equal(got, want))


# ------------------------------------------------------------------------------------------------------------------------ casts
def _from_bits(dt, bits):
    return np.array([bits], dtype=np.uint32 if dt == "f32" else np.uint64).view(NP[dt])[0]


def _neighbours(ft, c):
    """the source-type neighbours of the integer c: the nearest value and the one below and above it (which straddle c where c is not representable)"""
    x = ft(float(c))
    return [np.nextafter(x, ft(-np.inf)), x, np.nextafter(x, ft(np.inf))]


def _pad_odd(vals, dt):
    """to an odd length above 128, repeating the table: the cast kernel's last validity word is then a partial one"""
    vals = list(vals)
    k = 0
    while len(vals) <= 128 or len(vals) % 2 == 0:
        vals.append(vals[k]); k += 1
    return np.array(vals, dtype=NP[dt])


def float_cast_table(dt):
    ft = NP[dt]
    fi = np.finfo(ft)
    vals = []
    for t in INTS:
        lo, hi = int_range(t)
        for c in (lo - 1, lo, hi, hi + 1):
            vals += _neighbours(ft, c)
    one, denorm = ft(1.0), np.nextafter(ft(0.0), ft(1.0))
    for v in (ft(0.0), ft(0.5), np.nextafter(one, ft(0.0)), one, denorm, fi.max):
        vals += [v, -v]
    nans = [_from_bits(dt, b) for b in ((0x7fc00001, 0xffc00abc) if dt == "f32" else (0x7ff8000000000001, 0xfff8000000000abc))]
    vals += nans + [ft(np.inf), ft(-np.inf)]
    if dt == "f64":      # f64 -> f32: ties, overflow to inf, results that are denormal
        f32max, e = float(np.finfo(np.float32).max), 2.0 ** -149
        edge = 2.0 ** 128 - 2.0 ** 103                       # half an ulp above f32's maximum: the first value that rounds to inf
        for v in (1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, np.nextafter(1.0 + 2.0 ** -24, 2.0), 16777217.0, 16777219.0,
                  f32max, np.nextafter(edge, 0.0), edge, 2.0 ** 128, 1e300,
                  e, 1.5 * e, 2.5 * e, 0.5 * e, np.nextafter(0.5 * e, 1.0), np.nextafter(0.5 * e, 0.0), 2.0 ** -126, 2.0 ** -126 * (1 - 2.0 ** -25), 2.0 ** -127, 1e-300):
            vals += [np.float64(v), np.float64(-v)]
    return _pad_odd(vals, dt)


def int_cast_table(dt):
    lo, hi = int_range(dt)
    vals = [lo, hi, -1, 0, 1]
    for t in INTS:
        tlo, thi = int_range(t)
        vals += [tlo - 1, tlo, thi, thi + 1]
    into_float = [2 ** 24 + 1, 2 ** 24 + 2, 2 ** 24 + 3, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1, 2 ** 53 + 1, 2 ** 53 + 2, 2 ** 53 + 3,
                  2 ** 63 - 2 ** 38, 2 ** 63 - 2 ** 38 - 1, 2 ** 63 - 2 ** 9, 2 ** 63 - 2 ** 9 - 1]      # the last four: ties just below 2^63 as f32 and as f64
    vals += into_float + [-v for v in into_float]
    return _pad_odd([v for v in vals if lo <= v <= hi], dt)


def cast_table(dt):
    return float_cast_table(dt) if is_float(dt) else int_cast_table(dt)


def int_to_f32(v):
    """int -> float32, round half to even, in integer arithmetic"""
    m = abs(int(v))
    if m >= 1 << 24:
        sh = m.bit_length() - 24
        q, r, half = m >> sh, m & ((1 << sh) - 1), 1 << (sh - 1)
        if r > half or (r == half and (q & 1)):
            q += 1
        m = q << sh
    return np.float32(float(-m if v < 0 else m))     # at most 24 significant bits: both conversions are exact


def cast_reference(a, to):
    """(values, ok) of a non-strict cast of every row of `a`: a value the target cannot hold gives a null (ok False, value 0)"""
    frm = a.dtype
    n = len(a)
    out, ok = np.zeros(n, dtype=NP[to]), np.ones(n, bool)
    if is_float(to):
        if frm.kind == "f":
            with np.errstate(over="ignore"):      # f64 -> f32 overflows to inf on purpose
                out = a.astype(NP[to])
        elif to == "f64":
            out = np.array([float(int(x)) for x in a], dtype=np.float64)
        else:
            out = np.array([int_to_f32(int(x)) for x in a], dtype=np.float32)
        return out, ok
    lo, hi = int_range(to)
    for i, x in enumerate(a):
        if frm.kind == "f" and not math.isfinite(x):
            ok[i] = False
            continue
        t = int(x)                 # Python truncates a float toward zero, exactly
        if lo <= t <= hi:
            out[i] = t
        else:
            ok[i] = False
    return out, ok


def every_third_null(n):
    v = np.ones(n, bool)
    v[2::3] = False
    return v


# ------------------------------------------------------------------------------------------------------------------- reductions
SUM_OUT = {"i8": "i64", "i16": "i64", "u8": "i64", "u16": "i64", "i32": "i32", "u32": "u32", "i64": "i64", "u64": "u64"}


def vec(dt):
    return 16 // np.dtype(NP[dt]).itemsize


def reduce_rows(dt):
    """several workgroups whatever grid the device chooses, a tail of whole runs and a tail of rows"""
    v = vec(dt)
    return 5 * 256 * v * 4 + 64 * v + 3


def lone_rows(dt):
    v, n = vec(dt), reduce_rows(dt)
    return [0, 1, v - 1, v, 64 * v - 1, 64 * v, n // 2, n - 4, n - 1]


def wrap(x, dt):
    lo, hi = int_range(dt)
    return (x - lo) % (hi - lo + 1) + lo


def reduce_reference(a, valid=None):
    """sum / mean / min / max / count of the valid rows, exact.  Integers: Python ints, the sum wrapped at the width the library sums at, the mean a Fraction.
    Floats: min / max skip NaN unless nothing else is there; the sum is math.fsum (NaN when a NaN or both infinities are present), the mean sum / count."""
    dt = [k for k, t in NP.items() if np.dtype(t) == a.dtype][0]
    rows = a if valid is None else a[valid]
    cnt = int(len(rows))
    if cnt == 0:
        return {"count": 0, "sum": 0.0 if is_float(dt) else 0, "mean": None, "min": None, "max": None}
    if not is_float(dt):
        xs = [int(x) for x in rows]
        return {"count": cnt, "sum": wrap(sum(xs), SUM_OUT[dt]), "mean": Fraction(sum(xs), cnt), "min": min(xs), "max": max(xs)}
    xs = [float(x) for x in rows]
    ordered = [x for x in xs if x == x]
    if len(ordered) < cnt or (math.inf in xs and -math.inf in xs):
        s = math.nan
    elif math.inf in xs or -math.inf in xs:
        s = math.inf if math.inf in xs else -math.inf
    else:
        s = math.fsum(xs)
    return {"count": cnt, "sum": s, "mean": s / cnt, "min": min(ordered) if ordered else math.nan, "max": max(ordered) if ordered else math.nan}


def walk_validity(n):
    """exactly one bit per 64-row word: bit (7 w) % 64 of word w (the last, partial word keeps it only if the row exists)"""
    v = np.zeros(n, bool)
    w = np.arange((n + 63) // 64)
    rows = w * 64 + (7 * w) % 64
    v[rows[rows < n]] = True
    return v


def word_validity(n):
    """whole words valid, alternating with whole words null"""
    return ((np.arange(n) >> 6) & 1) == 0


def walk_values(dt, n):
    i = np.arange(n, dtype=np.int64)
    if np.dtype(NP[dt]).itemsize < 4:
        return (i % 127 + 1).astype(NP[dt])
    return (i + 1).astype(NP[dt])


# ------------------------------------------------------------------------------------------------------------- Boolean columns
BOOL_LENGTHS = [1, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049]
COMBOS = [(p, q) for p in (True, False, None) for q in (True, False, None)]


def bool_operands(n):
    """two columns as (values, valid): the nine (true / false / null)^2 pairs in turn from row 0, and once more over the last nine rows -- so all of them lie in the
    first word, and in the last word wherever that word has nine rows.  Null rows carry a TRUE value bit in the left column and a false one in the right: an operator
    that read the value of a null row shows."""
    idx = np.arange(n) % 9
    if n >= 9:
        idx[n - 9:] = np.arange(9)
    p = np.array([COMBOS[k][0] for k in idx], dtype=object)
    q = np.array([COMBOS[k][1] for k in idx], dtype=object)
    av, bv = np.array([x is not None for x in p], bool), np.array([x is not None for x in q], bool)
    a = np.array([True if x is None else x for x in p], bool)
    b = np.array([False if x is None else x for x in q], bool)
    return (a, av), (b, bv)


def third_bool(n):
    """a mask that is coprime with the pattern of nine: (values, valid)"""
    i = np.arange(n)
    return (i % 5) < 2, (i % 7) != 3


BOOL_CMP = {0: np.equal, 1: np.not_equal, 2: np.less, 3: np.less_equal, 4: np.greater, 5: np.greater_equal}      # PLX_EQ .. PLX_GE


def bool_cmp_reference(op, a, b):
    return BOOL_CMP[op](a.astype(np.uint8), b.astype(np.uint8))


def kleene(op, a, av, b, bv):
    """(values, valid) of a & b / a | b in three-valued logic; ^ is null where either side is"""
    if op == "and":
        v = a & b
        ok = (~b & bv) | (~a & av) | (av & bv)
    elif op == "or":
        v = a | b
        ok = (a & av) | (b & bv) | (av & bv)
    else:
        v, ok = a ^ b, av & bv
    return v, ok


# ---------------------------------------------------------------------------------------------------------------- concatenation
CONCAT_LENGTHS = [0, 31, 1, 31, 65, 1, 31, 1, 200, 64, 63, 0]


def concat_offsets():
    return np.concatenate([[0], np.cumsum(CONCAT_LENGTHS)])[:-1].tolist()


def concat_chunk(k, n):
    """chunk k of n rows: {name: (values, valid or None)}; every third chunk has no validity at all"""
    i = np.arange(n, dtype=np.int64)
    cols = {"a": (i * 1_000_003 + k).astype(np.int64), "u": ((i * 7 + k) % 251).astype(np.uint8), "b": ((i + k) % 3) != 0}
    out = {}
    for j, (name, v) in enumerate(cols.items()):
        valid = None if k % 3 == 2 else ((i + j + k) % 4) != 1
        out[name] = (v, valid)
    return out


# ---------------------------------------------------------------------------------------------------- filter -> frame over many columns
FILTER_LENGTHS = [1, 127, 129, 1023, 1025, 2049, 20_011]
PRIMES = [1_000_003, 10_007, 7919, 104_729, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73]
DENSE_COLUMNS = ["i32", "u8", "i64", "i16", "f64", "u32", "i8", "bool", "u64", "f32", "u16", "i64", "i32", "i16", "u8"]      # 4 x 8 bytes, 4 x 4, 3 x 2, 3 x 1 + the Boolean
SPARSE_COLUMNS = ["i64", "i32", "i64", "i64", "i32", "i32", "i64", "i32", "i64"]


def stamped(dt, c, n):
    """row * prime_c + c: a value names its row and its column (wrapped at the column's width; exact in the float columns)"""
    x = np.arange(n, dtype=np.int64) * PRIMES[c] + c
    if dt == "bool":
        return (x % 3) == 0
    if is_float(dt):
        return (x % (1 << 22)).astype(NP[dt])
    return x.astype(NP[dt])


# ---------------------------------------------------------------------------------------------------------- borrowed columns
SKIPS = {8: [1, 3], 4: [1, 2, 3], 2: [1, 7], 1: [1, 15]}


def borrowed_rows(dt):
    return [1, 2 * 64 * vec(dt) + 5]


def window_values(dt, n):
    """small non-zero values with both signs where the type has them: every arithmetic operator is defined on every row"""
    i = np.arange(n, dtype=np.int64)
    x = (i * 37 + 11) % 97 + 1
    if dt[0] != "u":
        x = np.where(i % 3 == 1, -x, x)
    return x.astype(NP[dt])
