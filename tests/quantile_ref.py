"""The reference for median / quantile: plain numpy, nothing of the product is imported.

ref_quantile(valid_values, q, interpolation) restates the contract (from polars-core/src/chunked_array/ops/aggregate/quantile.rs): the valid values
sorted in their own dtype with NaN last, pos = (n - 1) * q in one f64 multiply, the two picked elements converted to f64, then the rule.  accept() is the acceptance
of a device result against it.  Run as a module's test (test_quantile_cpu.py) it checks itself against np.quantile on NaN-free data."""
import math

import numpy as np

INTERPOLATIONS = ("nearest", "lower", "higher", "midpoint", "linear")
QS = (0.0, 1.0, 0.5, 0.25, 1.0 / 3.0, 0.999)


def picked(valid_values, q, interpolation):
    """(a, b, pos, lo, hi): the f64 values at ranks lo / hi of the sorted valid values (for "nearest" both are the nearest rank)"""
    v = np.sort(np.asarray(valid_values))              # NaN last; -0.0 and +0.0 compare equal, either may come first
    n = len(v)
    pos = float(np.float64(n - 1) * np.float64(q))
    lo, hi = min(int(math.floor(pos)), n - 1), min(int(math.ceil(pos)), n - 1)
    if interpolation == "nearest":
        lo = hi = min(int(math.floor(pos + 0.5)), n - 1)
    return float(v[lo]), float(v[hi]), pos, lo, hi


def ref_quantile(valid_values, q, interpolation):
    """None for no valid value, else the f64 quantile"""
    if len(valid_values) == 0:
        return None
    a, b, pos, lo, hi = picked(valid_values, q, interpolation)
    if interpolation in ("lower", "nearest"):
        return a
    if interpolation == "higher":
        return b
    with np.errstate(invalid="ignore", over="ignore"):
        if interpolation == "midpoint":
            return a if a == b else float((np.float64(a) + np.float64(b)) / np.float64(2.0))
        if interpolation == "linear":
            return a if (a == b or lo == hi) else float(np.float64(pos - lo) * (np.float64(b) - np.float64(a)) + np.float64(a))
    raise ValueError(interpolation)


def accept(got, valid_values, q, interpolation, f32=False):
    """The acceptance of a device result: None against None; NaN against NaN; nearest / lower / higher / midpoint equal as f64 values; linear within
    2 * 2^-53 * (|a| + |b|) (an FMA contraction changes one rounding of a product no larger than |b - a|; doubled for the final rounding).  Float32 outputs: the
    reference rounded to f32, within one f32 ulp."""
    want = ref_quantile(valid_values, q, interpolation)
    if want is None or got is None:
        return want is None and got is None
    if math.isnan(want) or math.isnan(got):
        return math.isnan(want) and math.isnan(got)
    if f32:
        w = np.float32(want)
        if math.isinf(float(w)) or math.isinf(got):
            return float(w) == got
        return abs(float(np.float32(got)) - float(w)) <= float(np.spacing(np.abs(w)))
    if interpolation != "linear":
        return got == want
    a, b, _, _, _ = picked(valid_values, q, interpolation)
    if math.isinf(want) or math.isinf(got):
        return got == want
    return abs(got - want) <= 2.0 * 2.0 ** -53 * (abs(a) + abs(b))


def self_check():
    """against np.quantile on NaN-free data: lower / higher / midpoint bit-equal; linear within 4 * 2^-53 relative (numpy's lerp has another form); nearest equal
    except where pos has fraction exactly 0.5, where this rule goes up (numpy: half to even).  Returns the number of cases compared."""
    rng = np.random.default_rng(415)
    cases = 0
    for n in (1, 2, 3, 4, 5, 6, 7, 10, 33, 64, 65, 70):
        for kind in ("normal", "ties"):
            v = rng.normal(10.0, 3.0, n) if kind == "normal" else rng.integers(-3, 4, n).astype(np.float64)
            for q in QS:
                for it in INTERPOLATIONS:
                    mine = ref_quantile(v, q, it)
                    theirs = float(np.quantile(v, q, method=it))
                    pos = float(np.float64(n - 1) * np.float64(q))
                    if it in ("lower", "higher", "midpoint"):
                        assert mine == theirs, (n, kind, q, it, mine, theirs)
                    elif it == "linear":
                        assert abs(mine - theirs) <= 4 * 2.0 ** -53 * max(abs(mine), abs(theirs)), (n, kind, q, it, mine, theirs)
                    elif pos - math.floor(pos) != 0.5:
                        assert mine == theirs, (n, kind, q, it, mine, theirs)
                    cases += 1
    for n, q, want in ((2, 0.5, 1), (6, 0.5, 3), (3, 0.25, 1)):          # half away from zero
        assert ref_quantile(np.arange(n), q, "nearest") == want, (n, q)
    assert ref_quantile(np.array([]), 0.5, "linear") is None
    assert math.isnan(ref_quantile(np.array([1.0, np.nan]), 1.0, "nearest")) and ref_quantile(np.array([1.0, 2.0, np.nan]), 0.5, "linear") == 2.0
    big = np.array([2 ** 53 + 1, 2 ** 53 + 3, 2 ** 53 + 5], dtype=np.int64)          # sorted as integers, rounded when picked
    assert ref_quantile(big, 0.5, "lower") == float(2 ** 53 + 3)
    return cases
