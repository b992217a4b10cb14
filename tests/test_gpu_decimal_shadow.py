"""Decimal shadows of f64 columns (csrc/decimal.hpp, csrc/encoded_inputs.hpp, DESIGN.md "Encoded shadows") against numpy.

The three-run pattern of tests/test_gpu_encoded_inputs.py (plain, building, encoded; keyed through the LDS-table sink, unkeyed through the register sink), with the
row threshold of the decimal kind set to 0 by a fixture that restores the configured value.  What a column must report is worked out here from the data, with the
chooser's own order: the dictionary is tried first, so a column with at most 256 distinct bit patterns among its valid rows says dict8 -- every column of 1, 127,
128 or 129 rows does -- and only past that does a column of decimals say decimal32; the tests assert that from 677 rows on the must-encode columns ARE past it.
Integer results, counts and min / max are exact; f64 sums within RTOL = 1e-6 of numpy (the bound of the file the helpers come from)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_encoded_inputs import ROOT, ROWS, aggs_of, check, drop_statistics, encodings_in, frame_of, reference, three_runs

pytestmark = pytest.mark.gpu

KINDS = ("sum", "min", "max")
DEEP_ROWS = (1 << 20) + (1 << 18)


@pytest.fixture
def no_threshold(pl):
    F = pl._ffi
    before = F.encoded_decimal_min_rows()
    F.encoded_set_decimal_min_rows(0)
    yield
    F.encoded_set_decimal_min_rows(before)


def expected(v, valid=None):
    """dict8 when the dictionary takes the column; else decimal32 when every valid row is a decimal of at most nine digits that spans less than 2^32; else None"""
    x = v if valid is None else v[valid]
    if len(x) == 0:
        return None
    if len(np.unique(x.view(np.uint64))) <= 256:
        return "dict8"
    if not np.all(np.isfinite(x)) or np.any((x == 0) & np.signbit(x)):
        return None
    for e in range(10):
        k = np.rint(x * 10.0**e)
        if np.all(np.abs(k) < 2.0**53) and np.array_equal((k / 10.0**e).view(np.uint64), x.view(np.uint64)):
            return "decimal32" if k.max() - k.min() < 2.0**32 else None
    return None


# ---- columns -------------------------------------------------------------------------------------------------------------------------------
def encoding_data(n):
    rng = np.random.default_rng(4000 + n)
    valid = rng.random(n) < 0.7
    valid[0] = True
    nul = rng.integers(0, 10_000_000, n) / 100.0
    nul[~valid] = np.where(rng.random(int((~valid).sum())) < 0.5, np.nan, 0.1 + 0.2)      # null rows hold NaN and non-decimals
    k = rng.integers(0, 10_000_000, n)
    return {
        "g": (rng.integers(0, 4, n).astype(np.uint8), None),
        "p": (rng.integers(0, 100, n).astype(np.int64), None),
        "price": (np.round(rng.integers(1, 51, n) * rng.integers(90_000, 210_000, n) / 100.0, 2), None),
        "ints": (rng.integers(0, 1_000_000, n).astype(np.float64), None),                  # exponent 0
        "neg": (rng.integers(-5_000_000, 5_000_000, n) / 1000.0, None),                    # a base other than 0
        "nul": (nul, valid),
        "mul": (k / 100.0, None),                                                          # k / 100 and k * 0.01 differ in some rows
    }, k


def rejected_data(n):
    rng = np.random.default_rng(5000 + n)
    wide = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.float64)
    wide[0] = 0.0
    wide[-1] = 2.0**32                                                                     # a span of exactly 2^32 (from two rows on)
    negz = rng.integers(1, 1_000_000, n) / 100.0
    negz[n // 2] = -0.0
    nanv = rng.integers(1, 1_000_000, n) / 100.0
    nanv[n // 3] = np.nan
    return {
        "g": (rng.integers(0, 4, n).astype(np.uint8), None),
        "p": (rng.integers(0, 100, n).astype(np.int64), None),
        "rnd": (900.0 + 1e5 * rng.random(n), None),
        "wide": (wide, None),
        "negz": (negz, None),
        "nanv": (nanv, None),
        "few": (rng.integers(0, 256, n) / 100.0, None),                                    # at most 256 distinct decimals: the dictionary keeps it
    }


@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("n", ROWS)
def test_columns_of_decimals_encode(pl, no_threshold, n, keyed):
    data, k = encoding_data(n)
    df = frame_of(pl, data)
    keep = data["p"][0] < 70
    expect = {name: expected(*data[name]) for name in ("price", "ints", "neg", "nul", "mul")}
    if n >= 677:
        assert set(expect.values()) == {"decimal32"}, expect
        assert (data["neg"][0] < 0).any() and ((k / 100.0) != (k * 0.01)).any()
    else:
        assert set(expect.values()) == {"dict8"}, expect
    expect["p"] = "affine8"
    three_runs(pl, df, data, [("price", KINDS), ("ints", KINDS), ("neg", KINDS)], pl.col("p") < 70, keep, keyed, {c: expect[c] for c in ("p", "price", "ints", "neg")}, ("decimal", n))
    three_runs(pl, df, data, [("nul", KINDS + ("count", "mean")), ("mul", KINDS)], pl.col("p") < 70, keep, keyed, {c: expect[c] for c in ("p", "nul", "mul")}, ("decimal, second set", n))


@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("n", ROWS)
def test_columns_that_are_no_decimals_stay_plain(pl, no_threshold, n, keyed):
    data = rejected_data(n)
    df = frame_of(pl, data)
    keep = data["p"][0] >= 20
    expect = {name: expected(*data[name]) for name in ("rnd", "wide", "negz", "nanv", "few")}
    assert expect["few"] == "dict8"
    if n >= 677:
        assert [expect[c] for c in ("rnd", "wide", "negz", "nanv")] == [None] * 4, expect
    expect["p"] = "affine8"
    three_runs(pl, df, data, [("rnd", KINDS), ("wide", KINDS), ("negz", KINDS)], pl.col("p") >= 20, keep, keyed, {c: expect[c] for c in ("p", "rnd", "wide", "negz")}, ("rejected", n))
    three_runs(pl, df, data, [("nanv", KINDS), ("few", KINDS)], pl.col("p") >= 20, keep, keyed, {c: expect[c] for c in ("p", "nanv", "few")}, ("rejected, second set", n))


# ---- lifecycle -----------------------------------------------------------------------------------------------------------------------------
def price_frame(pl, n=677):
    rng = np.random.default_rng(9)
    data = {"g": (rng.integers(0, 4, n).astype(np.uint8), None), "v": (10 + rng.integers(0, 50, n).astype(np.int64), None),
            "x": (np.round(rng.integers(1, 51, n) * rng.integers(90_000, 210_000, n) / 100.0, 2), None)}
    return data, frame_of(pl, data)


def price_query(pl, df):
    return df.lazy().filter(pl.col("v") > 12).group_by("g").agg(pl.col("v").sum().alias("s"), pl.col("x").sum().alias("xs"), pl.len().alias("n"))


def test_borrowed_buffers_never_encode(pl, no_threshold):
    import torch
    data, _ = price_frame(pl)
    tx = torch.from_numpy(data["x"][0]).cuda()
    torch.cuda.synchronize()
    df = pl.DataFrame([pl.Series("g", data["g"][0]), pl.Series("v", data["v"][0]), pl.Series.from_torch("x", tx)])
    keep = data["v"][0] > 12
    for _ in range(4):
        out = price_query(pl, df).collect().to_dict()
        assert "x:" not in pl.last_plan_encodings(), pl.last_plan_encodings()
        assert np.isclose(sum(out["xs"]), data["x"][0][keep].sum(), rtol=1e-6, atol=0.0) and sum(out["n"]) == int(keep.sum())


def test_switch_turns_the_feature_off_in_a_fresh_process():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\nimport polars_amd as pl\nimport test_gpu_decimal_shadow as T\npl.init(0)\n"
            "assert pl._ffi.encoded_decimal_min_rows() == 0\ndata, df = T.price_frame(pl)\nfor _ in range(4):\n    T.price_query(pl, df).collect()\n"
            "    assert pl.last_plan_encodings() == '', pl.last_plan_encodings()\nprint('never encoded')\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PLX_ENCODED_INPUTS="0", PLX_ENCODED_DECIMAL_MIN_ROWS="0"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "never encoded" in r.stdout, r.stdout + r.stderr


def test_the_row_threshold(pl):
    """At the default a price column of 2^18 + 5 rows gets no shadow (and is not tried again); with the threshold at 0 it does."""
    F = pl._ffi
    before = F.encoded_decimal_min_rows()
    data, df = price_frame(pl, (1 << 18) + 5)
    try:
        F.encoded_set_decimal_min_rows(1 << 22)
        seen = []
        for _ in range(3):
            price_query(pl, df).collect()
            seen.append(encodings_in(pl.last_plan_encodings()))
        assert seen == [{}, {"v": "affine8"}, {"v": "affine8"}], seen
        F.encoded_set_decimal_min_rows(0)
        drop_statistics(pl, df)
        seen = []
        for _ in range(3):
            price_query(pl, df).collect()
            seen.append(encodings_in(pl.last_plan_encodings()))
        assert seen == [{}, {"v": "affine8", "x": "decimal32"}, {"v": "affine8", "x": "decimal32"}], seen
    finally:
        F.encoded_set_decimal_min_rows(before)


def encoder_launches(pl, fn):
    """names of the encoder passes (kernels_encode.hip) `fn` launches"""
    F = pl._ffi
    F.check(F.lib().plx_profile_clear()); F.check(F.lib().plx_profile_enable(1))
    try:
        fn()
        F.check(F.lib().plx_synchronize())
        recs = (F.ProfileRecord * 4096)()
        n = C.c_int32()
        F.check(F.lib().plx_profile_fetch(recs, 4096, C.byref(n)))
        return [recs[i].name.decode() for i in range(n.value) if recs[i].name.decode().startswith("encode_")]
    finally:
        F.check(F.lib().plx_profile_enable(0))


def test_one_non_decimal_deep_in_the_column_discards_the_shadow(pl, no_threshold):
    """10 MB of two-decimal values, so the chooser samples every second row, and one 0.1 + 0.2 on an odd row past the middle: the sample accepts the column, the
    encode pass -- which decodes every row again -- does not, and the column is never tried again."""
    n = DEEP_ROWS
    rng = np.random.default_rng(21)
    x = rng.integers(0, 50_000_000, n) / 100.0
    row = (n // 2 + 98_765) | 1
    x[row] = 0.1 + 0.2
    step = (n + (1 << 20) - 1) >> 20      # build_shadow's sample stride
    assert step == 2 and row % step != 0 and row > n // 2 and expected(x[::step]) == "decimal32" and expected(x) is None
    data = {"g": (rng.integers(0, 4, n).astype(np.uint8), None), "x": (x, None)}
    df = frame_of(pl, data)
    cols = [("x", KINDS)]
    ref = reference(data, cols, np.ones(n, bool), data["g"][0])
    launches = []
    for run in range(4):
        launches.append(encoder_launches(pl, lambda: check(df.lazy().filter(pl.col("g") < 4).group_by("g").agg(*aggs_of(pl, cols)).collect(), ref, True, ("deep", run))))
        assert "decimal32" not in pl.last_plan_encodings(), (run, pl.last_plan_encodings())
    assert launches[0] == [] and "encode_decimal_sample" in launches[1] and "encode_decimal" in launches[1], launches
    assert launches[2] == [] and launches[3] == [], launches


# ---- Q1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [677, (1 << 18) + 5])
def test_q1_with_five_encodings_aot_jit_and_generic_agree(pl, no_threshold, n):
    """tests/test_gpu_encoded_inputs.py test_encoded_q1_aot_jit_and_generic_agree with the price column encoded as well: the ahead-of-time kernel of the
    five-encoding shape, and -- with one null in l_quantity, a shape of its own -- the run-time compiled kernel and the generic interpreter.  Each mode's encoded run
    equals its plain run, the two modes equal each other, and they equal the ahead-of-time run in every column l_quantity does not enter."""
    from polars_amd import datagen, queries
    from test_gpu_encoded_inputs import RTOL
    F = pl._ffi
    li = datagen.lineitem_host(n, seed=33)
    lt = datagen.logical_dtypes(pl)
    want_enc = {"l_shipdate": "affine16", "l_quantity": "affine8", "l_extendedprice": "decimal32", "l_discount": "dict8", "l_tax": "dict8"}
    assert expected(li["l_extendedprice"]) == "decimal32"
    keys = ["l_returnflag", "l_linestatus"]

    def first_and_third_run(df):
        outs = []
        for _ in range(3):
            outs.append(queries.q1(df.lazy()).collect().sort_host(keys))
        assert encodings_in(pl.last_plan_encodings()) == want_enc, pl.last_plan_encodings()
        return outs[0], outs[2], pl.last_plan()

    def assert_same(a, b, what, cols=None):
        for col in (cols or a):
            if isinstance(a[col][0], float):
                assert np.allclose(a[col], b[col], rtol=RTOL, atol=0.0), (what, col)
            else:
                assert a[col] == b[col], (what, col)

    res = {}
    plain, res["aot"], plan = first_and_third_run(datagen.to_frame(pl, li, datagen.LINEITEM_Q1_COLS))
    assert "fused_scan[aot]" in plan, plan
    assert_same(plain, res["aot"], "aot against its plain run")
    valid = np.ones(n, bool)
    valid[0] = False
    try:
        for mode, min_rows in (("jit", 0), ("generic", -1)):
            F.jit_set_min_rows(min_rows)
            df = pl.DataFrame([pl.Series(c, li[c], dtype=lt.get(c), validity=valid if c == "l_quantity" else None) for c in datagen.LINEITEM_Q1_COLS])
            plain_m, res[mode], plan = first_and_third_run(df)
            assert f"fused_scan[{mode}]" in plan, plan
            assert_same(plain_m, res[mode], mode + " against its plain run")
    finally:
        F.jit_set_min_rows(1 << 22)
    assert_same(res["jit"], res["generic"], "jit against generic")
    assert_same(res["aot"], res["jit"], "aot against jit", keys + ["sum_base_price", "sum_disc_price", "sum_charge", "avg_price", "avg_disc", "count_order"])
