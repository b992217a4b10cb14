"""Encoded shadows of low-cardinality columns (csrc/encoded_inputs.hpp, DESIGN.md "Encoded shadows") against numpy.

Every query runs three times on library-owned columns (pl.Series -> plx_column_from_host): the plain scan, the scan that builds the shadows, the scan that reads
them.  All three results are compared with numpy, and the third run must name (pl.last_plan_encodings(), beside the plan text) exactly the encodings the data admits (worked out here from the data: span, gcd,
distinct bit patterns).  A filter + group_by on a small u8 key runs the LDS-table sink, the same query without the key the register sink.  Integer sums, counts
and min / max are exact; f64 sums within RTOL = 1e-6, the bound tests/test_gpu_groupby_routes.py uses against numpy."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-6
ROWS = [1, 127, 128, 129, 677, (1 << 18) + 5]
DAY_US = 86_400_000_000
I64 = np.iinfo(np.int64)


# ---- what the data admits ------------------------------------------------------------------------------------------------------------
def expected_affine(v, valid=None):
    x = v if valid is None else v[valid]
    if len(x) == 0:
        return None
    mn, mx = int(x.min()), int(x.max())
    span = mx - mn
    if span >= 1 << 62:
        return None
    stride = 1
    if span > 65535:
        stride = int(np.gcd.reduce((x - mn).astype(np.uint64)))
    top = span // stride
    return None if top > 65535 else ("affine8" if top <= 255 else "affine16")


def expected_dict(v, valid=None):
    bits = v.view(np.uint64)
    bits = bits if valid is None else bits[valid]
    return "dict8" if 0 < len(np.unique(bits)) <= 256 else None


def encodings_in(plan):
    """{column: encoding} out of pl.last_plan_encodings()"""
    m = re.search(r"encoded\{([^}]*)\}", plan)
    return dict(t.split(":") for t in m.group(1).split(",")) if m else {}


def drop_statistics(pl, df):
    for s in df.get_columns():
        pl._ffi.check(pl._ffi.lib().plx_column_drop_statistics(s._h))


# ---- the two query forms ---------------------------------------------------------------------------------------------------------------
def aggs_of(pl, cols):
    out = [pl.len().alias("n")]
    for name, kinds in cols:
        for kind in kinds:
            out.append(getattr(pl.col(name), kind)().alias(f"{name}_{kind}"))
    return out


def reference(data, cols, keep, g):
    """{key tuple: {aggregate: value}} over the rows in `keep`; g None: one group with the key ()"""
    groups = {(): keep} if g is None else {(int(k),): keep & (g == k) for k in np.unique(g[keep])}
    ref = {}
    for key, rows in groups.items():
        r = {"n": int(rows.sum())}
        for name, kinds in cols:
            v, valid = data[name]
            sel = rows if valid is None else rows & valid
            x = v[sel]
            for kind in kinds:
                if kind == "count":
                    r[f"{name}_count"] = int(sel.sum())
                elif len(x) == 0:
                    r[f"{name}_{kind}"] = (0.0 if v.dtype == np.float64 else 0) if kind == "sum" else None
                elif kind == "sum":
                    r[f"{name}_sum"] = float(x.sum()) if v.dtype == np.float64 else int(x.sum(dtype=np.int64))
                elif kind == "mean":
                    r[f"{name}_mean"] = float(x.astype(np.float64).sum() / len(x))
                elif v.dtype == np.float64:      # min / max ignore NaN; all NaN -> NaN
                    o = x[~np.isnan(x)]
                    r[f"{name}_{kind}"] = float("nan") if len(o) == 0 else float(o.min() if kind == "min" else o.max())
                else:
                    r[f"{name}_{kind}"] = int(x.min() if kind == "min" else x.max())
        ref[key] = r
    return ref


def same(got, want, what):
    if isinstance(want, float):
        assert got is not None, what
        if np.isnan(want):
            assert np.isnan(got), (what, got, want)
        elif np.isinf(want) or what[-1].endswith(("_min", "_max")):
            assert got == want, (what, got, want)
        else:
            assert np.isclose(got, want, rtol=RTOL, atol=0.0), (what, got, want)
    else:
        assert got == want, (what, got, want)


def check(out, ref, keyed, what):
    d = out.to_dict()
    got = {}
    for i in range(len(d["n"])):
        got[(int(d["g"][i]),) if keyed else ()] = {k: d[k][i] for k in d if k != "g"}
    if not keyed and not ref[()]["n"]:
        assert got[()]["n"] == 0, what
        return
    assert set(got) == {k for k, r in ref.items() if r["n"]}, (what, sorted(got), sorted(ref))
    for key, r in ref.items():
        for name, want in r.items():
            if r["n"]:
                same(got[key][name], want, (what, key, name))


def three_runs(pl, df, data, cols, pred_expr, keep, keyed, expect, what):
    """plain, building, encoded -- on a frame whose statistics (shadows, scan counts) were just dropped.  `expect`: {column: encoding or None}."""
    drop_statistics(pl, df)
    ref = reference(data, cols, keep, data["g"][0] if keyed else None)
    plans = []
    for run in range(3):
        lf = df.lazy().filter(pred_expr)
        lf = lf.group_by("g").agg(*aggs_of(pl, cols)) if keyed else lf.select(*aggs_of(pl, cols))
        out = lf.collect()
        plans.append(pl.last_plan_encodings())
        assert ("lds_table" if keyed else "register_sink") in pl.last_plan(), pl.last_plan()
        check(out, ref, keyed, (what, "keyed" if keyed else "plain", run))
    assert plans[0] == "", plans[0]
    want = {k: v for k, v in expect.items() if v}
    assert encodings_in(plans[1]) == want and encodings_in(plans[2]) == want, (what, plans, want)
    return plans


def frame_of(pl, data):
    return pl.DataFrame([pl.Series(name, v, validity=valid) if valid is not None else pl.Series(name, v) for name, (v, valid) in data.items()])


# ---- affine ------------------------------------------------------------------------------------------------------------------------------
def integer_data(n):
    rng = np.random.default_rng(n)
    k16 = rng.integers(0, 65536, n)
    if n > 70000:
        k16[:65536] = rng.permutation(65536)      # every code, 0 and 65535 included
    big = rng.integers(0, 65537, n)
    if n > 70000:
        big[:65537] = rng.permutation(65537)      # 65537 distinct multiples: one too many
    data = {
        "g": (rng.integers(0, 4, n).astype(np.uint8), None),
        "p": (rng.integers(0, 100, n).astype(np.int64), None),
        "a8": (1000 + rng.integers(0, 256, n).astype(np.int64), None),
        "a16": (-5_000_000_000 + 7 * k16.astype(np.int64), None),                 # a negative base
        "day": (8035 * DAY_US + DAY_US * rng.integers(1, 2647, n).astype(np.int64), None),
        "const": (np.full(n, -42, np.int64), None),
        "big": (3 * big.astype(np.int64) - 17, None),
        "ext": (np.where(rng.random(n) < 0.5, I64.min, I64.max).astype(np.int64), None),
        "i32": (rng.integers(-100, 100, n).astype(np.int32), None),
    }
    return data


@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("n", ROWS)
def test_affine_columns(pl, n, keyed):
    data = integer_data(n)
    df = frame_of(pl, data)
    keep = data["p"][0] < 70
    pred = pl.col("p") < 70
    expect = {name: expected_affine(data[name][0]) for name in ("p", "a8", "a16", "day", "const", "big", "ext", "i32")}
    assert expect["const"] == "affine8" and expect["a8"] == "affine8" and (n < 1000 or (expect["a16"] == "affine16" and expect["day"] == "affine16"))
    assert expect["i32"] == "affine8" and (n < 70000 or expect["big"] is None) and (n == 1 or len(np.unique(data["ext"][0])) < 2 or expect["ext"] is None)
    first = [("a8", ("sum", "min", "max")), ("a16", ("sum", "min", "max")), ("day", ("sum", "min", "max")), ("i32", ("min", "max"))]
    three_runs(pl, df, data, first, pred, keep, keyed, {k: expect[k] for k in ("p", "a8", "a16", "day", "i32")}, ("affine", n))
    second = [("const", ("sum", "min", "max")), ("big", ("sum", "min", "max")), ("ext", ("sum", "min", "max"))]      # (the sum of the extremes wraps, here as there)
    three_runs(pl, df, data, second, pred, keep, keyed, {k: expect[k] for k in ("p", "const", "big", "ext")}, ("affine, second set", n))


@pytest.mark.parametrize("keyed", [True, False])
def test_predicates_on_an_encoded_column(pl, keyed):
    """== != < <= > >= against constants below the base, above the maximum, between two codes and exactly on a code: the decoded value is compared, never the code."""
    n = 677
    rng = np.random.default_rng(5)
    base, stride = -1_000_003, 1000
    v = base + stride * rng.integers(0, 300, n).astype(np.int64)
    v[:2] = base, base + 299 * stride
    data = {"g": (rng.integers(0, 4, n).astype(np.uint8), None), "v": (v, None), "w": (rng.integers(-9, 9, n).astype(np.int64), None)}
    df = frame_of(pl, data)
    cols = [("w", ("sum",)), ("v", ("sum", "min", "max"))]
    three_runs(pl, df, data, cols, pl.col("v") >= base, np.ones(n, bool), keyed, {"v": "affine16", "w": "affine8"}, "predicates: warm-up")
    ops = {"==": lambda a, b: a == b, "!=": lambda a, b: a != b, "<": lambda a, b: a < b, "<=": lambda a, b: a <= b, ">": lambda a, b: a > b, ">=": lambda a, b: a >= b}
    for const in (base - 1, base - 10**12, base + 299 * stride + 1, base + 17 * stride + 500, base + 17 * stride, base, base + 299 * stride):
        for name, f in ops.items():
            c = pl.col("v")
            e = {"==": c == const, "!=": c != const, "<": c < const, "<=": c <= const, ">": c > const, ">=": c >= const}[name]
            keep = f(v, const)
            lf = df.lazy().filter(e)
            lf = lf.group_by("g").agg(*aggs_of(pl, cols)) if keyed else lf.select(*aggs_of(pl, cols))
            out = lf.collect()
            assert encodings_in(pl.last_plan_encodings()).get("v") == "affine16", pl.last_plan_encodings()
            check(out, reference(data, cols, keep, data["g"][0] if keyed else None), keyed, ("predicate", name, const))


# ---- dictionary ----------------------------------------------------------------------------------------------------------------------------
def float_data(n):
    rng = np.random.default_rng(1000 + n)
    special = np.array([-0.0, 0.0, np.inf], np.float64).view(np.uint64)
    nans = np.array([0x7ff8000000000000, 0x7ff8000000000001], np.uint64)      # two NaN payloads: two entries
    pats = np.concatenate([special, nans, rng.normal(size=251).view(np.uint64)])      # 256 patterns
    fin = np.round(rng.integers(0, 11, n) / 100.0, 2)
    many = rng.normal(size=257)
    idx257 = rng.integers(0, 257, n)
    if n > 1000:
        idx257[:257] = np.arange(257)
    idx = rng.integers(0, 256, n)
    if n > 1000:
        idx[:256] = np.arange(256)
    return {
        "g": (rng.integers(0, 4, n).astype(np.uint8), None),
        "p": (rng.integers(0, 100, n).astype(np.int64), None),
        "d": (pats[idx].view(np.float64), None),
        "fin": (fin, None),
        "d257": (many[idx257], None),
    }


@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("n", ROWS)
def test_dictionary_columns(pl, n, keyed):
    data = float_data(n)
    df = frame_of(pl, data)
    keep = data["p"][0] >= 20
    expect = {"p": expected_affine(data["p"][0]), "d": expected_dict(data["d"][0]), "fin": expected_dict(data["fin"][0]), "d257": expected_dict(data["d257"][0])}
    assert expect["d"] == "dict8" and expect["fin"] == "dict8" and (n < 1000 or expect["d257"] is None)
    cols = [("d", ("sum", "min", "max")), ("fin", ("sum", "mean", "min", "max")), ("d257", ("sum", "min", "max"))]
    three_runs(pl, df, data, cols, pl.col("p") >= 20, keep, keyed, expect, ("dict", n))


# ---- nulls ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("n", [677, (1 << 18) + 5])
def test_null_rows_hold_values_far_outside_the_valid_range(pl, n, keyed):
    rng = np.random.default_rng(77 + n)
    iv, fv = rng.random(n) < 0.8, rng.random(n) < 0.8
    i = 500 + 3 * rng.integers(0, 200, n).astype(np.int64)
    i[~iv] = np.where(rng.random(int((~iv).sum())) < 0.5, -(1 << 62), 1 << 62)
    f = rng.integers(0, 9, n) / 100.0
    f[~fv] = rng.normal(size=300)[rng.integers(0, 300, int((~fv).sum()))]      # 300 more patterns, all under nulls
    data = {"g": (rng.integers(0, 4, n).astype(np.uint8), None), "i": (i, iv), "f": (f, fv)}
    df = frame_of(pl, data)
    cols = [("i", ("sum", "min", "max", "count")), ("f", ("sum", "min", "max", "count", "mean"))]
    expect = {"i": expected_affine(i, iv), "f": expected_dict(f, fv)}
    assert expect == {"i": "affine16", "f": "dict8"}
    three_runs(pl, df, data, cols, pl.col("g") < 3, data["g"][0] < 3, keyed, expect, ("nulls", n))


# ---- lifecycle -----------------------------------------------------------------------------------------------------------------------------
def small_frame(pl, n=677):
    rng = np.random.default_rng(9)
    data = {"g": (rng.integers(0, 4, n).astype(np.uint8), None), "v": (10 + rng.integers(0, 50, n).astype(np.int64), None), "x": (rng.integers(0, 9, n) / 100.0, None)}
    return data, frame_of(pl, data)


def small_query(pl, df):
    return df.lazy().filter(pl.col("v") > 12).group_by("g").agg(pl.col("v").sum().alias("s"), pl.col("x").sum().alias("xs"), pl.len().alias("n"))


def test_drop_statistics_drops_the_shadow_and_the_count(pl):
    data, df = small_frame(pl)
    plans = []
    for step in range(6):
        if step == 3:
            drop_statistics(pl, df)
        small_query(pl, df).collect()
        plans.append(encodings_in(pl.last_plan_encodings()))
    both = {"v": "affine8", "x": "dict8"}
    assert plans == [{}, both, both, {}, both, both], plans


def test_switch_turns_the_feature_off_in_a_fresh_process():
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\nimport polars_amd as pl\nimport test_gpu_encoded_inputs as T\npl.init(0)\n"
            "data, df = T.small_frame(pl)\nfor _ in range(4):\n    T.small_query(pl, df).collect()\n    assert pl.last_plan_encodings() == '', pl.last_plan_encodings()\nprint('never encoded')\n") % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PLX_ENCODED_INPUTS="0"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "never encoded" in r.stdout, r.stdout + r.stderr


def test_borrowed_buffers_never_encode(pl):
    import torch
    data, _ = small_frame(pl)
    tv, tx = torch.from_numpy(data["v"][0]).cuda(), torch.from_numpy(data["x"][0]).cuda()
    torch.cuda.synchronize()
    df = pl.DataFrame([pl.Series("g", data["g"][0]), pl.Series.from_torch("v", tv), pl.Series.from_torch("x", tx)])
    keep = data["v"][0] > 12
    for _ in range(4):
        out = small_query(pl, df).collect().to_dict()
        assert pl.last_plan_encodings() == "", pl.last_plan_encodings()
        assert sum(out["s"]) == int(data["v"][0][keep].sum()) and sum(out["n"]) == int(keep.sum())


# ---- program modes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [677, (1 << 18) + 5])
def test_encoded_q1_aot_jit_and_generic_agree(pl, n):
    """The encoded Q1 program through its ahead-of-time kernel, the run-time compiled kernel and the generic interpreter.  No switch takes the ahead-of-time kernel
    away from a shape that has one, so the other two run over the same rows with ONE null in l_quantity (row 0): a nullable input is a shape of its own, the program
    is the encoded Q1 program with a count beside the sum.  Each mode's third (encoded) run equals its own first (plain) run -- integers identical, f64 within RTOL --
    the two modes equal each other, and they equal the ahead-of-time run in every column l_quantity does not enter."""
    from polars_amd import datagen, queries
    F = pl._ffi
    li = datagen.lineitem_host(n, seed=33)
    lt = datagen.logical_dtypes(pl)
    want_enc = {"l_shipdate": "affine16", "l_quantity": "affine8", "l_discount": "dict8", "l_tax": "dict8"}
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
