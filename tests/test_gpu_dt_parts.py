"""The dt namespace on the GPU: the per-node kernel (Series.dt, plx_temporal_part) for every unit and part over the corpus of tests/dt_parts_ref.py, bit for bit;
fused programs with OP_DATEPART on the default route, per node (no_fusion) and with the run-time compiled kernel forced; (year, month) and month group-bys on
every route of the group-by driver; the expression plugin; queries.revenue_by_ship_month and queries.q6_year.  The reference is tests/dt_parts_ref.py throughout
(validated on the CPU by tests/test_dt_parts_cpu.py, which also pins the lowering and the programs themselves)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import dt_parts_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_TILES = 128 * 3 + 37          # full 128-row tiles of the fused scan, a ragged tail, validity words that end mid-word
RTOL = 1e-6                     # float sums against numpy, as tests/test_gpu_groupby_routes.py


def logical(pl, unit):
    return {"date": pl.Date, "ms": pl.Datetime("ms"), "us": pl.Datetime, "ns": pl.Datetime("ns")}[unit]


def out_logical(pl, part):
    return {"year": pl.Int32, "ordinal_day": pl.Int16, "date": pl.Date}.get(part, pl.Int8)


# ---- per node ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("unit", R.UNITS)
def test_series_dt_every_part_over_the_corpus(pl, unit, nullable):
    for n in (N_TILES, 0, 1, 63):
        v, valid = R.padded(unit, n, nullable)
        assert len(v) == n and (n != N_TILES or len(R.corpus(unit)[0]) <= n)          # the whole corpus is in
        s = pl.Series("when", v, logical(pl, unit), validity=valid)
        for part in R.PARTS:
            if not R.parts_of(unit, part):
                with pytest.raises(TypeError, match="needs a Datetime column"):
                    getattr(s.dt, part)()
                continue
            out = getattr(s.dt, part)()
            assert out.name == "when" and out.dtype == out_logical(pl, part) and out._query_dtype().np_dtype == R.out_dtype(part), (unit, part, out.dtype)
            got, got_valid = out._download()
            want = R.part(v, unit, part)
            assert got.dtype == want.dtype and np.array_equal(got, want), (unit, part, n, v[got != want][:4], got[got != want][:4], want[got != want][:4])      # null rows too
            if valid is None or valid.all():
                assert got_valid is None and out.null_count() == 0
            else:
                assert np.array_equal(got_valid, valid) and out.null_count() == int((~valid).sum()), (unit, part, n)


@pytest.mark.parametrize("unit", R.UNITS)
def test_values_borrowed_at_an_address_that_is_no_multiple_of_16(pl, unit):
    """Series.from_device over a buffer of the library's own, one element in: a Date column then starts 4 bytes, a Datetime column 8 bytes behind a 16-byte boundary, and
    the kernel takes its row-by-row form.  Held to the reference like the vector form; the rows next to the window are left alone."""
    v, _ = R.padded(unit, N_TILES + 1)
    base = pl.Series("base", v, logical(pl, unit))
    ptr = base.device_ptrs()[0]
    assert ptr % 16 == 0
    for skip, n in ((1, N_TILES), (1, 63), (1, 1), (3, 130)):
        s = pl.Series.from_device("when", logical(pl, unit), ptr + skip * v.itemsize, n, keepalive=base)
        assert s.device_ptrs()[0] % 16 != 0
        for part in R.PARTS:
            if R.parts_of(unit, part):
                got, got_valid = getattr(s.dt, part)()._download()
                want = R.part(v[skip:skip + n], unit, part)
                assert got_valid is None and got.dtype == want.dtype and np.array_equal(got, want), (unit, part, skip, n)
    assert np.array_equal(base._download()[0], v)


def test_the_entry_point_checks_its_operands(pl):
    import ctypes as C
    F = pl._ffi
    d, t, f = pl.Series("d", np.arange(5, dtype=np.int32), pl.Date), pl.Series("t", np.arange(5, dtype=np.int64), pl.Datetime), pl.Series("f", np.arange(5.0))
    h = C.c_uint64()
    for col, part, unit, msg in ((d, F.PART_YEAR, F.UNIT_US, "Int64"), (t, F.PART_YEAR, F.UNIT_DATE, "Int32"), (f, F.PART_YEAR, F.UNIT_US, "Int64"),
                                 (d, F.PART_HOUR, F.UNIT_DATE, "Datetime only"), (t, 10, F.UNIT_US, "out of range"), (t, 0, 4, "out of range")):
        with pytest.raises(pl.PlxError, match=msg):
            F.check(F.lib().plx_temporal_part(col._h, part, unit, C.byref(h)))
    with pytest.raises(TypeError, match="needs a Date or Datetime column"):
        f.dt.year()


def test_with_columns_select_and_an_unfusable_filter(pl):
    c = pl.col
    (d, dm), (t, _) = R.padded("date", N_TILES, True), R.padded("ns", N_TILES)
    df = pl.DataFrame([pl.Series("d", d, pl.Date, validity=dm), pl.Series("t", t, pl.Datetime("ns")), pl.Series("i", np.arange(N_TILES, dtype=np.int64))])
    out = df.lazy().with_columns(c("d").dt.year().alias("y"), c("t").dt.date().alias("day"), c("t").dt.date().dt.weekday().alias("wd")).select("i", "y", "day", "wd", c("t").dt.minute()).collect()
    assert "col('d').dt.year() [Date]" in pl.last_plan() and "col('t').dt.minute() [Datetime[ns]]" in pl.last_plan() and "per-node kernels" in pl.last_plan(), pl.last_plan()
    assert [out.schema[k] for k in ("y", "day", "wd", "t")] == [pl.Int32, pl.Date, pl.Int8, pl.Int8]
    res = out.to_dict()
    assert res["y"] == [int(v) if ok else None for v, ok in zip(R.part(d, "date", "year"), dm)]
    day = R.part(t, "ns", "date")
    assert res["day"] == day.tolist() and res["wd"] == R.part(day, "date", "weekday").tolist() and res["t"] == R.part(t, "ns", "minute").tolist()
    # a filter that keeps rows (nothing to aggregate: no fused scan) evaluates the part per node
    kept = df.lazy().filter((c("d").dt.month() <= 6) & (c("t").dt.hour() < 12)).select("i").collect().to_dict()["i"]
    assert kept == np.nonzero(dm & (R.part(d, "date", "month") <= 6) & (R.part(t, "ns", "hour") < 12))[0].tolist()


# ---- fused against per node -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    """About 5 000 rows: half drawn from the corpus, half ordinary dates of 1992..2003; d and t are nullable."""
    rng = np.random.default_rng(2030)
    n = 5003
    def draw(unit):
        corp, tpd = R.corpus(unit)[0], R.TICKS_PER_DAY[unit]
        return np.where(rng.random(n) < 0.5, corp[rng.integers(0, len(corp), n)], rng.integers(8035 * tpd, 12418 * tpd, n)).astype(corp.dtype)
    ones = np.ones(n, bool)
    cols = {"d": (draw("date"), rng.random(n) >= 1 / 3), "t": (draw("us"), rng.random(n) >= 1 / 3), "tn": (draw("ns"), ones), "x": (rng.normal(size=n), ones),
            "v": (rng.integers(-50, 50, n).astype(np.int64), rng.random(n) < 0.8), "flag": (rng.random(n) < 0.5, rng.random(n) < 0.75), "k": (rng.integers(0, 5, n).astype(np.int64), ones)}
    return n, cols


@pytest.fixture(scope="module")
def frame(pl, table):
    _, cols = table
    dts = {"d": pl.Date, "t": pl.Datetime, "tn": pl.Datetime("ns")}
    return pl.DataFrame([pl.Series(name, v, dts.get(name), validity=None if m.all() else m) for name, (v, m) in cols.items()])


def rows_by_key(out, keys):
    d = out.to_dict()
    return {tuple(d[k][i] for k in keys): {c: d[c][i] for c in d if c not in keys} for i in range(out.height)}


def three_ways(pl, q):
    """q on the default route, per node, and with the run-time compiled kernel forced (the switch of tests/test_gpu_when_then.py): [(name, result)]"""
    F = pl._ffi
    res = [("default", q.collect())]
    assert "Fused" in pl.last_plan() and "dt." in pl.last_plan(), pl.last_plan()
    res.append(("per_node", q.collect(no_fusion=True)))
    assert "Fused" not in pl.last_plan() or "materialised inputs" in pl.last_plan(), pl.last_plan()      # (a group-by then scans the columns the per-node kernels wrote)
    try:
        F.jit_set_min_rows(0)
        before = F.jit_stats()[0]
        res.append(("jit", q.collect()))
        assert "[jit]" in pl.last_plan() and F.jit_stats()[0] > before, pl.last_plan()
    finally:
        F.jit_set_min_rows(1 << 22)
    return res


def same(got, want):
    """exact for ints and None; floats within RTOL"""
    if isinstance(want, float) and got is not None:
        return bool(np.isclose(got, want, rtol=RTOL, atol=1e-9))
    return got == want


def test_filter_on_year_and_parts_as_aggregate_sources(pl, table, frame):
    n, cols = table
    c = pl.col
    q = (frame.lazy().filter((c("d").dt.year() == 2000) | (c("t").dt.month() == 12))
         .select(c("d").dt.day().cast(pl.Int64).sum().alias("s"), c("t").dt.ordinal_day().max().alias("mx"), c("tn").dt.hour().sum().alias("h"),
                 c("t").dt.second().count().alias("cnt"), c("x").sum().alias("sx"), pl.len().alias("n")))
    (d, dm), (t, tm), (tn, _), (x, _) = (cols[k] for k in ("d", "t", "tn", "x"))
    keep = ((R.part(d, "date", "year") == 2000) & dm) | ((R.part(t, "us", "month") == 12) & tm)
    want = {"s": int(R.part(d, "date", "day")[keep & dm].astype(np.int64).sum()), "mx": int(R.part(t, "us", "ordinal_day")[keep & tm].max()),
            "h": int(R.part(tn, "ns", "hour")[keep].astype(np.int64).sum()), "cnt": int((keep & tm).sum()), "sx": float(x[keep].sum()), "n": int(keep.sum())}
    assert 50 < want["n"] < n - 50
    results = three_ways(pl, q)
    for name, out in results:
        got = {k: v[0] for k, v in out.to_dict().items()}
        assert all(same(got[k], want[k]) for k in want), (name, got, want)
    ints = [{k: v for k, v in out.to_dict().items() if k != "sx"} for _, out in results]
    assert ints[0] == ints[1] == ints[2]


def group_reference(keys, valids, keep, aggs):
    want = {}
    for key in {tuple(int(k[i]) if m[i] else None for k, m in zip(keys, valids)) for i in np.nonzero(keep)[0]}:
        rows = keep.copy()
        for k, m, kv in zip(keys, valids, key):
            rows &= ~m if kv is None else (m & (k == kv))
        want[key] = {name: fn(rows) for name, fn in aggs.items()}
    return want


def assert_groups(got, want, what):
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want), key=str)[:6])
    for key, w in want.items():
        assert all(same(got[key][k], w[k]) for k in w), (what, key, got[key], w)


@pytest.mark.parametrize("col,unit", [("d", "date"), ("t", "us")])
def test_group_by_month_and_by_year_month(pl, table, frame, col, unit):
    n, cols = table
    c = pl.col
    (k, km), (x, _), (v, vm) = cols[col], cols["x"], cols["v"]
    aggs = [c("x").sum().alias("s"), c("v").sum().alias("vs"), c("v").min().alias("mn"), c("v").max().alias("mx"), pl.len().alias("n")]
    ref = {"s": lambda r: float(x[r].sum()), "vs": lambda r: int(v[r & vm].sum()), "mn": lambda r: int(v[r & vm].min()) if (r & vm).any() else None,
           "mx": lambda r: int(v[r & vm].max()) if (r & vm).any() else None, "n": lambda r: int(r.sum())}
    year, month = R.part(k, unit, "year"), R.part(k, unit, "month")
    want = group_reference([month], [km], np.ones(n, bool), ref)
    for name, out in three_ways(pl, frame.lazy().group_by(c(col).dt.month().alias("m")).agg(*aggs)):
        assert out.schema["m"] == pl.Int8
        assert_groups(rows_by_key(out, ["m"]), want, (col, "month", name))
    keep = km & (R.part(k, unit, "weekday") <= 5)
    want = group_reference([year, month], [km, km], keep, ref)
    for name, out in three_ways(pl, frame.lazy().filter(c(col).dt.weekday() <= 5).group_by(c(col).dt.year().alias("y"), c(col).dt.month().alias("m")).agg(*aggs)):
        assert out.schema["y"] == pl.Int32 and out.schema["m"] == pl.Int8
        assert_groups(rows_by_key(out, ["y", "m"]), want, (col, "year, month", name))


def test_a_part_inside_when_then(pl, table, frame):
    n, cols = table
    c = pl.col
    q = frame.lazy().group_by("k").agg(pl.when(c("d").dt.weekday() >= 6).then(c("x")).otherwise(0.0).sum().alias("weekend"),
                                       pl.when(c("flag")).then(c("t").dt.quarter().cast(pl.Int64)).otherwise(0).sum().alias("q"),
                                       pl.when(c("t").dt.minute() < 30).then(c("d").dt.day()).max().alias("mx"))
    (d, dm), (t, tm), (x, _), (flag, fm), (k, _) = (cols[nm] for nm in ("d", "t", "x", "flag", "k"))
    wk, fl, half = (R.part(d, "date", "weekday") >= 6) & dm, flag & fm, (R.part(t, "us", "minute") < 30) & tm
    want = {(kv,): {"weekend": float(x[(k == kv) & wk].sum()), "q": int(R.part(t, "us", "quarter")[(k == kv) & fl & tm].astype(np.int64).sum()),
                    "mx": int(R.part(d, "date", "day")[(k == kv) & half & dm].max())} for kv in range(5)}
    for name, out in three_ways(pl, q):
        assert_groups(rows_by_key(out, ["k"]), want, name)


def test_a_part_under_the_probe_side_predicate_of_a_join_pipeline(pl):
    c = pl.col
    rng = np.random.default_rng(33)
    nb, npr = 800, 6000
    bk, battr = rng.permutation(2000)[:nb].astype(np.int64), rng.integers(0, 6, nb).astype(np.int64)
    corp = R.corpus("date")[0]
    d = np.where(rng.random(npr) < 0.3, corp[rng.integers(0, len(corp), npr)], rng.integers(10957, 11688, npr)).astype(np.int32)
    dm, k, x = rng.random(npr) < 0.8, rng.integers(0, 2000, npr).astype(np.int64), rng.normal(size=npr)
    P = pl.DataFrame([pl.Series("k", k), pl.Series("d", d, pl.Date, validity=dm), pl.Series("x", x)])
    B = pl.DataFrame({"k": bk, "attr": battr})
    q = P.lazy().filter(c("d").dt.year() == 2000).join(B.lazy(), on="k").group_by("k", "attr").agg(c("x").sum().alias("s"), c("d").dt.month().max().alias("mm"), pl.len().alias("n"))
    attr_of = dict(zip(bk.tolist(), battr.tolist()))
    keep = dm & (R.part(d, "date", "year") == 2000) & np.isin(k, bk)
    month = R.part(d, "date", "month")
    want = {(kv, attr_of[kv]): {"s": float(x[keep & (k == kv)].sum()), "mm": int(month[keep & (k == kv)].max()), "n": int((keep & (k == kv)).sum())} for kv in set(k[keep].tolist())}
    assert len(want) > 100
    for name, out in three_ways(pl, q):
        assert_groups(rows_by_key(out, ["k", "attr"]), want, name)


# ---- the routes of the group-by driver ---------------------------------------------------------------------------------------------------------
def route_frame(pl, n, year_span, seed=5):
    """n rows of a nullable Date column whose years span `year_span` years from 1900, an Int64 and a Float64 value; tiled from one 2^16-row block, so the numpy reference
    is computed on the block (integer aggregates scale exactly, float sums within RTOL)."""
    rng = np.random.default_rng(seed)
    block = min(n, 1 << 16)
    reps = n // block
    assert reps * block == n
    lo = R.days_from_civil(1900, 1, 1)
    d = rng.integers(lo, R.days_from_civil(1900 + year_span, 1, 1), block).astype(np.int32)
    dm, v, x = rng.random(block) < 0.9, rng.integers(-1000, 1000, block).astype(np.int64), rng.normal(size=block)
    tile = lambda a: np.tile(a, reps)
    df = pl.DataFrame([pl.Series("d", tile(d), pl.Date, validity=tile(dm)), pl.Series("v", tile(v)), pl.Series("x", tile(x))])
    return df, (d, dm, v, x, reps)


def route_query(pl, df, keys):
    c = pl.col
    parts = {"y": c("d").dt.year().alias("y"), "m": c("d").dt.month().alias("m")}
    return df.lazy().group_by(*[parts[k] for k in keys]).agg(c("v").sum().alias("vs"), c("v").min().alias("mn"), c("v").max().alias("mx"), c("x").sum().alias("s"), pl.len().alias("n"))


def route_reference(block, keys):
    d, dm, v, x, reps = block
    part = {"y": R.part(d, "date", "year"), "m": R.part(d, "date", "month")}
    ref = {"vs": lambda r: int(v[r].sum()) * reps, "mn": lambda r: int(v[r].min()), "mx": lambda r: int(v[r].max()), "s": lambda r: float(x[r].sum()) * reps, "n": lambda r: int(r.sum()) * reps}
    return group_reference([part[k] for k in keys], [dm] * len(keys), np.ones(len(d), bool), ref)


ROUTES = [      # name, rows, years spanned, keys, collect flags, key ranges on, markers the plan must hold, markers it must not
    ("lds_table_year_month", 4096, 7, "ym", {}, True, ["lds_table(G="], ["partitioned(", "hbm_table"]),
    ("lds_table_month", 4096, 7, "m", {}, True, ["lds_table(G=16,"], ["partitioned(", "hbm_table"]),
    ("dense_hbm_table_year_month", 4096, 3000, "ym", {}, True, ["dense_hbm_table(G=65536)"], ["partitioned("]),
    ("hash_hbm_table_raw_year", 4096, 3000, "y", {}, False, ["hash_hbm_table(cap=2^"], ["partitioned(", "lds_table", "dense_hbm_table"]),
    ("hash_hbm_table_raw_month", 4096, 7, "m", {}, False, ["hash_hbm_table(cap=2^"], ["partitioned(", "lds_table"]),
    ("wide_hash_raw_year_month", 4096, 7, "ym", {}, False, ["wide_hash_hbm_table(words=3,cap=2^"], ["partitioned(", "lds_table"]),
    ("partitioned_packed_ids", 1 << 24, 3000, "ym", {}, True, [r"partitioned(v"], ["hbm_table"]),
    ("dense_hbm_table_no_partition", 1 << 24, 3000, "ym", {"no_partition": True}, True, ["dense_hbm_table(G=65536)"], ["partitioned("]),
    ("partitioned_single_key_raw_year", 1 << 24, 6000, "y", {}, False, [r"partitioned(v"], ["dense_hbm_table", "lds_table"]),
    ("partitioned_wide_keys_raw_year_month", 1 << 24, 600, "ym", {}, False, [r"partitioned(v", "lds_wide_key_table("], ["dense_hbm_table", "lds_table("]),
]


@pytest.mark.parametrize("name,n,span,keys,kw,ranges,want,never", ROUTES, ids=[r[0] for r in ROUTES])
def test_group_by_routes(pl, monkeypatch, name, n, span, keys, kw, ranges, want, never):
    """(year, month), year and month keys through the routes of run_fused_groupby.  With the key ranges of date parts switched off (PLX_TEMPORAL_KEY_RANGES=0) a part
    is a raw 64-bit key like any expression: the hash routes."""
    if not ranges:
        monkeypatch.setenv("PLX_TEMPORAL_KEY_RANGES", "0")
    df, block = route_frame(pl, n, span)
    out = route_query(pl, df, keys).collect(**kw)
    plan = pl.last_plan()
    print(f"plan[{name}]: {plan}")
    for w in want:
        assert w in plan, (w, plan)
    for w in never:
        assert w not in plan, (w, plan)
    if ranges and "y" in keys:
        assert "KeyRange{d.dt.year: 1900.." in plan, plan
    assert_groups(rows_by_key(out, list(keys)), route_reference(block, keys), name)


def test_first_generation_partition_kernels():
    """PLX_PART_V=1 is read once per process (the switch of tests/groupby_route_worker.py): a fresh child runs the packed (year, month) ids and the raw year key."""
    e = dict(os.environ)
    e["PLX_PART_V"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dt_route_worker.py")], capture_output=True, text=True, timeout=240, cwd=ROOT, env=e)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-1500:], r.stderr[-2500:])


# ---- the plugin, the queries ----------------------------------------------------------------------------------------------------------------------
def test_dt_part_through_the_plugin_abi(pl):
    import pyarrow as pa

    from tests import plugin_abi as P
    (d, dm), (t, tm) = R.padded("date", N_TILES, True), R.padded("ms", N_TILES, True)
    for arr, v, m, unit, kw_unit in ((pa.array(d, pa.int32(), mask=~dm).cast(pa.date32()), d, dm, "date", True), (pa.array(t, pa.int64(), mask=~tm).cast(pa.timestamp("ms")), t, tm, "ms", False)):
        for part in R.PARTS:
            kwargs = {"part": part, **({"unit": unit} if kw_unit else {})}          # without "unit" the input's Arrow format names it
            res, inp = P.call("plx_dt_part", [arr], kwargs, names=["when"])
            if not R.parts_of(unit, part):
                assert res is None and inp.released == 1 and "Datetime only" in P.last_error()
                continue
            want_type = {"year": pa.int32(), "ordinal_day": pa.int16(), "date": pa.date32()}.get(part, pa.int8())
            assert inp.released == 1 and inp.out_name == b"when" and res.type == want_type and res.null_count == int((~m).sum()), (unit, part, res.type)
            assert P.field("plx_dt_part", arr.type, kwargs, col_name="when") == pa.field("when", want_type)
            got = res.cast(pa.int32()).to_numpy(zero_copy_only=False) if part == "date" else res.to_numpy(zero_copy_only=False)
            assert np.array_equal(np.asarray(got[m], dtype=np.int64), R.part(v, unit, part)[m].astype(np.int64)), (unit, part)
    res, inp = P.call("plx_dt_part", [pa.array(d, pa.int32())], {"part": "year"})          # a plain Int32 series and no unit
    assert res is None and inp.released == 1 and "unit" in P.last_error()
    res, inp = P.call("plx_dt_part", [pa.array(d, pa.int32())], {"part": "fortnight", "unit": "date"})
    assert res is None and "part" in P.last_error()


def test_revenue_by_ship_month_and_q6_year(pl):
    from polars_amd import datagen, queries
    li = datagen.lineitem_host(20_000, seed=21)
    names = ("l_shipdate", "l_extendedprice", "l_discount", "l_quantity")
    df = datagen.to_frame(pl, li, names)
    ship, price, disc, qty = (li[k] for k in names)
    year, month = R.part(ship, "us", "year"), R.part(ship, "us", "month")
    keep = ship <= datagen.us(1998, 9, 2)
    rev = price * (1 - disc)
    ones = np.ones(len(ship), bool)
    want = group_reference([year, month], [ones, ones], keep, {"revenue": lambda r: float(rev[r].sum()), "n": lambda r: int(r.sum())})
    assert len(want) > 70
    for kw in ({}, {"no_fusion": True}):
        out = queries.revenue_by_ship_month(df.lazy()).collect(**kw)
        if not kw:
            assert "lds_table(G=" in pl.last_plan() and "KeyRange{l_shipdate.dt.year: 199" in pl.last_plan(), pl.last_plan()          # (year, month) packs into 3 + 4 bits
        assert_groups(rows_by_key(out, ["year", "month"]), want, kw)
    for y in (1994, 1997, 2005):
        sel = (year == y) & (disc >= 0.05) & (disc <= 0.07) & (qty < 24)
        got = [queries.q6_year(df.lazy(), y).collect(**kw).to_dict()["revenue"][0] for kw in ({}, {"no_fusion": True})]
        base = queries.q6(df.lazy(), y).collect().to_dict()["revenue"][0]
        assert got[0] == base, (y, got, base)                                                                       # the same rows, summed by the same kernel
        assert all(np.isclose(g, float((price * disc)[sel].sum()), rtol=RTOL) for g in got), (y, got)
