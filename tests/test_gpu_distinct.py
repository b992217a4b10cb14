"""n_unique / unique() on the device against tests/distinct_ref.py (canonical tokens: one NaN, -0 -> +0, a null a token of its own).  Every comparison is an exact
integer or an exact list of rows in row order; there is no tolerance.

Whole column (Series.n_unique -> plx_reduce_n_unique): per dtype the sizes around the ballot word, the one-workgroup sort and the sort tile, three validity patterns,
every legal route forced by PLX_NUNIQUE_ROUTE; the values that share a code with a null; the route bound.  Grouped (sorted segments shared with the quantiles): the
same sizes, the group shapes that decide a count, lists that share one sort, the three group-frame routes, a filter, an expression source, a join in front, the C
entries and the plugin symbol.  unique(): four keeps times three subsets at the same sizes, classes straddling a ballot word, null / NaN / Boolean keys, nine
columns refused, Series.unique, unique under a slice."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pytest

from tests import distinct_ref as D
from tests import groupby_route_inputs as R
from tests import plugin_abi as P

pytestmark = pytest.mark.gpu

NP = {"Int8": np.int8, "UInt16": np.uint16, "Int32": np.int32, "Int64": np.int64, "UInt64": np.uint64, "Float32": np.float32, "Float64": np.float64, "Boolean": np.bool_}
SIZES = (0, 1, 2, 63, 64, 65, 2048, 2049, 4097, 2 * 4096 + 5)
REASON = "n_unique: a distinct count (sorted-segment route)"
Q_REASON = "median / quantile: an order statistic (sorted-segment route)"
I64_MAX, I64_MIN, U64_MAX = (1 << 63) - 1, -(1 << 63), (1 << 64) - 1


def draw(rng, npdt, n):
    """n values with repeats: drawn from a pool of about n / 3 values of the dtype's whole range"""
    m = max(1, n // 3)
    if npdt == np.bool_:
        return rng.random(n) < 0.5
    if npdt == np.int64:
        pool = rng.integers(I64_MIN, I64_MAX, m, dtype=np.int64, endpoint=True)
    elif npdt == np.uint64:
        pool = rng.integers(0, U64_MAX, m, dtype=np.uint64, endpoint=True)
    elif np.issubdtype(npdt, np.integer):
        ii = np.iinfo(npdt)
        pool = rng.integers(ii.min, int(ii.max) + 1, m).astype(npdt)
    else:
        pool = rng.normal(0.0, 3.0, m).astype(npdt)
    return pool[rng.integers(0, m, n)] if n else pool[:0]


def frame_of(pl, cols, dtypes=None):
    return pl.DataFrame([pl.Series(name, v, (dtypes or {}).get(name), validity=m) for name, (v, m) in cols.items()])


def bitmap_legal(x, valid):
    """the rule of the bitmap route: an integer column (not UInt64) with a valid row whose exact range is at most max(64 n, 2^20) bits"""
    xs = x if valid is None else x[valid]
    if x.dtype.kind not in "iu" or x.dtype == np.uint64 or len(xs) == 0:
        return False
    return int(xs.max()) - int(xs.min()) + 1 <= max(64 * len(x), 1 << 20)


# ---- whole column --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(NP))
def test_series_n_unique_sizes_validity_routes(pl, monkeypatch, dtype):
    npdt = NP[dtype]
    rng = np.random.default_rng(160 + list(NP).index(dtype))
    checked = 0
    for n in SIZES:
        x = draw(rng, npdt, n)
        for name, valid in (("none", None), ("some", rng.random(n) < 0.7), ("all_null", np.zeros(n, bool))):
            want = D.n_unique(x, valid)
            assert (want == 0) == (n == 0) and (name != "all_null" or want == min(n, 1))
            s = pl.Series("x", x, getattr(pl, dtype), validity=valid)
            for route in ("", "bitmap", "sort"):
                if route:
                    monkeypatch.setenv("PLX_NUNIQUE_ROUTE", route)
                else:
                    monkeypatch.delenv("PLX_NUNIQUE_ROUTE", raising=False)
                got = s.n_unique()
                plan = pl.last_plan()
                assert got == want, (dtype, n, name, route, got, want, plan)
                if n == 0:
                    assert plan == "n_unique[empty]", plan
                elif dtype == "Boolean":
                    assert plan == "n_unique[boolean]", plan
                else:
                    legal = bitmap_legal(x, valid if name != "none" else None)
                    assert plan.startswith("n_unique[bitmap range=" if (legal and route != "sort") else "n_unique[sorted codes: passes="), (dtype, n, name, route, plan)
                checked += 1
    assert checked == len(SIZES) * 9


def test_special_values_in_one_column(pl, monkeypatch):
    monkeypatch.delenv("PLX_NUNIQUE_ROUTE", raising=False)
    rng = np.random.default_rng(161)
    n = 4097
    # INT64_MAX / UINT64_MAX share the code of a null: the value and the null count separately
    for npdt, top in ((np.int64, I64_MAX), (np.uint64, U64_MAX)):
        x = np.full(n, top, dtype=npdt)
        x[::3] = 5
        valid = rng.random(n) < 0.6
        valid[:6] = [True, True, True, False, False, False]
        for v, want in ((valid, 3), (None, 2), (x == top, 2), (x != top, 2)):
            s = pl.Series("x", x, validity=v)
            assert s.n_unique() == want == D.n_unique(x, v), (npdt, want, pl.last_plan())      # (an Int64 column whose valid rows all hold one value takes the bitmap)
            monkeypatch.setenv("PLX_NUNIQUE_ROUTE", "sort")
            assert s.n_unique() == want and "sorted codes" in pl.last_plan(), (npdt, want, pl.last_plan())
            monkeypatch.delenv("PLX_NUNIQUE_ROUTE")
        only = pl.Series("x", np.full(70, top, dtype=npdt), validity=np.arange(70) % 2 == 0)
        assert only.n_unique() == 2
    x = np.array([I64_MIN, I64_MIN, I64_MAX, 0, -1, I64_MIN + 1], np.int64)
    assert pl.Series("x", x).n_unique() == 5 and pl.Series("x", x, validity=np.array([1, 1, 0, 1, 1, 1], bool)).n_unique() == 5
    # floats: -0 == +0, every NaN is one value whatever its payload or sign, the infinities, f32 denormals
    nan2 = np.array([0x7FF8000000000001, 0xFFF8000000000000, 0x7FF0000000000001], np.uint64).view(np.float64)
    f = np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, 1.5, 1.5]), nan2])
    assert pl.Series("f", f).n_unique() == 5 == D.n_unique(f)
    assert pl.Series("f", f, validity=np.arange(len(f)) != 4).n_unique() == 6
    den = np.array([1, 2, 2, 0x80000001, 0, 0x80000000], np.uint32).view(np.float32)      # two denormals, a repeated one, a negative one, +0 and -0
    assert pl.Series("d", den).n_unique() == 4 == D.n_unique(den)
    # a constant column: every digit is skipped, no pass runs
    for npdt, val in ((np.float64, 0.1), (np.int64, -7), (np.uint64, U64_MAX)):
        s = pl.Series("c", np.full(n, val, dtype=npdt))
        monkeypatch.setenv("PLX_NUNIQUE_ROUTE", "sort")
        assert s.n_unique() == 1 and pl.last_plan() == "n_unique[sorted codes: passes=0, skipped=8]", pl.last_plan()
    monkeypatch.delenv("PLX_NUNIQUE_ROUTE")
    # the same column twice: the same count (integer OR / ADD atomics only)
    y = draw(rng, np.int32, 100_003) % 5000
    assert pl.Series("y", y).n_unique() == pl.Series("y", y).n_unique() == D.n_unique(y)


def test_the_bitmap_bound_names_the_route(pl, monkeypatch):
    monkeypatch.delenv("PLX_NUNIQUE_ROUTE", raising=False)
    rng = np.random.default_rng(162)
    for n, bound in ((1000, 1 << 20), (20_000, 64 * 20_000)):          # the 128 KB floor, and 8 B a row above it
        for span, legal in ((bound, True), (bound + 1, False)):
            x = rng.integers(0, span, n).astype(np.int64) - 12345
            x[0], x[1] = -12345, -12345 + span - 1                      # the exact range is `span`
            valid = np.ones(n, bool); valid[5] = False
            s = pl.Series("x", x, validity=valid)
            assert s.n_unique() == D.n_unique(x, valid)
            assert pl.last_plan().startswith("n_unique[bitmap range=%d]" % span if legal else "n_unique[sorted codes: passes="), (n, span, pl.last_plan())
            monkeypatch.setenv("PLX_NUNIQUE_ROUTE", "bitmap")           # "bitmap" names the default rule: outside the bound it changes nothing
            assert s.n_unique() == D.n_unique(x, valid) and ("bitmap" in pl.last_plan()) == legal
            monkeypatch.delenv("PLX_NUNIQUE_ROUTE")
    # Date / Datetime / Categorical columns are integer columns: Categorical compares codes
    d = rng.integers(8000, 8100, 500).astype(np.int32)
    assert pl.Series("d", d, pl.Date).n_unique() == D.n_unique(d) and "bitmap" in pl.last_plan()
    t = rng.integers(0, 1 << 50, 500).astype(np.int64)
    assert pl.Series("t", t, pl.Datetime).n_unique() == D.n_unique(t) and "sorted codes" in pl.last_plan()
    cat = pl.Series("s", ["b", "a", None, "b", "c", "a"])
    assert cat.n_unique() == 4


# ---- grouped -------------------------------------------------------------------------------------------------------------------------------------
def host_groups(keys, keep):
    """{key tuple: row indices} over the rows of `keep`, in first-occurrence order"""
    parts = [D.tokens(v, m) for v, m in keys]
    groups = {}
    for r in np.nonzero(keep)[0]:
        groups.setdefault(tuple(p[r] for p in parts), []).append(r)
    return {k: np.array(rows) for k, rows in groups.items()}


def check_counts(out, key_names, groups, sources, specs, what):
    """every output row of every n_unique column against the reference over its group's rows; returns the key tuples in output order"""
    d = R.download(out)
    assert out.height == len(groups), (what, out.height, len(groups))
    kparts = [D.tokens(d[k][0], d[k][1]) for k in key_names]
    seen = []
    for r in range(out.height):
        kt = tuple(p[r] for p in kparts)
        assert kt in groups and kt not in seen, (what, "unknown or repeated group", kt)
        seen.append(kt)
        rows = groups[kt]
        for name, src in specs.items():
            v, m = sources[src]
            gv, gm = d[name]
            assert gm is None and gv.dtype == np.uint32, (what, name, "UInt32, never null")
            want = D.n_unique(v[rows], None if m is None else m[rows])
            assert int(gv[r]) == want >= 1, (what, kt, name, int(gv[r]), want)
    return seen


@pytest.mark.parametrize("n", SIZES)
def test_group_by_sizes(pl, n):
    """the sizes of the whole-column test; 0 rows: no group, the UInt32 column and the plan clause all the same"""
    rng = np.random.default_rng(300 + n)
    x, xm = rng.integers(0, 12, n).astype(np.float64), rng.random(n) > 0.2
    keyings = {"one group": np.zeros(n, np.int32), "every row its own group": rng.permutation(n).astype(np.int32), "a few": rng.integers(-2, 3, n).astype(np.int32)}
    for kname, k in keyings.items():
        df = frame_of(pl, {"k": (k, None), "x": (x, xm)})
        out = df.lazy().group_by("k").agg(pl.col("x").n_unique().alias("nu")).collect()
        plan = pl.last_plan()
        assert "n_unique[sorted segments: " in plan and "sources=1, outputs=1]" in plan and REASON in plan and "quantile[" not in plan, plan
        assert out["nu"].dtype == pl.UInt32 and out.columns == ["k", "nu"]
        if n == 0:
            assert out.height == 0 and "groups=0, sources=1, outputs=1]" in plan, plan
        check_counts(out, ["k"], host_groups([(k, None)], np.ones(n, bool)), {"x": (x, xm)}, {"nu": "x"}, (n, kname))


def test_group_by_after_a_filter_that_keeps_nothing(pl):
    """no row reaches the group-by: no segment, no group, and the list beside a median and a mean comes out empty with its dtypes"""
    rng = np.random.default_rng(299)
    n = 1000
    k, x = rng.integers(0, 5, n).astype(np.int32), rng.integers(0, 9, n).astype(np.float64)
    df = frame_of(pl, {"k": (k, None), "x": (x, rng.random(n) > 0.2)})
    c = pl.col
    for names, aggs, clause in ((["nu"], [c("x").n_unique().alias("nu")], "n_unique[sorted segments: "),
                                (["med", "nu", "m"], [c("x").median().alias("med"), c("x").n_unique().alias("nu"), c("x").mean().alias("m")],
                                 "n_unique[sorted segments: shares the sort of source 0, groups=0, sources=1, outputs=1]")):
        for mo in (False, True):
            out = df.lazy().filter(c("k") > 100).group_by("k", maintain_order=mo).agg(*aggs).collect()
            plan = pl.last_plan()
            assert out.height == 0 and out["nu"].dtype == pl.UInt32 and out["k"].dtype == pl.Int32 and out.columns == ["k"] + names, plan
            assert clause in plan and "groups=0, " in plan and (Q_REASON if "med" in names else REASON) in plan, plan
            assert len(out["nu"].to_numpy()) == 0
    assert df.lazy().filter(c("k") > 100).select(c("x").n_unique().alias("nu")).collect()["nu"].to_numpy().tolist() == [0]


def test_group_shapes_that_decide_a_count(pl):
    rng = np.random.default_rng(301)
    # 64 rows of key 0, 128 of key 1, 7 of key 2: the segment heads sit at bit 0 of three ballot words
    k = np.repeat(np.array([0, 1, 2], np.int16), [64, 128, 7])
    rng.shuffle(k)
    x = rng.integers(0, 5, len(k)).astype(np.int64)
    out = frame_of(pl, {"k": (k, None), "x": (x, None)}).lazy().group_by("k").agg(pl.col("x").n_unique().alias("nu")).collect()
    check_counts(out, ["k"], host_groups([(k, None)], np.ones(len(k), bool)), {"x": (x, None)}, {"nu": "x"}, "boundary")
    # groups that differ only by null versus value in the source; a NaN / -0 source; null keys; INT64_MAX beside nulls inside a group
    n = 600
    kf = rng.integers(0, 6, n).astype(np.float64)
    kf[rng.random(n) < 0.1] = np.nan
    km = rng.random(n) > 0.1
    x = rng.integers(0, 3, n).astype(np.float64)
    x[rng.random(n) < 0.2] = np.nan
    x[rng.random(n) < 0.2] = -0.0
    xm = rng.random(n) > 0.3
    xm[kf == 1.0] = False                                             # all null: 1
    xm[kf == 2.0] = True; x[kf == 2.0] = 7.0                          # one value, no null: 1
    g3 = np.nonzero(kf == 3.0)[0]
    x[g3] = 7.0; xm[g3] = True; xm[g3[0]] = False                     # the same value and one null: 2
    big = np.where(rng.random(n) < 0.5, I64_MAX, 3).astype(np.int64)
    bm = rng.random(n) > 0.4
    cols = {"k": (kf, km), "x": (x, xm), "big": (big, bm)}
    out = frame_of(pl, cols).lazy().group_by("k").agg(pl.col("x").n_unique().alias("nu"), pl.col("big").n_unique().alias("nb")).collect()
    assert "sources=2, outputs=2]" in pl.last_plan(), pl.last_plan()
    groups = host_groups([(kf, km)], np.ones(n, bool))
    assert D.NULL in {g[0] for g in groups} and "nan" in {g[0] for g in groups}
    check_counts(out, ["k"], groups, cols, {"nu": "x", "nb": "big"}, "null versus value")
    d = out.to_dict()
    row = {D.canon(kv, kv is not None): i for i, kv in enumerate(d["k"])}
    assert (d["nu"][row[1.0]], d["nu"][row[2.0]], d["nu"][row[3.0]]) == (1, 1, 2)
    # 2 and 8 key columns, nulls in key parts, a Boolean source
    keys = {"k%d" % j: (rng.integers(0, 2, n).astype([np.int8, np.int64, np.uint16, np.int32][j % 4]), rng.random(n) > 0.1 if j % 3 == 0 else None) for j in range(8)}
    flag, fm = rng.random(n) < 0.5, rng.random(n) > 0.3
    for nk in (2, 8):
        names = list(keys)[:nk]
        cols = dict({kk: keys[kk] for kk in names}, x=(x, xm), flag=(flag, fm))
        out = frame_of(pl, cols).lazy().group_by(*names).agg(pl.col("x").n_unique().alias("nu"), pl.col("flag").n_unique().alias("nf")).collect()
        check_counts(out, names, host_groups([keys[kk] for kk in names], np.ones(n, bool)), cols, {"nu": "x", "nf": "flag"}, ("keys", nk))


def test_lists_share_one_sort_per_source_and_keep_the_group_order(pl):
    rng = np.random.default_rng(302)
    n = 3000
    k = R.sparse(rng.integers(0, 37, n))
    x, xm = rng.integers(0, 40, n).astype(np.float64), rng.random(n) > 0.1
    y = rng.integers(-5, 5, n).astype(np.int32)
    cols = {"k": (k, None), "x": (x, xm), "y": (y, None)}
    df = frame_of(pl, cols)
    c = pl.col
    groups = host_groups([(k, None)], np.ones(n, bool))
    aggs = [c("x").median().alias("med"), c("x").n_unique().alias("nu"), c("x").mean().alias("m"), c("y").n_unique().alias("ny")]
    for mo in (False, True):
        out = df.lazy().group_by("k", maintain_order=mo).agg(*aggs).collect()
        plan = pl.last_plan()
        # one sort for x (the median's; the distinct count shares it), one for y
        assert "quantile[sorted segments: " in plan and "sources=1, outputs=1]; n_unique[sorted segments: shares the sort of source 0 + " in plan and "sources=2, outputs=2]" in plan, plan
        assert plan.count("sort[rows=%d," % n) == 2 and Q_REASON in plan, plan
        order = check_counts(out, ["k"], groups, cols, {"nu": "x", "ny": "y"}, ("list", mo))
        d = out.to_dict()
        for r, kt in enumerate(order):
            xs = x[groups[kt]][xm[groups[kt]]]
            assert d["med"][r] == float(np.median(xs)) and abs(d["m"][r] - xs.mean()) < 1e-9
        # the group order of the same query without the new aggregate: the same list minus its n_unique entries, through the same route
        plain = df.lazy().group_by("k", maintain_order=mo).agg(c("x").median().alias("med"), c("x").mean().alias("m")).collect().to_dict()
        assert "quantile[sorted segments: " in pl.last_plan() and "n_unique[" not in pl.last_plan(), pl.last_plan()
        # maintain_order=True defines the order (first occurrence) and the list keeps it row for row.  Without it the engine's group order is unspecified: these 37 sparse
        # keys take a hash table whose slots are claimed by atomics, and the same query run twice comes out in two orders -- there the same groups with the same medians
        # are all there is to compare
        if mo:
            assert d["k"] == plain["k"] and d["med"] == plain["med"] and [kt[0] for kt in order] == list(dict.fromkeys(k.tolist()))
        else:
            assert sorted(zip(d["k"], d["med"])) == sorted(zip(plain["k"], plain["med"]))
    out = df.group_by("k").n_unique()
    assert out.columns == ["k", "x", "y"] and out["x"].dtype == pl.UInt32
    check_counts(out, ["k"], groups, cols, {"x": "x", "y": "y"}, "GroupBy.n_unique")


ROUTE_WORD = {"lds": "lds_table(", "dense": "dense_hbm_table(", "hash": "]+hash_hbm_table("}


@pytest.mark.parametrize("route", ["lds", "dense", "hash"])
def test_group_frame_routes(pl, monkeypatch, route):
    monkeypatch.setenv("PLX_LEARN_DENSE_RANGE", "0")
    rng = np.random.default_rng(303 + list(ROUTE_WORD).index(route))
    n = 6000
    if route == "lds":
        k = (rng.integers(0, 4, n) - 1).astype(np.int16)
    elif route == "dense":
        ids = rng.integers(0, 40, n) * 1249
        ids[0], ids[1] = 0, 49_999
        k = ids.astype(np.uint16)
    else:
        k = R.sparse(rng.integers(0, 40, n))
    km = rng.random(n) > 0.05
    x, xm = rng.integers(0, 30, n).astype(np.int64), rng.random(n) > 0.15
    cols = {"k": (k, km), "x": (x, xm)}
    out = frame_of(pl, cols).lazy().group_by("k").agg(pl.col("x").n_unique().alias("nu"), pl.col("x").mean().alias("m"), pl.len().alias("n")).collect(**({"no_partition": True} if route == "hash" else {}))
    plan = pl.last_plan()
    assert ROUTE_WORD[route] in plan and "n_unique[sorted segments: " in plan, plan
    groups = host_groups([(k, km)], np.ones(n, bool))
    order = check_counts(out, ["k"], groups, cols, {"nu": "x"}, route)
    d = out.to_dict()
    for r, kt in enumerate(order):
        assert d["n"][r] == len(groups[kt])


def test_filter_in_front_expression_source_and_select(pl):
    rng = np.random.default_rng(304)
    n = 2500
    k = rng.integers(0, 9, n).astype(np.int16)
    a, b = rng.integers(-3, 4, n).astype(np.int64), rng.integers(-2, 3, n).astype(np.int64)
    bm = rng.random(n) > 0.1
    x = rng.normal(size=n)
    cols = {"k": (k, None), "a": (a, None), "b": (b, bm), "x": (x, None), "ab": (a * b, bm)}
    df = frame_of(pl, {kk: cols[kk] for kk in ("k", "a", "b", "x")})
    c = pl.col
    keep = (x > -0.5) & (k != 4)
    out = df.lazy().filter((c("x") > -0.5) & (c("k") != 4)).group_by("k").agg((c("a") * c("b")).n_unique().alias("nab"), c("a").n_unique().alias("na"), c("a").min().alias("amin")).collect()
    assert "n_unique[sorted segments: " in pl.last_plan() and "sources=2, outputs=2]" in pl.last_plan(), pl.last_plan()
    groups = host_groups([(k, None)], keep)
    assert (4,) not in groups and len(groups) == 8
    order = check_counts(out, ["k"], groups, cols, {"nab": "ab", "na": "a"}, "filtered")
    assert out.to_dict()["amin"] == [int(a[groups[kt]].min()) for kt in order]
    for lf, kp in ((df.lazy(), np.ones(n, bool)), (df.lazy().filter(c("x") > -0.5), x > -0.5)):
        out = lf.select((c("a") * c("b")).n_unique().alias("nab"), c("x").n_unique().alias("nx"), pl.n_unique("k").alias("nk")).collect()
        plan = pl.last_plan()
        assert "n_unique[bitmap range=" in plan and "n_unique[sorted codes: " in plan and REASON in plan, plan
        g = {kk: v[0] for kk, v in out.to_dict().items()}
        assert out["nab"].dtype == pl.UInt32 and g == {"nab": D.n_unique((a * b)[kp], bm[kp]), "nx": D.n_unique(x[kp]), "nk": D.n_unique(k[kp])}


def test_join_then_group_by_c_entries_and_the_plugin_symbol(pl):
    F = pl._ffi
    rng = np.random.default_rng(305)
    nb, n = 50, 3000
    bk = R.sparse(rng.permutation(1000)[:nb])
    g = rng.integers(0, 6, nb).astype(np.int16)
    pk = bk[rng.integers(0, nb, n)]
    pk[rng.random(n) < 0.1] = 12345
    w = rng.integers(0, 25, n).astype(np.int64)
    build = frame_of(pl, {"k": (bk, None), "g": (g, None)})
    probe = frame_of(pl, {"k": (pk, None), "w": (w, None)})
    out = probe.lazy().join(build.lazy(), on="k").group_by("g").agg(pl.col("w").n_unique().alias("nw"), pl.len().alias("n")).collect()
    assert "n_unique[sorted segments: " in pl.last_plan(), pl.last_plan()
    g_of = dict(zip(bk.tolist(), g.tolist()))
    hit = np.array([kk in g_of for kk in pk.tolist()])
    jg = np.array([g_of.get(kk, -1) for kk in pk.tolist()], np.int16)
    check_counts(out, ["g"], host_groups([(jg, None)], hit), {"w": (w, None)}, {"nw": "w"}, "join")
    # the C entries: plx_reduce_n_unique; plx_reduce points to it; all three group-by entries take the kind
    s, ks = pl.Series("w", w), pl.Series("k", (pk % 7).astype(np.int16))
    u = C.c_uint32()
    F.check(F.lib().plx_reduce_n_unique(s._h, C.byref(u)))
    assert u.value == D.n_unique(w)
    v, dt, ok = F.Scalar(), C.c_int32(), C.c_int32()
    assert F.lib().plx_reduce(F.AGG_N_UNIQUE, s._h, C.byref(v), C.byref(dt), C.byref(ok)) == 1 and "plx_reduce_n_unique" in F.lib().plx_last_error().decode()
    keys, vals, aggs = (C.c_uint64 * 1)(ks._h), (C.c_uint64 * 2)(s._h, s._h), (C.c_int32 * 2)(F.AGG_N_UNIQUE, F.AGG_MEAN)
    groups = host_groups([((pk % 7).astype(np.int16), None)], np.ones(n, bool))
    for entry in ("plx_groupby_agg", "plx_groupby_agg_ddof", "plx_groupby_agg_params"):
        ok_, oa = (C.c_uint64 * 1)(), (C.c_uint64 * 2)()
        extra = {"plx_groupby_agg": (), "plx_groupby_agg_ddof": (None,), "plx_groupby_agg_params": (None, None, None)}[entry]
        F.check(getattr(F.lib(), entry)(keys, 1, vals, aggs, 2, 0, *extra, ok_, oa))
        assert "n_unique[sorted segments: " in pl.last_plan() and "sources=1, outputs=1]" in pl.last_plan(), pl.last_plan()
        gk = pl.Series._from_handle("k", ok_[0], pl.Int16).to_numpy()
        nu = pl.Series._from_handle("nu", oa[0], pl.UInt32)
        assert nu.null_count() == 0 and [int(t) for t in nu.to_numpy()] == [D.n_unique(w[groups[(int(kv),)]]) for kv in gk], entry
    # plx_distinct_mask
    h = C.c_uint64()
    F.check(F.lib().plx_distinct_mask(keys, 1, F.UNIQUE_LAST, C.byref(h)))
    mask = pl.Series._from_handle("m", h.value, pl.Boolean)
    assert np.nonzero(mask.to_numpy())[0].tolist() == D.unique_rows([((pk % 7).astype(np.int16), None)], "last") and "distinct_mask[keep=last, " in pl.last_plan()
    assert F.lib().plx_distinct_mask(keys, 1, 4, C.byref(h)) == 1 and "plx_unique_keep" in F.lib().plx_last_error().decode()
    nine = (C.c_uint64 * 9)(*([ks._h] * 9))
    assert F.lib().plx_distinct_mask(nine, 9, 0, C.byref(h)) == F.ERR_UNSUPPORTED and "1..8 columns, got 9" in F.lib().plx_last_error().decode()
    # the plugin symbol: a chunked input with nulls, UInt32 under the input's name
    valid = rng.random(n) < 0.8
    arr = pa.array(w, mask=~valid)
    res, inp = P.call("plx_n_unique", [pa.chunked_array([arr.slice(0, 400), arr.slice(400)])], None, names=["w"])
    assert res is not None, P.last_error()
    assert inp.released == 1 and len(res) == 1 and res.type == pa.uint32() and inp.out_name == b"w" and res[0].as_py() == D.n_unique(w, valid)
    res, _ = P.call("plx_n_unique", [pa.array([True, None, True])])
    assert res is not None and res[0].as_py() == 2


# ---- unique() ------------------------------------------------------------------------------------------------------------------------------------
def rows_of(out, cols):
    """the output frame as a list of token tuples, one per row, in output order"""
    d = R.download(out)
    parts = [D.tokens(d[name][0], d[name][1]) for name in cols]
    return list(zip(*parts)) if out.height else []


@pytest.mark.parametrize("n", SIZES)
def test_unique_keeps_subsets_and_sizes(pl, n):
    rng = np.random.default_rng(400 + n)
    a, am = rng.integers(0, max(2, n // 4), n).astype(np.int64), rng.random(n) > 0.1
    b = rng.integers(0, 3, n).astype(np.float64)
    b[rng.random(n) < 0.1] = np.nan
    b[rng.random(n) < 0.1] = -0.0
    flag, fm = rng.random(n) < 0.5, rng.random(n) > 0.2
    cols = {"a": (a, am), "b": (b, None), "flag": (flag, fm)}
    df = frame_of(pl, cols)
    parts = [D.tokens(*cols[name]) for name in cols]
    all_rows = list(zip(*parts)) if n else []
    for subset in (None, "a", ["b", "flag"]):
        names = list(cols) if subset is None else [subset] if isinstance(subset, str) else subset
        for keep in D.KEEPS:
            want = D.unique_rows([cols[name] for name in names], keep)
            out = df.unique(subset, keep=keep, maintain_order=bool(n % 2))
            plan = pl.last_plan()
            assert rows_of(out, list(cols)) == [all_rows[r] for r in want], (n, subset, keep, plan)      # unsorted: row order is the contract
            served = "first (asked: any)" if keep == "any" else keep
            assert "Distinct{subset=[%s], keep=%s, order=rows, " % (", ".join(names), served) in plan and "kept=%d of %d}" % (len(want), n) in plan, plan


def test_unique_class_shapes(pl):
    rng = np.random.default_rng(401)
    # duplicates straddling a multiple of 64: in the sorted order class 1 covers positions 60..69, class 2 starts at 128
    k = np.repeat(np.array([0, 1, 2, 3], np.int32), [60, 10, 58, 40])
    rng.shuffle(k)
    v = np.arange(len(k), dtype=np.int64)
    df = frame_of(pl, {"k": (k, None), "v": (v, None)})
    for keep in D.KEEPS:
        want = D.unique_rows([(k, None)], keep)
        assert df.unique("k", keep=keep)["v"].to_numpy().tolist() == want, keep
    # all rows equal; no duplicates
    same = frame_of(pl, {"k": (np.full(200, 7, np.int16), None), "v": (np.arange(200), None)})
    assert same.unique("k", keep="first")["v"].to_numpy().tolist() == [0] and same.unique("k", keep="last")["v"].to_numpy().tolist() == [199] and same.unique("k", keep="none").height == 0
    perm = rng.permutation(3000).astype(np.int64)
    nodup = frame_of(pl, {"k": (perm, None)})
    for keep in D.KEEPS:
        assert nodup.unique(keep=keep)["k"].to_numpy().tolist() == perm.tolist()
    # null and NaN keys: null == null, NaN == NaN, a null is no NaN
    x = np.array([np.nan, 1.0, np.nan, 0.0, -0.0, 2.0, 2.0, 1.0])
    xm = np.array([1, 1, 1, 1, 1, 0, 0, 1], bool)
    fx = frame_of(pl, {"x": (x, xm), "i": (np.arange(8), None)})
    assert fx.unique("x", keep="first")["i"].to_numpy().tolist() == [0, 1, 3, 5] == D.unique_rows([(x, xm)], "first")
    assert fx.unique("x", keep="last")["i"].to_numpy().tolist() == [2, 4, 6, 7] and fx.unique("x", keep="none").height == 0
    # nine subset columns are refused by name; an unknown keep and an unknown column
    nine = frame_of(pl, {"c%d" % j: (np.arange(5), None) for j in range(9)})
    with pytest.raises(pl.UnsupportedError, match="subset of 9 columns.*1..8"):
        nine.unique()
    assert nine.unique(["c%d" % j for j in range(8)]).height == 5
    with pytest.raises(ValueError, match="keep must be one of"):
        nine.unique(keep="some")
    with pytest.raises(KeyError, match="zz"):
        nine.unique("zz")
    # Series.unique: first-occurrence order; unique under a slice, and a slice under unique
    s = pl.Series("k", k)
    first = list(dict.fromkeys(k.tolist()))
    assert s.unique().to_numpy().tolist() == first == s.unique(maintain_order=True).to_numpy().tolist() and "distinct_mask[keep=first, " in pl.last_plan()
    big = frame_of(pl, {"k": (rng.integers(0, 50, 5000).astype(np.int64), None), "v": (np.arange(5000), None)})
    kk = big["k"].to_numpy()
    assert big.lazy().unique("k", keep="last").slice(3, 10).collect()["v"].to_numpy().tolist() == D.unique_rows([(kk, None)], "last")[3:13]
    assert big.lazy().slice(100, 3000).unique("k", keep="first").collect()["v"].to_numpy().tolist() == [100 + r for r in D.unique_rows([(kk[100:3100], None)], "first")]
    lf = big.lazy().unique("k")
    lf.collect()
    assert "Distinct[subset=[k], keep=first (asked: any), order=rows]" in lf.explain() and "Distinct{subset=[k]" in lf.explain()
