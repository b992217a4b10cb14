"""median / quantile on the device against tests/quantile_ref.py (numpy: sort in the native dtype with NaN last, pick two values, the rule of DESIGN.md 4.15).

Acceptance (quantile_ref.accept): nearest / lower / higher / midpoint equal as f64 values, NaN matching NaN; linear within 2 * 2^-53 * (|a| + |b|) -- a function of
the two picked values, no rtol; Float32 outputs within one f32 ulp of the reference rounded to f32.  |values| stay far below 1e300.

Per node (Series.quantile -> plx_reduce_quantile -> the radix select): seven dtypes, the sizes at which a kernel takes another path (one workgroup, a grid-stride
loop, several workgroups), the validity patterns, five interpolations times six q; the digit-round edges; NaN / inf / -0.0; the C entry points and the plugin symbol.
Grouped (sorted segments): the sizes around the ballot word, the one-workgroup rank sort and the sort tile, every kind of group that decides between null and a
value or that the sort's equality joins, mixed aggregate lists, maintain_order, a filter and an expression source, the three routes of the group frame, a join in
front, the C entry points."""
import ctypes as C
import math
import struct

import numpy as np
import pyarrow as pa
import pytest

from tests import groupby_route_inputs as R
from tests import plugin_abi as P
from tests import quantile_ref as Q

pytestmark = pytest.mark.gpu

NP = {"Int8": np.int8, "UInt16": np.uint16, "Int32": np.int32, "Int64": np.int64, "UInt64": np.uint64, "Float32": np.float32, "Float64": np.float64}
K_BLOCK = 256                         # csrc/kconfig.hpp
ALL = [(q, it) for it in Q.INTERPOLATIONS for q in Q.QS]


def bits(x):
    return None if x is None else struct.pack("<d", x)


def draw(rng, npdt, n):
    if npdt == np.int64:
        return rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64, endpoint=True)      # the full range: above 2^53 in magnitude almost surely
    if npdt == np.uint64:
        return rng.integers(0, 1 << 64, n, dtype=np.uint64)      # above 2^63: a signed conversion would show
    if np.issubdtype(npdt, np.integer):
        ii = np.iinfo(npdt)
        return rng.integers(ii.min, int(ii.max) + 1, n).astype(npdt)
    return rng.normal(10.0, 3.0, n).astype(npdt)


def frame_of(pl, cols, dtypes=None):
    return pl.DataFrame([pl.Series(name, v, (dtypes or {}).get(name), validity=m) for name, (v, m) in cols.items()])


# ---- per node ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(NP))
def test_series_quantile_sizes_validity_interpolations(pl, dtype):
    npdt = NP[dtype]
    rng = np.random.default_rng(70 + list(NP).index(dtype))
    n_checked = 0
    for n in (0, 1, 2, K_BLOCK - 1, K_BLOCK, K_BLOCK + 1, 2 * K_BLOCK * 8 + 5):
        x = draw(rng, npdt, n)
        patterns = {"none": None, "half": rng.random(n) < 0.5, "all_null": np.zeros(n, bool)}
        if n >= 1:
            one = np.zeros(n, bool); one[rng.integers(0, n)] = True
            last = np.zeros(n, bool); last[n - 1] = True
            patterns.update(one_valid=one, only_last=last)
        for name, valid in patterns.items():
            s = pl.Series("x", x, getattr(pl, dtype), validity=valid)
            xs = x if valid is None else x[valid]
            for q, it in ALL:
                got = s.quantile(q, it)
                assert Q.accept(got, xs, q, it, f32=dtype == "Float32"), (dtype, n, name, q, it, got, Q.ref_quantile(xs, q, it))
                n_checked += 1
            assert Q.accept(s.median(), xs, 0.5, "linear", f32=dtype == "Float32"), (dtype, n, name)
            if len(xs) == 0:
                assert s.median() is None and s.quantile(0.0) is None
    assert n_checked >= 30 * 30


def test_series_digit_rounds_and_special_values(pl):
    n = 2 * K_BLOCK * 8 + 5
    rng = np.random.default_rng(71)
    # a constant column: every valid row agrees on every digit below the first round
    for npdt, val in ((np.float64, 0.1), (np.float64, -1e299), (np.int32, -7), (np.uint64, (1 << 64) - 1), (np.float32, 3.3), (np.int64, -(1 << 63))):
        s = pl.Series("c", np.full(n, val, dtype=npdt))
        for q, it in ALL:
            assert Q.accept(s.quantile(q, it), np.full(3, val, dtype=npdt), q, it, f32=npdt == np.float32), (npdt, val, q, it)
        assert "quantile_select[rows=%d, valid=%d, rounds=1," % (n, n) in pl.last_plan(), pl.last_plan()
    # two distinct values that differ only in the lowest byte: the select ends at shift 0, through one more round than the constant column
    two = np.where(rng.random(n) < 0.5, np.int64(0x0123456789ABCD01), np.int64(0x0123456789ABCD02))
    s = pl.Series("t", two)
    for q, it in ALL:
        assert Q.accept(s.quantile(q, it), two, q, it), (q, it)
    assert s.quantile(0.0) == float(0x0123456789ABCD01) and s.quantile(1.0) == float(0x0123456789ABCD02)
    s.median()
    assert "rounds=2," in pl.last_plan(), pl.last_plan()
    # all eight digits differ: eight rounds
    wide = rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64)
    pl.Series("w", wide).median()
    assert "rounds=8," in pl.last_plan(), pl.last_plan()
    # ranks lo and hi in different top-digit buckets: the code at hi comes from the min pass
    s = pl.Series("pm", np.array([-1.0, 1.0]))
    assert s.median() == 0.0 and "next=min_pass" in pl.last_plan(), pl.last_plan()
    assert s.quantile(0.5, "lower") == -1.0 and "next=none" in pl.last_plan()
    assert s.quantile(0.5, "higher") == 1.0 and s.quantile(0.5, "nearest") == 1.0 and s.quantile(0.5, "midpoint") == 0.0 and s.quantile(0.25, "linear") == -0.5
    s = pl.Series("same", np.array([3.0, 5.0, 5.0, 5.0, 9.0]))
    assert s.quantile(0.4, "linear") == 5.0 and "next=same" in pl.last_plan(), pl.last_plan()      # pos 1.6: ranks 1 and 2 hold the same code
    # NaN is an ordinary, largest element; the infinities rank at the ends
    y = rng.normal(size=1001)
    y[[3, 500]] = np.nan; y[7] = np.inf; y[9] = -np.inf
    s = pl.Series("y", y)
    for q, it in ALL:
        assert Q.accept(s.quantile(q, it), y, q, it), (q, it, s.quantile(q, it))
    assert math.isnan(s.quantile(1.0)) and s.quantile(0.0) == -np.inf and math.isfinite(s.median())
    assert math.isnan(pl.Series("nn", np.array([np.nan, np.nan])).median())
    m = np.ones(len(y), bool); m[[3, 500]] = False                    # ... unless those rows are null
    assert pl.Series("y", y, validity=m).quantile(1.0) == np.inf
    yf = y.astype(np.float32)
    for q, it in ALL:
        assert Q.accept(pl.Series("yf", yf).quantile(q, it), yf, q, it, f32=True), (q, it)
    # -0.0 with +0.0: one value
    z = np.array([-0.0, 0.0, -0.0, 0.0, 1.0])
    for q, it in ALL:
        assert Q.accept(pl.Series("z", z).quantile(q, it), z, q, it), (q, it)
    assert pl.Series("z", z[:4]).median() == 0.0
    # the same column twice: the same bits (the select's atomics are integer counts, AND, OR and MIN)
    for s2 in (s, pl.Series("x", y, validity=rng.random(len(y)) < 0.5), pl.Series("i", rng.integers(-9, 9, 100_003).astype(np.int8))):
        for q, it in ((0.5, "linear"), (1 / 3, "midpoint"), (0.999, "nearest")):
            assert bits(s2.quantile(q, it)) == bits(s2.quantile(q, it))


def test_refusals_c_entry_points_and_the_plugin_symbol(pl):
    F = pl._ffi
    rng = np.random.default_rng(72)
    x = rng.normal(size=1000)
    s = pl.Series("x", x)
    v, dt, ok = F.Scalar(), C.c_int32(), C.c_int32()
    for q, it in ALL:
        F.check(F.lib().plx_reduce_quantile(s._h, q, F.QUANTILE_INTERPOLATIONS[it], C.byref(v), C.byref(dt), C.byref(ok)))
        assert ok.value == 1 and dt.value == F.F64 and Q.accept(v.f64, x, q, it), (q, it)
    sf, se = pl.Series("f", x.astype(np.float32)), pl.Series("e", x[:3], validity=np.zeros(3, bool))
    F.check(F.lib().plx_reduce_quantile(sf._h, 0.5, F.QUANTILE_LINEAR, C.byref(v), C.byref(dt), C.byref(ok)))
    assert dt.value == F.F32 and Q.accept(float(np.float32(v.f32)), x.astype(np.float32), 0.5, "linear", f32=True)
    F.check(F.lib().plx_reduce_quantile(se._h, 0.5, F.QUANTILE_LINEAR, C.byref(v), C.byref(dt), C.byref(ok)))
    assert ok.value == 0
    assert F.lib().plx_reduce(F.AGG_QUANTILE, s._h, C.byref(v), C.byref(dt), C.byref(ok)) == 1 and "plx_reduce_quantile" in F.lib().plx_last_error().decode()
    for bad in (float("nan"), -1e-9, 1.0 + 1e-9):
        assert F.lib().plx_reduce_quantile(s._h, bad, 0, C.byref(v), C.byref(dt), C.byref(ok)) == 1 and "[0, 1]" in F.lib().plx_last_error().decode()
    assert F.lib().plx_reduce_quantile(s._h, 0.5, 5, C.byref(v), C.byref(dt), C.byref(ok)) == 1
    b = pl.Series("b", x > 0)
    assert F.lib().plx_reduce_quantile(b._h, 0.5, 0, C.byref(v), C.byref(dt), C.byref(ok)) == F.ERR_UNSUPPORTED and "bool" in F.lib().plx_last_error().decode().lower()
    with pytest.raises(TypeError, match="Boolean"):
        b.median()
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        s.quantile(1.5)
    with pytest.raises(ValueError, match="interpolation"):
        s.quantile(0.5, "equiprobable")
    # ... and so does a plan (the mirror's lowering; plx_reduce_quantile above is the engine's own refusal)
    with pytest.raises(TypeError, match="Boolean"):
        pl.DataFrame([b]).lazy().select(pl.col("b").median()).collect()
    # plx_groupby_agg_params: q / interpolation per aggregate; NULL arrays = the median; plx_groupby_agg_ddof refuses the kind
    k = rng.integers(0, 4, 1000).astype(np.int16)
    ks = pl.Series("k", k)
    keys, vals = (C.c_uint64 * 1)(ks._h), (C.c_uint64 * 4)(s._h, s._h, s._h, s._h)
    aggs = (C.c_int32 * 4)(F.AGG_QUANTILE, F.AGG_QUANTILE, F.AGG_STD, F.AGG_MEAN)
    qs, its, dd = (C.c_double * 4)(0.25, 0.999, 0.0, 0.0), (C.c_int32 * 4)(F.QUANTILE_LOWER, F.QUANTILE_LINEAR, 0, 0), (C.c_int32 * 4)(1, 1, 0, 1)
    for with_params in (False, True):
        ok_, oa = (C.c_uint64 * 1)(), (C.c_uint64 * 4)()
        F.check(F.lib().plx_groupby_agg_params(keys, 1, vals, aggs, 4, 0, dd if with_params else None, qs if with_params else None, its if with_params else None, ok_, oa))
        assert "quantile[sorted segments: " in pl.last_plan() and "groups=4, sources=1, outputs=2]" in pl.last_plan(), pl.last_plan()
        gk = pl.Series._from_handle("k", ok_[0], pl.Int16).to_numpy()
        cols = [pl.Series._from_handle("a", h, pl.Float64).to_numpy() for h in oa]
        assert sorted(gk.tolist()) == [0, 1, 2, 3]
        for i, kv in enumerate(gk):
            xs = x[k == kv]
            assert Q.accept(float(cols[0][i]), xs, 0.25 if with_params else 0.5, "lower" if with_params else "linear")
            assert Q.accept(float(cols[1][i]), xs, 0.999 if with_params else 0.5, "linear")
            assert abs(cols[2][i] - np.std(xs, ddof=0 if with_params else 1)) < 1e-12 and abs(cols[3][i] - xs.mean()) < 1e-12
    ok_, oa = (C.c_uint64 * 1)(), (C.c_uint64 * 4)()
    assert F.lib().plx_groupby_agg_ddof(keys, 1, vals, aggs, 4, 0, dd, ok_, oa) == 1 and "plx_groupby_agg_params" in F.lib().plx_last_error().decode()
    # the plugin symbol: a chunked input with nulls, Float32 stays Float32, all null -> null, Boolean refused
    valid = rng.random(len(x)) < 0.8
    arr = pa.array(x, mask=~valid)
    res, inp = P.call("plx_median", [pa.chunked_array([arr.slice(0, 400), arr.slice(400)])], None, names=["x"])
    assert res is not None, P.last_error()
    assert inp.released == 1 and len(res) == 1 and res.type == pa.float64() and inp.out_name == b"x" and Q.accept(res[0].as_py(), x[valid], 0.5, "linear")
    res, _ = P.call("plx_median", [pa.array(np.array([1.5, 2.5], np.float32))])
    assert res is not None and res.type == pa.float32() and res[0].as_py() == 2.0
    res, _ = P.call("plx_median", [pa.array([None, None], pa.float64())])
    assert res is not None and res[0].as_py() is None
    res, inp = P.call("plx_median", [pa.array([True, False])])
    assert res is None and inp.released == 1 and "bool" in P.last_error().lower()


# ---- grouped ---------------------------------------------------------------------------------------------------------------------------------
def canon(v, ok):
    """a key part as the sort's equality sees it: null == null, NaN == NaN, -0 == +0"""
    if not ok:
        return None
    if isinstance(v, (float, np.floating)):
        return "nan" if math.isnan(v) else float(v) + 0.0
    return int(v)


def host_groups(keys, keep):
    """{key tuple: row indices} over the rows of `keep`, in first-occurrence order"""
    parts = [(v, np.ones(len(v), bool) if m is None else m) for v, m in keys]
    groups = {}
    for r in np.nonzero(keep)[0]:
        groups.setdefault(tuple(canon(v[r], m[r]) for v, m in parts), []).append(r)
    return {k: np.array(rows) for k, rows in groups.items()}


def check_frame(out, key_names, groups, sources, specs, what):
    """every output row of every quantile column against ref_quantile over its group's valid values; returns the key tuples in output order"""
    d = R.download(out)
    assert out.height == len(groups), (what, out.height, len(groups))
    kparts = [(d[k][0], np.ones(out.height, bool) if d[k][1] is None else d[k][1]) for k in key_names]
    seen = []
    for r in range(out.height):
        kt = tuple(canon(v[r], m[r]) for v, m in kparts)
        assert kt in groups and kt not in seen, (what, "unknown or repeated group", kt)
        seen.append(kt)
        rows = groups[kt]
        for name, (src, q, it) in specs.items():
            v, m = sources[src]
            xs = v[rows] if m is None else v[rows][m[rows]]
            gv, gm = d[name]
            got = None if (gm is not None and not gm[r]) else float(gv[r])
            assert Q.accept(got, xs, q, it, f32=v.dtype == np.float32), (what, kt, name, got, Q.ref_quantile(xs, q, it), len(xs))
    return seen


REASON = "median / quantile: an order statistic (sorted-segment route)"
SPECS3 = {"med": ("x", 0.5, "linear"), "q1": ("x", 0.25, "lower"), "q3": ("x", 0.75, "higher")}


def agg_list(pl, specs):
    return [pl.col(src).quantile(q, it).alias(name) for name, (src, q, it) in specs.items()]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 2048, 2049, 4097, 2 * 4096 + 5])
def test_group_by_sizes(pl, n):
    """2048 / 2049 straddle the one-workgroup rank sort and the radix sort, 64 is the ballot word, 4096 the sort tile"""
    rng = np.random.default_rng(200 + n)
    x, xm = rng.normal(0.0, 100.0, n), rng.random(n) > 0.2
    keyings = {"one group": np.zeros(n, np.int32), "every row its own group": rng.permutation(n).astype(np.int32), "a few": rng.integers(-2, 3, n).astype(np.int32)}
    for kname, k in keyings.items():
        df = frame_of(pl, {"k": (k, None), "x": (x, xm)})
        out = df.lazy().group_by("k").agg(*agg_list(pl, SPECS3)).collect()
        plan = pl.last_plan()
        assert "quantile[sorted segments: " in plan and "sources=1, outputs=3]" in plan and REASON in plan, plan
        assert ("rank_sort[rows=%d," % n in plan) == (n <= 2048) and ("radix_sort[rows=%d," % n in plan) == (n > 2048), plan
        check_frame(out, ["k"], host_groups([(k, None)], np.ones(n, bool)), {"x": (x, xm)}, SPECS3, (n, kname))


def test_group_boundary_at_a_multiple_of_64(pl):
    """64 rows of key 0, 128 of key 1, 7 of key 2: in the sorted order the heads sit at rows 0, 64 and 192 -- bit 0 of three ballot words"""
    rng = np.random.default_rng(201)
    k = np.repeat(np.array([0, 1, 2], np.int16), [64, 128, 7])
    rng.shuffle(k)
    x = rng.normal(size=len(k))
    out = frame_of(pl, {"k": (k, None), "x": (x, None)}).lazy().group_by("k").agg(*agg_list(pl, SPECS3)).collect()
    check_frame(out, ["k"], host_groups([(k, None)], np.ones(len(k), bool)), {"x": (x, None)}, SPECS3, "boundary")


def test_groups_that_decide_between_null_and_a_value_and_the_sorts_equality(pl):
    rng = np.random.default_rng(202)
    n = 400
    # a Float64 key: 0 .. 4, a NaN group, -0.0 and +0.0 in one group, a null-key group
    kf = rng.integers(0, 5, n).astype(np.float64)
    kf[rng.random(n) < 0.1] = np.nan
    kf[(kf == 0) & (rng.random(n) < 0.5)] = -0.0
    kf[:4] = [-0.0, 0.0, np.nan, 1.0]
    km = rng.random(n) > 0.1
    km[:4] = True
    x, xm = rng.normal(size=n), rng.random(n) > 0.3
    xm[kf == 2.0] = False                                           # every value of group 2.0 is null: a null, and the row is present
    g3, g4 = np.nonzero((kf == 3.0) & km)[0], np.nonzero((kf == 4.0) & km)[0]
    xm[g3] = False; xm[g3[0]] = True                                 # exactly one valid value
    xm[g4] = False; xm[g4[:2]] = True                                # exactly two
    f = rng.normal(size=n).astype(np.float32)
    big = rng.integers((1 << 53) + 1, (1 << 62), n, dtype=np.int64) | 1      # odd integers above 2^53: no f64 holds them
    cols = {"k": (kf, km), "x": (x, xm), "f": (f, xm), "big": (big, None)}
    specs = dict(SPECS3, fmed=("f", 0.5, "linear"), fq=("f", 1 / 3, "midpoint"), bmed=("big", 0.5, "linear"), blo=("big", 0.999, "lower"), bhi=("big", 0.0, "higher"))
    df = frame_of(pl, cols)
    out = df.lazy().group_by("k").agg(*agg_list(pl, specs)).collect()
    assert "sources=3, outputs=8]" in pl.last_plan(), pl.last_plan()
    assert out["fmed"].dtype == pl.Float32 and out["bmed"].dtype == pl.Float64 and out["med"].dtype == pl.Float64
    groups = host_groups([(kf, km)], np.ones(n, bool))
    assert set(groups) == {(None,), ("nan",), (0.0,), (1.0,), (2.0,), (3.0,), (4.0,)}
    check_frame(out, ["k"], groups, cols, specs, "float key")
    d = out.to_dict()
    row = {canon(kv, kv is not None): i for i, kv in enumerate(d["k"])}
    assert d["med"][row[2.0]] is None and d["q1"][row[2.0]] is None and d["fmed"][row[2.0]] is None and d["bmed"][row[2.0]] is not None
    assert d["med"][row[3.0]] == x[g3[0]] and d["q3"][row[3.0]] == x[g3[0]]
    assert d["q1"][row[4.0]] == min(x[g4[:2]]) and d["q3"][row[4.0]] == max(x[g4[:2]]) and min(x[g4[:2]]) < d["med"][row[4.0]] < max(x[g4[:2]])
    # a two-column key with a null in one part: (1, null) and (1, 7) are different groups, (null, 7) and (null, null) too
    a = rng.integers(0, 3, n).astype(np.int64)
    b = rng.integers(6, 8, n).astype(np.int8)
    am, bm = rng.random(n) > 0.2, rng.random(n) > 0.2
    cols2 = {"a": (a, am), "b": (b, bm), "x": (x, xm)}
    out = frame_of(pl, cols2).lazy().group_by("a", "b").agg(*agg_list(pl, SPECS3)).collect()
    groups = host_groups([(a, am), (b, bm)], np.ones(n, bool))
    assert len(groups) == 12 and (None, None) in groups
    check_frame(out, ["a", "b"], groups, cols2, SPECS3, "two-column key")


def test_mixed_lists_share_one_sort_per_source_and_keep_the_group_order(pl):
    rng = np.random.default_rng(203)
    n = 3000
    k = R.sparse(rng.integers(0, 37, n))
    x, xm = rng.normal(5.0, 2.0, n), rng.random(n) > 0.1
    y = rng.integers(-50, 50, n).astype(np.int32)
    cols = {"k": (k, None), "x": (x, xm), "y": (y, None)}
    df = frame_of(pl, cols)
    c = pl.col
    groups = host_groups([(k, None)], np.ones(n, bool))
    for two in (False, True):
        specs = dict(SPECS3)
        aggs = agg_list(pl, specs) + [c("x").std().alias("sd"), c("x").sum().alias("s"), pl.len().alias("n")]
        if two:
            more = {"ymed": ("y", 0.5, "linear"), "ynear": ("y", 0.5, "nearest")}
            aggs += agg_list(pl, more) + [c("y").max().alias("ymax")]
            specs.update(more)
        for mo in (False, True):
            out = df.lazy().group_by("k", maintain_order=mo).agg(*aggs).collect()
            plan = pl.last_plan()
            assert ("sources=2, outputs=5]" if two else "sources=1, outputs=3]") in plan and plan.count("sort[rows=%d," % n) == (2 if two else 1), plan
            order = check_frame(out, ["k"], groups, cols, specs, ("mixed", two, mo))
            d = out.to_dict()
            for r, kt in enumerate(order):
                rows = groups[kt]
                xs = x[rows][xm[rows]]
                assert d["n"][r] == len(rows) and abs(d["s"][r] - xs.sum()) <= 1e-9 * np.abs(xs).sum() and abs(d["sd"][r] - np.std(xs, ddof=1)) <= 1e-9
                if two:
                    assert d["ymax"][r] == y[rows].max()
            if mo:
                # first-occurrence order, exactly as the same query without the quantiles
                plain = df.lazy().group_by("k", maintain_order=True).agg(c("x").sum().alias("s")).collect().to_dict()
                assert d["k"] == plain["k"] and [kt[0] for kt in order] == list(dict.fromkeys(k.tolist()))      # (the f64 sums themselves are atomics: last-bit differences between two runs)


def test_filter_in_front_and_an_expression_source(pl):
    rng = np.random.default_rng(204)
    n = 2500
    k = rng.integers(0, 9, n).astype(np.int16)
    a, b = rng.integers(-300, 300, n).astype(np.int64), rng.integers(-20, 20, n).astype(np.int64)
    bm = rng.random(n) > 0.1
    x = rng.normal(size=n)
    cols = {"k": (k, None), "a": (a, None), "b": (b, bm), "x": (x, None), "ab": (a * b, bm)}
    df = frame_of(pl, {kk: cols[kk] for kk in ("k", "a", "b", "x")})
    c = pl.col
    keep = (x > -0.5) & (k != 4)                                    # the filter empties group 4
    out = df.lazy().filter((c("x") > -0.5) & (c("k") != 4)).group_by("k").agg((c("a") * c("b")).median().alias("abmed"), c("x").quantile(0.999, "linear").alias("xq"), c("a").min().alias("amin")).collect()
    assert "quantile[sorted segments: " in pl.last_plan() and "sources=2, outputs=2]" in pl.last_plan(), pl.last_plan()
    groups = host_groups([(k, None)], keep)
    assert (4,) not in groups and len(groups) == 8
    order = check_frame(out, ["k"], groups, cols, {"abmed": ("ab", 0.5, "linear"), "xq": ("x", 0.999, "linear")}, "filtered")
    assert out.to_dict()["amin"] == [int(a[groups[kt]].min()) for kt in order]
    # whole-column select through the plan: per node, with and without the filter
    for lf, kp in ((df.lazy(), np.ones(n, bool)), (df.lazy().filter(c("x") > -0.5), x > -0.5)):
        out = lf.select((c("a") * c("b")).median().alias("abmed"), c("x").quantile(0.25, "midpoint").alias("xq"), c("x").mean().alias("m")).collect()
        plan = pl.last_plan()
        assert "quantile_select[" in plan and REASON in plan, plan
        g = {kk: v[0] for kk, v in out.to_dict().items()}
        assert Q.accept(g["abmed"], (a * b)[kp & bm], 0.5, "linear") and Q.accept(g["xq"], x[kp], 0.25, "midpoint") and abs(g["m"] - x[kp].mean()) < 1e-12


ROUTE_WORD = {"lds": "lds_table(", "dense": "dense_hbm_table(", "hash": "]+hash_hbm_table("}


@pytest.mark.parametrize("route", ["lds", "dense", "hash"])
def test_group_frame_routes(pl, monkeypatch, route):
    """the group frame (keys, group order, the cell aggregates) from the LDS-table, dense-HBM and hash-HBM routes: the group counts and key ranges decide the route"""
    monkeypatch.setenv("PLX_LEARN_DENSE_RANGE", "0")
    rng = np.random.default_rng(205 + list(ROUTE_WORD).index(route))
    n = 6000
    if route == "lds":
        ids = rng.integers(0, 4, n)
        k = (ids - 1).astype(np.int16)
    elif route == "dense":
        ids = rng.integers(0, 40, n) * 1249
        ids[0], ids[1] = 0, 49_999
        k = ids.astype(np.uint16)
    else:
        ids = rng.integers(0, 40, n)
        k = R.sparse(ids)
    km = rng.random(n) > 0.05
    x, xm = rng.normal(20.0, 2.0, n), rng.random(n) > 0.15
    cols = {"k": (k, km), "x": (x, xm)}
    out = frame_of(pl, cols).lazy().group_by("k").agg(*agg_list(pl, SPECS3), pl.col("x").mean().alias("m"), pl.len().alias("n")).collect(**({"no_partition": True} if route == "hash" else {}))
    plan = pl.last_plan()
    assert ROUTE_WORD[route] in plan and "quantile[sorted segments: " in plan, plan
    groups = host_groups([(k, km)], np.ones(n, bool))
    order = check_frame(out, ["k"], groups, cols, SPECS3, route)
    d = out.to_dict()
    for r, kt in enumerate(order):
        rows = groups[kt]
        assert d["n"][r] == len(rows) and abs(d["m"][r] - x[rows][xm[rows]].mean()) < 1e-9


def test_join_then_group_by_with_a_median(pl):
    rng = np.random.default_rng(206)
    nb, n = 50, 3000
    bk = R.sparse(rng.permutation(1000)[:nb])
    g = rng.integers(0, 6, nb).astype(np.int16)
    pk = bk[rng.integers(0, nb, n)]
    pk[rng.random(n) < 0.1] = 12345                                 # probe rows without a partner
    w = rng.normal(size=n)
    build = frame_of(pl, {"k": (bk, None), "g": (g, None)})
    probe = frame_of(pl, {"k": (pk, None), "w": (w, None)})
    out = probe.lazy().join(build.lazy(), on="k").group_by("g").agg(pl.col("w").median().alias("med"), pl.col("w").quantile(0.25, "lower").alias("q1"), pl.len().alias("n")).collect()
    assert "quantile[sorted segments: " in pl.last_plan(), pl.last_plan()
    g_of = dict(zip(bk.tolist(), g.tolist()))
    hit = np.array([kk in g_of for kk in pk.tolist()])
    jg = np.array([g_of.get(kk, -1) for kk in pk.tolist()], np.int16)
    groups = host_groups([(jg, None)], hit)
    order = check_frame(out, ["g"], groups, {"w": (w, None)}, {"med": ("w", 0.5, "linear"), "q1": ("w", 0.25, "lower")}, "join")
    assert out.to_dict()["n"] == [len(groups[kt]) for kt in order]
