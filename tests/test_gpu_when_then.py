"""when / then / otherwise on the GPU: the per-node select kernel (plx_if_then_else, with_columns) at every word and tile edge, width and operand form;
fused programs with OP_SELECT against the per-node evaluator and numpy; the run-time compiled kernel, the generic interpreter and the per-node kernels on one
query; Q12 / Q14-shaped joins; the expression plugin.  The reference is numpy throughout: np.where(predicate value & predicate validity, then, otherwise) for
values and for validity.  The lowering and the programs themselves are pinned on the CPU (tests/test_when_then_cpu.py)."""
import ctypes as C
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1000, 100_003]      # the 64-row word, the 4-word (256-row) fast path, an odd tail, more than one block
DTYPES = ["Int8", "Int16", "Int32", "Int64", "Float32", "Float64", "Boolean"]
FORMS = ["column", "scalar", "null"]


def values_of(rng, dtype, n):
    if dtype == "Boolean":
        return rng.random(n) < 0.5
    if dtype.startswith("Float"):
        return rng.normal(size=n).astype(np.float32 if dtype == "Float32" else np.float64)
    info = np.iinfo(getattr(np, dtype.lower()))
    return rng.integers(info.min, info.max, n, dtype=getattr(np, dtype.lower()), endpoint=True)


def where(pred, then, other):
    (pv, pm), (av, am), (bv, bm) = pred, then, other
    t = pv & pm
    return np.where(t, av, bv), np.where(t, am, bm)


def check_column(s, want_v, want_m, what):
    got_v, got_m = s._download()
    assert len(got_v) == len(want_v), what
    assert s.null_count() == int((~want_m).sum()), what
    if want_m.all():
        assert got_m is None, what
    else:
        assert np.array_equal(got_m, want_m), what
    assert np.array_equal(got_v[want_m], want_v[want_m]), what


@pytest.mark.parametrize("dtype", DTYPES)
def test_select_kernel_through_the_c_entry_point(pl, dtype):
    F = pl._ffi
    rng = np.random.default_rng(DTYPES.index(dtype))
    dt = getattr(pl, dtype)
    for n in SIZES:
        mv, mm = rng.random(n) < 0.5, rng.random(n) < 0.8
        sides = {}
        for side in "ab":
            v, m = values_of(rng, dtype, max(n, 1)), rng.random(max(n, 1)) < 0.7
            sides[side] = {"column": (pl.Series(side, v[:n], dt, validity=m[:n]), v[:n], m[:n]),
                           "plain": (pl.Series(side, v[:n], dt), v[:n], np.ones(n, bool)),
                           "scalar": (pl.Series(side, v[:1], dt), np.full(n, v[0]), np.ones(n, bool)),
                           "null": (pl.Series(side, v[:1], dt, validity=np.zeros(1, bool)), np.full(n, v[0]), np.zeros(n, bool))}
        for mask_valid in (True, False):
            mask = pl.Series("m", mv, pl.Boolean, validity=mm) if mask_valid else pl.Series("m", mv, pl.Boolean)
            pred = (mv, mm if mask_valid else np.ones(n, bool))
            for fa in FORMS + ["plain"]:
                for fb in FORMS + ["plain"]:
                    (sa, av, am), (sb, bv, bm) = sides["a"][fa], sides["b"][fb]
                    h = C.c_uint64()
                    F.check(F.lib().plx_if_then_else(mask._h, sa._h, sb._h, C.byref(h)))
                    out = pl.Series._from_handle("r", h.value, dt)
                    want_v, want_m = where(pred, (av, am), (bv, bm))
                    check_column(out, want_v, want_m, (dtype, n, mask_valid, fa, fb))
                    if want_m.all() and fa in ("plain", "scalar") and fb in ("plain", "scalar"):
                        assert out.device_ptrs()[1] == 0, (dtype, n, fa, fb)          # a result that cannot be null carries no bitmap


def test_select_kernel_checks_its_operands(pl):
    F = pl._ffi
    m, a, b = pl.Series("m", np.array([True, False, True])), pl.Series("a", np.arange(3, dtype=np.int64)), pl.Series("b", np.arange(3, dtype=np.int32))
    h = C.c_uint64()
    with pytest.raises(pl.PlxError, match="dtype"):
        F.check(F.lib().plx_if_then_else(m._h, a._h, b._h, C.byref(h)))
    with pytest.raises(pl.PlxError, match="Boolean"):
        F.check(F.lib().plx_if_then_else(a._h, a._h, a._h, C.byref(h)))
    short = pl.Series("c", np.arange(2, dtype=np.int64))
    with pytest.raises(pl.PlxError, match="length"):
        F.check(F.lib().plx_if_then_else(m._h, a._h, short._h, C.byref(h)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_with_columns_runs_the_select_kernel(pl, dtype):
    rng = np.random.default_rng(100 + DTYPES.index(dtype))
    dt = getattr(pl, dtype)
    c = pl.col
    for n in SIZES:
        mv, mm = rng.random(n) < 0.5, rng.random(n) < 0.8
        av, am = values_of(rng, dtype, n), rng.random(n) < 0.7
        bv = values_of(rng, dtype, n)
        lit = values_of(rng, dtype, 1)[0]
        df = pl.DataFrame([pl.Series("m", mv, pl.Boolean, validity=mm), pl.Series("a", av, dt, validity=am), pl.Series("b", bv, dt)])
        out = df.lazy().with_columns(pl.when(c("m")).then(c("a")).otherwise(c("b")).alias("cc"), pl.when(c("m")).then(c("a")).otherwise(pl.lit(lit.item(), dt)).alias("cs"),
                                     pl.when(c("m")).then(c("a")).alias("cn"), pl.when(c("m")).then(None).otherwise(c("b")).alias("nc"),
                                     pl.when(c("m").is_not_null()).then(c("b")).otherwise(pl.lit(lit.item(), dt)).alias("never_null")).collect()
        ones, zeros = np.ones(n, bool), np.zeros(n, bool)
        assert out.schema["cc"] == dt and out.schema["cn"] == dt and out.schema["nc"] == dt
        check_column(out["cc"], *where((mv, mm), (av, am), (bv, ones)), (dtype, n, "cc"))
        check_column(out["cs"], *where((mv, mm), (av, am), (np.full(n, lit), ones)), (dtype, n, "cs"))
        check_column(out["cn"], *where((mv, mm), (av, am), (av, zeros)), (dtype, n, "cn"))
        check_column(out["nc"], *where((mv, mm), (bv, zeros), (bv, ones)), (dtype, n, "nc"))
        check_column(out["never_null"], *where((mm, ones), (bv, ones), (np.full(n, lit), ones)), (dtype, n, "never_null"))
        assert out["never_null"].device_ptrs()[1] == 0


# ---- fused against per node --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(2028)
    n = 300_000
    ones = np.ones(n, bool)
    cols = {"a": (rng.integers(-20, 20, n).astype(np.int64), rng.random(n) < 0.8), "b": (rng.integers(-50, 50, n).astype(np.int64), ones),
            "x": (rng.normal(size=n), rng.random(n) < 0.7), "y": (rng.normal(size=n), ones), "k": (rng.integers(0, 5, n).astype(np.int64), ones),
            "flag": (rng.random(n) < 0.5, rng.random(n) < 0.75)}
    return n, cols


@pytest.fixture(scope="module")
def frame(pl, table):
    _, cols = table
    return pl.DataFrame([pl.Series(name, v, validity=None if m.all() else m) for name, (v, m) in cols.items()])


def route(plan):
    """The plan description without the sizes of its program and of its result (a conditional key has its otherwise value as one more group): what is left names the
    route -- pipeline, kernel kind, sink and the sink's capacity."""
    return re.sub(r"\b(inputs|ops|aggs|groups)=\d+", "", plan)


def rows_by_key(out, keys):
    d = out.to_dict()
    return {tuple(d[k][i] for k in keys): {c: d[c][i] for c in d if c not in keys} for i in range(out.height)}


def collect_both(pl, q, plain):
    """q fused and per node; the fused run must take the route of `plain` (q with every ternary replaced by its then operand)."""
    plain.collect()
    want_route = route(pl.last_plan())
    fused = q.collect()
    plan = pl.last_plan()
    assert "Fused" in plan and route(plan) == want_route, (plan, want_route)
    return fused, q.collect(no_fusion=True)


def test_filter_and_whole_frame_aggregates(pl, table, frame):
    n, cols = table
    c = pl.col
    def q(t):
        src = frame.lazy().filter(c("b") > -40)
        return src.select(t(c("flag"), c("x") * c("y"), 0.0).sum().alias("s"), t(c("a") > 0, c("a"), c("b")).sum().alias("si"), t(c("flag"), c("x"), None).count().alias("cnt"),
                          t(c("a") > 0, c("a"), 7).min().alias("mn"), pl.len().alias("n"))
    tern = lambda p, a, b: pl.when(p).then(a).otherwise(b) if b is not None else pl.when(p).then(a)
    (a, am), (b, _), (x, xm), (y, _), flag = (cols[k] for k in ("a", "b", "x", "y", "flag"))
    ones = np.ones(n, bool)
    keep = b > -40
    sv, sm = where(flag, (x * y, xm), (np.zeros(n), ones))
    iv, im = where((a > 0, am), (a, am), (b, ones))
    cm = where(flag, (x, xm), (x, ~ones))[1]
    mv, mm = where((a > 0, am), (a, am), (np.full(n, 7), ones))
    for out in collect_both(pl, q(tern), q(lambda p, a, b: a)):
        d = out.to_dict()
        assert np.isclose(d["s"][0], sv[keep & sm].sum(), rtol=1e-9)
        assert d["si"][0] == int(iv[keep & im].sum()) and d["cnt"][0] == int((keep & cm).sum()) and d["mn"][0] == int(mv[keep & mm].min()) and d["n"][0] == int(keep.sum())


def test_group_by_aggregates_of_a_ternary(pl, table, frame):
    n, cols = table
    c = pl.col
    def q(t):
        e = t(c("flag"), c("x"), c("y"))
        return frame.lazy().group_by("k").agg(e.sum().alias("s"), e.mean().alias("m"), e.min().alias("mn"), e.count().alias("c"), t(c("a") > 0, c("a"), c("b")).sum().alias("si"))
    (a, am), (b, _), (x, xm), (y, _), (k, _), flag = (cols[nm] for nm in ("a", "b", "x", "y", "k", "flag"))
    ones = np.ones(n, bool)
    ev, em = where(flag, (x, xm), (y, ones))
    iv, im = where((a > 0, am), (a, am), (b, ones))
    for out in collect_both(pl, q(lambda p, a, b: pl.when(p).then(a).otherwise(b)), q(lambda p, a, b: a)):
        got = rows_by_key(out, ["k"])
        assert sorted(got) == [(i,) for i in range(5)]
        for i in range(5):
            g, rows = got[(i,)], (k == i) & em
            assert np.isclose(g["s"], ev[rows].sum(), rtol=1e-9) and np.isclose(g["m"], ev[rows].mean(), rtol=1e-9) and g["mn"] == ev[rows].min()
            assert g["c"] == int(rows.sum()) and g["si"] == int(iv[(k == i) & im].sum())


def test_ternary_group_key_and_ternary_in_the_filter(pl, table, frame):
    n, cols = table
    c = pl.col
    (a, am), (b, _), (x, xm), (k, _), flag = (cols[nm] for nm in ("a", "b", "x", "k", "flag"))
    ones = np.ones(n, bool)
    # the key: a computed expression on either side of the comparison (a plain column would bit-pack from its statistics, a computed key never does)
    def q(t):
        return frame.lazy().group_by(t(c("a") > 0, c("k") * 2, -1).alias("g")).agg(c("x").sum().alias("s"), pl.len().alias("n"))
    gv, gm = where((a > 0, am), (k * 2, ones), (np.full(n, -1), ones))
    assert gm.all()
    for out in collect_both(pl, q(lambda p, a, b: pl.when(p).then(a).otherwise(b)), q(lambda p, a, b: a)):
        got = rows_by_key(out, ["g"])
        assert sorted(got) == sorted((int(v),) for v in np.unique(gv))
        for (g,), row in got.items():
            assert row["n"] == int((gv == g).sum()) and np.isclose(row["s"], x[(gv == g) & xm].sum(), rtol=1e-9)
    # the filter: rows whose chosen side is null drop, like any null predicate
    def f(t):
        return frame.lazy().filter(t(c("flag"), c("a"), c("b")) > 3).select(c("b").sum().alias("sb"), pl.len().alias("n"))
    fv, fm = where(flag, (a, am), (b, ones))
    keep = fm & (fv > 3)
    for out in collect_both(pl, f(lambda p, a, b: pl.when(p).then(a).otherwise(b)), f(lambda p, a, b: a)):
        d = out.to_dict()
        assert d["n"][0] == int(keep.sum()) and d["sb"][0] == int(b[keep].sum())


def test_compiled_interpreted_and_per_node_agree_bit_for_bit(pl, table, frame):
    """One program without an ahead-of-time kernel: the run-time compiled kernel, the generic interpreter (the JIT switched off) and the per-node kernels."""
    F = pl._ffi
    c = pl.col
    e = pl.when(c("flag")).then(c("a")).otherwise(c("b"))
    q = (frame.lazy().filter(pl.when(c("a") > 0).then(c("b")).otherwise(c("a") * 3) > -30).group_by("k")
         .agg(e.sum().alias("s"), e.min().alias("mn"), e.max().alias("mx"), pl.when(c("flag")).then(c("a")).count().alias("c"), pl.when(c("b") > 0).then(1).otherwise(0).sum().alias("h"), pl.len().alias("n")))
    res = {}
    try:
        for mode, min_rows in (("jit", 0), ("generic", -1)):
            F.jit_set_min_rows(min_rows)
            before = F.jit_stats()[0]
            res[mode] = rows_by_key(q.collect(), ["k"])
            assert f"fused_scan[{mode}]" in pl.last_plan(), pl.last_plan()
            assert (F.jit_stats()[0] > before) == (mode == "jit")
    finally:
        F.jit_set_min_rows(1 << 22)
    res["per_node"] = rows_by_key(q.collect(no_fusion=True), ["k"])
    assert res["jit"] == res["generic"] == res["per_node"] and len(res["jit"]) == 5
    n, cols = table
    (a, am), (b, _), (k, _), flag = (cols[nm] for nm in ("a", "b", "k", "flag"))
    ones = np.ones(n, bool)
    pv, pm = where((a > 0, am), (b, ones), (a * 3, am))
    keep = pm & (pv > -30)
    ev, em = where(flag, (a, am), (b, ones))
    for i in range(5):
        g, rows = res["jit"][(i,)], keep & (k == i)
        assert g == {"s": int(ev[rows & em].sum()), "mn": int(ev[rows & em].min()), "mx": int(ev[rows & em].max()), "c": int((rows & flag[0] & flag[1] & am).sum()),
                     "h": int((rows & (b > 0)).sum()), "n": int(rows.sum())}


# ---- Q12 / Q14 ---------------------------------------------------------------------------------------------------------------------
def test_q12_and_q14_sums(pl):
    from polars_amd import queries as Q
    rng = np.random.default_rng(1214)
    n, n_orders, n_parts = 1 << 18, 1 << 16, 20_000
    okey = rng.permutation(n_orders).astype(np.int64) * 4 + 1
    prio = rng.integers(0, 5, n_orders).astype(np.int64)
    pkey = rng.permutation(n_parts).astype(np.int64)
    ptype = rng.integers(0, 150, n_parts).astype(np.int64)
    l_okey = okey[rng.integers(0, n_orders, n)] + (rng.random(n) < 0.1)          # a tenth of the rows has no order
    l_pkey = rng.integers(0, n_parts + 2000, n).astype(np.int64)                  # some parts are unknown
    mode = rng.integers(0, 7, n).astype(np.int64)
    price, disc = rng.uniform(900, 100_000, n), rng.integers(0, 11, n) / 100.0
    li = pl.DataFrame({"l_orderkey": l_okey, "l_partkey": l_pkey, "l_shipmode": mode, "l_extendedprice": price, "l_discount": disc})
    orders = pl.DataFrame({"o_orderkey": okey, "o_orderpriority": prio})
    part = pl.DataFrame({"p_partkey": pkey, "p_type": ptype})
    prio_of = dict(zip(okey.tolist(), prio.tolist()))
    lp = np.array([prio_of.get(v, -1) for v in l_okey.tolist()])
    type_of = np.full(n_parts + 2000, -1)
    type_of[pkey] = ptype
    lt = type_of[l_pkey]
    rev = price * (1 - disc)
    for kw in ({}, {"no_fusion": True}):
        got = rows_by_key(Q.q12(li.lazy(), orders.lazy()).collect(**kw), ["l_shipmode"])
        assert sorted(got) == [(3,), (5,)]
        for m in (3, 5):
            rows = (mode == m) & (lp >= 0)
            assert got[(m,)] == {"high_line_count": int((rows & (lp <= 1)).sum()), "low_line_count": int((rows & (lp > 1)).sum())}, (kw, m)
        d = Q.q14_sums(li.lazy(), part.lazy()).collect(**kw).to_dict()
        assert np.isclose(d["promo_revenue"][0], rev[(lt >= 0) & (lt < 25)].sum(), rtol=1e-9) and np.isclose(d["revenue"][0], rev[lt >= 0].sum(), rtol=1e-9), kw


# ---- the expression plugin ---------------------------------------------------------------------------------------------------------
def test_when_then_otherwise_through_the_plugin_abi(pl):
    import pyarrow as pa

    from tests import plugin_abi as P
    rng = np.random.default_rng(3)
    n = 100_003
    mv, mm = rng.random(n) < 0.5, rng.random(n) < 0.9
    a, am = rng.integers(-1000, 1000, n).astype(np.int64), rng.random(n) < 0.8
    b = rng.integers(-1000, 1000, n).astype(np.int64)
    arr = lambda v, m=None: pa.array(v, mask=None if m is None else ~m)
    res, inp = P.call("plx_when_then_otherwise", [arr(mv, mm), arr(a, am), arr(b)], names=["m", "a", "b"])
    assert inp.released == 3 and inp.out_name == b"a" and res.type == pa.int64()
    want_v, want_m = where((mv, mm), (a, am), (b, np.ones(n, bool)))
    assert res.null_count == int((~want_m).sum())
    got = res.to_numpy(zero_copy_only=False)
    assert np.array_equal(got[want_m].astype(np.int64), want_v[want_m])
    res, _ = P.call("plx_when_then_otherwise", [arr(mv, mm), arr(a, am), arr(np.array([7], np.int64))])      # a length-1 series broadcasts
    want_v, want_m = where((mv, mm), (a, am), (np.full(n, 7), np.ones(n, bool)))
    assert res.null_count == int((~want_m).sum()) and np.array_equal(res.to_numpy(zero_copy_only=False)[want_m].astype(np.int64), want_v[want_m])
    res, inp = P.call("plx_when_then_otherwise", [arr(a), arr(a), arr(b)])
    assert res is None and inp.released == 3 and "Boolean" in P.last_error()
