"""join_asof on the device: every result row by row and every validity bit against tests/asof_ref.py, through the Python interface and through
plx_join_asof_indices for the raw index column; the default route (LDS samples) and PLX_ASOF_ROUTE=global."""
import ctypes as C
import datetime as dt

import numpy as np
import pytest

from polars_amd import _ffi as F
from tests import asof_ref as A

pytestmark = pytest.mark.gpu

T = F.ASOF_THREADS
HOWS = [(s, strict) for s in A.STRATEGIES for strict in (False, True)]
I64_MIN, I64_MAX, U64_MAX = -(1 << 63), (1 << 63) - 1, (1 << 64) - 1


# ---- helpers -----------------------------------------------------------------------------------------------------------------------------------------------------------
def indices(pl, lo, ro, lb=(), rb=(), *, strategy="backward", strict=False, tolerance=None, lov=None, rov=None, lbv=None, rbv=None, dtypes=None):
    """plx_join_asof_indices over host arrays -> (idx, valid or None, plan text); dtypes: logical dtypes of (on, by parts...)"""
    dtypes = dtypes or [None] * (1 + len(lb))
    keep = []
    def col(v, valid, d):
        s = pl.Series("k", v, d, validity=valid)
        keep.append(s)
        return s._h
    l_on, r_on = col(lo, lov, dtypes[0]), col(ro, rov, dtypes[0])
    nb = len(lb)
    lbh = (C.c_uint64 * max(nb, 1))(*[col(lb[j], None if lbv is None else lbv[j], dtypes[1 + j]) for j in range(nb)])
    rbh = (C.c_uint64 * max(nb, 1))(*[col(rb[j], None if rbv is None else rbv[j], dtypes[1 + j]) for j in range(nb)])
    tol = None
    if tolerance is not None:
        tol = F.Scalar()
        if np.asarray(lo).dtype.kind == "f":
            tol.f64 = float(tolerance)
        else:
            tol.u = int(tolerance)
    out = C.c_uint64()
    F.check(F.lib().plx_join_asof_indices(F.ASOF_STRATEGIES[strategy] | (F.ASOF_STRICT if strict else 0), lbh, rbh, nb, l_on, r_on, C.byref(tol) if tol is not None else None, C.byref(out)))
    plan = pl.last_plan()
    s = pl.Series._from_handle("idx", out.value)
    assert s.dtype == pl.UInt32 and len(s) == len(lo)
    idx, valid = s._download()
    return idx, valid, plan


def both_routes(monkeypatch):
    for route in ("", "global"):
        if route:
            monkeypatch.setenv("PLX_ASOF_ROUTE", route)
        else:
            monkeypatch.delenv("PLX_ASOF_ROUTE", raising=False)
        yield route


def right_with_runs(rng, m, stride):
    """m sorted Int64 values in steps of 0 (duplicates), 1, 2 and 4, with a run of duplicates across every few sample positions / stride ends"""
    steps = rng.choice(np.array([0, 0, 1, 2, 4]), m)
    for k in range(1, 6):
        p = k * stride * max(1, (m // stride) // 6)
        steps[max(p - 2, 1):p + 3] = 0
    return (np.cumsum(steps) - 3).astype(np.int64)


def left_at_the_edges(rng, r, stride, n):
    """n left values: below and above every right value, equal to the first and the last row, equal to a sample and one above / below it, inside the duplicate runs, random"""
    m = len(r)
    if m == 0:
        return rng.integers(-5, 5, n).astype(np.int64)
    pos = [0, m - 1] + [j * stride for j in (1, 2, 3, (m - 1) // stride - 1, (m - 1) // stride)] + [k * stride * max(1, (m // stride) // 6) + d for k in range(1, 6) for d in (-3, -2, 0, 2, 3)]
    vals = [int(r[0]) - 1, int(r[0]) - 7, int(r[-1]) + 1, int(r[-1]) + 9]
    for p in pos:
        if 0 <= p < m:
            vals += [int(r[p]) - 1, int(r[p]), int(r[p]) + 1]
    vals = np.array(vals, np.int64)
    rest = rng.integers(int(r[0]) - 2, int(r[-1]) + 3, max(n - len(vals), 0))
    return np.concatenate([vals, rest])[:n].astype(np.int64)


# ---- sizes ----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", A.STRATEGIES)
def test_sizes_around_the_sample_geometry_and_the_workgroup(pl, monkeypatch, strategy):
    S = F.asof_samples_for(1)
    rng = np.random.default_rng(200 + A.STRATEGIES.index(strategy))
    calls = 0
    for m in (0, 1, 2, S - 1, S, S + 1, 2 * S, 2 * S + 1, 2 * S + 78):          # 2 S + 78 rows: stride 3, the last stride holds one row
        stride = max(1, -(-m // S))
        r = right_with_runs(rng, m, stride)
        left = left_at_the_edges(rng, r, stride, T + 1)
        for strict in (False, True):
            want_idx, want_ok = A.join_asof(left, r, strategy=strategy, strict=strict)
            for n in (0, 1, 63, 64, 65, T - 1, T, T + 1):                       # the rows are searched independently: a prefix of the left side has a prefix of the result
                for route in both_routes(monkeypatch):
                    idx, valid, plan = indices(pl, left[:n], r, strategy=strategy, strict=strict)
                    A.check(idx, valid, want_idx[:n], want_ok[:n], (strategy, strict, m, n, route))
                    if n == 0 or m == 0:
                        assert plan == "asof[empty]", plan
                    else:
                        assert plan == f"asof[{strategy}{' strict' if strict else ''}, by=0, right=in order, rows={n} x {m}, samples={0 if route else S}]", plan
                    calls += 1
    assert calls == 9 * 2 * 8 * 2


def test_a_tolerance_at_every_size_and_a_shuffled_left_side(pl, monkeypatch):
    S = F.asof_samples_for(1)
    rng = np.random.default_rng(210)
    for m in (S + 1, 2 * S + 78):
        stride = -(-m // S)
        r = right_with_runs(rng, m, stride)
        left = rng.permutation(left_at_the_edges(rng, r, stride, T + 65))       # rows' results come in left order
        for strategy, strict in HOWS:
            for tolerance in (0, 1):
                want = A.join_asof(left, r, strategy=strategy, strict=strict, tolerance=tolerance)
                for route in both_routes(monkeypatch):
                    idx, valid, _ = indices(pl, left, r, strategy=strategy, strict=strict, tolerance=tolerance)
                    A.check(idx, valid, *want, (strategy, strict, m, tolerance, route))


# ---- by ----------------------------------------------------------------------------------------------------------------------------------------------------------------
def grouped_sides(rng, m, n, parts, nulls):
    """right: sorted by (by parts, on) with groups of 1 .. 40 rows at even ids (first / last rows land on samples and beside them); left: present groups, the absent odd
    ids between them and ids beyond the last; parts: 1 (Int32) or 3 (Int32, Float64 with NaN and both zeros, Boolean)"""
    sizes = []
    while sum(sizes) < m:
        sizes.append(int(rng.choice(np.array([1, 1, 2, 3, 7, 40]))))
    gid = np.repeat(np.arange(len(sizes)) * 2, sizes)[:m].astype(np.int32)
    on = np.concatenate([np.sort(rng.integers(0, 30, s)) for s in sizes])[:m].astype(np.int64)
    fvals = np.array([-0.0, 0.0, 1.5, np.nan])
    if parts == 3:
        # the float and Boolean parts are functions of the group id, so the right side stays in tuple order: (gid, f, b, on)
        rb = [gid, fvals[[0, 2, 3, 2]][(gid // 2) % 4], ((gid // 2) % 2).astype(bool)]
    else:
        rb = [gid]
    lg = rng.integers(-1, int(gid[-1]) + 4, n).astype(np.int32)
    lo = rng.integers(-2, 33, n).astype(np.int64)
    if parts == 3:
        lf = fvals[[1, 2, 3, 2]][(lg // 2) % 4]                                  # +0 on the left where the right holds -0: they are equal; NaN == NaN
        lb = [lg, lf, ((lg // 2) % 2).astype(bool)]
    else:
        lb = [lg]
    valid = dict(lov=None, rov=None, lbv=None, rbv=None)
    if nulls:
        valid = dict(lov=rng.random(n) < 0.9, rov=rng.random(m) < 0.9, lbv=[rng.random(n) < 0.9 for _ in lb], rbv=[rng.random(m) < 0.9 for _ in rb])
    return lo, on, lb, rb, valid


@pytest.mark.parametrize("parts", [1, 3])
def test_by_parts_groups_at_sample_edges_absent_groups_nan_zero_and_nulls(pl, monkeypatch, parts):
    S = F.asof_samples_for(parts + 1)
    rng = np.random.default_rng(220 + parts)
    for m, nulls in ((S + 3, False), (2 * S + 1, False), (2 * S + 1, True)):
        lo, ro, lb, rb, v = grouped_sides(rng, m, T + 70, parts, nulls)
        ref_valid = dict(left_on_valid=v["lov"], right_on_valid=v["rov"], left_by_valid=v["lbv"], right_by_valid=v["rbv"])
        dropped = 0
        if nulls:
            usable = v["rov"].copy()
            for b in v["rbv"]:
                usable &= b
            dropped = int((~usable).sum())
            assert dropped > 0
        for strategy, strict in HOWS:
            want = A.join_asof(lo, ro, lb, rb, strategy=strategy, strict=strict, **ref_valid)
            assert want[1].any() and not want[1].all()
            for route in both_routes(monkeypatch):
                idx, valid, plan = indices(pl, lo, ro, lb, rb, strategy=strategy, strict=strict, **v)
                A.check(idx, valid, *want, (parts, m, nulls, strategy, strict, route))
                assert f"by={parts}, right=in order" in plan and f"samples={0 if route else S}]" in plan and "sorted:" not in plan, plan
                assert (f"dropped null keys={dropped}, rows={len(lo)} x {m - dropped}," in plan) if nulls else ("dropped" not in plan), plan


def test_a_shuffled_right_side_is_sorted_once_and_gives_the_sorted_sides_result(pl, monkeypatch):
    rng = np.random.default_rng(230)
    S = F.asof_samples_for(2)
    lo, ro, lb, rb, _ = grouped_sides(rng, S + 500, T + 9, 1, False)
    shuffle = rng.permutation(len(ro))
    ro2, rb2 = ro[shuffle], [rb[0][shuffle]]
    rov = rng.random(len(ro)) < 0.95
    for strategy, strict in HOWS:
        for route in both_routes(monkeypatch):
            idx, valid, plan = indices(pl, lo, ro, lb, rb, strategy=strategy, strict=strict)
            assert "right=in order" in plan and "sort" not in plan.replace("asof[", ""), plan           # no sort ran
            idx2, valid2, plan2 = indices(pl, lo, ro2, lb, rb2, strategy=strategy, strict=strict)
            assert "right=sorted: " in plan2 and "in order" not in plan2, plan2
            want2 = A.join_asof(lo, ro2, lb, rb2, strategy=strategy, strict=strict)
            A.check(idx2, valid2, *want2, (strategy, strict, route, "shuffled"))
            # the same right rows are matched: among equal (by, on) the candidate order is the right row order, so compare the matched keys
            A.check(idx, valid, *A.join_asof(lo, ro, lb, rb, strategy=strategy, strict=strict), (strategy, strict, route))
            ok = np.ones(len(lo), bool) if valid is None else valid
            assert np.array_equal(ok, np.ones(len(lo), bool) if valid2 is None else valid2)
            assert np.array_equal(ro[idx[ok]], ro2[idx2[ok]]) and np.array_equal(rb[0][idx[ok]], rb2[0][idx2[ok]])
            # shuffled and with null keys: the compaction and the sort compose
            idx3, valid3, plan3 = indices(pl, lo, ro2, lb, rb2, strategy=strategy, strict=strict, rov=rov)
            assert "right=sorted: " in plan3 and f"dropped null keys={int((~rov).sum())}" in plan3, plan3
            A.check(idx3, valid3, *A.join_asof(lo, ro2, lb, rb2, strategy=strategy, strict=strict, right_on_valid=rov), (strategy, strict, route, "shuffled, nulls"))
    idx, valid, plan = indices(pl, lo, ro, lb, rb, rov=np.zeros(len(ro), bool))                                 # no usable right row at all
    assert valid is not None and not valid.any()


# ---- values ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_int64_at_its_ends_and_uint64_above_2_63_through_the_c_entry(pl, monkeypatch):
    for route in both_routes(monkeypatch):
        lo = np.array([I64_MIN, I64_MIN, -1, 0, I64_MAX], np.int64)
        ro = np.array([I64_MAX], np.int64)
        for tolerance, want_ok in ((U64_MAX, [1, 1, 1, 1, 1]), (U64_MAX - 1, [0, 0, 1, 1, 1]), (1 << 63, [0, 0, 1, 1, 1]), ((1 << 63) - 1, [0, 0, 0, 1, 1]), (None, [1, 1, 1, 1, 1])):
            for strategy in ("forward", "nearest"):
                idx, valid, _ = indices(pl, lo, ro, strategy=strategy, tolerance=tolerance)
                want = A.join_asof(lo, ro, strategy=strategy, tolerance=tolerance)
                assert want[1].tolist() == [bool(x) for x in want_ok]
                A.check(idx, valid, *want, (route, strategy, tolerance))
        lo = np.array([I64_MAX, 0], np.int64)
        ro = np.array([I64_MIN, I64_MIN, -5], np.int64)
        for tolerance in (U64_MAX, U64_MAX - 1, 1 << 63, (1 << 63) - 1, 5, 4):
            for strategy, strict in HOWS:
                idx, valid, _ = indices(pl, lo, ro, strategy=strategy, strict=strict, tolerance=tolerance)
                A.check(idx, valid, *A.join_asof(lo, ro, strategy=strategy, strict=strict, tolerance=tolerance), (route, strategy, strict, tolerance))
        lo = np.array([0, (1 << 63) - 1, 1 << 63, (1 << 63) + 5, U64_MAX], np.uint64)
        ro = np.array([1, 1 << 63, (1 << 63) + 4, (1 << 63) + 6, U64_MAX - 1], np.uint64)
        for tolerance in (None, 0, 1, U64_MAX):
            for strategy, strict in HOWS:
                idx, valid, _ = indices(pl, lo, ro, strategy=strategy, strict=strict, tolerance=tolerance)
                A.check(idx, valid, *A.join_asof(lo, ro, strategy=strategy, strict=strict, tolerance=tolerance), (route, "u64", strategy, strict, tolerance))


@pytest.mark.parametrize("npdt", [np.int8, np.int32, np.float32, np.float64])
def test_on_dtypes_with_nan_infinities_zeros_and_nulls(pl, monkeypatch, npdt):
    rng = np.random.default_rng(240)
    n, m = 300, 200
    if np.dtype(npdt).kind == "f":
        pool = np.array([-np.inf, -np.inf, -2.5, -0.0, 0.0, 0.25, 1.0, 1.0, 3.5, 1e30, np.inf, np.nan], npdt)
        lo, ro = pool[rng.integers(0, len(pool), n)], np.sort(pool[rng.integers(0, len(pool), m)])      # (np.sort puts NaN last: the sort's order)
        tolerances = (None, 0.0, 1.25, float("inf"))
    else:
        ii = np.iinfo(npdt)
        lo, ro = rng.integers(ii.min, ii.max, n, endpoint=True).astype(npdt), np.sort(rng.integers(max(ii.min, -500), min(ii.max, 500), m, endpoint=True).astype(npdt))
        tolerances = (None, 0, 3)
    lov, rov = rng.random(n) < 0.9, rng.random(m) < 0.9
    for route in both_routes(monkeypatch):
        for tolerance in tolerances:
            for strategy, strict in HOWS:
                idx, valid, plan = indices(pl, lo, ro, strategy=strategy, strict=strict, tolerance=tolerance, lov=lov, rov=rov)
                A.check(idx, valid, *A.join_asof(lo, ro, strategy=strategy, strict=strict, tolerance=tolerance, left_on_valid=lov, right_on_valid=rov), (npdt, route, tolerance, strategy, strict))
                assert "right=in order" in plan, plan                              # -0 before +0, NaN last: equal codes and the greatest code


def frame_of(pl, cols, dtypes=None):
    return pl.DataFrame([pl.Series(name, v, (dtypes or {}).get(name), validity=m) for name, (v, m) in cols.items()])


def matched_rows(df, name="j"):
    """the payload column that holds the right row index -> (idx, valid)"""
    return df[name]._download()


def test_temporal_on_with_a_timedelta_tolerance(pl, monkeypatch):
    rng = np.random.default_rng(250)
    n, m = 400, 300
    for dtype, unit_per_s, tolerance in ((pl.Datetime("ms"), 1_000, dt.timedelta(seconds=2)), (pl.Datetime("ns"), 1_000_000_000, dt.timedelta(microseconds=1500)),
                                         (pl.Datetime, 1_000_000, dt.timedelta(seconds=1)), (pl.Date, None, dt.timedelta(days=3))):
        if unit_per_s is None:
            lo, ro, npdt, tol = rng.integers(19000, 19100, n), rng.integers(19000, 19100, m), np.int32, 3
        else:
            tol = (tolerance.days * 86400 + tolerance.seconds) * unit_per_s + tolerance.microseconds * unit_per_s // 1_000_000
            lo, ro, npdt = 1_700_000_000 * unit_per_s + rng.integers(0, 40 * tol, n), 1_700_000_000 * unit_per_s + rng.integers(0, 40 * tol, m), np.int64
        lo, ro = lo.astype(npdt), ro.astype(npdt)
        L = frame_of(pl, {"t": (lo, None), "a": (np.arange(n), None)}, {"t": dtype})
        R = frame_of(pl, {"t": (ro, None), "j": (np.arange(m), None)}, {"t": dtype})
        for route in both_routes(monkeypatch):
            for strategy, strict in HOWS:
                got = L.join_asof(R, on="t", strategy=strategy, allow_exact_matches=not strict, tolerance=tolerance)
                assert got.columns == ["t", "a", "j"] and got.schema["t"] == dtype and got["a"].to_numpy().tolist() == list(range(n))
                A.check(*matched_rows(got), *A.join_asof(lo, ro, strategy=strategy, strict=strict, tolerance=tol), (dtype, route, strategy, strict))
                assert "right=sorted: " in pl.last_plan() and "JoinAsof{asof[" in pl.last_plan(), pl.last_plan()
    with pytest.raises(TypeError, match=r"join keys Datetime\[ms\] and Datetime\[ns\]"):                      # mixed units: the TypeError that join raises
        frame_of(pl, {"t": (np.arange(5), None)}, {"t": pl.Datetime("ms")}).join_asof(frame_of(pl, {"t": (np.arange(5), None)}, {"t": pl.Datetime("ns")}), on="t")


# ---- columns and places -------------------------------------------------------------------------------------------------------------------------------------------------
def test_columns_names_expressions_payloads_lazy_eager_and_neighbouring_nodes(pl):
    rng = np.random.default_rng(260)
    n, m = 500, 400
    lo, ro = rng.integers(0, 2000, n).astype(np.int64), rng.integers(0, 2000, m).astype(np.int64)
    lg, rg = rng.integers(0, 6, n).astype(np.int32), rng.integers(0, 5, m).astype(np.int32)
    cats = ["bid", "ask", "mid"]
    codes = rng.integers(0, 3, m).astype(np.uint32)
    L = frame_of(pl, {"sym": (lg, None), "t": (lo, None), "price": (rng.random(n), None)})
    R = frame_of(pl, {"sym": (rg, None), "t": (ro, None), "price": (rng.random(m), None), "side": (codes, None), "j": (np.arange(m), None)}, {"side": pl.Categorical(cats)})
    want = A.join_asof(lo, ro, [lg], [rg])
    assert want[1].any() and not want[1].all()
    got = L.join_asof(R, on="t", by="sym")
    assert got.columns == ["sym", "t", "price", "price_right", "side", "j"] and got.height == n
    A.check(*matched_rows(got), *want)
    assert got["t"].to_numpy().tolist() == lo.tolist() and got["price"].to_numpy().tolist() == L["price"].to_numpy().tolist()      # the left columns are the input's own
    assert got["side"].to_list() == [cats[codes[i]] if ok else None for i, ok in zip(want[0], want[1])]                               # a Categorical payload travels with its dictionary
    pv, pvalid = got["price_right"]._download()
    assert np.array_equal(pvalid, want[1]) and np.array_equal(pv[want[1]], R["price"].to_numpy()[want[0][want[1]]])
    assert pl.last_plan().count("JoinAsof{asof[backward, by=1, right=sorted: ") == 1 and "gather x3}" in pl.last_plan(), pl.last_plan()
    assert L.join_asof(R, on="t", by="sym", coalesce=True, suffix="_q").columns == ["sym", "t", "price", "price_q", "side", "j"]
    both = L.join_asof(R, on="t", by="sym", coalesce=False, suffix="_q")
    assert both.columns == ["sym", "t", "price", "sym_q", "t_q", "price_q", "side", "j"] and "gather x5}" in pl.last_plan()
    tq, tvalid = both["t_q"]._download()
    assert np.array_equal(tvalid, want[1]) and np.array_equal(tq[want[1]], ro[want[0][want[1]]]) and np.array_equal(both["sym_q"]._download()[0][want[1]], lg[want[1]])
    # other names on the right; lazy
    R2 = R.rename({"t": "qt", "sym": "qsym"})
    lazy = L.lazy().join_asof(R2.lazy(), left_on="t", right_on="qt", by_left="sym", by_right="qsym", strategy="forward")
    assert list(lazy.collect_schema()) == ["sym", "t", "price", "price_right", "side", "j"]
    out = lazy.collect()
    assert out.columns == list(lazy.collect_schema())
    A.check(*matched_rows(out), *A.join_asof(lo, ro, [lg], [rg], strategy="forward"))
    assert "JoinAsof[strategy=forward, by=[" in lazy.explain() and "JoinAsof{asof[forward" in lazy.explain()
    # an expression as `on` does not merge
    ex = L.join_asof(R, left_on=pl.col("t") + 1, right_on="t", by="sym")
    assert ex.columns == ["sym", "t", "price", "t_right", "price_right", "side", "j"]
    A.check(*matched_rows(ex), *A.join_asof(lo + 1, ro, [lg], [rg]))
    # integers of different width meet in their supertype
    L16 = frame_of(pl, {"sym": (lg, None), "t": (lo.astype(np.int16), None)})
    A.check(*matched_rows(L16.join_asof(R, on="t", by="sym", strategy="nearest")), *A.join_asof(lo, ro, [lg], [rg], strategy="nearest"))
    # after a filter, before a group_by
    keep_l, keep_r = lg != 2, ro % 3 != 0
    q = L.lazy().filter(pl.col("sym") != 2).join_asof(R.lazy().filter(pl.col("t") % 3 != 0), on="t", by="sym").group_by("sym").agg(pl.len().alias("rows"), pl.col("j").count().alias("hits"))
    res = q.collect().sort_host("sym")
    w = A.join_asof(lo[keep_l], ro[keep_r], [lg[keep_l]], [rg[keep_r]])
    syms = sorted(set(lg[keep_l].tolist()))
    assert res["sym"] == syms and res["rows"] == [int((lg[keep_l] == s).sum()) for s in syms] and res["hits"] == [int(w[1][lg[keep_l] == s].sum()) for s in syms]
    assert "JoinAsof{" in pl.last_plan(), pl.last_plan()
    # empty sides
    assert L.join_asof(R.slice(0, 0), on="t", by="sym")["j"].null_count() == n and "asof[empty]" in pl.last_plan()
    assert L.slice(0, 0).join_asof(R, on="t", by="sym").height == 0


def test_quote_before_trade_against_the_reference(pl):
    from polars_amd import datagen, queries
    trades, quotes = datagen.trades_quotes_native(pl, 5000, 3000, seed=5, n_syms=20, span_us=40_000_000)
    assert trades.schema == {"sym": pl.Int32, "ts": pl.Datetime, "price": pl.Float64} and quotes.height == 3000
    got = queries.quote_before_trade(trades.lazy(), quotes.lazy()).collect().sort_host("sym")
    plan = pl.last_plan()
    assert "JoinAsof{asof[backward, by=1, right=sorted: " in plan and "rows=5000 x 3000" in plan, plan
    ts, qs = trades["sym"].to_numpy(), quotes["sym"].to_numpy()
    tt, qt = trades["ts"].to_numpy(), quotes["ts"].to_numpy()
    tp, qp = trades["price"].to_numpy(), quotes["price"].to_numpy()
    idx, ok = A.join_asof(tt, qt, [ts], [qs], tolerance=1_000_000)
    assert 0.2 < ok.mean() < 0.999
    syms = sorted(set(ts.tolist()))
    assert got["sym"] == syms and got["trades"] == [int((ts == s).sum()) for s in syms] and got["quoted"] == [int(ok[ts == s].sum()) for s in syms]
    for s, mean, mx in zip(syms, got["mean_over_quote"], got["max_quote"]):
        sel = (ts == s) & ok
        assert mx == qp[idx[sel]].max() and abs(mean - float(np.mean(tp[sel] - qp[idx[sel]]))) <= 1e-9 * 200, (s, mean)      # a mean of ~250 differences below 20 each in f64


# ---- refusals on the device path -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_with_real_columns(pl):
    n = 10
    L = frame_of(pl, {"c": (np.zeros(n, np.uint32), None), "b": (np.zeros(n, bool), None), "t": (np.arange(n), None)}, {"c": pl.Categorical(["x"])})
    with pytest.raises(TypeError, match="Categorical by parts are not on this path yet"):
        L.join_asof(L, on="t", by="c")
    with pytest.raises(TypeError, match="`on` is Boolean"):
        L.join_asof(L, on="b")
    with pytest.raises(TypeError, match="`on` is Categorical"):
        L.join_asof(L, on="c")
    out = C.c_uint64()
    none = (C.c_uint64 * 1)()
    assert F.lib().plx_join_asof_indices(0, none, none, 0, L["b"]._h, L["b"]._h, None, C.byref(out)) == F.ERR_UNSUPPORTED and "`on` of dtype" in F.lib().plx_last_error().decode()
    assert F.lib().plx_join_asof_indices(3, none, none, 0, L["t"]._h, L["t"]._h, None, C.byref(out)) == 1 and "no plx_asof_strategy" in F.lib().plx_last_error().decode()
    assert F.lib().plx_join_asof_indices(0, none, none, 8, L["t"]._h, L["t"]._h, None, C.byref(out)) == F.ERR_UNSUPPORTED and "8 by parts" in F.lib().plx_last_error().decode()
    tol = F.Scalar()
    tol.f64 = -1.0
    x = pl.Series("x", np.zeros(3))
    assert F.lib().plx_join_asof_indices(0, none, none, 0, x._h, x._h, C.byref(tol), C.byref(out)) == 1 and "tolerance" in F.lib().plx_last_error().decode()
    tol.f64 = float("nan")
    assert F.lib().plx_join_asof_indices(0, none, none, 0, x._h, x._h, C.byref(tol), C.byref(out)) == 1 and "tolerance" in F.lib().plx_last_error().decode()
    with pytest.raises(F.PlxError, match="different lengths"):
        indices(pl, np.arange(4), np.arange(4), [np.arange(3).astype(np.int32)], [np.arange(4).astype(np.int32)])
