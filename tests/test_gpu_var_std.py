"""var / std on the device, against numpy's two-pass np.var per group, within the accuracy contract of DESIGN.md 4.14 (tests/program_eval_var.py within_contract:
|var - ref| <= 8 n eps (sigma^2 + D^2) n / (n - ddof), std through its square with twice the bound -- a function of the test's own data, no rtol).

Per node (Series.var / Series.std -> plx_reduce_var -> var_pivot_kernel + var_kernel + var_finish_kernel): every size at which the kernel takes another path
(tail only, one run, run + tail, two workgroups), seven dtypes, three ddof, the validity patterns that decide between null and a value; NaN / inf; a constant
column; a common offset of 1e15; bit-identical repeats; the C entry point and the two plugin symbols.
Fused (three cells about a pivot) and per node side by side: whole-column selects around the wave tile and the pivot sample, group-bys on the LDS / dense HBM / hash
HBM / wide-key routes with every kind of group that decides between null and a value, level differences between groups, one partitioned run, both forms of
join -> group-by, the run-time compiled kernel, Float32."""
import ctypes as C
import os
import struct

import numpy as np
import pyarrow as pa
import pytest

from tests import groupby_route_inputs as R
from tests import plugin_abi as P
from tests import program_eval_var as pv

pytestmark = pytest.mark.gpu

NP = {"Int8": np.int8, "UInt16": np.uint16, "Int32": np.int32, "Int64": np.int64, "UInt64": np.uint64, "Float32": np.float32, "Float64": np.float64}
K_BLOCK = 256                         # csrc/kconfig.hpp


def bits(x):
    return None if x is None else struct.pack("<d", x)


def draw(rng, npdt, n):
    if npdt == np.int64:
        return rng.integers(-(1 << 62), 1 << 62, n, dtype=np.int64)
    if npdt == np.uint64:
        return rng.integers(0, 1 << 64, n, dtype=np.uint64)      # above 2^63: a signed conversion would show
    if np.issubdtype(npdt, np.integer):
        ii = np.iinfo(npdt)
        return rng.integers(ii.min, int(ii.max) + 1, n).astype(npdt)
    return rng.normal(10.0, 3.0, n).astype(npdt)


def spread(x):
    x = np.asarray(x, np.float64)
    return float(x.max() - x.min()) if len(x) else 0.0


def check_series(pl, s, x, valid, ddofs, f32, what):
    xs = (x if valid is None else x[valid]).astype(np.float64)
    D = spread(xs)
    for ddof in ddofs:
        v, sd = s.var(ddof), s.std(ddof)
        assert pv.within_contract(v, xs, ddof, D, f32=f32), (what, "var", ddof, v, np.var(xs, ddof=ddof) if len(xs) > ddof else None)
        assert pv.within_contract(sd, xs, ddof, D, want_std=True, f32=f32), (what, "std", ddof, sd)
        if len(xs) == 1 and ddof == 0:
            assert v == 0.0 and sd == 0.0, (what, v, sd)


# ---- per node ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(NP))
def test_series_var_std_sizes_validity_ddof(pl, dtype):
    npdt = NP[dtype]
    V = 16 // np.dtype(npdt).itemsize
    run, B = 64 * V, K_BLOCK * V * 4
    rng = np.random.default_rng(7 + list(NP).index(dtype))
    ddofs = (0, 1, 3)
    n_checked = 0
    for n in (0, 1, 2, run - 1, run, run + 1, 2 * run + 3, B + 5, 2 * B + 5):
        x = draw(rng, npdt, n)
        patterns = {"none": None, "half": rng.random(n) < 0.5, "all_null": np.zeros(n, bool)}
        if n >= 1:
            one = np.zeros(n, bool); one[rng.integers(0, n)] = True
            last = np.zeros(n, bool); last[n - 1] = True
            patterns.update(one_valid=one, only_last=last)
        for ddof in ddofs:
            for extra in (0, 1):                                  # exactly ddof valid rows: null; ddof + 1: a value
                if 0 < ddof + extra <= n:
                    m = np.zeros(n, bool); m[rng.permutation(n)[:ddof + extra]] = True
                    patterns[f"valid_{ddof}+{extra}"] = m
        for name, valid in patterns.items():
            s = pl.Series("x", x, getattr(pl, dtype), validity=valid)
            check_series(pl, s, x, valid, ddofs, dtype == "Float32", (dtype, n, name))
            n_checked += 1
            if name == "all_null":
                assert s.var(0) is None and s.std(0) is None
            if name.startswith("valid_"):
                k = int(name[6:].split("+")[0])
                assert (s.var(k) is None) == name.endswith("+0") and (s.std(k) is None) == name.endswith("+0"), (dtype, n, name)
    assert n_checked >= 50


def test_series_nan_inf_constant_offset_and_repeats(pl):
    rng = np.random.default_rng(11)
    n = 2 * 64 * 2 + 3 + 2048                                    # runs of two workgroups' worth and a tail
    x = rng.normal(size=n)
    for special in (np.nan, np.inf, -np.inf):
        for pos in (0, 77, n - 1):
            y = x.copy(); y[pos] = special
            s = pl.Series("x", y)
            assert np.isnan(s.var()) and np.isnan(s.std(0)), (special, pos, s.var())
            m = np.ones(n, bool); m[pos] = False                  # ... unless that row is null
            sm = pl.Series("x", y, validity=m)
            assert pv.within_contract(sm.var(), y[m], 1, spread(y[m]))
    for npdt, val in ((np.float64, 0.1), (np.float64, -1e300), (np.int32, -7), (np.uint64, (1 << 64) - 1), (np.float32, 3.3)):
        s = pl.Series("c", np.full(n, val, dtype=npdt))
        assert s.var() == 0.0 and s.std() == 0.0 and s.var(0) == 0.0, (npdt, val, s.var())
    # a common offset: within the contract with D = 1.  The offset cancels exactly in x - 1e15 (every value is a multiple of 1/8 there), so the reference is
    # np.var of the shifted values; np.var of the raw values is itself off by the square of its mean's rounding error (printed, not asserted)
    u = rng.random(4101)
    y = 1e15 + u
    s = pl.Series("y", y)
    exact = y - 1e15
    got = s.var()
    print(f"offset 1e15: got {got!r}, np.var(x - 1e15) {np.var(exact, ddof=1)!r}, np.var(x) {np.var(y, ddof=1)!r}, bound {pv.contract_bound(exact, 1, 1.0)!r}")
    assert pv.within_contract(got, exact, 1, 1.0) and pv.within_contract(s.std(0), exact, 0, 1.0, want_std=True)
    ym = rng.random(len(y)) < 0.5
    assert pv.within_contract(pl.Series("y", y, validity=ym).var(), exact[ym], 1, 1.0)
    # more leading nulls than the origin search looks at (2^20 rows): the origin falls back to 0, the result is still inside the contract
    nl = (1 << 20) + 64
    z = np.concatenate([np.zeros(nl), rng.normal(3.0, 1.0, 5003)])
    zm = np.arange(len(z)) >= nl
    sz = pl.Series("z", z, validity=zm)
    assert pv.within_contract(sz.var(), z[zm], 1, float(np.abs(z[zm]).max())) and pv.within_contract(sz.std(0), z[zm], 0, float(np.abs(z[zm]).max()), want_std=True)
    # the same call twice: identical bits (no atomics anywhere)
    for s2 in (s, pl.Series("x", x, validity=rng.random(n) < 0.5), pl.Series("i", rng.integers(-9, 9, 100_003).astype(np.int8))):
        assert bits(s2.var()) == bits(s2.var()) and bits(s2.std(0)) == bits(s2.std(0))


def test_refusals_and_c_entry_points(pl):
    F = pl._ffi
    rng = np.random.default_rng(12)
    x = rng.normal(size=1000)
    s = pl.Series("x", x)
    v, dt, ok = F.Scalar(), C.c_int32(), C.c_int32()
    for ddof, want_std in ((0, 0), (1, 1), (5, 0)):
        F.check(F.lib().plx_reduce_var(s._h, ddof, want_std, C.byref(v), C.byref(dt), C.byref(ok)))
        assert ok.value == 1 and dt.value == F.F64 and pv.within_contract(v.f64, x, ddof, spread(x), want_std=bool(want_std))
    sf, se = pl.Series("f", x.astype(np.float32)), pl.Series("e", x[:3])
    F.check(F.lib().plx_reduce_var(sf._h, 1, 0, C.byref(v), C.byref(dt), C.byref(ok)))
    assert dt.value == F.F32 and pv.within_contract(float(np.float32(v.f32)), x.astype(np.float32), 1, spread(x), f32=True)
    F.check(F.lib().plx_reduce_var(se._h, 3, 0, C.byref(v), C.byref(dt), C.byref(ok)))
    assert ok.value == 0
    assert F.lib().plx_reduce(F.AGG_VAR, s._h, C.byref(v), C.byref(dt), C.byref(ok)) == 1 and "plx_reduce_var" in F.lib().plx_last_error().decode()
    assert F.lib().plx_reduce_var(s._h, 256, 0, C.byref(v), C.byref(dt), C.byref(ok)) == 1
    b = pl.Series("b", x > 0)
    assert F.lib().plx_reduce_var(b._h, 1, 0, C.byref(v), C.byref(dt), C.byref(ok)) == F.ERR_UNSUPPORTED and "bool" in F.lib().plx_last_error().decode().lower()
    with pytest.raises(TypeError, match="Boolean"):
        b.var()
    with pytest.raises(TypeError, match="0..255"):
        s.std(ddof=1.5)
    # plx_groupby_agg: ddof 1; plx_groupby_agg_ddof: one per aggregate
    k = rng.integers(0, 4, 1000).astype(np.int16)
    ks = pl.Series("k", k)
    keys, vals = (C.c_uint64 * 1)(ks._h), (C.c_uint64 * 3)(s._h, s._h, s._h)
    aggs, dd = (C.c_int32 * 3)(F.AGG_VAR, F.AGG_STD, F.AGG_MEAN), (C.c_int32 * 3)(0, 2, 9)
    for with_ddof in (False, True):
        ok_, oa = (C.c_uint64 * 1)(), (C.c_uint64 * 3)()
        if with_ddof:
            F.check(F.lib().plx_groupby_agg_ddof(keys, 1, vals, aggs, 3, 0, dd, ok_, oa))
        else:
            F.check(F.lib().plx_groupby_agg(keys, 1, vals, aggs, 3, 0, ok_, oa))
        gk = pl.Series._from_handle("k", ok_[0], pl.Int16).to_numpy()
        cols = [pl.Series._from_handle("a", h, pl.Float64).to_numpy() for h in oa]
        assert sorted(gk.tolist()) == [0, 1, 2, 3]
        for i, kv in enumerate(gk):
            xs = x[k == kv]
            assert pv.within_contract(float(cols[0][i]), xs, 0 if with_ddof else 1, spread(x))
            assert pv.within_contract(float(cols[1][i]), xs, 2 if with_ddof else 1, spread(x), want_std=True)
            assert abs(cols[2][i] - xs.mean()) < 1e-12


def test_plugin_symbols(pl):
    rng = np.random.default_rng(13)
    x = rng.normal(5.0, 2.0, 10_007)
    valid = rng.random(len(x)) < 0.8
    arr = pa.array(x, mask=~valid)
    chunked = pa.chunked_array([arr.slice(0, 4000), arr.slice(4000)])
    for name, is_std in (("plx_var", False), ("plx_std", True)):
        for kwargs, ddof in ((None, 1), ({"ddof": 0}, 0), ({"ddof": 3}, 3)):
            res, inp = P.call(name, [chunked], kwargs, names=["x"])
            assert res is not None, P.last_error()
            assert inp.released == 1 and len(res) == 1 and res.type == pa.float64() and inp.out_name == b"x"
            assert pv.within_contract(res[0].as_py(), x[valid], ddof, spread(x[valid]), want_std=is_std), (name, kwargs, res)
        res, _ = P.call(name, [pa.array(np.array([1.5], np.float32))], {"ddof": 1})
        assert res is not None and res.type == pa.float32() and res[0].as_py() is None           # one row, ddof 1: null
        res, inp = P.call(name, [arr], {"ddof": 300})
        assert res is None and inp.released == 1 and "0..255" in P.last_error()
        res, inp = P.call(name, [pa.array([True, False])])
        assert res is None and inp.released == 1 and "bool" in P.last_error().lower()


# ---- fused and per node, side by side --------------------------------------------------------------------------------------------------------
def both(pl, q, fused_word="Fused", **kw):
    """q fused and with no_fusion -> [(name, frame)]"""
    a = q.collect(**kw)
    plan = pl.last_plan()
    assert fused_word in plan and "var pivot" in plan, plan
    b = q.collect(no_fusion=True, **kw)
    return [("fused", a, plan), ("per_node", b, pl.last_plan())]


def one_row(out):
    return {k: v[0] for k, v in out.to_dict().items()}


def frame_of(pl, cols, dtypes=None):
    return pl.DataFrame([pl.Series(name, v, (dtypes or {}).get(name), validity=m) for name, (v, m) in cols.items()])


@pytest.mark.parametrize("n", [1, 127, 128, 129, 4096 + 7])
def test_whole_column_select(pl, n):
    rng = np.random.default_rng(100 + n)
    x, xm = rng.normal(50.0, 4.0, n), rng.random(n) < 0.8
    i = rng.integers(-1000, 1000, n).astype(np.int32)
    y = rng.uniform(1.0, 2.0, n)
    df = frame_of(pl, {"x": (x, xm), "i": (i, None), "y": (y, None)})
    c = pl.col
    aggs = [c("x").var().alias("xv"), c("x").std(0).alias("xs"), c("i").var(0).alias("iv"), (c("x") * c("y")).std().alias("xys"), c("x").mean().alias("m"), pl.len().alias("n")]
    xy = x * y
    for filt, keep in ((None, np.ones(n, bool)), (c("i") >= 0, i >= 0)):
        q = (df.lazy() if filt is None else df.lazy().filter(filt)).select(*aggs)
        for name, out, plan in both(pl, q):
            g = one_row(out)
            assert g["n"] == int(keep.sum())
            assert pv.within_contract(g["xv"], x[keep & xm], 1, spread(x[xm]) if xm.any() else 0.0), (name, n, g, plan)
            assert pv.within_contract(g["xs"], x[keep & xm], 0, spread(x[xm]) if xm.any() else 0.0, want_std=True), (name, n, g)
            assert pv.within_contract(g["iv"], i[keep].astype(np.float64), 0, spread(i)), (name, n, g)
            assert pv.within_contract(g["xys"], xy[keep & xm], 1, spread(xy[xm]) if xm.any() else 0.0, want_std=True), (name, n, g)


def test_pivot_falls_back_to_zero(pl):
    """the first 4096 rows are all null: no sample, p = 0, and the contract holds with D = max |x|"""
    rng = np.random.default_rng(21)
    n = 4096 + 3000
    x = rng.normal(0.0, 3.0, n)
    m = np.arange(n) >= 4096
    df = frame_of(pl, {"x": (x, m)})
    q = df.lazy().select(pl.col("x").var().alias("v"), pl.col("x").std(0).alias("s"))
    for name, out, plan in both(pl, q):
        if name == "fused":
            assert "var pivot x=0;" in plan, plan
        g = one_row(out)
        D = float(np.abs(x[m]).max())
        assert pv.within_contract(g["v"], x[m], 1, D) and pv.within_contract(g["s"], x[m], 0, D, want_std=True), (name, g)


def group_case(rng, n, route):
    """keys of one route + values: a null-key group, null values, a group of one row (row 1), a group whose every value is null"""
    small = n <= 1000
    if route == "lds":
        ids = rng.integers(0, 3, n)
        ids[1] = 3
        keys = {"k": ((ids - 1).astype(np.int16), None)}
    elif route == "dense":
        ids = rng.integers(0, 40, n) * 1249 if small else rng.integers(0, 49_999, n)
        ids[0], ids[1] = 0, 49_999
        keys = {"k": (ids.astype(np.uint16), None)}
    else:
        ids = rng.integers(0, 40, n) if small else rng.integers(0, 4999, n)
        ids[1] = 4999
        keys = {"k": (R.sparse(ids), None)} if route == "hash" else {"k": (R.full64(ids), None), "k2": (R.full64(ids + 12345), None)}
    kvalid = rng.random(n) > 0.05                                    # a null-key group
    kvalid[1] = True
    keys["k"] = (keys["k"][0], kvalid)
    if route == "wide":
        keys["k2"] = (np.where(kvalid, keys["k2"][0], np.int64(77)), None)      # (one null group: the second key column does not split it)
    gid = np.where(kvalid, ids, -1)
    x = rng.normal(20.0, 2.0, n)
    xm = rng.random(n) > 0.15
    xm[gid == gid[n // 2]] = False                                   # a group whose every value is null
    xm[1] = True                                                     # the one-row group: null at ddof 1, 0.0 at ddof 0
    y = rng.uniform(0.5, 1.5, n)
    i = rng.integers(-30000, 30000, n).astype(np.int32)
    emptied = gid[[r for r in range(n) if gid[r] not in (gid[n // 2], gid[1])][0]]
    i[gid == emptied] = -7                                           # a group that the filter i > 0 empties
    i[1] = 5
    cols = dict(keys)
    cols.update(x=(x, xm), y=(y, None), i=(i, None))
    return cols, list(keys), gid


def grouped_two_pass(inv, G, sel, x):
    """count, mean and centred sum of squares of x[sel] per group: the two-pass variance of every group at once"""
    g = inv[sel]
    cnt = np.bincount(g, minlength=G).astype(np.float64)
    mean = np.bincount(g, weights=x[sel], minlength=G) / np.maximum(cnt, 1.0)
    m2 = np.bincount(g, weights=(x[sel] - mean[g]) ** 2, minlength=G)
    return cnt, mean, m2


def check_grouped(got, got_valid, gidx, stats, ddof, is_std, D, what):
    """every output row against the two-pass reference of its group within the contract"""
    cnt, _, m2 = (a[gidx] for a in stats)
    want_valid = cnt > ddof
    got_valid = np.ones(len(got), bool) if got_valid is None else got_valid
    assert np.array_equal(got_valid, want_valid), (what, "null groups", int((got_valid != want_valid).sum()))
    ok = want_valid
    ref = m2[ok] / (cnt[ok] - ddof)
    bound = 8.0 * cnt[ok] * pv.EPS * (m2[ok] / cnt[ok] + D * D) * cnt[ok] / (cnt[ok] - ddof)
    g = got[ok].astype(np.float64)
    if is_std:
        g, bound = g * g, 2.0 * bound
    bad = np.nonzero(~(np.abs(g - ref) <= bound))[0]
    assert len(bad) == 0, (what, f"{len(bad)} of {int(ok.sum())} groups outside the contract", g[bad[:3]], ref[bad[:3]], bound[bad[:3]])
    exact_zero = ok & (cnt == 1)
    assert np.all(got[exact_zero] == 0.0), (what, "one row at ddof 0 is exactly 0.0")


ROUTE_WORD = {"lds": "lds_table(", "dense": "dense_hbm_table(", "hash": "]+hash_hbm_table(", "wide": "wide_hash_hbm_table("}


@pytest.mark.parametrize("n", [389, 1 << 16])
@pytest.mark.parametrize("route", ["lds", "dense", "hash", "wide"])
def test_group_by_routes(pl, monkeypatch, route, n):
    monkeypatch.setenv("PLX_LEARN_DENSE_RANGE", "0")
    rng = np.random.default_rng(1000 + n + ["lds", "dense", "hash", "wide"].index(route))
    cols, key_names, gid = group_case(rng, n, route)
    (x, xm), (y, _), (i, _) = cols["x"], cols["y"], cols["i"]
    df = frame_of(pl, cols)
    c = pl.col
    aggs = [c("x").var().alias("xv1"), c("x").var(0).alias("xv0"), c("x").std().alias("xs1"), c("i").var().alias("iv"), (c("x") * c("y")).var(0).alias("xyv"),
            c("x").mean().alias("m"), c("x").sum().alias("s"), c("x").min().alias("mn"), pl.len().alias("n")]
    xy, fi = x * y, i.astype(np.float64)
    Dx, Di, Dxy = spread(x[xm]), spread(i), spread(xy[xm])
    ug, inv = np.unique(gid, return_inverse=True)
    G = len(ug)
    src_k = cols["k"][0]
    key_of = np.zeros(G, src_k.dtype)
    key_of[inv] = src_k
    index_of = {(None if ug[j] == -1 else int(key_of[j])): j for j in range(G)}
    kw = {"no_partition": True} if route == "hash" else {}
    for filt, keep in ((None, np.ones(n, bool)), (c("i") > 0, i > 0)):      # (the filter empties groups: among them one-row groups whose i is not positive)
        q = (df.lazy() if filt is None else df.lazy().filter(filt)).group_by(*key_names).agg(*aggs)
        rows_all = grouped_two_pass(inv, G, keep, fi)
        st_x, st_xy = grouped_two_pass(inv, G, keep & xm, x), grouped_two_pass(inv, G, keep & xm, xy)
        present = rows_all[0] > 0
        assert filt is None or present.sum() < G                # the filter empties at least one group
        for name, out, plan in both(pl, q, **kw):
            what = (name, route, n, "filtered" if filt is not None else "all rows")
            if name == "fused":
                assert ROUTE_WORD[route] in plan, plan
            d = R.download(out)
            kv, kok = d["k"]
            kok = np.ones(len(kv), bool) if kok is None else kok
            gidx = np.array([index_of[int(kv[r]) if kok[r] else None] for r in range(out.height)], dtype=np.int64)
            assert out.height == int(present.sum()) and np.array_equal(np.sort(gidx), np.nonzero(present)[0]), (what, out.height, int(present.sum()))
            assert np.array_equal(d["n"][0].astype(np.int64), rows_all[0][gidx].astype(np.int64)), what
            check_grouped(d["xv1"][0], d["xv1"][1], gidx, st_x, 1, False, Dx, what + ("xv1",))
            check_grouped(d["xv0"][0], d["xv0"][1], gidx, st_x, 0, False, Dx, what + ("xv0",))
            check_grouped(d["xs1"][0], d["xs1"][1], gidx, st_x, 1, True, Dx, what + ("xs1",))
            check_grouped(d["iv"][0], d["iv"][1], gidx, rows_all, 1, False, Di, what + ("iv",))
            check_grouped(d["xyv"][0], d["xyv"][1], gidx, st_xy, 0, False, Dxy, what + ("xyv",))
            cnt, mean, _ = (a[gidx] for a in st_x)
            has = cnt > 0
            mvalid = np.ones(len(kv), bool) if d["m"][1] is None else d["m"][1]
            assert np.array_equal(mvalid, has) and np.allclose(d["m"][0][has], mean[has], rtol=1e-9), what
            assert (~has).sum() >= 1, what                       # the all-null group (and whatever the nulls emptied): var, std and mean are null there
            if filt is None:
                one = gidx == index_of[int(src_k[1])]
                assert one.sum() == 1 and cnt[one][0] == 1, what
                v1ok = np.ones(len(kv), bool) if d["xv1"][1] is None else d["xv1"][1]
                assert not v1ok[one][0] and d["xv0"][0][one][0] == 0.0, what      # one row: null at ddof 1, 0.0 at ddof 0
            # a sample of the groups against np.var itself
            for r in rng.permutation(out.height)[:25]:
                rows = keep & (inv == gidx[r])
                val = lambda nm: None if (d[nm][1] is not None and not d[nm][1][r]) else float(d[nm][0][r])
                assert pv.within_contract(val("xv1"), x[rows & xm], 1, Dx) and pv.within_contract(val("xs1"), x[rows & xm], 1, Dx, want_std=True), (what, r)
                assert pv.within_contract(val("iv"), fi[rows], 1, Di) and pv.within_contract(val("xyv"), xy[rows & xm], 0, Dxy), (what, r)
                if (rows & xm).any():
                    assert val("mn") == x[rows & xm].min() and abs(val("s") - x[rows & xm].sum()) <= 1e-9 * np.abs(x[rows & xm]).sum(), (what, r)


def test_level_differences_between_groups(pl):
    """group g holds 1000 g + N(0, 1), 64 groups of 1024 rows: D / sigma is about 6e4, the bound a few 1e-3 relative -- the hole of the fused path, stated and held."""
    rng = np.random.default_rng(31)
    G, per = 64, 1024
    g = np.repeat(np.arange(G), per)
    rng.shuffle(g)
    x = 1000.0 * g + rng.normal(size=G * per)
    df = frame_of(pl, {"k": (g.astype(np.int16), None), "x": (x, None)})
    q = df.lazy().group_by("k").agg(pl.col("x").var().alias("v"), pl.col("x").std(0).alias("s"))
    D = spread(x)
    for name, out, plan in both(pl, q):
        d = out.to_dict()
        worst = 0.0
        for kv, v, s in zip(d["k"], d["v"], d["s"]):
            xs = x[g == kv]
            assert pv.within_contract(v, xs, 1, D) and pv.within_contract(s, xs, 0, D, want_std=True), (name, kv, v, np.var(xs, ddof=1))
            worst = max(worst, abs(v - np.var(xs, ddof=1)) / np.var(xs, ddof=1))
        print(f"level differences [{name}]: worst relative error {worst:.3e}, bound {pv.contract_bound(x[g == 0], 1, D) / np.var(x[g == 0], ddof=1):.3e} relative")


def test_partitioned_route(pl):
    """2^24 rows (the partitioned routes start there), 300 000 sparse keys, x.var() + x.mean(): two f64 sources and a key in the record.  The reference is the
    two-pass variance of every group at once (bincount), checked against np.var itself for a sample of the groups."""
    rng = np.random.default_rng(41)
    n, G = R.N24, 300_000
    ids = rng.integers(0, G, n)
    x = rng.normal(100.0, 5.0, n)
    df = pl.DataFrame([pl.Series("k", R.sparse(ids)), pl.Series("x", x)])
    out = df.lazy().group_by("k").agg(pl.col("x").var().alias("v"), pl.col("x").mean().alias("m")).collect()
    plan = pl.last_plan()
    assert "partitioned(" in plan and "var pivot x=" in plan and "hbm_table" not in plan, plan
    cnt = np.bincount(ids, minlength=G).astype(np.float64)
    mean = np.bincount(ids, weights=x, minlength=G) / cnt
    m2 = np.bincount(ids, weights=(x - mean[ids]) ** 2, minlength=G)
    ref = m2 / (cnt - 1)
    for gsel in rng.integers(0, G, 20):
        assert abs(ref[gsel] - np.var(x[ids == gsel], ddof=1)) <= 4 * cnt[gsel] * pv.EPS * ref[gsel]
    d = R.download(out)
    back = ((d["k"][0] + 10 ** 12) // 1_000_003).astype(np.int64)
    assert out.height == G and np.array_equal(np.sort(back), np.arange(G))
    v, mm = d["v"][0], d["m"][0]
    D = spread(x)
    bound = 8.0 * cnt[back] * pv.EPS * (m2[back] / cnt[back] + D * D) * cnt[back] / (cnt[back] - 1)
    bad = np.nonzero(~(np.abs(v - ref[back]) <= bound))[0]
    assert len(bad) == 0 and d["v"][1] is None, (len(bad), v[bad[:3]], ref[back][bad[:3]])
    assert np.allclose(mm, mean[back], rtol=1e-12)


def test_join_group_by_both_forms(pl, monkeypatch):
    monkeypatch.setenv("PLX_JOIN_MATERIALISE", "2")
    rng = np.random.default_rng(51)
    nb, n = 1 << 8, 1 << 12
    bk = R.sparse(rng.permutation(1000)[:nb])
    b_y, b_c = rng.integers(0, 6, nb).astype(np.int16), rng.uniform(0, 10, nb)
    pk = bk[rng.integers(0, nb, n)]
    w, wm = rng.normal(7.0, 2.0, n), rng.random(n) > 0.1
    B = pl.DataFrame([pl.Series("k", bk), pl.Series("y", b_y), pl.Series("c", b_c)])
    Pf = pl.DataFrame([pl.Series("k", pk), pl.Series("w", w, validity=wm)])
    row_of = {int(k): r for r, k in enumerate(bk)}
    brow = np.array([row_of[int(k)] for k in pk])
    # in place: var of a probe-side column, grouped by the join key
    q = Pf.lazy().join(B.lazy(), on="k").group_by("k").agg(pl.col("w").var().alias("v"), pl.col("w").std(0).alias("s"), pl.len().alias("n"))
    for name, out, plan in both(pl, q, fused_word="FusedJoinGroupBy{build="):
        d = out.to_dict()
        assert out.height == len(np.unique(pk))
        for kv, v, s, cnt in zip(d["k"], d["v"], d["s"], d["n"]):
            rows = pk == kv
            assert cnt == int(rows.sum())
            assert pv.within_contract(v, w[rows & wm], 1, spread(w[wm])) and pv.within_contract(s, w[rows & wm], 0, spread(w[wm]), want_std=True), (name, kv, v)
    # pair form: var of a build-side column, grouped by a build-side column
    q = Pf.lazy().join(B.lazy(), on="k").group_by("y").agg(pl.col("c").var().alias("v"), pl.col("c").std(2).alias("s"), pl.len().alias("n"))
    for name, out, plan in both(pl, q, fused_word="FusedJoinGroupBy{pair form"):
        d = out.to_dict()
        assert sorted(d["y"]) == sorted(np.unique(b_y[brow]).tolist())
        cj = b_c[brow]
        for yv, v, s, cnt in zip(d["y"], d["v"], d["s"], d["n"]):
            rows = b_y[brow] == yv
            assert cnt == int(rows.sum())
            assert pv.within_contract(v, cj[rows], 1, spread(b_c)) and pv.within_contract(s, cj[rows], 2, spread(b_c), want_std=True), (name, yv, v)


def test_run_time_compiled_kernel_and_generic_interpreter_agree(pl):
    F = pl._ffi
    rng = np.random.default_rng(61)
    n = 50_003
    k = rng.integers(0, 9, n).astype(np.int16)
    x, xm = rng.normal(-3.0, 1.5, n), rng.random(n) > 0.2
    df = frame_of(pl, {"k": (k, None), "x": (x, xm)})
    q = df.lazy().filter(pl.col("x") < 0).group_by("k").agg(pl.col("x").var().alias("v"), pl.col("x").std(0).alias("s"), pl.col("x").count().alias("cnt"))
    generic = q.collect()
    assert "[generic]" in pl.last_plan(), pl.last_plan()
    try:
        F.jit_set_min_rows(0)
        before = F.jit_stats()[0]
        jit = q.collect()
        assert "[jit]" in pl.last_plan() and F.jit_stats()[0] > before, pl.last_plan()
    finally:
        F.jit_set_min_rows(1 << 22)
    a, b = generic.sort_host("k"), jit.sort_host("k")
    assert a["k"] == b["k"] and a["cnt"] == b["cnt"]
    keep = (x < 0) & xm
    for kv, va, vb, sa, sb in zip(a["k"], a["v"], b["v"], a["s"], b["s"]):
        xs = x[keep & (k == kv)]
        for v, s in ((va, sa), (vb, sb)):
            assert pv.within_contract(v, xs, 1, spread(x[xm])) and pv.within_contract(s, xs, 0, spread(x[xm]), want_std=True)
        # the same cells up to the order of the additions: far inside the contract of either
        assert abs(va - vb) <= pv.contract_bound(xs, 1, spread(x[xm]))


def test_float32_source_gives_float32(pl):
    rng = np.random.default_rng(71)
    n = 10_001
    f = rng.normal(2.0, 1.0, n).astype(np.float32)
    k = rng.integers(0, 5, n).astype(np.int16)
    df = frame_of(pl, {"k": (k, None), "f": (f, None)})
    out = df.lazy().group_by("k").agg(pl.col("f").var().alias("v"), pl.col("f").std(0).alias("s")).collect()
    assert out.schema["v"] == pl.Float32 and out.schema["s"] == pl.Float32 and out["v"].to_numpy().dtype == np.float32
    d = out.to_dict()
    for kv, v, s in zip(d["k"], d["v"], d["s"]):
        xs = f[k == kv].astype(np.float64)
        assert pv.within_contract(v, xs, 1, spread(f), f32=True) and pv.within_contract(s, xs, 0, spread(f), want_std=True, f32=True), (kv, v, s)
    sel = df.lazy().select(pl.col("f").std().alias("s")).collect()
    assert sel.schema["s"] == pl.Float32 and pv.within_contract(sel.to_dict()["s"][0], f.astype(np.float64), 1, spread(f), want_std=True, f32=True)
    assert pv.within_contract(df["f"].var(), f.astype(np.float64), 1, spread(f), f32=True)


def test_h2o_sd_example_fused_and_per_node(pl):
    from polars_amd import queries as Q
    rng = np.random.default_rng(81)
    n = 100_003
    id4, id5, v3 = rng.integers(1, 101, n).astype(np.int32), rng.integers(1, 101, n).astype(np.int32), rng.uniform(0, 100, n)
    df = pl.DataFrame([pl.Series("id4", id4), pl.Series("id5", id5), pl.Series("v3", v3)])
    code = id4.astype(np.int64) * 1000 + id5
    order = np.argsort(code, kind="stable")
    starts = np.flatnonzero(np.r_[True, np.diff(code[order]) != 0])
    groups = {int(code[order[s]]): v3[order[s:e]] for s, e in zip(starts, np.r_[starts[1:], n])}
    for name, out, plan in both(pl, Q.h2o_sd(df.lazy())):
        d = out.to_dict()
        assert out.height == len(groups)
        for a, b, sd, m in zip(d["id4"], d["id5"], d["v3_sd"], d["v3_mean"]):
            xs = groups[a * 1000 + b]
            assert pv.within_contract(sd, xs, 1, spread(v3), want_std=True) and abs(m - xs.mean()) <= 1e-12 * 100, (name, a, b, sd)


def test_h2o_sd_example_partitioned(pl):
    """queries.h2o_sd on a partitioned route: 2^24 rows (the partitioned routes start there), id4 and id5 in 1..1000 -- a 20-bit packed id, 10^6 groups -- against the
    two-pass variance of every group at once (bincount), checked against np.var itself for a sample of the groups; the same frame per node for the same answers."""
    from polars_amd import queries as Q
    rng = np.random.default_rng(82)
    n, K = R.N24, 1000
    id4, id5, v3 = rng.integers(1, K + 1, n).astype(np.int32), rng.integers(1, K + 1, n).astype(np.int32), rng.uniform(0, 100, n)
    df = pl.DataFrame([pl.Series("id4", id4), pl.Series("id5", id5), pl.Series("v3", v3)])
    code = (id4.astype(np.int64) - 1) * K + (id5 - 1)
    G = K * K
    cnt = np.bincount(code, minlength=G).astype(np.float64)
    mean = np.bincount(code, weights=v3, minlength=G) / np.maximum(cnt, 1.0)
    m2 = np.bincount(code, weights=(v3 - mean[code]) ** 2, minlength=G)
    present = np.nonzero(cnt > 0)[0]
    for gsel in present[rng.integers(0, len(present), 20)]:
        if cnt[gsel] > 1:
            ref = np.var(v3[code == gsel], ddof=1)
            assert abs(m2[gsel] / (cnt[gsel] - 1) - ref) <= 4 * cnt[gsel] * pv.EPS * ref
    D = spread(v3)
    for name, kw in (("partitioned", {}), ("per_node", {"no_fusion": True})):
        out = Q.h2o_sd(df.lazy()).collect(**kw)
        plan = pl.last_plan()
        if name == "partitioned":
            assert "partitioned(" in plan and "var pivot v3=" in plan and "hbm_table" not in plan, plan
        d = R.download(out)
        back = (d["id4"][0].astype(np.int64) - 1) * K + (d["id5"][0] - 1)
        assert out.height == len(present) and np.array_equal(np.sort(back), present), (name, out.height, len(present))
        c = cnt[back]
        ok = c > 1
        sd_valid = np.ones(len(back), bool) if d["v3_sd"][1] is None else d["v3_sd"][1]
        assert np.array_equal(sd_valid, ok), (name, "one-row groups are null at ddof 1")
        ref = m2[back][ok] / (c[ok] - 1)
        bound = 2.0 * 8.0 * c[ok] * pv.EPS * (m2[back][ok] / c[ok] + D * D) * c[ok] / (c[ok] - 1)      # std: through its square, twice the bound
        got = d["v3_sd"][0][ok].astype(np.float64) ** 2
        bad = np.nonzero(~(np.abs(got - ref) <= bound))[0]
        assert len(bad) == 0, (name, len(bad), got[bad[:3]], ref[bad[:3]], bound[bad[:3]])
        assert np.allclose(d["v3_mean"][0], mean[back], rtol=1e-12, atol=0), name
