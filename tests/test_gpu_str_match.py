"""String predicates on the GPU: strview_match_kernel over raw views (Series.str on a column of deferred views) and over a device dictionary
(plx_strdict_match), bitmap_lookup_kernel (plx_bitmap_lookup), and str.starts_with / ends_with / contains inside plans -- fused (OP_BITLOOKUP inside the scan) and
per node -- as a filter, under ~ and &, as the condition of when/then/otherwise, as a group key, and in TPC-H Q14 with its real predicate.  The reference is Python's
bytes.startswith / endswith / in on the host strings (tests/str_match_corpus.py, cross-checked with pyarrow on the CPU side); Booleans are compared exactly, values
and validity.  Numeric columns hold multiples of 1/8, so every sum is exact in f64 whatever the order of the additions, and is compared exactly too."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pytest

from tests import str_match_corpus as K

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 63, 64, 65, 129, 1000]


@pytest.fixture(scope="module")
def corpus():
    views, data = K.views_of(K.STRINGS)
    refs = {(kind, p): K.reference(kind, K.STRINGS, p) for kind in K.KINDS for p in K.PATTERNS}        # computed once, shared, never changed
    return views, data, refs


def raw_series(pl, views, data):
    v = pl.Series("v", np.ascontiguousarray(views).reshape(-1), pl.UInt64)
    d = pl.Series("d", np.frombuffer(data, np.uint8), pl.UInt8) if data is not None else None
    return pl.Series.from_device_views("s", v, d, encode="deferred")


def check_bool(s, want, what):
    want_v, want_m = K.split(want)
    got_v, got_m = s._download()
    assert len(got_v) == len(want_v), what
    got_m = np.ones(len(want_v), bool) if got_m is None else got_m
    assert np.array_equal(got_m, want_m) and np.array_equal(got_v & got_m, want_v), what
    assert s.null_count() == int((~want_m).sum()), what


# ---- the kernel over raw views ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ROWS)
def test_raw_views_long_and_inline_with_a_pool(pl, corpus, n):
    F = pl._ffi
    views, data, refs = corpus
    s = raw_series(pl, K.tile_views(views, n), data)
    for (kind, p), ref in refs.items():
        out = getattr(s.str, K.KINDS[kind])(p)
        assert out.dtype == pl.Boolean and out.name == "s"
        want = K.tile(ref, n)
        check_bool(out, want, (K.KINDS[kind], p, n))
        st, hv, hm, _ = K.host_match(K.tile_views(views, n), data, kind, p)                     # ... and equals the host twin
        assert st == 0 and np.array_equal(hv, K.split(want)[0]) and np.array_equal(hm, K.split(want)[1])
    assert s._is_raw_views()                                                                      # nothing encoded the column


@pytest.mark.parametrize("n", ROWS)
def test_raw_views_inline_only_without_a_pool(pl, corpus, n):
    views, data, refs = corpus
    rows = [i for i, x in enumerate(K.STRINGS) if x is None or len(x.encode()) <= 12]
    s = raw_series(pl, K.tile_views(views[rows], n), None)
    for (kind, p), ref in refs.items():
        check_bool(getattr(s.str, K.KINDS[kind])(p), K.tile([ref[i] for i in rows], n), (K.KINDS[kind], p, n))
    assert s._is_raw_views()


def test_raw_views_errors_and_the_prefix_path(pl, corpus):
    F = pl._ffi
    views, data, refs = corpus
    long_rows = [i for i, x in enumerate(K.STRINGS) if x is not None and len(x.encode()) > 12]
    longs = K.tile_views(views[long_rows], 200)
    no_pool = raw_series(pl, longs, None)
    for p in ("", "P", "PROM", "zero"):                                                           # decided from the 4-byte prefix in the view: no pool needed
        want = K.tile([K.reference(F.STR_STARTS_WITH, [K.STRINGS[i]], p)[0] for i in long_rows], 200)
        check_bool(no_pool.str.starts_with(p), want, p)
    check_bool(no_pool.str.starts_with("QROMO PLATED"), [False] * 200, "prefix mismatch")        # rejected by the prefix before the pool is needed
    with pytest.raises(pl.PlxError, match="needs the data buffer"):
        no_pool.str.ends_with("x")
    with pytest.raises(pl.PlxError, match="needs the data buffer"):
        no_pool.str.starts_with("PROMO")
    bad = longs.copy()
    bad[137, 1] = (int(bad[137, 1]) & 0xFFFFFFFF) | ((len(data) - 2) << 32)                       # one view whose bytes would end past the pool: flagged, never read
    with pytest.raises(pl.PlxError, match="points outside its buffer"):
        raw_series(pl, bad, data).str.contains("a")
    with pytest.raises(pl.UnsupportedError, match="64 bytes"):
        raw_series(pl, longs, data).str.contains("y" * 65)
    check_bool(raw_series(pl, longs, data).str.contains("y" * 64), [False] * 200, "64 bytes")
    # a bitmap on the UInt64 column of views is not how a view column carries nulls (it would count words, not views): refused, not ignored
    flat = np.ascontiguousarray(longs).reshape(-1)
    masked = pl.Series("v", flat, pl.UInt64, validity=np.arange(len(flat)) != 3)
    with pytest.raises(pl.PlxError, match="stamped views"):
        pl.Series.from_device_views("s", masked, None, encode="deferred").str.starts_with("P")
    with pytest.raises(TypeError, match="regular expressions"):
        no_pool.str.contains("a.*", literal=False)
    with pytest.raises(TypeError, match="string column"):
        pl.Series("i", np.arange(4)).str.starts_with("a")


# ---- the kernel over a device dictionary -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", [False, True])
def test_device_dictionary_match_in_code_order(pl, corpus, binary):
    F = pl._ffi
    strings = K.tile(K.STRINGS, 300)
    arr = pa.array([K.as_bytes(x) for x in strings], pa.binary_view()) if binary else pa.array(strings, pa.string_view())
    s = pl.Series.from_arrow("s", arr)
    cats = s.dtype.categories
    assert hasattr(cats, "_load") and cats._h and len(cats) == len({x for x in K.STRINGS if x is not None})
    got = {}
    for kind in K.KINDS:
        for p in K.PATTERNS:
            pb = K.as_bytes(p)
            h = C.c_uint64()
            F.check(F.lib().plx_strdict_match(cats._h, kind, pb, len(pb), C.byref(h)))
            col = pl.Series._from_handle("m", h.value, pl.Boolean)
            assert len(col) == len(cats) and col.null_count() == 0
            got[(kind, p)] = col._download()[0]
    # Series.str on the dictionary column: dictionary match + lookup by code, without downloading the dictionary
    rows = {(kind, p): getattr(s.str, K.KINDS[kind])(p if not binary else K.as_bytes(p)) for kind in K.KINDS for p in ("PROMO", "ld!!", "\0", "")}
    assert cats._items is None and cats._h
    entries = list(cats)                                                                         # (downloads the dictionary: last)
    for (kind, p), bits in got.items():
        assert bits.tolist() == K.reference(kind, entries, p), (K.KINDS[kind], p)
    for (kind, p), col in rows.items():
        check_bool(col, K.reference(kind, strings, p), (K.KINDS[kind], p))


# ---- the per-node lookup kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["UInt8", "UInt16", "UInt32", "Int8", "Int32", "Int64"])
def test_bitmap_lookup_kernel(pl, dtype):
    F = pl._ffi
    rng = np.random.default_rng(len(dtype))
    npdt = np.dtype(dtype.lower())
    for n in (0, 1, 64, 65, 1000):
        for range_ in (1, 64, 65, 200):
            lut = rng.random(range_) < 0.5
            hi = min(int(np.iinfo(npdt).max), range_ + 20)
            lo = -5 if npdt.kind == "i" else 0
            codes = rng.integers(lo, hi, n, endpoint=True).astype(npdt)                            # codes at, beyond and (signed) below the range
            valid = rng.random(n) < 0.8
            for with_nulls in (True, False):
                cs, ls = pl.Series("c", codes, getattr(pl, dtype), validity=valid if with_nulls else None), pl.Series("l", lut, pl.Boolean)
                h = C.c_uint64()
                F.check(F.lib().plx_bitmap_lookup(cs._h, ls._h, C.byref(h)))
                inside = (codes.astype(np.int64) >= 0) & (codes.astype(np.int64) < range_)
                want = np.where(inside, lut[np.clip(codes.astype(np.int64), 0, range_ - 1)], False)
                m = valid if with_nulls else np.ones(n, bool)
                check_bool(pl.Series._from_handle("o", h.value, pl.Boolean), [bool(v) if ok else None for v, ok in zip(want, m)], (dtype, n, range_, with_nulls))
    h = C.c_uint64()
    f64, u8, ok = pl.Series("f", np.zeros(3)), pl.Series("c", np.zeros(3, np.uint8)), pl.Series("l", np.ones(3, bool))
    with_null = pl.Series("l", np.ones(3, bool), pl.Boolean, validity=np.array([True, False, True]))
    with pytest.raises(pl.PlxError, match="integer column"):
        F.check(F.lib().plx_bitmap_lookup(f64._h, ok._h, C.byref(h)))
    with pytest.raises(pl.PlxError, match="Boolean column"):
        F.check(F.lib().plx_bitmap_lookup(u8._h, u8._h, C.byref(h)))
    with pytest.raises(pl.PlxError, match="must not hold nulls"):
        F.check(F.lib().plx_bitmap_lookup(u8._h, with_null._h, C.byref(h)))


# ---- through plans ---------------------------------------------------------------------------------------------------------------------------
TYPES = ["PROMO BURNISHED TIN", "STANDARD PLATED STEEL", "PROMO ANODIZED COPPER", "ECONOMY PROMO", "SMALL BRUSHED BRASS", "PROMO", "LARGE PROM", "PROMO PLATED",
         "MEDIUM POLISHED NICKEL PROMO", "promo lower case", "", "PROMOTION"]


def plan_table(pl, n, device_dict):
    rng = np.random.default_rng(n + int(device_dict))
    strings = [None if rng.random() < 0.15 else TYPES[i] for i in rng.integers(0, len(TYPES), n)]
    k = rng.integers(0, 4, n).astype(np.int64)
    x, xm = rng.integers(-800, 800, n) / 8.0, rng.random(n) < 0.85
    y = rng.integers(-9, 9, n).astype(np.int64)
    s = pl.Series.from_arrow("s", pa.array(strings, pa.string_view() if device_dict else pa.string()))
    df = pl.DataFrame([s, pl.Series("k", k), pl.Series("x", x, pl.Float64, validity=xm), pl.Series("y", y)])
    return df, strings, k, x, xm, y


@pytest.mark.parametrize("device_dict", [True, False], ids=["device_dictionary", "host_list"])
@pytest.mark.parametrize("n", [1000, 3 * 128 + 1])
def test_plans_fused_and_per_node(pl, n, device_dict):
    F = pl._ffi
    c = pl.col
    df, strings, k, x, xm, y = plan_table(pl, n, device_dict)
    where = "device" if device_dict else "host"
    n_cats = len(df["s"].dtype.categories)
    ref = np.array([v if v is not None else False for v in K.reference(F.STR_STARTS_WITH, strings, "PROMO")], dtype=bool)
    valid = np.array([v is not None for v in strings])
    pred = c("s").str.starts_with("PROMO")
    note = f"str.starts_with('PROMO') over {n_cats} categories [{where}]"

    def group_rows(d, key):
        return {kk: {name: d[name][i] for name in d if name != key} for i, kk in enumerate(d[key])}

    for kw in ({}, {"no_fusion": True}):
        # filter -> frame, rows in input order
        for p, keep in ((pred, ref & valid), (~pred, ~ref & valid), (pred & (c("y") > 0), ref & valid & (y > 0)), (c("s").str.contains("PLATED") | c("s").str.ends_with("PROMO"),
                        valid & np.array([s is not None and ("PLATED" in s or s.endswith("PROMO")) for s in strings]))):
            out = df.lazy().filter(p).select("y", "k", "x").collect(**kw)
            assert "str." in pl.last_plan() and f"[{where}]" in pl.last_plan(), pl.last_plan()
            d = out.to_dict()
            assert d["y"] == y[keep].tolist() and d["k"] == k[keep].tolist(), (kw, repr(p))
            assert d["x"] == [v if ok else None for v, ok in zip(x[keep].tolist(), xm[keep].tolist())]
        # filter -> group_by
        d = df.lazy().filter(pred).group_by("k").agg(c("x").sum().alias("sx"), pl.len().alias("n")).collect(**kw).to_dict()
        assert note in pl.last_plan(), pl.last_plan()
        got = group_rows(d, "k")
        keep = ref & valid
        assert sorted(got) == sorted(set(k[keep].tolist()))
        for kk in got:
            sel = keep & (k == kk)
            assert got[kk] == {"sx": float(x[sel & xm].sum()), "n": int(sel.sum())}, (kw, kk)
        # one scan of a conditional aggregate
        d = df.lazy().select(pl.when(pred).then(c("x")).otherwise(0.0).sum().alias("sx"), pl.when(~pred).then(1).otherwise(0).sum().alias("n_not")).collect(**kw).to_dict()
        assert note in pl.last_plan() and d["sx"] == [float(x[ref & valid & xm].sum())] and d["n_not"] == [int((~ref & valid).sum())], (kw, d)
        if not kw:
            assert "fused_scan" in pl.last_plan(), pl.last_plan()                                  # the conditional aggregate stays one scan
        # the predicate as a group key: true, false and null groups
        d = df.lazy().group_by(pred.alias("p")).agg(pl.len().alias("n"), c("y").sum().alias("sy")).collect(**kw).to_dict()
        got = group_rows(d, "p")
        want = {key: {"n": int(sel.sum()), "sy": int(y[sel].sum())} for key, sel in ((True, ref & valid), (False, ~ref & valid), (None, ~valid)) if sel.any()}
        assert got == want, (kw, got, want)
        # as an output column
        out = df.lazy().with_columns(pred.alias("p")).select("p", "y").collect(**kw)
        check_bool(out["p"], [bool(r) if ok else None for r, ok in zip(ref, valid)], kw)
        assert out["y"].to_numpy().tolist() == y.tolist()
    if device_dict:
        cats = df["s"].dtype.categories
        assert cats._items is None and cats._h                                                     # no query downloaded the dictionary


def test_q14_with_its_real_predicate(pl):
    from polars_amd import queries as Q
    rng = np.random.default_rng(14)
    n, n_parts = 2000, 200
    syll = [a + " " + b + " " + m for a in ("STANDARD", "SMALL", "MEDIUM", "LARGE", "ECONOMY", "PROMO") for b in ("ANODIZED", "BURNISHED", "PLATED") for m in ("TIN", "NICKEL", "BRASS")]
    ptype = [syll[i] for i in rng.integers(0, len(syll), n_parts)]
    pkey = rng.permutation(n_parts).astype(np.int64)
    l_pkey = rng.integers(0, n_parts + 20, n).astype(np.int64)                                      # some parts are unknown
    price, disc = rng.integers(3600, 400_000, n) / 4.0, rng.integers(0, 3, n) / 4.0                  # products and sums exact in f64
    li = pl.DataFrame({"l_partkey": l_pkey, "l_extendedprice": price, "l_discount": disc})
    type_of = {int(kk): t for kk, t in zip(pkey, ptype)}
    lt = [type_of.get(int(v)) for v in l_pkey]
    rev = price * (1 - disc)
    known = np.array([t is not None for t in lt])
    promo = np.array([t is not None and t.startswith("PROMO") for t in lt])
    assert promo.any() and (known & ~promo).any()
    for arrow_type in (pa.string_view(), pa.string()):
        part = pl.DataFrame([pl.Series("p_partkey", pkey), pl.Series.from_arrow("p_type", pa.array(ptype, arrow_type))])
        for kw in ({}, {"no_fusion": True}):
            d = Q.q14_promo(li.lazy(), part.lazy()).collect(**kw).to_dict()
            assert d == {"promo_revenue": [float(rev[promo].sum())], "revenue": [float(rev[known].sum())]}, (kw, d)
            assert "str.starts_with('PROMO')" in pl.last_plan()
            d = Q.q14_promo(li.lazy(), part.lazy(), prefix="NO SUCH TYPE").collect(**kw).to_dict()   # a pattern no category matches: all false, not an error
            assert d == {"promo_revenue": [0.0], "revenue": [float(rev[known].sum())]}, (kw, d)


def test_join_pipelines_with_string_predicates(pl):
    """String predicates on both inputs of a join -> group_by (inner and left: the count / build / probe and the unmatched programs of the fused pipeline) and in front of
    a semi / anti join (the filter program that also tests the membership bitmap), fused and per node, against pandas / numpy."""
    from tests.test_program_eval_cpu import _pandas_join_groupby
    c = pl.col
    rng = np.random.default_rng(99)
    nb, npr = 300, 2000
    bt = [None if rng.random() < 0.1 else TYPES[i] for i in rng.integers(0, len(TYPES), nb)]
    pu = [None if rng.random() < 0.1 else TYPES[i] for i in rng.integers(0, len(TYPES), npr)]
    bk, attr, flag = rng.permutation(600)[:nb].astype(np.int64), rng.integers(0, 4, nb).astype(np.int64), rng.integers(0, 100, nb).astype(np.int64)
    pk, pkm, v = rng.integers(0, 700, npr).astype(np.int64), rng.random(npr) < 0.95, rng.integers(-50, 50, npr).astype(np.int64)
    B = pl.DataFrame([pl.Series("k", bk), pl.Series("attr", attr), pl.Series("flag", flag), pl.Series.from_arrow("t", pa.array(bt, pa.string_view()))])
    P = pl.DataFrame([pl.Series("k", pk, pl.Int64, validity=pkm), pl.Series("v", v), pl.Series.from_arrow("u", pa.array(pu, pa.string()))])
    code = lambda strings: (np.array([TYPES.index(s) if s is not None else 0 for s in strings], dtype=np.int64), np.array([s is not None for s in strings]))
    bcols = {"k": (bk, None), "attr": (attr, None), "flag": (flag, None), "t": code(bt)}
    pcols = {"k": (pk, pkm), "v": (v, None), "u": code(pu)}
    starts = [i for i, s in enumerate(TYPES) if s.startswith("PROMO")]
    has = [i for i, s in enumerate(TYPES) if "PROMO" in s]
    bpred, ppred = (lambda f: f["t"].isin(starts).fillna(False).astype(bool)), (lambda f: f["u"].isin(has).fillna(False).astype(bool))
    aggs = (c("v").sum().alias("s"), pl.len().alias("n"))
    for how in ("inner", "left"):
        want = _pandas_join_groupby(bcols, pcols, how, ["k", "attr"], bpred=bpred, ppred=ppred)
        assert len(want) > 50
        for kw in ({}, {"no_fusion": True}):
            lf = P.lazy().filter(c("u").str.contains("PROMO")).join(B.lazy().filter(c("t").str.starts_with("PROMO")), on="k", how=how).group_by("k", "attr").agg(*aggs)
            d = lf.collect(**kw).to_dict()
            got = {(d["k"][i], d["attr"][i]): {"s": d["s"][i], "n": d["n"][i]} for i in range(len(d["k"]))}
            assert got == want, (how, kw, pl.last_plan())
            assert "str.contains('PROMO')" in pl.last_plan() and "str.starts_with('PROMO')" in pl.last_plan()
    # semi / anti: rows of P that pass the predicate and have (no) partner among the rows of B that pass theirs, in P's order
    bkeys = set(bk[flag < 60].tolist())
    pm = np.array([s is not None and s.endswith("PROMO") for s in pu])
    inb = np.array([ok and int(k) in bkeys for k, ok in zip(pk, pkm)])
    for how, keep in (("semi", pm & inb), ("anti", pm & ~inb)):
        for kw in ({}, {"no_fusion": True}):
            d = P.lazy().filter(c("u").str.ends_with("PROMO")).join(B.lazy().filter(c("flag") < 60), on="k", how=how).select("v").collect(**kw).to_dict()
            assert d["v"] == v[keep].tolist(), (how, kw, pl.last_plan())
