"""Fused join -> group-by with DUPLICATE build keys (engine.cpp fused_join_groupby, multi-value mode of the build table: chains of build rows per key, a group = a build
row, every probe row contributes to each row of its key's chain).  Reference: the build tables map a key to a list of rows (crates/polars-ops/src/frame/join/hash_join/
single_keys.rs:16-167) and the probe emits one pair per entry (single_keys_inner.rs:11-38); the group-by above sees one joined row per pair.  Ground truth here: pandas
merge -> groupby on the host, integer results bit-exact, float sums 1e-6 relative; every query also runs unfused (PLX_PLAN_NO_FUSION: pair list -> gather -> group-by)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
pd = pytest.importorskip("pandas")

HASH_MULT = np.uint64(0x9E3779B97F4A7C15)


def _expected(pkey, pvalid, x, w, bkey, battr, battr_valid, by_attr):
    """inner join on k, then group by (k[, a]) with sum(x), sum(w), len: pandas on the host"""
    P = pd.DataFrame({"k": pkey, "x": x, "w": w})[pvalid]
    B = pd.DataFrame({"k": bkey, "a": pd.array(battr, dtype="Int64")})
    if battr_valid is not None:
        B.loc[~battr_valid, "a"] = pd.NA
    J = P.merge(B, on="k", how="inner")
    keys = ["k", "a"] if by_attr else ["k"]
    g = J.groupby(keys, dropna=False, sort=True).agg(sx=("x", "sum"), sw=("w", "sum"), n=("x", "size")).reset_index()
    return g


def _check(out, exp, by_attr):
    cols = ["k", "a"] if by_attr else ["k"]
    got = pd.DataFrame({c: pd.array(out[c].to_list(), dtype="Int64") for c in cols} | {"sx": out["sx"].to_numpy(), "sw": out["sw"].to_numpy(), "n": out["n"].to_numpy().astype(np.int64)})
    got = got.sort_values(cols, na_position="last").reset_index(drop=True)
    exp = exp.sort_values(cols, na_position="last").reset_index(drop=True)
    assert len(got) == len(exp), (len(got), len(exp))
    for c in cols:
        assert got[c].isna().tolist() == exp[c].isna().tolist() and got[c].dropna().astype(np.int64).tolist() == exp[c].dropna().astype(np.int64).tolist(), c
    assert got["sx"].astype(np.int64).tolist() == exp["sx"].astype(np.int64).tolist()
    assert got["n"].tolist() == exp["n"].astype(np.int64).tolist()
    assert np.allclose(got["sw"].to_numpy(), exp["sw"].to_numpy(), rtol=1e-6, atol=0)


def _frames(pl, rng, n, n_keys, hashed, null_attr=False, same_attr=False, dense=False):
    """build side: every key 1..8 times (dbgen partsupp has 4 rows per part); probe side: keys uniform over [0, 2 * n_keys) (half of them match nothing), 3 % null"""
    reps = rng.integers(1, 9, n_keys)
    ids = np.repeat(np.arange(n_keys, dtype=np.int64), reps)
    rng.shuffle(ids)
    nb = len(ids)
    # the attribute: a per-row value (so (k, a) is unique per build row) or -- same_attr -- one of TWO values per key: duplicate build rows that are ONE group
    battr = rng.integers(0, 2, nb).astype(np.int64) if same_attr else np.arange(nb, dtype=np.int64) * 7 + 3
    battr_valid = (rng.random(nb) > 0.2) if null_attr else None
    enc = (lambda a: (a.astype(np.uint64) * HASH_MULT).astype(np.int64)) if hashed else ((lambda a: a * 3 + 17) if not dense else (lambda a: a + 5))
    pid = rng.integers(0, 2 * n_keys, n).astype(np.int64)
    pvalid = rng.random(n) > 0.03
    x = rng.integers(-100, 100, n).astype(np.int64)
    w = rng.normal(size=n)
    bkey, pkey = enc(ids), enc(pid)
    B = pl.DataFrame([pl.Series("k", bkey), pl.Series("a", battr, validity=battr_valid) if battr_valid is not None else pl.Series("a", battr)])
    P = pl.DataFrame([pl.Series("k", pkey, validity=pvalid), pl.Series("x", x), pl.Series("w", w)])
    return B, P, (pkey, pvalid, x, w, bkey, battr, battr_valid)


def _query(pl, P, B, by_attr, **kw):
    c = pl.col
    keys = ("k", "a") if by_attr else ("k",)
    return P.lazy().join(B.lazy(), on="k").group_by(*keys).agg(c("x").sum().alias("sx"), c("w").sum().alias("sw"), pl.len().alias("n")).collect(**kw)


@pytest.mark.parametrize("hashed,by_attr", [(True, True), (False, True), (True, False)])
def test_duplicate_build_keys_take_the_fused_multi_value_path(pl, hashed, by_attr):
    rng = np.random.default_rng(41 + 2 * hashed + by_attr)
    n, n_keys = (1 << 22) + 4321, 150_000
    B, P, host = _frames(pl, rng, n, n_keys, hashed)
    out = _query(pl, P, B, by_attr)
    plan = pl.last_plan()
    assert "FusedJoinGroupBy{" in plan and "multi-value (row chains" in plan, plan
    _check(out, _expected(*host, by_attr), by_attr)
    ref = _query(pl, P, B, by_attr, no_fusion=True)
    assert "FusedJoinGroupBy" not in pl.last_plan()
    _check(ref, _expected(*host, by_attr), by_attr)


def test_duplicate_keys_found_by_the_direct_address_build_fall_through_to_the_chains(pl):
    """A dense build key range takes the bitmap build first; two pairs on one bit = duplicate keys -> the hash-table pipeline in multi-value mode (no second detection pass)."""
    rng = np.random.default_rng(5)
    B, P, host = _frames(pl, rng, (1 << 22) + 99, 120_000, hashed=False, dense=True)
    out = _query(pl, P, B, True)
    plan = pl.last_plan()
    assert "multi-value (row chains" in plan and "direct-address" not in plan, plan
    _check(out, _expected(*host, True), True)


def test_duplicate_rows_that_are_one_group_share_their_cells(pl):
    """Build rows of one key that agree on the build-side group column are ONE group of the reference's group-by (each probe row counted once per build row): the chain's
    representative rows (canonicalise_chains) collect them -- with and without nulls in that column (null == null for grouping)."""
    for seed, null_attr in ((11, False), (12, True)):
        rng = np.random.default_rng(seed)
        B, P, host = _frames(pl, rng, (1 << 22) + 7, 90_000, hashed=True, null_attr=null_attr, same_attr=True)
        out = _query(pl, P, B, True)
        assert "multi-value (row chains" in pl.last_plan(), pl.last_plan()
        _check(out, _expected(*host, True), True)


def test_multi_value_path_through_the_partitioned_probe_and_edge_keys(pl, monkeypatch):
    """The partitioned hash probe in front of the chains (forced), build keys that include the EMPTY pattern (-1: all ones) and 0, each several times."""
    rng = np.random.default_rng(77)
    n, n_keys = (1 << 22) + 1001, 60_000
    B, P, host = _frames(pl, rng, n, n_keys, hashed=True)
    pkey, pvalid, x, w, bkey, battr, bvalid = host
    special = np.array([-1, -1, -1, 0, 0, np.iinfo(np.int64).min, np.iinfo(np.int64).min], dtype=np.int64)
    bkey = np.concatenate([bkey, special]); battr = np.concatenate([battr, np.arange(len(special), dtype=np.int64) + 10 ** 12])
    pkey = pkey.copy(); pkey[:3000] = rng.choice(special, 3000)
    B = pl.DataFrame({"k": bkey, "a": battr})
    P = pl.DataFrame([pl.Series("k", pkey, validity=pvalid), pl.Series("x", x), pl.Series("w", w)])
    monkeypatch.setenv("PLX_PROBE_PARTITIONED", "2")
    out = _query(pl, P, B, True)
    plan = pl.last_plan()
    assert "multi-value (row chains" in plan and "partitioned_hash_probe(" in plan, plan
    _check(out, _expected(pkey, pvalid, x, w, bkey, battr, None, True), True)


def test_float_build_group_column_with_duplicate_keys_runs_unfused(pl):
    """A float build-side group column cannot be compared bitwise (-0.0 == 0.0, NaN == NaN for grouping): duplicate keys then leave the fused path, same answer."""
    rng = np.random.default_rng(3)
    nb, n = 50_000, 400_000
    bkey = rng.integers(0, 20_000, nb).astype(np.int64)
    a = rng.choice(np.array([0.0, 1.5, 2.5]), nb)
    pkey = rng.integers(0, 40_000, n).astype(np.int64)
    x = rng.integers(0, 10, n).astype(np.int64)
    B = pl.DataFrame({"k": bkey, "a": a}); P = pl.DataFrame({"k": pkey, "x": x})
    out = P.lazy().join(B.lazy(), on="k").group_by("k", "a").agg(pl.col("x").sum().alias("sx"), pl.len().alias("n")).collect()
    assert "FusedJoinGroupBy" not in pl.last_plan()
    J = pd.DataFrame({"k": pkey, "x": x}).merge(pd.DataFrame({"k": bkey, "a": a}), on="k")
    g = J.groupby(["k", "a"]).agg(sx=("x", "sum"), n=("x", "size")).reset_index().sort_values(["k", "a"])
    got = pd.DataFrame({"k": out["k"].to_numpy(), "a": out["a"].to_numpy(), "sx": out["sx"].to_numpy(), "n": out["n"].to_numpy().astype(np.int64)}).sort_values(["k", "a"])
    assert got["k"].tolist() == g["k"].tolist() and got["a"].tolist() == g["a"].tolist() and got["sx"].tolist() == g["sx"].tolist() and got["n"].tolist() == g["n"].tolist()


# ---- LEFT joins on the fused path (single_keys_left.rs:106-195): matched rows as the inner join, unmatched rows grouped by their own key with nulls in the build columns ----
def _expected_left(pkey, pvalid, x, w, bkey, battr, battr_valid, by_attr):
    inner = _expected(pkey, pvalid, x, w, bkey, battr, battr_valid, by_attr)
    P = pd.DataFrame({"k": pd.array(pkey, dtype="Int64"), "x": x, "w": w})
    P.loc[~pvalid, "k"] = pd.NA
    un = P[~(pvalid & np.isin(pkey, bkey))]                       # no build row with this key (a null key matches nothing)
    g = un.groupby("k", dropna=False, sort=True).agg(sx=("x", "sum"), sw=("w", "sum"), n=("x", "size")).reset_index()
    if by_attr:
        g.insert(1, "a", pd.array([pd.NA] * len(g), dtype="Int64"))
        inner["a"] = inner["a"].astype("Int64")
    inner["k"] = inner["k"].astype("Int64")
    if not by_attr:
        # grouped by the key alone, a key's matched and unmatched rows cannot both exist: the two parts never share a group
        pass
    return pd.concat([inner, g], ignore_index=True)


def _query_left(pl, P, B, by_attr, **kw):
    c = pl.col
    keys = ("k", "a") if by_attr else ("k",)
    return P.lazy().join(B.lazy(), on="k", how="left").group_by(*keys).agg(c("x").sum().alias("sx"), c("w").sum().alias("sw"), pl.len().alias("n")).collect(**kw)


@pytest.mark.parametrize("dups,by_attr", [(False, True), (True, True), (True, False)])
def test_left_join_group_by_takes_the_fused_path(pl, dups, by_attr):
    """LEFT JOIN -> group_by on the fused pipeline: unique and duplicate build keys, null probe keys (their own group, null key), probe keys beyond the build range."""
    rng = np.random.default_rng(301 + 2 * dups + by_attr)
    n, n_keys = (1 << 22) + 999, 120_000
    B, P, host = _frames(pl, rng, n, n_keys, hashed=False, dense=True)
    pkey, pvalid, x, w, bkey, battr, bvalid = host
    if not dups:      # one row per key
        bkey, first = np.unique(bkey, return_index=True)
        battr = battr[first]
        B = pl.DataFrame({"k": bkey, "a": battr})
    out = _query_left(pl, P, B, by_attr)
    plan = pl.last_plan()
    assert "FusedJoinGroupBy{" in plan and "LeftJoinUnmatched{" in plan and ("multi-value" in plan) == dups, plan
    exp = _expected_left(pkey, pvalid, x, w, bkey, battr, None, by_attr)
    _check(out, exp, by_attr)
    ref = _query_left(pl, P, B, by_attr, no_fusion=True)
    assert "FusedJoinGroupBy" not in pl.last_plan()
    _check(ref, exp, by_attr)


def test_left_join_with_predicates_on_both_sides_and_every_row_unmatched(pl):
    """Predicates below a left join: the left one filters rows, the right one only decides which rows MATCH (a left row whose partners all fail it is unmatched, not dropped);
    and a build side that keeps no row at all: every left row is unmatched."""
    rng = np.random.default_rng(77)
    n, nb = (1 << 22) + 5, 200_000
    bkey = rng.permutation(nb).astype(np.int64)
    battr = rng.integers(0, 1000, nb).astype(np.int64)
    pkey = rng.integers(0, nb + 50_000, n).astype(np.int64)
    x = rng.integers(-9, 9, n).astype(np.int64)
    w = rng.random(n)
    B = pl.DataFrame({"k": bkey, "a": battr}); P = pl.DataFrame({"k": pkey, "x": x, "w": w})
    c = pl.col
    for cut in (500, -1):
        q = (P.lazy().filter(c("x") > -5).join(B.lazy().filter(c("a") < cut), on="k", how="left").group_by("k", "a")
             .agg(c("x").sum().alias("sx"), c("w").sum().alias("sw"), pl.len().alias("n")))
        out = q.collect()
        assert "LeftJoinUnmatched{" in pl.last_plan(), pl.last_plan()
        keep = x > -5
        bk = battr < cut
        exp = _expected_left(pkey[keep], np.ones(int(keep.sum()), bool), x[keep], w[keep], bkey[bk], battr[bk], None, True)
        _check(out, exp, True)


# ---- the stages of the driver (plan_join_groupby ... unmatched_left_groups) at the shapes the cases above leave out: small sides (2^16 + 3 probe rows: no multiple of the
# 128-row tile; 1000 build keys), nested filter joins on either side, result sets without a group ----
N_SMALL, KEYS_SMALL = (1 << 16) + 3, 1000


def _filter_side(pl, rng, name, n_keys, cut=70):
    """a nested join's filter side: unique keys 0..n_keys-1 in no order, a predicate column; -> (frame, the keys that pass `f < cut`)"""
    keys = rng.permutation(n_keys).astype(np.int64)
    f = rng.integers(0, 100, n_keys).astype(np.int64)
    return pl.DataFrame({name: keys, "f_" + name: f}), keys[f < cut]


def test_left_join_group_by_with_a_nested_filter_join_on_each_side(pl):
    """(P join FP) LEFT JOIN (B join FB) -> group_by: the filter on the left DROPS left rows, the one on the right only decides which build rows can match.  Three programs
    number their lookup bitmaps differently here: build (FB = 0), probe (FP = 1), and the unmatched rows' own (FP = 0, the build keys' membership bitmap = 1)."""
    rng = np.random.default_rng(611)
    B, P, host = _frames(pl, rng, N_SMALL, KEYS_SMALL, hashed=False, dense=True)
    pkey, pvalid, x, w, bkey, battr, _ = host
    bkey, first = np.unique(bkey, return_index=True)      # one row per key
    battr = battr[first]
    bf = rng.integers(0, 400, len(bkey)).astype(np.int64)
    pf = rng.integers(0, 600, N_SMALL).astype(np.int64)   # a third of them beyond FP's keys
    FB, fb_keys = _filter_side(pl, rng, "bf", 400)
    FP, fp_keys = _filter_side(pl, rng, "pf", 500)
    B = pl.DataFrame({"k": bkey, "a": battr, "bf": bf})
    P = pl.DataFrame([pl.Series("k", pkey, validity=pvalid), pl.Series("x", x), pl.Series("w", w), pl.Series("pf", pf)])
    c = pl.col
    q = (P.lazy().join(FP.lazy().filter(c("f_pf") < 70), on="pf").join(B.lazy().join(FB.lazy().filter(c("f_bf") < 70), on="bf"), on="k", how="left")
         .group_by("k", "a").agg(c("x").sum().alias("sx"), c("w").sum().alias("sw"), pl.len().alias("n")))
    keep, bk = np.isin(pf, fp_keys), np.isin(bf, fb_keys)
    exp = _expected_left(pkey[keep], pvalid[keep], x[keep], w[keep], bkey[bk], battr[bk], None, True)
    out = q.collect()
    plan = pl.last_plan()
    assert plan.count("SemiFilter{") == 2 and "FusedJoinGroupBy{" in plan and "LeftJoinUnmatched{" in plan, plan
    _check(out, exp, True)
    ref = q.collect(no_fusion=True)
    assert "FusedJoinGroupBy" not in pl.last_plan() and "SemiFilter" not in pl.last_plan()
    _check(ref, exp, True)


def test_left_join_whose_every_left_row_has_a_partner_appends_no_group(pl):
    """The unmatched rows' group-by finds no group: nothing is appended, the height is the matched groups'.  The same frames with a few keys beyond the build side: groups."""
    rng = np.random.default_rng(612)
    bkey = (rng.permutation(KEYS_SMALL) + 5).astype(np.int64)
    battr = np.arange(KEYS_SMALL, dtype=np.int64) * 7 + 3
    x = rng.integers(-100, 100, N_SMALL).astype(np.int64)
    w = rng.normal(size=N_SMALL)
    B = pl.DataFrame({"k": bkey, "a": battr})
    every = np.ones(N_SMALL, bool)
    for beyond, tail_groups in ((0, 0), (40, 40)):
        pkey = rng.integers(5, KEYS_SMALL + 5, N_SMALL).astype(np.int64)
        pkey[:KEYS_SMALL + beyond] = np.arange(5, KEYS_SMALL + 5 + beyond)      # every build key, and `beyond` keys past them
        P = pl.DataFrame({"k": pkey, "x": x, "w": w})
        out = _query_left(pl, P, B, True)
        plan = pl.last_plan()
        assert "FusedJoinGroupBy{" in plan and "LeftJoinUnmatched{" in plan, plan
        assert ("groups=%d}}" % tail_groups) in plan[plan.index("LeftJoinUnmatched{"):], plan
        assert out.height == KEYS_SMALL + tail_groups
        exp = _expected_left(pkey, every, x, w, bkey, battr, None, True)
        _check(out, exp, True)
        _check(_query_left(pl, P, B, True, no_fusion=True), exp, True)


@pytest.mark.parametrize("hashed", [False, True])
def test_inner_join_group_by_without_a_matching_row_is_empty(pl, hashed):
    """No probe key is among the build keys, on the direct-address table and (hashed keys) on the hash table: no group, and the columns are still those of the query."""
    rng = np.random.default_rng(613 + hashed)
    B, P, host = _frames(pl, rng, N_SMALL, KEYS_SMALL, hashed=hashed, dense=True)
    pkey, pvalid, x, w, bkey, battr, _ = host
    bkey, first = np.unique(bkey, return_index=True)
    battr = battr[first]
    n = 30_001
    pkey = pkey[~np.isin(pkey, bkey)][:n]      # (half the probe keys of _frames match nothing: those)
    assert len(pkey) == n
    B = pl.DataFrame({"k": bkey, "a": battr})
    P = pl.DataFrame([pl.Series("k", pkey, validity=pvalid[:n]), pl.Series("x", x[:n]), pl.Series("w", w[:n])])
    out = _query(pl, P, B, True)
    plan = pl.last_plan()
    assert "FusedJoinGroupBy{" in plan and "groups=0}" in plan and ("hash table" if hashed else "direct-address table") in plan, plan
    ref = _query(pl, P, B, True, no_fusion=True)
    assert "FusedJoinGroupBy" not in pl.last_plan()
    assert out.height == 0 and ref.height == 0 and out.columns == ["k", "a", "sx", "sw", "n"] and out.schema == ref.schema, (out.schema, ref.schema)
    exp = _expected(pkey, pvalid[:n], x[:n], w[:n], bkey, battr, None, True)
    assert len(exp) == 0
    _check(out, exp, True)


def test_duplicate_build_keys_behind_a_nested_filter_join_through_the_partitioned_probe(pl, monkeypatch):
    """Chains of build rows, a build-side nested filter join (its bitmap is tested by the count and build scans) and the partitioned hash probe (forced) in one query."""
    rng = np.random.default_rng(614)
    n = (1 << 22) + 5
    B, P, host = _frames(pl, rng, n, KEYS_SMALL, hashed=True)
    pkey, pvalid, x, w, bkey, battr, _ = host
    bf = rng.integers(0, 400, len(bkey)).astype(np.int64)
    FB, fb_keys = _filter_side(pl, rng, "bf", 400)
    B = pl.DataFrame({"k": bkey, "a": battr, "bf": bf})
    c = pl.col
    q = (P.lazy().join(B.lazy().join(FB.lazy().filter(c("f_bf") < 70), on="bf"), on="k")
         .group_by("k", "a").agg(c("x").sum().alias("sx"), c("w").sum().alias("sw"), pl.len().alias("n")))
    bk = np.isin(bf, fb_keys)
    exp = _expected(pkey, pvalid, x, w, bkey[bk], battr[bk], None, True)
    monkeypatch.setenv("PLX_PROBE_PARTITIONED", "2")
    out = q.collect()
    plan = pl.last_plan()
    assert "SemiFilter{bf -> bitmap" in plan and "multi-value (row chains" in plan and "partitioned_hash_probe(" in plan, plan
    _check(out, exp, True)
    _check(q.collect(no_fusion=True), exp, True)
