"""Joins on multi-column keys of any width (kernels_join_wide.hip, join::join_indices_wide): key parts that do not pack into one Int64 -- Float32 / Float64 / UInt64
parts, full-range Int64 parts -- are joined through a table of row ids whose key words are compared column by column.  Ground truth: the CPU oracle on row-encoded
keys (orc.encode_key_rows: one id per distinct key tuple, floats canonicalised like the kernels do; then orc.join / orc.semi_anti_join on the ids), the scheme of
tests/test_gpu_sort.py::test_multi_key_join_matches_row_encoded_oracle.  Both frames carry a row number (lrow, rrow).  Without a requested order the pair SETS are
compared, with one the output is compared UNSORTED (left_right / right_left row for row against np.lexsort; left / right: a monotone primary plus the same set).
Every test asserts the route through pl.last_plan()."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NL, NR = 40_000, 9_000
NO_RIGHT = np.int64(1) << 40            # stands for "no right row": one pair per unmatched left row, so it never ties
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max


# ---------------------------------------------------------------------------------------------------------------- helpers ---
def _series(pl, name, values, valid=None):
    return pl.Series(name, values, validity=valid) if valid is not None else pl.Series(name, values)


def _frames(pl, names, lcols, rcols, rnames=None):
    """lcols / rcols = [(values, valid or None)] per key column"""
    nl, nr = len(lcols[0][0]), len(rcols[0][0])
    L = pl.DataFrame([_series(pl, n, v, m) for n, (v, m) in zip(names, lcols)] + [pl.Series("lrow", np.arange(nl, dtype=np.int64))])
    R = pl.DataFrame([_series(pl, n, v, m) for n, (v, m) in zip(rnames or names, rcols)] + [pl.Series("rrow", np.arange(nr, dtype=np.int64))])
    return L, R


def _oracle_cols(cols):
    return [((v.astype(np.uint8) if v.dtype == np.bool_ else v), m) for v, m in cols]


class Ref:
    """the oracle's answers for one pair of key column lists, computed once"""

    def __init__(self, orc, lcols, rcols):
        self.orc = orc
        self.nl = len(lcols[0][0])
        self.lk, self.lv, self.rk, self.rv = orc.encode_key_rows(_oracle_cols(lcols), _oracle_cols(rcols))
        self._pairs = {}

    def pairs(self, how):
        """(lrow, rrow or NO_RIGHT, rvalid), in no particular order"""
        if how not in self._pairs:
            li, ri, rvalid = self.orc.join(self.orc.JOIN_LEFT if how == "left" else self.orc.JOIN_INNER, self.lk, self.lv, self.rk, self.rv)
            if rvalid is None:
                rvalid = np.ones(len(li), bool)
            self._pairs[how] = (li.astype(np.int64), np.where(rvalid, ri.astype(np.int64), NO_RIGHT), rvalid)
        return self._pairs[how]

    def kept(self, how):
        return self.orc.semi_anti_join(self.orc.JOIN_SEMI if how == "semi" else self.orc.JOIN_ANTI, self.lk, self.lv, self.rk, self.rv).astype(np.int64)


def _got(out):
    lrow = out["lrow"].to_numpy().astype(np.int64)
    rrow, rv = out["rrow"]._download()
    rv = rv if rv is not None else np.ones(out.height, bool)
    return lrow, np.where(rv, rrow.astype(np.int64), NO_RIGHT), rv


def _check_pairs(out, ref_pairs, order="none"):
    lrow, rrow, rvalid = ref_pairs
    g_l, g_r, g_v = _got(out)
    assert len(g_l) == len(lrow), (len(g_l), len(lrow))
    if order in ("left_right", "right_left"):
        o = np.lexsort((rrow, lrow)) if order == "left_right" else np.lexsort((lrow, rrow))
        assert np.array_equal(g_l, lrow[o]) and np.array_equal(g_r, rrow[o]) and np.array_equal(g_v, rvalid[o]), order
        return
    if order == "left":
        assert np.all(np.diff(g_l) >= 0), "left row numbers are not non-decreasing"
    if order == "right":
        assert np.all(np.diff(g_r) >= 0), "right row numbers are not non-decreasing"
    og, ow = np.lexsort((g_r, g_l)), np.lexsort((rrow, lrow))
    assert np.array_equal(g_l[og], lrow[ow]) and np.array_equal(g_r[og], rrow[ow]) and np.array_equal(g_v[og], rvalid[ow]), order


def _wide_plan(pl, how="inner"):
    plan = pl.last_plan()
    name = {"semi": "wide_hash_semi_join[", "anti": "wide_hash_anti_join["}.get(how, "wide_hash_join[")
    assert "wide_hash_" in plan and name in plan and "packed" not in plan, plan
    return plan


def _join_and_check(pl, L, R, ref, how, on, order="none", **kw):
    out = L.lazy().join(R.lazy(), how=how, maintain_order=order, **on).collect(**kw)
    plan = _wide_plan(pl, how)
    if how in ("semi", "anti"):
        assert np.array_equal(out["lrow"].to_numpy().astype(np.int64), ref.kept(how)), how
    else:
        _check_pairs(out, ref.pairs(how), order)
    return out, plan


def _orders_for(how):
    return ("none", "left", "right", "left_right", "right_left") if how == "inner" else ("none", "left", "left_right")


# ------------------------------------------------------------------------------------------------------------ mixed dtypes ---
@pytest.fixture(scope="module")
def mixed(orc):
    """(Int64, UInt64, Float64, Boolean) keys: full-range integers with the all-ones / zero / extreme patterns, NaNs of both signs, zeros of both signs, infinities"""
    rng = np.random.default_rng(7)
    a_pool = np.concatenate([np.array([-1, 0, I64_MIN, I64_MAX], np.int64), rng.integers(I64_MIN, I64_MAX, 26, dtype=np.int64, endpoint=True)])
    u_pool = np.concatenate([np.array([0, 2**64 - 1, 2**63], np.uint64), rng.integers(0, 2**64 - 1, 5, dtype=np.uint64, endpoint=True)])
    neg_nan = np.array([0xFFF8000000000001], np.uint64).view(np.float64)[0]
    f_pool = np.concatenate([np.array([np.nan, neg_nan, 0.0, -0.0, np.inf, -np.inf]), rng.normal(size=6) * 1e3])
    assert len(a_pool) == 30 and len(u_pool) == 8 and len(f_pool) == 12 and np.signbit(neg_nan) and np.isnan(neg_nan)

    def side(n):
        return [a_pool[rng.integers(0, 30, n)], u_pool[rng.integers(0, 8, n)], f_pool[rng.integers(0, 12, n)], rng.integers(0, 2, n).astype(bool)]
    l, r = side(NL), side(NR)
    lam, rfm = rng.random(NL) < 0.97, rng.random(NR) < 0.9
    lcols = [(l[0], lam), (l[1], None), (l[2], None), (l[3], None)]
    rcols = [(r[0], None), (r[1], None), (r[2], rfm), (r[3], None)]
    return dict(names=["a", "u", "f", "c"], lcols=lcols, rcols=rcols, ref=Ref(orc, lcols, rcols))


def _mixed_case(pl, m, how):
    L, R = _frames(pl, m["names"], m["lcols"], m["rcols"])
    out, plan = _join_and_check(pl, L, R, m["ref"], how, dict(on=m["names"]))
    assert "words=4 (key part 0 spans more than 63 bits)" in plan, plan
    if how in ("semi", "anti"):
        assert out.columns == ["a", "u", "f", "c", "lrow"] and out.height > 1000
        return
    assert out.columns == ["a", "u", "f", "c", "lrow", "rrow"]
    if how == "inner":
        assert out.height > 10_000
        assert "dup-keys" in plan, plan
        g_l, g_r, _ = _got(out)
        lf, rf = m["lcols"][2][0][g_l], m["rcols"][2][0][g_r]
        assert np.any(np.isnan(lf) & np.isnan(rf)), "no matched pair with NaN on both sides"
        assert np.any(np.isnan(lf) & np.isnan(rf) & (np.signbit(lf) != np.signbit(rf))), "no NaN pair of different bit patterns"
        assert np.any((lf == 0) & (rf == 0) & (np.signbit(lf) != np.signbit(rf))), "no matched pair of zeros of opposite sign"
    else:
        assert out.height >= NL


@pytest.mark.parametrize("how", ["inner", "left", "semi", "anti"])
def test_mixed_dtypes(pl, mixed, how):
    _mixed_case(pl, mixed, how)


# ------------------------------------------------------------------------------------------------- two full-range Int64 parts ---
@pytest.fixture(scope="module")
def two_i64(orc):
    """pools of 100 x 100 full-range values; unique build side: 6 000 distinct pairs; dup build side: about three rows per key"""
    rng = np.random.default_rng(8)
    pa = rng.integers(I64_MIN, I64_MAX, 100, dtype=np.int64, endpoint=True)
    pb = rng.integers(I64_MIN, I64_MAX, 100, dtype=np.int64, endpoint=True)
    assert len(np.unique(pa)) == 100 and len(np.unique(pb)) == 100
    lt = rng.integers(0, 10_000, NL)
    ut = rng.permutation(10_000)[:6_000]
    dt = rng.integers(0, 3_000, NR)

    def cols(t):
        return [(pa[t // 100], None), (pb[t % 100], None)]
    return dict(l=cols(lt), uniq=cols(ut), dup=cols(dt), ref_uniq=Ref(orc, cols(lt), cols(ut)), ref_dup=Ref(orc, cols(lt), cols(dt)),
                ref_swapped=Ref(orc, cols(dt), cols(lt)), matched=int(np.isin(lt, ut).sum()))


@pytest.mark.parametrize("how", ["inner", "left"])
def test_two_full_range_int64_columns_unique_build_keys(pl, two_i64, how):
    t = two_i64
    L, R = _frames(pl, ["a", "b"], t["l"], t["uniq"])
    out, plan = _join_and_check(pl, L, R, t["ref_uniq"], how, dict(on=["a", "b"]))
    assert "unique-keys" in plan and "build=right rows=6000" in plan and "words=2" in plan, plan
    assert "key spans do not pack" in plan or "spans more than 63 bits" in plan, plan
    assert 20_000 < t["matched"] < 28_000
    assert out.height == (t["matched"] if how == "inner" else NL)


@pytest.mark.parametrize("how,order", [(h, o) for h in ("inner", "left") for o in _orders_for(h)])
def test_every_order_over_a_duplicate_key_build_side(pl, two_i64, how, order):
    t = two_i64
    L, R = _frames(pl, ["a", "b"], t["l"], t["dup"])
    out, plan = _join_and_check(pl, L, R, t["ref_dup"], how, dict(on=["a", "b"]), order)
    assert "dup-keys" in plan and ("order=" in plan) == (order != "none") and (order == "none" or f"order={order}: " in plan), plan
    assert out.height > 20_000


@pytest.mark.parametrize("order", ["left", "right"])
def test_smaller_left_side_is_the_build_side(pl, two_i64, order):
    t = two_i64
    L, R = _frames(pl, ["a", "b"], t["dup"], t["l"])                  # 9 000 x 40 000
    out, plan = _join_and_check(pl, L, R, t["ref_swapped"], "inner", dict(on=["a", "b"]), order)
    assert "build=left rows=9000" in plan and f"order={order}: " in plan, plan
    assert out.height > 20_000


# ------------------------------------------------------------------------------------------ keys that differ in one part only ---
@pytest.fixture(scope="module")
def one_part(orc):
    """three full-range Int64 parts from pools of 4 values: the build side holds the 32 tuples of even index, the probe side draws from all 64.  `last`: the tuple index
    runs fastest in the LAST column (keys equal in the first two parts, different in the last); `first`: fastest in the FIRST column."""
    rng = np.random.default_rng(9)
    pools = [rng.integers(I64_MIN, I64_MAX, 4, dtype=np.int64, endpoint=True) for _ in range(3)]
    assert all(len(np.unique(p)) == 4 for p in pools)
    bt = np.concatenate([np.arange(0, 64, 2), rng.integers(0, 32, 968) * 2])          # each even tuple at least once
    rng.shuffle(bt)
    pt = rng.integers(0, 64, 20_000)
    out = {}
    for variant in ("last", "first"):
        def cols(t):
            digits = [t // 16, (t // 4) % 4, t % 4]
            if variant == "first":
                digits = digits[::-1]
            return [(pools[j][digits[j]], None) for j in range(3)]
        out[variant] = dict(l=cols(pt), r=cols(bt), ref=Ref(orc, cols(pt), cols(bt)), matched=int((pt % 2 == 0).sum()))
    return out


def _one_part_case(pl, one_part, variant):
    c = one_part[variant]
    L, R = _frames(pl, ["a", "b", "c"], c["l"], c["r"])
    for how in ("inner", "anti"):
        out, plan = _join_and_check(pl, L, R, c["ref"], how, dict(on=["a", "b", "c"]))
        assert "words=3" in plan, plan
        if how == "anti":
            assert out.height == 20_000 - c["matched"] and out.height > 5_000
        else:
            assert out.height > 100_000                                                # about 31 build rows per matched probe row


@pytest.mark.parametrize("variant", ["last", "first"])
def test_keys_that_differ_in_one_part_only(pl, one_part, variant):
    _one_part_case(pl, one_part, variant)


# --------------------------------------------------------------------------------------------------------------- tag hook ---
@pytest.mark.parametrize("bits", ["0", "2"])
def test_tag_bits_hook_forces_the_word_compare(pl, mixed, one_part, monkeypatch, bits):
    """PLX_JOIN_WIDE_TAG_BITS: with 0 tag bits every occupied slot a walk passes is a tag match, so "same tag, different key" is decided by the word compare alone"""
    monkeypatch.setenv("PLX_JOIN_WIDE_TAG_BITS", bits)
    _mixed_case(pl, mixed, "inner")
    _mixed_case(pl, mixed, "anti")
    _one_part_case(pl, one_part, "last")
    _one_part_case(pl, one_part, "first")


# ----------------------------------------------------------------------------------------------------------- wide == packed ---
def test_wide_route_equals_packed_route_on_keys_that_pack(pl, orc, monkeypatch):
    """(Int32, Int64, Boolean) keys with nulls: the input of the packed-key test of tests/test_gpu_sort.py, rebuilt here"""
    rng = np.random.default_rng(21)
    la, ra = rng.integers(-50, 50, NL).astype(np.int32), rng.integers(-60, 40, NR).astype(np.int32)
    lb, rb = rng.integers(0, 300, NL).astype(np.int64) * 1_000_003, rng.integers(0, 300, NR).astype(np.int64) * 1_000_003
    lc, rc = rng.integers(0, 2, NL).astype(bool), rng.integers(0, 2, NR).astype(bool)
    lam, rbm = rng.random(NL) < 0.97, rng.random(NR) < 0.9
    lcols, rcols = [(la, lam), (lb, None), (lc, None)], [(ra, None), (rb, rbm), (rc, None)]
    L, R = _frames(pl, ["a", "b", "c"], lcols, rcols)
    ref = Ref(orc, lcols, rcols)
    for how in ("inner", "left"):
        monkeypatch.setenv("PLX_JOIN_WIDE_KEYS", "2")
        wide = L.join(R, on=["a", "b", "c"], how=how)
        plan = _wide_plan(pl)
        assert "PLX_JOIN_WIDE_KEYS=2" in plan and "words=3" in plan, plan
        monkeypatch.delenv("PLX_JOIN_WIDE_KEYS")
        packed = L.join(R, on=["a", "b", "c"], how=how)
        assert "packed 3 key columns" in pl.last_plan() and "wide_hash_" not in pl.last_plan(), pl.last_plan()
        _check_pairs(wide, ref.pairs(how))
        _check_pairs(packed, ref.pairs(how))
        w, p = _got(wide), _got(packed)
        ow, op = np.lexsort((w[1], w[0])), np.lexsort((p[1], p[0]))
        assert all(np.array_equal(x[ow], y[op]) for x, y in zip(w, p))
        assert wide.columns == packed.columns == ["a", "b", "c", "lrow", "rrow"] and wide.height > 1000
    for how in ("semi", "anti"):
        monkeypatch.setenv("PLX_JOIN_WIDE_KEYS", "2")
        wide = L.join(R, on=["a", "b", "c"], how=how)
        _wide_plan(pl, how)
        monkeypatch.delenv("PLX_JOIN_WIDE_KEYS")
        packed = L.join(R, on=["a", "b", "c"], how=how)
        assert "packed 3 key columns" in pl.last_plan(), pl.last_plan()
        assert np.array_equal(wide["lrow"].to_numpy(), ref.kept(how)) and np.array_equal(packed["lrow"].to_numpy(), ref.kept(how))


# ---------------------------------------------------------------------------------------------------- narrow and float parts ---
@pytest.mark.parametrize("how", ["inner", "left", "semi", "anti"])
def test_narrow_and_float32_parts(pl, orc, how):
    """(Int8, Float32, UInt16) with nulls on both sides: narrow parts are sign- / zero-extended, Float32 is canonicalised through its widening to double"""
    rng = np.random.default_rng(11)
    neg_nan32 = np.array([0xFFC00001], np.uint32).view(np.float32)[0]
    f_pool = np.array([np.nan, neg_nan32, 0.0, -0.0, np.inf, -np.inf, 1.5, -2.25, 3.0e38, 1.0e-40], np.float32)      # the last one is a denormal
    a_pool = np.array([-128, -1, 0, 1, 127, 5, -77], np.int8)
    u_pool = np.array([0, 1, 255, 256, 32768, 65535], np.uint16)

    def side(n):
        return a_pool[rng.integers(0, len(a_pool), n)], f_pool[rng.integers(0, len(f_pool), n)], u_pool[rng.integers(0, len(u_pool), n)]
    l, r = side(NL), side(NR)
    lcols = [(l[0], rng.random(NL) < 0.95), (l[1], rng.random(NL) < 0.95), (l[2], None)]
    rcols = [(r[0], None), (r[1], rng.random(NR) < 0.9), (r[2], rng.random(NR) < 0.9)]
    L, R = _frames(pl, ["a", "f", "u"], lcols, rcols)
    out, plan = _join_and_check(pl, L, R, Ref(orc, lcols, rcols), how, dict(on=["a", "f", "u"]))
    assert "Float32 key part" in plan and "words=3" in plan, plan
    assert out.height > 1000


# --------------------------------------------------------------------------------------------------------------------- edges ---
def _i64_pair(rng, n, pool=50):
    pa = rng.integers(I64_MIN, I64_MAX, pool, dtype=np.int64, endpoint=True)
    pb = rng.integers(I64_MIN, I64_MAX, pool, dtype=np.int64, endpoint=True)
    return lambda m: [(pa[rng.integers(0, pool, m)], None), (pb[rng.integers(0, pool, m)], None)]


def test_empty_right_side(pl, orc):
    side = _i64_pair(np.random.default_rng(12), 0)
    lcols, rcols = side(5_000), [(np.zeros(0, np.int64), None), (np.zeros(0, np.int64), None)]
    L, R = _frames(pl, ["a", "b"], lcols, rcols)
    ref = Ref(orc, lcols, rcols)
    heights = {}
    for how in ("inner", "left", "semi", "anti"):
        out, _ = _join_and_check(pl, L, R, ref, how, dict(on=["a", "b"]))
        heights[how] = out.height
        if how == "left":
            assert not _got(out)[2].any()
    assert heights == {"inner": 0, "left": 5_000, "semi": 0, "anti": 5_000}


def test_empty_left_side(pl, orc):
    side = _i64_pair(np.random.default_rng(13), 0)
    lcols, rcols = [(np.zeros(0, np.int64), None), (np.zeros(0, np.int64), None)], side(3_000)
    L, R = _frames(pl, ["a", "b"], lcols, rcols)
    ref = Ref(orc, lcols, rcols)
    for how in ("inner", "left", "semi", "anti"):
        out, _ = _join_and_check(pl, L, R, ref, how, dict(on=["a", "b"]))
        assert out.height == 0


def test_every_right_key_null(pl, orc):
    rng = np.random.default_rng(14)
    side = _i64_pair(rng, 0)
    lcols, r = side(5_000), side(2_000)
    half = np.arange(2_000) % 2 == 0
    rcols = [(r[0][0], half), (r[1][0], ~half)]                   # every right row has exactly one null part
    L, R = _frames(pl, ["a", "b"], lcols, rcols)
    ref = Ref(orc, lcols, rcols)
    heights = {}
    for how in ("inner", "left", "semi", "anti"):
        out, _ = _join_and_check(pl, L, R, ref, how, dict(on=["a", "b"]))
        heights[how] = out.height
    assert heights == {"inner": 0, "left": 5_000, "semi": 0, "anti": 5_000}


def test_more_than_one_grid_stride_round(pl, orc):
    """300 000 x 50 000 rows: more rows than one pass of the grid (k::grid_for(n, kBlock * 2)) covers"""
    rng = np.random.default_rng(15)
    side = _i64_pair(rng, 0, pool=300)
    lcols, rcols = side(300_000), side(50_000)
    L, R = _frames(pl, ["a", "b"], lcols, rcols)
    ref = Ref(orc, lcols, rcols)
    out, plan = _join_and_check(pl, L, R, ref, "inner", dict(on=["a", "b"]), "left_right")
    assert "rows=50000" in plan and "probe rows=300000" in plan, plan
    assert out.height > 100_000
    _join_and_check(pl, L, R, ref, "anti", dict(on=["a", "b"]))


def test_left_on_right_on_names_and_unfused_plan(pl, orc):
    """different key names on the two sides: the right key columns stay out of the result (coalesced), as _finish_join gives them; the same through PLX_PLAN_NO_FUSION"""
    rng = np.random.default_rng(16)
    side = _i64_pair(rng, 0)
    lcols, rcols = side(NL), side(NR)
    L, R = _frames(pl, ["a", "b"], lcols, rcols, rnames=["x", "y"])
    ref = Ref(orc, lcols, rcols)
    for kw in ({}, {"no_fusion": True}):
        for how in ("inner", "left"):
            out, plan = _join_and_check(pl, L, R, ref, how, dict(left_on=["a", "b"], right_on=["x", "y"]), "left", **kw)
            assert out.columns == ["a", "b", "lrow", "rrow"] and out.height > 10_000
            g_l = out["lrow"].to_numpy()
            assert np.array_equal(out["a"].to_numpy(), lcols[0][0][g_l]) and np.array_equal(out["b"].to_numpy(), lcols[1][0][g_l])
        out, _ = _join_and_check(pl, L, R, ref, "semi", dict(left_on=["a", "b"], right_on=["x", "y"]), **kw)
        assert out.columns == ["a", "b", "lrow"] and out.height > 1000


# -------------------------------------------------------------------------------------------------------------------- limits ---
def test_nine_key_columns_raise_with_the_limit(pl):
    rng = np.random.default_rng(17)
    names = [f"k{j}" for j in range(9)]
    cols = lambda n: [(rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64), None) for _ in names]
    L, R = _frames(pl, names, cols(100), cols(50))
    with pytest.raises(pl.PlxError, match="at most 8 key columns") as e:
        L.join(R, on=names)
    assert e.value.code == 3                                       # PLX_ERR_UNSUPPORTED
    out = L.join(R, on=names[:8], how="left")                      # 8 is joined
    assert "words=8" in _wide_plan(pl) and out.height == 100


def test_wide_route_switched_off_raises_as_before(pl, monkeypatch):
    rng = np.random.default_rng(18)
    lcols = [(rng.integers(0, 10, 100).astype(np.int64), None), (rng.integers(0, 10, 100).astype(np.float64), None)]
    rcols = [(rng.integers(0, 10, 50).astype(np.int64), None), (rng.integers(0, 10, 50).astype(np.float64), None)]
    L, R = _frames(pl, ["a", "f"], lcols, rcols)
    monkeypatch.setenv("PLX_JOIN_WIDE_KEYS", "0")
    with pytest.raises(pl.PlxError, match="multi-column join keys must be integer / boolean / dictionary codes on this path") as e:
        L.join(R, on=["a", "f"])
    assert e.value.code == 3
