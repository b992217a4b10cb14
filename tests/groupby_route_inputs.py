"""Inputs, planner arithmetic and the numpy reference of the group-by route tests (tests/test_gpu_groupby_routes.py, tests/groupby_route_worker.py,
tests/test_groupby_route_inputs_cpu.py).  Plain numpy: nothing here imports the product, so the properties each GPU case relies on -- what the planner's
sample sees, how many distinct keys there are, how many bits a packed id needs -- are checked on the CPU, next to a restatement of the arithmetic of
run_fused_groupby's helpers (engine.cpp: sample_keys, estimate_groups, size_hash_table, lower_keys; kernels_partition.hip: partition_plan, partition_plan2).

A case is a dict: n, cols {name: (values, valid or None)}, keys [name], aggs [(alias, op, column or None)], and -- for join cases -- build / probe tables."""
import math

import numpy as np

RTOL = 1e-6                      # tests/test_gpu_queries.py
SAMPLE_ROWS = 1 << 20            # engine.cpp kPartSampleRows: the strided sample of the partitioned routes
PREFIX_ROWS = 1 << 22            # engine.cpp size_hash_table S: the prefix sample of every other route
SAMPLE_BLOCKS = 8                # engine.cpp kSampleBlocks
HOT_FRACTION = 4096              # engine.cpp kHotFraction
MAX_HOT = 256                    # fused.hpp kP2MaxHot
LDS_TABLE_BYTES = 144 * 1024     # partition_plan / partition_plan2: what a partition's LDS table may take


# ------------------------------------------------------------------------------------------------ what the planner samples
def sample_rows(n, S=SAMPLE_ROWS):
    """Row indices of sample_keys (engine.cpp): 8 blocks, per = (S / 8) & ~127 rows each, block b starts at b * ((n / 8) & ~127)."""
    per, stride = (S // SAMPLE_BLOCKS) & ~127, (n // SAMPLE_BLOCKS) & ~127
    return np.concatenate([np.arange(b * stride, min(b * stride + per, n), dtype=np.int64) for b in range(SAMPLE_BLOCKS) if b * stride < n])


def prefix_rows(n, S=PREFIX_ROWS):
    """The other sample (size_hash_table when it is not strided: no_partition, PLX_PART_V=1): the first 2^22 rows."""
    return np.arange(min(n, S), dtype=np.int64)


# ------------------------------------------------------------------------------------------------ planner arithmetic, restated
def ceil_log2(x):
    return max(0, (int(x) - 1).bit_length())


def estimate_groups(d, S):
    """engine.cpp estimate_groups: solve d = G (1 - exp(-S / G)) for G."""
    if d >= S * 0.999:
        return 1e18
    lo, hi = float(d), 1e15
    for _ in range(200):
        mid = math.sqrt(lo * hi)
        if mid * (1.0 - math.exp(-S / mid)) < d:
            lo = mid
        else:
            hi = mid
    return hi


def sample_estimate(sampled_codes, null_code=None):
    """sample_keys on the sampled rows' keys (any integer code per key; `null_code`: the code of the null key, which is never hot)
    -> (distinct, number of hot keys, estimated groups).  Hot: >= max(64, rows / 4096) sampled rows, the 256 heaviest."""
    u, cnt = np.unique(sampled_codes, return_counts=True)
    S = len(sampled_codes)
    thr = max(64, S // HOT_FRACTION)
    hot = cnt >= thr
    if null_code is not None:
        hot &= u != null_code
    hot_cnt = np.sort(cnt[hot])[::-1][:MAX_HOT]
    n_hot, hot_rows, d = len(hot_cnt), int(hot_cnt.sum()), len(u)
    d_rest, s_rest = max(0, d - n_hot), max(1.0, S - hot_rows)
    return d, n_hot, (estimate_groups(d_rest, s_rest) if d_rest > 0 else 0.0) + n_hot


def hash_slots(n_aggs, wide_words=0):
    """partition_plan2, hash mode: slots of one partition's LDS table.  Single key: 8 (1 + n_aggs) bytes a slot, 144 KB / that - 2, at most 2^14.
    Wide keys (`wide_words` = key words + null-mask word): 16 + 8 (words + n_aggs) bytes a group, an even count, at most 4096."""
    if wide_words:
        return min((LDS_TABLE_BYTES // (16 + 8 * (wide_words + n_aggs))) & ~1, 4096)
    return min(LDS_TABLE_BYTES // (8 * (1 + n_aggs)) - 2, 1 << 14)


def hash_plan(n_aggs, est, wide_words=0):
    """partition_plan2, hash mode -> log2_parts for `est` groups (None: no plan).  The smallest of 64..512 partitions whose tables hold `est` at a load
    of 0.85; 512 partitions are still taken up to a load of 0.95."""
    slots = hash_slots(n_aggs, wide_words)
    if slots < 256:
        return None
    lp = 6
    while lp < 9 and (1 << lp) * slots * 0.85 < est:
        lp += 1
    if (1 << lp) * slots * 0.85 < est and (1 << lp) * slots * 0.95 < est:
        return None
    return lp


def v1_plan(n_aggs, est):
    """partition_plan (first generation) -> (log2_slots, log2_parts) or None: the largest power of two <= 2^14 slots with (slots + 2) * 8 (1 + n_aggs)
    bytes within 144 KB, 64..1024 partitions of slots * 0.62 groups each."""
    ls = 14
    while ls > 8 and ((1 << ls) + 2) * 8 * (1 + n_aggs) > LDS_TABLE_BYTES:
        ls -= 1
    lp = 6
    while lp < 10 and (1 << lp) * (1 << ls) * 0.62 < est:
        lp += 1
    return None if (1 << lp) * (1 << ls) * 0.62 < est else (ls, lp)


def packed_bits(case):
    """lower_keys: a key column takes max(1, ceil_log2(max - min + 1 + (1 if nullable))) bits of the packed id."""
    bits = 0
    for k in case["keys"]:
        v, valid = case["cols"][k]
        vv = v if valid is None else v[valid]
        bits += max(1, ceil_log2(int(vv.max()) - int(vv.min()) + 1 + (0 if valid is None else 1)))
    return bits


def key_codes(case, rows=None):
    """One int64 code per row that is equal exactly where the key tuples are equal (null = a value of its own) -> (codes, code of the all-null / null key or None)."""
    code, null_code = None, None
    if "ids" in case:                                   # the builder's own group ids (the keys are an injective image of them): no sort needed
        ids = case["ids"] if rows is None else case["ids"][rows]
        nullable = [case["cols"][k][1] for k in case["keys"] if case["cols"][k][1] is not None]
        if not nullable:
            return ids.astype(np.int64), None
        ok = nullable[0] if rows is None else nullable[0][rows]
        assert len(nullable) == 1
        if len(case["keys"]) == 1:
            return np.where(ok, ids, int(case["ids"].max()) + 1).astype(np.int64), int(case["ids"].max()) + 1
        return np.where(ok, ids.astype(np.int64) * 2, case["null_ids"][ids].astype(np.int64) * 2 + 1), None
    for k in case["keys"]:
        v, valid = case["cols"][k]
        if rows is not None:
            v, valid = v[rows], (None if valid is None else valid[rows])
        u, inv = np.unique(v if valid is None else np.where(valid, v, v[0]), return_inverse=True)
        inv = inv.astype(np.int64)
        if valid is not None:
            inv[~valid] = len(u)
        code = inv if code is None else code * (len(u) + 1) + inv
        if len(case["keys"]) == 1 and valid is not None:
            null_code = len(u)
    return code, null_code


# ------------------------------------------------------------------------------------------------ the reference
def reference(keys, valid, aggs):
    """The group-by in plain numpy.  keys: key column arrays (integers); valid: one bool array or None per key column (a null key is a key value of its own);
    aggs: [(alias, op, (values, valid or None) or None)], op in sum | count | len | min | max | mean.
    -> {"uniques": per key column its sorted distinct non-null values, "codes": sorted combined code of every group, "aggs": {alias: (values, valid)}}.
    Null rows of a value column take no part; a group without any: sum 0, count 0, min / max / mean null (valid False)."""
    n = len(keys[0]) if keys else 0
    uniques, code = [], np.zeros(n, np.int64)
    for col, ok in zip(keys, valid):
        assert np.issubdtype(col.dtype, np.integer), col.dtype
        u, inv = np.unique(col if ok is None or n == 0 else col[ok], return_inverse=True)
        if ok is None or n == 0:
            c = inv.astype(np.int64)
        else:
            c = np.full(n, len(u), np.int64)
            c[ok] = inv
        uniques.append(u)
        code = code * (len(u) + 1) + c                      # (at most a few million distinct values a column: far from 2^63)
    codes, gid = np.unique(code, return_inverse=True)
    G = len(codes)
    out = {}
    for alias, op, src in aggs:
        if op == "len":
            out[alias] = (np.bincount(gid, minlength=G).astype(np.int64), np.ones(G, bool))
            continue
        v, ok = src
        g, v = (gid, v) if ok is None else (gid[ok], v[ok])
        cnt = np.bincount(g, minlength=G).astype(np.int64)
        if op == "count":
            out[alias] = (cnt, np.ones(G, bool))
        elif op in ("sum", "mean"):
            if np.issubdtype(v.dtype, np.integer):
                bound = (int(np.abs(v).max()) if len(v) else 0) * (int(cnt.max()) if G else 0)
                if bound < 2 ** 53:      # |every partial sum| < 2^53: the float64 accumulator of bincount holds these integers exactly
                    s = np.bincount(g, weights=v, minlength=G).astype(np.int64)
                else:
                    s = np.zeros(G, np.int64)
                    np.add.at(s, g, v.astype(np.int64))
            else:
                s = np.bincount(g, weights=v.astype(np.float64), minlength=G)
            if op == "sum":
                out[alias] = (s, np.ones(G, bool))
            else:
                out[alias] = (s.astype(np.float64) / np.maximum(cnt, 1), cnt > 0)
        elif op in ("min", "max"):
            if np.issubdtype(v.dtype, np.integer):
                r = np.full(G, np.iinfo(v.dtype).max if op == "min" else np.iinfo(v.dtype).min, v.dtype)
            else:
                r = np.full(G, np.inf if op == "min" else -np.inf, v.dtype)
            (np.minimum if op == "min" else np.maximum).at(r, g, v)
            out[alias] = (r, cnt > 0)
        else:
            raise ValueError(op)
    return {"uniques": uniques, "codes": codes, "aggs": out}


def case_reference(case):
    cols = case["cols"]
    return reference([cols[k][0] for k in case["keys"]], [cols[k][1] for k in case["keys"]], [(a, op, None if c is None else cols[c]) for a, op, c in case["aggs"]])


def assert_groups_equal(got, ref, key_names, what=""):
    """got: {column name: (values, valid or None)} as downloaded from the result frame.  Every group of `ref` is there exactly once, with its keys (the null
    group included); integer aggregates, count and len are equal, float aggregates are within RTOL -- group by group."""
    G = len(ref["codes"])
    h = len(got[key_names[0]][0])
    assert h == G, (what, "groups", h, G)
    if G == 0:
        return
    code = np.zeros(G, np.int64)
    for name, u in zip(key_names, ref["uniques"]):
        v, ok = got[name]
        ok = np.ones(G, bool) if ok is None else np.asarray(ok, bool)
        pos = np.minimum(np.searchsorted(u, v), max(len(u) - 1, 0))
        assert len(u) > 0 or not ok.any(), (what, name)
        if len(u):
            assert bool(np.all((u[pos] == v) | ~ok)), (what, name, "a key value that is not in the input")
        code = code * (len(u) + 1) + np.where(ok, pos, len(u))
    order = np.argsort(code, kind="stable")
    assert np.array_equal(code[order], ref["codes"]), (what, "the key tuples (null group included) are not those of the reference")
    for alias, (want, want_ok) in ref["aggs"].items():
        v, ok = got[alias]
        ok = np.ones(G, bool) if ok is None else np.asarray(ok, bool)
        v, ok = np.asarray(v)[order], ok[order]
        assert np.array_equal(ok, want_ok), (what, alias, "null groups")
        if np.issubdtype(want.dtype, np.integer):
            assert np.issubdtype(v.dtype, np.integer), (what, alias, v.dtype)
            bad = np.nonzero((v.astype(np.int64) != want.astype(np.int64)) & want_ok)[0]
        else:
            bad = np.nonzero(~np.isclose(v.astype(np.float64), want, rtol=RTOL, atol=1e-9) & want_ok)[0]
        assert len(bad) == 0, (what, alias, f"{len(bad)} of {G} groups differ", v[bad[:5]], want[bad[:5]])


# ------------------------------------------------------------------------------------------------ inputs
def sparse(ids):
    """Int64 keys that are no dense range (span of 1e6 ids: 2^40)."""
    return ids.astype(np.int64) * 1_000_003 - 10 ** 12


def full64(ids):
    """Int64 keys over all 64 bits (their exact range, once learned, spans more than 2^62: such a key never packs)."""
    return (ids.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)).view(np.int64)


def _plant(g, rng, few, n, strided=True, prefix=False):
    """rows the planner samples see only `few` ids"""
    if strided:
        r = sample_rows(n)
        g[r] = rng.integers(0, few, len(r))
    if prefix:
        g[:PREFIX_ROWS] = rng.integers(0, few, min(n, PREFIX_ROWS))


def _values(rng, n, x_null=0.0):
    v = rng.integers(-1000, 1000, n).astype(np.int64)
    x = rng.uniform(-1, 1, n)
    return (v, None), (x, (rng.random(n) > x_null) if x_null else None)


N24 = 1 << 24
CFG3_AGGS = [("v_sum", "sum", "v"), ("v_count", "count", "v")]


def build(name):
    rng = np.random.default_rng(abs(hash_name(name)))
    n = N24
    if name in ("dense_flag", "dense_small"):
        # (a, b) packs into 9 + 6 = 15 bits: beyond the 12 bits of the LDS table, within the 28 of the dense HBM table
        n = N24 if name == "dense_flag" else 3_000_000
        v, x = _values(rng, n, 0.2)
        return {"n": n, "keys": ["a", "b"], "aggs": [("s", "sum", "v"), ("c", "count", "x"), ("mx", "max", "x"), ("n", "len", None)],
                "cols": {"a": (rng.integers(0, 300, n).astype(np.int16), None), "b": (rng.integers(-20, 20, n).astype(np.int8), rng.random(n) > 0.01), "v": v, "x": x}}
    if name == "hash_nosample":
        n = 3_000_001
        v, x = _values(rng, n)
        return {"n": n, "keys": ["k"], "aggs": [("s", "sum", "v"), ("c", "count", "v"), ("n", "len", None)],
                "cols": {"k": (sparse(rng.integers(0, 200_000, n)), rng.random(n) > 0.001), "v": (v[0], rng.random(n) > 0.1)}}
    if name == "grow":
        g = rng.integers(0, 150_000, n)
        _plant(g, rng, 300, n, strided=False, prefix=True)
        v, _ = _values(rng, n)
        return {"n": n, "keys": ["k"], "aggs": [("s", "sum", "v"), ("mn", "min", "v"), ("n", "len", None)], "cols": {"k": (sparse(g), None), "v": v}, "ids": g}
    if name == "overflow_retry":
        g = rng.integers(0, 1_000_000, n)
        _plant(g, rng, 7000, n, strided=True, prefix=True)
        v, _ = _values(rng, n)
        return {"n": n, "keys": ["key"], "aggs": CFG3_AGGS, "cols": {"key": (sparse(g), None), "v": v}, "ids": g}
    if name in ("hot_fits", "hot_fallback"):
        fits = name == "hot_fits"
        G = 120_000 if fits else 1_000_000
        g = rng.integers(0, G, n)
        g[rng.random(n) < 0.5] = 77_777
        v, x = _values(rng, n, 0.1 if fits else 0.0)
        if fits:
            return {"n": n, "keys": ["key"], "aggs": [("s", "sum", "v"), ("c", "count", "v"), ("mn", "min", "x"), ("m", "mean", "x")],
                    "cols": {"key": (full64(g), rng.random(n) > 0.001), "v": v, "x": x}, "ids": g}
        return {"n": n, "keys": ["key"], "aggs": [("s", "sum", "v"), ("xs", "sum", "x"), ("n", "len", None)], "cols": {"key": (sparse(g), None), "v": v, "x": x}, "ids": g}
    if name == "learned":
        n = 17_000_000
        v, _ = _values(rng, n)
        return {"n": n, "keys": ["key"], "aggs": CFG3_AGGS, "cols": {"key": (rng.integers(1000, 301_000, n).astype(np.int64), None), "v": v}}
    if name in ("packed_hash", "packed_overflow"):
        # (a, b) packs into 13 + 13 = 26 bits: beyond the 25 of the direct-address LDS tables, within the 28 of the dense HBM table
        occupied = 300_000 if name == "packed_hash" else 2_000_000
        ids = rng.choice(8192 * 8191, occupied, replace=False)
        g = rng.integers(0, occupied, n)
        if name == "packed_overflow":
            _plant(g, rng, 6000, n)
        g[:4] = [int(np.argmin(ids)), int(np.argmax(ids)), int(np.argmin(ids % 8191)), int(np.argmax(ids % 8191))]
        a, b = (ids // 8191)[g].astype(np.int32), (ids % 8191)[g].astype(np.int32)
        v, x = _values(rng, n, 0.1)
        aggs = [("s", "sum", "v"), ("xs", "sum", "x"), ("n", "len", None)] if name == "packed_hash" else [("s", "sum", "v"), ("n", "len", None)]
        cols = {"a": (a, None), "b": (b, rng.random(n) > 0.001), "v": v}
        if name == "packed_hash":
            cols["x"] = x
        return {"n": n, "keys": ["a", "b"], "aggs": aggs, "cols": cols, "ids": g, "null_ids": ids // 8191}
    if name in ("v2_unavailable", "v1_single_key"):
        g = rng.integers(0, 300_000, n)
    if name == "v2_unavailable":
        v, _ = _values(rng, n)
        return {"n": n, "keys": ["k"], "aggs": [("s", "sum", "v"), ("mn", "min", "v"), ("n", "len", None)], "cols": {"k": (sparse(g), None), "v": v}, "ids": g}
    if name == "v1_single_key":
        v, x = _values(rng, n, 0.1)
        return {"n": n, "keys": ["k"], "aggs": [("s", "sum", "v"), ("m", "mean", "x"), ("n", "len", None)],
                "cols": {"k": (sparse(g), rng.random(n) > 0.001), "v": v, "x": x}, "ids": g}
    if name == "v1_packed_ids":
        return {"n": n, "keys": ["k"], "aggs": [("v_sum", "sum", "v"), ("v_mean", "mean", "v")], "dictionary": ["k"],
                "cols": {"k": (rng.integers(0, 400_000, n).astype(np.uint32), None), "v": (rng.uniform(-100, 100, n), None)}}
    if name == "v1_edges":
        # a sparse single key as v1_single_key's; the value columns carry the planted edge groups of tests/agg_edges.py (Int64 kinds in v, Float64 kinds in x)
        try:
            from tests import agg_edges
        except ImportError:
            import agg_edges
        g = rng.integers(0, 300_000, n)
        p = agg_edges.planted(g, None, 300_000)
        kvalid = (rng.random(n) > 0.001) | np.isin(g, np.array(sorted(p["chosen"])))
        return {"n": n, "keys": ["k"], "aggs": [(op, op, "v") for op in ("sum", "mean", "min", "max", "count")] + [("len", "len", None)],
                "cols": {"k": (sparse(g), kvalid), "v": p["v"], "x": p["x"]}, "ids": g, "chosen": p["chosen"]}
    if name == "v1_wide_keys":
        g = rng.integers(0, 100_000, n)
        v, _ = _values(rng, n)
        return {"n": n, "keys": ["a", "b"], "aggs": [("s", "sum", "v"), ("n", "len", None)], "cols": {"a": (full64(g), None), "b": (full64(g + 12345), None), "v": v}}
    raise KeyError(name)


def hash_name(name):
    return int.from_bytes(name.encode()[:8].ljust(8, b"\0"), "little") & 0x7FFFFFFF      # (a fixed seed per case: str hashes differ from process to process)


def build_join():
    """Cases 11-13: 300 000 build rows with unique sparse keys (z != 3 keeps ~98 % of them), 2^24 probe rows that all find a surviving build row -- but only 40 000
    different ones: the bound the plan knows (one group per surviving build row) is far above what any sample of the joined rows suggests."""
    rng = np.random.default_rng(1113)
    nb, n = 300_000, N24
    bk = sparse(rng.permutation(1_000_000)[:nb])
    build = {"k": bk, "y": rng.integers(0, 300, nb).astype(np.int16), "z": rng.integers(0, 50, nb).astype(np.int8),
             "h": rng.integers(-(1 << 62), 1 << 62, nb).astype(np.int64), "c": rng.uniform(0, 10, nb)}
    alive = np.nonzero(build["z"] != 3)[0]
    used = rng.choice(alive, 40_000, replace=False)
    probe = {"k": bk[used[rng.integers(0, len(used), n)]], "w": rng.uniform(-1, 1, n), "x": rng.integers(-1000, 1000, n).astype(np.int64)}
    return {"n": n, "build": build, "probe": probe, "build_rows": int(len(alive))}


JOIN_QUERIES = {      # keys, aggregates over the joined rows ("wc" = w * c: a probe column times a build column)
    "join_single_key": (["k"], [("s", "sum", "wc"), ("xs", "sum", "x"), ("n", "len", None)]),
    "join_packed_ids": (["y", "z"], [("xs", "sum", "x"), ("cs", "sum", "c"), ("n", "len", None)]),
    "join_wide_keys": (["k", "h"], [("s", "sum", "wc"), ("xs", "sum", "x"), ("n", "len", None)]),
}


def joined_case(j, which):
    """The joined rows on the host: np.searchsorted of the probe keys in the sorted unique surviving build keys."""
    keys, aggs = JOIN_QUERIES[which]
    if "joined" in j:
        return {"n": j["joined_n"], "keys": keys, "aggs": aggs, "cols": j["joined"]}
    b, p = j["build"], j["probe"]
    alive = np.nonzero(b["z"] != 3)[0]
    order = alive[np.argsort(b["k"][alive])]
    sk = b["k"][order]
    pos = np.searchsorted(sk, p["k"])
    hit = (pos < len(sk)) & (sk[np.minimum(pos, len(sk) - 1)] == p["k"])
    rows = order[pos[hit]]
    cols = {"k": (p["k"][hit], None), "x": (p["x"][hit], None), "wc": (p["w"][hit] * b["c"][rows], None)}
    for c in ("y", "z", "h", "c"):
        cols[c] = (b[c][rows], None)
    j["joined"], j["joined_n"] = cols, int(hit.sum())
    return {"n": j["joined_n"], "keys": keys, "aggs": aggs, "cols": cols}


# ------------------------------------------------------------------------------------------------ case -> frame / query / downloaded result (`pl`: the product, passed in)
def frame(pl, case):
    return pl.DataFrame([pl.Series(name, v, dtype=pl.Categorical([], pl.UInt32) if name in case.get("dictionary", ()) else None, validity=ok) for name, (v, ok) in case["cols"].items()])


def agg_exprs(pl, aggs, exprs=None):
    col = lambda c: (exprs or {}).get(c, pl.col(c))
    return [pl.len().alias(a) if op == "len" else getattr(col(c), op)().alias(a) for a, op, c in aggs]


def query(pl, lf, case):
    return lf.group_by(*case["keys"]).agg(*agg_exprs(pl, case["aggs"]))


def download(out):
    return {c: out[c]._download() for c in out.columns}
