"""Inputs, sizing arithmetic and the numpy reference of the hash-join build recovery tests (tests/test_gpu_join_build_recovery.py, tests/test_join_build_inputs_cpu.py).
Plain numpy: nothing here imports the product.  HashBuild::run (engine.cpp) sizes the table of a build side of >= 2^24 rows from a sample, rebuilds it once from the
exact count when the sample misjudged, switches the windowed (LDS-filled) build off when a window of a rightly sized table fills up, and rebuilds with row chains
when build keys repeat.  Each case below is an input whose DATA sends the build down one of these branches; the CPU test proves the properties, next to a restatement
of the arithmetic they follow from, and the GPU test asserts the branch from the plan text and compares every pair / group with the reference here.

A case is a dict: name, rid (uint64 ids), rk (Int64 build keys = rid * HASH_MULT mod 2^64), s (one-byte selector: the build side's predicate is s != 0), a (Int64
build attribute), pk / x (probe key and value), part_build (PLX_JOIN_PART_BUILD or None), order (argsort of rk) and porder (argsort of pk)."""
import functools

import numpy as np

H = 1 << 24                                   # the smallest build side that is sized from a sample (engine.cpp HashBuild::run)
N_PROBE = H + 4321                            # one row longer than needed: the shorter side builds an inner join (resolve_join_sides)
H_SMALL, N_PROBE_SMALL = 1_200_000, (1 << 22) + 4321
HASH_MULT = 0x9E3779B97F4A7C15                # tests/test_gpu_join_partitioned.py: odd, so id -> id * HASH_MULT mod 2^64 is a bijection
TABLE_MULT = 0x55FBFD6BFC5458E9               # fused.hpp kP2HashMult: slot of a key = (key * TABLE_MULT mod 2^64) >> (64 - log2_cap)
SAMPLE_BLOCKS, SAMPLE_BLOCK_ROWS = 4, 1 << 18  # HashBuild::run kCountBlocks, per
WINDOW_LOG2 = 13                              # engine.cpp kJoinWindowLog2: windows of 8192 slots
WINDOW = 1 << WINDOW_LOG2
WINDOWED_MIN_LOG2_CAP = WINDOW_LOG2 + 8       # partitioned_build_wanted
PROBE_LIMIT = 1 << 16                         # fused_sinks.hpp JoinBuildSink: the longest probe sequence of the plain build
MIN_LOG2_CAP = {"group_by": 4, "frame": 8}    # HashBuildOptions::min_log2_cap of the two callers
M64 = (1 << 64) - 1
CASES = ["sample_right", "sample_load", "sample_overflow_windowed", "sample_sees_nothing", "crowded_window", "windowed_finds_duplicates", "misjudged_and_duplicates"]


def mul64(a, m):
    """a * m mod 2^64, as Int64"""
    with np.errstate(over="ignore"):
        return (np.asarray(a).astype(np.uint64) * np.uint64(m & M64)).view(np.int64)


def hashed(ids):
    return mul64(ids, HASH_MULT)


# ------------------------------------------------------------------------------------------------ sizing arithmetic, restated
def sample_rows(height):
    """HashBuild::run: block b starts at b * ((H / 4) & ~127) and holds min(2^18, H - start) rows."""
    stride = (height // SAMPLE_BLOCKS) & ~127
    return np.concatenate([np.arange(b * stride, min(b * stride + SAMPLE_BLOCK_ROWS, height), dtype=np.int64) for b in range(SAMPLE_BLOCKS) if b * stride < height])


def sampled_estimate(keep):
    """nb = (uint64)(hits / seen * H * 1.25) + 4096 -> (hits, seen, nb)"""
    rows = sample_rows(len(keep))
    hits, seen = int(np.count_nonzero(keep[rows])), len(rows)
    return hits, seen, int(hits / max(seen, 1) * len(keep) * 1.25) + 4096


def ceil_log2(x):
    """engine.cpp ceil_log2_u64: the smallest b with 2^b >= x"""
    return max(0, int(x) - 1).bit_length()


def log2_cap(nb, sampled, min_log2):
    """log2_cap = max(min, ceil_log2((uint64)(max(nb, 1) * (sampled ? 1.6 : 2.0))))"""
    return max(min_log2, ceil_log2(int(max(nb, 1) * (1.6 if sampled else 2.0))))


def window_of(keys, cap_log2):
    """join_bin_kernel: (key * kP2HashMult) >> (64 - (log2_cap - log2_window))"""
    return (mul64(keys, TABLE_MULT).view(np.uint64) >> np.uint64(64 - (cap_log2 - WINDOW_LOG2))).astype(np.int64)


def window_fills(keys, cap_log2):
    return np.bincount(window_of(keys, cap_log2), minlength=1 << (cap_log2 - WINDOW_LOG2))


def windowed(case, cap_log2):
    """partitioned_build_wanted: PLX_JOIN_PART_BUILD 0 never | 1 (default) build sides of >= 2^24 rows | 2 any size; never below 2^21 slots"""
    mode = int(case["part_build"] or 1)
    return mode > 0 and cap_log2 >= WINDOWED_MIN_LOG2_CAP and (mode >= 2 or len(case["rk"]) >= 1 << 24)


def sizing(case, route="group_by"):
    """-> first: log2_cap of the first attempt, exact: log2_cap from the exact count, sampled, passing (build rows that pass), load (of the first table)"""
    keep = case["s"] != 0
    passing = int(np.count_nonzero(keep))
    sampled = len(keep) >= 1 << 24
    first = log2_cap(sampled_estimate(keep)[2], True, MIN_LOG2_CAP[route]) if sampled else log2_cap(passing, False, MIN_LOG2_CAP[route])
    return {"first": first, "exact": log2_cap(passing, False, MIN_LOG2_CAP[route]), "sampled": sampled, "passing": passing, "load": passing / (1 << first)}


# ------------------------------------------------------------------------------------------------ inputs
def _ids(rng, n):
    return np.arange(n, dtype=np.uint64) * np.uint64(3) + rng.integers(0, 3, n).astype(np.uint64)       # distinct, ids < 3 n


def _probe(rng, rid, n):
    """~8 % of the probe rows carry the id of a random build row (so about 5 % hit a SURVIVING one), the others an id no build row has"""
    take = rng.random(n) < 0.08
    pid = np.where(take, rid[rng.integers(0, len(rid), n)], np.uint64(3 * len(rid)) + rng.integers(0, 1 << 40, n).astype(np.uint64))
    return hashed(pid), rng.integers(-1000, 1000, n).astype(np.int64)


@functools.lru_cache(maxsize=None)
def large_shared():
    """R (2^24 rows) and L (2^24 + 4321 rows) of cases 1-4 and 7, built once"""
    rng = np.random.default_rng(2401)
    rid = _ids(rng, H)
    rk = hashed(rid)
    pk, x = _probe(rng, rid, N_PROBE)
    return {"rid": rid, "rk": rk, "a": rng.integers(-1000, 1000, H).astype(np.int64), "pk": pk, "x": x, "order": np.argsort(rk, kind="stable"), "porder": np.argsort(pk, kind="stable")}


def _rate_selector(rng, n, sampled_rate, other_rate):
    s = (rng.random(n) < other_rate).astype(np.int8)
    rows = sample_rows(n)
    s[rows] = rng.random(len(rows)) < sampled_rate
    return s


def _write_second_rows(rng, case, n_dup, agree_every=2):
    """n_dup passing rows' keys are written into n_dup OTHER passing rows (each key then occurs twice); every `agree_every`-th pair also agrees on the attribute"""
    ok = np.nonzero((case["s"] != 0) & (case["rk"] != -1))[0]
    pick = rng.choice(ok, 2 * n_dup, replace=False)
    src, dst = pick[:n_dup], pick[n_dup:]
    for c in ("rid", "rk", "a"):
        case[c] = case[c].copy()
    case["rid"][dst], case["rk"][dst] = case["rid"][src], case["rk"][src]
    case["a"][dst[::agree_every]] = case["a"][src[::agree_every]]
    case["a"][dst[1::agree_every]] = case["a"][src[1::agree_every]] + 1
    case["order"] = np.argsort(case["rk"], kind="stable")


def build(name):
    rng = np.random.default_rng(CASES.index(name) + 77)
    if name in ("crowded_window", "windowed_finds_duplicates"):
        rid = _ids(rng, H_SMALL)
        case = {"name": name, "part_build": "2", "rid": rid, "a": rng.integers(-1000, 1000, H_SMALL).astype(np.int64), "s": (rng.random(H_SMALL) < 0.95).astype(np.int8)}
        if name == "crowded_window":
            # 9000 keys whose table hash h = key * TABLE_MULT shares its top 14 bits: one window (the top log2_cap - 13 <= 14 bits) and 256 adjacent home slots of a 2^22 table
            rows = rng.choice(H_SMALL, 9000, replace=False)
            h = (np.uint64(0x2A5B) << np.uint64(50)) | rng.integers(0, 1 << 50, 9000).astype(np.uint64)
            key = mul64(h, pow(TABLE_MULT, -1, 1 << 64))
            rid[rows] = mul64(key, pow(HASH_MULT, -1, 1 << 64)).view(np.uint64)
            case["s"][rows] = 1
            case["crowded_rows"] = rows
        case["rk"] = hashed(rid)
        if name == "windowed_finds_duplicates":
            e = rng.choice(H_SMALL, 2, replace=False)                 # the key whose bits are the table's EMPTY pattern, twice
            rid[e] = np.uint64((M64 * pow(HASH_MULT, -1, 1 << 64)) & M64)
            case["rk"] = hashed(rid)
            case["s"][e] = 1
            _write_second_rows(rng, case, 12_000)
        case["pk"], case["x"] = _probe(rng, case["rid"], N_PROBE_SMALL)
        if name == "windowed_finds_duplicates":
            case["pk"][:2] = -1
        case["order"] = np.argsort(case["rk"], kind="stable")
        case["porder"] = np.argsort(case["pk"], kind="stable")
        return case
    case = dict(large_shared(), name=name, part_build=None)
    if name == "sample_right":
        case["s"] = (rng.random(H) < 0.4).astype(np.int8)
    elif name == "sample_load":
        case["s"] = _rate_selector(rng, H, 0.24, 0.41)        # (0.25 * 1.25 * 1.6 = 0.5: at 25 % the + 4096 tips the first table over 2^23, so a little below)
    elif name in ("sample_overflow_windowed", "misjudged_and_duplicates"):
        case["s"] = _rate_selector(np.random.default_rng(79), H, 1.0 / 16, 1.0)       # what a date range does on time-ordered data (one selector for both cases)
        if name == "misjudged_and_duplicates":
            _write_second_rows(rng, case, 1000)
    elif name == "sample_sees_nothing":
        case["s"] = np.zeros(H, np.int8)
        case["s"][300_000:3_300_000] = 1                        # between the sample blocks at rows 0 and 2^22
    else:
        raise KeyError(name)
    return case


def shuffled_selector(case, seed=5):
    """the same number of passing rows, spread evenly: the sample is right (the cost-of-recovery comparison)"""
    return np.random.default_rng(seed).permutation(case["s"])


# ------------------------------------------------------------------------------------------------ the reference
def survivors(case):
    """-> (the surviving build keys, sorted; their build rows)"""
    rows = case["order"][(case["s"] != 0)[case["order"]]]
    return case["rk"][rows], rows


def pairs(case):
    """The join in plain numpy: np.searchsorted of the probe keys in the sorted surviving build keys.
    -> (probe rows, build rows) of every matching pair, and the probe rows without a match (a left join keeps them, with nulls on the build side)."""
    sk, rows = survivors(case)
    porder = case["porder"]
    sp = case["pk"][porder]                                    # (sorted needles: the binary searches walk the build keys front to back)
    lo, hi = np.searchsorted(sk, sp, "left"), np.searchsorted(sk, sp, "right")
    cnt = hi - lo
    hit = cnt > 0
    c = cnt[hit]
    first = np.cumsum(c) - c
    within = np.arange(int(c.sum()), dtype=np.int64) - np.repeat(first, c)
    return np.repeat(porder[hit], c), rows[np.repeat(lo[hit], c) + within], porder[~hit]


def sort_pairs(p, b):
    o = np.lexsort((b, p))
    return np.asarray(p)[o].astype(np.int64), np.asarray(b)[o].astype(np.int64)


def groups(case):
    """group_by(k, a).agg(x.sum(), len) over the joined rows -> (k, a, sum of x, len), sorted by (k, a)"""
    p, b, _ = pairs(case)
    return group_rows(case["pk"][p], case["a"][b], case["x"][p])


def group_rows(k, a, x):
    o = np.lexsort((a, k))
    k, a, x = k[o], a[o], x[o]
    if len(k) == 0:
        return k, a, x, np.zeros(0, np.int64)
    head = np.nonzero(np.concatenate([[True], (k[1:] != k[:-1]) | (a[1:] != a[:-1])]))[0]
    return k[head], a[head], np.add.reduceat(x, head), np.diff(np.concatenate([head, [len(k)]])).astype(np.int64)


# ------------------------------------------------------------------------------------------------ case -> frames / queries (`pl`: the product, passed in)
def frames(pl, case):
    """fresh frames (what a column has learned -- its keys repeat as a build key -- stays with the frame): L(k, x, lr), R(k, s, a, rr); lr / rr are row numbers"""
    L = pl.DataFrame({"k": case["pk"], "x": case["x"], "lr": np.arange(len(case["pk"]), dtype=np.int32)})
    R = pl.DataFrame({"k": case["rk"], "s": case["s"], "a": case["a"], "rr": np.arange(len(case["rk"]), dtype=np.int32)})
    return L, R


def group_by_query(pl, L, R):
    c = pl.col
    return L.lazy().join(R.lazy().filter(c("s") != 0), on="k").group_by("k", "a").agg(c("x").sum().alias("sx"), pl.len().alias("n"))


def frame_query(pl, L, R, how):
    c = pl.col
    return L.lazy().join(R.lazy().filter(c("s") != 0), on="k", how=how).select(c("lr"), c("rr"))
