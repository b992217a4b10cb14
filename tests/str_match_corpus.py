"""The corpus of the string-predicate tests (CPU and GPU), the reference and the helpers both share.

Strings are seen the way the library sees them: as the 16-byte views and the data buffer of a pyarrow string_view array.  The reference is Python's
bytes.startswith / endswith / in on the UTF-8 bytes (None stays None), cross-checked against pyarrow.compute."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc

from polars_amd import _ffi as F

KINDS = {F.STR_STARTS_WITH: "starts_with", F.STR_ENDS_WITH: "ends_with", F.STR_CONTAINS: "contains"}

# lengths 0, 1, 3, 4, 5, 11, 12, 13, 20 and 40; equal 4-byte prefixes with different tails; multi-byte UTF-8; a zero byte; nulls
STRINGS = [
    "", "a", "abc", "abcd", "abcde", "hello world", "hello world!", "hello world!!",
    "PROMO PLATED TIN 20x", "PROMO ANODIZED STEEL and a forty-byte ta", None,
    "PROMO BRUSHED COPPER", "PROMISE of a long tail", "PROM", "PROMO", "STANDARD POLISHED BRASS", "ECONOMY PROMO",
    "héllo wörld ünï", "naïve", "ab\0cd", "zero\0inside a longer string", "abc\0", None, "x" * 12, "x" * 13,
]
assert sorted({len(s.encode()) for s in STRINGS if s is not None} & {0, 1, 3, 4, 5, 11, 12, 13, 20, 40}) == [0, 1, 3, 4, 5, 11, 12, 13, 20, 40]

# lengths 0, 1, 3, 4, 5, 8, 12, 13 and 20; at the start, in the middle and at the end of a string; longer than the string; the whole string;
# "c\0" / "abc\0\0" would match only the zero padding of the inline view of "abc" and must not
PATTERNS = [
    "", "a", "x", "abc", "PRO", "rld", "abcd", "PROM", "ld!!", "abcde", "PROMO", "world", "PROMO PL", "lo world", " a forty", "-byte ta",
    "hello world!", "ello world!!", "ATED TIN 20x", "hello world!!", "ISE of a long", "PROMO PLATED TIN 20x", "ANODIZED STEEL and a", " and a forty-byte ta",
    "c\0", "abc\0\0", "\0", "\0c", "ö", "wörld ü", "ï", "inside a longer string", "STANDARD POLISHED BRASS and more than that",
]
assert {len(p.encode()) for p in PATTERNS} >= {0, 1, 3, 4, 5, 8, 12, 13, 20}


def as_bytes(x):
    return None if x is None else (x.encode("utf-8") if isinstance(x, str) else bytes(x))


def reference(kind, strings, pattern):
    """Python's own semantics on bytes; None -> None."""
    p = as_bytes(pattern)
    out = []
    for s in strings:
        b = as_bytes(s)
        out.append(None if b is None else (b.startswith(p) if kind == F.STR_STARTS_WITH else b.endswith(p) if kind == F.STR_ENDS_WITH else p in b))
    return out


def arrow_reference(kind, strings, pattern):
    arr = pa.array(strings, pa.string_view())
    fn = {F.STR_STARTS_WITH: pc.starts_with, F.STR_ENDS_WITH: pc.ends_with, F.STR_CONTAINS: pc.match_substring}[kind]
    try:
        return fn(arr, pattern=pattern).to_pylist()
    except pa.ArrowNotImplementedError:          # a pyarrow whose string kernels do not take views yet: the same strings as a string array
        return fn(arr.cast(pa.string()), pattern=pattern).to_pylist()


def split(values):
    """[True | False | None] -> (values with False under nulls, validity) as bool arrays."""
    return np.array([bool(v) for v in values], dtype=bool), np.array([v is not None for v in values], dtype=bool)


def views_of(strings, binary=False):
    """(views: uint64 array [n, 2] with the nulls stamped (length word 0xFFFFFFFF), data: the bytes behind views of more than 12 bytes) of a pyarrow view array."""
    arr = pa.array([as_bytes(s) for s in strings], pa.binary_view()) if binary else pa.array(strings, pa.string_view())
    a, s = F.ArrowArray(), F.ArrowSchema()
    arr._export_to_c(C.addressof(a), C.addressof(s))
    try:
        n, nb = a.length, a.n_buffers
        assert a.offset == 0 and nb <= 4, "one data buffer at the most"
        views = np.frombuffer(C.string_at(a.buffers[1], 16 * n), np.uint64).reshape(n, 2).copy() if n else np.zeros((0, 2), np.uint64)
        data = b""
        if nb == 4:
            size = C.cast(a.buffers[3], C.POINTER(C.c_int64))[0]
            data = C.string_at(a.buffers[2], size)
    finally:
        for st, ty in ((a, F.ArrowArray), (s, F.ArrowSchema)):
            if st.release:
                C.CFUNCTYPE(None, C.POINTER(ty))(st.release)(C.byref(st))
    for i, x in enumerate(strings):
        if x is None:
            views[i] = (0xFFFFFFFF, 0)
    return views, data


def tile(seq, n):
    """The first n entries of seq repeated for ever."""
    return [seq[i % len(seq)] for i in range(n)]


def tile_views(views, n):
    return views[np.arange(n) % len(views)].copy() if n else np.zeros((0, 2), np.uint64)


def unpack(words, n):
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)


def host_match(views, data, kind, pattern, data_none=False):
    """plx_strview_match_host -> (status, values, validity, raw words); data_none: pass data = NULL."""
    n = len(views)
    p = as_bytes(pattern)
    words = (n + 63) // 64
    ob, ov = np.full(words + 1, 0xA5A5A5A5A5A5A5A5, np.uint64), np.full(words + 1, 0xA5A5A5A5A5A5A5A5, np.uint64)      # (a canary word behind the output)
    v = np.ascontiguousarray(views)
    st = F.lib().plx_strview_match_host(v.ctypes.data if n else None, None if data_none else data, 0 if data_none else len(data), n, kind, p, len(p), ob.ctypes.data, ov.ctypes.data)
    assert ob[words] == 0xA5A5A5A5A5A5A5A5 and ov[words] == 0xA5A5A5A5A5A5A5A5
    return st, unpack(ob[:words], n), unpack(ov[:words], n), (ob[:words], ov[:words])
