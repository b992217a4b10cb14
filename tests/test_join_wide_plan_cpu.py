"""Multi-column join keys at the boundary, no GPU needed: a join on three key columns reaches plx_ir with three key pairs, the Polars attachment hands key lists with
a Float64 / UInt64 part on unchanged, and the C library exports the entry the engine takes for keys that do not pack (join::join_indices_wide is behind plx_collect)."""
import polars_amd as pl
from polars_amd import _ffi as F
from polars_amd import polars_engine as eng
from tests import test_polars_engine_cpu as T


def _frames(rnames=("a", "u", "f")):
    left = pl.DataFrame([T.ph("a", pl.Int64), T.ph("u", pl.UInt64), T.ph("f", pl.Float64), T.ph("x", pl.Int32)])
    right = pl.DataFrame([T.ph(rnames[0], pl.Int64, n=1 << 16), T.ph(rnames[1], pl.UInt64, n=1 << 16), T.ph(rnames[2], pl.Float64, n=1 << 16), T.ph("y", pl.Int32, n=1 << 16)])
    return left, right


def _join_nodes(low):
    return [d for d in low.irs if d["kind"] == F.IR_JOIN]


def test_three_key_columns_reach_the_ir_as_three_key_pairs():
    left, right = _frames()
    lf = left.lazy().join(right.lazy(), on=["a", "u", "f"], how="left", maintain_order="left_right")
    low, root, schema = lf._lower()
    (j,) = _join_nodes(low)
    assert len(j["keys"]) == 3 and len(j["keys_right"]) == 3
    ir, n_ir, ae, n_ae, keep = low.to_c()
    assert ir[root].n_keys == 3 and ir[root].n_keys_right == 3
    assert list(dict(schema)) == ["a", "u", "f", "x", "y"]           # the three right key columns are coalesced away


def test_left_on_right_on_lists_of_different_names():
    left, right = _frames(("ra", "ru", "rf"))
    low, root, schema = left.lazy().join(right.lazy(), left_on=["a", "u", "f"], right_on=["ra", "ru", "rf"])._lower()
    (j,) = _join_nodes(low)
    assert len(j["keys"]) == 3 and len(j["keys_right"]) == 3
    assert list(dict(schema)) == ["a", "u", "f", "x", "y"]


def test_polars_engine_passes_float_and_uint64_key_parts_on():
    left, right = _frames()
    low, root, _ = left.lazy().join(right.lazy(), on=["a", "u", "f"], how="inner", suffix="_r")._lower()
    nt = T.FakeTraverser(low, root)
    node = nt.view_current_node()
    assert type(node).__name__ == "Join" and len(node.left_on) == 3 and len(node.right_on) == 3
    back = eng.Translator(nt, frame_of=lambda n: n.df).plan()
    low2, _, schema2 = back._lower()
    (j,) = _join_nodes(low2)
    assert len(j["keys"]) == 3 and len(j["keys_right"]) == 3
    assert list(dict(schema2)) == ["a", "u", "f", "x", "y"]
