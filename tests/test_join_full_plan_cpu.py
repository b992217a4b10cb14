"""Full and right joins and the coalesce option at the boundary, no GPU needed: the mirror API accepts them and nothing else, the lowered IR node carries
plx_join_how / plx_ir.coalesce, collect_schema() follows the column rules of include/polars_amd.h, the trailing struct field sits where a C caller that
zero-initialises plx_ir expects it, the plan importer refuses what the contract refuses (before it needs a device) and the Polars attachment passes the options on."""
import ctypes as C
import os
import subprocess

import pytest

import polars_amd as pl
from polars_amd import _ffi as F
from polars_amd import polars_engine as eng
from tests import test_polars_engine_cpu as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOWS = {"inner": 0, "left": 1, "semi": 2, "anti": 3, "full": 4, "right": 5}
COALESCE = {None: 0, True: 1, False: 2}


def _join_nodes(low):
    return [d for d in low.irs if d["kind"] == F.IR_JOIN]


def _placeholder(name, dtype):
    return T.ph(name, dtype)


@pytest.fixture(scope="module")
def sides():
    L = pl.DataFrame([_placeholder("k", pl.Int64), _placeholder("a", pl.Int32), _placeholder("v", pl.Float64)])
    R = pl.DataFrame([_placeholder("k", pl.Int64), _placeholder("a", pl.Int32), _placeholder("w", pl.Float64)])
    return L, R


def _want_columns(how, coalesce):
    if how in ("semi", "anti"):
        return ["k", "a", "v"]
    merge = (how != "full") if coalesce is None else coalesce
    if not merge:
        return ["k", "a", "v", "k_right", "a_right", "w"]
    if how == "right":
        return ["a", "v", "k", "a_right", "w"]
    return ["k", "a", "v", "a_right", "w"]


@pytest.mark.parametrize("how", list(HOWS))
@pytest.mark.parametrize("coalesce", [None, True, False])
def test_every_kind_and_option_lowers_and_has_its_schema(sides, how, coalesce):
    L, R = sides
    lf = L.lazy().join(R.lazy(), on="k", how=how, coalesce=coalesce)
    low, root, _ = lf._lower()
    (j,) = _join_nodes(low)
    assert j["how"] == HOWS[how] and j["coalesce"] == COALESCE[coalesce]
    ir, n_ir, ae, n_ae, keep = low.to_c()
    assert ir[root].how == HOWS[how] and ir[root].coalesce == COALESCE[coalesce]
    schema = lf.collect_schema()
    assert list(schema) == _want_columns(how, coalesce)
    assert schema["k"] == pl.Int64 and (how in ("semi", "anti") or schema["w"] == pl.Float64)
    if "k_right" in schema:
        assert schema["k_right"] == pl.Int64
    # a projection above the join sees the same names (scan push-down walks the same rule)
    assert list(lf.select(*_want_columns(how, coalesce)).collect_schema()) == _want_columns(how, coalesce)
    # explain() keeps its shape
    text = L.lazy().join(R.lazy(), on="k", how=how, coalesce=coalesce, maintain_order="right" if how == "right" else "left").explain()
    assert f"Join[how={how}, maintain_order={'right' if how == 'right' else 'left'}]" in text, text


def test_expression_keys_do_not_coalesce(sides):
    L, R = sides
    lf = L.lazy().join(R.lazy(), left_on=pl.col("k") + 1, right_on="k", how="right")
    assert list(lf.collect_schema()) == ["k", "a", "v", "k_right", "a_right", "w"]
    lf = L.lazy().join(R.lazy(), left_on=["k", pl.col("a") * 2], right_on=["k", "a"], how="full", coalesce=True)
    assert list(lf.collect_schema()) == ["k", "a", "v", "a_right", "w"]


def test_bad_values_raise_at_call_time(sides):
    L, R = sides
    for bad in ("outer", "cross", "Full", "", None, 4):
        with pytest.raises(ValueError, match="how"):
            L.lazy().join(R.lazy(), on="k", how=bad)
    for bad in ("true", 1, 0, "none"):
        with pytest.raises(ValueError, match="coalesce"):
            L.lazy().join(R.lazy(), on="k", coalesce=bad)
    with pytest.raises(ValueError, match="coalesce"):
        L.join(R, on="k", how="full", coalesce="yes")              # DataFrame.join: before anything runs


def test_the_ffi_mirror_matches_the_header():
    assert (F.JOIN_INNER, F.JOIN_LEFT, F.JOIN_SEMI, F.JOIN_ANTI, F.JOIN_FULL, F.JOIN_RIGHT) == (0, 1, 2, 3, 4, 5)
    assert (F.JOIN_COALESCE_DEFAULT, F.JOIN_COALESCE, F.JOIN_KEEP_BOTH) == (0, 1, 2)
    assert F.IR._fields_[-1][0] == "coalesce" and F.IR._fields_[-2][0] == "slice_len"
    assert F.IR.coalesce.offset == F.IR.slice_len.offset + 8 and C.sizeof(F.IR) == F.IR.coalesce.offset + 8      # one int32 + tail padding of an 8-aligned struct
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert "pub coalesce: i32" in f.read()


def test_c_caller_that_zero_initialises_plx_ir_sees_the_trailing_field(tmp_path):
    """`plx_ir node = {0}` means "as before": coalesce = 0 is the join kind's default; the offsets are printed and compared with the ctypes mirror"""
    src = tmp_path / "join_full.c"
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include "polars_amd.h"
_Static_assert(PLX_JOIN_INNER == 0 && PLX_JOIN_LEFT == 1 && PLX_JOIN_SEMI == 2 && PLX_JOIN_ANTI == 3 && PLX_JOIN_FULL == 4 && PLX_JOIN_RIGHT == 5, "plx_join_how numbering");
_Static_assert(offsetof(plx_ir, coalesce) == offsetof(plx_ir, slice_len) + sizeof(int64_t), "coalesce is the trailing field, after slice_len");
int main(void) {
  plx_ir node = {0};
  if (node.coalesce != 0 || node.how != PLX_JOIN_INNER) return 1;
  node.kind = PLX_IR_JOIN;
  node.how = PLX_JOIN_FULL;
  node.coalesce = 2;
  if (plx_version() != ((PLX_ABI_MAJOR << 16) | PLX_ABI_MINOR)) return 10;
  printf("%zu %zu %zu\n", offsetof(plx_ir, slice_len), offsetof(plx_ir, coalesce), sizeof(plx_ir));
  return node.coalesce == 2 && node.how == 4 ? 0 : 2;
}
''')
    exe = tmp_path / "join_full"
    inc, libdir = os.path.join(ROOT, "include"), os.path.join(ROOT, "polars_amd")
    cmd = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", inc, str(src), "-o", str(exe), "-L", libdir, "-lpolars_amd", f"-Wl,-rpath,{libdir}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    assert [int(x) for x in run.stdout.split()] == [F.IR.slice_len.offset, F.IR.coalesce.offset, C.sizeof(F.IR)]


def _status(lf, **override):
    low, root, _ = lf._lower()
    _join_nodes(low)[0].update(override)
    ir, n_ir, ae, n_ae, keep = low.to_c()
    fus, sid = C.c_int32(), C.c_int32()
    why = C.create_string_buffer(512)
    rc = F.lib().plx_describe_fusion(ir, n_ir, ae, n_ae, root, C.byref(fus), C.byref(sid), why, 512)
    del keep
    return rc, F.lib().plx_last_error().decode()


def test_plan_import_refuses_by_status_code_before_it_needs_a_device():
    li, orders = T.frames()
    ERR_INVALID = 1
    def q(how, order="none", coalesce=None):
        return li.lazy().join(orders.lazy(), left_on="l_orderkey", right_on="o_orderkey", how=how, maintain_order=order, coalesce=coalesce).group_by("o_orderkey" if how == "right" else "l_orderkey").agg(pl.col("l_quantity").sum())
    for bad in (3, -1, 77):
        rc, msg = _status(q("full"), coalesce=bad)
        assert rc == ERR_INVALID and "coalesce" in msg, (rc, msg)
    for bad in (6, -1):
        rc, msg = _status(q("inner"), how=bad)
        assert rc == ERR_INVALID and "how" in msg, (rc, msg)
    for order in ("left", "left_right"):
        rc, msg = _status(q("right", order))
        assert rc == F.ERR_UNSUPPORTED and f"maintain_order={order}" in msg and "right join" in msg, (rc, msg)
    for order in ("right", "right_left"):                     # the left join's refusal stays as it is
        rc, msg = _status(q("left", order))
        assert rc == F.ERR_UNSUPPORTED and f"maintain_order={order}" in msg and "left join" in msg, (rc, msg)
    for how, order, coalesce in (("right", "right_left", None), ("right", "none", False), ("full", "left_right", True), ("full", "right", None), ("inner", "left", False), ("semi", "none", False)):
        rc, msg = _status(q(how, order, coalesce))
        assert rc == 0, (how, order, coalesce, rc, msg)


def test_fused_join_group_by_declines_full_right_and_keep_both_with_a_reason():
    li, orders = T.frames()
    def why(how, coalesce=None):
        lf = li.lazy().join(orders.lazy(), left_on="l_orderkey", right_on="o_orderkey", how=how, coalesce=coalesce).group_by("o_orderkey" if how == "right" else "l_orderkey").agg(pl.col("l_quantity").sum())
        low, root, _ = lf._lower()
        ir, n_ir, ae, n_ae, keep = low.to_c()
        fus, sid = C.c_int32(), C.c_int32()
        buf = C.create_string_buffer(512)
        rc = F.lib().plx_describe_fusion(ir, n_ir, ae, n_ae, root, C.byref(fus), C.byref(sid), buf, 512)
        assert rc == 0, F.lib().plx_last_error().decode()
        return fus.value, buf.value.decode()
    base_fus, base_why = why("inner")
    for how, coalesce, text in (("full", None, "full and right joins"), ("right", None, "full and right joins"), ("full", True, "full and right joins"), ("inner", False, "coalesce=false"),
                                ("left", False, "coalesce=false")):
        fus, reason = why(how, coalesce)
        assert fus == 0 and text in reason and "per-node route" in reason, (how, coalesce, fus, reason)
    assert why("inner", True) == (base_fus, base_why)             # coalesce = 1 on an inner join is the default: nothing about the fused pipelines changes


class OptionTraverser(T.FakeTraverser):
    """the stand-in traverser with join options of its own in the tuple visitor/nodes.rs hands over: (how, nulls_equal, slice, suffix, coalesce, maintain_order)"""

    def __init__(self, low, root, **opts):
        super().__init__(low, root)
        self.opts = opts

    def view_current_node(self):
        node = super().view_current_node()
        if type(node).__name__ == "Join":
            how, nulls_equal, jslice, suffix, coalesce, order = node.options
            o = self.opts
            node.options = (o.get("how", how), o.get("nulls_equal", nulls_equal), o.get("slice", jslice), suffix, o.get("coalesce", coalesce), o.get("order", order))
        return node


@pytest.mark.parametrize("how,coalesce,want", [("full", False, 0), ("right", True, 0), ("right", False, 2), ("inner", False, 2), ("left", False, 2), ("left", True, 0)])
def test_polars_engine_passes_the_kind_and_the_option_on(how, coalesce, want):
    """the optimized plan carries `coalesce` resolved to a bool: a value equal to the kind's default goes on as 0, the other one as 1 / 2"""
    li, orders = T.frames()
    low, root, _ = li.lazy().join(orders.lazy(), left_on="l_orderkey", right_on="o_orderkey", suffix="_o")._lower()
    back = eng.Translator(OptionTraverser(low, root, how=how, coalesce=coalesce), frame_of=lambda node: node.df).plan()
    low2, _, _ = back._lower()
    (j,) = _join_nodes(low2)
    assert j["how"] == HOWS[how] and j["coalesce"] == want and j["suffix"] == "_o"
    assert ("o_orderkey" in back.collect_schema()) == (not coalesce or how == "right")


def test_polars_engine_still_refuses_nulls_equal_a_slice_and_the_orders_the_engine_refuses():
    li, orders = T.frames()
    low, root, _ = li.lazy().join(orders.lazy(), left_on="l_orderkey", right_on="o_orderkey")._lower()
    for how in ("full", "right", "inner"):
        with pytest.raises(eng.NotSupported, match="nulls_equal=True"):
            eng.Translator(OptionTraverser(low, root, how=how, coalesce=how != "full", nulls_equal=True), frame_of=lambda node: node.df).plan()
        with pytest.raises(eng.NotSupported, match="slice="):
            eng.Translator(OptionTraverser(low, root, how=how, coalesce=how != "full", slice=(0, 10)), frame_of=lambda node: node.df).plan()
    for order in ("left", "left_right"):
        with pytest.raises(eng.NotSupported, match="maintain_order"):
            eng.Translator(OptionTraverser(low, root, how="right", order=order), frame_of=lambda node: node.df).plan()
    with pytest.raises(eng.NotSupported, match="how=cross"):
        eng.Translator(OptionTraverser(low, root, how="cross"), frame_of=lambda node: node.df).plan()


def test_new_join_kernels_do_not_spill_and_the_other_kinds_keep_their_count_kernels():
    """the flag store lives in count kernels of its own (join_full_count_kernel / join_wide_full_count_kernel); the mask, append and coalescing kernels use no scratch"""
    from tests.test_kernel_resources_cpu import resource_usage
    res = resource_usage("kernels_join.hip")
    for part in ("join_count_kernel", "join_full_count_kernel", "join_unmatched_mask_kernel", "join_append_unmatched_kernel"):
        assert sum(part in name for name in res) == 1, (part, sorted(res))
    assert sum("coalesce_key_kernel" in name for name in res) == 4, sorted(res)           # element widths 1, 2, 4, 8
    for name, r in res.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
    res = resource_usage("kernels_join_wide.hip")
    for part in ("join_wide_count_kernel", "join_wide_full_count_kernel"):
        assert sum(part in name for name in res) == 1, (part, sorted(res))
    for name, r in res.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs"]) <= 128, (name, r)


def test_keys_of_different_dtypes_are_cast_and_do_not_coalesce_on_right_and_full_joins():
    """lowering casts such keys to their supertype; the engine merges plain columns only, so the schema keeps both key columns (inner / left: the rule they had)"""
    L = pl.DataFrame([_placeholder("k", pl.Int32), _placeholder("v", pl.Float64)])
    R = pl.DataFrame([_placeholder("k", pl.Int64), _placeholder("w", pl.Float64)])
    for how, coalesce in (("right", None), ("right", True), ("full", True)):
        lf = L.lazy().join(R.lazy(), on="k", how=how, coalesce=coalesce)
        low, root, _ = lf._lower()
        (j,) = _join_nodes(low)
        assert low.aexprs[j["keys"][0]]["kind"] == F.AE_CAST and low.aexprs[j["keys_right"][0]]["kind"] == F.AE_COLUMN
        schema = lf.collect_schema()
        assert list(schema) == ["k", "v", "k_right", "w"] and schema["k"] == pl.Int32 and schema["k_right"] == pl.Int64, (how, coalesce, schema)
    same = pl.DataFrame([_placeholder("k", pl.Int64), _placeholder("v", pl.Float64)])
    assert list(same.lazy().join(R.lazy(), on="k", how="right").collect_schema()) == ["v", "k", "w"]
