"""Join maintain_order at the boundary, no GPU needed: the mirror API accepts the five orders of the reference's JoinArgs.maintain_order and nothing else, the
lowered IR node carries plx_join_order, explain() names it, the scan push-down keeps it, the Polars attachment passes it on, the C header exports the enumerators
and the engine refuses what the contract in include/polars_amd.h refuses (before it needs a device)."""
import ctypes as C
import os
import subprocess

import pytest

import polars_amd as pl
from polars_amd import _ffi as F
from polars_amd import io as plio
from polars_amd import plan as P
from polars_amd import polars_engine as eng
from tests import test_polars_engine_cpu as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = {"none": 0, "left": 1, "right": 2, "left_right": 3, "right_left": 4}


def _join_nodes(low):
    return [d for d in low.irs if d["kind"] == F.IR_JOIN]


@pytest.mark.parametrize("order", list(ORDERS))
def test_join_accepts_the_five_orders_and_lowers_them(order):
    li, orders = T.frames()
    lf = li.lazy().join(orders.lazy(), left_on="l_orderkey", right_on="o_orderkey", maintain_order=order)
    low, root, _ = lf._lower()
    (j,) = _join_nodes(low)
    assert j["maintain_order"] == ORDERS[order]
    ir, n_ir, ae, n_ae, keep = low.to_c()
    assert ir[root].maintain_order == ORDERS[order]
    text = lf.explain()
    if order == "none":
        assert "maintain_order" not in text
    else:
        assert f"maintain_order={order}" in text, text


def test_join_rejects_an_unknown_order_at_call_time():
    li, orders = T.frames()
    for bad in ("Left", "both", "", None, True):
        with pytest.raises(ValueError, match="maintain_order"):
            li.lazy().join(orders.lazy(), left_on="l_orderkey", right_on="o_orderkey", maintain_order=bad)
    with pytest.raises(ValueError, match="maintain_order"):
        li.join(orders, left_on="l_orderkey", right_on="o_orderkey", maintain_order="sideways")     # DataFrame.join: before anything runs


def test_default_is_none_and_the_ffi_constants_match_the_header():
    li, orders = T.frames()
    low, _, _ = li.lazy().join(orders.lazy(), left_on="l_orderkey", right_on="o_orderkey")._lower()
    assert _join_nodes(low)[0]["maintain_order"] == 0
    assert (F.JOIN_ORDER_NONE, F.JOIN_ORDER_LEFT, F.JOIN_ORDER_RIGHT, F.JOIN_ORDER_LEFT_RIGHT, F.JOIN_ORDER_RIGHT_LEFT) == (0, 1, 2, 3, 4)
    assert P.JOIN_ORDERS == ORDERS


def test_push_down_over_scan_and_join_keeps_the_order():
    li, orders = T.frames()
    c = pl.col
    lf = (li.lazy().filter(c("l_quantity") > 3).join(orders.lazy().filter(c("o_shippriority") == 0), left_on="l_orderkey", right_on="o_orderkey", how="left", maintain_order="left_right")
          .select("l_orderkey", "o_custkey").head(10))
    plio.push_down(lf._node)
    plio.push_down(lf._node, {"l_orderkey"}, None)
    low, _, _ = lf._lower()
    assert _join_nodes(low)[0]["maintain_order"] == F.JOIN_ORDER_LEFT_RIGHT
    assert "Join[how=left, maintain_order=left_right]" in lf.explain()


class OrderedTraverser(T.FakeTraverser):
    """the stand-in traverser with a join order in the options tuple, as visitor/nodes.rs hands it over"""

    def __init__(self, low, root, order):
        super().__init__(low, root)
        self.order = order

    def view_current_node(self):
        node = super().view_current_node()
        if type(node).__name__ == "Join":
            how, nulls_equal, jslice, suffix, coalesce, _ = node.options
            node.options = (how, nulls_equal, jslice, suffix, coalesce, self.order)
        return node


@pytest.mark.parametrize("how,order", [("inner", "left_right"), ("inner", "right"), ("left", "left"), ("semi", "right_left")])
def test_polars_engine_passes_the_join_order_on(how, order):
    li, orders = T.frames()
    low, root, _ = li.lazy().join(orders.lazy(), left_on="l_orderkey", right_on="o_orderkey", how=how, suffix="_o")._lower()
    nt = OrderedTraverser(low, root, order)
    assert nt.view_current_node().options == (how, False, None, "_o", True, order)
    back = eng.Translator(nt, frame_of=lambda node: node.df).plan()
    low2, _, _ = back._lower()
    assert _join_nodes(low2)[0]["maintain_order"] == ORDERS[order]
    assert f"maintain_order={order}" in back.explain()


def test_polars_engine_leaves_what_the_engine_refuses_to_the_cpu_engine():
    li, orders = T.frames()
    low, root, _ = li.lazy().join(orders.lazy(), left_on="l_orderkey", right_on="o_orderkey", how="left")._lower()
    for order in ("right", "right_left", "sideways"):
        with pytest.raises(eng.NotSupported, match="maintain_order"):
            eng.Translator(OrderedTraverser(low, root, order), frame_of=lambda node: node.df).plan()


def _status(lf, order_override=None):
    low, root, _ = lf._lower()
    if order_override is not None:
        _join_nodes(low)[0]["maintain_order"] = order_override
    ir, n_ir, ae, n_ae, keep = low.to_c()
    fus, sid = C.c_int32(), C.c_int32()
    why = C.create_string_buffer(512)
    rc = F.lib().plx_describe_fusion(ir, n_ir, ae, n_ae, root, C.byref(fus), C.byref(sid), why, 512)
    del keep
    return rc, F.lib().plx_last_error().decode()


def test_engine_refuses_by_status_code_before_it_needs_a_device():
    """the plan importer checks plx_join_order: outside 0..4 -> PLX_ERR_INVALID, left join + right* -> PLX_ERR_UNSUPPORTED naming the option; never ignored"""
    li, orders = T.frames()
    ERR_INVALID = 1
    inner = li.lazy().join(orders.lazy(), left_on="l_orderkey", right_on="o_orderkey").group_by("l_orderkey").agg(pl.col("l_quantity").sum())
    for bad in (5, -1, 77):
        rc, msg = _status(inner, bad)
        assert rc == ERR_INVALID and "maintain_order" in msg, (rc, msg)
    for order in ("right", "right_left"):
        left = li.lazy().join(orders.lazy(), left_on="l_orderkey", right_on="o_orderkey", how="left", maintain_order=order).group_by("l_orderkey").agg(pl.col("l_quantity").sum())
        rc, msg = _status(left)
        assert rc == F.ERR_UNSUPPORTED and f"maintain_order={order}" in msg, (rc, msg)
    for how, order in (("left", "left_right"), ("inner", "right_left"), ("semi", "right")):
        ok = li.lazy().join(orders.lazy(), left_on="l_orderkey", right_on="o_orderkey", how=how, maintain_order=order).group_by("l_orderkey").agg(pl.col("l_quantity").sum())
        rc, msg = _status(ok)
        assert rc == 0, (rc, msg)


def test_c_header_exports_the_join_orders(tmp_path):
    src = tmp_path / "join_order.c"
    src.write_text(r'''
#include "polars_amd.h"
_Static_assert(PLX_JOIN_ORDER_NONE == 0 && PLX_JOIN_ORDER_LEFT == 1 && PLX_JOIN_ORDER_RIGHT == 2 && PLX_JOIN_ORDER_LEFT_RIGHT == 3 && PLX_JOIN_ORDER_RIGHT_LEFT == 4,
               "plx_join_order numbering");
int main(void) {
  plx_ir node = {0};
  plx_join_order o = PLX_JOIN_ORDER_LEFT_RIGHT;
  node.kind = PLX_IR_JOIN;
  node.maintain_order = (int32_t)o;
  if (plx_version() != ((PLX_ABI_MAJOR << 16) | PLX_ABI_MINOR)) return 10;
  return node.maintain_order == 3 ? 0 : 1;
}
''')
    exe = tmp_path / "join_order"
    inc, libdir = os.path.join(ROOT, "include"), os.path.join(ROOT, "polars_amd")
    cmd = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", inc, str(src), "-o", str(exe), "-L", libdir, "-lpolars_amd", f"-Wl,-rpath,{libdir}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)


def test_ordering_kernels_do_not_spill():
    """the new __global__ functions (pack / unpack / run ordering) and the key-only radix scatter: no scratch, and the key-only scatter stages 34 KB of LDS, not 50"""
    from tests.test_kernel_resources_cpu import resource_usage
    res = resource_usage("kernels_join_order.hip")
    assert {n for n in res if "pair_pack" in n or "pair_unpack" in n or "run_order" in n}.__len__() == 3, sorted(res)
    for name, r in res.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
    res = resource_usage("kernels_sort.hip")
    keyonly = [r for n, r in res.items() if "radix_scatter_kernel" in n and "ILb0" in n]
    payload = [r for n, r in res.items() if "radix_scatter_kernel" in n and "ILb1" in n]
    assert len(keyonly) == 1 and len(payload) == 1, sorted(res)
    assert int(keyonly[0]["ScratchSize [bytes/lane]"]) == 0 and int(payload[0]["ScratchSize [bytes/lane]"]) == 0
    assert int(keyonly[0]["LDS Size [bytes/block]"]) < int(payload[0]["LDS Size [bytes/block]"]) <= 64 * 1024
