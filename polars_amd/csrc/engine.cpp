// engine.cpp -- plan import, dtype inference, the materialising evaluator, the fused
// pipeline compiler and the executors.  See engine.hpp for the reference mapping.
#include "engine.hpp"

#include "asof.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <functional>
#include <memory>
#include <numeric>
#include <optional>
#include <set>
#include <sstream>

#include "cumulative.hpp"
#include "distinct.hpp"
#include "encoded_inputs.hpp"
#include "fused_shapes.hpp"
#include "groupby_tail.hpp"
#include "jit.hpp"
#include "join.hpp"
#include "kernels.hpp"
#include "kernels_fused.hpp"
#include "ops.hpp"
#include "quantile.hpp"
#include "rolling.hpp"
#include "sort.hpp"
#include "temporal.hpp"
#include "variance.hpp"

namespace plx {
namespace engine {

using namespace fused;

struct Unsupported : std::exception {
  std::string why;
  explicit Unsupported(std::string w) : why(std::move(w)) {}
  const char* what() const noexcept override { return why.c_str(); }
};

// ------------------------------------------------------------------ import ----
Plan import_plan(const plx_ir* ir, int n_ir, const plx_aexpr* ae, int n_ae, uint32_t flags) {
  Plan p;
  p.flags = flags;
  PLX_REQUIRE(ir && n_ir > 0, PLX_ERR_INVALID, "execute_plan: empty IR arena");
  for (int i = 0; i < n_ae; i++) {
    AE e;
    e.kind = ae[i].kind; e.op = ae[i].op; e.lhs = ae[i].lhs; e.rhs = ae[i].rhs; e.dtype = ae[i].dtype; e.is_null = ae[i].is_null; e.lit = ae[i].lit;
    if (ae[i].name) e.name = ae[i].name;
    if (e.kind == PLX_AE_TERNARY) {
      e.cond = ae[i].cond;
      PLX_REQUIRE(e.cond >= 0 && e.lhs >= 0 && e.rhs >= 0, PLX_ERR_INVALID, "ternary expression needs a predicate (cond), a then (lhs) and an otherwise (rhs) input");
    }
    if (e.kind == PLX_AE_BITMAP_LOOKUP) {
      PLX_REQUIRE(e.lhs >= 0, PLX_ERR_INVALID, "bitmap lookup needs an integer input (lhs)");
      e.lut = get_column(ae[i].lit.u);
      PLX_REQUIRE(e.lut->dtype == PLX_BOOL, PLX_ERR_INVALID, "bitmap lookup: the lookup bitmap must be a Boolean column");
      PLX_REQUIRE(!e.lut->validity || e.lut->null_count == 0 || (e.lut->values && column_null_count(e.lut) == 0), PLX_ERR_INVALID, "bitmap lookup: the lookup bitmap must not hold nulls");
    }
    if (e.kind == PLX_AE_TEMPORAL) {
      PLX_REQUIRE(e.lhs >= 0, PLX_ERR_INVALID, "date part needs a Date / Datetime input (lhs)");
      PLX_REQUIRE(e.lit.u < (uint64_t)temporal::kNumUnits && temporal::part_ok(e.op, (int)e.lit.u), PLX_ERR_INVALID,
                  "date part: part " + std::to_string(e.op) + " of unit " + std::to_string((long long)e.lit.i) + " (plx_temporal_part_kind 0..9, plx_time_unit 0..3; the time of day and date() exist for a Datetime only)");
    }
    if (e.kind == PLX_AE_AGG && (e.op == PLX_AGG_VAR || e.op == PLX_AGG_STD))
      PLX_REQUIRE(e.lhs >= 0 && e.lit.u <= 255, PLX_ERR_INVALID, "var / std: the node carries ddof 0..255 in lit.u, got " + std::to_string((long long)e.lit.i));
    if (e.kind == PLX_AE_AGG && e.op == PLX_AGG_QUANTILE)
      PLX_REQUIRE(e.lhs >= 0 && quantile::q_ok(e.lit.f64) && quantile::interpolation_ok(e.dtype), PLX_ERR_INVALID,
                  "quantile: the node carries q in [0, 1] in lit.f64 and a plx_quantile_interpolation 0..4 in its dtype slot, got q=" + std::to_string(e.lit.f64) + ", interpolation=" + std::to_string(e.dtype));
    PLX_REQUIRE(e.lhs < i && e.rhs < i && e.cond < i, PLX_ERR_INVALID, "AExpr arena must be topologically ordered (children before parents)");
    if (e.kind == PLX_AE_WINDOW_KEY) {
      PLX_REQUIRE(e.lhs >= 0, PLX_ERR_INVALID, "window key link needs a key expression (lhs)");
      PLX_REQUIRE(e.rhs < 0 || ae[e.rhs].kind == PLX_AE_WINDOW_KEY, PLX_ERR_INVALID, "window key link: rhs must be the next link or -1");
    }
    if (e.kind == PLX_AE_WINDOW) {
      PLX_REQUIRE(e.lhs >= 0, PLX_ERR_INVALID, "window expression needs a function (lhs)");
      PLX_REQUIRE(e.rhs >= 0 && ae[e.rhs].kind == PLX_AE_WINDOW_KEY, PLX_ERR_INVALID, "window expression without a key: rhs must be the first PLX_AE_WINDOW_KEY link");
      int n_links = 0;
      for (int l = e.rhs; l >= 0; l = ae[l].rhs) n_links++;
      PLX_REQUIRE(n_links <= window::kMaxKeys, PLX_ERR_UNSUPPORTED, "window over " + std::to_string(n_links) + " keys; a window takes 1.." + std::to_string(window::kMaxKeys) + " keys on this path");
    }
    if (e.kind == PLX_AE_CUMULATIVE) {
      PLX_REQUIRE(e.lhs >= 0, PLX_ERR_INVALID, "cumulative expression needs an operand (lhs)");
      PLX_REQUIRE(cumulative::op_ok(e.op), PLX_ERR_INVALID, "cumulative expression: op " + std::to_string(e.op) + " is no plx_cum_op (0 = sum, 1 = min, 2 = max, 3 = count)");
      PLX_REQUIRE(e.lit.u <= 1, PLX_ERR_INVALID, "cumulative expression: reverse rides in lit.u as 0 / 1, got " + std::to_string((long long)e.lit.i));
    }
    if (e.kind == PLX_AE_RANK) {
      PLX_REQUIRE(e.lhs >= 0, PLX_ERR_INVALID, "rank expression needs an operand (lhs)");
      PLX_REQUIRE(cumulative::method_ok(e.op), PLX_ERR_INVALID, "rank expression: method " + std::to_string(e.op) + " is no plx_rank_method (0 = average, 1 = min, 2 = max, 3 = dense, 4 = ordinal)");
      PLX_REQUIRE(e.lit.u <= 1, PLX_ERR_INVALID, "rank expression: descending rides in lit.u as 0 / 1, got " + std::to_string((long long)e.lit.i));
    }
    if (e.kind == PLX_AE_SHIFT) {
      PLX_REQUIRE(e.lhs >= 0, PLX_ERR_INVALID, "shift / diff expression needs an operand (lhs)");
      PLX_REQUIRE(e.op == 0 || e.op == 1, PLX_ERR_INVALID, "shift / diff expression: op " + std::to_string(e.op) + " is neither 0 (shift) nor 1 (diff)");
      PLX_REQUIRE(e.rhs < 0 || (e.op == 0 && e.rhs < i && ae[e.rhs].kind == PLX_AE_LITERAL && !ae[e.rhs].is_null), PLX_ERR_INVALID,
                  "shift expression: fill_value (rhs) must be a non-null literal node or -1, and diff takes none");
    }
    if (e.kind == PLX_AE_ROLLING) {
      PLX_REQUIRE(e.lhs >= 0, PLX_ERR_INVALID, "rolling expression needs an operand (lhs)");
      PLX_REQUIRE(rolling::op_ok(e.op), PLX_ERR_INVALID, "rolling expression: op " + std::to_string(e.op) + " is no plx_rolling_op (0 = sum, 1 = mean, 2 = min, 3 = max)");
      const rolling::Params rp = rolling::unpack_params(e.lit.u);
      PLX_REQUIRE(rp.window >= 1 && rp.window <= 0x7fffffffull, PLX_ERR_INVALID, "rolling expression: window_size (lit.u bits 0..31) must be at least 1 and below 2^31, got " + std::to_string((long long)rp.window));
      PLX_REQUIRE(rp.min_samples >= 1 && rp.min_samples <= rp.window, PLX_ERR_INVALID, "rolling expression: min_samples (lit.u bits 32..62) must lie in 1..window_size, got " + std::to_string((long long)rp.min_samples));
    }
    p.ae.push_back(std::move(e));
  }
  // a key link stands below a window (as its rhs) or below another link (as its rhs), nowhere else
  for (int i = 0; i < n_ae; i++) {
    const AE& e = p.ae[i];
    auto is_link = [&](int c) { return c >= 0 && p.ae[c].kind == PLX_AE_WINDOW_KEY; };
    const bool takes_links = e.kind == PLX_AE_WINDOW || e.kind == PLX_AE_WINDOW_KEY;
    PLX_REQUIRE(!is_link(e.lhs) && !is_link(e.cond) && (takes_links || !is_link(e.rhs)), PLX_ERR_INVALID, "window key link outside a window expression's key list");
  }
  for (int i = 0; i < n_ir; i++) {
    IRN n;
    n.kind = ir[i].kind; n.input = ir[i].input; n.input_right = ir[i].input_right; n.predicate = ir[i].predicate; n.frame = ir[i].frame;
    for (int j = 0; j < ir[i].n_exprs; j++) n.exprs.push_back(ir[i].exprs[j]);
    for (int j = 0; j < ir[i].n_keys; j++) n.keys.push_back(ir[i].keys[j]);
    for (int j = 0; j < ir[i].n_keys_right; j++) n.keys_right.push_back(ir[i].keys_right[j]);
    n.how = ir[i].how; n.maintain_order = ir[i].maintain_order;
    if (n.kind == PLX_IR_JOIN) {
      // plx_join_order: never silently ignored
      PLX_REQUIRE(n.maintain_order >= PLX_JOIN_ORDER_NONE && n.maintain_order <= PLX_JOIN_ORDER_RIGHT_LEFT, PLX_ERR_INVALID, "join: maintain_order outside 0..4 (plx_join_order)");
      PLX_REQUIRE(!(n.how == PLX_JOIN_LEFT && (n.maintain_order == PLX_JOIN_ORDER_RIGHT || n.maintain_order == PLX_JOIN_ORDER_RIGHT_LEFT)), PLX_ERR_UNSUPPORTED,
                  std::string("left join with maintain_order=") + join::join_order_name(n.maintain_order) + ": only maintain_order none / left / left_right are on this path for a left join");
      PLX_REQUIRE(!(n.how == PLX_JOIN_RIGHT && (n.maintain_order == PLX_JOIN_ORDER_LEFT || n.maintain_order == PLX_JOIN_ORDER_LEFT_RIGHT)), PLX_ERR_UNSUPPORTED,
                  std::string("right join with maintain_order=") + join::join_order_name(n.maintain_order) + ": only maintain_order none / right / right_left are on this path for a right join");
      PLX_REQUIRE(n.how >= PLX_JOIN_INNER && n.how <= PLX_JOIN_RIGHT, PLX_ERR_INVALID, "join: how outside 0..5 (plx_join_how)");
      n.coalesce = ir[i].coalesce;
      PLX_REQUIRE(n.coalesce >= 0 && n.coalesce <= 2, PLX_ERR_INVALID, "join: coalesce outside 0..2 (0 = the join kind's default, 1 = coalesce, 2 = keep both key columns)");
    }
    if (n.kind == PLX_IR_JOIN_ASOF) {
      // everything that can be refused without a device is refused here
      PLX_REQUIRE(asof::how_ok(n.how), PLX_ERR_INVALID, "join_asof: strategy " + std::to_string(n.how) + " in the how slot is no plx_asof_strategy (0 = backward, 1 = forward, 2 = nearest), optionally OR'd with PLX_ASOF_STRICT (4)");
      PLX_REQUIRE(n.input >= 0 && n.input_right >= 0, PLX_ERR_INVALID, "join_asof needs two inputs");
      PLX_REQUIRE(!n.keys.empty() && n.keys.size() == n.keys_right.size(), PLX_ERR_INVALID,
                  "join_asof: " + std::to_string(n.keys.size()) + " left keys against " + std::to_string(n.keys_right.size()) + " right keys (the by parts, then `on`: at least one, the same number on both sides)");
      PLX_REQUIRE((int)n.keys.size() <= asof::kMaxWords, PLX_ERR_UNSUPPORTED,
                  "join_asof: " + std::to_string(n.keys.size()) + " keys; an as-of join takes `on` and 0.." + std::to_string(asof::kMaxBy) + " by parts on this path");
      PLX_REQUIRE(n.maintain_order == 0, PLX_ERR_INVALID, "join_asof: maintain_order must be 0 (the result is always in left row order), got " + std::to_string(n.maintain_order));
      n.coalesce = ir[i].coalesce;
      PLX_REQUIRE(n.coalesce >= 0 && n.coalesce <= 2, PLX_ERR_INVALID, "join_asof: coalesce outside 0..2 (0 = the default, 1 = coalesce, 2 = keep both key columns)");
      if (n.predicate != -1) {
        PLX_REQUIRE(n.predicate >= 0 && n.predicate < n_ae && p.ae[n.predicate].kind == PLX_AE_LITERAL && !p.ae[n.predicate].is_null, PLX_ERR_INVALID,
                    "join_asof: the tolerance (the predicate slot) must be the index of a non-null literal node, or -1");
        const AE& t = p.ae[n.predicate];
        const bool negative = dtype_is_float(t.dtype) ? !((t.dtype == PLX_F32 ? (double)t.lit.f32 : t.lit.f64) >= 0.0) : dtype_is_signed(t.dtype) && t.lit.i < 0;
        PLX_REQUIRE(!negative, PLX_ERR_INVALID, "join_asof: the tolerance must be a number >= 0, got " + (dtype_is_float(t.dtype) ? std::to_string(t.dtype == PLX_F32 ? (double)t.lit.f32 : t.lit.f64) : std::to_string((long long)t.lit.i)));
      }
    }
    if (n.kind == PLX_IR_DISTINCT) {
      PLX_REQUIRE(distinct::keep_ok(n.how), PLX_ERR_INVALID, "distinct: keep " + std::to_string(n.how) + " in the how slot is no plx_unique_keep (0 = any, 1 = first, 2 = last, 3 = none)");
      PLX_REQUIRE(n.maintain_order == 0 || n.maintain_order == 1, PLX_ERR_INVALID, "distinct: maintain_order outside 0 / 1");
      PLX_REQUIRE(n.input >= 0 && !n.keys.empty(), PLX_ERR_INVALID, "distinct needs an input and at least one subset column");
      PLX_REQUIRE((int)n.keys.size() <= sort::kSegmentMaxKeys, PLX_ERR_UNSUPPORTED,
                  "distinct: a subset of " + std::to_string(n.keys.size()) + " columns; the subset takes 1.." + std::to_string(sort::kSegmentMaxKeys) + " columns on this path");
    }
    if (ir[i].suffix) n.suffix = ir[i].suffix;
    if (n.kind == PLX_IR_SORT) {
      for (int j = 0; j < ir[i].n_keys; j++) {
        n.sort_descending.push_back(ir[i].sort_descending ? ir[i].sort_descending[j] : 0);
        n.sort_nulls_last.push_back(ir[i].sort_nulls_last ? ir[i].sort_nulls_last[j] : 0);
      }
    }
    n.slice_offset = ir[i].slice_offset; n.slice_len = ir[i].slice_len;
    auto chk = [&](int e) { PLX_REQUIRE(e >= 0 && e < n_ae, PLX_ERR_INVALID, "IR node references an expression outside the arena"); };
    for (int e : n.exprs) chk(e);
    for (int e : n.keys) chk(e);
    for (int e : n.keys_right) chk(e);
    if (n.kind == PLX_IR_FILTER) chk(n.predicate);
    auto no_link = [&](int e) { PLX_REQUIRE(e < 0 || p.ae[e].kind != PLX_AE_WINDOW_KEY, PLX_ERR_INVALID, "window key link outside a window expression's key list"); };
    for (int e : n.exprs) no_link(e);
    for (int e : n.keys) no_link(e);
    for (int e : n.keys_right) no_link(e);
    no_link(n.predicate);
    if (n.kind == PLX_IR_GROUPBY) {
      std::function<bool(int)> has_window = [&](int e) { return e >= 0 && (p.ae[e].kind == PLX_AE_WINDOW || has_window(p.ae[e].lhs) || has_window(p.ae[e].rhs) || has_window(p.ae[e].cond)); };
      for (int e : n.keys) PLX_REQUIRE(!has_window(e), PLX_ERR_INVALID, "group_by: a window expression (.over) cannot stand in the keys of a group_by");
      for (int e : n.exprs) PLX_REQUIRE(!has_window(e), PLX_ERR_INVALID, "group_by: a window expression (.over) cannot stand in the aggregate list of a group_by; aggregate first, or use the window in select / with_columns");
      std::function<bool(int)> has_rowfn = [&](int e) { return e >= 0 && (p.ae[e].kind == PLX_AE_CUMULATIVE || p.ae[e].kind == PLX_AE_RANK || p.ae[e].kind == PLX_AE_SHIFT || p.ae[e].kind == PLX_AE_ROLLING || has_rowfn(p.ae[e].lhs) || has_rowfn(p.ae[e].rhs) || has_rowfn(p.ae[e].cond)); };
      for (int e : n.keys) PLX_REQUIRE(!has_rowfn(e), PLX_ERR_INVALID, "group_by: a cumulative / ranking expression (cum_sum, cum_min, cum_max, cum_count, rank) or a shift / diff / rolling expression cannot stand in the keys of a group_by; compute it in with_columns first");
      for (int e : n.exprs) PLX_REQUIRE(!has_rowfn(e), PLX_ERR_INVALID, "group_by: a cumulative / ranking expression (cum_sum, cum_min, cum_max, cum_count, rank) or a shift / diff / rolling expression cannot stand in the aggregate list of a group_by; it keeps one value per row -- use it in select / with_columns, with .over(keys) for partitions");
    }
    PLX_REQUIRE(n.input < i && n.input_right < i, PLX_ERR_INVALID, "IR arena must be topologically ordered (inputs before consumers)");
    p.ir.push_back(std::move(n));
  }
  return p;
}

// -------------------------------------------------------------- dtype rules ----
static int sum_out_dtype(int dt) {
  switch (dt) {
    case PLX_BOOL: return PLX_U32;
    case PLX_I8: case PLX_I16: case PLX_U8: case PLX_U16: return PLX_I64;
    default: return dt;
  }
}
static bool is_cmp_op(int op) { return op >= PLX_OP_EQ && op <= PLX_OP_GE; }
static bool is_arith_op(int op) { return op >= PLX_OP_PLUS && op <= PLX_OP_MODULUS; }
static bool is_logic_op(int op) { return op >= PLX_OP_AND && op <= PLX_OP_XOR; }

// the physical dtype a PLX_AE_TEMPORAL node's unit asks of its operand
static int temporal_input_dtype(const AE& x) { return (int)x.lit.u == temporal::kUnitDate ? PLX_I32 : PLX_I64; }

int infer_dtype(const Plan& plan, int e, const Frame& schema) {
  const AE& x = plan.ae.at(e);
  switch (x.kind) {
    case PLX_AE_COLUMN: {
      int i = schema.find(x.name);
      if (i < 0) fail(PLX_ERR_NOT_FOUND, "column not found: " + x.name);
      return schema.cols[i]->dtype;
    }
    case PLX_AE_LITERAL: return x.dtype;
    case PLX_AE_ALIAS: return infer_dtype(plan, x.lhs, schema);
    case PLX_AE_CAST: return x.dtype;
    case PLX_AE_NOT: case PLX_AE_IS_NULL: case PLX_AE_IS_NOT_NULL: return PLX_BOOL;
    case PLX_AE_FILL_NULL: return infer_dtype(plan, x.lhs, schema);
    case PLX_AE_BITMAP_LOOKUP: {
      const int in = infer_dtype(plan, x.lhs, schema);
      PLX_REQUIRE(dtype_is_int(in), PLX_ERR_INVALID, std::string("bitmap lookup: the input must be an integer expression, not ") + dtype_name(in));
      return PLX_BOOL;
    }
    case PLX_AE_TEMPORAL: {
      const int in = infer_dtype(plan, x.lhs, schema);
      PLX_REQUIRE(in == temporal_input_dtype(x), PLX_ERR_INVALID, std::string("date part: a Date is an Int32 expression and a Datetime an Int64 expression, not ") + dtype_name(in) + " (unit " + std::to_string((int)x.lit.u) + ")");
      return ops::temporal_part_dtype(x.op);
    }
    case PLX_AE_TERNARY: {
      const int l = infer_dtype(plan, x.lhs, schema), r = infer_dtype(plan, x.rhs, schema);
      PLX_REQUIRE(infer_dtype(plan, x.cond, schema) == PLX_BOOL, PLX_ERR_INVALID, "when/then/otherwise: the predicate must be Boolean");
      PLX_REQUIRE(l == r, PLX_ERR_INVALID, std::string("when/then/otherwise branches have different dtypes (") + dtype_name(l) + ", " + dtype_name(r) + "); the optimizer's type coercion must insert casts");
      return l;
    }
    case PLX_AE_LEN: return PLX_U32;
    case PLX_AE_WINDOW: return infer_dtype(plan, x.lhs, schema);      // the dtype the function has in a group-by
    case PLX_AE_CUMULATIVE: {
      const int in = infer_dtype(plan, x.lhs, schema);
      const int out = cumulative::result_dtype(x.op, in);
      if (out < 0) fail(PLX_ERR_UNSUPPORTED, std::string(cumulative::op_name(x.op)) + " of a " + dtype_name(in) + " expression: integer, float and Boolean operands only");
      return out;
    }
    case PLX_AE_RANK: infer_dtype(plan, x.lhs, schema); return cumulative::rank_dtype(x.op);
    case PLX_AE_SHIFT: {
      const int in = infer_dtype(plan, x.lhs, schema);
      const int out = x.op == 1 ? rolling::diff_dtype(in) : (in >= PLX_BOOL && in <= PLX_F64 ? in : -1);
      if (out < 0) fail(PLX_ERR_UNSUPPORTED, std::string(x.op == 1 ? "diff" : "shift") + " of a " + dtype_name(in) + " expression: " + (x.op == 1 ? "integer and float operands only" : "integer, float and Boolean operands only"));
      if (x.rhs >= 0) PLX_REQUIRE(plan.ae.at(x.rhs).dtype == in, PLX_ERR_INVALID, std::string("shift: the fill_value literal's dtype ") + dtype_name(plan.ae.at(x.rhs).dtype) + " differs from the operand's " + dtype_name(in));
      return out;
    }
    case PLX_AE_ROLLING: {
      const int in = infer_dtype(plan, x.lhs, schema);
      const int out = rolling::result_dtype(x.op, in);
      if (out < 0) fail(PLX_ERR_UNSUPPORTED, std::string(rolling::op_name(x.op)) + " of a " + dtype_name(in) + " expression: integer, float and Boolean operands only");
      return out;
    }
    case PLX_AE_AGG: {
      int in = infer_dtype(plan, x.lhs, schema);
      switch (x.op) {
        case PLX_AGG_SUM: return sum_out_dtype(in);
        case PLX_AGG_MEAN: return in == PLX_F32 ? PLX_F32 : PLX_F64;
        case PLX_AGG_VAR: case PLX_AGG_STD:
          PLX_REQUIRE(dtype_is_int(in) || dtype_is_float(in), PLX_ERR_UNSUPPORTED, std::string(x.op == PLX_AGG_STD ? "std" : "var") + " of a " + dtype_name(in) + " expression: numeric operands only");
          return in == PLX_F32 ? PLX_F32 : PLX_F64;
        case PLX_AGG_QUANTILE:
          PLX_REQUIRE(dtype_is_int(in) || dtype_is_float(in), PLX_ERR_UNSUPPORTED, std::string("median / quantile of a ") + dtype_name(in) + " expression: integer and float operands only");
          return in == PLX_F32 ? PLX_F32 : PLX_F64;
        case PLX_AGG_COUNT: case PLX_AGG_LEN: case PLX_AGG_N_UNIQUE: return PLX_U32;
        default: return in;
      }
    }
    case PLX_AE_BINARY: {
      int l = infer_dtype(plan, x.lhs, schema), r = infer_dtype(plan, x.rhs, schema);
      if (is_cmp_op(x.op) || is_logic_op(x.op)) return PLX_BOOL;
      PLX_REQUIRE(l == r, PLX_ERR_INVALID, std::string("binary expression operands have different dtypes (") + dtype_name(l) + ", " + dtype_name(r) + "); the optimizer's type coercion must insert casts");
      if (x.op == PLX_OP_TRUE_DIVIDE && !dtype_is_float(l)) return PLX_F64;
      return l;
    }
    default: fail(PLX_ERR_UNSUPPORTED, "unsupported AExpr kind " + std::to_string(x.kind));
  }
}

std::string output_name(const Plan& plan, int e) {
  const AE& x = plan.ae.at(e);
  switch (x.kind) {
    case PLX_AE_ALIAS: return x.name;
    case PLX_AE_COLUMN: return x.name;
    case PLX_AE_LITERAL: return "literal";
    case PLX_AE_LEN: return "len";
    default: return x.lhs >= 0 ? output_name(plan, x.lhs) : "literal";  // leftmost leaf, like polars
  }
}

// A window (PLX_AE_WINDOW) is a row-level value to everything around it: it does not reduce its node (no aggregate), it reads columns (a column outside an
// aggregate), and the aggregates inside it belong to its own group-by (collect_aggs stops at it).
// A cumulative or ranking node (PLX_AE_CUMULATIVE / PLX_AE_RANK) is row-level in the same way: one value per row, its operand is its own business.
// ... and so is a shift / diff or rolling node (PLX_AE_SHIFT / PLX_AE_ROLLING): a fixed number of neighbouring rows of the same order.
static bool is_neighbour_fn(const AE& x) { return x.kind == PLX_AE_SHIFT || x.kind == PLX_AE_ROLLING; }
static bool is_rowfn(const AE& x) { return x.kind == PLX_AE_CUMULATIVE || x.kind == PLX_AE_RANK || is_neighbour_fn(x); }
static bool contains_agg(const Plan& plan, int e) {
  if (e < 0) return false;
  const AE& x = plan.ae[e];
  if (x.kind == PLX_AE_WINDOW || is_rowfn(x)) return false;
  if (x.kind == PLX_AE_AGG || x.kind == PLX_AE_LEN) return true;
  return contains_agg(plan, x.lhs) || contains_agg(plan, x.rhs) || contains_agg(plan, x.cond);
}
static bool contains_window(const Plan& plan, int e) {
  if (e < 0) return false;
  const AE& x = plan.ae[e];
  return x.kind == PLX_AE_WINDOW || contains_window(plan, x.lhs) || contains_window(plan, x.rhs) || contains_window(plan, x.cond);
}
static bool contains_rowfn(const Plan& plan, int e) {
  if (e < 0) return false;
  const AE& x = plan.ae[e];
  return is_rowfn(x) || contains_rowfn(plan, x.lhs) || contains_rowfn(plan, x.rhs) || contains_rowfn(plan, x.cond);
}
static bool contains_neighbour_fn(const Plan& plan, int e) {
  if (e < 0) return false;
  const AE& x = plan.ae[e];
  return is_neighbour_fn(x) || contains_neighbour_fn(plan, x.lhs) || contains_neighbour_fn(plan, x.rhs) || contains_neighbour_fn(plan, x.cond);
}
// why a fused pipeline leaves an expression list that holds a per-row function to the per-node route
static const char* rowfn_route_note(const Plan& plan, int e) {
  return contains_neighbour_fn(plan, e) ? "shift / diff / rolling expression: per-node route" : "cumulative / ranking expression: per-node route";
}
static bool contains_column_outside_agg(const Plan& plan, int e) {
  if (e < 0) return false;
  const AE& x = plan.ae[e];
  if (x.kind == PLX_AE_WINDOW || is_rowfn(x)) return true;
  if (x.kind == PLX_AE_AGG || x.kind == PLX_AE_LEN) return false;
  if (x.kind == PLX_AE_COLUMN) return true;
  return contains_column_outside_agg(plan, x.lhs) || contains_column_outside_agg(plan, x.rhs) || contains_column_outside_agg(plan, x.cond);
}
static bool contains_column(const Plan& plan, int e) {
  if (e < 0) return false;
  const AE& x = plan.ae[e];
  if (x.kind == PLX_AE_COLUMN) return true;
  return contains_column(plan, x.lhs) || contains_column(plan, x.rhs) || contains_column(plan, x.cond);
}
static void collect_aggs(const Plan& plan, int e, std::vector<int>& out) {
  if (e < 0) return;
  const AE& x = plan.ae[e];
  if (x.kind == PLX_AE_WINDOW || is_rowfn(x)) return;
  if (x.kind == PLX_AE_AGG || x.kind == PLX_AE_LEN) { if (std::find(out.begin(), out.end(), e) == out.end()) out.push_back(e); return; }
  collect_aggs(plan, x.lhs, out);
  collect_aggs(plan, x.rhs, out);
  collect_aggs(plan, x.cond, out);
}

// -------------------------------------------------- materialising evaluator ----
// One kernel per node; every node materialises its column (reference-shaped).
// `overrides` maps expression ids to precomputed columns (aggregation results).
struct Evaluated { ColumnPtr col; bool scalar; };  // scalar: length-1, broadcastable

using ops::scalar_of;

// what the per-node reductions that have a route of their own ran (the radix select of a median): eval() appends, the executor that called it moves the text into
// the plan description
static thread_local std::string t_node_notes;
static void flush_node_notes(Plan& plan) { plan.desc += t_node_notes; t_node_notes.clear(); }

static Evaluated eval(const Plan& plan, int e, const Frame& df, const std::map<int, ColumnPtr>* overrides) {
  check_cancel();
  if (overrides) { auto it = overrides->find(e); if (it != overrides->end()) return {it->second, false}; }
  const AE& x = plan.ae.at(e);
  switch (x.kind) {
    case PLX_AE_COLUMN: {
      int i = df.find(x.name);
      if (i < 0) fail(PLX_ERR_NOT_FOUND, "column not found: " + x.name);
      return {df.cols[i], false};
    }
    case PLX_AE_LITERAL: return {ops::full_column(x.dtype, x.lit, !x.is_null, 1), true};
    case PLX_AE_ALIAS: return eval(plan, x.lhs, df, overrides);
    case PLX_AE_CAST: { Evaluated c = eval(plan, x.lhs, df, overrides); return {ops::cast(c.col, x.dtype), c.scalar}; }
    case PLX_AE_NOT: { Evaluated c = eval(plan, x.lhs, df, overrides); return {ops::bool_not(c.col), c.scalar}; }
    case PLX_AE_IS_NULL: case PLX_AE_IS_NOT_NULL: {
      // the validity bitmap IS the answer: a Boolean column that shares it as its values (no kernel), never null itself
      Evaluated c = eval(plan, x.lhs, df, overrides);
      ColumnPtr b;
      if (c.col->validity && column_null_count(c.col) > 0) {
        b = std::make_shared<Column>();
        b->dtype = PLX_BOOL; b->len = c.col->len; b->values = c.col->validity; b->null_count = 0;
      } else {
        plx_scalar one; one.u = 1;
        b = ops::full_column(PLX_BOOL, one, true, c.col->len);
      }
      return {x.kind == PLX_AE_IS_NULL ? ops::bool_not(b) : b, c.scalar};
    }
    case PLX_AE_FILL_NULL: {
      Evaluated c = eval(plan, x.lhs, df, overrides);
      const AE& l = plan.ae.at(x.rhs);
      PLX_REQUIRE(l.kind == PLX_AE_LITERAL && !l.is_null, PLX_ERR_UNSUPPORTED, "fill_null with a non-literal value");
      PLX_REQUIRE(l.dtype == c.col->dtype, PLX_ERR_INVALID, std::string("fill_null literal dtype ") + dtype_name(l.dtype) + " differs from the column's " + dtype_name(c.col->dtype));
      return {ops::fill_null(c.col, l.lit), c.scalar};
    }
    case PLX_AE_BITMAP_LOOKUP: {
      Evaluated c = eval(plan, x.lhs, df, overrides);
      return {ops::bitmap_lookup(c.col, x.lut), c.scalar};
    }
    case PLX_AE_TEMPORAL: {
      Evaluated c = eval(plan, x.lhs, df, overrides);
      return {ops::temporal_part(c.col, x.op, (int)x.lit.u), c.scalar};
    }
    case PLX_AE_TERNARY: {
      // a length-1 operand broadcasts inside the kernel (select_kernel's scalar forms); all three scalar: a scalar
      Evaluated p = eval(plan, x.cond, df, overrides), a = eval(plan, x.lhs, df, overrides), b = eval(plan, x.rhs, df, overrides);
      PLX_REQUIRE(p.col->dtype == PLX_BOOL, PLX_ERR_INVALID, "when/then/otherwise: the predicate must be Boolean");
      PLX_REQUIRE(a.col->dtype == b.col->dtype, PLX_ERR_INVALID, std::string("when/then/otherwise branches have different dtypes (") + dtype_name(a.col->dtype) + ", " + dtype_name(b.col->dtype) + ")");
      return {ops::if_then_else(p.col, a.col, b.col), p.scalar && a.scalar && b.scalar};
    }
    case PLX_AE_LEN: { ops::ScalarValue s; s.dtype = PLX_U32; s.valid = true; s.v.u = (uint32_t)df.height; return {ops::scalar_column(s), true}; }
    // a window's column is finished before the node's expressions are evaluated (run_windows) and found in `overrides` above; one that is not there stands where no
    // executor collects windows
    case PLX_AE_WINDOW: fail(PLX_ERR_UNSUPPORTED, "window expression (.over): only the expressions of select / with_columns and the predicate of filter take one");
    // ... and so is a cumulative or ranking node's
    case PLX_AE_CUMULATIVE: case PLX_AE_RANK:
      fail(PLX_ERR_UNSUPPORTED, std::string(x.kind == PLX_AE_RANK ? "rank" : cumulative::op_name(x.op)) + ": a cumulative / ranking expression stands in the expressions of select / with_columns and the predicate of filter only");
    case PLX_AE_SHIFT: case PLX_AE_ROLLING:
      fail(PLX_ERR_UNSUPPORTED, std::string(x.kind == PLX_AE_SHIFT ? (x.op == 1 ? "diff" : "shift") : rolling::op_name(x.op)) + ": a shift / diff / rolling expression stands in the expressions of select / with_columns and the predicate of filter only");
    case PLX_AE_AGG: {
      Evaluated c = eval(plan, x.lhs, df, overrides);
      if (x.op == PLX_AGG_VAR || x.op == PLX_AGG_STD) return {ops::scalar_column(ops::reduce_var(c.col, (int)x.lit.u, x.op == PLX_AGG_STD)), true};
      if (x.op == PLX_AGG_QUANTILE) {
        std::string d;
        const ops::ScalarValue v = ops::reduce_quantile(c.col, x.lit.f64, x.dtype, &d);
        t_node_notes += d + "; ";
        return {ops::scalar_column(v), true};
      }
      if (x.op == PLX_AGG_N_UNIQUE) {
        std::string d;
        const ops::ScalarValue v = ops::reduce_n_unique(c.col, &d);
        t_node_notes += d + "; ";
        return {ops::scalar_column(v), true};
      }
      return {ops::scalar_column(ops::reduce(x.op, c.col)), true};
    }
    case PLX_AE_BINARY: {
      Evaluated l = eval(plan, x.lhs, df, overrides), r = eval(plan, x.rhs, df, overrides);
      const bool both_scalar = l.scalar && r.scalar;
      if (is_logic_op(x.op)) {
        ColumnPtr a = l.col, b = r.col;
        if (l.scalar && !r.scalar) { bool v; plx_scalar s = scalar_of(a, &v); a = ops::full_column(PLX_BOOL, s, v, b->len); }
        if (r.scalar && !l.scalar) { bool v; plx_scalar s = scalar_of(b, &v); b = ops::full_column(PLX_BOOL, s, v, a->len); }
        return {ops::bool_binop(x.op - PLX_OP_AND, a, b), both_scalar};
      }
      if (is_cmp_op(x.op)) {
        const int op = x.op - PLX_OP_EQ;
        if (r.scalar && !l.scalar) { bool v; plx_scalar s = scalar_of(r.col, &v); PLX_REQUIRE(l.col->dtype == r.col->dtype, PLX_ERR_INVALID, "cmp: dtype mismatch"); return {ops::cmp_scalar(op, l.col, s, !v), false}; }
        if (l.scalar && !r.scalar) {
          // lit OP col == col OP' lit with the operator mirrored
          static const int mirror[6] = {PLX_EQ, PLX_NE, PLX_GT, PLX_GE, PLX_LT, PLX_LE};
          bool v; plx_scalar s = scalar_of(l.col, &v); PLX_REQUIRE(l.col->dtype == r.col->dtype, PLX_ERR_INVALID, "cmp: dtype mismatch");
          return {ops::cmp_scalar(mirror[op], r.col, s, !v), false};
        }
        return {ops::cmp(op, l.col, r.col), both_scalar};
      }
      PLX_REQUIRE(is_arith_op(x.op), PLX_ERR_UNSUPPORTED, "unsupported operator");
      const int op = x.op - PLX_OP_PLUS;
      if (r.scalar && !l.scalar) {
        bool v; plx_scalar s = scalar_of(r.col, &v);
        PLX_REQUIRE(l.col->dtype == r.col->dtype, PLX_ERR_INVALID, "arith: dtype mismatch");
        if (!v) return {ops::full_column(op == PLX_TRUE_DIV && !dtype_is_float(l.col->dtype) ? PLX_F64 : l.col->dtype, plx_scalar{0}, false, l.col->len), false};
        return {ops::arith_scalar(op, l.col, s, false), false};
      }
      if (l.scalar && !r.scalar) {
        bool v; plx_scalar s = scalar_of(l.col, &v);
        PLX_REQUIRE(l.col->dtype == r.col->dtype, PLX_ERR_INVALID, "arith: dtype mismatch");
        if (!v) return {ops::full_column(op == PLX_TRUE_DIV && !dtype_is_float(r.col->dtype) ? PLX_F64 : r.col->dtype, plx_scalar{0}, false, r.col->len), false};
        return {ops::arith_scalar(op, r.col, s, true), false};
      }
      return {ops::arith(op, l.col, r.col), both_scalar};
    }
    default: fail(PLX_ERR_UNSUPPORTED, "unsupported AExpr kind");
  }
}

static ColumnPtr broadcast(const Evaluated& ev, int64_t height) {
  if (!ev.scalar || ev.col->len == height) return ev.col;
  bool v; plx_scalar s = scalar_of(ev.col, &v);
  return ops::full_column(ev.col->dtype, s, v, height);
}

// ----------------------------------------------------- fused program compiler ----
struct DNode {
  uint8_t code = OP_NOP, c = 0;
  int a = -1, b = -1;
  int p = -1;       // third source node (OP_SELECT: the predicate; its slot becomes Op::c)
  uint64_t imm = 0;
  int col = -1;     // frame column index for OP_LOAD
  char ty = 'i';    // 'i' signed, 'u' unsigned 64, 'f' f64, 'b' bool
  bool nullable = false;
  int uses = 0, slot = -1;
  bool emitted = false;
};

class Compiler {
 public:
  Compiler(const Plan& p, const Frame& f) : plan(p), df(&f), n_rows(f.height) {}
  const Plan& plan;
  const Frame* df;               // name resolution / dtype inference scope (may be switched to a view of the same rows)
  int64_t n_rows;
  std::vector<ColumnPtr> cols;   // distinct input columns referenced so far
  std::vector<DNode> nodes;
  std::map<std::string, int> memo;
  std::vector<std::pair<uint8_t, int>> aggs;  // (kind, src node or -1)
  int pred = -1, key = -1;
  std::vector<int> wide_keys;  // raw key nodes of a wide (multi-word) group key

  int add(DNode n) {
    std::ostringstream k;
    k << (int)n.code << ':' << n.a << ':' << n.b << ':' << n.p << ':' << (int)n.c << ':' << n.imm << ':' << n.col << ':' << n.ty;
    auto it = memo.find(k.str());
    if (it != memo.end()) return it->second;
    nodes.push_back(n);
    memo[k.str()] = (int)nodes.size() - 1;
    return (int)nodes.size() - 1;
  }
  int mk(uint8_t code, int a, int b, char ty, uint8_t c = 0) {
    DNode n; n.code = code; n.a = a; n.b = b; n.ty = ty; n.c = c;
    n.nullable = (a >= 0 && nodes[a].nullable) || (b >= 0 && nodes[b].nullable);
    return add(n);
  }
  int konst(uint64_t bits, char ty) { DNode n; n.code = OP_CONST; n.imm = bits; n.ty = ty; return add(n); }
  int konst_f(double d) { uint64_t b; memcpy(&b, &d, 8); return konst(b, 'f'); }
  int ifnull(int a, uint64_t code) { DNode n; n.code = OP_IFNULL; n.a = a; n.b = a; n.imm = code; n.ty = nodes[a].ty; n.nullable = false; return add(n); }
  // membership of integer node `a` in lookup bitmap `lut` (args.lut[lut] is filled in by the caller before the launch)
  // node `a` with its validity cut down to the rows where boolean node `m` is valid and true (OP_MASKV)
  int mask_valid(int a, int m) { DNode n; n.code = OP_MASKV; n.a = a; n.b = m; n.ty = nodes[a].ty; n.nullable = true; return add(n); }
  // when(p).then(a).otherwise(b) (OP_SELECT): the chosen side's value and validity
  int select(int p, int a, int b, char ty) { DNode n; n.code = OP_SELECT; n.a = a; n.b = b; n.p = p; n.ty = ty; n.nullable = nodes[a].nullable || nodes[b].nullable; return add(n); }
  // Lookup bitmaps of one program (args.lut, kMaxLuts of them), one numbering: indices below lut_base belong to the pipeline that owns this compiler (the membership
  // bitmaps of its semi joins: it fills them in before its launches and says how many it needs BEFORE anything is lowered); the bitmaps of PLX_AE_BITMAP_LOOKUP nodes
  // follow from lut_base up, handed out and filled in here -- args travels with the compiler to every launch of its program.
  int lut_base = 0;
  std::vector<ColumnPtr> static_luts;
  int static_lut(const ColumnPtr& col) {
    for (size_t i = 0; i < static_luts.size(); i++) if (static_luts[i].get() == col.get()) return lut_base + (int)i;
    const int idx = lut_base + (int)static_luts.size();
    if (idx >= kMaxLuts) throw Unsupported("the program needs more than " + std::to_string(kMaxLuts) + " lookup bitmaps (kMaxLuts: bitmap lookups and the membership bitmaps of semi joins share them)");
    static_luts.push_back(col);
    args.lut[idx] = Lut{col->values ? col->values->as<unsigned long long>() : nullptr, (uint64_t)col->len};
    return idx;
  }
  int bit_lookup(int a, int lut, int64_t kmin) { DNode n; n.code = OP_BITLOOKUP; n.a = a; n.b = a; n.c = (uint8_t)lut; n.imm = (uint64_t)kmin; n.ty = 'b'; n.nullable = nodes[a].nullable; return add(n); }
  int col_id(const ColumnPtr& c) {
    for (size_t i = 0; i < cols.size(); i++) if (cols[i].get() == c.get()) return (int)i;
    cols.push_back(c);
    return (int)cols.size() - 1;
  }
  int load(int frame_col) {
    const ColumnPtr& c = df->cols[frame_col];
    const int col = col_id(c);
    DNode n; n.code = OP_LOAD; n.col = col; n.nullable = (bool)c->validity || c->null_count > 0;
    switch (c->dtype) {
      case PLX_F64: n.ty = 'f'; break;
      case PLX_U64: n.ty = 'u'; break;
      case PLX_BOOL: n.ty = 'b'; break;
      case PLX_F32: throw Unsupported("f32 columns are evaluated in f32 by the per-node kernels, not in the f64 fused program");
      default: n.ty = 'i'; break;
    }
    return add(n);
  }
  static uint64_t widen_literal(int dt, plx_scalar s) {
    switch (dt) {
      case PLX_I8: return (uint64_t)(int64_t)(int8_t)s.u;
      case PLX_I16: return (uint64_t)(int64_t)(int16_t)s.u;
      case PLX_I32: return (uint64_t)(int64_t)(int32_t)s.u;
      case PLX_U8: return s.u & 0xff;
      case PLX_U16: return s.u & 0xffff;
      case PLX_U32: return s.u & 0xffffffffull;
      case PLX_BOOL: return s.u & 1;
      default: return s.u;
    }
  }
  bool is_literal(int e, double* as_f64, int dt_hint) const {
    const AE* x = &plan.ae[e];
    while (x->kind == PLX_AE_ALIAS) x = &plan.ae[x->lhs];
    if (x->kind != PLX_AE_LITERAL || x->is_null) return false;
    switch (x->dtype) {
      case PLX_F64: *as_f64 = x->lit.f64; return true;
      case PLX_F32: *as_f64 = x->lit.f32; return true;
      case PLX_U64: *as_f64 = (double)x->lit.u; return true;
      case PLX_BOOL: return false;
      default: *as_f64 = (double)(int64_t)widen_literal(x->dtype, x->lit); return true;
    }
    (void)dt_hint;
  }

  int lower(int e) {
    const AE& x = plan.ae.at(e);
    switch (x.kind) {
      case PLX_AE_COLUMN: {
        int i = df->find(x.name);
        if (i < 0) fail(PLX_ERR_NOT_FOUND, "column not found: " + x.name);
        return load(i);
      }
      case PLX_AE_LITERAL: {
        if (x.is_null) throw Unsupported("null literal");
        if (x.dtype == PLX_F32) throw Unsupported("f32 literal");
        char ty = x.dtype == PLX_F64 ? 'f' : x.dtype == PLX_U64 ? 'u' : x.dtype == PLX_BOOL ? 'b' : 'i';
        return konst(widen_literal(x.dtype, x.lit), ty);
      }
      case PLX_AE_ALIAS: return lower(x.lhs);
      case PLX_AE_NOT: { int a = lower(x.lhs); if (nodes[a].ty != 'b') throw Unsupported("not on non-boolean"); return mk(OP_NOT, a, a, 'b'); }
      case PLX_AE_IS_NULL: case PLX_AE_IS_NOT_NULL: {
        // valid(a) as a value, with the opcodes the kernels already have: (a ==bits a) is 1 with a's validity; IFNULL(.., 0) turns
        // the null into 0.  A source that cannot be null folds to a constant.
        int a = lower(x.lhs);
        int nn = nodes[a].nullable ? ifnull(mk(OP_CMP_U, a, a, 'b', (uint8_t)PLX_EQ), 0) : konst(1, 'b');
        return x.kind == PLX_AE_IS_NOT_NULL ? nn : mk(OP_NOT, nn, nn, 'b');
      }
      case PLX_AE_FILL_NULL: {
        const int dt = infer_dtype(plan, x.lhs, *df);
        const AE& l = plan.ae.at(x.rhs);
        if (l.kind != PLX_AE_LITERAL || l.is_null) throw Unsupported("fill_null with a non-literal value");
        if (l.dtype != dt) fail(PLX_ERR_INVALID, std::string("fill_null literal dtype ") + dtype_name(l.dtype) + " differs from the column's " + dtype_name(dt));
        if (dt == PLX_F32) throw Unsupported("f32 fill_null");
        int a = lower(x.lhs);
        return nodes[a].nullable ? ifnull(a, widen_literal(l.dtype, l.lit)) : a;
      }
      case PLX_AE_BITMAP_LOOKUP: {
        const int in = infer_dtype(plan, x.lhs, *df);
        if (!dtype_is_int(in)) fail(PLX_ERR_INVALID, std::string("bitmap lookup: the input must be an integer expression, not ") + dtype_name(in));
        const int a = lower(x.lhs);
        return bit_lookup(a, static_lut(x.lut), 0);
      }
      case PLX_AE_TEMPORAL: {
        infer_dtype(plan, e, *df);      // (fails when the operand is not I32 with unit Date / I64 with a Datetime unit)
        const int a = lower(x.lhs);
        // one source, no immediate; part and unit ride in Op::c, i.e. in the Shape: the compiled kernels fold the switch.  The result is the 64-bit widening of the
        // part's dtype, nullable exactly when the operand is
        return mk(OP_DATEPART, a, a, 'i', temporal::pack(x.op, (int)x.lit.u));
      }
      case PLX_AE_TERNARY: {
        const int dt = infer_dtype(plan, e, *df);      // (fails when the branches differ in dtype or the predicate is not Boolean)
        if (dt == PLX_F32) throw Unsupported("f32 when/then/otherwise");
        const int p = lower(x.cond);
        if (nodes[p].ty != 'b') throw Unsupported("when/then/otherwise predicate is not boolean");
        if (nodes[p].code == OP_CONST) return lower((nodes[p].imm & 1) ? x.lhs : x.rhs);      // a constant predicate: the chosen branch
        auto null_literal = [&](int b) { const AE* y = &plan.ae.at(b); while (y->kind == PLX_AE_ALIAS) y = &plan.ae.at(y->lhs); return y->kind == PLX_AE_LITERAL && y->is_null; };
        const bool a_null = null_literal(x.lhs), b_null = null_literal(x.rhs);
        if (a_null && b_null) throw Unsupported("when/then/otherwise of two null literals");
        // a null-literal branch needs no constant: the other branch with its validity cut down to the rows that choose it (OP_MASKV)
        if (b_null) return mask_valid(lower(x.lhs), p);
        if (a_null) { const int t = nodes[p].nullable ? ifnull(p, 0) : p; return mask_valid(lower(x.rhs), mk(OP_NOT, t, t, 'b')); }
        const int a = lower(x.lhs), b = lower(x.rhs);
        if (a == b) return a;
        // both branches hold the dtype's 64-bit widening already (a cast that only widens leaves its operand's tag on the node: the tag follows the dtype here)
        return select(p, a, b, dt == PLX_F64 ? 'f' : dt == PLX_U64 ? 'u' : dt == PLX_BOOL ? 'b' : 'i');
      }
      case PLX_AE_CAST: {
        int from = infer_dtype(plan, x.lhs, *df), to = x.dtype;
        int a = lower(x.lhs);
        if (from == to) return a;
        if (to == PLX_F64 && dtype_is_int(from)) return mk(nodes[a].ty == 'u' ? OP_U2F : OP_I2F, a, a, 'f');
        if (dtype_is_int(from) && (to == PLX_I64) && from != PLX_U64) return a;  // value-preserving widening
        if (dtype_is_unsigned(from) && to == PLX_U64) return a;
        throw Unsupported(std::string("cast ") + dtype_name(from) + " -> " + dtype_name(to) + " inside a fused program");
      }
      case PLX_AE_BINARY: {
        int ldt = infer_dtype(plan, x.lhs, *df), rdt = infer_dtype(plan, x.rhs, *df);
        if (is_logic_op(x.op)) {
          int a = lower(x.lhs), b = lower(x.rhs);
          if (nodes[a].ty != 'b' || nodes[b].ty != 'b') throw Unsupported("bitwise and/or on integers");
          int n = mk(x.op == PLX_OP_AND ? OP_AND : x.op == PLX_OP_OR ? OP_OR : OP_XOR, a, b, 'b');
          return n;
        }
        if (ldt != rdt) fail(PLX_ERR_INVALID, std::string("binary expression operands have different dtypes (") + dtype_name(ldt) + ", " + dtype_name(rdt) + ")");
        if (is_cmp_op(x.op)) {
          if (ldt == PLX_BOOL) throw Unsupported("comparison of boolean columns");
          int a = lower(x.lhs), b = lower(x.rhs);
          uint8_t code = nodes[a].ty == 'f' ? OP_CMP_F : nodes[a].ty == 'u' ? OP_CMP_U : OP_CMP_I;
          return mk(code, a, b, 'b', (uint8_t)(x.op - PLX_OP_EQ));
        }
        if (!(ldt == PLX_I64 || ldt == PLX_U64 || ldt == PLX_F64)) throw Unsupported(std::string("arithmetic on ") + dtype_name(ldt) + " wraps at the column width; done by the per-node kernels");
        const bool f = ldt == PLX_F64;
        switch (x.op) {
          case PLX_OP_PLUS: { int a = lower(x.lhs), b = lower(x.rhs); return mk(f ? OP_ADD_F : OP_ADD_I, a, b, nodes[a].ty); }
          case PLX_OP_MINUS: { int a = lower(x.lhs), b = lower(x.rhs); return mk(f ? OP_SUB_F : OP_SUB_I, a, b, nodes[a].ty); }
          case PLX_OP_MULTIPLY: { int a = lower(x.lhs), b = lower(x.rhs); return mk(f ? OP_MUL_F : OP_MUL_I, a, b, nodes[a].ty); }
          case PLX_OP_TRUE_DIVIDE: {
            int a = lower(x.lhs);
            if (!f) a = mk(nodes[a].ty == 'u' ? OP_U2F : OP_I2F, a, a, 'f');
            double lit;
            if (is_literal(x.rhs, &lit, rdt)) {
              // col / lit == col * (1 / lit)  (float.rs:113-115, signed.rs:218-221)
              int inv = konst_f(1.0 / lit);
              return mk(OP_MUL_F, a, inv, 'f');
            }
            int b = lower(x.rhs);
            if (!f) b = mk(nodes[b].ty == 'u' ? OP_U2F : OP_I2F, b, b, 'f');
            return mk(OP_DIV_F, a, b, 'f');
          }
          case PLX_OP_FLOOR_DIVIDE: case PLX_OP_MODULUS: {
            if (f) throw Unsupported("float floor-div / mod inside a fused program");
            int a = lower(x.lhs), b = lower(x.rhs);
            const bool u = nodes[a].ty == 'u';
            const uint8_t code = x.op == PLX_OP_FLOOR_DIVIDE ? (u ? OP_FDIV_U : OP_FDIV_I) : (u ? OP_MOD_U : OP_MOD_I);
            int n = mk(code, a, b, nodes[a].ty);
            nodes[n].nullable = true;   // divisor 0 -> null (signed.rs:35-70)
            return n;
          }
          default: throw Unsupported("operator inside a fused program");
        }
      }
      case PLX_AE_WINDOW: case PLX_AE_WINDOW_KEY: throw Unsupported(contains_rowfn(plan, x.lhs) ? rowfn_route_note(plan, x.lhs) : "window expression: per-node route");
      case PLX_AE_CUMULATIVE: case PLX_AE_RANK: throw Unsupported("cumulative / ranking expression: per-node route");
      case PLX_AE_SHIFT: case PLX_AE_ROLLING: throw Unsupported("shift / diff / rolling expression: per-node route");
      default: throw Unsupported("aggregation nested inside a row expression");
    }
  }

  int add_agg(uint8_t kind, int src) {
    for (size_t i = 0; i < aggs.size(); i++) if (aggs[i].first == kind && aggs[i].second == src) return (int)i;
    if ((int)aggs.size() >= kMaxAggs) throw Unsupported("more than " + std::to_string(kMaxAggs) + " distinct aggregates in one pass");
    aggs.push_back({kind, src});
    return (int)aggs.size() - 1;
  }
  int count_agg(int src) { return nodes[src].nullable ? add_agg(AGG_COUNT, src) : add_agg(AGG_LEN, -1); }

  // ---- var / std: sums about a pivot ----
  // The cells of the sinks are commutative atomics: they can hold sum(x - p) and sum((x - p)^2), not a Welford state.  p = the mean of the source expression over the
  // first kVarPivotRows rows of the frame (the query's predicate left out), from a throw-away fused select and one small download; 0 when none of those rows is valid,
  // when that mean is not finite, and when nothing may be launched (compile only).  Any convex combination of source values lies inside [min, max] of the source, which
  // is all the accuracy contract asks of it.  One pivot per (program, source node).
  static constexpr int64_t kVarPivotRows = 4096;
  bool device_pivot = false;                       // set by the drivers that are about to run the program on the device
  std::vector<std::pair<int, double>> var_pivots;  // (f64 source node, p)
  std::vector<std::pair<int, double>> pivot_by_expr;   // (source expression of the plan, p): every var / std node lowered here
  std::vector<std::pair<int, double>> seed_pivots;     // pivots another compiler of the same plan took over the same rows (the left join's second program): no second pre-pass
  std::string var_note;                            // "var pivot x=...; " per source, for the plan description
  double var_pivot(int src_expr, int sf) {
    for (auto& pv : var_pivots) if (pv.first == sf) { pivot_by_expr.push_back({src_expr, pv.second}); return pv.second; }
    double p = 0.0;
    bool seeded = false;
    for (auto& pv : seed_pivots) if (pv.first == src_expr) { p = pv.second; seeded = true; }
    const int64_t rows = std::min<int64_t>(n_rows, kVarPivotRows);
    if (!seeded && device_pivot && rows > 0) {
      Compiler t(plan, *df);
      t.n_rows = rows;
      const int s = t.lower(src_expr);
      const int tf = t.nodes[s].ty == 'f' ? s : t.mk(t.nodes[s].ty == 'u' ? OP_U2F : OP_I2F, s, s, 'f');
      const int sum_idx = t.add_agg(AGG_SUM_F, tf), cnt_idx = t.count_agg(s);
      t.finish();
      uint64_t host[kMaxAggs] = {0};
      k::fused_regagg(t.shape, t.args, find_static_shape(t.shape), host);
      const uint64_t cnt = t.shape.aggs[cnt_idx].kind == AGG_LEN ? (uint64_t)rows : host[cnt_idx];
      double sum; memcpy(&sum, &host[sum_idx], 8);
      if (cnt) p = sum / (double)cnt;
      if (!std::isfinite(p)) p = 0.0;
    }
    var_pivots.push_back({sf, p});
    pivot_by_expr.push_back({src_expr, p});
    std::ostringstream o; o.precision(17);
    o << "var pivot " << output_name(plan, src_expr) << "=" << p << "; ";
    var_note += o.str();
    return p;
  }

  // an order statistic is no sum of cells: a list that holds one is declined as a whole, before a var / std beside it spends its pivot pre-pass
  static constexpr const char* kOrderStatistic = "median / quantile: an order statistic (sorted-segment route)";
  // ... and so is a distinct count; a list that holds both keeps the quantile's reason
  static constexpr const char* kDistinctCount = "n_unique: a distinct count (sorted-segment route)";
  void decline_order_statistics(const std::vector<int>& agg_nodes) const {
    for (int a : agg_nodes) if (plan.ae.at(a).kind == PLX_AE_AGG && plan.ae[a].op == PLX_AGG_QUANTILE) throw Unsupported(kOrderStatistic);
    for (int a : agg_nodes) if (plan.ae.at(a).kind == PLX_AE_AGG && plan.ae[a].op == PLX_AGG_N_UNIQUE) throw Unsupported(kDistinctCount);
  }

  // lowers one AGG / LEN node; returns how to finalise it
  FinalSpec lower_agg(int e) {
    const AE& x = plan.ae.at(e);
    FinalSpec fs{}; fs.a = fs.b = fs.c = kNone;
    if (x.kind == PLX_AE_LEN) { fs.kind = FIN_TRUNC32; fs.a = (uint8_t)add_agg(AGG_LEN, -1); fs.out_dtype = PLX_U32; return fs; }
    const int in_dt = infer_dtype(plan, x.lhs, *df);
    if (x.op == PLX_AGG_LEN) { fs.kind = FIN_TRUNC32; fs.a = (uint8_t)add_agg(AGG_LEN, -1); fs.out_dtype = PLX_U32; return fs; }
    if (x.op == PLX_AGG_QUANTILE) throw Unsupported(kOrderStatistic);
    if (x.op == PLX_AGG_N_UNIQUE) throw Unsupported(kDistinctCount);
    // Boolean inputs: sum = number of true values (UInt32, sum_output_dtype) and mean = their fraction; a boolean slot holds 0 / 1,
    // so both reuse the integer cells.  min / max of booleans would need a bit-packed finalisation: per-node path.
    if (x.op == PLX_AGG_VAR || x.op == PLX_AGG_STD) infer_dtype(plan, e, *df);      // (fails, naming the dtype, when the operand is not numeric)
    if (in_dt == PLX_BOOL && x.op != PLX_AGG_COUNT && x.op != PLX_AGG_SUM && x.op != PLX_AGG_MEAN) throw Unsupported("min / max of a boolean expression");
    int src = lower(x.lhs);
    switch (x.op) {
      case PLX_AGG_SUM:
        fs.out_dtype = (uint8_t)sum_out_dtype(in_dt);
        if (in_dt == PLX_F64) { fs.kind = FIN_COPY64; fs.a = (uint8_t)add_agg(AGG_SUM_F, src); }
        else { fs.kind = dtype_width(fs.out_dtype) == 4 ? FIN_TRUNC32 : FIN_COPY64; fs.a = (uint8_t)add_agg(AGG_SUM_I, src); }
        return fs;
      case PLX_AGG_MEAN: {
        int sf = src;
        if (in_dt != PLX_F64) sf = mk(nodes[src].ty == 'u' ? OP_U2F : OP_I2F, src, src, 'f');
        fs.kind = FIN_MEAN; fs.a = (uint8_t)add_agg(AGG_SUM_F, sf); fs.b = (uint8_t)count_agg(src); fs.out_dtype = PLX_F64;
        return fs;
      }
      case PLX_AGG_MIN: case PLX_AGG_MAX: {
        const bool mn = x.op == PLX_AGG_MIN;
        fs.out_dtype = (uint8_t)in_dt;
        if (in_dt == PLX_F64) { fs.kind = FIN_MINMAX_F; fs.a = (uint8_t)add_agg(mn ? AGG_MIN_F : AGG_MAX_F, src); fs.b = (uint8_t)count_agg(src); fs.c = (uint8_t)add_agg(AGG_COUNT_ORD, src); }
        else { fs.kind = FIN_MINMAX_I; fs.a = (uint8_t)add_agg(nodes[src].ty == 'u' ? (mn ? AGG_MIN_U : AGG_MAX_U) : (mn ? AGG_MIN_I : AGG_MAX_I), src); fs.b = (uint8_t)count_agg(src); }
        return fs;
      }
      case PLX_AGG_COUNT: fs.kind = FIN_TRUNC32; fs.a = (uint8_t)count_agg(src); fs.out_dtype = PLX_U32; return fs;
      case PLX_AGG_VAR: case PLX_AGG_STD: {
        // d = s - p, q = d * d; cells sum(d), sum(q), count(src): std / var / any ddof over one source share all three (add_agg dedups).  p is an immediate of
        // OP_CONST, so the Shape does not depend on it
        // (the source is an integer or an f64 node here: load() refuses Float32 columns, so fs.out_dtype is always f64 from this compiler -- Float32 results come from
        //  groupby_columns' f64 view and from the per-node kernel)
        int sf = src;
        if (nodes[src].ty != 'f') sf = mk(nodes[src].ty == 'u' ? OP_U2F : OP_I2F, src, src, 'f');
        const int d = mk(OP_SUB_F, sf, konst_f(var_pivot(x.lhs, sf)), 'f');
        const int q = mk(OP_MUL_F, d, d, 'f');
        fs.kind = x.op == PLX_AGG_STD ? FIN_STD : FIN_VAR;
        fs.a = (uint8_t)add_agg(AGG_SUM_F, d); fs.c = (uint8_t)add_agg(AGG_SUM_F, q); fs.b = (uint8_t)count_agg(src);
        fs.ddof = (uint8_t)x.lit.u; fs.out_dtype = PLX_F64;
        return fs;
      }
      default: throw Unsupported("aggregation kind");
    }
  }

  // ---- scheduling: DFS post-order, lowest-free-slot allocation, slots freed at last use
  Shape shape{};
  Args args{};
  std::vector<int> input_cols;
  std::vector<bool> slot_busy = std::vector<bool>(kSlots, false);

  void count_uses(int n, std::vector<bool>& seen) {
    if (n < 0) return;
    nodes[n].uses++;
    if (seen[n]) return;
    seen[n] = true;
    if (nodes[n].code != OP_LOAD && nodes[n].code != OP_CONST) {
      count_uses(nodes[n].a, seen);
      if (nodes[n].b != nodes[n].a) count_uses(nodes[n].b, seen);
      if (third_source(nodes[n])) count_uses(nodes[n].p, seen);
    }
  }
  // the predicate of an OP_SELECT, when it is a node of its own (one use per DISTINCT source, as for a == b)
  static bool third_source(const DNode& d) { return d.p >= 0 && d.p != d.a && d.p != d.b; }
  void release(int n) {
    if (n < 0) return;
    if (--nodes[n].uses == 0) slot_busy[nodes[n].slot] = false;
  }
  int emit(int n) {
    DNode& d = nodes[n];
    if (d.emitted) return d.slot;
    const bool leaf = d.code == OP_LOAD || d.code == OP_CONST;
    int sa = -1, sb = -1, sp = -1;
    if (!leaf) {
      sa = emit(d.a);
      sb = (d.b == d.a) ? sa : emit(d.b);
      if (d.p >= 0) sp = emit(d.p);      // (an emitted node returns its slot)
      release(d.a);
      if (d.b != d.a) release(d.b);
      if (third_source(d)) release(d.p);
    }
    int slot = -1;
    for (int s = 0; s < kSlots; s++) if (!slot_busy[s]) { slot = s; break; }
    if (slot < 0) throw Unsupported("expression needs more than 16 live values");
    slot_busy[slot] = true;
    if (shape.n_ops >= kMaxOps) throw Unsupported("expression program longer than 32 ops");
    const int pc = shape.n_ops++;
    Op op{}; op.code = d.code; op.dst = (uint8_t)slot; op.c = d.c;
    if (d.code == OP_LOAD) {
      int idx = -1;
      for (size_t i = 0; i < input_cols.size(); i++) if (input_cols[i] == d.col) idx = (int)i;
      if (idx < 0) {
        if ((int)input_cols.size() >= kMaxInputs) throw Unsupported("more than 10 input columns");
        input_cols.push_back(d.col); idx = (int)input_cols.size() - 1;
        const ColumnPtr& c = cols[d.col];
        shape.in_dtype[idx] = (uint8_t)c->dtype; shape.in_nullable[idx] = d.nullable ? 1 : 0;
        args.in[idx].values = c->data(); args.in[idx].validity = d.nullable ? c->valid_words() : nullptr;      // (the same pointer either way: nullable <=> the column has a bitmap; fused_sinks.hpp trust_nullable relies on it)
      }
      op.a = (uint8_t)idx;
    } else if (d.code == OP_CONST) {
      args.imm[pc] = d.imm;
    } else {
      op.a = (uint8_t)sa; op.b = (uint8_t)sb;
      if (d.p >= 0) op.c = (uint8_t)sp;
      if (d.code == OP_IFNULL || d.code == OP_BITLOOKUP) args.imm[pc] = d.imm;
    }
    shape.ops[pc] = op;
    d.slot = slot; d.emitted = true;
    return slot;
  }
  void finish() {
    std::vector<bool> seen(nodes.size(), false);
    std::vector<int> roots;
    if (pred >= 0) roots.push_back(pred);
    if (key >= 0) roots.push_back(key);
    for (int kn : wide_keys) roots.push_back(kn);
    for (auto& a : aggs) if (a.second >= 0) roots.push_back(a.second);
    for (int r : roots) count_uses(r, seen);   // each root reference holds its slot to the end
    shape.pred = kNone; shape.key = kNone;
    // Loads first: every column load of a row tile is issued before the first dependent op, so a lane has all
    // its input columns in flight at once (memory-level parallelism) instead of load -> wait -> use per column.
    {
      std::vector<int> order;
      std::vector<bool> vis(nodes.size(), false);
      std::function<void(int)> dfs = [&](int n) {
        if (n < 0 || vis[n]) return;
        vis[n] = true;
        if (nodes[n].code == OP_LOAD) { order.push_back(n); return; }
        if (nodes[n].code == OP_CONST) return;
        dfs(nodes[n].a);
        if (nodes[n].b != nodes[n].a) dfs(nodes[n].b);
        dfs(nodes[n].p);
      };
      for (int r : roots) dfs(r);
      for (int n : order) emit(n);
    }
    if (pred >= 0) shape.pred = (uint8_t)emit(pred);
    if (key >= 0) shape.key = (uint8_t)emit(key);
    shape.n_keys = (uint8_t)wide_keys.size();
    for (size_t i = 0; i < wide_keys.size(); i++) shape.keys[i] = (uint8_t)emit(wide_keys[i]);
    shape.n_aggs = (uint8_t)aggs.size();
    for (size_t i = 0; i < aggs.size(); i++) {
      shape.aggs[i].kind = aggs[i].first;
      shape.aggs[i].src = aggs[i].second >= 0 ? (uint8_t)emit(aggs[i].second) : 0;
    }
    shape.n_inputs = (uint8_t)input_cols.size();
    args.n_rows = n_rows;
  }
};

// ----------------------------------------------------------- group keys -----------
struct KeyPart {
  int expr = -1;
  int dtype = 0;
  bool nullable = false;   // the key expression can be null (=> the output key column carries a validity bitmap)
  KeyDecode dec{};
};
struct KeyPlan {
  std::vector<KeyPart> parts;
  bool packed = false;   // keys bit-packed into a dense id (always valid)
  bool wide = false;     // 2..4 raw key columns compared word by word (WideAggSink)
  bool wide_nullable = false;
  std::vector<int> wide_nodes;
  int total_bits = 64;
  std::string note;      // what the planner did to get the key's range, for the plan description
};

static int ceil_log2_u64(uint64_t x) { int b = 0; while (b < 64 && (1ull << b) < x) b++; return b; }

// Lowers the group keys into one 64-bit key node. Narrow / multi-column keys are packed
// using column min/max statistics; a single wide key is used raw.
// Bounds of an integer column nobody has statistics for, GUESSED from a strided sample of 2^20 rows (1024 runs of 1024 rows: ~20 us) and widened by 1/1024 of the sampled
// span on either side (for uniformly spread values the expected gap between the sample's extremes and the column's is a millionth of the span).  They are installed as
// UNTRUSTED bounds (like plx_column_set_bounds): every kernel that addresses a table or narrows a value with them checks each row, so a wrong guess costs a second run of
// the query from an exact range pass (fused_groupby), never a wrong answer.  What this buys: one collect() over a column seen for the first time plans like every later
// one -- direct-address tables, narrowed values -- without the exact min / max passes over key and value columns (8 B / row each: 3 ms of a 9 ms first run at 1e9 rows).
static bool assume_ranges() { static const bool v = [] { const char* e = getenv("PLX_ASSUME_RANGES"); return !(e && e[0] == '0'); }(); return v; }
static bool assume_range(const ColumnPtr& col) {
  if (!assume_ranges() || !col || col->range_state != 0 || col->no_assume || !col->values || col->len < ((int64_t)1 << 24) || !dtype_is_int(col->dtype) || col->dtype == PLX_U64) return false;
  int64_t smn = 0, smx = 0;
  if (!k::sample_minmax(col, &smn, &smx, 1024)) return false;
  const unsigned __int128 span = (unsigned __int128)((__int128)smx - (__int128)smn);
  if (span >= ((unsigned __int128)1 << 62)) return false;
  const int64_t slack = (int64_t)(span >> 10) + 64;
  int64_t lo_lim = INT64_MIN, hi_lim = INT64_MAX;
  switch (col->dtype) {
    case PLX_I8: lo_lim = -128; hi_lim = 127; break; case PLX_U8: lo_lim = 0; hi_lim = 255; break;
    case PLX_I16: lo_lim = -32768; hi_lim = 32767; break; case PLX_U16: lo_lim = 0; hi_lim = 65535; break;
    case PLX_I32: lo_lim = INT32_MIN; hi_lim = INT32_MAX; break; case PLX_U32: lo_lim = 0; hi_lim = 0xffffffffll; break;
    default: break;
  }
  __int128 lo = std::max<__int128>((__int128)smn - slack, lo_lim);
  __int128 hi = std::min<__int128>((__int128)smx + slack, hi_lim);
  // non-negative values whose span costs the same number of bits from 0 as from their minimum: from 0 (ids and counts usually start there, and a key program without
  // the subtraction is the shape the ahead-of-time kernels were built for)
  if (smn >= 0) {
    auto bits_of = [](__int128 span) { int b = 1; while (b < 62 && ((__int128)1 << b) < span + 2) b++; return b; };
    if (bits_of(hi) == bits_of(hi - lo)) lo = 0;
  }
  // everything up to the next power of two above the span costs the same number of key bits (and value bits): take it -- a heavy-tailed id column (ids handed out by
  // popularity) shows its largest ids to no sample
  { int b = 1; while (b < 62 && ((__int128)1 << b) < hi - lo + 2) b++; hi = std::min<__int128>(lo + ((__int128)1 << b) - 2, hi_lim); }
  col->range_state = 1; col->range_min = (int64_t)lo; col->range_max = (int64_t)hi; col->range_trusted = false; col->range_assumed = true;
  return true;
}
static bool learn_dense_ranges() { const char* e = getenv("PLX_LEARN_DENSE_RANGE"); return !(e && e[0] == '0'); }   // (measurement / tests: 0 = the first run plans without a range pass)
// the plain column behind any aliases of expression `e`, or null when `e` is anything else
static const AE* plain_column(const Plan& plan, int e) {
  const AE* x = &plan.ae[e];
  while (x->kind == PLX_AE_ALIAS) x = &plan.ae[x->lhs];
  return x->kind == PLX_AE_COLUMN ? x : nullptr;
}
// the date-part node behind any aliases of expression `e`, or null
static const AE* temporal_node(const Plan& plan, int e) {
  const AE* x = &plan.ae[e];
  while (x->kind == PLX_AE_ALIAS) x = &plan.ae[x->lhs];
  return x->kind == PLX_AE_TEMPORAL ? x : nullptr;
}
static bool temporal_key_ranges() { const char* e = getenv("PLX_TEMPORAL_KEY_RANGES"); return !(e && e[0] == '0'); }   // (measurement: 0 = a date part is a raw 64-bit key, as any expression)
static KeyPlan lower_keys(Compiler& c, const std::vector<int>& key_exprs) {
  KeyPlan kp;
  const Plan& plan = c.plan;
  const int nk = (int)key_exprs.size();
  std::vector<int> knodes(nk);
  struct Info { bool have_range = false; int64_t mn = 0, mx = 0; bool nullable = false; ColumnPtr col; };
  std::vector<Info> info(nk);
  bool all_packable = true;
  for (int i = 0; i < nk; i++) {
    const int e = key_exprs[i];
    KeyPart part; part.expr = e; part.dtype = infer_dtype(plan, e, *c.df);
    knodes[i] = c.lower(e);
    info[i].nullable = c.nodes[knodes[i]].nullable;
    part.nullable = info[i].nullable;
    const AE* x = plain_column(plan, e);
    const AE* tp = temporal_key_ranges() ? temporal_node(plan, e) : nullptr;
    if (part.dtype == PLX_BOOL) { info[i].have_range = true; info[i].mn = 0; info[i].mx = 1; }
    else if (tp) {
      // A date part's range is known without looking at the data: month 1..12, weekday 1..7, ... -- exact by construction, so nothing here is a guess and nothing
      // needs the per-row check.  year and date are monotone in the value: year(min) .. year(max) of a plain column's own range, taken under the rules a column key's
      // range is (exact statistics, one pass cached on the immutable column; bounds the planner only guessed count when every row has been checked against them since;
      // bounds the caller declared make the table sinks check every row, as they do for the column itself: untrusted_key_bounds looks at the program's inputs).
      // Anything else under the part (an expression, a ms Datetime whose days leave i32) stays a raw 64-bit key.
      const int tpart = tp->op, tunit = (int)tp->lit.u;
      if (tpart != temporal::kYear && tpart != temporal::kDatePart) { info[i].have_range = true; info[i].mn = temporal::part_min(tpart); info[i].mx = temporal::part_max(tpart); }
      else if (const AE* cx = plain_column(plan, tp->lhs)) {
        ColumnPtr col = c.df->cols[c.df->find(cx->name)];
        int64_t cmn = 0, cmx = 0;
        bool have = false;
        if (col->values && ops::int_range(col, &cmn, &cmx, col->range_verified)) have = true;
        else if (col->range_state == 1) { have = true; cmn = col->range_min; cmx = col->range_max; }
        else if (col->range_state == 2) have = true;      // no valid row: any range will do
        const int64_t tpd = temporal::ticks_per_day(tunit);
        auto day_of = [&](int64_t v) { return tunit == temporal::kUnitDate ? (int64_t)(int32_t)v : (v / tpd - ((v % tpd) < 0 ? 1 : 0)); };
        if (have && tpart == temporal::kDatePart && (day_of(cmn) < temporal::kI32Min || day_of(cmx) > temporal::kI32Max)) have = false;      // (the low 32 bits of such a day count are not monotone)
        if (have) {
          info[i].have_range = true; info[i].mn = temporal::part(cmn, tunit, tpart); info[i].mx = temporal::part(cmx, tunit, tpart);
          kp.note += "KeyRange{" + std::string(cx->name) + (tpart == temporal::kYear ? ".dt.year" : ".dt.date") + ": " + std::to_string(info[i].mn) + ".." + std::to_string(info[i].mx) + " from the column's range}; ";
        } else all_packable = false;
      } else all_packable = false;
    }
    else if (dtype_is_int(part.dtype) && x) {
      ColumnPtr col = c.df->cols[c.df->find(x->name)];
      bool cheap = dtype_width(part.dtype) <= 2 || nk > 1 || col->range_state != 0;
      // A single wide key whose range nobody has looked at yet: the range pass over it costs 8 B / row (1.5 ms per 1e9 rows) -- worth it exactly when the keys are
      // dense ids, which then take the direct-address tables at once instead of hash partitions on this run and direct ones on the next (1e9 rows over 1e6 dense ids:
      // first run 10.2 -> 7 ms; zipf-distributed ones, whose sample undercounts the groups and overflowed the hash tables once: 22.8 -> 9 ms).  A sample of 65536
      // rows says whether they LOOK dense (sparse 64-bit keys span far more than 2^26 in any sample: no pass for them).
      if (!cheap && part.dtype != PLX_U64 && col->values && col->len >= ((int64_t)1 << 24) && learn_dense_ranges()) {
        int64_t smn = 0, smx = 0;
        if (k::sample_minmax(col, &smn, &smx) && (unsigned __int128)((__int128)smx - (__int128)smn) < ((unsigned __int128)1 << 26)) {
          cheap = true;
          // (a guess is safe for ONE non-nullable key: every id below 2^bits decodes to the right key whatever the bounds were, anything beyond is reported by the
          //  tables; a nullable key's null code sits right above the assumed maximum, and the parts of a multi-column key overflow into each other: exact passes there)
          if (nk == 1 && !info[i].nullable && assume_range(col)) kp.note += "KeyRange{" + std::string(x->name) + ": sample looks dense -> bounds assumed from the sample, checked per row}; ";
          else kp.note += "KeyRange{" + std::string(x->name) + ": sample looks dense -> range pass}; ";
        }
      }
      // several key columns: whether they bit-pack is decided from their ranges -- guessed from the sample like a single key's (a sampled span beyond 2^62 settles it
      // without any pass: such a column packs with nothing)
      bool hopeless = false;
      if (cheap && nk > 1 && col->range_state == 0 && part.dtype != PLX_U64 && dtype_width(part.dtype) > 2 && col->values && col->len >= ((int64_t)1 << 24) && assume_ranges() && !col->no_assume) {
        int64_t smn = 0, smx = 0;
        if (k::sample_minmax(col, &smn, &smx, 1024) && (unsigned __int128)((__int128)smx - (__int128)smn) >= ((unsigned __int128)1 << 61)) hopeless = true;
        // (otherwise: the exact pass -- bounds that are only guessed must not pack several columns into one id: a value beyond its part's bits would spill into the next part)
      }
      if (part.dtype == PLX_U64 || hopeless) all_packable = false;
      else if (cheap) {
        // bounds that are only GUESSED (assume_range, possibly by an earlier query: as a single key under a filter -- only the passing rows were checked -- or as a narrowed
        // value column) may address ONE non-nullable key's table, where a wrong guess is reported; under a null code or packed next to other columns a value beyond them
        // would merge groups silently.  There: exact statistics, unless the guess has been verified over every row since.
        const bool may_assume = (nk == 1 && !info[i].nullable) || col->range_verified;
        if (col->values && ops::int_range(col, &info[i].mn, &info[i].mx, may_assume)) info[i].have_range = true;
        else if (col->range_state == 1) { info[i].have_range = true; info[i].mn = col->range_min; info[i].mx = col->range_max; }
        else if (col->range_state == 2) { info[i].have_range = true; info[i].mn = 0; info[i].mx = 0; }
        else all_packable = false;
      } else all_packable = false;
    } else all_packable = false;
    kp.parts.push_back(part);
  }
  int bits_total = 0;
  std::vector<int> bits(nk, 0);
  if (all_packable) {
    for (int i = 0; i < nk; i++) {
      unsigned __int128 range = (unsigned __int128)((__int128)info[i].mx - (__int128)info[i].mn) + 1 + (info[i].nullable ? 1 : 0);
      if (range > ((unsigned __int128)1 << 62)) { all_packable = false; break; }
      bits[i] = std::max(1, ceil_log2_u64((uint64_t)range));
      bits_total += bits[i];
    }
    if (bits_total > 62) all_packable = false;
  }
  if (all_packable) {
    kp.packed = true; kp.total_bits = bits_total;
    int acc = -1, shift = 0;
    for (int i = 0; i < nk; i++) {
      int n = knodes[i];
      if (info[i].mn != 0) n = c.mk(OP_SUB_I, n, c.konst((uint64_t)info[i].mn, 'i'), 'i');
      const uint64_t null_code = info[i].nullable ? (uint64_t)((__int128)info[i].mx - (__int128)info[i].mn + 1) : ~0ull;
      if (info[i].nullable) n = c.ifnull(n, null_code);
      if (shift) n = c.mk(OP_MUL_I, n, c.konst(1ull << shift, 'i'), 'i');
      acc = acc < 0 ? n : c.mk(OP_ADD_I, acc, n, 'i');
      KeyDecode& d = kp.parts[i].dec;
      d.shift = shift; d.mask = (1ull << bits[i]) - 1; d.min = info[i].mn; d.null_code = null_code; d.dtype = kp.parts[i].dtype;
      shift += bits[i];
    }
    c.key = acc;
    return kp;
  }
  if (nk != 1) {
    // wide key: the reference row-encodes (group_by/mod.rs:88-94); here each key column stays one
    // 64-bit word (floats canonicalised) and the hash sink compares the words.
    if (nk > kMaxKeys) throw Unsupported("more than " + std::to_string(kMaxKeys) + " group keys that do not bit-pack");
    kp.wide = true; kp.packed = false; kp.total_bits = 64 * nk;
    for (int i = 0; i < nk; i++) {
      int n = knodes[i];
      if (kp.parts[i].dtype == PLX_F64) n = c.mk(OP_CANON_F, n, n, 'f');
      kp.wide_nodes.push_back(n);
      kp.wide_nullable = kp.wide_nullable || c.nodes[n].nullable;
      KeyDecode& d = kp.parts[i].dec;
      d.shift = 0; d.mask = ~0ull; d.min = 0; d.null_code = ~0ull; d.dtype = kp.parts[i].dtype;
    }
    c.key = -1;
    c.wide_keys = kp.wide_nodes;
    return kp;
  }
  int n = knodes[0];
  if (kp.parts[0].dtype == PLX_F64) n = c.mk(OP_CANON_F, n, n, 'f');
  c.key = n;
  KeyDecode& d = kp.parts[0].dec;
  d.shift = 0; d.mask = ~0ull; d.min = 0; d.null_code = ~0ull; d.dtype = kp.parts[0].dtype;  // raw key: nullness comes from the valid flag
  kp.packed = false; kp.total_bits = 64;
  return kp;
}

// ------------------------------------------------------ fused pipeline driver -----
struct FusedAggResult {
  int64_t n_groups = 0;
  Buf acc;            // [n_groups][n_aggs] cells
  Buf packed_keys;    // [n_groups] u64 (group-by only)
  Buf key_valid;      // [n_groups] u8 flags (raw keys) or null
  Buf wide_words;     // wide keys: [n_keys][stride] u64
  Buf wide_valid;     // wide keys: [n_keys][stride] u8
  int64_t wide_stride = 0;
  int n_aggs = 0;
};

static uint64_t next_pow2(uint64_t x) { uint64_t p = 1; while (p < x) p <<= 1; return p; }

// distinct-count estimate from a sample: solve d = G (1 - exp(-S / G)) for G
static double estimate_groups(double d, double S) {
  if (d >= S * 0.999) return 1e18;
  double lo = d, hi = 1e15;
  for (int it = 0; it < 200; it++) { double mid = std::sqrt(lo * hi); double f = mid * (1.0 - std::exp(-S / mid)); if (f < d) lo = mid; else hi = mid; }
  return hi;
}

// occupied slots of an aggregation table -> dense (packed key, valid flag, cells) arrays in `res`.
// Small tables are compacted in ONE pass into slot-count-sized outputs (no count pass, one sync).
static int64_t compact_into(const uint64_t* keys, const uint64_t* acc, int64_t n_slots, int64_t cap, int n_aggs, int occ_agg, FusedAggResult& res) {
  int64_t upper = n_slots;
  if (n_slots > (int64_t(1) << 16)) upper = k::table_compact(keys, acc, n_slots, cap, n_aggs, occ_agg, nullptr, nullptr, nullptr);
  const int64_t g1 = std::max<int64_t>(upper, 1);
  res.packed_keys = dev_alloc(sizeof(uint64_t) * (size_t)g1);
  res.key_valid = dev_alloc((size_t)g1);
  res.acc = dev_alloc(sizeof(uint64_t) * (size_t)g1 * n_aggs);
  const int64_t g = k::table_compact(keys, acc, n_slots, cap, n_aggs, occ_agg, res.packed_keys->as<uint64_t>(), res.key_valid->as<uint8_t>(), res.acc->as<uint64_t>());
  res.n_groups = g; res.n_aggs = n_aggs;
  return g;
}

static int64_t run_hash_agg(const Shape& sh, const Args& args, int static_id, int log2_cap, int len_idx, FusedAggResult& out, bool count_only) {
  const uint64_t cap = 1ull << log2_cap;
  const int64_t slots = (int64_t)cap + 2;
  Buf keys = dev_alloc(sizeof(uint64_t) * (size_t)slots);
  Buf acc = dev_alloc(sizeof(uint64_t) * (size_t)slots * sh.n_aggs);
  Buf ovf = dev_alloc_zero(8);
  k::fill_u64(keys->as<uint64_t>(), slots, kEmptyKey);
  k::init_agg_cells(acc->as<uint64_t>(), slots, sh);
  HashTable t; t.keys = keys->as<unsigned long long>(); t.acc = acc->as<unsigned long long>(); t.overflow = ovf->as<unsigned int>(); t.wave_combine = 0;
  t.log2_cap = (uint32_t)log2_cap; t.max_probe = (uint32_t)std::min<uint64_t>(cap, 1u << 10);
  k::fused_hash_agg(sh, args, t, static_id);
  uint32_t o = 0; d2h_sync(&o, ovf->ptr, 4);
  if (o) return -1;
  if (count_only) return k::table_compact(keys->as<uint64_t>(), acc->as<uint64_t>(), slots, (int64_t)cap, sh.n_aggs, -1, nullptr, nullptr, nullptr);
  (void)len_idx;
  return compact_into(keys->as<uint64_t>(), acc->as<uint64_t>(), slots, (int64_t)cap, sh.n_aggs, -1, out);
}

static Args offset_args(const Shape& sh, const Args& a, int64_t row0, int64_t rows);
// `sample_blocks` > 0 (the planner's distinct-count sample; count_only): only that many evenly spaced blocks of args.n_rows / ... rows are aggregated -- `sample_rows` in
// all -- instead of the whole input: a prefix says nothing about clustered or sorted data (it undercounts, and the partitioned path then runs into full LDS tables).
// Blocks stay below the JIT threshold, so the sample runs the interpreter: no run-time compilation for a pass over a million rows.
static int64_t run_wide_agg(const Shape& sh, const Args& args, int log2_cap, bool nullable, FusedAggResult& out, bool count_only, int sample_blocks = 0, int64_t sample_rows = 0) {
  const uint64_t cap = 1ull << log2_cap;
  const int nw = sh.n_keys + (nullable ? 1 : 0);
  Buf tags = dev_alloc(sizeof(uint64_t) * cap);
  Buf words = dev_alloc(sizeof(uint64_t) * cap * (size_t)nw);
  Buf acc = dev_alloc(sizeof(uint64_t) * cap * sh.n_aggs);
  Buf ovf = dev_alloc_zero(8);
  k::fill_u64(tags->as<uint64_t>(), (int64_t)cap, kEmptyKey);
  k::init_agg_cells(acc->as<uint64_t>(), (int64_t)cap, sh);
  WideTable t; t.tags = tags->as<unsigned long long>(); t.words = words->as<unsigned long long>(); t.acc = acc->as<unsigned long long>();
  t.overflow = ovf->as<unsigned int>(); t.log2_cap = (uint32_t)log2_cap; t.max_probe = (uint32_t)std::min<uint64_t>(cap, 1u << 10);
  t.n_words = (uint32_t)nw; t.has_null_word = nullable ? 1u : 0u;
  if (sample_blocks > 0) {
    const int64_t n = args.n_rows, per = (sample_rows / sample_blocks) & ~(int64_t)127, stride = (n / sample_blocks) & ~(int64_t)127;
    for (int b = 0; b < sample_blocks; b++) {
      const int64_t row0 = (int64_t)b * stride, rows = std::min<int64_t>(per, n - row0);
      if (rows > 0) k::fused_wide_agg(sh, offset_args(sh, args, row0, rows), t);
    }
  } else k::fused_wide_agg(sh, args, t);
  uint32_t o = 0; d2h_sync(&o, ovf->ptr, 4);
  if (o) return -1;
  int64_t g = k::wide_compact(t, sh.n_keys, sh.n_aggs, 0, nullptr, nullptr, nullptr);
  if (count_only) return g;
  out.n_groups = g; out.n_aggs = sh.n_aggs;
  const int64_t stride = std::max<int64_t>(g, 1);
  out.wide_stride = stride;
  out.wide_words = dev_alloc(sizeof(uint64_t) * (size_t)stride * sh.n_keys);
  out.wide_valid = dev_alloc((size_t)stride * sh.n_keys);
  out.acc = dev_alloc(sizeof(uint64_t) * (size_t)stride * sh.n_aggs);
  k::wide_compact(t, sh.n_keys, sh.n_aggs, stride, out.wide_words->as<uint64_t>(), out.wide_valid->as<uint8_t>(), out.acc->as<uint64_t>());
  return g;
}

// Sample of the input for the group-by planner: kSampleBlocks evenly spaced blocks of rows (a prefix alone says nothing about
// clustered data) aggregated into one HBM hash table.  -> number of distinct keys in the sample (-1: table overflow) and the
// heavy hitters (keys holding >= 1/1024 of the sampled rows), which the partitioned path pre-aggregates instead of scattering.
constexpr int kSampleBlocks = 8;
// rows the partitioned group-by samples per query (distinct-count estimate + heavy hitters): 2^20 strided rows cost ~0.15 ms at
// 1e9 rows; a key is "hot" from 1/1024 of the sample up, i.e. 1024 occurrences
constexpr int64_t kPartSampleRows = (int64_t)1 << 20;
constexpr int64_t kHotFraction = 4096;
static Args offset_args(const Shape& sh, const Args& a, int64_t row0, int64_t rows) {
  Args o = a;
  for (int i = 0; i < sh.n_inputs; i++) {
    if (o.in[i].values) o.in[i].values = (const uint8_t*)o.in[i].values + (sh.in_dtype[i] == PLX_BOOL ? (size_t)(row0 / 8) : (size_t)row0 * dtype_width(sh.in_dtype[i]));
    if (o.in[i].validity) o.in[i].validity = o.in[i].validity + row0 / 64;
  }
  o.n_rows = rows;
  return o;
}
// Returns the number of distinct keys in the sample (-1: table overflow).  *groups_est (if given): estimated number of groups of the
// whole input -- the heavy hitters are taken out of the sample first (estimate_groups assumes equally likely keys: one key holding
// half of the rows would halve the estimate and the LDS tables planned from it would run at twice their load).
static int64_t sample_keys(const Shape& full, const Args& args, int static_id, int full_len_idx, int64_t S, std::vector<uint64_t>* hot, double* groups_est) {
  // the sample only counts rows per key: the query's other aggregates are dropped (half the table atomics for a two-aggregate
  // query), which makes it a different program shape -- 2^20 rows in blocks below the JIT threshold run the interpreter, fast enough
  Shape sh = full;
  int len_idx = full_len_idx;
  if (full_len_idx >= 0 && full.n_aggs > 1) { sh.n_aggs = 1; sh.aggs[0] = full.aggs[full_len_idx]; len_idx = 0; static_id = -1; }
  const int log2_cap = ceil_log2_u64((uint64_t)S) + 1;
  const uint64_t cap = 1ull << log2_cap;
  const int64_t slots = (int64_t)cap + 2;
  Buf keys = dev_alloc(sizeof(uint64_t) * (size_t)slots), acc = dev_alloc(sizeof(uint64_t) * (size_t)slots * sh.n_aggs), ovf = dev_alloc_zero(8);
  k::fill_u64(keys->as<uint64_t>(), slots, kEmptyKey);
  k::init_agg_cells(acc->as<uint64_t>(), slots, sh);
  HashTable t; t.keys = keys->as<unsigned long long>(); t.acc = acc->as<unsigned long long>(); t.overflow = ovf->as<unsigned int>(); t.wave_combine = 1;
  t.log2_cap = (uint32_t)log2_cap; t.max_probe = 1u << 14;
  const int64_t n = args.n_rows, per = (S / kSampleBlocks) & ~(int64_t)127, stride = (n / kSampleBlocks) & ~(int64_t)127;
  for (int b = 0; b < kSampleBlocks; b++) {
    const int64_t row0 = (int64_t)b * stride;
    const int64_t rows = std::min<int64_t>(per, n - row0);
    if (rows > 0) k::fused_hash_agg(sh, offset_args(sh, args, row0, rows), t, static_id);
  }
  uint32_t o = 0; d2h_sync(&o, ovf->ptr, 4);
  if (o) return -1;
  uint64_t hot_rows = 0;
  // a key is "hot" from 1/4096 of the sampled rows (256 of 2^20: a stable count) -- at 1e9 rows ~2.4e5 rows that would otherwise serialise on one LDS address
  // in one aggregation workgroup (~0.5 ms); the kP2MaxHot heaviest are kept
  if (hot) k::select_hot_keys(t, sh.n_aggs, len_idx, (uint64_t)std::max<int64_t>(64, (per * kSampleBlocks) / kHotFraction), hot, &hot_rows);
  const int64_t d = k::table_compact(keys->as<uint64_t>(), acc->as<uint64_t>(), slots, (int64_t)cap, sh.n_aggs, -1, nullptr, nullptr, nullptr);
  if (groups_est) {
    const double n_hot = hot ? (double)hot->size() : 0.0, s_rest = std::max(1.0, (double)(per * kSampleBlocks) - (double)hot_rows), d_rest = std::max(0.0, (double)d - n_hot);
    *groups_est = d < 0 ? 1e18 : (d_rest > 0 ? estimate_groups(d_rest, s_rest) : 0.0) + n_hot;
  }
  return d;
}
// PLX_PROBE_PARTITIONED: 0 = never, 2 = whenever the kernels are available (tests: small inputs, any key order), default = by size / density / key order
// The partitioned (LDS-filled) build of a join hash table: PLX_JOIN_PART_BUILD = 0 never | 1 (default) build sides of >= 2^24 rows | 2 whenever the geometry allows.
// Windows of 2^13 slots (96 KB of LDS: 8-byte keys + 4-byte rows), no larger than a region of the partitioned probe (256 regions: kernels_partition.hip probe_pass_kernel).
static const uint32_t kJoinWindowLog2 = [] { const char* e = getenv("PLX_JOIN_WINDOW_LOG2"); const int v = e ? atoi(e) : 13; return (uint32_t)(v >= 10 && v <= 13 ? v : 13); }();      // (PLX_JOIN_WINDOW_LOG2: measurement)
static bool partitioned_build_wanted(int64_t build_rows, int log2_cap) {
  const char* e = getenv("PLX_JOIN_PART_BUILD");      // (read at every build: the tests switch it)
  const int mode = e ? atoi(e) : 1;
  if (mode <= 0 || log2_cap < (int)kJoinWindowLog2 + 8) return false;
  return mode >= 2 || build_rows >= ((int64_t)1 << 24);
}
static int partitioned_probe_mode() { const char* e = getenv("PLX_PROBE_PARTITIONED"); return e && e[0] == '0' ? 0 : e && e[0] == '2' ? 2 : 1; }
static bool probe_late_loads() { static const bool v = [] { const char* e = getenv("PLX_PROBE_LATE"); return !(e && e[0] == '0'); }(); return v; }
static int part_version() { static const int v = [] { const char* e = getenv("PLX_PART_V"); return (e && e[0] == '1') ? 1 : 2; }(); return v; }
static bool hot_keys_enabled() { static const bool v = [] { const char* e = getenv("PLX_PART_HOT"); return !(e && e[0] == '0'); }(); return v; }

// Value ranges of the record sources that are plain integer columns (cached column statistics, one reduction pass the first time a
// column is asked): the partitioned group-by packs its records with them (fused::kPackNarrow / kPackFused).
static void source_ranges(const Compiler& c, k::SrcRange out[kMaxSrc]) {
  const Shape& sh = c.shape;
  const RecLayout2 L = rec_layout2(sh, kP2Hash, kPackNarrow);
  for (uint32_t j = 0; j < L.n_src && j < (uint32_t)kMaxSrc; j++) {
    out[j] = k::SrcRange{};
    const int in = slot_input(sh, L.src_slot[j]);
    if (in < 0 || in >= (int)c.input_cols.size()) continue;
    const ColumnPtr& col = c.cols[c.input_cols[in]];
    if (!dtype_is_int(col->dtype) || col->dtype == PLX_U64) continue;
    // make_record2 stores (v - base) in 32 bits WITHOUT a per-row range check: only ranges the library computed itself may narrow a value
    // (bounds declared by the caller -- plx_column_set_bounds, IPC dictionary sizes -- are checked per row where they address tables, never trusted here)
    // -- except the planner's own guesses (assume_range): those narrow WITH a per-row check (PartPlan2::check_src) and a second run if it fails
    if (col->range_state == 0) assume_range(col);
    if (col->range_state != 0 && !col->range_trusted && !col->range_assumed) continue;
    int64_t mn = 0, mx = 0;
    if (ops::int_range(col, &mn, &mx, true)) { out[j].known = true; out[j].mn = mn; out[j].mx = mx; out[j].check = col->range_assumed && !col->range_verified; }
  }
}
// does any input column of the compiled query carry bounds nobody measured (declared by the caller, or assumed by the planner)?  Then the table sinks report ids outside
// their tables (LdsAggSink / DenseAggSink `oob`) and the host looks at the flag.
static bool untrusted_key_bounds(const Compiler& c) {
  for (auto& col : c.cols) if (col->range_state == 1 && !col->range_trusted) return true;
  return false;
}
static void check_oob_flag(const Buf& oob) {
  if (!oob) return;
  uint32_t f = 0;
  d2h_sync(&f, oob->ptr, 4);
  if (f) fail(PLX_ERR_INVALID, "group key outside the bounds declared or assumed for its column");
}
// A partitioned run WITHOUT a predicate put every row of its narrowed value columns through the per-row check (PartPlan2::check_src) and raised no flag: their assumed
// bounds are now verified -- valid for every row, if not tight -- and later runs take the kernels without the check.
static void mark_sources_verified(const Compiler& c) {
  const Shape& sh = c.shape;
  if (sh.pred != kNone) return;
  const RecLayout2 L = rec_layout2(sh, kP2Hash, kPackNarrow);
  for (uint32_t j = 0; j < L.n_src && j < (uint32_t)kMaxSrc; j++) {
    const int in = slot_input(sh, L.src_slot[j]);
    if (in < 0 || in >= (int)c.input_cols.size()) continue;
    const ColumnPtr& col = c.cols[c.input_cols[in]];
    if (col->range_assumed) col->range_verified = true;
  }
}

// The planner's sample of a key column (see Column::key_sample).
// `sig`: the program that produced the sampled key VALUES (ops + immediates): the same column enters as raw values on its first group-by and -- once its range has
// been learned -- as packed ids (key - min) on the next; hot keys of one encoding never match rows of the other (a stale list is harmless for the result
// -- the rows simply take the scatter -- but one key holding half of the rows then costs 28 ms of same-address LDS atomics instead of 0.1 ms)
struct KeySample { int64_t n_rows = 0, distinct = -1; double groups_est = 1e18; std::vector<uint64_t> hot; bool with_hot = false; uint64_t sig = 0; };
static uint64_t key_program_signature(const Shape& sh, const Args& args) {
  uint64_t h = 0xcbf29ce484222325ull;
  auto mix = [&](const void* p, size_t n) { const unsigned char* b = (const unsigned char*)p; for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001b3ull; } };
  mix(&sh, sizeof(Shape));
  mix(args.imm, sizeof(args.imm));
  return h;
}
// the frame column a single-column group key reads directly, when the query has no predicate (then the sample depends on nothing else)
static ColumnPtr plain_key_column(const Compiler& c, const KeyPlan& kp) {
  if (c.shape.pred != kNone || kp.parts.size() != 1) return nullptr;
  const AE* x = plain_column(c.plan, kp.parts[0].expr);
  if (!x) return nullptr;
  const int ci = c.df->find(x->name);
  return ci >= 0 && c.df->cols[ci]->len == c.args.n_rows ? c.df->cols[ci] : nullptr;
}
static bool sample_cache_enabled() { static const bool v = [] { const char* e = getenv("PLX_SAMPLE_CACHE"); return !(e && e[0] == '0'); }(); return v; }
static int64_t sample_keys(const Shape& full, const Args& args, int static_id, int full_len_idx, int64_t S, std::vector<uint64_t>* hot, double* groups_est);
static int64_t sample_keys_cached(const ColumnPtr& key_col, const Shape& sh, const Args& args, int static_id, int len_idx, int64_t S, std::vector<uint64_t>* hot, double* groups_est,
                                  std::string& desc) {
  // (atomic_load / atomic_store: two host threads may plan group-bys over the same column at once -- each on its own stream, core.cpp)
  const std::shared_ptr<void> held = key_col && sample_cache_enabled() ? std::atomic_load(&key_col->key_sample) : nullptr;
  if (held) {
    const KeySample& ks = *std::static_pointer_cast<KeySample>(held);
    if (ks.n_rows == args.n_rows && (ks.with_hot || !hot) && ks.sig == key_program_signature(sh, args)) {
      if (hot) *hot = ks.hot;
      if (groups_est) *groups_est = ks.groups_est;
      desc += "cached_";
      return ks.distinct;
    }
  }
  double g = 1e18;
  const int64_t d = sample_keys(sh, args, static_id, len_idx, S, hot, &g);
  if (groups_est) *groups_est = g;
  if (key_col && sample_cache_enabled() && d >= 0) {
    auto ks = std::make_shared<KeySample>();
    ks->n_rows = args.n_rows; ks->distinct = d; ks->groups_est = g; ks->with_hot = hot != nullptr; ks->sig = key_program_signature(sh, args);
    if (hot) ks->hot = *hot;
    std::atomic_store(&key_col->key_sample, std::shared_ptr<void>(ks));
  }
  return d;
}

// ---- encoded inputs: narrow shadows of low-cardinality columns (encoded_inputs.hpp, DESIGN.md "Encoded shadows") ----
// The whole policy lives here.  A column QUALIFIES in a scan when the program reads it whole through a plain OP_LOAD, the scan ends in the register or the LDS
// aggregate sink (the only callers), the library owns its buffer (a borrowed one can be rewritten by its owner behind our back), and its codes would take at most a
// quarter of its bytes: 8-byte integers and f64, 4-byte integers when one byte a row is enough -- or half of them, for an f64 column of decimals of at least
// kDecimalMinRows rows (build_decimal_shadow).  The SECOND qualifying scan since the statistics were last dropped
// tries to build the shadow before it launches; one that fails -- too many values, no memory, a row that does not decode to itself -- is never tried again.
static bool encoded_inputs_enabled() { static const bool v = [] { const char* e = getenv("PLX_ENCODED_INPUTS"); return !(e && e[0] == '0'); }(); return v; }
// Decimal shadows take HALF the column's bytes, so they are built for columns of at least this many rows only (the figure at which the run-time compiler starts, jit.cpp):
// below it the scans are launch-bound, and 4 bytes a row saved is not worth 4 bytes a row held.  PLX_ENCODED_DECIMAL_MIN_ROWS / plx_encoded_set_decimal_min_rows.
constexpr int64_t kDecimalMinRows = (int64_t)1 << 22;
static std::atomic<int64_t> g_decimal_min_rows{[] { const char* e = getenv("PLX_ENCODED_DECIMAL_MIN_ROWS"); return e && e[0] ? (int64_t)atoll(e) : kDecimalMinRows; }()};
void encoded_set_decimal_min_rows(int64_t min_rows) { g_decimal_min_rows.store(min_rows < 0 ? 0 : min_rows, std::memory_order_relaxed); }
int64_t encoded_decimal_min_rows() { return g_decimal_min_rows.load(std::memory_order_relaxed); }
// f64 column whose dictionary gave up -> u32 codes of its decimals (decimal.hpp), or null.  `step`: the stride of the sample (at most 2^20 rows): a column of arbitrary
// doubles is rejected by it in microseconds.  The sample chooses the exponent and whether base 0 will do; a base other than 0 is the EXACT minimum, from one full pass
// at the chosen exponent.  The encode pass checks every valid row: one that is no decimal at the exponent, or lies outside the codes' range, discards the shadow.
static std::shared_ptr<EncodedShadow> build_decimal_shadow(const ColumnPtr& col, int64_t step) {
  const int64_t n = col->len;
  if (n < g_decimal_min_rows.load(std::memory_order_relaxed)) return nullptr;
  const double* v = col->values->as<double>();
  decimal::Choice ch = decimal::choose(enc::decimal_stats(v, col->valid_words(), n, step < 1 ? 1 : step, 0, decimal::kMaxExp));
  if (ch.ok && step > 1 && ch.base != 0) ch = decimal::choose(enc::decimal_stats(v, col->valid_words(), n, 1, ch.e, ch.e), ch.e, ch.e);
  if (!ch.ok) return nullptr;
  auto s = std::make_shared<EncodedShadow>();
  s->kind = EncodedShadow::kDecimal; s->width = 4; s->base = ch.base; s->stride = (uint64_t)ch.e;
  s->codes = dev_alloc((size_t)((n + 7) / 8) * 8 * sizeof(uint32_t));      // the encoder stores eight codes at a time
  if (!enc::decimal_encode(v, col->valid_words(), n, ch.base, ch.e, s->codes->as<uint32_t>())) return nullptr;
  return s;
}
static std::shared_ptr<EncodedShadow> build_shadow(const ColumnPtr& col) {
  auto s = std::make_shared<EncodedShadow>();
  const int64_t n = col->len;
  const size_t groups = (size_t)((n + 7) / 8) * 8;      // the encoders store eight codes at a time
  if (col->dtype == PLX_F64) {
    std::vector<uint64_t> pats;
    const int64_t step = (n + ((int64_t)1 << 20) - 1) >> 20;      // a strided sample of at most 2^20 rows first: a high-cardinality column costs microseconds, not a pass
    const bool dict_ok = (step <= 1 || enc::dict_collect(col->values->as<uint64_t>(), col->valid_words(), n, step, &pats)) &&
                         enc::dict_collect(col->values->as<uint64_t>(), col->valid_words(), n, 1, &pats);
    if (!dict_ok) return build_decimal_shadow(col, step);      // too many patterns for a dictionary: a column of decimals still has four-byte codes
    if (pats.empty()) return nullptr;
    s->kind = EncodedShadow::kDict; s->width = 1; s->n_dict = (int)pats.size();
    pats.resize(kDictSlots, 0);
    s->dict = dev_alloc(sizeof(uint64_t) * kDictSlots);
    s->codes = dev_alloc(groups);
    h2d_async(s->dict->ptr, pats.data(), sizeof(uint64_t) * kDictSlots);
    PLX_HIP(hipStreamSynchronize(stream()));
    if (!enc::dict_encode(col->values->as<uint64_t>(), col->valid_words(), n, s->dict->as<unsigned long long>(), s->n_dict, s->codes->as<uint8_t>())) return nullptr;
    return s;
  }
  // integers: the EXACT range of the valid rows -- the column's cached one only when the library measured it itself, never declared or assumed bounds
  int64_t mn, mx;
  if (col->range_state == 1 && col->range_trusted && !col->range_assumed) { mn = col->range_min; mx = col->range_max; }
  else {
    const k::ReduceResult rr = k::reduce_all(col->dtype, col->data(), col->valid_words(), n);
    if (rr.n_valid == 0) return nullptr;
    mn = (int64_t)rr.minmax_lo; mx = (int64_t)rr.minmax_hi;
  }
  uint64_t g = 0;
  if (enc::affine_needs_gcd(mn, mx)) {
    if (col->dtype != PLX_I64) return nullptr;      // (a 4-byte column needs one-byte codes: a span past 65535 would have to be a multiple of 2^8 strides -- not worth a pass)
    g = enc::affine_gcd(col->values->as<int64_t>(), col->valid_words(), n, mn);
  }
  const enc::AffineChoice ch = enc::choose_affine(mn, mx, g);
  if (!ch.ok || ch.width * 4 > dtype_width(col->dtype)) return nullptr;
  s->kind = EncodedShadow::kAffine; s->width = ch.width; s->base = ch.base; s->stride = ch.stride;
  s->codes = dev_alloc(groups * (size_t)ch.width);
  if (!enc::affine_encode(col->dtype, col->data(), col->valid_words(), n, ch.base, ch.stride, ch.width, s->codes->ptr)) return nullptr;
  return s;
}
// the shadow this scan of `col` reads, or null; `may_build`: this is a scan that runs (a compile-only caller sees what is there and counts nothing)
static std::shared_ptr<EncodedShadow> encoded_shadow_for_scan(const ColumnPtr& col, bool may_build) {
  if (!encoded_inputs_enabled()) return nullptr;
  std::shared_ptr<EncodedShadow> s = std::atomic_load(&col->shadow);
  if (s && s->kind != EncodedShadow::kNone) return s;
  if (!may_build || (s && s->never_encode) || !col->values || !col->values->owned || col->len <= 0) return nullptr;
  if (col->dtype != PLX_I64 && col->dtype != PLX_F64 && col->dtype != PLX_I32 && col->dtype != PLX_U32) return nullptr;
  auto next = std::make_shared<EncodedShadow>();
  next->scans = (s ? s->scans : 0) + 1;
  if (next->scans >= 2) {
    std::shared_ptr<EncodedShadow> built;
    try { built = build_shadow(col); }
    catch (const Error& e) { if (e.code != PLX_ERR_OOM) throw; (void)hipGetLastError(); }      // no memory for the codes: the query runs plain
    if (built) { built->scans = next->scans; next = built; }
    else next->never_encode = true;
  }
  std::atomic_store(&col->shadow, next);
  return next->kind != EncodedShadow::kNone ? next : nullptr;
}
// The program a register / LDS aggregate scan runs: c.shape / c.args, or their rewrite over the shadows of the inputs that have one.
struct ScanProgram { Shape shape; Args args; int static_id; std::string note; };
static ScanProgram scan_program_with_encodings(const Compiler& c, bool may_build) {
  ScanProgram sp{c.shape, c.args, -1, ""};
  enc::InputEncoding e[kMaxInputs];
  bool any = false;
  for (int i = 0; i < c.shape.n_inputs; i++) {
    const ColumnPtr& col = c.cols[c.input_cols[i]];
    if (c.args.in[i].values != col->data() || c.args.n_rows != col->len) continue;      // not the whole column
    const std::shared_ptr<EncodedShadow> s = encoded_shadow_for_scan(col, may_build);
    if (!s) continue;
    e[i].kind = s->kind; e[i].width = s->width; e[i].base = s->base; e[i].stride = s->stride;
    e[i].codes = s->codes ? s->codes->ptr : nullptr; e[i].dict = s->dict ? s->dict->as<unsigned long long>() : nullptr;
    any = true;      // (the codes outlive the launch: a buffer freed later goes back to a pool that is stream-ordered, see DevBuf)
  }
  uint32_t taken = 0;
  if (any && enc::encode_program(c.shape, c.args, e, &sp.shape, &sp.args, &taken)) {
    sp.note = "encoded{";
    bool first = true;
    for (int i = 0; i < c.shape.n_inputs; i++) {
      if (!((taken >> i) & 1u)) continue;
      std::string name = "?";
      for (size_t j = 0; j < c.df->cols.size(); j++) if (c.df->cols[j] == c.cols[c.input_cols[i]]) name = c.df->names[j];
      sp.note += std::string(first ? "" : ",") + name + ":" + (e[i].kind == EncodedShadow::kDict ? "dict" : e[i].kind == EncodedShadow::kDecimal ? "decimal" : "affine") + std::to_string(8 * e[i].width);
      first = false;
    }
    sp.note += "}";
  }
  sp.static_id = find_static_shape(sp.shape);
  return sp;
}

// ---- the fused group-by driver: run_fused_groupby chooses the route, each route is one function that says whether it produced the result ----
namespace {
// What a route needs to finish the RESULT itself -- the output columns, not only the cells: the finalisation of every aggregate (the key parts are in the KeyPlan) --
// and the columns it hands back when it did (`taken`).  Only lds_table looks at it (groupby_tail_finish below).
struct TailRequest {
  const std::vector<FinalSpec>& specs;
  std::vector<ColumnPtr> key_cols, agg_cols;      // one per key part / per spec, `res.n_groups` rows each, host mirrors attached
  bool taken = false;
};
// what the routes of one run share
struct GroupByRun {
  Compiler& c; const KeyPlan& kp; const Shape& sh; const Args& args;      // (sh, args: c.shape, c.args)
  const int len_idx, static_id;
  const bool may_partition;      // the plan allows the partitioned routes and the input is large enough for them to pay
  FusedAggResult& res; std::string& desc;
  TailRequest* tail = nullptr;   // null: the route leaves cells and packed keys in `res` and the caller finalises them
};
bool groupby_tail_finish(GroupByRun& q, const Buf& cells, int G, const Buf& oob);
// "fused_scan[<mode>]+": how the scan program in front of a sink was obtained
std::string scan_tag(int static_id, int64_t n_rows) { return std::string("fused_scan[") + jit::program_mode(static_id, n_rows) + "]+"; }

// the table-in-one-kernel routes end alike: compact the cells, then look at the flag the sink raises for a group id outside its table
void finish_table(GroupByRun& q, const Buf& cells, int64_t G, const Buf& oob) {
  compact_into(nullptr, cells->as<uint64_t>(), G, -1, q.sh.n_aggs, q.len_idx, q.res);
  check_oob_flag(oob);
  q.res.key_valid = nullptr;  // packed keys carry their own null codes
}
// What the library KNOWS about the values of input i of the running program (q.sh / q.args: plain, or rewritten over shadows): the codes of an affine shadow span their
// width, a narrow integer column its type, a 64-bit column its measured range -- exact statistics only, never bounds a caller declared or the planner assumed.
bool input_value_bounds(const GroupByRun& q, int i, int64_t* lo, int64_t* hi) {
  if (i < 0 || i >= (int)q.c.input_cols.size() || q.args.in[i].validity) return false;
  const ColumnPtr& col = q.c.cols[q.c.input_cols[i]];
  const std::shared_ptr<EncodedShadow> s = std::atomic_load(&col->shadow);
  const bool codes = s && s->kind == EncodedShadow::kAffine && s->codes && q.args.in[i].values == s->codes->ptr;
  if (!codes && q.args.in[i].values != col->data()) {
    // rows [off, off + n) of the column: its statistics cover them
    const char* p = (const char*)q.args.in[i].values; const char* b = (const char*)col->data();
    if (!b || p < b || p >= b + (size_t)col->len * dtype_width(col->dtype) || q.sh.in_dtype[i] != col->dtype) return false;
  }
  switch (q.sh.in_dtype[i]) {
    case PLX_U8: *lo = 0; *hi = 255; return true;
    case PLX_U16: *lo = 0; *hi = 65535; return true;
    case PLX_U32: *lo = 0; *hi = 0xffffffffll; return true;
    case PLX_I8: *lo = -128; *hi = 127; return true;
    case PLX_I16: *lo = -32768; *hi = 32767; return true;
    case PLX_I32: *lo = INT32_MIN; *hi = INT32_MAX; return true;
    case PLX_I64: case PLX_U64:
      if (codes || col->range_state != 1 || !col->range_trusted || col->range_assumed) return false;
      if (q.sh.in_dtype[i] == PLX_U64 && col->range_min < 0) return false;
      *lo = col->range_min; *hi = col->range_max; return true;
    default: return false;
  }
}
// the cell plan of this scan (fused_cells.hpp): facts about the sources of its integer sums, from the columns behind the inputs
CellPlan shared_cells_plan(const GroupByRun& q) {
  AggFacts f{};
  f.n_rows = (uint64_t)q.args.n_rows; f.wg_rows = k::lds_agg_wg_rows(q.args.n_rows);
  for (int k = 0; k < q.sh.n_aggs; k++) {
    if (q.sh.aggs[k].kind != AGG_SUM_I) continue;
    const int in = affine_source_input(q.sh, q.sh.aggs[k].src);
    int64_t lo = 0, hi = 0;
    if (in < 0 || !input_value_bounds(q, in, &lo, &hi) || !affine_source_interval(q.sh, q.args, q.sh.aggs[k].src, &lo, &hi)) continue;
    f.known[k] = 1; f.lo[k] = lo; f.hi[k] = hi;
  }
  return plan_cells(q.sh, f);
}
void lds_table(GroupByRun& q) {
  const int G = 1 << q.kp.total_bits;
  Buf cells = dev_alloc(sizeof(uint64_t) * (size_t)G * q.sh.n_aggs);
  Buf oob = untrusted_key_bounds(q.c) ? dev_alloc_zero(8) : nullptr;      // key bounds nobody measured: the sink reports a group id outside the table
  const CellPlan cell_plan = shared_cells_plan(q);
  k::fused_lds_agg(q.sh, q.args, G, q.static_id, cells->as<uint64_t>(), oob ? oob->as<unsigned int>() : nullptr, &cell_plan);
  q.desc += scan_tag(q.static_id, q.args.n_rows) + "lds_table(G=" + std::to_string(G) + ",copies=" + std::to_string(k::lds_agg_copies(G, q.sh.n_aggs)) + ")";
  if (q.tail && groupby_tail_finish(q, cells, G, oob)) return;
  finish_table(q, cells, G, oob);
}
void dense_hbm_table(GroupByRun& q) {
  const int64_t G = (int64_t)1 << q.kp.total_bits;
  Buf cells = dev_alloc(sizeof(uint64_t) * (size_t)(G + 1) * q.sh.n_aggs);
  k::init_agg_cells(cells->as<uint64_t>(), G + 1, q.sh);
  Buf oob = untrusted_key_bounds(q.c) ? dev_alloc_zero(8) : nullptr;
  DenseTable t; t.acc = cells->as<unsigned long long>(); t.key_min = 0; t.n_groups = G; t.oob = oob ? oob->as<unsigned int>() : nullptr;
  k::fused_dense_agg(q.sh, q.args, t, q.static_id);
  q.desc += scan_tag(q.static_id, q.args.n_rows) + "dense_hbm_table(G=" + std::to_string(G) + ")";
  finish_table(q, cells, G, oob);
}

// what a partitioned aggregation hands back as group keys
enum PartKeys { kPackedIds /* carry their own null codes */, kKeysWithValidity, kWideWords };
void take_partitioned(GroupByRun& q, PartKeys keys, int64_t g, const Buf& ok, const Buf& okv, const Buf& oacc, int64_t stride, const std::string& pd) {
  FusedAggResult& res = q.res;
  res.n_groups = g; res.n_aggs = q.sh.n_aggs; res.acc = oacc;
  if (keys == kWideWords) { res.wide_words = ok; res.wide_valid = okv; res.wide_stride = stride; }
  else { res.packed_keys = ok; res.key_valid = keys == kKeysWithValidity ? okv : nullptr; }
  q.desc += scan_tag(q.static_id, q.args.n_rows) + pd;
}
// first-generation kernels (PLX_PART_V=1 only)
bool partitioned_v1(GroupByRun& q, double est_groups, bool any_nullable, PartKeys keys) {
  PartitionPlan pp;
  if (!k::partition_plan(q.sh, est_groups, any_nullable, &pp)) return false;
  std::string pd;
  Buf ok, okv, oacc;
  const int64_t g = k::partitioned_agg(q.sh, q.args, pp, q.static_id, &ok, &okv, &oacc, &pd);
  if (g < 0) { q.desc += "lds-overflow+"; return false; }
  take_partitioned(q, keys, g, ok, okv, oacc, 0, pd);
  return true;
}
// second generation: what its three call sites differ in
struct PartTry {
  double plan_for = 0;                // groups the LDS tables are planned for
  double fallback = 0;                // > 0: planned for instead, once, when `plan_for` fits no plan on the first attempt
  int packed_bits = -1;               // > 0: the key is a dense packed id of that many bits
  std::vector<uint64_t> hot;          // heavy hitters: aggregated in the scatter pass instead of being scattered
  k::SrcRange ranges[kMaxSrc];        // source_ranges(): filled by the caller, which reads its other statistics after that call
  k::SrcRange key_rng;                // exact range of the key / the packed id, where known
  ColumnPtr stat_col;                 // the column that learns its key range from the scatter pass
  int attempts = 3;                   // a table that fills up is reported by the aggregation pass: the plan grows and the pass is repeated
  bool grow_to_largest = false;       // growth rule after an overflow, see below
  PartKeys keys = kPackedIds;
};
bool partitioned_v2(GroupByRun& q, PartTry& t) {
  for (int attempt = 0; attempt < t.attempts; attempt++) {
    PartPlan2 p2;
    auto plan = [&](double groups) { return k::partition_plan2(q.sh, groups, t.packed_bits, q.len_idx, q.args.n_rows, (int)t.hot.size(), &p2, t.ranges, &t.key_rng); };
    if (!plan(t.plan_for) && !(attempt == 0 && t.fallback > 0 && plan(t.fallback))) return false;
    std::string pd;
    Buf ok, okv, oacc;
    int64_t key_range[2] = {1, 0}, stride = 0;
    const int64_t g = k::partitioned_agg2(q.sh, q.args, p2, q.static_id, t.hot, &ok, &okv, &oacc, &pd, t.stat_col ? key_range : nullptr, &stride);
    if (g >= 0) {
      if (t.stat_col && key_range[0] <= key_range[1]) { t.stat_col->range_state = 1; t.stat_col->range_min = key_range[0]; t.stat_col->range_max = key_range[1]; t.stat_col->range_trusted = true; pd += "+key_range_learned"; }
      if (p2.check_src) mark_sources_verified(q.c);
      if (t.keys == kKeysWithValidity) q.desc += "hot=" + std::to_string(t.hot.size()) + "+";      // (as found: the single-key site alone names its hot list here)
      take_partitioned(q, t.keys, g, ok, okv, oacc, stride, pd);
      return true;
    }
    if (g == -2) { q.desc += "v2-unavailable+"; return false; }
    q.desc += t.attempts == 1 ? "lds-overflow+" : "lds-overflow(P=" + std::to_string(1u << p2.log2_parts) + ")+";      // (as found: the one-attempt site does not name its P)
    if (p2.log2_parts >= 9) return false;
    // a table filled up: the sample undercounted (clustered keys).  grow_to_largest: one more attempt at the LARGEST plan (512 partitions); if that overflows too the HBM
    // table takes over -- never a ladder of full scatter + aggregate passes over all rows.  Otherwise: beyond what this plan's tables hold at all.
    // (as found: 0.8 of the largest plan's slots for wide keys, 1.01 of this plan's slots for a single key)
    t.plan_for = std::max(t.plan_for * 2.0, t.grow_to_largest ? (double)((uint64_t)p2.n_slots << 9) * 0.8 : (double)((uint64_t)p2.n_slots << p2.log2_parts) * 1.01);
  }
  return false;
}

// large inputs over many (packed) group ids: per-row atomics on the dense HBM table are bound by the device atomic
// rate just like the hash table -> partition + LDS aggregation on the packed id (kernels_partition.hip)
bool partitioned_packed_ids(GroupByRun& q) {
  const int bits = q.kp.total_bits;
  const int64_t n = q.args.n_rows;
  const double est = std::min((double)((uint64_t)1 << std::min(bits, 40)), (double)n);
  if (part_version() != 2) return partitioned_v1(q, est, false, kPackedIds);
  // second generation: direct-address LDS tables over the dense id when they fit (hash tables otherwise); a strided sample
  // finds the heavy hitters, which are aggregated in the scatter pass instead of being scattered
  PartTry t;
  t.plan_for = est; t.packed_bits = bits; t.attempts = 1;
  if (hot_keys_enabled() || bits > 25) {
    double g_est = 1e18;
    const int64_t d = sample_keys_cached(plain_key_column(q.c, q.kp), q.sh, q.args, q.static_id, q.len_idx, kPartSampleRows, hot_keys_enabled() ? &t.hot : nullptr, &g_est, q.desc);
    if (d >= 0) t.plan_for = std::min(est, std::min(g_est, (double)n) * 1.3);
    q.desc += "sample(distinct=" + std::to_string(d) + ",hot=" + std::to_string(t.hot.size()) + ")+";
  }
  const double hint = q.c.plan.group_hint;
  if (hint > 0) { t.plan_for = std::min(est, hint * 1.02 + 64.0); q.desc += "groups<=" + std::to_string((int64_t)hint) + "(plan)+"; }
  source_ranges(q.c, t.ranges);
  // (too many id bits for direct-address tables -> hash partitions of the packed id: its range is [0, 2^total_bits) by construction -- when the bounds behind the
  // packing were measured, not guessed -- so ids of < 48 bits travel as 48-bit offsets, two rows a record: fused::kPackPair)
  if (bits < 48 && !untrusted_key_bounds(q.c)) { t.key_rng.known = true; t.key_rng.mn = 0; t.key_rng.mx = (int64_t)(((uint64_t)1 << bits) - 1); }
  return partitioned_v2(q, t);
}

// hash table: size from a sampled distinct-count estimate.  groups < 0: an input too small to sample (and to partition)
struct HashSizing { double groups = -1.0; std::vector<uint64_t> hot; int log2_cap = 0; };
HashSizing size_hash_table(GroupByRun& q) {
  const KeyPlan& kp = q.kp;
  const int64_t n = q.args.n_rows;
  HashSizing hs;
  const int64_t S = (int64_t)1 << 22;
  if (n <= 2 * S) { hs.log2_cap = std::max(10, ceil_log2_u64((uint64_t)n * 2)); return hs; }
  Args sa = q.args; sa.n_rows = S;
  FusedAggResult tmp;
  const bool strided = q.may_partition && !kp.wide && part_version() == 2;
  const int64_t Sd = strided || kp.wide ? kPartSampleRows : S;
  double g_est = -1.0;
  int64_t d = kp.wide ? run_wide_agg(q.sh, q.args, 21, kp.wide_nullable, tmp, true, kSampleBlocks, Sd)
                      : (strided ? sample_keys_cached(plain_key_column(q.c, kp), q.sh, q.args, q.static_id, q.len_idx, Sd, hot_keys_enabled() ? &hs.hot : nullptr, &g_est, q.desc)
                                 : run_hash_agg(q.sh, sa, q.static_id, 23, q.len_idx, tmp, true));
  double G = d < 0 ? 1e18 : (g_est >= 0.0 ? g_est : estimate_groups((double)d, (double)Sd));
  G = std::min(G, (double)n);
  const double hint = q.c.plan.group_hint;
  if (hint > 0) { G = std::min(hint, (double)n); q.desc += "groups<=" + std::to_string((int64_t)hint) + "(plan)+"; }
  hs.groups = G;
  hs.log2_cap = std::max(12, ceil_log2_u64((uint64_t)(G * 2.0) + 1));
  q.desc += "sample(distinct=" + std::to_string(d) + "/" + std::to_string(Sd) + ")+";
  return hs;
}
// many rows, many groups: per-row global atomics are bound by the ~24 G/s device atomic rate; partition the
// rows and aggregate each partition in LDS instead (kernels_partition.hip)
// a wide (multi-column, unpackable) key takes the same partitioned path: records carry one word per key column, partitions come from the hash of the
// words + null mask, the LDS tables compare word by word (the reference row-encodes such keys: crates/polars-row, hash_keys.rs:334 RowEncodedKeys)
bool partitioned_wide_keys(GroupByRun& q, double G) {
  if (part_version() != 2) return false;
  PartTry t;
  source_ranges(q.c, t.ranges);
  t.plan_for = q.c.plan.group_hint > 0 ? G * 1.02 + 64.0 : G * 1.3;
  t.grow_to_largest = true; t.keys = kWideWords;
  return partitioned_v2(q, t);
}
bool partitioned_single_key(GroupByRun& q, double G, std::vector<uint64_t>& hot) {
  Compiler& c = q.c;
  if (part_version() != 2) {
    bool any_null = c.key >= 0 && c.nodes[c.key].nullable;
    for (auto& a : c.aggs) if (a.second >= 0 && c.nodes[a.second].nullable) any_null = true;
    return partitioned_v1(q, G * 1.3, any_null, kKeysWithValidity);
  }
  PartTry t;
  source_ranges(c, t.ranges);
  ColumnPtr key_col;      // the frame column behind a single plain signed-integer key
  const KeyPart* k0 = q.kp.parts.size() == 1 ? &q.kp.parts[0] : nullptr;
  if (k0 && dtype_is_int(k0->dtype) && k0->dtype != PLX_U64)
    if (const AE* x = plain_column(c.plan, k0->expr)) { const int ci = c.df->find(x->name); if (ci >= 0) key_col = c.df->cols[ci]; }
  // A raw signed-integer key column scanned without a predicate: the scatter pass also records the exact key range, which is
  // cached on the column like any other statistic -- the NEXT group-by / join on it can plan dense (direct-address) tables.
  if (key_col && q.sh.pred == kNone && key_col->range_state == 0 && key_col->len == q.args.n_rows) t.stat_col = key_col;
  // ... and once the exact range of such a key is known (learned that way, or computed): 64-bit keys spanning < 2^48 travel as 48-bit offsets, two rows a record
  // (fused::kPackPair in hash mode; only ranges the library computed itself: a declared or assumed range is never used unchecked)
  if (key_col && key_col->range_state == 1 && key_col->range_trusted) { t.key_rng.known = true; t.key_rng.mn = key_col->range_min; t.key_rng.mx = key_col->range_max; }
  // How many groups to plan for.  The estimate assumes equally likely keys; heavy hitters in the sample mean a heavy TAIL too, and a tail the sample
  // undercounts badly (zipf 1.1 over 1e6 keys: 1.5e5 distinct keys in 2^20 sampled rows, 1e6 in 1e9 rows): with skew the tables are planned for 4 x the
  // estimate.  A table that fills up anyway is reported by the aggregation pass; the plan is then doubled (more partitions) and the pass repeated -- never
  // the per-row HBM-table path, which a skewed input turns into seconds of same-address atomics.
  t.hot = std::move(hot);
  t.plan_for = c.plan.group_hint > 0 ? G * 1.02 + 64.0 : (!t.hot.empty() && G < 1e17) ? G * 4.0 : G * 1.3;      // (a bound from the plan is not an estimate: no safety factor)
  if (!t.hot.empty()) t.fallback = G * 1.3;      // 4 x does not fit 512 partitions: the plain estimate does
  t.keys = kKeysWithValidity;
  return partitioned_v2(q, t);
}
// hash / wide-hash HBM table of 2^log2_cap slots, grown x4 on overflow
void hash_hbm_table(GroupByRun& q, int log2_cap) {
  const KeyPlan& kp = q.kp;
  for (int attempt = 0; attempt < 8; attempt++) {
    int64_t g = kp.wide ? run_wide_agg(q.sh, q.args, log2_cap, kp.wide_nullable, q.res, false) : run_hash_agg(q.sh, q.args, q.static_id, log2_cap, q.len_idx, q.res, false);
    if (g >= 0) {
      q.desc += scan_tag(kp.wide ? -1 : q.static_id, q.args.n_rows) + (kp.wide ? "wide_hash_hbm_table(words=" + std::to_string(q.sh.n_keys + (kp.wide_nullable ? 1 : 0)) + ",cap=2^" : "hash_hbm_table(cap=2^") + std::to_string(log2_cap) + ")";
      return;
    }
    log2_cap += 2;
    q.desc += "grow+";
    PLX_REQUIRE(log2_cap <= 34, PLX_ERR_OOM, "group-by hash table would exceed 2^34 slots");
  }
  fail(PLX_ERR_OOM, "group-by hash table kept overflowing");
}
}  // namespace

static bool lds_table_route(const KeyPlan& kp, const Shape& sh) { return kp.packed && kp.total_bits <= 12 && k::lds_agg_copies(1 << kp.total_bits, sh.n_aggs) > 0; }
static void run_fused_groupby(Compiler& c, const KeyPlan& kp, int len_idx, FusedAggResult& res, std::string& desc, std::string& encoded, TailRequest* tail = nullptr) {
  const Shape& sh = c.shape;
  const int64_t n = c.args.n_rows;
  res.n_aggs = sh.n_aggs;
  if (n == 0) { res.n_groups = 0; res.acc = dev_alloc(8); res.packed_keys = dev_alloc(8); return; }
  GroupByRun q{c, kp, sh, c.args, len_idx, find_static_shape(sh), !(c.plan.flags & PLX_PLAN_NO_PARTITION) && n >= ((int64_t)1 << 24), res, desc, tail};
  if (lds_table_route(kp, sh)) {
    // the route is chosen on the plain program; this one may read encoded inputs (every other route keeps the plain program and its record packing)
    const ScanProgram sp = scan_program_with_encodings(c, true);
    if (sp.note.empty()) return lds_table(q);
    GroupByRun qe{c, kp, sp.shape, sp.args, len_idx, sp.static_id, q.may_partition, res, desc, tail};
    lds_table(qe);
    encoded += sp.note + "; ";      // (beside the plan text, not in it: Plan::encoded)
    return;
  }
  if (kp.packed && kp.total_bits > 12 && q.may_partition && partitioned_packed_ids(q)) return;
  if (kp.packed && kp.total_bits <= 28 && ((size_t)sh.n_aggs << (kp.total_bits + 3)) <= (size_t(8) << 30)) return dense_hbm_table(q);
  HashSizing hs = size_hash_table(q);
  if (q.may_partition && hs.groups >= 4096.0 && (kp.wide ? partitioned_wide_keys(q, hs.groups) : partitioned_single_key(q, hs.groups, hs.hot))) return;
  hash_hbm_table(q, hs.log2_cap);
}

// Output columns are allocated here and filled by ONE finalize_batch launch per query
// (was one launch per key and per aggregate: ~10 launches + 2 popcount syncs for TPC-H Q1).
// which finalisations can produce a null (a group none of whose rows counted), and the spec as the kernels take it
static bool final_nullable(const FinalSpec& fs) { return fs.kind == FIN_MEAN || fs.kind == FIN_MINMAX_I || fs.kind == FIN_MINMAX_F || fs.kind == FIN_VAR || fs.kind == FIN_STD; }
static FinalSpec final_job_spec(const FinalSpec& fs) {
  FinalSpec f = fs;
  if (fs.kind == FIN_COPY64 && dtype_width(fs.out_dtype) < 4) f.kind = FIN_NARROW;
  return f;
}
static ColumnPtr finalize_column(const FusedAggResult& r, const FinalSpec& fs, FinBatch& batch) {
  const int64_t G = r.n_groups;
  auto out = std::make_shared<Column>();
  out->dtype = fs.out_dtype; out->len = G;
  out->values = dev_alloc(values_bytes(fs.out_dtype, G));
  const bool nullable = final_nullable(fs);
  if (nullable) out->validity = dev_alloc_zero(bitmap_bytes(G)); else out->null_count = 0;
  const FinalSpec f = final_job_spec(fs);
  PLX_REQUIRE(batch.n < kMaxFinJobs, PLX_ERR_UNSUPPORTED, "too many output columns in one fused aggregation");
  FinJob& j = batch.jobs[batch.n++];
  j = FinJob{};
  j.is_key = 0; j.fs = f; j.out = out->values->ptr; j.out_valid = nullable ? out->validity->as<uint64_t>() : nullptr;
  return out;
}
// The end of every fused aggregation: a column per aggregate of `r`, the ONE finalize_batch launch of the result set (the caller has put its key columns into `batch`
// already; no groups: no launch), then the output expressions over those columns, appended to `frame`.
// the output expressions over the finalised aggregate columns (`overrides`: aggregate node -> its column of n_groups rows), appended to `frame`
static void append_output_expressions(const Plan& plan, const std::map<int, ColumnPtr>& overrides, const std::vector<int>& out_exprs, int64_t n_groups, Frame& frame) {
  Frame groups; groups.height = n_groups;
  for (int e : out_exprs) {
    Evaluated ev = eval(plan, e, groups, &overrides);
    frame.names.push_back(output_name(plan, e));
    frame.cols.push_back(broadcast(ev, n_groups));      // (a column of n_groups rows already, unless the expression is a scalar)
  }
}
static void append_aggregate_columns(const Plan& plan, const FusedAggResult& r, const std::vector<int>& agg_nodes, const std::vector<FinalSpec>& specs, const std::vector<int>& out_exprs, FinBatch& batch, Frame& frame) {
  std::map<int, ColumnPtr> overrides;
  for (size_t i = 0; i < agg_nodes.size(); i++) overrides[agg_nodes[i]] = finalize_column(r, specs[i], batch);
  k::finalize_batch(r.acc->as<uint64_t>(), r.n_aggs, r.n_groups, batch);
  append_output_expressions(plan, overrides, out_exprs, r.n_groups, frame);
}

static ColumnPtr decode_key_column(const FusedAggResult& r, const KeyPart& part, int key_index, FinBatch& batch) {
  const int64_t G = r.n_groups;
  auto out = std::make_shared<Column>();
  out->dtype = part.dtype; out->len = G;
  out->values = part.dtype == PLX_BOOL ? dev_alloc_zero(bitmap_bytes(G)) : dev_alloc(values_bytes(part.dtype, G));
  if (part.nullable) out->validity = dev_alloc_zero(bitmap_bytes(G)); else out->null_count = 0;   // a null key forms its own group
  KeyDecode kd = part.dec;
  if (part.dtype == PLX_F32) kd.dtype = PLX_F32;
  PLX_REQUIRE(batch.n < kMaxFinJobs, PLX_ERR_UNSUPPORTED, "too many output columns in one fused aggregation");
  FinJob& j = batch.jobs[batch.n++];
  j = FinJob{};
  j.is_key = 1; j.kd = kd; j.out = out->values->ptr; j.out_valid = part.nullable ? out->validity->as<uint64_t>() : nullptr;
  if (r.wide_words) {
    j.packed = r.wide_words->as<unsigned long long>() + (size_t)key_index * r.wide_stride;
    j.kvalid = r.wide_valid->as<unsigned char>() + (size_t)key_index * r.wide_stride;
  } else {
    j.packed = r.packed_keys->as<unsigned long long>();
    j.kvalid = r.key_valid ? r.key_valid->as<unsigned char>() : nullptr;
  }
  return out;
}

// ---- the tail of the LDS-table route in one kernel, one copy and one sync (k::groupby_tail, groupby_tail.hpp; DESIGN.md 4.11 "One tail kernel") ----
static thread_local int t_last_groupby_tail = 0;
int last_groupby_tail() { return t_last_groupby_tail; }
namespace {
// an output column of the tail: `rows` rows of capacity, nothing zeroed (the kernel writes every validity word it owns), and its job
ColumnPtr tail_column(int dtype, bool nullable, int64_t rows, FinJob& j) {
  auto out = std::make_shared<Column>();
  out->dtype = dtype; out->len = rows;
  out->values = dev_alloc(values_bytes(dtype, rows));
  if (nullable) out->validity = dev_alloc(bitmap_bytes(rows)); else out->null_count = 0;
  j = FinJob{};
  j.out = out->values->ptr; j.out_valid = nullable ? out->validity->as<uint64_t>() : nullptr;
  return out;
}
// The cells [G][n_aggs] of an LDS-table scan are enqueued: compact, decode the keys, finalise the aggregates and fetch the result.  false: not taken (nothing was
// launched) and the caller finishes the old way.  Raises what check_oob_flag raises, from the same place.
bool groupby_tail_finish(GroupByRun& q, const Buf& cells, int G, const Buf& oob) {
  TailRequest& t = *q.tail;
  const size_t n_cols = q.kp.parts.size() + t.specs.size();
  if (!k::groupby_tail_knob() || n_cols == 0 || n_cols > (size_t)kMaxFinJobs || G > gbt::kTailMaxSlots || !pinned_bounce()) return false;
  int32_t dtypes[kMaxFinJobs]; uint8_t nullable[kMaxFinJobs];
  int n = 0;
  for (const KeyPart& part : q.kp.parts) { dtypes[n] = part.dtype; nullable[n++] = part.nullable ? 1 : 0; }
  for (const FinalSpec& fs : t.specs) { dtypes[n] = fs.out_dtype; nullable[n++] = final_nullable(fs) ? 1 : 0; }
  gbt::TailLayout L;
  gbt::tail_layout(&L, G, dtypes, nullable, n);
  if (!gbt::tail_block_fits(L, kBounceBytes)) return false;
  // 1. the output columns at capacity G (pool allocations, no GPU work)
  FinBatch batch{};
  std::vector<ColumnPtr> cols;
  for (const KeyPart& part : q.kp.parts) {
    FinJob& j = batch.jobs[batch.n++];
    cols.push_back(tail_column(part.dtype, part.nullable, G, j));
    j.is_key = 1; j.kd = part.dec;
    if (part.dtype == PLX_F32) j.kd.dtype = PLX_F32;
  }
  for (const FinalSpec& fs : t.specs) {
    FinJob& j = batch.jobs[batch.n++];
    cols.push_back(tail_column(fs.out_dtype, final_nullable(fs), G, j));
    j.is_key = 0; j.fs = final_job_spec(fs);
  }
  // 2. behind the scan (and partials_finish_kernel): the tail kernel
  Buf block = dev_alloc(L.total);
  k::groupby_tail(cells->as<uint64_t>(), q.sh.n_aggs, G, q.len_idx, oob ? oob->as<unsigned int>() : nullptr, batch, block->ptr);
  // 3. one copy into the page-locked bounce buffer, one sync; the bytes are the mirror
  auto bytes = std::make_shared<std::vector<uint8_t>>(L.total);
  {
    std::lock_guard<std::mutex> lk(bounce_mutex());
    PLX_HIP(hipMemcpyAsync(pinned_bounce(), block->ptr, L.total, hipMemcpyDeviceToHost, stream()));
    PLX_HIP(hipStreamSynchronize(stream()));
    memcpy(bytes->data(), pinned_bounce(), L.total);
  }
  gbt::TailHeader h;
  memcpy(&h, bytes->data(), sizeof h);
  PLX_REQUIRE(h.version == gbt::kTailLayoutVersion && h.n_groups <= (uint32_t)G, PLX_ERR_INVALID, "group-by tail: the result block has no valid header");
  if (h.oob) fail(PLX_ERR_INVALID, "group key outside the bounds declared or assumed for its column");
  const int64_t g = h.n_groups;
  for (int j = 0; j < n; j++) {
    Column& c = *cols[j];
    c.len = g;
    auto m = std::make_shared<HostMirror>();
    m->bytes = bytes; m->values_off = L.values_off[j]; m->values_bytes = L.values_bytes[j];
    if (c.validity) {
      m->valid_off = L.valid_off[j]; m->valid_bytes = (size_t)L.words * 8;
      int64_t valid = 0;
      for (uint32_t w = 0; w < L.words; w++) { uint64_t x; memcpy(&x, bytes->data() + m->valid_off + (size_t)w * 8, 8); valid += (int64_t)gbt::tail_popc64(x); }
      c.null_count = g - valid;
    }
    c.host = std::move(m);
  }
  q.res.n_groups = g; q.res.n_aggs = q.sh.n_aggs; q.res.acc = cells;      // (the cells stay uncompacted: nobody reads them after the tail)
  t.key_cols.assign(cols.begin(), cols.begin() + (ptrdiff_t)q.kp.parts.size());
  t.agg_cols.assign(cols.begin() + (ptrdiff_t)q.kp.parts.size(), cols.end());
  t.taken = true;
  t_last_groupby_tail = 1;
  return true;
}
}  // namespace

// order groups by first occurrence (maintain_order): host argsort of the FIRST_ROW cells
static ColumnPtr first_row_permutation(const FusedAggResult& r, int first_idx) {
  const int64_t G = r.n_groups;
  std::vector<uint64_t> cells((size_t)G * r.n_aggs);
  d2h_sync(cells.data(), r.acc->ptr, cells.size() * 8);
  std::vector<uint32_t> perm((size_t)G);
  std::iota(perm.begin(), perm.end(), 0u);
  std::sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return cells[(size_t)a * r.n_aggs + first_idx] < cells[(size_t)b * r.n_aggs + first_idx]; });
  return column_from_host(PLX_U32, perm.data(), nullptr, 0, G);
}

// ---- machine-readable dump of a compiled pipeline (dump_program_json) ----
struct ProgramDump {
  std::string json;
};
static thread_local ProgramDump* t_program_dump = nullptr;   // set only for the duration of a dump_program_json call
static std::string jstr(const std::string& x) { std::string o = "\""; for (char ch : x) { if (ch == '"' || ch == '\\') o += '\\'; o += ch; } return o + "\""; }
// the register program of one compiled scan as JSON fields (no braces); input names are looked up in `frame` by buffer identity
static std::string program_fields(const Compiler& c, const Frame& frame, const Shape* sh_run = nullptr, const Args* args_run = nullptr) {
  std::ostringstream o;
  const Shape& sh = sh_run ? *sh_run : c.shape;      // (the program as it runs: c's own, or its rewrite over encoded inputs -- same inputs, same order)
  const Args& args = args_run ? *args_run : c.args;
  o << "\"n_rows\":" << c.args.n_rows << ",\"inputs\":[";
  auto name_of = [&](int col_id) -> std::string {   // input_cols holds the compiler's own column ids: map the buffer back to its frame column
    const ColumnPtr& buf = c.cols[col_id];
    for (size_t j = 0; j < frame.cols.size(); j++) if (frame.cols[j] == buf) return frame.names[j];
    return "?";
  };
  for (int i = 0; i < sh.n_inputs; i++)
    o << (i ? "," : "") << "{\"name\":" << jstr(name_of(c.input_cols[i])) << ",\"dtype\":" << (int)sh.in_dtype[i] << ",\"nullable\":" << (int)sh.in_nullable[i] << "}";
  o << "],\"ops\":[";
  for (int i = 0; i < sh.n_ops; i++)
    o << (i ? "," : "") << "[" << (int)sh.ops[i].code << "," << (int)sh.ops[i].dst << "," << (int)sh.ops[i].a << "," << (int)sh.ops[i].b << "," << (int)sh.ops[i].c << ",\"" << args.imm[i] << "\"]";
  o << "],\"pred\":" << (int)sh.pred << ",\"key\":" << (int)sh.key << ",\"keys\":[";
  for (int i = 0; i < sh.n_keys; i++) o << (i ? "," : "") << (int)sh.keys[i];
  o << "],\"aggs\":[";
  for (int i = 0; i < sh.n_aggs; i++) o << (i ? "," : "") << "[" << (int)sh.aggs[i].kind << "," << (int)sh.aggs[i].src << "]";
  o << "]";
  // ops the predicate / key depend on (a probe scan runs the others only for the lanes that find a build row)
  const ProgramSplit split = split_program(sh);
  o << ",\"early_mask\":" << split.early << ",\"any_late\":" << (split.any_late ? 1 : 0);
  return o.str();
}
static std::string finals_outputs_fields(const Plan& plan, const std::vector<int>& agg_nodes, const std::vector<FinalSpec>& specs, const std::vector<int>& out_exprs) {
  std::ostringstream o;
  o << "\"finals\":[";
  for (size_t i = 0; i < specs.size(); i++)
    o << (i ? "," : "") << "{\"kind\":" << (int)specs[i].kind << ",\"a\":" << (int)specs[i].a << ",\"b\":" << (int)specs[i].b << ",\"c\":" << (int)specs[i].c << ",\"out_dtype\":" << (int)specs[i].out_dtype << ",\"ddof\":" << (int)specs[i].ddof << "}";
  o << "],\"outputs\":[";
  for (size_t i = 0; i < out_exprs.size(); i++) {
    int e = out_exprs[i];
    while (plan.ae[e].kind == PLX_AE_ALIAS) e = plan.ae[e].lhs;
    int idx = -1;                                   // index into finals when the output IS one aggregate (else: a row expression over aggregates)
    for (size_t j = 0; j < agg_nodes.size(); j++) if (agg_nodes[j] == e) idx = (int)j;
    o << (i ? "," : "") << "{\"name\":" << jstr(output_name(plan, out_exprs[i])) << ",\"final\":" << idx << "}";
  }
  o << "]";
  return o.str();
}
static std::string compiled_json(const char* kind, const Plan& plan, const Compiler& c, const ScanProgram& sp, const KeyPlan* kp, const std::vector<int>& agg_nodes,
                                 const std::vector<FinalSpec>& specs, const std::vector<int>& out_exprs, int len_idx, int first_idx, bool maintain_order) {
  std::ostringstream o;
  o << "{\"kind\":\"" << kind << "\"," << program_fields(c, *c.df, &sp.shape, &sp.args);
  if (!sp.note.empty()) o << ",\"encoded\":" << jstr(sp.note);
  o << ",\"len_idx\":" << len_idx << ",\"first_idx\":" << first_idx << ",\"maintain_order\":" << (maintain_order ? 1 : 0);
  if (kp) {
    o << ",\"key_plan\":{\"packed\":" << (kp->packed ? 1 : 0) << ",\"wide\":" << (kp->wide ? 1 : 0) << ",\"parts\":[";
    for (size_t i = 0; i < kp->parts.size(); i++) {
      const KeyPart& kpart = kp->parts[i];
      o << (i ? "," : "") << "{\"name\":" << jstr(output_name(plan, kpart.expr)) << ",\"dtype\":" << kpart.dtype << ",\"nullable\":" << (kpart.nullable ? 1 : 0) << ",\"shift\":" << kpart.dec.shift
        << ",\"mask\":\"" << kpart.dec.mask << "\",\"min\":\"" << kpart.dec.min << "\",\"null_code\":\"" << kpart.dec.null_code << "\"}";
    }
    o << "]}";
  }
  o << "," << finals_outputs_fields(plan, agg_nodes, specs, out_exprs) << "}";
  return o.str();
}
static void dump_compiled(ProgramDump* dump, const char* kind, const Plan& plan, const Compiler& c, const ScanProgram& sp, const KeyPlan* kp, const std::vector<int>& agg_nodes,
                          const std::vector<FinalSpec>& specs, const std::vector<int>& out_exprs, int len_idx, int first_idx, bool maintain_order) {
  if (dump) dump->json = compiled_json(kind, plan, c, sp, kp, agg_nodes, specs, out_exprs, len_idx, first_idx, maintain_order);
}
// conjunction of the predicates `preds` lowered into `c`: its node, or -1 when there is none
static int and_predicates(Compiler& c, const std::vector<int>& preds) {
  int p = -1;
  for (int pe : preds) { int n = c.lower(pe); if (c.nodes[n].ty != 'b') throw Unsupported("predicate is not boolean"); p = p < 0 ? n : c.mk(OP_AND, p, n, 'b'); }
  return p;
}

// Select(aggregations) over [Filter]* over `src`
static bool fused_select(Plan& plan, const IRN& node, const std::vector<int>& preds, const FramePtr& src, FramePtr& out, Shape* shape_out, int* sid_out,
                         std::string* why, bool compile_only) {
  for (int e : node.exprs) if (contains_rowfn(plan, e)) { if (why) *why = rowfn_route_note(plan, e); return false; }
  for (int e : node.exprs) if (contains_window(plan, e)) { if (why) *why = "window expression: per-node route"; return false; }
  for (int e : node.exprs) if (!contains_agg(plan, e) || contains_column_outside_agg(plan, e)) { if (why) *why = "select mixes row expressions and aggregations"; return false; }
  // select(lit(2.5).sum()) aggregates a one-row literal (sum 2.5, count 1, whatever the filter keeps), as the per-node evaluator does: a fused program would
  // repeat the constant on every row it scans
  {
    std::vector<int> lit_check;
    for (int e : node.exprs) collect_aggs(plan, e, lit_check);
    for (int a : lit_check)
      if (plan.ae[a].kind == PLX_AE_AGG && !contains_column(plan, plan.ae[a].lhs)) {
        if (why) *why = "aggregate of a literal is a scalar, not a value per row; done by the per-node kernels";
        return false;
      }
  }
  Compiler c(plan, *src);
  c.device_pivot = !compile_only;
  std::vector<int> agg_nodes;
  std::vector<FinalSpec> specs;
  try {
    for (int e : node.exprs) collect_aggs(plan, e, agg_nodes);
    c.decline_order_statistics(agg_nodes);
    c.pred = and_predicates(c, preds);
    for (int a : agg_nodes) specs.push_back(c.lower_agg(a));
    c.finish();
  } catch (const Unsupported& u) { if (why) *why = u.why; return false; }
  const ScanProgram sp = scan_program_with_encodings(c, !compile_only && src->height > 0);
  const int static_id = sp.static_id;
  if (shape_out) *shape_out = sp.shape;
  if (sid_out) *sid_out = static_id;
  if (compile_only) { dump_compiled(t_program_dump, "select", plan, c, sp, nullptr, agg_nodes, specs, node.exprs, -1, -1, false); return true; }
  FusedAggResult r; r.n_groups = 1; r.n_aggs = c.shape.n_aggs;
  std::vector<uint64_t> host(kMaxAggs, 0);
  if (src->height == 0) { for (int k2 = 0; k2 < c.shape.n_aggs; k2++) host[k2] = agg_identity(c.shape.aggs[k2].kind); }
  else k::fused_regagg(sp.shape, sp.args, static_id, host.data());
  r.acc = dev_alloc(sizeof(uint64_t) * kMaxAggs);
  h2d_async(r.acc->ptr, host.data(), sizeof(uint64_t) * (size_t)c.shape.n_aggs);
  PLX_HIP(hipStreamSynchronize(stream()));
  plan.desc += c.var_note + std::string("FusedFilterAgg{fused_scan[") + jit::program_mode(static_id, c.args.n_rows) + "]+register_sink, inputs=" + std::to_string(c.shape.n_inputs) + ", ops=" + std::to_string(c.shape.n_ops) + ", aggs=" + std::to_string(c.shape.n_aggs) + "}; ";
  if (!sp.note.empty()) plan.encoded += sp.note + "; ";
  out = std::make_shared<Frame>();
  out->height = 1;
  FinBatch batch{};
  append_aggregate_columns(plan, r, agg_nodes, specs, node.exprs, batch, *out);
  return true;
}

// the columns' bounds that the planner had only ASSUMED (assume_range) are forgotten, and never guessed again; returns whether there was any
static bool forget_assumed_bounds(const std::vector<ColumnPtr>& cols) {
  bool guessed = false;
  for (auto& col : cols) if (col->range_assumed) { col->range_state = 0; col->range_trusted = true; col->range_assumed = false; col->range_verified = false; col->no_assume = true; std::atomic_store(&col->key_sample, std::shared_ptr<void>()); guessed = true; }
  return guessed;
}
// GroupBy(keys, aggregations) over [Filter]* over `src`
static bool fused_groupby(Plan& plan, const IRN& node, const std::vector<int>& preds, const FramePtr& src, FramePtr& out, Shape* shape_out, int* sid_out,
                          std::string* why, bool compile_only) {
  for (int e : node.exprs) if (contains_rowfn(plan, e)) { if (why) *why = rowfn_route_note(plan, e); return false; }
  for (int e : node.exprs) if (contains_window(plan, e)) { if (why) *why = "window expression: per-node route"; return false; }
  for (int e : node.exprs) if (!contains_agg(plan, e) || contains_column_outside_agg(plan, e)) { if (why) *why = "group_by aggregation list contains a non-aggregated column"; return false; }
  Compiler c(plan, *src);
  c.device_pivot = !compile_only;
  std::vector<int> agg_nodes;
  std::vector<FinalSpec> specs;
  KeyPlan kp;
  int len_idx = -1, first_idx = -1;
  try {
    for (int e : node.exprs) collect_aggs(plan, e, agg_nodes);
    c.decline_order_statistics(agg_nodes);
    c.pred = and_predicates(c, preds);
    kp = lower_keys(c, node.keys);
    len_idx = c.add_agg(AGG_LEN, -1);
    for (int a : agg_nodes) specs.push_back(c.lower_agg(a));
    if (node.maintain_order) first_idx = c.add_agg(AGG_FIRST_ROW, -1);
    c.finish();
  } catch (const Unsupported& u) { if (why) *why = u.why; return false; }
  if (compile_only) {
    // what the run would launch: the LDS-table route reads the encoded inputs that exist (nothing is counted or built here)
    const ScanProgram sp = lds_table_route(kp, c.shape) ? scan_program_with_encodings(c, false) : ScanProgram{c.shape, c.args, find_static_shape(c.shape), ""};
    if (shape_out) *shape_out = sp.shape;
    if (sid_out) *sid_out = sp.static_id;
    dump_compiled(t_program_dump, "group_by", plan, c, sp, &kp, agg_nodes, specs, node.exprs, len_idx, first_idx, node.maintain_order != 0);
    return true;
  }
  if (shape_out) *shape_out = c.shape;
  if (sid_out) *sid_out = find_static_shape(c.shape);
  FusedAggResult r;
  std::string d;
  // the LDS-table route may finish the result itself (groupby_tail_finish) -- not under maintain_order, whose permutation reads compacted cells
  TailRequest tail{specs};
  t_last_groupby_tail = 0;
  try {
    run_fused_groupby(c, kp, len_idx, r, d, plan.encoded, node.maintain_order ? nullptr : &tail);
  } catch (const Error& e) {
    // a row outside bounds the planner had only ASSUMED (assume_range): forget the guesses, never guess about these columns again, and run the query once more --
    // its statistics now come from exact passes.  (Bounds the caller declared are the caller's promise: that error stands.)
    if (!forget_assumed_bounds(c.cols) || e.code != PLX_ERR_INVALID) throw;
    plan.desc += "AssumedBoundsViolated{exact statistics, second run}; ";
    return fused_groupby(plan, node, preds, src, out, shape_out, sid_out, why, compile_only);
  }
  plan.desc += kp.note + c.var_note + "FusedFilterGroupBy{" + d + ", inputs=" + std::to_string(c.shape.n_inputs) + ", ops=" + std::to_string(c.shape.n_ops) + ", aggs=" + std::to_string(c.shape.n_aggs) + ", groups=" + std::to_string(r.n_groups) + "}; ";
  out = std::make_shared<Frame>();
  out->height = r.n_groups;
  if (tail.taken) {
    for (size_t pi = 0; pi < kp.parts.size(); pi++) { out->names.push_back(output_name(plan, kp.parts[pi].expr)); out->cols.push_back(tail.key_cols[pi]); }
    std::map<int, ColumnPtr> overrides;
    for (size_t i = 0; i < agg_nodes.size(); i++) overrides[agg_nodes[i]] = tail.agg_cols[i];
    append_output_expressions(plan, overrides, node.exprs, r.n_groups, *out);
    return true;
  }
  FinBatch batch{};
  for (size_t pi = 0; pi < kp.parts.size(); pi++) { out->names.push_back(output_name(plan, kp.parts[pi].expr)); out->cols.push_back(decode_key_column(r, kp.parts[pi], (int)pi, batch)); }
  append_aggregate_columns(plan, r, agg_nodes, specs, node.exprs, batch, *out);
  if (node.maintain_order && r.n_groups > 1) {
    ColumnPtr perm = first_row_permutation(r, first_idx);
    for (auto& col : out->cols) col = ops::gather(col, perm);
  }
  return true;
}


static int peel_filters_node(const Plan& plan, int input) { while (plan.ir[input].kind == PLX_IR_FILTER) input = plan.ir[input].input; return input; }
// peel [Filter]* below an aggregation node
static int peel_filters(const Plan& plan, int input, std::vector<int>& preds) {
  while (plan.ir[input].kind == PLX_IR_FILTER) { preds.push_back(plan.ir[input].predicate); input = plan.ir[input].input; }
  std::reverse(preds.begin(), preds.end());
  return input;
}

// ------------------------------------------------ fused Join -> GroupBy pipeline ----
// GroupBy(keys, aggs) directly over an inner Join of two ([Filter]* Scan) inputs, when
//   * the join has one plain-column integer key pair,
//   * the group keys are the join key plus plain columns of the BUILD side (the shorter input,
//     hash_join/mod.rs:41-50), so a group is one build row,
//   * every aggregate reads PROBE-side columns only,
//   * the build keys that survive the build-side predicate are unique (checked at run time).
// TPC-H Q3 has this shape.  Pipeline: count build rows -> build scan (predicate fused) -> probe scan
// (predicate + expressions fused, aggregates land in the matching slot) -> compact -> gather the
// build-side key columns.  Anything else returns false and the caller runs the per-node path.
// ---- inner joins that only FILTER (semi-join rewrite) ---------------------------------------------------------------------
// `X JOIN Y ON x = y` where one side (the filter side) has unique join keys and contributes no column to anything above the
// join is a semi join of the other (payload) side: TPC-H Q3's `customer[c_mktsegment == ..] JOIN orders` only restricts orders.
// The filter side becomes a membership bitmap over its key range (one fused scan of the filter side), the payload side's
// scan tests `bit(key)` as one more conjunct of its predicate (OP_BITLOOKUP) -- no join output is materialised.
struct SemiFilter {
  FramePtr F;                 // filter side
  std::vector<int> fpreds;    // its predicates
  int fkey = -1;              // join key column of F
  int pkey = -1;              // join key column of the payload frame
};
static void collect_columns(const Plan& plan, int e, std::set<std::string>& out) {
  if (e < 0) return;
  const AE& x = plan.ae.at(e);
  if (x.kind == PLX_AE_COLUMN) { out.insert(x.name); return; }
  collect_columns(plan, x.lhs, out);
  collect_columns(plan, x.rhs, out);
  collect_columns(plan, x.cond, out);
}
// Resolves one input of the outer join to a scan node: [Filter]* Scan, or [Filter]* Join(inner; A, B) with A, B = [Filter]* Scan
// where one of A / B is a pure filter with respect to `used` (the column names referenced above).  Appends the payload side's
// predicates to `preds` and the filter to `semis`; returns the payload scan node or -1 (why set).
// Full and right joins, and joins that keep both key columns (coalesce = 2), are served by the per-node route at every size: the reason the fused pipelines give (null: none).
static const char* join_takes_per_node_route(const IRN& jn) {
  if (jn.how == PLX_JOIN_FULL || jn.how == PLX_JOIN_RIGHT) return "full and right joins take the per-node route";
  if (jn.coalesce == 2) return "coalesce=false (both key columns kept) takes the per-node route";
  return nullptr;
}
// What every fused join pipeline checks first: the join is not the per-node route's, the caller has no reason of its own against it (`own`, or null), it has one key pair and
// is of a kind the pipeline runs (semi_anti: semi / anti; else inner / left), and both keys are plain columns.  The reason, or null and the two keys.
static const char* single_key_join(const Plan& plan, const IRN& jn, bool semi_anti, const char* own, const AE*& lkx, const AE*& rkx) {
  if (const char* per_node = join_takes_per_node_route(jn)) return per_node;
  if (own) return own;
  const bool kind = semi_anti ? jn.how == PLX_JOIN_SEMI || jn.how == PLX_JOIN_ANTI : jn.how == PLX_JOIN_INNER || jn.how == PLX_JOIN_LEFT;
  if (!kind || jn.keys.size() != 1 || jn.keys_right.size() != 1) return semi_anti ? "not a single-key semi or anti join" : "not a single-key inner or left join";
  lkx = plain_column(plan, jn.keys[0]);
  rkx = plain_column(plan, jn.keys_right[0]);
  return lkx && rkx ? nullptr : "join keys are expressions";
}
static int resolve_join_side(const Plan& plan, int node, std::set<std::string> used, std::vector<int>& preds, std::vector<SemiFilter>& semis, std::string* why) {
  auto no = [&](const char* m) { if (why) *why = m; return -1; };
  const int n = peel_filters(plan, node, preds);
  if (plan.ir[n].kind == PLX_IR_SCAN) return n;
  if (plan.ir[n].kind != PLX_IR_JOIN) return no("join inputs are not filtered scans");
  const IRN& j = plan.ir[n];
  if (j.how != PLX_JOIN_INNER || j.keys.size() != 1 || j.keys_right.size() != 1) return no("nested join is not a single-key inner join");
  if (j.coalesce == 2) return no("nested join keeps both key columns (coalesce=false)");
  const AE* ka = plain_column(plan, j.keys[0]);
  const AE* kb = plain_column(plan, j.keys_right[0]);
  if (!ka || !kb) return no("nested join keys are expressions");
  std::vector<int> ap, bp;
  const int a = peel_filters(plan, j.input, ap), b = peel_filters(plan, j.input_right, bp);
  if (plan.ir[a].kind != PLX_IR_SCAN || plan.ir[b].kind != PLX_IR_SCAN) return no("nested join inputs are not filtered scans");
  FramePtr A = get_frame(plan.ir[a].frame), B = get_frame(plan.ir[b].frame);
  const int kai = A->find(ka->name), kbi = B->find(kb->name);
  if (kai < 0 || kbi < 0) return no("nested join key column not found");
  if (A->cols[kai]->dtype != B->cols[kbi]->dtype || !dtype_is_int(A->cols[kai]->dtype) || A->cols[kai]->dtype == PLX_U64) return no("nested join key is not a signed / narrow integer column pair of one dtype");
  for (size_t i = 0; i < B->names.size(); i++) if ((int)i != kbi && A->find(B->names[i]) >= 0) return no("nested join sides share a column name (suffix renaming is not modelled)");
  for (int pe : preds) collect_columns(plan, pe, used);        // predicates above the nested join see the joined frame
  bool used_a = false, used_b = false;
  for (auto& nm : A->names) used_a = used_a || used.count(nm);
  for (size_t i = 0; i < B->names.size(); i++) if ((int)i != kbi) used_b = used_b || used.count(B->names[i]);
  if (used.count(kb->name) && kb->name != ka->name) return no("the right key of the nested join is referenced above it (coalesced away)");
  SemiFilter sf;
  int payload = -1;
  if (!used_a) { sf.F = A; sf.fpreds = ap; sf.fkey = kai; sf.pkey = kbi; payload = b; preds.insert(preds.begin(), bp.begin(), bp.end()); }
  else if (!used_b) { sf.F = B; sf.fpreds = bp; sf.fkey = kbi; sf.pkey = kai; payload = a; preds.insert(preds.begin(), ap.begin(), ap.end()); }
  else return no("both sides of the nested join are referenced above it");
  semis.push_back(sf);
  return payload;
}
// key range of a semi filter's key column: exact statistics when the column has data, the declared range of a placeholder
static bool semi_key_range(const SemiFilter& sf, int64_t* mn, int64_t* mx) {
  const ColumnPtr& c = sf.F->cols[sf.fkey];
  if (c->values) return ops::int_range(c, mn, mx);
  if (c->range_state == 1) { *mn = c->range_min; *mx = c->range_max; return true; }
  *mn = 0; *mx = 0;
  return true;
}

// ------------------------------------------------ the stages the fused join pipelines share ----
// fused_join_groupby, fused_join_frame and fused_semi_anti_frame (below) resolve their sides, name the joined columns and build their tables here.  The
// structs that hold a table own its device buffers: the table's raw pointers live exactly as long as the struct.
namespace {

// PLX_JOIN_TRACE=1 (debugging aid): every stage of the hash-table pipeline announced on stderr behind a stream synchronisation -- a stage that hangs is the last one named
static const bool jtrace = getenv("PLX_JOIN_TRACE") && getenv("PLX_JOIN_TRACE")[0] == '1';
#define JTRACE(...) do { if (jtrace) { PLX_HIP(hipStreamSynchronize(stream())); fprintf(stderr, "[plx join] " __VA_ARGS__); fputc('\n', stderr); fflush(stderr); } } while (0)

// The inputs of a join on one plain integer key pair, as written (L, R) and as run (B = build side, P = probe side).
struct JoinSides {
  FramePtr L, R, B, P;
  int lki = -1, rki = -1, bki = -1, pki = -1;      // the key column's index in each frame
  int kdt = 0;                                     // its dtype (the same on both sides)
  bool build_right = false;
  std::vector<int> bpreds, ppreds;                 // the predicates of the build / probe side
};
// false + *why: the pipelines do not take this pair of inputs
static bool resolve_join_sides(JoinSides& s, const FramePtr& L, const FramePtr& R, const AE* lkx, const AE* rkx, bool left_join, const std::vector<int>& lpreds, const std::vector<int>& rpreds,
                               const char** why) {
  s.L = L; s.R = R;
  s.lki = L->find(lkx->name); s.rki = R->find(rkx->name);
  if (s.lki < 0 || s.rki < 0) { *why = "join key column not found"; return false; }
  s.kdt = L->cols[s.lki]->dtype;
  if (s.kdt != R->cols[s.rki]->dtype || !dtype_is_int(s.kdt)) { *why = "join key is not an integer column pair of one dtype"; return false; }
  if (L->height >= 0xffffffffll || R->height >= 0xffffffffll) { *why = "side exceeds u32 row indices"; return false; }
  s.build_right = left_join || L->height > R->height;   // det_hash_prone_order (hash_join/mod.rs:41-50): probe = the longer relation; a left join probes with its left table (single_keys_left.rs)
  s.B = s.build_right ? R : L; s.P = s.build_right ? L : R;
  s.bki = s.build_right ? s.rki : s.lki; s.pki = s.build_right ? s.lki : s.rki;
  s.bpreds = s.build_right ? rpreds : lpreds; s.ppreds = s.build_right ? lpreds : rpreds;
  return true;
}

// Columns of the joined frame (_finish_join, general.rs:17-49): left columns, then right columns except the coalesced right key; a right name that clashes gets the suffix.
struct JoinedCol { std::string name; int side; int idx; };     // side 0 = left, 1 = right; idx = the column's index in that side's frame
static bool joined_columns(const Frame& L, const Frame& R, int rki, const std::string& suffix, std::vector<JoinedCol>& outs, const char** why) {
  std::set<std::string> seen;
  for (size_t i = 0; i < L.names.size(); i++) { outs.push_back({L.names[i], 0, (int)i}); seen.insert(L.names[i]); }
  for (size_t i = 0; i < R.names.size(); i++) {
    if ((int)i == rki) continue;
    std::string name = R.names[i];
    if (seen.count(name)) name += suffix;
    if (seen.count(name)) { *why = "duplicate output column name"; return false; }
    seen.insert(name);
    outs.push_back({name, 1, (int)i});
  }
  return true;
}

// Membership bitmap over the key range [kmin, kmin + range): one fused scan of a side sets bit (key - kmin) of every row that passes its predicate and counts those rows
// (BitmapBuildSink); the other side's program tests it with OP_BITLOOKUP.
struct MemberBitmap {
  Buf bits, rows_dev;
  int64_t kmin = 0;
  uint64_t range = 1;
  // Can a bitmap cover the keys [mn, mx] of a side of `height` rows?  At most 2^34 keys and 256 per row (+ 4096).  !have (an empty side, no statistics): one bit that nobody sets.
  bool cover(bool have, int64_t mn, int64_t mx, int64_t height) {
    const unsigned __int128 range128 = have ? (unsigned __int128)((__int128)mx - (__int128)mn) + 1 : 1;
    if (range128 > ((unsigned __int128)1 << 34) || (have && range128 > (unsigned __int128)height * 256 + 4096)) return false;
    kmin = mn; range = (uint64_t)range128;
    return true;
  }
  // the empty bitmap; given the side's program (its key = the key column) also the scan that fills it
  void build(const Compiler* c) {
    bits = dev_alloc_zero(sizeof(uint64_t) * (size_t)(range / 64 + 2)); rows_dev = dev_alloc_zero(8);
    if (!c) return;
    BitmapBuild bb; bb.bits = bits->as<unsigned long long>(); bb.count = rows_dev->as<unsigned long long>(); bb.kmin = kmin; bb.range = range;
    k::fused_bitmap_build(c->shape, c->args, bb, find_static_shape(c->shape));
  }
  uint64_t rows_in() const { uint64_t n = 0; d2h_sync(&n, rows_dev->ptr, 8); return n; }       // (synchronises)
  Lut lut() const { return Lut{bits->as<unsigned long long>(), range}; }
};

// Direct-address table for build keys with a small range (cached column statistics): a bitmap over the key range + a rank per word + the {key, row} pairs the build scan
// appended, by ordinal.  Needs no count pass.  The caller sets dt.opts before try_build and dt.acc after it.
struct DirectBuild {
  enum Result { kNotEligible, kBuilt, kDuplicateKeys };
  Buf bits, rank, okey, orow, used;
  Buf meta;                      // [0] ordinal counter, [2..3] flags, [4..5] pairs appended (u64)
  DirectJoinTable dt{};
  uint64_t range = 0, ord_cap = 0;
  uint64_t nb = 0;               // build rows that passed = slots (unique keys)
  int64_t n_ord = 0;             // ordinals the build scan handed out (live pairs and the unused rest of every wave's last chunk)
  Result try_build(const Plan& plan, const Compiler& cb, const Frame& B, int bki, bool known_dups) {
    int64_t kmn = 0, kmx = 0;
    if ((plan.flags & PLX_PLAN_NO_DIRECT_JOIN) || known_dups || B.height <= 0 || B.cols[bki]->dtype == PLX_U64 || !ops::int_range(B.cols[bki], &kmn, &kmx)) return kNotEligible;
    const unsigned __int128 range128 = (unsigned __int128)((__int128)kmx - (__int128)kmn) + 1;
    // pair list capacity: every build row may pass + one ordinal chunk (1024, kOrdChunk) per wave
    ord_cap = (uint64_t)B.height + (uint64_t)k::scan_waves(B.height) * 1024 + 1024;
    if (range128 > ((unsigned __int128)1 << 34) || range128 > (unsigned __int128)B.height * 256 || ord_cap >= 0xfffffff0ull) return kNotEligible;
    range = (uint64_t)range128;
    const size_t n_blocks = (size_t)(range / 512 + 1), n_words = n_blocks * 8;
    bits = dev_alloc_zero(sizeof(uint64_t) * n_words); rank = dev_alloc(sizeof(uint32_t) * n_words);
    okey = dev_alloc(sizeof(uint64_t) * ord_cap); orow = dev_alloc(sizeof(uint32_t) * ord_cap); used = dev_alloc_zero(sizeof(uint32_t) * (ord_cap / 1024 + 2));
    meta = dev_alloc_zero(32);
    dt.bits = bits->as<unsigned long long>(); dt.rank = rank->as<unsigned int>(); dt.ord_key = okey->as<unsigned long long>(); dt.ord_row = orow->as<unsigned int>();
    dt.chunk_used = used->as<unsigned int>(); dt.counter = meta->as<unsigned int>(); dt.flags = meta->as<unsigned int>() + 2; dt.acc = nullptr; dt.kmin = kmn; dt.range = range; dt.n_ord = (unsigned int)ord_cap;
    k::fused_direct_build(cb.shape, cb.args, dt, find_static_shape(cb.shape));
    // every wave closes its last chunk when it finishes, so chunk_used is final once the build scan is: the rank launch counts
    // the pairs over the whole reserved capacity (the ordinal counter itself is only read back with the rank's sync)
    uint64_t pairs = 0;
    nb = k::direct_rank(dt, rank->as<uint32_t>(), (int64_t)ord_cap, meta->as<uint64_t>() + 2, &pairs);   // synchronises: flags and the ordinal counter are final too
    uint32_t m4[4] = {0, 0, 0, 0};
    d2h_sync(m4, meta->ptr, 16);
    PLX_REQUIRE(!m4[3], PLX_ERR_INVALID, "direct join build: ordinal overflow");
    if (pairs != nb) return kDuplicateKeys;                        // two pairs shared a bit: the hash-table pipeline runs such keys (chains of rows)
    n_ord = (int64_t)std::min<uint64_t>(m4[0], ord_cap);
    return kBuilt;
  }
};

// Hash table of the build side: 16-byte {key, row} slots filled by the build scan `cb` (its predicate fused; k::fused_join_build, or window by window from LDS:
// k::partitioned_join_build), chains of rows per key (`links`) when the build keys repeat.
struct HashBuildOptions {
  int min_log2_cap;          // smallest table (the plan text prints cap=2^N)
  bool start_chained;        // the build keys are known to repeat: chains from the first attempt
  bool chains_allowed;       // false: run() gives up on duplicate build keys
  bool want_cells;           // a windowed build also lists its keys and rows by key number (k::JoinCells)
  const char* plain_how;     // build_how of a build that was not windowed
};
struct HashBuild {
  Buf keys, flags, links;
  JoinAggTable t{};
  k::JoinCells cells;
  int log2_cap = 4;
  uint64_t cap = 0;
  uint64_t nb = 0;           // build rows in the table
  bool multi = false;        // multi-value mode (chains)
  std::string build_how;
  // `cnt` counts the rows `cb` inserts.  false: the build keys repeat and chains are not allowed (the column remembers that its keys repeat: repeats_as_build_key).
  bool run(const Compiler& cnt, const Compiler& cb, const Frame& B, int bki, const HashBuildOptions& o) {
    // Size of the build table.  The number of build rows that pass the build side's predicate is a by-product of the build scan itself (JoinBuildSink counts what
    // it inserts), so a large build side is sized from a strided sample of the count program (4 blocks of 2^18 rows, + 25 %) instead of a counting pass over the
    // whole side; if the sample misjudged (table more than 0.7 full, or a probe sequence overflowed) the table is rebuilt once from the exact count.
    auto exact_count = [&]() -> uint64_t { std::vector<uint64_t> host(kMaxAggs, 0); k::fused_regagg(cnt.shape, cnt.args, find_static_shape(cnt.shape), host.data()); return host[0]; };
    bool sized_by_sample = false;
    if (B.height > 0) {
      static const bool no_sample = getenv("PLX_JOIN_COUNT_SAMPLE") && getenv("PLX_JOIN_COUNT_SAMPLE")[0] == '0';
      if (B.height >= ((int64_t)1 << 24) && !no_sample) {
        constexpr int kCountBlocks = 4;                  // every block is a launch + a host round trip (~40 us)
        const int64_t per = (int64_t)1 << 18, stride = (B.height / kCountBlocks) & ~(int64_t)127;
        uint64_t hits = 0, seen = 0;
        for (int b = 0; b < kCountBlocks; b++) {
          const int64_t row0 = (int64_t)b * stride, rows_b = std::min<int64_t>(per, B.height - row0);
          if (rows_b <= 0) continue;
          std::vector<uint64_t> host(kMaxAggs, 0);
          k::fused_regagg(cnt.shape, offset_args(cnt.shape, cnt.args, row0, rows_b), -1, host.data());
          hits += host[0]; seen += (uint64_t)rows_b;
        }
        nb = (uint64_t)((double)hits / (double)std::max<uint64_t>(seen, 1) * (double)B.height * 1.25) + 4096;
        sized_by_sample = true;
      } else nb = exact_count();
    }
    const ColumnPtr& bkey = B.cols[bki];
    if (o.start_chained) { bkey->repeats_as_build_key = true; if (!o.chains_allowed) return false; multi = true; }
    bool resized = false, pbuild_off = false, built = false;
    std::string retries;       // every attempt that was thrown away, in order: the plan text names them in front of build_how (resized(..)+ windowed-off+ chained+)
    for (int attempt = 0; attempt < 4 && !built; attempt++) {
      if (multi && !links) links = dev_alloc(sizeof(uint64_t) * (size_t)std::max<int64_t>(B.height, 1));
      // (the sampled count already carries 25 %: x1.6 keeps the load at or below ~0.6 without doubling a table that x2 would push over the next power of two)
      log2_cap = std::max(o.min_log2_cap, ceil_log2_u64((uint64_t)((double)std::max<uint64_t>(nb, 1) * (sized_by_sample ? 1.6 : 2.0))));
      cap = 1ull << log2_cap;
      keys = dev_alloc(sizeof(uint64_t) * 2 * (cap + 1)); flags = dev_alloc_zero(32);       // {key, row} slots: kEmptyKey and kNoRow32 are both all-ones
      t.slots = keys->as<unsigned long long>(); t.flags = flags->as<unsigned int>(); t.acc = nullptr;
      t.count = flags->as<unsigned long long>() + 1; t.log2_cap = (uint32_t)log2_cap;
      t.links = multi ? links->as<unsigned long long>() : nullptr;
      t.slow_step_budget = sized_by_sample ? (uint32_t)std::min<uint64_t>(cap, 0x7fffffffu) : 0u;       // (a sampled size has the exact count behind it: give up early)
      JTRACE("build attempt %d multi=%d cap=2^%d nb=%llu", attempt, (int)multi, log2_cap, (unsigned long long)nb);
      // a large build side with (so far) unique keys: partitioned, the table filled window by window from LDS -- no device atomic per row (k::partitioned_join_build)
      t.log2_window = 0;
      build_how = retries + o.plain_how;
      bool pbuilt = false;
      if (!multi && !pbuild_off && partitioned_build_wanted(B.height, log2_cap)) {
        t.log2_window = kJoinWindowLog2;
        std::string bd;
        pbuilt = k::partitioned_join_build(cb.shape, cb.args, find_static_shape(cb.shape), t, o.want_cells ? &cells : nullptr, &bd);
        if (pbuilt) build_how = retries + bd; else t.log2_window = 0;
      }
      if (!pbuilt) {
        PLX_HIP(hipMemsetAsync(keys->ptr, 0xff, sizeof(uint64_t) * 2 * (cap + 1), stream()));
        k::fused_join_build(cb.shape, cb.args, t, find_static_shape(cb.shape));
      }
      JTRACE("build done");
      uint64_t fl64[2] = {0, 0};
      d2h_sync(fl64, flags->ptr, 16);
      const uint32_t dup = (uint32_t)fl64[0], ovf = (uint32_t)(fl64[0] >> 32);
      // A sample that misjudged and duplicate keys can both show in one attempt (a build that overflowed may or may not have met two rows of a key first): both are
      // acted on at once, and the markers are written in this fixed order, so the plan text does not depend on which of the two the attempt happened to notice.
      bool again = false;
      // the sample misjudged (on whichever attempt: the multi-value rebuild keeps the sampled size): once more, from the exact count.  Only a sampled size can be wrong:
      // a table sized from an exact count is at most half full, and an overflow there is a crowded window (below) or an error.
      if (!resized && sized_by_sample && (ovf || fl64[1] * 10 > cap * 7)) {
        retries += std::string("resized(") + (ovf ? "overflow" : "load") + ",from=2^" + std::to_string(log2_cap) + ")+";
        nb = ovf ? exact_count() : fl64[1];
        sized_by_sample = false; resized = true; again = true;
      }
      if (dup) {                                       // (raised by a build without links only: JoinBuildSink, join_fill_kernel)
        bkey->repeats_as_build_key = true;
        if (!o.chains_allowed) return false;
        multi = true;                                  // build once more, chaining the rows of a key (the table's size stays unless it was misjudged: it was planned for the rows, not the keys)
        retries += "chained+"; again = true;
      }
      if (again) continue;
      if (ovf && pbuilt) { pbuild_off = true; retries += "windowed-off+"; continue; }   // a window filled up although the table is sized right (keys that crowd one window): the plain build probes the whole table
      PLX_REQUIRE(!ovf, PLX_ERR_OOM, "join build: probe sequence overflow");
      nb = fl64[1];                                                                   // exact from here on
      built = true;
    }
    PLX_REQUIRE(built, PLX_ERR_OOM, "join build: no finished table after four attempts (" + retries + ")");
    return true;
  }
};

// Which probes are partitioned first (PLX_PROBE_PARTITIONED: 0 = none, 2 = all).  Direct-address table: worth it when the bitmap is far larger than an L2 (4 MB), few
// rows can match and the probe keys come in no order (sampled once per column).
static bool partition_direct_probe(int pmode, const Frame& P, int pki, uint64_t range, uint64_t nb) {
  if (!(pmode == 2 || (pmode == 1 && P.height >= ((int64_t)1 << 24) && range >= ((uint64_t)1 << 28) && nb * 8 <= range))) return false;
  const ColumnPtr& pk = P.cols[pki];
  if (pk->order_state == 0) pk->order_state = k::sample_sortedness(pk) >= 0.9 ? 1 : 2;
  return pmode == 2 || pk->order_state == 2;
}
// Hash table: a table beyond the caches (64 MB) probed by a much longer relation.
static bool partition_hash_probe(int pmode, const Frame& P, uint64_t cap, uint64_t nb) {
  return pmode == 2 || (pmode == 1 && P.height >= ((int64_t)1 << 24) && (cap + 1) * 16 > ((uint64_t)64 << 20) && nb * 16 <= (uint64_t)P.height);
}
// Runs the probe program `cp` over the candidate rows `hits` only: its input columns gathered at them, `launch(args)` is the probe kernel.  Returns the gathered columns:
// they live until the caller has synchronised the stream.
template <class Launch> static std::vector<ColumnPtr> probe_gathered(const Compiler& cp, const ColumnPtr& hits, Launch&& launch) {
  Args a2 = cp.args;
  a2.n_rows = hits->len;
  std::vector<ColumnPtr> srcs;
  for (int i = 0; i < cp.shape.n_inputs; i++) srcs.push_back(cp.cols[cp.input_cols[i]]);
  std::vector<ColumnPtr> keep = ops::gather_columns(srcs, hits);
  for (int i = 0; i < cp.shape.n_inputs; i++) { a2.in[i].values = keep[i]->data(); a2.in[i].validity = cp.shape.in_nullable[i] ? keep[i]->valid_words() : nullptr; }
  launch(a2);
  return keep;
}
}  // namespace

// ------------------------------------------------ fused Join -> GroupBy pipeline ----
// GroupBy(keys incl. the join key, aggregates over the probe side) over Join(inner | left; one plain integer key pair) over two `[Filter]* Scan` inputs, each possibly
// behind a nested filter join (SemiFilter): a group is a build row, the probe scan adds into its cells.  plan_join_groupby decides everything, then one function per stage.
struct GroupKey { bool is_join_key; int build_col; int expr; int dtype; };
// One nested filter join: the side it restricts (0 = build, 1 = probe), its index among that side's filters, its lookup bitmap's number in that side's programs (build
// side: index; probe side: behind the build side's), and the scan of its filter side
struct SemiUse { const SemiFilter* sf; int side; int index; int lut; std::unique_ptr<Compiler> scan; };
// Everything decided before anything runs.  Stays where it is: cp.df, cs.df and ca.df point at pview, the uses at the filters.
struct JoinGroupBy {
  JoinGroupBy& operator=(JoinGroupBy&&) = delete;       // (neither copied nor moved)
  bool left_join = false;
  JoinSides sides;
  std::vector<SemiFilter> bsemis, psemis;
  std::vector<SemiUse> semis;                           // the build side's, then the probe side's
  std::vector<GroupKey> gkeys;
  Frame pview;                                          // the probe side under the joined frame's names: what the aggregates read
  std::optional<Compiler> cnt, cb, cp, cs, ca;          // count, build, probe, the partitioned probe's scatter; ca: the left join's unmatched rows (group-by over the probe side)
  std::vector<int> agg_nodes;
  std::vector<FinalSpec> specs, aspecs;
  KeyPlan akp;
  int len_idx = -1, a_len_idx = -1;
  bool device_pivot = false;                            // the programs are about to run: a var / std source gets its pivot from the device (Compiler::var_pivot)
  MemberBitmap unmatched_keys;                          // left join: the build keys that pass the build side's predicate
};

// the programs of `j` (throws Unsupported)
static void compile_join_programs(const Plan& plan, const IRN& gb, JoinGroupBy& j) {
  const JoinSides& s = j.sides;
  const int nbs = (int)j.bsemis.size(), nps = (int)j.psemis.size();
  // conjunction of the side's predicates and of the membership tests of its semi filters (lookup bitmap i = args.lut[lut0 + i])
  auto and_preds = [&](Compiler& c, const std::vector<int>& preds, const std::vector<SemiFilter>& semis, int lut0) {
    int p = and_predicates(c, preds);
    for (size_t i = 0; i < semis.size(); i++) {
      int64_t mn = 0, mx = 0;
      if (!semi_key_range(semis[i], &mn, &mx)) mn = mx = 0;      // empty filter side: the bitmap is empty, nothing matches
      // (rows the cheaper conjuncts already rejected do not look the bitmap up: OP_MASKV; the conjunction is the same either way)
      const int kn = c.load(semis[i].pkey);
      const int n = c.bit_lookup(p < 0 ? kn : c.mask_valid(kn, p), lut0 + (int)i, mn);
      p = p < 0 ? n : c.mk(OP_AND, p, n, 'b');
    }
    return p;
  };
  Compiler &cnt = j.cnt.emplace(plan, *s.B), &cb = j.cb.emplace(plan, *s.B), &cp = j.cp.emplace(plan, *s.P), &cs = j.cs.emplace(plan, *s.P), &ca = j.ca.emplace(plan, *s.P);
  cnt.lut_base = cb.lut_base = nbs;
  cp.lut_base = cs.lut_base = nbs + nps;
  ca.lut_base = nps + 1;
  cnt.pred = and_preds(cnt, s.bpreds, j.bsemis, 0);
  const int bk_cnt = cnt.load(s.bki);
  cnt.add_agg(cnt.nodes[bk_cnt].nullable ? AGG_COUNT : AGG_LEN, cnt.nodes[bk_cnt].nullable ? bk_cnt : -1);
  cnt.finish();
  cb.pred = and_preds(cb, s.bpreds, j.bsemis, 0);
  cb.key = cb.load(s.bki);
  cb.finish();
  cp.pred = and_preds(cp, s.ppreds, j.psemis, nbs);
  cp.key = cp.load(s.pki);
  cp.df = &j.pview;
  cp.device_pivot = ca.device_pivot = j.device_pivot;
  j.len_idx = cp.add_agg(AGG_LEN, -1);
  for (int e : gb.exprs) collect_aggs(plan, e, j.agg_nodes);
  cp.decline_order_statistics(j.agg_nodes);
  for (int a : j.agg_nodes) j.specs.push_back(cp.lower_agg(a));
  cp.finish();
  // the probe side's predicate + key alone, row id as payload: the program of the partitioned probe's scatter (k::partitioned_probe_hits)
  cs.pred = and_preds(cs, s.ppreds, j.psemis, nbs);
  cs.key = cs.load(s.pki);
  cs.df = &j.pview;
  cs.add_agg(AGG_FIRST_ROW, -1);
  cs.finish();
  if (j.left_join) {
    int p = and_preds(ca, s.ppreds, j.psemis, 0);                                  // (its own lookup numbering: the probe side's semi filters, then the membership bitmap)
    const int kn = ca.load(s.pki);
    ca.df = &j.pview;                                                              // (after the loads by column index, which are the probe frame's: pview orders its columns by name)
    const int member = ca.ifnull(ca.bit_lookup(p < 0 ? kn : ca.mask_valid(kn, p), nps, j.unmatched_keys.kmin), 0);      // a null key is among nobody's keys
    const int unmatched = ca.mk(OP_NOT, member, member, 'b');
    ca.pred = p < 0 ? unmatched : ca.mk(OP_AND, p, unmatched, 'b');
    int jk_expr = -1;
    for (auto& gk : j.gkeys) if (gk.is_join_key) jk_expr = gk.expr;
    j.akp = lower_keys(ca, std::vector<int>{jk_expr});
    j.a_len_idx = ca.add_agg(AGG_LEN, -1);
    ca.seed_pivots = cp.pivot_by_expr;      // the same sources over the same probe rows
    for (int a : j.agg_nodes) j.aspecs.push_back(ca.lower_agg(a));
    ca.finish();
  }
  // one program per semi filter: build-side filters first, then probe-side
  for (int side = 0; side < 2; side++) {
    const std::vector<SemiFilter>& sv = side == 0 ? j.bsemis : j.psemis;
    for (size_t i = 0; i < sv.size(); i++) {
      j.semis.push_back(SemiUse{&sv[i], side, (int)i, side == 0 ? (int)i : nbs + (int)i, std::make_unique<Compiler>(plan, *sv[i].F)});
      Compiler& cf = *j.semis.back().scan;
      cf.pred = and_preds(cf, sv[i].fpreds, {}, 0);
      cf.key = cf.load(sv[i].fkey);
      cf.finish();
    }
  }
}

// The checks, the two sides, the group keys and the programs.  false + why: the pipeline does not take this plan (nothing has run)
static bool plan_join_groupby(const Plan& plan, const IRN& gb, JoinGroupBy& j, std::string* why) {
  auto no = [&](const char* m) { if (why) *why = m; return false; };
  if (gb.input < 0 || plan.ir[gb.input].kind != PLX_IR_JOIN) return no("input is not a join");
  const IRN& jn = plan.ir[gb.input];
  const AE *lkx = nullptr, *rkx = nullptr;
  if (const char* bad = single_key_join(plan, jn, false, nullptr, lkx, rkx)) return no(bad);
  // LEFT join (single_keys_left.rs:106-195: every left row survives; rows without a match carry nulls in the right table's columns): the matched rows are the inner join's
  // -- the same pipeline with the RIGHT table as the build side -- and the unmatched ones are a group-by of their own over the left table, keyed by the join key, behind
  // the predicate "key not among the build keys" (a membership bitmap over the build key range, tested inside the scan: OP_BITLOOKUP); their groups carry nulls in the
  // build-side group columns.  Needs a build key range a bitmap can cover; otherwise the per-node path runs the join.
  j.left_join = jn.how == PLX_JOIN_LEFT;
  if (gb.maintain_order) return no("maintain_order");
  std::vector<int> lpreds, rpreds;
  std::vector<SemiFilter> lsemis, rsemis;
  std::set<std::string> used;                       // column names referenced above the join inputs
  for (int e : gb.keys) collect_columns(plan, e, used);
  for (int e : gb.exprs) collect_columns(plan, e, used);
  used.insert(lkx->name); used.insert(rkx->name);
  const int lsrc = resolve_join_side(plan, jn.input, used, lpreds, lsemis, why);
  if (lsrc < 0) return false;
  const int rsrc = resolve_join_side(plan, jn.input_right, used, rpreds, rsemis, why);
  if (rsrc < 0) return false;
  if (lsemis.size() + rsemis.size() > (size_t)kMaxLuts) return no("more nested filter joins than lookup bitmaps");
  JoinSides& s = j.sides;
  const char* bad = nullptr;
  if (!resolve_join_sides(s, get_frame(plan.ir[lsrc].frame), get_frame(plan.ir[rsrc].frame), lkx, rkx, j.left_join, lpreds, rpreds, &bad)) return no(bad);
  const FramePtr &B = s.B, &P = s.P;
  j.bsemis = s.build_right ? rsemis : lsemis;
  j.psemis = s.build_right ? lsemis : rsemis;
  std::vector<JoinedCol> jcols;
  if (!joined_columns(*s.L, *s.R, s.rki, jn.suffix, jcols, &bad)) return no(bad);
  std::map<std::string, const JoinedCol*> joined;      // by name
  for (const JoinedCol& jc : jcols) joined[jc.name] = &jc;
  const int build_side = s.build_right ? 1 : 0;
  // group keys
  bool has_join_key = false;
  for (int e : gb.keys) {
    const AE* x = plain_column(plan, e);
    if (!x) return no("group key is an expression");
    auto it = joined.find(x->name);
    if (it == joined.end()) fail(PLX_ERR_NOT_FOUND, "column not found: " + x->name);
    const JoinedCol& sc = *it->second;
    const bool is_key = (sc.side == 0 && sc.idx == s.lki);   // the coalesced key column carries the left name
    if (is_key) { has_join_key = true; j.gkeys.push_back({true, -1, e, s.kdt}); }
    else if (sc.side == build_side) j.gkeys.push_back({false, sc.idx, e, B->cols[sc.idx]->dtype});
    else return no("group key from the probe side that is not the join key");
  }
  if (!has_join_key) return no("group keys do not include the join key");
  // aggregates: probe-side columns only, resolved through the joined names
  Frame& pview = j.pview;
  pview.height = P->height;
  for (auto& kv : joined) if (kv.second->side != build_side) { pview.names.push_back(kv.first); pview.cols.push_back(P->cols[kv.second->idx]); }
  if (!s.build_right) { pview.names.push_back(lkx->name); pview.cols.push_back(P->cols[s.pki]); }  // coalesced key: probe values == build values on matches
  std::function<bool(int)> probe_only = [&](int e) -> bool {
    if (e < 0) return true;
    const AE& x = plan.ae[e];
    if (x.kind == PLX_AE_COLUMN) return pview.find(x.name) >= 0;
    return probe_only(x.lhs) && probe_only(x.rhs) && probe_only(x.cond);
  };
  for (int e : gb.exprs) {
    if (!contains_agg(plan, e) || contains_column_outside_agg(plan, e)) return no("aggregation list contains a non-aggregated column");
    if (!probe_only(e)) return no("aggregate reads a build-side column");
  }
  if (j.left_join) {
    if (j.psemis.size() + 1 > (size_t)kMaxLuts) return no("left join: no lookup bitmap left for the membership test");
    if (s.kdt == PLX_U64) return no("left join on UInt64 keys");
    int64_t a_kmn = 0, a_kmx = 0;
    bool have = false;                                          // (a placeholder column -- compile-only callers -- has its declared range or none)
    if (B->height > 0 && B->cols[s.bki]->values) have = ops::int_range(B->cols[s.bki], &a_kmn, &a_kmx);
    else if (B->height > 0 && B->cols[s.bki]->range_state == 1) { a_kmn = B->cols[s.bki]->range_min; a_kmx = B->cols[s.bki]->range_max; have = true; }
    if (!j.unmatched_keys.cover(have, a_kmn, a_kmx, B->height)) return no("left join: build key range too wide for the membership bitmap");
  }
  try { compile_join_programs(plan, gb, j); } catch (const Unsupported& u) { if (why) *why = u.why; return false; }
  return true;
}

// the three scans + how groups, group keys and outputs are derived from them (tests/program_eval.py evaluate_join)
static std::string dump_join_groupby(const Plan& plan, const IRN& gb, const JoinGroupBy& j) {
  const Frame &B = *j.sides.B, &P = *j.sides.P;
  std::ostringstream o;
  o << "{\"kind\":\"join_group_by\",\"how\":\"" << (j.left_join ? "left" : "inner") << "\",\"build_side\":\"" << (j.sides.build_right ? "right" : "left") << "\",\"build_key\":" << jstr(B.names[j.sides.bki]) << ",\"probe_key\":" << jstr(P.names[j.sides.pki])
    << ",\"count\":{" << program_fields(*j.cnt, B) << "},\"build\":{" << program_fields(*j.cb, B) << "},\"probe\":{" << program_fields(*j.cp, P) << "},\"len_idx\":" << j.len_idx << ",\"group_keys\":[";
  for (size_t i = 0; i < j.gkeys.size(); i++)
    o << (i ? "," : "") << "{\"name\":" << jstr(output_name(plan, j.gkeys[i].expr)) << ",\"is_join_key\":" << (j.gkeys[i].is_join_key ? 1 : 0) << ",\"build_col\":"
      << (j.gkeys[i].is_join_key ? std::string("null") : jstr(B.names[j.gkeys[i].build_col])) << ",\"dtype\":" << j.gkeys[i].dtype << "}";
  o << "]," << finals_outputs_fields(plan, j.agg_nodes, j.specs, gb.exprs) << ",\"semis\":[";
  for (const SemiUse& u : j.semis) {
    int64_t mn = 0, mx = 0; semi_key_range(*u.sf, &mn, &mx);
    o << (&u != &j.semis[0] ? "," : "") << "{\"side\":\"" << (u.side == 0 ? "build" : "probe") << "\",\"lut\":" << u.lut << ",\"kmin\":\"" << mn << "\",\"kmax\":\"" << mx
      << "\",\"filter_key\":" << jstr(u.sf->F->names[u.sf->fkey]) << ",\"payload_key\":" << jstr((u.side == 0 ? B : P).names[u.sf->pkey]) << ",\"filter\":{" << program_fields(*u.scan, *u.sf->F) << "}}";
  }
  o << "]";
  // a left join's unmatched rows: a group-by program over the probe side whose predicate ends in NOT member(key) -- lookup bitmap `lut` = the build keys that pass the build program
  if (j.left_join) o << ",\"unmatched\":{\"lut\":" << j.psemis.size() << ",\"kmin\":\"" << j.unmatched_keys.kmin << "\",\"range\":\"" << j.unmatched_keys.range << "\",\"program\":"
                     << compiled_json("group_by", plan, *j.ca, ScanProgram{j.ca->shape, j.ca->args, -1, ""}, &j.akp, j.agg_nodes, j.aspecs, gb.exprs, j.a_len_idx, -1, false) << "}";
  o << "}";
  return o.str();
}

// The semi filters: one fused scan of each filter side -> membership bitmap, handed to the programs of the side it restricts.  Its set bits must equal the rows that passed
// (unique filter keys), otherwise the nested join multiplies rows and the per-node path has to run it (false + why)
static bool build_semi_bitmaps(Plan& plan, JoinGroupBy& j, std::vector<MemberBitmap>& semi_bits, std::string* why) {
  auto no = [&](const char* m) { if (why) *why = m; return false; };
  for (size_t ci = 0; ci < j.semis.size(); ci++) {
    const SemiUse& u = j.semis[ci];
    const SemiFilter& sf = *u.sf;
    int64_t mn = 0, mx = 0;
    const bool have = sf.F->height > 0 && semi_key_range(sf, &mn, &mx);
    MemberBitmap& mb = semi_bits[ci];
    if (!mb.cover(have, mn, mx, sf.F->height)) return no("nested filter join: key range too wide for a bitmap");
    mb.build(have ? u.scan.get() : nullptr);
    if (have) {
      const uint64_t rows_in = mb.rows_in();
      if ((uint64_t)k::bitmap_popcount(mb.bits->as<uint64_t>(), (int64_t)mb.range) != rows_in) return no("nested filter join: the filter side's keys are not unique");
      plan.desc += "SemiFilter{" + sf.F->names[sf.fkey] + " -> bitmap range=" + std::to_string(mb.range) + " rows=" + std::to_string(rows_in) + "/" + std::to_string(sf.F->height) + "}; ";
    }
    const Lut lut = mb.lut();
    if (u.side == 0) { j.cnt->args.lut[u.lut] = lut; j.cb->args.lut[u.lut] = lut; }
    else { j.cp->args.lut[u.lut] = lut; j.cs->args.lut[u.lut] = lut; if (j.left_join) j.ca->args.lut[u.index] = lut; }      // (the left tail numbers the probe side's filters from 0)
  }
  return true;
}

// What a route leaves: the groups' cells and packed keys, compacted, the build row of every group, and whether a group is a build ROW (multi-value mode) rather than a key
struct JoinGroups {
  FusedAggResult r;
  ColumnPtr rows = std::make_shared<Column>();
  bool multi = false;
};

// The partitioned probe of either table: `hits_of(&rows, &how)` scatters the probe side by key and lists the rows that can match (false: it does not take this table, nothing
// was probed), `probe(args)` is the ordinary probe kernel, run over those rows only (gathered).  `gathered(columns, n)`: what else the route does with them before they go.
template <class Hits, class Probe, class Gathered>
static bool probe_through_partitions(const Compiler& cp, Hits&& hits_of, Probe&& probe, Gathered&& gathered, std::string& how) {
  ColumnPtr hits;
  std::string pd;
  if (!hits_of(&hits, &pd)) return false;
  if (hits->len > 0) {
    std::vector<ColumnPtr> keep = probe_gathered(cp, hits, probe);
    gathered(keep, hits->len);
    PLX_HIP(hipStreamSynchronize(stream()));       // the gathered columns live until the kernels have read them
  }
  how = pd + "+gather+probe_agg";
  return true;
}

// Direct-address table when the build key range is small (cached column statistics); needs no count pass.  false: not taken -- the range is too wide, or the build keys
// repeat (known_dups is then set: the hash-table route runs them in multi-value mode)
static bool direct_table_route(Plan& plan, const JoinGroupBy& j, bool& known_dups, JoinGroups& g) {
  const Frame &B = *j.sides.B, &P = *j.sides.P;
  const Compiler &cp = *j.cp, &cs = *j.cs;
  DirectBuild direct;
  direct.dt.opts = probe_late_loads() ? kDirectLateLoads : 0u;
  const DirectBuild::Result built = direct.try_build(plan, *j.cb, B, j.sides.bki, known_dups);
  if (built == DirectBuild::kDuplicateKeys) known_dups = true;
  if (built != DirectBuild::kBuilt) return false;
  DirectJoinTable& dt = direct.dt;
  const uint64_t range = direct.range, nb = direct.nb;
  const int probe_static_id = find_static_shape(cp.shape);
  FusedAggResult& r = g.r;
  const int64_t n_slots = (int64_t)nb, s1 = std::max<int64_t>(n_slots, 1);
  Buf acc2 = dev_alloc(sizeof(uint64_t) * (size_t)s1 * cp.shape.n_aggs);
  k::init_agg_cells(acc2->as<uint64_t>(), s1, cp.shape);   // LEN = 0: build rows no probe row matched never show up
  dt.acc = acc2->as<unsigned long long>();
  // Probe.  Keys in (rough) key order walk the bitmap out of the L2; keys in no order fetch one line per row across the fabric: those
  // are partitioned by key range first and probed against LDS-resident bitmap slices, and the ordinary probe kernel then runs over
  // the matching rows only (gathered).  Worth it when the bitmap is far larger than an L2 (4 MB) and few rows can match.
  std::string probe_how = "probe_agg";
  Buf touch;
  // the pair-list compaction below looks every build pair up in bitmap, rank and LEN cells -- random lines for a shuffled build side.  Only keys
  // among the candidates can have been matched: a 2^26-bit filter of their hashes (8 MB: cache-resident) lets the compaction skip the rest
  auto touch_filter = [&](const std::vector<ColumnPtr>& keep, int64_t n_hits) {
    const int key_in = slot_input(cp.shape, cp.shape.key);
    if (key_in < 0 || (size_t)key_in >= keep.size()) return;
    constexpr unsigned int kLog2TouchBits = 26;
    touch = dev_alloc_zero(sizeof(uint64_t) * ((size_t)1 << (kLog2TouchBits - 6)));
    ColumnPtr k64 = keep[key_in]->dtype == PLX_I64 ? keep[key_in] : ops::cast(keep[key_in], PLX_I64);
    k::touch_filter_set(k64->values->as<int64_t>(), k64->valid_words(), n_hits, kLog2TouchBits, touch->as<uint64_t>());
    dt.touch_filter = touch->as<unsigned long long>(); dt.log2_touch_bits = kLog2TouchBits;
  };
  if (!(partition_direct_probe(partitioned_probe_mode(), P, j.sides.pki, range, nb) &&
        probe_through_partitions(cp, [&](ColumnPtr* hits, std::string* pd) { return k::partitioned_probe_hits(cs.shape, cs.args, dt, nb, find_static_shape(cs.shape), hits, pd); },
                                 [&](const Args& a2) { k::fused_direct_probe_agg(cp.shape, a2, dt, probe_static_id); }, touch_filter, probe_how)))
    k::fused_direct_probe_agg(cp.shape, cp.args, dt, probe_static_id);
  // one pass over the pair list into buffers sized for every slot (G <= n_slots)
  r.packed_keys = dev_alloc(sizeof(uint64_t) * (size_t)s1);
  r.acc = dev_alloc(sizeof(uint64_t) * (size_t)s1 * r.n_aggs);
  g.rows->values = dev_alloc(values_bytes(PLX_U32, s1));
  r.n_groups = n_slots ? k::direct_agg_compact(dt, direct.n_ord, r.n_aggs, j.len_idx, r.packed_keys->as<uint64_t>(), g.rows->values->as<uint32_t>(), r.acc->as<uint64_t>()) : 0;
  g.rows->len = r.n_groups;
  plan.desc += std::string("FusedJoinGroupBy{build=") + (j.sides.build_right ? "right" : "left") + " rows=" + std::to_string(nb) + "/" + std::to_string(B.height) + " direct-address table range=" +
               std::to_string(range) + " (bitmap + rank) unique-keys, probe rows=" + std::to_string(P.height) + ", fused_scan[" + jit::program_mode(probe_static_id, cp.args.n_rows) + "]+" + probe_how + ", aggs=" +
               std::to_string(r.n_aggs) + ", groups=" + std::to_string(r.n_groups) + "}; ";
  return true;
}

// Duplicate build keys (the reference's tables map a key to a LIST of build rows: single_keys.rs:16-167, probe_inner emits one pair per entry, single_keys_inner.rs:11-38):
// the hash-table pipeline then runs in multi-value mode -- chains of build rows per key, a group = a build ROW (or the rows of a key that agree on the build-side group
// columns: canonicalise_chains), every probe row adds to the cells of each row of its key's chain.  Possible when those group columns are integer-typed (compared bitwise):
// `rep` lists them; false: one of them is not, or PLX_JOIN_MULTI=0.
static bool chain_group_columns(const JoinGroupBy& j, RepCols& rep) {
  bool multi_ok = !(getenv("PLX_JOIN_MULTI") && getenv("PLX_JOIN_MULTI")[0] == '0');
  for (auto& gk : j.gkeys) {
    if (gk.is_join_key) continue;
    const ColumnPtr& col = j.sides.B->cols[gk.build_col];
    const int w = col->dtype == PLX_BOOL || col->dtype == PLX_F32 || col->dtype == PLX_F64 ? 0 : dtype_width(col->dtype);
    if (!w || rep.n >= kMaxRepCols) { multi_ok = false; break; }
    rep.vals[rep.n] = col->data(); rep.valid[rep.n] = (const unsigned long long*)col->valid_words(); rep.width[rep.n] = w; rep.n++;
  }
  return multi_ok;
}

// Hash table of the build side, unique keys or (known_dups, or found by the build) chains of rows.  false + why: the build keys repeat in a way the chains do not take
static bool hash_table_route(Plan& plan, const JoinGroupBy& j, bool known_dups, bool multi_ok, const RepCols& rep_cols, JoinGroups& g, std::string* why) {
  auto no = [&](const char* m) { if (why) *why = m; return false; };
  const Frame &B = *j.sides.B, &P = *j.sides.P;
  const Compiler &cp = *j.cp, &cs = *j.cs;
  HashBuild hb;
  if (!hb.run(*j.cnt, *j.cb, B, j.sides.bki, HashBuildOptions{4, known_dups, multi_ok, true, "join_build"})) return no("build keys are not unique (and a build-side group column is not integer-typed)");
  JoinAggTable& t = hb.t;
  const uint64_t nb = hb.nb;
  const bool multi = g.multi = hb.multi;
  uint32_t merged_rows = 0;      // multi-value mode: build rows that share their group with an earlier row of their key
  if (multi) {
    Buf cflags = dev_alloc_zero(8);
    constexpr unsigned int kMaxChain = 1024;
    JTRACE("canonicalise: %d columns", rep_cols.n);
    k::canonicalise_chains(t, rep_cols, kMaxChain, cflags->as<unsigned int>());
    JTRACE("canonicalise done");
    uint32_t cfl[2] = {0, 0};
    d2h_sync(cfl, cflags->ptr, 8);
    if (cfl[0]) return no("a build key repeats more than 1024 times");
    merged_rows = cfl[1];
  }
  // one cell set per KEY, also in multi-value mode (the groups are expanded from the key's cells by chains_agg_compact): a slot's cells, or -- a windowed table numbers
  // its keys -- the key's
  const int probe_static_id = find_static_shape(cp.shape);
  FusedAggResult& r = g.r;
  const int64_t n_cells = t.log2_window ? (int64_t)nb + 1 : (int64_t)hb.cap + 1;
  Buf acc = dev_alloc(sizeof(uint64_t) * (size_t)n_cells * cp.shape.n_aggs);
  t.acc = acc->as<unsigned long long>();
  k::init_agg_cells(acc->as<uint64_t>(), n_cells, cp.shape);
  // Probe.  A table beyond the caches (64 MB) probed by a much longer relation: every probe row would fetch a line across the fabric (SF100 Q3 on keys without
  // a dense range: 3.2e8 random probes of a 400 MB table).  The probe side is partitioned by the key's HASH instead and each partition is tested against an
  // LDS Bloom filter of the table's keys in it (k::partitioned_hash_probe_hits: the radix-partitioned probe of single_keys_inner.rs:11-149 with the partition's
  // filter in LDS); the hash probe below then runs over the surviving candidates only and compares whole keys.
  std::string probe_how = "probe_agg";
  const bool partitioned = partition_hash_probe(partitioned_probe_mode(), P, hb.cap, nb) &&
      probe_through_partitions(cp, [&](ColumnPtr* hits, std::string* pd) { return k::partitioned_hash_probe_hits(cs.shape, cs.args, t, nb, find_static_shape(cs.shape), hits, pd); },
                               [&](const Args& a2) { k::fused_probe_agg(cp.shape, a2, t, probe_static_id); }, [](const std::vector<ColumnPtr>&, int64_t) {}, probe_how);
  JTRACE("probe (partitioned: %d)", (int)partitioned);
  if (!partitioned) k::fused_probe_agg(cp.shape, cp.args, t, probe_static_id);
  JTRACE("probe done");
  // ONE compaction pass into buffers sized for every build row (G <= nb): no counting pass over the table first
  const int64_t g1 = std::max<int64_t>((int64_t)nb, 1);
  if (!multi) {
    r.packed_keys = dev_alloc(sizeof(uint64_t) * (size_t)g1);
    r.acc = dev_alloc(sizeof(uint64_t) * (size_t)g1 * r.n_aggs);
    g.rows->values = dev_alloc(values_bytes(PLX_U32, g1));
  }
  // (measured on SF100 Q3 with hashed keys: listing the touched slots from the candidates' probe -- one returning atomic per row -- costs that probe 0.5 ms, a
  // candidates' filter in front of the LEN cells 0.2 ms; streaming the LEN cells is 0.37 ms)
  int64_t G;
  if (multi) G = k::chains_agg_compact(t, cp.shape, acc->as<uint64_t>(), j.len_idx, &g.rows->values, &r.acc);
  else if (t.log2_window) G = k::cells_agg_compact(hb.cells, acc->as<uint64_t>(), n_cells, r.n_aggs, j.len_idx, r.packed_keys->as<uint64_t>(), g.rows->values->as<uint32_t>(), r.acc->as<uint64_t>());
  else G = k::join_agg_compact(t, r.n_aggs, j.len_idx, r.packed_keys->as<uint64_t>(), g.rows->values->as<uint32_t>(), r.acc->as<uint64_t>());
  JTRACE("compacted: %lld groups", (long long)G);
  PLX_REQUIRE(multi || G <= g1, PLX_ERR_INVALID, "join: more groups than build rows");
  r.n_groups = g.rows->len = G;
  plan.desc += std::string("FusedJoinGroupBy{build=") + (j.sides.build_right ? "right" : "left") + " rows=" + std::to_string(nb) + "/" + std::to_string(B.height) + " hash table cap=2^" + std::to_string(hb.log2_cap) + " [" + hb.build_how + "]" +
               (multi ? " multi-value (row chains, a group = a build row; " + std::to_string(merged_rows) + " rows share another row's group), probe rows=" : " unique-keys, probe rows=") + std::to_string(P.height) + ", fused_scan[" + jit::program_mode(probe_static_id, cp.args.n_rows) + "]+" + probe_how + ", aggs=" + std::to_string(r.n_aggs) + ", groups=" + std::to_string(G) + "}; ";
  return true;
}

// the matched groups' frame: keys, then aggregates
static FramePtr matched_groups_frame(const Plan& plan, const IRN& gb, const JoinGroupBy& j, const JoinGroups& g) {
  const Frame& B = *j.sides.B;
  auto out = std::make_shared<Frame>();
  out->height = g.r.n_groups;
  FinBatch batch{};
  for (auto& gk : j.gkeys) {
    out->names.push_back(output_name(plan, gk.expr));
    if (gk.is_join_key && g.multi) out->cols.push_back(ops::gather(B.cols[j.sides.bki], g.rows));      // (inner join: the build row's key IS the group's key)
    else if (gk.is_join_key) {
      KeyPart part; part.expr = gk.expr; part.dtype = gk.dtype;
      part.dec.shift = 0; part.dec.mask = ~0ull; part.dec.min = 0; part.dec.null_code = ~0ull; part.dec.dtype = gk.dtype;
      out->cols.push_back(decode_key_column(g.r, part, 0, batch));
    } else out->cols.push_back(ops::gather(B.cols[gk.build_col], g.rows));
  }
  append_aggregate_columns(plan, g.r, j.agg_nodes, j.specs, gb.exprs, batch, *out);
  return out;
}

// A left join's unmatched left rows, appended to `out`: membership bitmap of the build keys that pass the build side's predicate, then a fused group-by over the left table
// behind "key not a member"; their groups carry nulls in the build-side group columns.  false: a row outside bounds the planner had only ASSUMED for the probe key / value
// columns (lower_keys(ca) and source_ranges run outside fused_groupby's own handler) -- the guesses are forgotten, never made again, and the caller runs the whole join once more
static bool unmatched_left_groups(Plan& plan, const IRN& gb, JoinGroupBy& j, Frame& out) {
  const Frame& B = *j.sides.B;
  Compiler& ca = *j.ca;
  j.unmatched_keys.build(B.height > 0 ? &*j.cb : nullptr);
  ca.args.lut[j.psemis.size()] = j.unmatched_keys.lut();
  FusedAggResult ar;
  std::string ad;
  try {
    run_fused_groupby(ca, j.akp, j.a_len_idx, ar, ad, plan.encoded);
  } catch (const Error& e) {
    if (!forget_assumed_bounds(ca.cols) || e.code != PLX_ERR_INVALID) throw;
    plan.desc += "AssumedBoundsViolated{exact statistics, second run}; ";
    return false;
  }
  plan.desc += "LeftJoinUnmatched{membership bitmap range=" + std::to_string(j.unmatched_keys.range) + ", " + j.akp.note + "FusedFilterGroupBy{" + ad + ", groups=" + std::to_string(ar.n_groups) + "}}; ";
  const int64_t G = out.height, U = ar.n_groups;
  Frame tail;
  FinBatch batch{};
  for (auto& gk : j.gkeys) {
    tail.names.push_back(output_name(plan, gk.expr));
    if (gk.is_join_key) tail.cols.push_back(decode_key_column(ar, j.akp.parts[0], 0, batch));
    else tail.cols.push_back(ops::full_column(B.cols[gk.build_col]->dtype, plx_scalar{0}, false, U));       // no build row: null
  }
  append_aggregate_columns(plan, ar, j.agg_nodes, j.aspecs, gb.exprs, batch, tail);
  if (U == 0) return true;
  for (size_t i = 0; i < out.cols.size(); i++) {
    ColumnPtr b = tail.cols[i];
    if (b->dtype != out.cols[i]->dtype) b = ops::cast(b, out.cols[i]->dtype);
    out.cols[i] = G > 0 ? ops::concat({out.cols[i], b}) : b;
  }
  out.height = G + U;
  return true;
}

static bool fused_join_groupby(Plan& plan, const IRN& gb, FramePtr& out, std::string* why, std::vector<Shape>* shapes_out = nullptr, bool compile_only = false) {
  JoinGroupBy j;
  j.device_pivot = !compile_only;
  if (!plan_join_groupby(plan, gb, j, why)) return false;
  // count, build, probe, the semi filters' scans, and LAST the probe side's predicate + key program of the partitioned probe's scatter
  if (shapes_out) { shapes_out->push_back(j.cnt->shape); shapes_out->push_back(j.cb->shape); shapes_out->push_back(j.cp->shape); for (auto& u : j.semis) shapes_out->push_back(u.scan->shape); shapes_out->push_back(j.cs->shape); }
  if (compile_only) {
    if (t_program_dump) t_program_dump->json = dump_join_groupby(plan, gb, j);
    return true;
  }
  // ---- run.  The semi bitmaps live until the last scan that tests them (the left tail's); what a table route allocates, until it has compacted its groups
  std::vector<MemberBitmap> semi_bits(j.semis.size());
  if (!build_semi_bitmaps(plan, j, semi_bits, why)) return false;
  bool known_dups = j.sides.B->height > 0 && j.sides.B->cols[j.sides.bki]->repeats_as_build_key;
  RepCols rep_cols{};
  const bool multi_ok = chain_group_columns(j, rep_cols);
  JoinGroups g;
  g.r.n_aggs = j.cp->shape.n_aggs;
  g.rows->dtype = PLX_U32; g.rows->null_count = 0;
  if (!direct_table_route(plan, j, known_dups, g) && !hash_table_route(plan, j, known_dups, multi_ok, rep_cols, g, why)) return false;
  out = matched_groups_frame(plan, gb, j, g);
  if (j.left_join && !unmatched_left_groups(plan, gb, j, *out)) return fused_join_groupby(plan, gb, out, why, shapes_out, compile_only);
  plan.desc += j.cp->var_note;      // (once per source, from the run that produced the result)
  return true;
}

#undef JTRACE

// ----------------------------------------------------------------- executors ----
static FramePtr exec_node(Plan& plan, int node_id);

// [Filter]* over a materialised frame without FilterExec's intermediates (filter.rs:94-145: predicate column -> Boolean mask -> one filter call per column): the
// conjunction of the predicates is compiled into a register program whose scan leaves only 16 bytes of ballots + a count per 128 rows (k::fused_ballots), a device
// scan turns the counts into offsets, and ONE kernel then writes the kept rows of every fixed-width column densely and in order (k::compact_by_ballots); validity
// bitmaps and Boolean columns go through the bitmap compaction of kernels_filter.hip with the same selection.  Traffic: predicate inputs once + payload once + output
// once.  `want_rows`: also the kept row indices; rows_only: nothing else.  false: the predicate does not compile (f32 arithmetic, null literals...) -- per-node path.
// member (may be null): one more conjunct -- the row's key column `key_col` is (anti: is NOT) a member of the bitmap `bits` over [kmin, kmin + range): the probe side of a semi /
// anti join whose other side has become a membership bitmap (fused_semi_anti_frame).  A null key is nobody's member: semi drops it, anti keeps it.
struct MemberTest { int key_col; const unsigned long long* bits; int64_t kmin; uint64_t range; bool anti; };
static bool fused_filter_frame(Plan& plan, const std::vector<int>& preds, const FramePtr& src, FramePtr& out, std::string* why, ColumnPtr* want_rows = nullptr, bool rows_only = false,
                               const MemberTest* member = nullptr) {
  Compiler c(plan, *src);
  try {
    c.lut_base = member ? 1 : 0;
    int p = and_predicates(c, preds);
    if (member) {
      const int kn = c.load(member->key_col);
      int m = c.ifnull(c.bit_lookup(p < 0 ? kn : c.mask_valid(kn, p), 0, member->kmin), 0);      // (rows the predicates already rejected do not look the bitmap up: OP_MASKV)
      if (member->anti) m = c.mk(OP_NOT, m, m, 'b');
      p = p < 0 ? m : c.mk(OP_AND, p, m, 'b');
    }
    if (p < 0) throw Unsupported("no predicate");
    c.pred = p;
    c.finish();
    if (member) c.args.lut[0] = Lut{member->bits, member->range};
  } catch (const Unsupported& u) { if (why) *why = u.why; return false; }
  const int64_t n = src->height;
  out = std::make_shared<Frame>();
  out->names = src->names;
  auto empty_rows = [] { auto e = std::make_shared<Column>(); e->dtype = PLX_U32; e->len = 0; e->null_count = 0; e->values = dev_alloc(8); return e; };
  if (n == 0) { out->cols = src->cols; out->height = 0; if (want_rows) *want_rows = empty_rows(); return true; }
  PLX_REQUIRE(n < 0xffffffffll || !want_rows, PLX_ERR_UNSUPPORTED, "filter: row indices beyond u32 IdxSize");
  const int64_t n_wt = (n + 127) / 128;
  Buf ballots = dev_alloc(sizeof(uint64_t) * 2 * (size_t)n_wt), counts = dev_alloc(sizeof(uint32_t) * (size_t)n_wt);
  BallotOut bo{ballots->as<unsigned long long>(), counts->as<unsigned int>()};
  const int static_id = find_static_shape(c.shape);
  k::fused_ballots(c.shape, c.args, bo, static_id);
  const k::Selection sel = k::selection_finish(ballots, counts, n);
  const int64_t m = sel.n_out;
  out->height = m;
  ColumnPtr rows;
  if (want_rows) { rows = empty_rows(); rows->len = m; rows->values = dev_alloc(values_bytes(PLX_U32, std::max<int64_t>(m, 1))); *want_rows = rows; }
  int n_moved = 0, n_bitmaps = 0;
  std::vector<ColumnPtr> outs(rows_only ? 0 : src->cols.size());
  // A SPARSE selection (under a sixteenth of the rows: a selective predicate, a semi join against a small side) does not stream every column through the compaction
  // kernel -- that reads all of them whatever is kept -- but takes the kept ROW IDS (one thread per wave tile walks the ballots) and gathers: the lines of the kept rows only.
  static const bool no_sparse = getenv("PLX_FILTER_SPARSE") && getenv("PLX_FILTER_SPARSE")[0] == '0';
  if (!rows_only && !no_sparse && m < n && m * 16 <= n && n < 0xffffffffll) {
    ColumnPtr ids = rows;
    if (!ids) { ids = empty_rows(); ids->len = m; ids->values = dev_alloc(values_bytes(PLX_U32, std::max<int64_t>(m, 1))); }
    k::compact_by_ballots(sel, k::CompactCols{}, ids->values->as<uint32_t>());
    out->cols.assign(src->cols.size(), nullptr);
    for (size_t b0 = 0; b0 < src->cols.size(); b0 += (size_t)k::kGatherMultiMax) {
      std::vector<ColumnPtr> part(src->cols.begin() + b0, src->cols.begin() + std::min(src->cols.size(), b0 + (size_t)k::kGatherMultiMax));
      std::vector<ColumnPtr> got = ops::gather_columns(part, ids);
      for (size_t j = 0; j < got.size(); j++) out->cols[b0 + j] = got[j];
    }
    PLX_HIP(hipStreamSynchronize(stream()));
    plan.desc += "FusedFilter{fused_scan[" + std::string(jit::program_mode(static_id, n)) + "]+ballots -> scan -> row ids -> gather x" + std::to_string(src->cols.size()) + (want_rows ? ", row ids" : "") +
                 ", kept=" + std::to_string(m) + "/" + std::to_string(n) + "}; ";
    return true;
  }
  if (m == n && !rows_only) { out->cols = src->cols; }                      // every row kept (filter/mod.rs:47-49)
  else if (!rows_only) {
    k::CompactCols cc{};
    bool need_plan = false;
    for (size_t i = 0; i < src->cols.size(); i++) {
      const ColumnPtr& col = src->cols[i];
      auto o = std::make_shared<Column>();
      o->dtype = col->dtype; o->len = m;
      const int w = dtype_width(col->dtype);
      o->values = col->dtype == PLX_BOOL ? dev_alloc_zero(bitmap_bytes(m)) : dev_alloc(values_bytes(col->dtype, m));
      if (col->validity) { o->validity = dev_alloc_zero(bitmap_bytes(m)); need_plan = true; } else o->null_count = 0;
      if (col->dtype == PLX_BOOL || !(w == 1 || w == 2 || w == 4 || w == 8)) need_plan = true;
      outs[i] = o;
    }
    // fixed-width values: kCompactMaxCols columns per launch of the all-columns kernel
    for (size_t i = 0; i < src->cols.size();) {
      cc = k::CompactCols{};
      for (; i < src->cols.size() && cc.n_cols < k::kCompactMaxCols; i++) {
        const ColumnPtr& col = src->cols[i];
        const int w = dtype_width(col->dtype);
        if (col->dtype == PLX_BOOL || !(w == 1 || w == 2 || w == 4 || w == 8)) continue;
        cc.in[cc.n_cols] = col->data(); cc.out[cc.n_cols] = outs[i]->values->ptr; cc.width[cc.n_cols] = (uint8_t)w; cc.n_cols++;
      }
      if (cc.n_cols || (rows && !n_moved)) k::compact_by_ballots(sel, cc, rows && !n_moved ? rows->values->as<uint32_t>() : nullptr);
      if (rows && !n_moved) rows = nullptr;
      n_moved += cc.n_cols;
    }
    if (need_plan) {
      Buf mask;
      const k::FilterPlan fp = k::selection_to_plan(sel, &mask);
      for (size_t i = 0; i < src->cols.size(); i++) {
        const ColumnPtr& col = src->cols[i];
        const int w = dtype_width(col->dtype);
        if (col->dtype == PLX_BOOL || !(w == 1 || w == 2 || w == 4 || w == 8)) {
          k::filter_apply(fp, w, col->data(), col->valid_words(), outs[i]->values->ptr, outs[i]->validity ? outs[i]->validity->as<uint64_t>() : nullptr);
          n_bitmaps++;
        } else if (col->validity) { k::filter_apply(fp, 0, col->valid_words(), nullptr, outs[i]->validity->ptr, nullptr); n_bitmaps++; }      // the validity bitmap compacted as a bitmap
      }
      PLX_HIP(hipStreamSynchronize(stream()));       // `mask` and the plan's offsets live until the compactions that read them are done
    }
    out->cols = outs;
  }
  if (rows) k::compact_by_ballots(sel, k::CompactCols{}, rows->values->as<uint32_t>());      // (row ids only)
  PLX_HIP(hipStreamSynchronize(stream()));           // the selection's buffers live until the kernels that read them are done
  plan.desc += "FusedFilter{fused_scan[" + std::string(jit::program_mode(static_id, n)) + "]+ballots -> scan -> " + (rows_only ? std::string("row ids") : "compaction of " + std::to_string(n_moved) +
               " columns in one pass" + (n_bitmaps ? " (+" + std::to_string(n_bitmaps) + " bitmaps through the selection bitmap)" : "") + (want_rows ? ", row ids" : "")) +
               ", kept=" + std::to_string(m) + "/" + std::to_string(n) + "}; ";
  return true;
}
// fused_filter_frame as a step of a join pipeline: the kept rows only (`rows`), or the filtered frame behind a membership test; what it would add to the plan text comes
// back in `phrase`, behind `lead` and without the closing "; ", for the pipeline's own entry.
static bool filter_phrase(Plan& plan, const std::vector<int>& preds, const FramePtr& src, FramePtr& out, std::string* why, ColumnPtr* rows, const MemberTest* member, const char* lead, std::string& phrase) {
  const size_t mark = plan.desc.size();
  if (!fused_filter_frame(plan, preds, src, out, why, rows, rows != nullptr, member)) return false;
  phrase = lead + plan.desc.substr(mark);
  plan.desc.resize(mark);
  while (!phrase.empty() && (phrase.back() == ' ' || phrase.back() == ';')) phrase.pop_back();
  return true;
}

// ------------------------------------------------------------ window expressions ----
// `f.over(keys)` (WindowExpr, mapping group_to_rows): the windows of a node's expression list are collected, bucketed by key list, and every bucket runs ONE
// group-by with the union of its aggregates (groupby_columns: all eleven kinds, shared cells and sorted segments), evaluates each function over the group frame the
// way exec_groupby_materialised evaluates an aggregate list, and sends the G-row columns back to the rows through one row -> group map and one broadcast
// (kernels_window.hip).  eval() then finds the finished columns in the override map.  DESIGN.md 4.17.
static void collect_windows(const Plan& plan, int e, std::vector<int>& out) {
  if (e < 0) return;
  const AE& x = plan.ae[e];
  // (a cumulative or ranking node that stands by itself is collected with the windows: its partition is the whole column)
  if (x.kind == PLX_AE_WINDOW || is_rowfn(x)) { if (std::find(out.begin(), out.end(), e) == out.end()) out.push_back(e); return; }
  collect_windows(plan, x.lhs, out);
  collect_windows(plan, x.rhs, out);
  collect_windows(plan, x.cond, out);
}
// the same expression, node by node (the arena holds one copy per place an expression was written)
static bool same_expr(const Plan& plan, int a, int b) {
  if (a == b) return true;
  if (a < 0 || b < 0) return false;
  const AE &x = plan.ae[a], &y = plan.ae[b];
  if (x.kind != y.kind || x.op != y.op || x.dtype != y.dtype || x.is_null != y.is_null || x.lit.u != y.lit.u || x.name != y.name || x.lut != y.lut) return false;
  return same_expr(plan, x.lhs, y.lhs) && same_expr(plan, x.rhs, y.rhs) && same_expr(plan, x.cond, y.cond);
}
static std::vector<int> window_keys(const Plan& plan, int w) {
  std::vector<int> keys;
  for (int l = plan.ae[w].rhs; l >= 0; l = plan.ae[l].rhs) keys.push_back(plan.ae[l].lhs);
  return keys;
}
// the group-by, the functions over the group frame, the map and the broadcast of one bucket: keys (N rows), values / aggs / params as groupby_columns takes them,
// finish(oaggs, G) -> the G-row columns to send back.  *desc = "Window{...}"
template <class Finish>
static std::vector<ColumnPtr> window_bucket(const std::vector<ColumnPtr>& keys, const std::vector<ColumnPtr>& values, const std::vector<int>& aggs, const std::vector<AggParams>& params,
                                            const std::string& key_names, Finish&& finish, std::string* desc) {
  std::vector<ColumnPtr> okeys, oaggs;
  std::string gd;
  groupby_columns(keys, values, aggs, false, okeys, oaggs, &gd, &params);
  const int64_t G = okeys.empty() ? 0 : okeys[0]->len;
  std::vector<ColumnPtr> gcols = finish(oaggs, G);
  const window::RowMap map = window::map_rows(keys, okeys);
  std::vector<ColumnPtr> out = window::broadcast(map, gcols);
  if (desc) *desc = "Window{keys=[" + key_names + "], aggs=" + std::to_string(aggs.size()) + ", groups=" + std::to_string(G) + ", rows=" + std::to_string(keys[0]->len) + ", route=" + map.desc + "; " + gd + "}; ";
  return out;
}
static ColumnPtr empty_column(int dtype) {
  auto c = std::make_shared<Column>();
  c->dtype = dtype; c->len = 0; c->null_count = 0; c->values = dev_alloc(values_bytes(dtype, 1) + 8);
  return c;
}
// ---- cumulative and ranking functions ----
// One per-row function of a node: `id` is the node eval() will look up (the PLX_AE_CUMULATIVE / PLX_AE_RANK itself, or the PLX_AE_WINDOW around it), `fn` the
// function, `keys` the window's keys (none: the whole column).
struct RowFn { int id, fn; std::vector<int> keys; };
static std::string rowfn_name(const AE& x) {
  if (x.kind == PLX_AE_SHIFT) return x.op == 1 ? "diff" : "shift";
  if (x.kind == PLX_AE_ROLLING) return rolling::op_name(x.op);
  return x.kind == PLX_AE_RANK ? "rank" : cumulative::op_name(x.op);
}
// Buckets by key list: the cumulative functions of a bucket share one stable sort of the rows by the keys and one head mask (cumulative::scan_order); its ranks
// share one sort_segments per (operand, descending) (cumulative::rank_order).  Every finished column goes into `done` under the function's id.
static void run_rowfns(Plan& plan, const std::vector<RowFn>& fns, const Frame& in, std::map<int, ColumnPtr>& done) {
  struct Bucket { std::vector<int> keys; std::vector<RowFn> fns; };
  std::vector<Bucket> buckets;
  for (const RowFn& r : fns) {
    const AE& f = plan.ae[r.fn];
    const std::string name = rowfn_name(f);
    PLX_REQUIRE(!contains_rowfn(plan, f.lhs), PLX_ERR_UNSUPPORTED, name + ": a cumulative / ranking expression inside the operand of another one is not built; compute the inner one in with_columns first");
    PLX_REQUIRE(!contains_window(plan, f.lhs), PLX_ERR_UNSUPPORTED, name + ": a window expression (.over) inside the operand of a cumulative / ranking expression is not built; compute it in with_columns first");
    PLX_REQUIRE(!contains_agg(plan, f.lhs), PLX_ERR_UNSUPPORTED, name + ": an aggregate inside the operand of a cumulative / ranking expression is not built; the operand is a row-level expression");
    for (int kx : r.keys) {
      PLX_REQUIRE(!contains_window(plan, kx) && !contains_rowfn(plan, kx), PLX_ERR_INVALID, "window expression: a key that holds a window");
      PLX_REQUIRE(!contains_agg(plan, kx), PLX_ERR_INVALID, "window expression: a key that holds an aggregate (" + output_name(plan, kx) + "); keys are row expressions");
    }
    Bucket* b = nullptr;
    for (Bucket& c : buckets) {
      bool same = c.keys.size() == r.keys.size();
      for (size_t j = 0; same && j < r.keys.size(); j++) same = same_expr(plan, c.keys[j], r.keys[j]);
      if (same) { b = &c; break; }
    }
    if (!b) { buckets.push_back(Bucket{r.keys, {}}); b = &buckets.back(); }
    b->fns.push_back(r);
  }
  for (const Bucket& b : buckets) {
    std::string key_names;
    for (int kx : b.keys) key_names += (key_names.empty() ? "" : ", ") + output_name(plan, kx);
    std::vector<RowFn> cums, ranks, shifts, rolls;
    for (const RowFn& r : b.fns) {
      const int kind = plan.ae[r.fn].kind;
      (kind == PLX_AE_RANK ? ranks : kind == PLX_AE_SHIFT ? shifts : kind == PLX_AE_ROLLING ? rolls : cums).push_back(r);
    }
    // the windows of the bucket's rolling functions, as written, for the plan text
    std::string roll_w;
    for (const RowFn& r : rolls) {
      const std::string w = std::to_string((long long)rolling::unpack_params(plan.ae[r.fn].lit.u).window);
      if (("+" + roll_w + "+").find("+" + w + "+") == std::string::npos) roll_w += (roll_w.empty() ? "" : "+") + w;
    }
    const std::string rows = ", rows=" + std::to_string(in.height);
    if (in.height == 0) {      // an empty frame: empty columns of the right dtype, the plan text in the shape of every other
      for (int kx : b.keys) infer_dtype(plan, kx, in);
      for (const RowFn& r : b.fns) done[r.id] = empty_column(infer_dtype(plan, r.fn, in));
      if (!cums.empty()) plan.desc += "Cumulative{keys=[" + key_names + "], fns=" + std::to_string(cums.size()) + rows + ", route=cumulative[empty]}; ";
      if (!ranks.empty()) plan.desc += "Rank{keys=[" + key_names + "], fns=" + std::to_string(ranks.size()) + rows + ", route=rank[empty]}; ";
      if (!shifts.empty()) plan.desc += "Shift{keys=[" + key_names + "], fns=" + std::to_string(shifts.size()) + rows + ", route=shift[empty]}; ";
      if (!rolls.empty()) plan.desc += "Rolling{keys=[" + key_names + "], fns=" + std::to_string(rolls.size()) + rows + ", w=" + roll_w + ", route=rolling[empty]}; ";
      continue;
    }
    std::vector<ColumnPtr> keys;
    for (int kx : b.keys) keys.push_back(broadcast(eval(plan, kx, in, nullptr), in.height));
    // one column per operand expression, the same operand written twice included
    std::vector<std::pair<int, ColumnPtr>> operands;
    auto operand = [&](int e) {
      for (auto& kv : operands) if (same_expr(plan, kv.first, e)) return kv.second;
      operands.emplace_back(e, broadcast(eval(plan, e, in, nullptr), in.height));
      return operands.back().second;
    };
    flush_node_notes(plan);
    // cumulative, shift and rolling functions of the bucket share ONE stable sort of the rows by the keys and one head mask; the shift and rolling functions also
    // share the mask's prefix and compacted starts (their O(1) segment bounds)
    cumulative::ScanOrder order;
    if (!cums.empty() || !shifts.empty() || !rolls.empty()) order = cumulative::scan_order(keys, in.height);
    rolling::Segments segs;
    if (!shifts.empty() || !rolls.empty()) segs = rolling::segments_of(order);
    const std::string order_desc = order.desc.rfind("cumulative[", 0) == 0 ? order.desc.substr(std::string("cumulative[").size()) : order.desc;      // "whole column]" | "sorted rows: ...]"
    if (!cums.empty()) {
      for (size_t i = 0; i < cums.size(); i++) {
        const RowFn& r = cums[i];
        const AE& f = plan.ae[r.fn];
        infer_dtype(plan, r.fn, in);      // (the operand's dtype is refused by name before anything runs)
        size_t twin = i;                  // the same function written twice is scanned once
        for (size_t j = 0; j < i && twin == i; j++) if (same_expr(plan, cums[j].fn, r.fn)) twin = j;
        done[r.id] = twin < i ? done[cums[twin].id] : cumulative::scan_column(order, operand(f.lhs), f.op, f.lit.u != 0);
      }
      plan.desc += "Cumulative{keys=[" + key_names + "], fns=" + std::to_string(cums.size()) + rows + ", route=" + order.desc + "}; ";
    }
    if (!shifts.empty()) {
      for (size_t i = 0; i < shifts.size(); i++) {
        const RowFn& r = shifts[i];
        const AE& f = plan.ae[r.fn];
        infer_dtype(plan, r.fn, in);      // (the operand's dtype and the fill literal's are refused by name before anything runs)
        size_t twin = i;
        for (size_t j = 0; j < i && twin == i; j++) if (same_expr(plan, shifts[j].fn, r.fn)) twin = j;
        if (twin < i) { done[r.id] = done[shifts[twin].id]; continue; }
        const plx_scalar* fill = f.rhs >= 0 ? &plan.ae[f.rhs].lit : nullptr;
        done[r.id] = rolling::shift_column(order, segs, operand(f.lhs), f.lit.i, fill, f.op == 1);
      }
      plan.desc += "Shift{keys=[" + key_names + "], fns=" + std::to_string(shifts.size()) + rows + ", route=shift[" + order_desc + "}; ";
    }
    if (!rolls.empty()) {
      std::string routes;
      for (size_t i = 0; i < rolls.size(); i++) {
        const RowFn& r = rolls[i];
        const AE& f = plan.ae[r.fn];
        infer_dtype(plan, r.fn, in);
        size_t twin = i;
        for (size_t j = 0; j < i && twin == i; j++) if (same_expr(plan, rolls[j].fn, r.fn)) twin = j;
        if (twin < i) { done[r.id] = done[rolls[twin].id]; continue; }
        std::string route;
        done[r.id] = rolling::rolling_column(order, segs, operand(f.lhs), f.op, rolling::unpack_params(f.lit.u), &route);
        if (routes.find(route) == std::string::npos) routes += (routes.empty() ? "" : " + ") + route;
      }
      plan.desc += "Rolling{keys=[" + key_names + "], fns=" + std::to_string(rolls.size()) + rows + ", w=" + roll_w + ", route=" + routes + (order.perm ? "; " + order_desc.substr(0, order_desc.size() - 1) : "") + "}; ";
    }
    std::vector<bool> ranked(ranks.size(), false);
    for (size_t i = 0; i < ranks.size(); i++) {
      if (ranked[i]) continue;
      const AE& f = plan.ae[ranks[i].fn];
      const cumulative::RankOrder order = cumulative::rank_order(keys, operand(f.lhs), f.lit.u != 0);
      std::string methods;
      int n_fns = 0;
      for (size_t j = i; j < ranks.size(); j++) {
        const AE& g = plan.ae[ranks[j].fn];
        if (ranked[j] || !same_expr(plan, f.lhs, g.lhs) || (f.lit.u != 0) != (g.lit.u != 0)) continue;
        ranked[j] = true; n_fns++;
        size_t twin = j;
        for (size_t t = i; t < j && twin == j; t++) if (ranked[t] && same_expr(plan, ranks[t].fn, ranks[j].fn)) twin = t;
        done[ranks[j].id] = twin < j ? done[ranks[twin].id] : cumulative::rank_column(order, g.op);
        const std::string m = cumulative::method_name(g.op);
        if (methods.find(m) == std::string::npos) methods += (methods.empty() ? "" : "+") + m;
      }
      plan.desc += "Rank{keys=[" + key_names + "], fns=" + std::to_string(n_fns) + rows + ", method=" + methods + (f.lit.u ? ", descending" : "") + ", route=" + order.desc + "}; ";
    }
  }
}
// the function a window wraps, through its aliases
static int window_function(const Plan& plan, int w) {
  int f = plan.ae[w].lhs;
  while (f >= 0 && plan.ae[f].kind == PLX_AE_ALIAS) f = plan.ae[f].lhs;
  return f;
}

static void run_windows(Plan& plan, const std::vector<int>& exprs, const Frame& in, std::map<int, ColumnPtr>& done) {
  std::vector<int> collected, wins;
  for (int e : exprs) collect_windows(plan, e, collected);
  if (collected.empty()) return;
  // the cumulative and ranking functions first: plain ones, and windows whose function is one
  std::vector<RowFn> rowfns;
  for (int w : collected) {
    if (is_rowfn(plan.ae[w])) { rowfns.push_back(RowFn{w, w, {}}); continue; }
    const int f = window_function(plan, w);
    if (f >= 0 && is_rowfn(plan.ae[f])) { rowfns.push_back(RowFn{w, f, window_keys(plan, w)}); continue; }
    PLX_REQUIRE(!contains_rowfn(plan, plan.ae[w].lhs), PLX_ERR_UNSUPPORTED,
                "window expression: its function mixes a cumulative / ranking expression with something else; .over(keys) goes directly on the cumulative / ranking expression (and on each aggregate), the arithmetic outside");
    wins.push_back(w);
  }
  if (!rowfns.empty()) run_rowfns(plan, rowfns, in, done);
  if (wins.empty()) return;
  struct Bucket { std::vector<int> keys, wins; };
  std::vector<Bucket> buckets;
  for (int w : wins) {
    const int f = plan.ae[w].lhs;
    const std::vector<int> keys = window_keys(plan, w);
    PLX_REQUIRE(!contains_window(plan, f), PLX_ERR_UNSUPPORTED, "window expression: a window inside the function of another window is not built");
    PLX_REQUIRE(contains_agg(plan, f) && !contains_column_outside_agg(plan, f), PLX_ERR_UNSUPPORTED,
                "window expression over [" + output_name(plan, keys[0]) + (keys.size() > 1 ? ", ..." : "") + "]: its function does not reduce to one value per partition (a column outside an aggregate, or no aggregate at all); "
                "window functions that do not aggregate (a bare column) are not built");
    for (int kx : keys) {
      PLX_REQUIRE(!contains_window(plan, kx), PLX_ERR_INVALID, "window expression: a key that holds a window");
      PLX_REQUIRE(!contains_agg(plan, kx), PLX_ERR_INVALID, "window expression: a key that holds an aggregate (" + output_name(plan, kx) + "); keys are row expressions");
    }
    Bucket* b = nullptr;
    for (Bucket& c : buckets) {
      bool same = c.keys.size() == keys.size();
      for (size_t j = 0; same && j < keys.size(); j++) same = same_expr(plan, c.keys[j], keys[j]);
      if (same) { b = &c; break; }
    }
    if (!b) { buckets.push_back(Bucket{keys, {}}); b = &buckets.back(); }
    b->wins.push_back(w);
  }
  for (const Bucket& b : buckets) {
    std::vector<ColumnPtr> keys, values;
    std::vector<int> aggs, agg_nodes;
    std::vector<AggParams> params;
    std::map<int, ColumnPtr> by_expr;
    std::string key_names;
    for (int kx : b.keys) key_names += (key_names.empty() ? "" : ", ") + output_name(plan, kx);
    for (int w : b.wins) collect_aggs(plan, plan.ae[w].lhs, agg_nodes);
    if (in.height == 0) {      // an empty frame: an empty column of the function's dtype, the plan text in the shape of every other
      for (int kx : b.keys) infer_dtype(plan, kx, in);      // (a key that names no column is still refused)
      for (int w : b.wins) done[w] = empty_column(infer_dtype(plan, plan.ae[w].lhs, in));
      plan.desc += "Window{keys=[" + key_names + "], aggs=" + std::to_string(agg_nodes.size()) + ", groups=0, rows=0, route=window[empty]}; ";
      continue;
    }
    for (int kx : b.keys) keys.push_back(broadcast(eval(plan, kx, in, nullptr), in.height));
    for (int a : agg_nodes) {
      const AE& x = plan.ae[a];
      AggParams ap;
      if (x.kind == PLX_AE_AGG && (x.op == PLX_AGG_VAR || x.op == PLX_AGG_STD)) ap.ddof = (int)x.lit.u;
      if (x.kind == PLX_AE_AGG && x.op == PLX_AGG_QUANTILE) { ap.q = x.lit.f64; ap.interpolation = x.dtype; }
      params.push_back(ap);
      if (x.kind == PLX_AE_LEN) { aggs.push_back(PLX_AGG_LEN); values.push_back(nullptr); continue; }
      // one column per source expression, the same source written twice included: aggregates over one source share cells and sorted segments
      ColumnPtr src;
      for (auto& kv : by_expr) if (same_expr(plan, kv.first, x.lhs)) { src = kv.second; break; }
      if (!src) src = by_expr.emplace(x.lhs, broadcast(eval(plan, x.lhs, in, nullptr), in.height)).first->second;
      aggs.push_back(x.op); values.push_back(src);
    }
    flush_node_notes(plan);
    std::string d;
    std::vector<ColumnPtr> cols = window_bucket(keys, values, aggs, params, key_names, [&](const std::vector<ColumnPtr>& oaggs, int64_t G) {
      std::map<int, ColumnPtr> overrides;
      for (size_t i = 0; i < agg_nodes.size(); i++) overrides[agg_nodes[i]] = oaggs[i];
      Frame gframe; gframe.height = G;
      std::vector<ColumnPtr> g;
      for (int w : b.wins) g.push_back(broadcast(eval(plan, plan.ae[w].lhs, gframe, &overrides), G));
      return g;
    }, &d);
    for (size_t i = 0; i < b.wins.size(); i++) done[b.wins[i]] = cols[i];
    plan.desc += d;
  }
}

// plx_window_agg: one window per aggregate over the same key columns
void window_columns(const std::vector<ColumnPtr>& keys, const std::vector<ColumnPtr>& values, const std::vector<int>& aggs, const std::vector<AggParams>* params,
                    std::vector<ColumnPtr>& out_cols, std::string* desc) {
  PLX_REQUIRE(!keys.empty(), PLX_ERR_INVALID, "window: need at least one key column");
  PLX_REQUIRE((int)keys.size() <= window::kMaxKeys, PLX_ERR_UNSUPPORTED, "window over " + std::to_string(keys.size()) + " keys; a window takes 1.." + std::to_string(window::kMaxKeys) + " keys on this path");
  PLX_REQUIRE(values.size() == aggs.size() && !aggs.empty(), PLX_ERR_INVALID, "window: values/aggs length mismatch");
  const int64_t n = keys[0]->len;
  for (auto& kc : keys) PLX_REQUIRE(kc->len == n, PLX_ERR_SHAPE, "window: key length mismatch");
  for (auto& v : values) PLX_REQUIRE(!v || v->len == n, PLX_ERR_SHAPE, "window: value length mismatch");
  PLX_REQUIRE(!params || params->size() == aggs.size(), PLX_ERR_INVALID, "window: params/aggs length mismatch");
  std::vector<AggParams> ps = params ? *params : std::vector<AggParams>(aggs.size());
  // the parameters are checked here, by name, whatever the height: an empty frame never reaches the group-by that checks them otherwise
  for (size_t i = 0; i < aggs.size(); i++) {
    PLX_REQUIRE(aggs[i] >= PLX_AGG_SUM && aggs[i] <= PLX_AGG_N_UNIQUE && aggs[i] != PLX_AGG_FIRST, PLX_ERR_INVALID, "window: aggregate " + std::to_string(aggs[i]) + " is no window aggregate (plx_agg_op but FIRST)");
    if (aggs[i] == PLX_AGG_VAR || aggs[i] == PLX_AGG_STD) PLX_REQUIRE(ps[i].ddof >= 0 && ps[i].ddof <= 255, PLX_ERR_INVALID, "window: ddof must be 0..255");
    if (aggs[i] == PLX_AGG_QUANTILE) {
      PLX_REQUIRE(quantile::q_ok(ps[i].q), PLX_ERR_INVALID, "window: quantile q must be a real number in [0, 1], got " + std::to_string(ps[i].q));
      PLX_REQUIRE(quantile::interpolation_ok(ps[i].interpolation), PLX_ERR_INVALID, "window: interpolation " + std::to_string(ps[i].interpolation) + " is no plx_quantile_interpolation (0..4)");
    }
  }
  if (n == 0) {
    for (size_t i = 0; i < aggs.size(); i++) {
      const int in = values[i] ? values[i]->dtype : PLX_U32;
      int dt = in;
      switch (aggs[i]) {
        case PLX_AGG_SUM: dt = sum_out_dtype(in); break;
        case PLX_AGG_MEAN: case PLX_AGG_VAR: case PLX_AGG_STD: case PLX_AGG_QUANTILE: dt = in == PLX_F32 ? PLX_F32 : PLX_F64; break;
        case PLX_AGG_COUNT: case PLX_AGG_LEN: case PLX_AGG_N_UNIQUE: dt = PLX_U32; break;
        default: break;
      }
      out_cols.push_back(empty_column(dt));
    }
    if (desc) *desc = "Window{keys=[" + std::to_string(keys.size()) + " columns], aggs=" + std::to_string(aggs.size()) + ", groups=0, rows=0, route=window[empty]}; ";
    return;
  }
  out_cols = window_bucket(keys, values, aggs, ps, std::to_string(keys.size()) + " columns", [](const std::vector<ColumnPtr>& oaggs, int64_t) { return oaggs; }, desc);
}

static FramePtr exec_filter(Plan& plan, const IRN& n) {
  if (!(plan.flags & PLX_PLAN_NO_FUSION)) {
    std::vector<int> preds;
    const int src_node = peel_filters(plan, n.input, preds);
    preds.push_back(n.predicate);
    FramePtr src = exec_node(plan, src_node);
    FramePtr out; std::string why;
    if (fused_filter_frame(plan, preds, src, out, &why)) return out;
    plan.desc += "(filter not fused: " + why + ") ";
    plan.memo[src_node] = src;
  }
  FramePtr in = exec_node(plan, n.input);
  std::map<int, ColumnPtr> wins;
  run_windows(plan, {n.predicate}, *in, wins);
  Evaluated m = eval(plan, n.predicate, *in, wins.empty() ? nullptr : &wins);
  ColumnPtr mask = broadcast(m, in->height);
  PLX_REQUIRE(mask->dtype == PLX_BOOL, PLX_ERR_INVALID, "filter predicate must be boolean");
  auto pm = ops::prepare_mask(mask);
  auto out = std::make_shared<Frame>();
  out->names = in->names;
  out->height = ops::prepared_rows(*pm);
  for (auto& c : in->cols) out->cols.push_back(ops::filter_prepared(c, *pm));
  plan.desc += "Filter{cmp->bitmap, filter_compact x" + std::to_string(in->cols.size()) + "}; ";
  return out;
}

static FramePtr exec_select(Plan& plan, const IRN& n, bool hstack, FramePtr in_given = nullptr) {
  FramePtr in = in_given ? in_given : exec_node(plan, n.input);
  auto out = std::make_shared<Frame>();
  std::vector<Evaluated> evs;
  bool all_scalar = true;
  std::map<int, ColumnPtr> wins;
  run_windows(plan, n.exprs, *in, wins);
  for (int e : n.exprs) { evs.push_back(eval(plan, e, *in, wins.empty() ? nullptr : &wins)); all_scalar = all_scalar && evs.back().scalar; }
  if (hstack) {
    *out = *in;
    for (size_t i = 0; i < n.exprs.size(); i++) {
      ColumnPtr c = broadcast(evs[i], in->height);
      std::string name = output_name(plan, n.exprs[i]);
      int at = out->find(name);
      if (at >= 0) out->cols[at] = c; else { out->names.push_back(name); out->cols.push_back(c); }
    }
    flush_node_notes(plan);
    plan.desc += "HStack{per-node kernels}; ";
    return out;
  }
  out->height = all_scalar ? 1 : in->height;
  for (size_t i = 0; i < n.exprs.size(); i++) {
    out->names.push_back(output_name(plan, n.exprs[i]));
    out->cols.push_back(all_scalar ? evs[i].col : broadcast(evs[i], in->height));
  }
  flush_node_notes(plan);
  plan.desc += "Select{per-node kernels}; ";
  return out;
}

static FramePtr exec_groupby_materialised(Plan& plan, const IRN& n, const FramePtr& in) {
  // evaluate key and aggregation-input expressions as columns, then the generic grouped aggregation
  std::vector<ColumnPtr> keys, values;
  std::vector<int> aggs, agg_nodes;
  std::vector<AggParams> params;
  std::map<int, ColumnPtr> by_expr;      // one column per source expression: the quantiles over one source share its sort
  for (int e : n.keys) keys.push_back(broadcast(eval(plan, e, *in, nullptr), in->height));
  for (int e : n.exprs) collect_aggs(plan, e, agg_nodes);
  for (int a : agg_nodes) {
    const AE& x = plan.ae[a];
    AggParams ap;
    if (x.kind == PLX_AE_AGG && (x.op == PLX_AGG_VAR || x.op == PLX_AGG_STD)) ap.ddof = (int)x.lit.u;
    if (x.kind == PLX_AE_AGG && x.op == PLX_AGG_QUANTILE) { ap.q = x.lit.f64; ap.interpolation = x.dtype; }
    params.push_back(ap);
    if (x.kind == PLX_AE_LEN) { aggs.push_back(PLX_AGG_LEN); values.push_back(nullptr); }
    else {
      auto it = by_expr.find(x.lhs);
      if (it == by_expr.end()) it = by_expr.emplace(x.lhs, broadcast(eval(plan, x.lhs, *in, nullptr), in->height)).first;
      aggs.push_back(x.op); values.push_back(it->second);
    }
  }
  flush_node_notes(plan);
  std::vector<ColumnPtr> okeys, oaggs;
  std::string d;
  groupby_columns(keys, values, aggs, n.maintain_order != 0, okeys, oaggs, &d, &params);
  plan.desc += "GroupBy{materialised inputs; " + d + "}; ";
  auto out = std::make_shared<Frame>();
  out->height = okeys.empty() ? 0 : okeys[0]->len;
  for (size_t i = 0; i < n.keys.size(); i++) { out->names.push_back(output_name(plan, n.keys[i])); out->cols.push_back(okeys[i]); }
  std::map<int, ColumnPtr> overrides;
  for (size_t i = 0; i < agg_nodes.size(); i++) overrides[agg_nodes[i]] = oaggs[i];
  Frame gframe; gframe.height = out->height;
  for (int e : n.exprs) {
    Evaluated ev = eval(plan, e, gframe, &overrides);
    out->names.push_back(output_name(plan, e));
    out->cols.push_back(broadcast(ev, out->height));
  }
  return out;
}


// ------------------------------------------------ fused Join -> frame pipeline ----
// Join(inner | left; one plain integer key pair) of two [Filter]* inputs that RETURNS A FRAME (the reference: JoinExec polars-mem-engine/src/executors/join.rs:41-121 ->
// _inner_join_from_series / _left_join_from_series polars-ops/src/frame/join/mod.rs:564-652 -> hash_join_tuples_inner single_keys_inner.rs:40-149 -> gathers).
// The filters never materialise their frames: the build side's predicate is fused into the build scan (k::fused_join_build: 16-byte {key, row} slots, chains of
// rows for duplicate keys), the probe side's into the scatter of the partitioned probe (k::partitioned_hash_probe_hits: rows radix-partitioned by the key's hash,
// each partition tested against an LDS filter of its region of the table) or -- joins that keep most probe rows, left joins, small tables -- into the one-pass
// row-id compaction (k::fused_filter); join::join_pairs then looks every CANDIDATE up once and lays the (probe row, build row) pairs out, and the payload columns
// `want` names (null: all) are gathered at them, several columns per launch.  PLX_JOIN_MATERIALISE: 0 = never, 2 = any size (tests), default from 2^24 probe rows.
static int join_wide_keys_mode() { const char* e = getenv("PLX_JOIN_WIDE_KEYS"); return e && e[0] == '0' ? 0 : e && e[0] == '2' ? 2 : 1; }   // (read at every join: the tests switch it)
static int join_materialise_mode() { const char* e = getenv("PLX_JOIN_MATERIALISE"); return e && e[0] == '0' ? 0 : e && e[0] == '2' ? 2 : 1; }
static bool fused_join_frame(Plan& plan, const IRN& jn, const std::set<std::string>* want, FramePtr& out, std::string* why, uint64_t* build_rows_out = nullptr, int* build_side_out = nullptr) {
  auto no = [&](const char* m) { if (why) *why = m; return false; };
  const int mode = join_materialise_mode();
  const AE *lkx = nullptr, *rkx = nullptr;
  if (const char* bad = single_key_join(plan, jn, false, mode == 0 ? "disabled (PLX_JOIN_MATERIALISE=0)" : nullptr, lkx, rkx)) return no(bad);
  const bool left_join = jn.how == PLX_JOIN_LEFT;
  std::vector<int> lpreds, rpreds;
  const int lsrc = peel_filters(plan, jn.input, lpreds), rsrc = peel_filters(plan, jn.input_right, rpreds);
  // (cheap checks on scans first: a join this path does not take must not have executed its inputs twice)
  auto height_of = [&](int node) -> int64_t { return plan.ir[node].kind == PLX_IR_SCAN ? get_frame(plan.ir[node].frame)->height : -1; };
  if (mode == 1 && height_of(lsrc) >= 0 && height_of(rsrc) >= 0 && std::max(height_of(lsrc), height_of(rsrc)) < ((int64_t)1 << 24)) return no("small inputs");
  FramePtr L = exec_node(plan, lsrc), R = exec_node(plan, rsrc);
  plan.memo[lsrc] = L; plan.memo[rsrc] = R;
  JoinSides sides;
  const char* bad = nullptr;
  if (!resolve_join_sides(sides, L, R, lkx, rkx, left_join, lpreds, rpreds, &bad)) return no(bad);
  const FramePtr &B = sides.B, &P = sides.P;
  const int bki = sides.bki, pki = sides.pki;
  const bool build_right = sides.build_right;
  const std::vector<int> &bpreds = sides.bpreds, &ppreds = sides.ppreds;
  if (mode == 1 && P->height < ((int64_t)1 << 24)) return no("small inputs");
  std::vector<JoinedCol> outs;
  if (!joined_columns(*L, *R, sides.rki, jn.suffix, outs, &bad)) return no(bad);
  Compiler cnt(plan, *B), cb(plan, *B), cs(plan, *P);
  try {
    cnt.pred = and_predicates(cnt, bpreds);
    const int bk_cnt = cnt.load(bki);
    cnt.add_agg(cnt.nodes[bk_cnt].nullable ? AGG_COUNT : AGG_LEN, cnt.nodes[bk_cnt].nullable ? bk_cnt : -1);
    cnt.finish();
    cb.pred = and_predicates(cb, bpreds);
    cb.key = cb.load(bki);
    cb.finish();
    cs.pred = and_predicates(cs, ppreds);
    cs.key = cs.load(pki);
    cs.add_agg(AGG_FIRST_ROW, -1);
    cs.finish();
  } catch (const Unsupported& u) { if (why) *why = u.why; return false; }
  // ---- direct-address table when the build keys have a dense range (cached column statistics): a bitmap over the key range + a rank per word + slot -> build row.  Probe
  // keys in key order walk the bitmap out of the L2 (the hits come out of the probe scan itself, in ballot form: DirectHitsSink); keys in no order are partitioned first
  // (k::partitioned_probe_hits).  Two pairs on one bit = duplicate build keys -> the hash-table pipeline below (chains).
  uint64_t nb = 0;
  bool done_direct = false, multi = B->height > 0 && B->cols[bki]->repeats_as_build_key;
  ColumnPtr pidx, bidx;
  std::string cand_how, pd, table_how;
  bool cand_in_row_order = true;            // false: the candidates are in partition order (partitioned probes) and were not put back
  // candidates of a partitioned probe go back into row order when the requested order can use it (join::order_pairs then has little or nothing to do)
  auto partitioned_candidates = [&](ColumnPtr& c) {
    if (!join::join_order_needs_probe_order(jn.maintain_order, build_right)) { cand_in_row_order = false; return; }
    std::string rd;
    join::restore_candidate_order(c, &rd);
    cand_how += " -> " + rd;
  };
  const int pmode = partitioned_probe_mode();
  {
    DirectBuild direct;
    const DirectBuild::Result built = direct.try_build(plan, cb, *B, bki, multi);
    if (built == DirectBuild::kDuplicateKeys) multi = true;
    else if (built == DirectBuild::kBuilt) {
      const DirectJoinTable& dt = direct.dt;
      const uint64_t range = direct.range;
      nb = direct.nb;
      Buf slot_row = dev_alloc(sizeof(uint32_t) * (size_t)std::max<uint64_t>(nb, 1));
      k::direct_slot_rows(dt, direct.n_ord, slot_row->as<uint32_t>());
      ColumnPtr cand;
      if (!left_join) {
        if (partition_direct_probe(pmode, *P, pki, range, nb)) {
          std::string ppd;
          if (k::partitioned_probe_hits(cs.shape, cs.args, dt, nb, find_static_shape(cs.shape), &cand, &ppd)) { cand_how = ppd; partitioned_candidates(cand); }
          else cand = nullptr;
        }
        if (!cand) {
          // the probe scan itself: predicate + bitmap test per row, ballots out; the hit rows' indices from the ballots (every one of them matches)
          const int64_t np = P->height, n_wt = (np + 127) / 128;
          cand = std::make_shared<Column>();
          cand->dtype = PLX_U32; cand->null_count = 0; cand->len = 0; cand->values = dev_alloc(8);
          if (np > 0) {
            Buf ballots = dev_alloc(sizeof(uint64_t) * 2 * (size_t)n_wt), counts = dev_alloc(sizeof(uint32_t) * (size_t)n_wt);
            const int sid = find_static_shape(cs.shape);
            k::fused_direct_hits(cs.shape, cs.args, dt, BallotOut{ballots->as<unsigned long long>(), counts->as<unsigned int>()}, sid);
            const k::Selection sel = k::selection_finish(ballots, counts, np);
            cand->len = sel.n_out;
            cand->values = dev_alloc(values_bytes(PLX_U32, std::max<int64_t>(sel.n_out, 1)));
            k::compact_by_ballots(sel, k::CompactCols{}, cand->values->as<uint32_t>());
            PLX_HIP(hipStreamSynchronize(stream()));
            cand_how = scan_tag(sid, np) + "direct hits (ballots -> row ids)";
          }
        }
      } else if (!ppreds.empty()) {
        FramePtr none; std::string fwhy;
        if (!filter_phrase(plan, ppreds, P, none, &fwhy, &cand, nullptr, "probe rows by ", cand_how)) { if (why) *why = "probe-side predicate: " + fwhy; return false; }
      } else cand_how = "every probe row";
      join::join_pairs_direct(jn.how, P->cols[pki], cand, dt, slot_row->as<uint32_t>(), pidx, bidx, &pd);
      PLX_HIP(hipStreamSynchronize(stream()));
      table_how = "direct-address table range=" + std::to_string(range) + " (bitmap + rank + slot rows) unique-keys";
      done_direct = true;
    }
  }
  if (build_rows_out && done_direct) *build_rows_out = nb;
  if (build_side_out) *build_side_out = build_right ? 1 : 0;
  if (!done_direct) {
  // ---- build (sized from a strided sample of the count program, rebuilt once if the sample misjudged; duplicate keys -> chains)
  HashBuild hb;
  hb.run(cnt, cb, *B, bki, HashBuildOptions{8, multi, true, false, ""});
  const JoinAggTable& t = hb.t;
  nb = hb.nb; multi = hb.multi;
  if (build_rows_out) *build_rows_out = nb;
  // ---- candidates
  ColumnPtr cand;
  if (!left_join && partition_hash_probe(pmode, *P, hb.cap, nb)) {
    std::string pd;
    if (k::partitioned_hash_probe_hits(cs.shape, cs.args, t, nb, find_static_shape(cs.shape), &cand, &pd)) { cand_how = pd; partitioned_candidates(cand); }
    else cand = nullptr;
  }
  if (!cand && !ppreds.empty()) {
    FramePtr none; std::string fwhy;
    if (!filter_phrase(plan, ppreds, P, none, &fwhy, &cand, nullptr, "probe rows by ", cand_how)) { if (why) *why = "probe-side predicate: " + fwhy; return false; }
  }
  if (!cand && cand_how.empty()) cand_how = "every probe row";
  // ---- pairs
  join::join_pairs(jn.how, P->cols[pki], cand, t, pidx, bidx, &pd);
  PLX_HIP(hipStreamSynchronize(stream()));
  table_how = "hash table cap=2^" + std::to_string(hb.log2_cap) + (hb.build_how.empty() ? "" : " [" + hb.build_how + "]") + (multi ? " multi-value (row chains)" : " unique-keys");
  }  // hash-table pipeline
  // ---- the order the join was asked to keep (plx_join_order): the pair list is ordered, the gathers below then produce the frame in that order
  if (jn.maintain_order != PLX_JOIN_ORDER_NONE) {
    join::PairProps props; props.probe_ordered = cand_in_row_order; props.runs_ordered = !multi;
    std::string od;
    join::order_pairs(jn.maintain_order, build_right, props, pidx, bidx, &od);
    pd += ", " + od;
  }
  // ---- payload: one multi-column gather per side
  const ColumnPtr& lidx = build_right ? pidx : bidx;
  const ColumnPtr& ridx = build_right ? bidx : pidx;
  out = std::make_shared<Frame>();
  out->height = pidx->len;
  std::vector<int> pick[2];
  std::vector<size_t> slot_of[2];
  for (size_t i = 0; i < outs.size(); i++) {
    if (want && !want->count(outs[i].name)) continue;
    out->names.push_back(outs[i].name); out->cols.push_back(nullptr);
    pick[outs[i].side].push_back(outs[i].idx); slot_of[outs[i].side].push_back(out->cols.size() - 1);
  }
  int n_gathered = 0;
  for (int side = 0; side < 2; side++) {
    const FramePtr& F = side == 0 ? L : R;
    const ColumnPtr& idx = side == 0 ? lidx : ridx;
    for (size_t b0 = 0; b0 < pick[side].size(); b0 += (size_t)k::kGatherMultiMax) {
      std::vector<ColumnPtr> srcs;
      for (size_t j = b0; j < std::min(pick[side].size(), b0 + (size_t)k::kGatherMultiMax); j++) srcs.push_back(F->cols[pick[side][j]]);
      std::vector<ColumnPtr> got = ops::gather_columns(srcs, idx);
      for (size_t j = 0; j < got.size(); j++) out->cols[slot_of[side][b0 + j]] = got[j];
      n_gathered += (int)got.size();
    }
  }
  PLX_HIP(hipStreamSynchronize(stream()));
  plan.desc += std::string("FusedJoinFrame{") + (left_join ? "left" : "inner") + ", build=" + (build_right ? "right" : "left") + " rows=" + std::to_string(nb) + "/" + std::to_string(B->height) + " " + table_how +
               ", probe rows=" + std::to_string(P->height) + ", candidates: " + cand_how + ", " + pd + ", gather x" + std::to_string(n_gathered) + "}; ";
  return true;
}

// Join(semi | anti, one integer key pair) over two `[Filter]*` inputs -> the left rows whose key is (not) among the right side's, left columns, left order
// (polars-ops/src/frame/join/hash_join/single_keys_semi_anti.rs: a hash SET of the right keys, one lookup per left row; dispatch_left_right.rs).  Here the right side
// -- its predicate fused into the scan -- becomes a membership BITMAP over its key range (BitmapBuildSink: the sink of the filter joins of §4.1), and the join is a
// FILTER of the left side: its own predicates AND the bitmap test in one predicate program, ballots -> one compaction pass over all left columns (fused_filter_frame).
// No pairs, no gathers.  Needs a right key range a bitmap can cover (<= 2^34 keys and <= 256 x the right rows); otherwise the per-node join runs.
static bool fused_semi_anti_frame(Plan& plan, const IRN& jn, FramePtr& out, std::string* why) {
  auto no = [&](const char* m) { if (why) *why = m; return false; };
  const AE *lkx = nullptr, *rkx = nullptr;
  if (const char* bad = single_key_join(plan, jn, true, join_materialise_mode() == 0 ? "disabled (PLX_JOIN_MATERIALISE=0)" : nullptr, lkx, rkx)) return no(bad);
  std::vector<int> lpreds, rpreds;
  const int lsrc = peel_filters(plan, jn.input, lpreds), rsrc = peel_filters(plan, jn.input_right, rpreds);
  FramePtr L = exec_node(plan, lsrc), R = exec_node(plan, rsrc);
  plan.memo[lsrc] = L; plan.memo[rsrc] = R;
  const int lki = L->find(lkx->name), rki = R->find(rkx->name);
  if (lki < 0 || rki < 0) return no("join key column not found");
  const int kdt = L->cols[lki]->dtype;
  if (kdt != R->cols[rki]->dtype || !dtype_is_int(kdt) || kdt == PLX_U64) return no("join key is not a signed / narrow integer column pair of one dtype");
  int64_t mn = 0, mx = 0;
  const bool have = R->height > 0 && R->cols[rki]->values && ops::int_range(R->cols[rki], &mn, &mx);
  MemberBitmap members;
  if (!members.cover(have, mn, mx, R->height)) return no("right key range too wide for a membership bitmap");
  const uint64_t range = members.range;
  uint64_t rows_in = 0;
  if (have) {
    Compiler cb(plan, *R);
    try {
      cb.pred = and_predicates(cb, rpreds);
      cb.key = cb.load(rki);
      cb.finish();
    } catch (const Unsupported& u) { if (why) *why = "right side: " + u.why; return false; }
    members.build(&cb);
    rows_in = members.rows_in();
  } else members.build(nullptr);
  const MemberTest mt{lki, members.bits->as<unsigned long long>(), mn, range, jn.how == PLX_JOIN_ANTI};
  std::string fwhy, fd;
  if (!filter_phrase(plan, lpreds, L, out, &fwhy, nullptr, &mt, "", fd)) { if (why) *why = "left side: " + fwhy; return false; }
  plan.desc += std::string("FusedSemiAntiJoin{") + (jn.how == PLX_JOIN_ANTI ? "anti" : "semi") + ", right rows=" + std::to_string(rows_in) + "/" + std::to_string(R->height) + " -> membership bitmap range=" +
               std::to_string(range) + ", left rows=" + std::to_string(L->height) + " filtered by " + fd + "}; ";
  return true;
}

static FramePtr exec_join(Plan& plan, const IRN& n) {
  if (!(plan.flags & PLX_PLAN_NO_FUSION) && (n.how == PLX_JOIN_SEMI || n.how == PLX_JOIN_ANTI)) {
    FramePtr out; std::string why;
    if (fused_semi_anti_frame(plan, n, out, &why)) return out;
    plan.desc += "(semi / anti join not fused: " + why + ") ";
  } else if (!(plan.flags & PLX_PLAN_NO_FUSION)) {
    FramePtr out; std::string why;
    if (fused_join_frame(plan, n, nullptr, out, &why)) return out;
    if (why != "small inputs") plan.desc += "(join not fused: " + why + ") ";
  }
  FramePtr left = exec_node(plan, n.input);
  FramePtr right = exec_node(plan, n.input_right);
  PLX_REQUIRE(!n.keys.empty() && n.keys.size() == n.keys_right.size(), PLX_ERR_INVALID, "join: left_on / right_on length mismatch");
  ColumnPtr lk, rk;
  std::vector<ColumnPtr> lraw, rraw;   // multi-column keys: the key columns as they are
  std::string wide_why;                // ... and why they are not packed into one Int64 (empty: they are)
  std::string packed_desc;
  if (n.keys.size() == 1) {
    lk = broadcast(eval(plan, n.keys[0], *left, nullptr), left->height);
    rk = broadcast(eval(plan, n.keys_right[0], *right, nullptr), right->height);
  } else {
    // Multi-column keys: the reference row-encodes them (polars-row via join/mod.rs:367-370).  Integer / boolean
    // keys are instead packed into ONE Int64 using the joint value range of both sides:
    //   packed = sum_j (key_j - min_j) * stride_j,  stride_j = prod_{i>j} (max_i - min_i + 1)
    // A null in any key column makes the packed key null, i.e. the row never matches (nulls_equal = false).
    // Keys that do not pack -- a Float32 / Float64 / UInt64 part, one column beyond 63 bits, a product of the spans beyond 9e18 -- take the wide route instead: a table
    // of row ids whose key words are compared column by column at the build rows (join::join_indices_wide).  PLX_JOIN_WIDE_KEYS: 2 = every multi-column key, 0 = never.
    const int wide_mode = join_wide_keys_mode();
    std::vector<ColumnPtr> lks, rks;
    std::vector<int64_t> mins, spans;
    auto no_pack = [&](const std::string& error, const std::string& why) { PLX_REQUIRE(wide_mode != 0, PLX_ERR_UNSUPPORTED, error); wide_why = why; };
    if (wide_mode == 2) wide_why = "PLX_JOIN_WIDE_KEYS=2";
    for (size_t j = 0; j < n.keys.size(); j++) {
      ColumnPtr a = broadcast(eval(plan, n.keys[j], *left, nullptr), left->height);
      ColumnPtr b = broadcast(eval(plan, n.keys_right[j], *right, nullptr), right->height);
      PLX_REQUIRE(a->dtype == b->dtype, PLX_ERR_INVALID, "join keys have different dtypes");
      lraw.push_back(a); rraw.push_back(b);
      if (!wide_why.empty()) continue;
      if (!(dtype_is_int(a->dtype) || a->dtype == PLX_BOOL)) { no_pack("multi-column join keys must be integer / boolean / dictionary codes on this path", std::string(a->dtype == PLX_F32 ? "Float32" : a->dtype == PLX_F64 ? "Float64" : dtype_name(a->dtype)) + " key part"); continue; }
      if (a->dtype == PLX_U64) { no_pack("multi-column join on UInt64 keys", "UInt64 key part"); continue; }
      if (a->dtype != PLX_I64) { a = ops::cast(a, PLX_I64); b = ops::cast(b, PLX_I64); }
      int64_t amn = 0, amx = 0, bmn = 0, bmx = 0;
      const bool ha = ops::int_range(a, &amn, &amx), hb = ops::int_range(b, &bmn, &bmx);
      int64_t mn = ha ? amn : bmn, mx = ha ? amx : bmx;
      if (ha && hb) { mn = std::min(amn, bmn); mx = std::max(amx, bmx); }
      if (!ha && !hb) { mn = 0; mx = 0; }
      if (!((double)mx - (double)mn < 9e18)) { no_pack("multi-column join keys span more than 63 bits", "key part " + std::to_string(j) + " spans more than 63 bits"); continue; }
      lks.push_back(a); rks.push_back(b); mins.push_back(mn); spans.push_back(mx - mn + 1);
    }
    if (wide_why.empty()) {
      double total = 1;
      for (int64_t sp : spans) total *= (double)sp;
      if (!(total < 9.0e18)) no_pack("multi-column join keys do not pack into 63 bits (needs row encoding)", "key spans do not pack into 63 bits");
    }
    auto pack = [&](std::vector<ColumnPtr>& ks) {
      ColumnPtr acc;
      int64_t stride = 1;
      for (size_t j = ks.size(); j-- > 0;) {
        plx_scalar s; s.i = mins[j];
        ColumnPtr t = ops::arith_scalar(PLX_SUB, ks[j], s, false);
        if (stride != 1) { plx_scalar m; m.i = stride; t = ops::arith_scalar(PLX_MUL, t, m, false); }
        acc = acc ? ops::arith(PLX_ADD, acc, t) : t;
        stride *= spans[j];
      }
      return acc;
    };
    if (wide_why.empty()) {
      lk = pack(lks); rk = pack(rks);
      packed_desc = "packed " + std::to_string(n.keys.size()) + " key columns into Int64; ";
    }
  }
  ColumnPtr li, ri;
  std::string d;
  bool dup_build_keys = false;
  int64_t unmatched_build = 0;         // full join: the pairs (no probe row, build row) at the end of the pair list
  const bool full = n.how == PLX_JOIN_FULL, right_join = n.how == PLX_JOIN_RIGHT;
  const bool coalesce = n.coalesce == 1 || (n.coalesce == 0 && !full);      // plx_ir.coalesce: 0 = the kind's default (full joins keep both keys)
  if (!wide_why.empty()) join::join_indices_wide(n.how, lraw, rraw, li, ri, &d, &dup_build_keys, &unmatched_build, wide_why);
  else join::join_indices(n.how, lk, rk, li, ri, &d, &dup_build_keys, &unmatched_build);
  d = packed_desc + d;
  if (n.maintain_order != PLX_JOIN_ORDER_NONE && n.how != PLX_JOIN_SEMI && n.how != PLX_JOIN_ANTI) {
    // join_indices emits at scanned offsets: probe order; its chains (duplicate build keys) are newest first.  It builds on the right unless the left side is not the larger one of an
    // inner / full join, or the join is a right join (always built on the left).  A full join's unmatched build rows follow the probe-ordered pairs.
    const bool probe_is_left = n.how == PLX_JOIN_LEFT || (!right_join && left->height > right->height);
    join::PairProps props; props.probe_ordered = true; props.runs_ordered = !dup_build_keys;
    if (full) props.build_tail = unmatched_build;
    std::string od;
    join::order_pairs(n.maintain_order, probe_is_left, props, probe_is_left ? li : ri, probe_is_left ? ri : li, &od);
    d += ", " + od;
  }
  if (n.how == PLX_JOIN_SEMI || n.how == PLX_JOIN_ANTI) {
    // left columns only, left order (single_keys_semi_anti.rs; _finish_join is not involved)
    plan.desc += "Join{" + d + ", gather x" + std::to_string(left->cols.size()) + "}; ";
    auto out = std::make_shared<Frame>();
    out->height = li->len; out->names = left->names;
    for (auto& c : left->cols) out->cols.push_back(ops::gather(c, li));
    return out;
  }
  static const char* const how_names[] = {"inner", "left", "semi", "anti", "full", "right"};
  plan.desc += "Join{" + d + ", how=" + how_names[n.how] + (n.coalesce == 0 ? "" : coalesce ? ", coalesce=true" : ", coalesce=false") + ", gather x" + std::to_string(left->cols.size() + right->cols.size()) + "}; ";
  // _finish_join (polars-ops/src/frame/join/general.rs:17-49): left columns, then right columns; name clashes on the right get the suffix.  A key pair of two plain columns
  // coalesces (plx_ir.coalesce; include/polars_amd.h): inner / left joins drop the right key, a right join drops the left key, a full join keeps the left key column filled
  // from whichever side has the row and drops the right key.  Without coalescing every column of both sides stays.
  std::vector<std::pair<std::string, std::string>> plain_keys;   // (left name, right name) of the key pairs made of two plain columns
  for (size_t j = 0; j < n.keys.size(); j++) {
    const AE* lkx = plain_column(plan, n.keys[j]);
    const AE* rkx = plain_column(plan, n.keys_right[j]);
    if (lkx && rkx) plain_keys.push_back({lkx->name, rkx->name});
  }
  auto out = std::make_shared<Frame>();
  out->height = li->len;
  for (size_t i = 0; i < left->cols.size(); i++) {
    const auto key = std::find_if(plain_keys.begin(), plain_keys.end(), [&](const std::pair<std::string, std::string>& k) { return k.first == left->names[i]; });
    if (coalesce && right_join && key != plain_keys.end()) continue;                     // the right key column carries the key
    out->names.push_back(left->names[i]);
    if (coalesce && full && key != plain_keys.end()) {
      const int rki = right->find(key->second);
      PLX_REQUIRE(rki >= 0, PLX_ERR_NOT_FOUND, "column not found: " + key->second);
      out->cols.push_back(join::coalesce_keys(left->cols[i], right->cols[rki], li, ri));
    } else out->cols.push_back(ops::gather(left->cols[i], li));
  }
  for (size_t i = 0; i < right->cols.size(); i++) {
    if (coalesce && !right_join && std::find_if(plain_keys.begin(), plain_keys.end(), [&](const std::pair<std::string, std::string>& k) { return k.second == right->names[i]; }) != plain_keys.end())
      continue;                                                                          // coalesced into the left key column
    std::string name = right->names[i];
    if (out->find(name) >= 0) name += n.suffix;
    out->names.push_back(name);
    out->cols.push_back(ops::gather(right->cols[i], ri));
  }
  return out;
}

// PLX_IR_JOIN_ASOF: the keys evaluated as exec_join does, one index column from asof::match, the frame by the column rules of a left join.  The left columns are the
// input's own: every left row appears once, in its place.
static FramePtr exec_join_asof(Plan& plan, const IRN& n) {
  FramePtr left = exec_node(plan, n.input);
  FramePtr right = exec_node(plan, n.input_right);
  std::vector<ColumnPtr> lby, rby;
  ColumnPtr lon, ron;
  for (size_t j = 0; j < n.keys.size(); j++) {
    ColumnPtr a = broadcast(eval(plan, n.keys[j], *left, nullptr), left->height);
    ColumnPtr b = broadcast(eval(plan, n.keys_right[j], *right, nullptr), right->height);
    if (j + 1 == n.keys.size()) { lon = a; ron = b; } else { lby.push_back(a); rby.push_back(b); }
  }
  flush_node_notes(plan);
  plx_scalar tol{};
  const plx_scalar* tolerance = nullptr;
  if (n.predicate >= 0) {
    const AE& t = plan.ae[n.predicate];
    const bool on_float = asof::dtype_is_float(lon->dtype);
    PLX_REQUIRE(on_float == dtype_is_float(t.dtype), PLX_ERR_INVALID,
                std::string("join_asof: a ") + dtype_name(t.dtype) + " tolerance against `on` of dtype " + dtype_name(lon->dtype) + "; the tolerance is a literal of the `on` dtype's family");
    if (on_float) tol.f64 = t.dtype == PLX_F32 ? (double)t.lit.f32 : t.lit.f64; else tol.u = t.lit.u;
    tolerance = &tol;
  }
  std::string d;
  ColumnPtr ri = asof::match(n.how, lby, rby, lon, ron, tolerance, &d);
  const bool coalesce = n.coalesce != 2;      // plx_ir.coalesce: the default of an as-of join is a left join's
  std::set<std::string> merged;               // the right columns of the key pairs made of two plain columns
  for (size_t j = 0; coalesce && j < n.keys.size(); j++) {
    const AE* lkx = plain_column(plan, n.keys[j]);
    const AE* rkx = plain_column(plan, n.keys_right[j]);
    if (lkx && rkx) merged.insert(rkx->name);
  }
  auto out = std::make_shared<Frame>();
  out->height = left->height;
  out->names = left->names;
  out->cols = left->cols;
  size_t gathered = 0;
  for (size_t i = 0; i < right->cols.size(); i++) {
    if (merged.count(right->names[i])) continue;
    std::string name = right->names[i];
    if (out->find(name) >= 0) name += n.suffix;
    out->names.push_back(name);
    out->cols.push_back(ops::gather(right->cols[i], ri));
    gathered++;
  }
  plan.desc += "JoinAsof{" + d + ", gather x" + std::to_string(gathered) + "}; ";
  return out;
}

// IR::Sort (+ a Slice directly above it: only the first offset+len rows of the order are produced, top-k)
static FramePtr exec_sort(Plan& plan, const IRN& n, int64_t limit) {
  FramePtr in = exec_node(plan, n.input);
  PLX_REQUIRE(!n.keys.empty(), PLX_ERR_INVALID, "sort needs at least one key");
  std::vector<sort::SortKey> keys;
  for (size_t j = 0; j < n.keys.size(); j++) {
    sort::SortKey sk;
    sk.col = broadcast(eval(plan, n.keys[j], *in, nullptr), in->height);
    sk.descending = n.sort_descending.size() > j && n.sort_descending[j];
    sk.nulls_last = n.sort_nulls_last.size() > j && n.sort_nulls_last[j];
    keys.push_back(sk);
  }
  std::string d;
  ColumnPtr idx = sort::sort_indices(keys, limit, &d);
  auto out = std::make_shared<Frame>();
  out->names = in->names; out->height = idx->len;
  for (auto& c : in->cols) out->cols.push_back(ops::gather(c, idx));
  plan.desc += "Sort{" + d + ", gather x" + std::to_string(in->cols.size()) + "}; ";
  return out;
}

static FramePtr exec_slice(Plan& plan, const IRN& n) {
  PLX_REQUIRE(n.slice_len >= 0, PLX_ERR_INVALID, "slice length must be non-negative");
  FramePtr in;
  const IRN* src = n.input >= 0 ? &plan.ir[n.input] : nullptr;
  PLX_REQUIRE(src, PLX_ERR_INVALID, "slice without an input");
  if (src->kind == PLX_IR_SORT && n.slice_offset >= 0 && n.slice_offset <= (int64_t)1 << 40 && n.slice_len <= (int64_t)1 << 40) {
    check_cancel();
    in = exec_sort(plan, *src, n.slice_offset + n.slice_len);
  } else in = exec_node(plan, n.input);
  // slice_offsets (polars-core/src/utils/mod.rs:340-358): negative offsets count from the end, both ends clamped
  const int64_t h = in->height;
  int64_t start = n.slice_offset < 0 ? n.slice_offset + h : n.slice_offset;
  int64_t stop = start + n.slice_len;   // offsets are far below the i64 range here (h < 2^32, len checked by the caller)
  start = std::min(std::max<int64_t>(start, 0), h); stop = std::min(std::max<int64_t>(stop, 0), h);
  if (start == 0 && stop == h) { plan.desc += "Slice{no-op}; "; return in; }
  auto out = std::make_shared<Frame>();
  out->names = in->names; out->height = stop - start;
  for (auto& c : in->cols) out->cols.push_back(ops::slice_copy(c, start, stop - start));
  plan.desc += "Slice{" + std::to_string(start) + ", " + std::to_string(stop - start) + "}; ";
  return out;
}

// IR::Distinct: the rows that are distinct over the subset, in the input's row order -- one stable sort of the subset, a row-order mask of the rows to keep
// (sort::distinct_rows), every column of the frame through the filter's compaction
static FramePtr exec_distinct(Plan& plan, const IRN& n) {
  FramePtr in = exec_node(plan, n.input);
  std::vector<ColumnPtr> keys;
  std::string subset;
  for (int e : n.keys) {
    keys.push_back(broadcast(eval(plan, e, *in, nullptr), in->height));
    subset += (subset.empty() ? "" : ", ") + output_name(plan, e);
  }
  flush_node_notes(plan);
  std::string sd;
  ColumnPtr mask = sort::distinct_rows(keys, n.how, nullptr, &sd);      // (no count here: preparing the mask counts it)
  auto pm = ops::prepare_mask(mask);
  const int64_t kept = ops::prepared_rows(*pm);
  auto out = std::make_shared<Frame>();
  out->names = in->names;
  out->height = kept;
  for (auto& c : in->cols) out->cols.push_back(ops::filter_prepared(c, *pm));
  plan.desc += std::string("Distinct{subset=[") + subset + "], keep=" + distinct::keep_name(distinct::keep_served(n.how)) + (n.how == PLX_UNIQUE_ANY ? " (asked: any)" : "") + ", order=rows, " + sd +
               ", kept=" + std::to_string(kept) + " of " + std::to_string(in->height) + "}; ";
  return out;
}

static FramePtr exec_node(Plan& plan, int node_id) {
  check_cancel();
  PLX_REQUIRE(node_id >= 0 && node_id < (int)plan.ir.size(), PLX_ERR_INVALID, "bad IR node index");
  const IRN& n = plan.ir[node_id];
  const bool fuse = !(plan.flags & PLX_PLAN_NO_FUSION);
  { auto it = plan.memo.find(node_id); if (it != plan.memo.end()) return it->second; }
  switch (n.kind) {
    case PLX_IR_SCAN: return get_frame(n.frame);
    case PLX_IR_FILTER: return exec_filter(plan, n);
    case PLX_IR_HSTACK: return exec_select(plan, n, true);
    case PLX_IR_SELECT: {
      if (fuse && n.input >= 0 && plan.ir[n.input].kind == PLX_IR_JOIN) {
        // projection pushed into the join: only the columns the select reads are gathered at the pairs
        std::set<std::string> want;
        for (int e : n.exprs) collect_columns(plan, e, want);
        FramePtr j; std::string why;
        // (a join the fused pipelines never take is left to exec_join, which names the reason once)
        if (!join_takes_per_node_route(plan.ir[n.input])) {
          if (fused_join_frame(plan, plan.ir[n.input], &want, j, &why)) return exec_select(plan, n, false, j);
          if (why != "small inputs") plan.desc += "(join not fused: " + why + ") ";
        }
      }
      if (fuse) {
        std::vector<int> preds;
        int src_node = peel_filters(plan, n.input, preds);
        bool aggs_only = !n.exprs.empty();
        for (int e : n.exprs) aggs_only = aggs_only && contains_agg(plan, e) && !contains_column_outside_agg(plan, e);
        if (aggs_only) {
          FramePtr src = exec_node(plan, src_node);
          FramePtr out; std::string why;
          if (fused_select(plan, n, preds, src, out, nullptr, nullptr, &why, false)) return out;
          plan.desc += "(not fused: " + why + ") ";
          plan.memo[src_node] = src;      // the per-node path below runs the same subtree: once is enough
        }
      }
      return exec_select(plan, n, false);
    }
    case PLX_IR_GROUPBY: {
      if (fuse && n.input >= 0 && plan.ir[n.input].kind == PLX_IR_JOIN) {
        FramePtr out; std::string why;
        if (fused_join_groupby(plan, n, out, &why)) return out;
        // The in-place form needs a group to be a build row and the aggregates to read the probe side.  Anything else -- aggregates over build-side columns
        // (sum(l_quantity * ps_supplycost)), group keys without the join key or from the probe side -- takes the PAIR form: the fused join -> frame pipeline
        // restricted to the columns the group-by reads (filters fused into build scan and candidate selection, pairs, one gather per side), then the ordinary fused
        // group-by over those joined columns.  The reference has no such restriction either (JoinExec -> GroupByExec, executors/join.rs:41-121, group_by.rs:60-98).
        std::set<std::string> want;
        for (int e : n.keys) collect_columns(plan, e, want);
        for (int e : n.exprs) collect_columns(plan, e, want);
        const size_t mark = plan.desc.size();
        FramePtr joined; std::string why2;
        uint64_t build_rows = 0;
        int build_side = 0;
        if (fused_join_frame(plan, plan.ir[n.input], &want, joined, &why2, &build_rows, &build_side)) {
          std::vector<int> no_preds;
          std::string why3;
          const std::string jd = plan.desc.substr(mark);
          plan.desc.resize(mark);
          const size_t mark2 = plan.desc.size();
          // group keys that are all functions of the build row (the join key or plain build-side columns): at most one group per surviving build row
          {
            const IRN& jn = plan.ir[n.input];
            FramePtr bf = exec_node(plan, peel_filters_node(plan, build_side ? jn.input_right : jn.input));
            bool of_build = !n.keys.empty();
            const AE* lk = plain_column(plan, jn.keys[0]);      // (a plain column: fused_join_frame took the join)
            for (int e : n.keys) {
              const AE* x = plain_column(plan, e);
              of_build = of_build && x && (x->name == lk->name || bf->find(x->name) >= 0 || (x->name.size() > jn.suffix.size() && bf->find(x->name.substr(0, x->name.size() - jn.suffix.size())) >= 0));
            }
            plan.group_hint = of_build ? (double)std::max<uint64_t>(build_rows, 1) : 0.0;
          }
          const bool gb_fused = fused_groupby(plan, n, no_preds, joined, out, nullptr, nullptr, &why3, false);
          plan.group_hint = 0;
          if (!gb_fused) out = exec_groupby_materialised(plan, n, joined);
          const std::string gd = plan.desc.substr(mark2);
          plan.desc.resize(mark2);
          plan.desc += "FusedJoinGroupBy{pair form (in-place form: " + why + "): " + jd + "then " + gd + "}; ";
          return out;
        }
        plan.desc += "(join+group_by not fused: " + why + (why2 == "small inputs" ? "" : "; pair form: " + why2) + ") ";
      }
      if (fuse) {
        std::vector<int> preds;
        int src_node = peel_filters(plan, n.input, preds);
        FramePtr src = exec_node(plan, src_node);
        FramePtr out; std::string why;
        if (fused_groupby(plan, n, preds, src, out, nullptr, nullptr, &why, false)) return out;
        plan.desc += "(not fused: " + why + ") ";
        plan.memo[src_node] = src;
      }
      FramePtr in = exec_node(plan, n.input);
      return exec_groupby_materialised(plan, n, in);
    }
    case PLX_IR_JOIN: return exec_join(plan, n);
    case PLX_IR_SORT: return exec_sort(plan, n, -1);
    case PLX_IR_SLICE: return exec_slice(plan, n);
    case PLX_IR_DISTINCT: return exec_distinct(plan, n);
    case PLX_IR_JOIN_ASOF: return exec_join_asof(plan, n);
    default: fail(PLX_ERR_UNSUPPORTED, "IR node kind " + std::to_string(n.kind) + " is outside the hot path (run it on the CPU engine)");
  }
}

FramePtr execute(Plan& plan, int root) {
  plan.desc.clear();
  t_node_notes.clear();
  return exec_node(plan, root);
}

bool describe_join_fusion(Plan& plan, int root, std::vector<Shape>* shapes, std::string* why_not) {
  const IRN& n = plan.ir.at(root);
  FramePtr out;
  return fused_join_groupby(plan, n, out, why_not, shapes, true);
}

bool describe_filter_fusion(Plan& plan, int root, Shape* shape, std::string* why_not) {
  const IRN& n = plan.ir.at(root);
  PLX_REQUIRE(n.kind == PLX_IR_FILTER, PLX_ERR_INVALID, "describe_filter_fusion: root is not a Filter");
  std::vector<int> preds;
  const int src_node = peel_filters(plan, n.input, preds);
  preds.push_back(n.predicate);
  PLX_REQUIRE(plan.ir[src_node].kind == PLX_IR_SCAN, PLX_ERR_UNSUPPORTED, "describe_filter_fusion: source must be a scan");
  FramePtr src = get_frame(plan.ir[src_node].frame);
  Compiler c(plan, *src);
  try {
    c.pred = and_predicates(c, preds);
    c.finish();
  } catch (const Unsupported& u) { if (why_not) *why_not = u.why; return false; }
  if (shape) *shape = c.shape;
  return true;
}

bool describe_fusion(Plan& plan, int root, Shape* shape, int* static_id, std::string* why_not) {
  const IRN& n = plan.ir.at(root);
  std::vector<int> preds;
  int src_node = peel_filters(plan, n.input, preds);
  PLX_REQUIRE(plan.ir[src_node].kind == PLX_IR_SCAN, PLX_ERR_UNSUPPORTED, "describe_fusion: source must be a scan");
  FramePtr src = get_frame(plan.ir[src_node].frame);
  FramePtr out;
  if (n.kind == PLX_IR_SELECT) return fused_select(plan, n, preds, src, out, shape, static_id, why_not, true);
  if (n.kind == PLX_IR_GROUPBY) return fused_groupby(plan, n, preds, src, out, shape, static_id, why_not, true);
  if (why_not) *why_not = "root is neither Select nor GroupBy";
  return false;
}

bool dump_program_json(Plan& plan, int root, std::string* json, std::string* why_not) {
  ProgramDump d;
  t_program_dump = &d;
  bool ok = false;
  try {
    const IRN& n = plan.ir.at(root);
    if (n.kind == PLX_IR_GROUPBY && n.input >= 0 && plan.ir[n.input].kind == PLX_IR_JOIN) ok = describe_join_fusion(plan, root, nullptr, why_not);
    else ok = describe_fusion(plan, root, nullptr, nullptr, why_not);
  } catch (...) { t_program_dump = nullptr; throw; }
  t_program_dump = nullptr;
  if (ok && json) *json = d.json;
  return ok && !d.json.empty();
}

// generic grouped aggregation over already materialised columns: builds a LOAD-only
// program and reuses the fused table kernels.
static void groupby_cells(const std::vector<ColumnPtr>& keys, const std::vector<ColumnPtr>& values, const std::vector<int>& aggs, bool maintain_order,
                          std::vector<ColumnPtr>& out_keys, std::vector<ColumnPtr>& out_aggs, std::string* desc, const std::vector<int>* ddof) {
  PLX_REQUIRE(!keys.empty(), PLX_ERR_INVALID, "group_by needs at least one key");
  PLX_REQUIRE(values.size() == aggs.size(), PLX_ERR_INVALID, "group_by: values/aggs length mismatch");
  PLX_REQUIRE(!ddof || ddof->size() == aggs.size(), PLX_ERR_INVALID, "group_by: ddof/aggs length mismatch");
  for (size_t i = 0; i < aggs.size(); i++) {
    if (aggs[i] != PLX_AGG_VAR && aggs[i] != PLX_AGG_STD) continue;
    PLX_REQUIRE(!ddof || ((*ddof)[i] >= 0 && (*ddof)[i] <= 255), PLX_ERR_INVALID, "group_by: ddof must be 0..255");
    PLX_REQUIRE(values[i], PLX_ERR_INVALID, "group_by: var / std need a value column");
    if (!(dtype_is_int(values[i]->dtype) || dtype_is_float(values[i]->dtype))) fail(PLX_ERR_UNSUPPORTED, std::string("group_by: var / std of a ") + dtype_name(values[i]->dtype) + " column: numeric columns only");
  }
  // synthesise a plan: frame of k0..kn, v0..vm; GroupBy over a scan
  auto f = std::make_shared<Frame>();
  f->height = keys[0]->len;
  Plan p;
  IRN scan; scan.kind = PLX_IR_SCAN; p.ir.push_back(scan);
  IRN gb; gb.kind = PLX_IR_GROUPBY; gb.input = 0; gb.maintain_order = maintain_order ? 1 : 0;
  for (size_t i = 0; i < keys.size(); i++) {
    PLX_REQUIRE(keys[i]->len == f->height, PLX_ERR_SHAPE, "group_by: key length mismatch");
    f->names.push_back("__k" + std::to_string(i)); f->cols.push_back(keys[i]);
    AE c; c.kind = PLX_AE_COLUMN; c.name = f->names.back(); p.ae.push_back(c);
    gb.keys.push_back((int)p.ae.size() - 1);
  }
  for (size_t i = 0; i < values.size(); i++) {
    AE a;
    if (aggs[i] == PLX_AGG_LEN || !values[i]) { a.kind = PLX_AE_LEN; }
    else {
      PLX_REQUIRE(values[i]->len == f->height, PLX_ERR_SHAPE, "group_by: value length mismatch");
      f->names.push_back("__v" + std::to_string(i)); f->cols.push_back(values[i]);
      AE c; c.kind = PLX_AE_COLUMN; c.name = f->names.back(); p.ae.push_back(c);
      a.kind = PLX_AE_AGG; a.op = aggs[i]; a.lhs = (int)p.ae.size() - 1;
      if (aggs[i] == PLX_AGG_VAR || aggs[i] == PLX_AGG_STD) a.lit.u = ddof ? (uint64_t)(*ddof)[i] : 1;
    }
    p.ae.push_back(a);
    AE al; al.kind = PLX_AE_ALIAS; al.lhs = (int)p.ae.size() - 1; al.name = "__a" + std::to_string(i); p.ae.push_back(al);
    gb.exprs.push_back((int)p.ae.size() - 1);
  }
  p.ir.push_back(gb);
  FramePtr out; std::string why;
  std::vector<int> preds;
  if (!fused_groupby(p, p.ir[1], preds, f, out, nullptr, nullptr, &why, false)) {
    // f32 / bool value columns: aggregate them through an f64 / integer view
    std::vector<ColumnPtr> v2 = values; bool changed = false;
    for (size_t i = 0; i < v2.size(); i++) if (v2[i] && v2[i]->dtype == PLX_F32) { v2[i] = ops::cast(v2[i], PLX_F64); changed = true; }
    std::vector<ColumnPtr> k2 = keys;
    for (auto& kc : k2) if (kc->dtype == PLX_F32) { kc = ops::cast(kc, PLX_F64); changed = true; }
    if (!changed) fail(PLX_ERR_UNSUPPORTED, "group_by: " + why);
    std::vector<ColumnPtr> ok, oa;
    groupby_cells(k2, v2, aggs, maintain_order, ok, oa, desc, ddof);
    for (size_t i = 0; i < keys.size(); i++) out_keys.push_back(keys[i]->dtype == PLX_F32 ? ops::cast(ok[i], PLX_F32) : ok[i]);
    for (size_t i = 0; i < values.size(); i++) {
      bool was_f32 = values[i] && values[i]->dtype == PLX_F32;
      // f32 sums / means / min / max report f32 (reduce/mean.rs:29-80)
      out_aggs.push_back(was_f32 && oa[i]->dtype == PLX_F64 && aggs[i] != PLX_AGG_COUNT ? ops::cast(oa[i], PLX_F32) : oa[i]);
    }
    return;
  }
  if (desc) *desc = p.desc;
  for (size_t i = 0; i < keys.size(); i++) out_keys.push_back(out->cols[i]);
  for (size_t i = 0; i < values.size(); i++) out_aggs.push_back(out->cols[keys.size() + i]);
}

// The aggregates that are sums of cells run through the synthesised fused plan (groupby_cells), which also owns the keys, the group order and maintain_order.  The
// order statistics and the distinct counts run over sorted segments, one sort per distinct source column whichever of the two read it, and are placed into the
// group frame by the rank of every group's key.
void groupby_columns(const std::vector<ColumnPtr>& keys, const std::vector<ColumnPtr>& values, const std::vector<int>& aggs, bool maintain_order,
                     std::vector<ColumnPtr>& out_keys, std::vector<ColumnPtr>& out_aggs, std::string* desc, const std::vector<AggParams>* params) {
  PLX_REQUIRE(values.size() == aggs.size(), PLX_ERR_INVALID, "group_by: values/aggs length mismatch");
  PLX_REQUIRE(!params || params->size() == aggs.size(), PLX_ERR_INVALID, "group_by: params/aggs length mismatch");
  std::vector<ColumnPtr> cell_values;
  std::vector<int> cell_aggs, cell_ddof, cell_of(aggs.size(), -1);
  // one entry per distinct source column of the aggregates that leave the cell list, in the order they first appear
  struct Source { ColumnPtr col; std::vector<size_t> quantiles, distincts; };
  std::vector<Source> sources;
  auto source_of = [&](const ColumnPtr& c) -> Source& {
    for (Source& sc : sources) if (sc.col == c) return sc;
    sources.push_back(Source{c, {}, {}});
    return sources.back();
  };
  size_t n_quantiles = 0, n_distincts = 0;
  for (size_t i = 0; i < aggs.size(); i++) {
    const AggParams ap = params ? (*params)[i] : AggParams{};
    if (aggs[i] == PLX_AGG_QUANTILE) {
      PLX_REQUIRE(quantile::q_ok(ap.q), PLX_ERR_INVALID, "group_by: quantile q must be a real number in [0, 1], got " + std::to_string(ap.q));
      PLX_REQUIRE(quantile::interpolation_ok(ap.interpolation), PLX_ERR_INVALID, "group_by: interpolation " + std::to_string(ap.interpolation) + " is no plx_quantile_interpolation (0..4)");
      PLX_REQUIRE(values[i], PLX_ERR_INVALID, "group_by: median / quantile need a value column");
      if (!(dtype_is_int(values[i]->dtype) || dtype_is_float(values[i]->dtype))) fail(PLX_ERR_UNSUPPORTED, std::string("group_by: median / quantile of a ") + dtype_name(values[i]->dtype) + " column: integer and float columns only");
      source_of(values[i]).quantiles.push_back(i);
      n_quantiles++;
      continue;
    }
    if (aggs[i] == PLX_AGG_N_UNIQUE) {
      PLX_REQUIRE(values[i], PLX_ERR_INVALID, "group_by: n_unique needs a value column");
      if (!(dtype_is_int(values[i]->dtype) || dtype_is_float(values[i]->dtype) || values[i]->dtype == PLX_BOOL)) fail(PLX_ERR_UNSUPPORTED, std::string("group_by: n_unique of a ") + dtype_name(values[i]->dtype) + " column: integer, float and Boolean columns only");
      source_of(values[i]).distincts.push_back(i);
      n_distincts++;
      continue;
    }
    cell_of[i] = (int)cell_aggs.size();
    cell_values.push_back(values[i]); cell_aggs.push_back(aggs[i]); cell_ddof.push_back(ap.ddof);
  }
  if (sources.empty()) { groupby_cells(keys, values, aggs, maintain_order, out_keys, out_aggs, desc, &cell_ddof); return; }
  if (cell_aggs.empty()) { cell_values.push_back(nullptr); cell_aggs.push_back(PLX_AGG_LEN); cell_ddof.push_back(1); }      // the group frame has to exist
  std::vector<ColumnPtr> cells;
  std::string d;
  groupby_cells(keys, cell_values, cell_aggs, maintain_order, out_keys, cells, &d, &cell_ddof);
  const int64_t G = out_keys[0]->len;
  for (auto& kc : keys) PLX_REQUIRE(kc->len == keys[0]->len, PLX_ERR_SHAPE, "group_by: key length mismatch");
  // rank of every group's key among the groups, in the order the segments come out in
  ColumnPtr place;
  if (G > 1) {
    std::vector<sort::SortKey> gk;
    for (const ColumnPtr& kc : out_keys) { sort::SortKey s; s.col = kc; s.nulls_last = true; gk.push_back(s); }
    place = sort::invert_permutation(sort::sort_indices(gk, -1, nullptr));
  }
  std::vector<ColumnPtr> placed(aggs.size());
  std::string q_sorts, d_sorts;
  int q_sources = 0, d_sources = 0;
  for (const Source& sc : sources) {
    PLX_REQUIRE(sc.col->len == keys[0]->len, PLX_ERR_SHAPE, "group_by: value length mismatch");
    const sort::SortedSegments seg = sort::sort_segments(keys, sc.col, G);
    if (!sc.quantiles.empty()) {
      std::vector<sort::QuantileSpec> specs;
      for (size_t j : sc.quantiles) { const AggParams ap = params ? (*params)[j] : AggParams{}; specs.push_back({ap.q, ap.interpolation}); }
      std::vector<ColumnPtr> cols = sort::segment_quantiles(seg, specs);
      for (size_t m = 0; m < sc.quantiles.size(); m++) placed[sc.quantiles[m]] = place ? ops::gather(cols[m], place) : cols[m];
      q_sorts += (q_sources ? " + " : "") + seg.sort_desc;
    }
    if (!sc.distincts.empty()) {
      ColumnPtr counts = sort::segment_distinct(seg);
      if (place) counts = ops::gather(counts, place);
      for (size_t j : sc.distincts) placed[j] = counts;
      d_sorts += (d_sources ? " + " : "") + (sc.quantiles.empty() ? seg.sort_desc : "shares the sort of source " + std::to_string(q_sources));
      d_sources++;
    }
    if (!sc.quantiles.empty()) q_sources++;
  }
  for (size_t i = 0; i < aggs.size(); i++) out_aggs.push_back(cell_of[i] >= 0 ? cells[(size_t)cell_of[i]] : placed[i]);
  const std::string tail = ", groups=" + std::to_string(G) + ", sources=";
  if (n_quantiles) d += "quantile[sorted segments: " + q_sorts + tail + std::to_string(q_sources) + ", outputs=" + std::to_string(n_quantiles) + "]";
  if (n_distincts) d += std::string(n_quantiles ? "; " : "") + "n_unique[sorted segments: " + d_sorts + tail + std::to_string(d_sources) + ", outputs=" + std::to_string(n_distincts) + "]";
  if (desc) *desc = d;
}

}  // namespace engine
}  // namespace plx
