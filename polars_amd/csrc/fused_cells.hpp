// fused_cells.hpp -- the cell plan of the LDS-table aggregate scans: which aggregates of a program own a cell of the workgroup's table and which are derived from another
// aggregate's cell when the workgroup finishes (fused_sinks.hpp LdsCellSink; DESIGN.md 4.11 "Shared cells").  Pure functions of the program shape and of bounds the
// engine knows about its inputs, shared by the host (engine.cpp lds_table, jit.cpp) and the compiled kernels, where the plan is a compile-time constant.
//
//   rule A  AGG_LEN and ONE AGG_SUM_I share a packed u64 cell, count << shift | sum.  The sum's source slot is written only by the OP_LOAD of a non-nullable
//           integer input and by in-place integer steps with constants (the affine decode of an encoded shadow), so every selected row is valid and the count of the
//           rows IS the count of the values; 0 <= v <= hi is known, and with R an upper bound on the rows one workgroup adds to its table
//           bits(R) + bits(R * hi) <= 64: neither field can overflow into the other.  shift = bits(R * hi) is a run-time parameter of the sink.
//   rule B  an AGG_SUM_F whose source is OP_I2F of a slot that an AGG_SUM_I aggregates (a mean of an integer column beside its sum) holds no cell: it is the
//           integer cell converted once.  Legal when n_rows * max(|lo|, |hi|) < 2^53: every partial sum is then an integer a double holds exactly, so the f64
//           atomics it replaces were exact too and the result keeps its bits.  Taken only from the cell rule A packed: a source that is nullable, an expression, unbounded or
//           negative, or a program without its AGG_LEN, keeps every cell it had.
// Neither rule applies: the plan is the identity, one cell per aggregate in program order.
#pragma once
#include "fused.hpp"

namespace plx {
namespace fused {

// what the engine knows about the value an aggregate's source slot holds in every selected row: lo <= v <= hi (known[k] = 0: nothing)
struct AggFacts {
  uint8_t known[kMaxAggs];
  int64_t lo[kMaxAggs], hi[kMaxAggs];
  uint64_t wg_rows;      // R: upper bound on the rows one workgroup feeds its table (kernels_fused.hip lds_agg_wg_rows)
  uint64_t n_rows;
};
struct CellPlan {
  uint8_t n_cells;                // LDS cells per group
  uint8_t packed;                 // the AGG_SUM_I whose cell also carries the row count (rule A), kNone: none
  uint8_t packed_len;             // the AGG_LEN that reads it
  uint8_t shift;                  // run-time: count << shift | sum (no part of the code)
  uint8_t cell[kMaxAggs];         // the cell aggregate k adds to, or is read from
  uint8_t from[kMaxAggs];         // kNone: k owns its cell; else the aggregate whose cell holds its value
  uint8_t owner[kMaxAggs];        // cell -> the aggregate that owns it
};
// the structural part of a plan as one word (template parameter of the sink, part of the JIT source and cache key): packed | packed_len << 8 | derived mask << 16;
// 0xffff = the identity
constexpr uint32_t kIdentityCells = 0xffffu;
PLX_HD constexpr uint32_t cell_plan_code(uint8_t packed, uint8_t packed_len, uint32_t derived) { return (uint32_t)packed | ((uint32_t)packed_len << 8) | (derived << 16); }

PLX_HD constexpr int bits_u64(uint64_t x) { int b = 0; while (x) { b++; x >>= 1; } return b; }

// the input behind an integer sum's source slot, when the slot's only writers are the OP_LOAD of ONE non-nullable integer input (its first writer) and in-place
// OP_MUL_I / OP_ADD_I steps whose other operand was last written by an OP_CONST; else -1
PLX_HD constexpr int affine_source_input(const Shape& sh, uint8_t slot) {
  int input = -1;
  for (int pc = 0; pc < sh.n_ops; pc++) {
    const Op op = sh.ops[pc];
    if (op.code == OP_NOP || op.dst != slot) continue;
    if (op.code == OP_LOAD) {
      if (input >= 0 || op.a >= sh.n_inputs || sh.in_nullable[op.a]) return -1;
      const uint8_t dt = sh.in_dtype[op.a];
      if (dt < 1 || dt > 8) return -1;      // PLX_I8 .. PLX_U64
      input = op.a;
      continue;
    }
    if (input < 0 || (op.code != OP_MUL_I && op.code != OP_ADD_I) || op.a != slot || op.b == slot) return -1;
    int def = -1;
    for (int q = 0; q < pc; q++) if (sh.ops[q].code != OP_NOP && sh.ops[q].dst == op.b) def = q;
    if (def < 0 || sh.ops[def].code != OP_CONST) return -1;
  }
  return input;
}
// the AGG_SUM_I that aggregates the integer slot behind SUM_F aggregate k (rule B's structure), or kNone
PLX_HD constexpr uint8_t i2f_sum_source(const Shape& sh, int k) {
  if (k >= sh.n_aggs || sh.aggs[k].kind != AGG_SUM_F) return kNone;
  const uint8_t d = sh.aggs[k].src;
  int def = -1;
  for (int pc = 0; pc < sh.n_ops; pc++) if (sh.ops[pc].code != OP_NOP && sh.ops[pc].dst == d) def = pc;
  if (def < 0 || sh.ops[def].code != OP_I2F || sh.ops[def].a == d) return kNone;
  const uint8_t s = sh.ops[def].a;
  for (int pc = def + 1; pc < sh.n_ops; pc++) if (sh.ops[pc].code != OP_NOP && sh.ops[pc].dst == s) return kNone;      // the sum reads a later value
  if (affine_source_input(sh, s) < 0) return kNone;
  for (int j = 0; j < sh.n_aggs; j++) if (sh.aggs[j].kind == AGG_SUM_I && sh.aggs[j].src == s) return (uint8_t)j;
  return kNone;
}

// a code -> the layout of the cells.  Codes come from plan_cells / full_cell_plan_code only.
PLX_HD constexpr CellPlan cell_plan_from_code(const Shape& sh, uint32_t code) {
  CellPlan p{};
  p.packed = kNone; p.packed_len = kNone; p.shift = 0;
  for (int k = 0; k < kMaxAggs; k++) { p.cell[k] = 0; p.from[k] = kNone; p.owner[k] = 0; }
  if ((code & 0xffffu) != kIdentityCells) {
    p.packed = (uint8_t)(code & 0xffu); p.packed_len = (uint8_t)((code >> 8) & 0xffu);
    p.from[p.packed_len] = p.packed;
  }
  for (int k = 0; k < sh.n_aggs; k++) if ((code >> (16 + k)) & 1u) p.from[k] = i2f_sum_source(sh, k);
  uint8_t n = 0;
  for (int k = 0; k < sh.n_aggs; k++) if (p.from[k] == kNone) { p.cell[k] = n; p.owner[n] = (uint8_t)k; n++; }
  for (int k = 0; k < sh.n_aggs; k++) if (p.from[k] != kNone) p.cell[k] = p.cell[p.from[k]];
  p.n_cells = n;
  return p;
}
PLX_HD constexpr uint32_t cell_plan_code(const CellPlan& p, const Shape& sh) {
  uint32_t derived = 0;
  for (int k = 0; k < sh.n_aggs; k++) if (p.from[k] != kNone && k != p.packed_len) derived |= 1u << k;
  return p.packed == kNone ? (kIdentityCells | (derived << 16)) : cell_plan_code(p.packed, p.packed_len, derived);
}
PLX_HD constexpr bool cell_plan_is_identity(const CellPlan& p, const Shape& sh) { return p.n_cells == sh.n_aggs; }

// does |v| * n stay below 2^53 for every v in [lo, hi]?
PLX_HD constexpr bool exact_f64_sum(int64_t lo, int64_t hi, uint64_t n_rows) {
  const uint64_t a = lo < 0 ? (uint64_t)0 - (uint64_t)lo : (uint64_t)lo, b = hi < 0 ? (uint64_t)0 - (uint64_t)hi : (uint64_t)hi;
  const uint64_t m = a > b ? a : b;
  if (m == 0 || n_rows == 0) return true;
  const uint64_t lim = 1ull << 53;
  return m < lim && n_rows <= (lim - 1) / m;      // n * m <= 2^53 - 1
}
// rule A's bound, and the shift it gives: bits(R) + bits(R * hi) <= 64
PLX_HD constexpr int packed_shift(uint64_t wg_rows, int64_t hi) {
  if (hi < 0 || wg_rows == 0) return -1;
  const uint64_t h = (uint64_t)hi;
  if (h != 0 && wg_rows > ~0ull / h) return -1;
  const int s = bits_u64(wg_rows * h);
  return bits_u64(wg_rows) + s <= 64 ? s : -1;
}

// the packed word: what one row adds, and what the folded word holds
PLX_HD constexpr uint64_t packed_row(uint32_t shift, uint64_t v) { return (1ull << shift) + v; }
PLX_HD constexpr uint64_t packed_count(uint64_t word, uint32_t shift) { return word >> shift; }
PLX_HD constexpr uint64_t packed_sum(uint64_t word, uint32_t shift) { return word & ((1ull << shift) - 1ull); }

// Shape + facts -> plan
PLX_HD constexpr CellPlan plan_cells(const Shape& sh, const AggFacts& f) {
  uint8_t packed = kNone, packed_len = kNone;
  int shift = 0;
  int len = -1, n_len = 0;
  for (int k = 0; k < sh.n_aggs; k++) if (sh.aggs[k].kind == AGG_LEN) { if (len < 0) len = k; n_len++; }
  if (n_len == 1) {
    for (int k = 0; k < sh.n_aggs && packed == kNone; k++) {
      if (sh.aggs[k].kind != AGG_SUM_I || !f.known[k] || f.lo[k] < 0 || affine_source_input(sh, sh.aggs[k].src) < 0) continue;
      const int s = packed_shift(f.wg_rows, f.hi[k]);
      if (s < 0) continue;
      packed = (uint8_t)k; packed_len = (uint8_t)len; shift = s;
    }
  }
  uint32_t derived = 0;
  for (int k = 0; k < sh.n_aggs; k++) {
    const uint8_t j = i2f_sum_source(sh, k);
    if (j == kNone || j != packed || !exact_f64_sum(f.lo[j], f.hi[j], f.n_rows)) continue;      // (the packed cell only: its source is non-nullable, bounded and not negative)
    derived |= 1u << k;
  }
  CellPlan p = cell_plan_from_code(sh, packed == kNone ? (kIdentityCells | (derived << 16)) : cell_plan_code(packed, packed_len, derived));
  p.shift = (uint8_t)shift;
  return p;
}
// the plan of a shape when every bound holds: what the ahead-of-time kernels with shared cells are compiled for
PLX_HD constexpr uint32_t full_cell_plan_code(const Shape& sh) {
  AggFacts f{};
  for (int k = 0; k < kMaxAggs; k++) { f.known[k] = 1; f.lo[k] = 0; f.hi[k] = 1; }
  f.wg_rows = 1; f.n_rows = 1;
  return cell_plan_code(plan_cells(sh, f), sh);
}

// The interval of the value `slot` holds after the program, from the interval [lo, hi] of the input behind it (affine_source_input(sh, slot) >= 0) and the program's
// constants; false when a step may wrap.
inline bool affine_source_interval(const Shape& sh, const Args& a, uint8_t slot, int64_t* lo, int64_t* hi) {
  for (int pc = 0; pc < sh.n_ops; pc++) {
    const Op op = sh.ops[pc];
    if (op.code == OP_NOP || op.dst != slot || op.code == OP_LOAD) continue;
    int def = -1;
    for (int q = 0; q < pc; q++) if (sh.ops[q].code != OP_NOP && sh.ops[q].dst == op.b) def = q;
    if (def < 0) return false;
    const int64_t c = (int64_t)a.imm[def];
    int64_t x = 0, y = 0;
    if (op.code == OP_MUL_I) { if (__builtin_mul_overflow(*lo, c, &x) || __builtin_mul_overflow(*hi, c, &y)) return false; }
    else if (op.code == OP_ADD_I) { if (__builtin_add_overflow(*lo, c, &x) || __builtin_add_overflow(*hi, c, &y)) return false; }
    else return false;
    *lo = x < y ? x : y; *hi = x < y ? y : x;
  }
  return true;
}

}  // namespace fused
}  // namespace plx
