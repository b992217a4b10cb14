// shared_cells_main.cpp -- stand-alone driver of the cell plan of the LDS-table scans (polars_amd/csrc/fused_cells.hpp: plan_cells, the packed word) with a host twin
// of the sink that runs it (polars_amd/csrc/fused_sinks.hpp LdsCellSink: init / consume / finish over C copies of every cell), built with
// -fsanitize=address,undefined by the tests.  (TEST INFRASTRUCTURE: never linked into libpolars_amd.so.)
//
// The twin keeps the sink's table layout, tbl[(g * NC + cell) * C + copy] in a heap block of exactly that size, adds what consume adds (one packed word per row for
// the shared cell, nothing for a derived aggregate, f64 / i64 additions for the others), folds the copies into copy 0 and unpacks as finish does.  What it is checked
// against shares nothing with the packing: one direct sum per group and aggregate.
//   (1) the plan of the two encoded Q1 shapes: 5 cells for 7 aggregates, the count and the mean's sum read from the quantity's cell
//   (2) both field maxima at once: 65535 rows of the value (2^48 - 1) / 65535 fill a 16-bit count field and a 48-bit sum field with ones
//   (3) u8 codes all 255 and u16 codes all 65535 at the LARGEST R the rule admits for them (every lane adds its rows as one batch: integer addition regrouped),
//       hi = 0 (shift 0, a count of 2^64 - 1), hi = 1, one row
//   (4) random groups and values, 16 / 8 / 1 copies, a group that receives nothing: counts and integer sums equal, the derived f64 cell has the BITS of the sequential
//       f64 sum it replaces, the other f64 cells the bits of the same additions in the same order
//   (5) the thresholds of the two rules, from plan_cells itself
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../polars_amd/csrc/fused_cells.hpp"
#include "../../polars_amd/csrc/fused_shapes.hpp"

using namespace plx::fused;

static long long bad = 0, checked = 0;
static void expect(bool ok, const char* what, unsigned long long got, unsigned long long want) {
  checked++;
  if (!ok && bad++ < 20) fprintf(stderr, "%s: got %llu (0x%llx), want %llu (0x%llx)\n", what, got, got, want, want);
}
static uint64_t f2u(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }
static double u2f(uint64_t u) { double x; memcpy(&x, &u, 8); return x; }

// ---- the twin ----------------------------------------------------------------------------------------------------------------------------
struct Twin {
  Shape sh; CellPlan pl; int G, C;
  uint64_t* tbl;      // exactly G * NC * C words
  Twin(const Shape& s, const CellPlan& p, int g, int c) : sh(s), pl(p), G(g), C(c) {
    tbl = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)G * pl.n_cells * C);
    for (int i = 0; i < G * pl.n_cells * C; i++) tbl[i] = agg_identity(sh.aggs[pl.owner[(i / C) % pl.n_cells]].kind);
  }
  ~Twin() { free(tbl); }
  // one row of lane `lane`: v[k] = the 64-bit pattern of aggregate k's source (as rf.get hands it to the sink)
  void consume(int lane, uint32_t gid, const uint64_t* v, uint64_t times = 1) {
    uint64_t* cells = tbl + (size_t)gid * pl.n_cells * C + (lane & (C - 1));
    for (int k = 0; k < sh.n_aggs; k++) {
      if (pl.from[k] != kNone) continue;
      uint64_t* cell = cells + pl.cell[k] * C;
      if (k == pl.packed) { *cell += packed_row(pl.shift, v[k]) * times; continue; }      // (times: a batch of equal rows, the same additions regrouped -- integer addition only)
      for (uint64_t t = 0; t < times; t++) {
        switch (sh.aggs[k].kind) {
          case AGG_SUM_F: *cell = f2u(u2f(*cell) + u2f(v[k])); break;
          case AGG_LEN: *cell += 1; break;
          default: *cell += v[k]; break;      // AGG_SUM_I
        }
      }
    }
  }
  // -> out[G][n_aggs]
  void finish(std::vector<uint64_t>* out) {
    for (int i = 0; i < G * pl.n_cells; i++) {
      const uint8_t kind = sh.aggs[pl.owner[i % pl.n_cells]].kind;
      uint64_t x = tbl[(size_t)i * C];
      for (int c = 1; c < C; c++) x = kind == AGG_SUM_F ? f2u(u2f(x) + u2f(tbl[(size_t)i * C + c])) : x + tbl[(size_t)i * C + c];
      tbl[(size_t)i * C] = x;
    }
    out->assign((size_t)G * sh.n_aggs, 0);
    for (int i = 0; i < G * sh.n_aggs; i++) {
      const int g = i / sh.n_aggs, k = i % sh.n_aggs;
      uint64_t x = tbl[((size_t)g * pl.n_cells + pl.cell[k]) * C];
      if (pl.packed != kNone && pl.cell[k] == pl.cell[pl.packed]) {
        x = k == pl.packed_len ? packed_count(x, pl.shift) : packed_sum(x, pl.shift);
        if (k != pl.packed && k != pl.packed_len) x = f2u((double)(long long)x);
      } else if (pl.from[k] != kNone) x = f2u((double)(long long)x);
      (*out)[i] = x;
    }
  }
};

// count(0), sum of q (1), sum of an f64 (2), the f64 sum of q behind its mean (3): q is input 0 decoded in place (x stride + base), the f64 input 1
static Shape small_shape(bool nullable = false, bool expression = false, bool count_other = false) {
  Shape s{};
  s.n_inputs = 3; s.n_aggs = 4; s.pred = kNone; s.key = 4;
  s.in_dtype[0] = 5; s.in_dtype[1] = 10; s.in_dtype[2] = 5; s.in_nullable[0] = nullable ? 1 : 0;
  int n = 0;
  s.ops[n++] = mkop(OP_LOAD, 0, 0, 0, 0);
  s.ops[n++] = mkop(OP_LOAD, 1, 1, 0, 0);
  s.ops[n++] = mkop(OP_LOAD, 4, 2, 0, 0);
  s.ops[n++] = mkop(OP_CONST, 5, 0, 0, 0);
  s.ops[n++] = mkop(OP_MUL_I, 0, 0, 5, 0);
  s.ops[n++] = mkop(OP_CONST, 5, 0, 0, 0);
  s.ops[n++] = mkop(OP_ADD_I, 0, 0, expression ? 4 : 5, 0);      // (expression: plus another column, not a constant)
  s.ops[n++] = mkop(OP_I2F, 2, 0, 0, 0);
  s.n_ops = (uint8_t)n;
  s.aggs[0] = Agg{(uint8_t)(count_other ? AGG_COUNT : AGG_LEN), (uint8_t)(count_other ? 4 : 0)};
  s.aggs[1] = Agg{AGG_SUM_I, 0};
  s.aggs[2] = Agg{AGG_SUM_F, 1};
  s.aggs[3] = Agg{AGG_SUM_F, 2};
  return s;
}
static AggFacts facts_for(const Shape& s, int64_t lo, int64_t hi, uint64_t R, uint64_t n) {
  AggFacts f{};
  for (int k = 0; k < s.n_aggs; k++) if (s.aggs[k].kind == AGG_SUM_I) { f.known[k] = 1; f.lo[k] = lo; f.hi[k] = hi; }
  f.wg_rows = R; f.n_rows = n;
  return f;
}

static void q1_plans() {
  for (int id : {(int)SHAPE_Q1_ENCODED, (int)SHAPE_Q1_ENCODED_PRICE}) {
    const Shape s = static_shape(id);
    const CellPlan p = plan_cells(s, facts_for(s, 1, 50, 470000, 600000000));
    expect(p.n_cells == 5, "Q1 cells", p.n_cells, 5);
    expect(p.packed == 1 && p.packed_len == 0 && p.from[0] == 1 && p.from[5] == 1, "Q1 sharing", p.from[5], 1);
    expect(p.shift == bits_u64(470000ull * 50), "Q1 shift", p.shift, bits_u64(470000ull * 50));
    for (int k : {1, 2, 3, 4, 6}) expect(p.from[k] == kNone, "Q1 owners", p.from[k], kNone);
    expect(cell_plan_code(p, s) == full_cell_plan_code(s), "Q1 code", cell_plan_code(p, s), full_cell_plan_code(s));
    const CellPlan q = cell_plan_from_code(s, cell_plan_code(p, s));
    expect(!memcmp(q.cell, p.cell, sizeof p.cell) && !memcmp(q.from, p.from, sizeof p.from) && !memcmp(q.owner, p.owner, sizeof p.owner) && q.n_cells == p.n_cells, "code round trip", 0, 0);
  }
}

static void field_maxima() {
  const Shape s = small_shape();
  const uint64_t R = 65535, hi = ((1ull << 48) - 1) / 65535;      // R * hi = 2^48 - 1
  const CellPlan p = plan_cells(s, facts_for(s, 0, (int64_t)hi, R, R));
  expect(p.n_cells == 2 && p.shift == 48, "maxima: plan", p.n_cells, 2);      // (n * hi = 2^48 - 1 < 2^53: the mean's cell is derived too)
  Twin t(s, p, 1, 16);
  const uint64_t v[4] = {0, hi, f2u(0.5), f2u((double)hi)};
  for (uint64_t i = 0; i < R; i++) t.consume((int)(i % 64), 0, v);
  std::vector<uint64_t> out;
  t.finish(&out);
  expect(t.tbl[0] == ~0ull, "maxima: the folded word is all ones", t.tbl[0], ~0ull);
  expect(out[0] == R, "maxima: count", out[0], R);
  expect(out[1] == R * hi, "maxima: sum", out[1], R * hi);
  expect(out[3] == f2u((double)(R * hi)), "maxima: derived", out[3], f2u((double)(R * hi)));
}

static void code_maxima() {
  Shape s2 = small_shape();
  s2.n_aggs = 2;      // the count and the integer sum alone: whole batches of equal rows are then one multiplication of the packed word
  for (uint64_t hi : {255ull, 65535ull, 0ull, 1ull}) {
    uint64_t lo = 1, top = ~0ull;      // the largest R rule A admits for this hi (the rule is monotone in R)
    while (lo < top) { const uint64_t mid = lo + (top - lo) / 2 + 1; if (packed_shift(mid, (int64_t)hi) >= 0) lo = mid; else top = mid - 1; }
    const uint64_t R = lo;
    expect(packed_shift(R, (int64_t)hi) >= 0 && (R == ~0ull || packed_shift(R + 1, (int64_t)hi) < 0), "largest R", R, 0);
    const CellPlan p = plan_cells(s2, facts_for(s2, 0, (int64_t)hi, R, 1));
    expect(p.packed == 1 && p.n_cells == 1, "code maxima: packed", p.packed, 1);
    Twin t(s2, p, 2, 16);
    const uint64_t v[2] = {0, hi};
    for (int lane = 0; lane < 16; lane++) t.consume(lane, 1, v, R / 16 + (lane == 0 ? R % 16 : 0));      // R rows of the largest value, all in group 1
    std::vector<uint64_t> out;
    t.finish(&out);
    expect(out[0] == 0 && out[1] == 0, "code maxima: the untouched group", out[0], 0);
    expect(out[2] == R, "code maxima: count", out[2], R);
    expect(out[3] == R * hi, "code maxima: sum", out[3], R * hi);
  }
  // one row
  const Shape s = small_shape();
  const CellPlan p = plan_cells(s, facts_for(s, 0, 255, 1, 1));
  Twin t(s, p, 1, 16);
  const uint64_t v[4] = {0, 255, f2u(2.5), f2u(255.0)};
  t.consume(37, 0, v);
  std::vector<uint64_t> out;
  t.finish(&out);
  expect(out[0] == 1 && out[1] == 255 && out[2] == f2u(2.5) && out[3] == f2u(255.0), "one row", out[1], 255);
}

static void random_groups() {
  std::mt19937_64 rng(7);
  const Shape s = small_shape();
  for (int copies : {16, 8, 1}) {
    for (int64_t base : {0ll, 5ll}) {
      const int G = 7;      // group 6 receives nothing
      const uint64_t n = 5000, stride = 3, hi = (uint64_t)base + stride * 255;
      const CellPlan p = plan_cells(s, facts_for(s, base, (int64_t)hi, n, n));
      expect(p.n_cells == 2, "random: cells", p.n_cells, 2);
      Twin t(s, p, G, copies);
      std::vector<uint64_t> cnt(G, 0), sum(G, 0);
      std::vector<std::vector<double>> fs(G, std::vector<double>(16, 0.0)), qs(G, std::vector<double>(16, 0.0));
      for (uint64_t i = 0; i < n; i++) {
        const uint32_t g = (uint32_t)(rng() % 6);
        const uint64_t q = (uint64_t)base + stride * (rng() % 256);
        const double x = (double)(rng() % 100000) / 100.0;
        const int lane = (int)(i % 64);
        const uint64_t v[4] = {0, q, f2u(x), f2u((double)(long long)q)};
        t.consume(lane, g, v);
        cnt[g]++; sum[g] += q; fs[g][lane & (copies - 1)] += x; qs[g][lane & (copies - 1)] += (double)q;
      }
      std::vector<uint64_t> out;
      t.finish(&out);
      for (int g = 0; g < G; g++) {
        double f = fs[g][0], qf = qs[g][0];
        for (int c = 1; c < copies; c++) { f += fs[g][c]; qf += qs[g][c]; }
        expect(out[g * 4 + 0] == cnt[g], "random: count", out[g * 4 + 0], cnt[g]);
        expect(out[g * 4 + 1] == sum[g], "random: sum", out[g * 4 + 1], sum[g]);
        expect(out[g * 4 + 2] == f2u(f), "random: f64 sum, same additions", out[g * 4 + 2], f2u(f));
        expect(out[g * 4 + 3] == f2u(qf), "random: derived cell has the bits of the f64 additions it replaces", out[g * 4 + 3], f2u(qf));
      }
    }
  }
}

static void thresholds() {
  const Shape s = small_shape();
  // rule A: bits(R) + bits(R * hi) = 64 packs, 65 does not
  const uint64_t R = (1ull << 24) - 1;      // 24 bits
  const uint64_t hi64 = ((1ull << 40) - 1) / R, hi65 = (1ull << 40) / R + 1;
  expect(bits_u64(R) + bits_u64(R * hi64) == 64 && bits_u64(R) + bits_u64(R * hi65) == 65, "rule A: the two cases", bits_u64(R * hi65), 41);
  expect(plan_cells(s, facts_for(s, 0, (int64_t)hi64, R, 1)).packed == 1, "rule A at 64", 0, 1);
  expect(plan_cells(s, facts_for(s, 0, (int64_t)hi65, R, 1)).n_cells == 4, "rule A at 65", 0, 1);
  expect(plan_cells(s, facts_for(s, 0, 1, (1ull << 32) - 1, 1)).packed == 1 && plan_cells(s, facts_for(s, 0, 1, 1ull << 32, 1)).n_cells == 4, "rule A: hi = 1, R = 2^32 - 1 | 2^32", 0, 1);
  expect(plan_cells(s, facts_for(s, 0, INT64_MAX, 3, 1)).n_cells == 4, "rule A: R * hi wraps", 0, 1);
  // rule B: n_rows * hi = 2^53 - 1 derives, 2^53 does not (2^53 - 1 = 6361 * 69431 * 20394401)
  const uint64_t n = 6361ull * 69431ull, h = 20394401ull;
  expect(n * h == (1ull << 53) - 1, "rule B: factors", n * h, (1ull << 53) - 1);
  const CellPlan at = plan_cells(s, facts_for(s, 0, (int64_t)h, 1000, n)), past = plan_cells(s, facts_for(s, 0, (int64_t)(1ull << 27), 1000, 1ull << 26));
  expect(at.n_cells == 2 && at.from[3] == 1, "rule B at 2^53 - 1", at.n_cells, 2);
  expect(past.n_cells == 3 && past.packed == 1 && past.from[3] == kNone, "rule B at 2^53: the mean keeps its cell, the count still shares", past.n_cells, 3);
  // the identity
  expect(plan_cells(small_shape(true), facts_for(s, 0, 255, 1000, 1000)).n_cells == 4, "a nullable source", 0, 1);
  expect(plan_cells(s, facts_for(s, -1, 255, 1000, 1000)).n_cells == 4, "a negative lower bound", 0, 1);
  expect(plan_cells(small_shape(false, true), facts_for(s, 0, 255, 1000, 1000)).n_cells == 4, "a source that is an expression", 0, 1);
  expect(plan_cells(small_shape(false, false, true), facts_for(s, 0, 255, 1000, 1000)).n_cells == 4, "a count of another column", 0, 1);
  AggFacts none{}; none.wg_rows = 1000; none.n_rows = 1000;
  expect(plan_cells(s, none).n_cells == 4, "no bound known", 0, 1);
  const CellPlan id = plan_cells(s, none);
  for (int k = 0; k < 4; k++) expect(id.cell[k] == k && id.from[k] == kNone && id.owner[k] == k, "identity layout", id.cell[k], (unsigned)k);
}

int main() {
  q1_plans();
  field_maxima();
  code_maxima();
  random_groups();
  thresholds();
  printf("%lld checks, %lld failed\n", checked, bad);
  return bad ? 1 : 0;
}
