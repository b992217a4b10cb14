// asof_main.cpp -- walks polars_amd/csrc/asof.hpp the way a lane of asof_search_kernel does (the sample stage over an array of exactly W * ns words, the global
// stage over arrays of exactly W * M words, pick, the tolerance) and holds every result against a direct loop over the candidates.  Built with
// g++ -fsanitize=address,undefined by tests/test_asof_cpu.py: a read past either array is an error, not a wrong answer.  Prints "checked=<n> bad=<n>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../polars_amd/csrc/asof.hpp"

using namespace plx;
using namespace plx::asof;

static long long checked = 0, bad = 0;
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static uint64_t code_i64(int64_t v) { return (uint64_t)v ^ quantile::kSign; }
static int64_t value_i64(uint64_t c) { return (int64_t)(c ^ quantile::kSign); }

// ---- the direct loop: the contract, candidate by candidate ----
template <int W> struct Side { std::vector<Tuple<W>> rows; };      // sorted: candidate order inside every group
struct Dist { bool nan; long double d; };                          // a long double holds 2^64 - 1 and every f64 exactly
static Dist dist_of(bool is_float, uint64_t a, uint64_t b) {
  if (a == b) return Dist{false, 0.0L};
  if (!is_float) { const __int128 x = (__int128)value_i64(a) - (__int128)value_i64(b); return Dist{false, (long double)(x < 0 ? -x : x)}; }
  const double d = std::fabs(quantile::unflip_f64(a) - quantile::unflip_f64(b));
  return Dist{d != d, (long double)d};
}
static bool closer_or_equal(const Dist& a, const Dist& b) { return (a.nan || b.nan) ? b.nan : a.d <= b.d; }
template <int W> static int64_t direct(int how, const Side<W>& s, const Tuple<W>& t, bool is_float, const Tolerance& tol) {
  const bool strict = strict_of(how);
  int64_t best = kNone;
  for (int64_t p = 0; p < (int64_t)s.rows.size(); p++) {
    const Tuple<W>& r = s.rows[p];
    if (!by_equal<W>(r, t)) continue;
    const uint64_t a = r.w[W - 1], b = t.w[W - 1];
    if (strategy_of(how) == PLX_ASOF_BACKWARD) { if (a < b || (!strict && a == b)) best = p; }
    else if (strategy_of(how) == PLX_ASOF_FORWARD) { if (best == kNone && (a > b || (!strict && a == b))) best = p; }
    else { if (strict && a == b) continue; if (best == kNone || closer_or_equal(dist_of(is_float, a, b), dist_of(is_float, s.rows[best].w[W - 1], b))) best = p; }
  }
  if (best == kNone) return kNone;
  const Dist d = dist_of(is_float, s.rows[best].w[W - 1], t.w[W - 1]);
  if (tol.kind == kIntTolerance && !(d.d <= (long double)tol.u)) return kNone;
  if (tol.kind == kFloatTolerance && (d.nan || !(d.d <= (long double)tol.f))) return kNone;
  return best;
}

// ---- one right side, both routes, every strategy, a set of left tuples ----
template <int W> static void run(const Side<W>& s, const std::vector<Tuple<W>>& lefts, bool is_float, const std::vector<Tolerance>& tols) {
  const int64_t M = (int64_t)s.rows.size();
  std::vector<uint64_t> code((size_t)W * M);                                   // exactly the words the kernel may read
  for (int64_t p = 0; p < M; p++) for (int w = 0; w < W; w++) code[(size_t)w * M + p] = s.rows[p].w[w];
  for (int p = 1; p < M; p++) if (tuple_less<W>(s.rows[p], s.rows[p - 1])) { bad++; return; }
  for (int route = 0; route < 2; route++) {
    const int S = route == 0 ? samples_for(W) : 0;
    const int64_t stride = stride_for(M, S), ns = sample_count(M, stride);
    if (S > 0 && (ns > S || (int64_t)W * ns > kLdsWords || (M > 0 && (ns - 1) * stride >= M))) { bad++; continue; }
    std::vector<uint64_t> sample((size_t)W * ns);                              // the LDS array at its exact size
    for (int64_t j = 0; j < ns; j++) for (int w = 0; w < W; w++) sample[(size_t)w * ns + j] = s.rows[j * stride].w[w];
    const Words samples{sample.data(), ns}, codes{code.data(), M};
    for (const Tuple<W>& t : lefts) {
      // the two bounds by themselves, against a count
      int64_t lo_want = 0, hi_want = 0;
      for (int64_t p = 0; p < M; p++) { if (tuple_less<W>(s.rows[p], t)) lo_want++; if (!tuple_less<W>(t, s.rows[p])) hi_want++; }
      checked += 2;
      if (search<W, false>(samples, ns, stride, codes, M, t) != lo_want) bad++;
      if (search<W, true>(samples, ns, stride, codes, M, t) != hi_want) bad++;
      for (int strategy = PLX_ASOF_BACKWARD; strategy <= PLX_ASOF_NEAREST; strategy++)
        for (int strict = 0; strict < 2; strict++)
          for (const Tolerance& tol : tols) {
            const int how = pack_how(strategy, strict != 0);
            const int64_t got = match_row<W>(how, samples, ns, stride, codes, M, t, is_float, tol), want = direct<W>(how, s, t, is_float, tol);
            checked++;
            if (got != want) { if (bad < 10) std::printf("W=%d M=%lld route=%d how=%d tol=%d got=%lld want=%lld\n", W, (long long)M, route, how, tol.kind, (long long)got, (long long)want); bad++; }
          }
    }
  }
}

// integer sides: groups of random size, `on` values with runs of duplicates; the left tuples sit at every edge of the sample geometry
template <int W> static void integer_grid(int64_t M) {
  Side<W> s;
  int64_t group = 0, value = -5;
  for (int64_t p = 0; p < M; p++) {
    if (W > 1 && p > 0 && rnd() % 97 == 0) { group += 1 + (int64_t)(rnd() % 2) * 2; value = -5; }      // groups 2 apart leave absent groups between present ones
    else if (p > 0 && rnd() % 3 != 0) value += 1 + (int64_t)(rnd() % 3) * (int64_t)(rnd() % 3);           // steps of 0 (duplicates), 1, 2, 4: gaps for equidistant pairs
    Tuple<W> t;
    for (int w = 0; w + 1 < W; w++) t.w[w] = code_i64(w == 0 ? group : 7);
    t.w[W - 1] = code_i64(value);
    s.rows.push_back(t);
  }
  const int S = samples_for(W);
  const int64_t stride = stride_for(M, S);
  std::vector<int64_t> at = {0, 1, M - 2, M - 1};
  for (int64_t j = 0; stride > 0 && j * stride < M; j += (j < 4 || j * stride > M - 4 * stride) ? 1 : 1 + (int64_t)(rnd() % 600)) { at.push_back(j * stride - 1); at.push_back(j * stride); at.push_back(j * stride + 1); }
  for (int k = 0; k < 40; k++) at.push_back(M > 0 ? (int64_t)(rnd() % (uint64_t)M) : 0);
  std::vector<Tuple<W>> lefts;
  for (int64_t p : at) {
    if (p < 0 || p >= M) continue;
    for (int64_t dv = -1; dv <= 1; dv++) { Tuple<W> t = s.rows[p]; t.w[W - 1] = code_i64(value_i64(t.w[W - 1]) + dv); lefts.push_back(t); }
    if (W > 1) for (int64_t dg = -1; dg <= 1; dg += 2) { Tuple<W> t = s.rows[p]; t.w[0] = code_i64(value_i64(t.w[0]) + dg); lefts.push_back(t); }      // a neighbouring (often absent) group
  }
  Tuple<W> low, high;
  for (int w = 0; w < W; w++) { low.w[w] = code_i64(w + 1 < W ? (w == 0 ? 0 : 7) : -1000); high.w[w] = code_i64(w + 1 < W ? (w == 0 ? group : 7) : 1000000000); }
  lefts.push_back(low); lefts.push_back(high);
  for (int w = 0; w < W; w++) { low.w[w] = 0; high.w[w] = ~0ull; }
  lefts.push_back(low); lefts.push_back(high);                                // below and above every right tuple
  run<W>(s, lefts, false, {Tolerance{kNoTolerance, 0, 0.0}, Tolerance{kIntTolerance, 0, 0.0}, Tolerance{kIntTolerance, 1, 0.0}});
}

static void value_edges() {
  // Int64 at its ends: the distance is 2^64 - 1
  Side<1> s;
  for (int64_t v : {INT64_MIN, INT64_MIN, (int64_t)-1, (int64_t)0, INT64_MAX, INT64_MAX}) { Tuple<1> t; t.w[0] = code_i64(v); s.rows.push_back(t); }
  std::vector<Tuple<1>> lefts;
  for (int64_t v : {INT64_MIN, INT64_MIN + 1, (int64_t)-1, (int64_t)0, (int64_t)1, INT64_MAX - 1, INT64_MAX}) { Tuple<1> t; t.w[0] = code_i64(v); lefts.push_back(t); }
  run<1>(s, lefts, false, {Tolerance{kNoTolerance, 0, 0.0}, Tolerance{kIntTolerance, ~0ull, 0.0}, Tolerance{kIntTolerance, ~0ull - 1, 0.0}, Tolerance{kIntTolerance, 1ull << 63, 0.0}, Tolerance{kIntTolerance, (1ull << 63) - 1, 0.0}});
  Side<1> ends;
  { Tuple<1> t; t.w[0] = code_i64(INT64_MAX); ends.rows.push_back(t); }
  { std::vector<Tuple<1>> l1; Tuple<1> t; t.w[0] = code_i64(INT64_MIN); l1.push_back(t);
    run<1>(ends, l1, false, {Tolerance{kIntTolerance, ~0ull, 0.0}, Tolerance{kIntTolerance, ~0ull - 1, 0.0}}); }
  // floats: NaN, the infinities, both zeros, duplicates; two groups
  const double inf = INFINITY, nan = NAN;
  const double vals[] = {-inf, -inf, -2.5, -0.0, 0.0, 0.0, 1.0, 1.0, 3.0, inf, inf, nan, nan};
  Side<2> f;
  for (int g = 0; g < 2; g++) for (double v : vals) { if (g == 1 && (v == inf || v != v)) continue; Tuple<2> t; t.w[0] = code_i64(g * 2); t.w[1] = quantile::flip_f64(v); f.rows.push_back(t); }
  std::vector<Tuple<2>> fl;
  for (int g = 0; g < 4; g++) for (double v : {-inf, -3.0, -2.5, -1.25, -0.0, 0.0, 0.5, 1.0, 2.0, 3.0, 1e300, inf, nan}) { Tuple<2> t; t.w[0] = code_i64(g); t.w[1] = quantile::flip_f64(v); fl.push_back(t); }
  run<2>(f, fl, true, {Tolerance{kNoTolerance, 0, 0.0}, Tolerance{kFloatTolerance, 0, 0.0}, Tolerance{kFloatTolerance, 0, 1.0}, Tolerance{kFloatTolerance, 0, inf}});
}

template <int W> static void sizes() {
  const int64_t S = samples_for(W);
  for (int64_t M : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)3, (int64_t)100, S - 1, S, S + 1, 2 * S, 2 * S + 1, 2 * S + 77, 3 * S - 5}) integer_grid<W>(M);
}

int main() {
  // the geometry by itself
  for (int W = 1; W <= kMaxWords; W++) if (samples_for(W) * W > kLdsWords || samples_for(W) < 1024) bad++;
  for (int64_t M : {1, 2, 8191, 8192, 8193, 16384, 16385, 100000, 100000000}) {
    for (int W = 1; W <= kMaxWords; W++) {
      const int64_t S = samples_for(W), stride = stride_for(M, S), ns = sample_count(M, stride);
      checked++;
      if (stride < 1 || ns < 1 || ns > S || (ns - 1) * stride >= M || ns * stride < M) bad++;
      for (int64_t j : {(int64_t)0, (int64_t)1, ns - 1, ns}) {
        if (j < 0 || j > ns) continue;
        const Range r = narrow(j, ns, stride, M);
        checked++;
        if (r.lo < 0 || r.hi > M || r.lo > r.hi || r.hi - r.lo >= stride) bad++;
      }
    }
  }
  for (int how = -1; how < 9; how++) { checked++; if (how_ok(how) != (how == 0 || how == 1 || how == 2 || how == 4 || how == 5 || how == 6)) bad++; }
  sizes<1>();
  sizes<2>();
  sizes<4>();
  integer_grid<8>(2 * samples_for(8) + 9);
  value_edges();
  std::printf("checked=%lld bad=%lld\n", checked, bad);
  return bad ? 1 : 0;
}
