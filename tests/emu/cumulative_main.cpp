// cumulative_main.cpp -- stand-alone driver of the cumulative / ranking arithmetic (polars_amd/csrc/cumulative.hpp: the segmented combine and its identities, the
// mirrored index of reverse, the per-lane pieces of a tile -- fold_thread, wave_step, fold_waves, scan_thread -- and the rank formulas: the one body of
// cum_reduce_kernel, cum_scan_kernel and rank_kernel), built with -fsanitize=address,undefined by the tests.  (TEST INFRASTRUCTURE: never linked into
// libpolars_amd.so.)
//
// The three launches are walked here the way the kernels walk them: tile by tile, lane by lane, the wave scan as log2(64) rounds of wave_step over a copy of the
// wave's registers (what __shfl_up hands every lane), the four wave totals through an array of kWaves entries (the LDS), the tile aggregates scanned by the same
// two routines over their own arrays, recursively above one tile of tiles.  Every buffer -- values, validity words, head-mask words, the permutation, the aggregate
// arrays, prefixes and starts -- is allocated at its exact size, so a read or write past any of them is an ASan report; a signed overflow in a sum is a UBSan one.
//
// What it is checked against is a sequential loop written out here from the contract, not from the header:
//   (1) sizes 0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2 * 2048 + 5, and 2048 * 2048 + 3 once (the aggregates need the recursive level);
//   (2) segment patterns: one partition, every row its own, a partition over three tiles and more, a head on a tile's first / last row, on a wave's lane 0 / lane
//       63 positions, random lengths 1..300; whole column (no mask, no permutation) and permuted (a random interleaving of the partitions);
//   (3) both index directions; sum (wrapping i32, f64 with +inf then -inf and NaN), min (i64 at its bounds), max (f64 ignoring NaN), count; random validity, a null
//       at every head, an all-null partition, null rows carrying a payload that would show;
//   (4) the rank formulas over sorted segments with ties, nulls last, for the five methods, against counting.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>
#include <random>
#include <vector>

#include "../../polars_amd/csrc/cumulative.hpp"

using namespace plx::cumulative;

static long long bad = 0, checked = 0;
static void expect(bool ok, const char* what, double got, double want, long long at) {
  checked++;
  if (!ok && bad++ < 20) fprintf(stderr, "%s: got %.17g, want %.17g (at %lld)\n", what, got, want, at);
}
template <class A> static bool same(A a, A b) {
  if constexpr (std::is_floating_point<A>::value) return (a != a && b != b) || a == b;
  else return a == b;
}
static std::vector<uint64_t> words_of(const std::vector<bool>& bits) {
  std::vector<uint64_t> w((bits.size() + 63) / 64, 0);
  for (size_t i = 0; i < bits.size(); i++) if (bits[i]) w[i >> 6] |= 1ull << (i & 63);
  return w;
}

// ---- the column as the kernels see it ----
template <class A> struct Column {
  int64_t n = 0;
  std::vector<A> x;                // exactly n values
  std::vector<uint64_t> valid;     // exactly ceil(n / 64) words
  std::vector<uint64_t> heads;     // permuted: exactly ceil(n / 64) words over the sorted order
  std::vector<uint32_t> perm;      // permuted: exactly n
  bool permuted = false, reverse = false, count = false;
};
// ColSrc::load, position by position
template <int OP, class A> static void load_lane(const Column<A>& c, int64_t base, Pair<A>* e) {
  for (int j = 0; j < kPerThread; j++) {
    const int64_t p = base + j;
    Pair<A> r = neutral<OP, A>();
    if (p < c.n) {
      const int64_t i = physical_index(p, c.n, c.reverse);
      int64_t row = i;
      if (c.permuted) { row = c.perm[i]; r.f = flag_at(c.heads.data(), i, c.n, c.reverse) ? 1u : 0u; }
      if ((c.valid[row >> 6] >> (row & 63)) & 1) r.v = c.count ? (A)1 : c.x[row];
    }
    e[j] = r;
  }
}
template <int OP, class A> static void store_lane(const Column<A>& c, int64_t base, const Pair<A>* e, std::vector<A>& out) {
  for (int j = 0; j < kPerThread; j++) {
    const int64_t p = base + j;
    if (p >= c.n) continue;
    const int64_t i = physical_index(p, c.n, c.reverse);
    out[c.permuted ? c.perm[i] : i] = e[j].v;
  }
}
// the pair arrays of a level of aggregates
template <class A> struct Pairs { std::vector<uint32_t> f; std::vector<A> v; };
template <int OP, class A> static void load_lane(const Pairs<A>& c, int64_t base, Pair<A>* e) {
  const int64_t n = (int64_t)c.v.size();
  for (int j = 0; j < kPerThread; j++) { const int64_t p = base + j; e[j] = p < n ? Pair<A>{c.v[p], c.f[p]} : neutral<OP, A>(); }
}

// the wave's inclusive scan: every round reads the registers of the round before, as __shfl_up does
template <int OP, class A> static void wave_scan(Pair<A>* t) {
  for (int s = 1; s < kWaveLanes; s <<= 1) {
    Pair<A> prev[kWaveLanes];
    for (int l = 0; l < kWaveLanes; l++) prev[l] = t[l];
    for (int l = 0; l < kWaveLanes; l++) t[l] = wave_step<OP, A>(prev[l], prev[l >= s ? l - s : l], l, s);
  }
}

// launch 1
template <int OP, class A, class Src> static Pairs<A> reduce_tiles(const Src& src, int64_t n) {
  const int64_t tiles = (n + kTile - 1) / kTile;
  Pairs<A> agg;
  agg.f.assign((size_t)tiles, 0); agg.v.assign((size_t)tiles, A());
  for (int64_t tile = 0; tile < tiles; tile++) {
    Pair<A> wave_tot[kWaves];
    for (int w = 0; w < kWaves; w++) {
      Pair<A> t[kWaveLanes];
      for (int l = 0; l < kWaveLanes; l++) {
        Pair<A> e[kPerThread];
        load_lane<OP, A>(src, tile * kTile + (int64_t)(w * kWaveLanes + l) * kPerThread, e);
        t[l] = fold_thread<OP, A>(e);
      }
      wave_scan<OP, A>(t);
      wave_tot[w] = t[kWaveLanes - 1];
    }
    const Pair<A> tot = fold_waves<OP, A>(wave_tot, kWaves);
    agg.f[(size_t)tile] = tot.f; agg.v[(size_t)tile] = tot.v;
  }
  return agg;
}
// launch 3: store(base, e) receives every lane's scanned positions
template <int OP, class A, class Src, class Store> static void scan_tiles(const Src& src, int64_t n, const Pairs<A>* carry, Store&& store) {
  const int64_t tiles = (n + kTile - 1) / kTile;
  for (int64_t tile = 0; tile < tiles; tile++) {
    Pair<A> wave_tot[kWaves], incl[kThreads];
    std::vector<Pair<A>> e((size_t)kThreads * kPerThread);
    for (int w = 0; w < kWaves; w++) {
      for (int l = 0; l < kWaveLanes; l++) {
        const int t = w * kWaveLanes + l;
        load_lane<OP, A>(src, tile * kTile + (int64_t)t * kPerThread, &e[(size_t)t * kPerThread]);
        incl[t] = fold_thread<OP, A>(&e[(size_t)t * kPerThread]);
      }
      wave_scan<OP, A>(&incl[w * kWaveLanes]);
      wave_tot[w] = incl[w * kWaveLanes + kWaveLanes - 1];
    }
    for (int t = 0; t < kThreads; t++) {
      const int w = t / kWaveLanes, l = t % kWaveLanes;
      const Pair<A> excl = l == 0 ? neutral<OP, A>() : incl[t - 1];
      Pair<A> c = neutral<OP, A>();
      if (carry && tile > 0) c = Pair<A>{carry->v[(size_t)tile - 1], carry->f[(size_t)tile - 1]};
      c = combine<OP, A>(combine<OP, A>(c, fold_waves<OP, A>(wave_tot, w)), excl);
      scan_thread<OP, A>(c, &e[(size_t)t * kPerThread]);
      store(tile * kTile + (int64_t)t * kPerThread, &e[(size_t)t * kPerThread]);
    }
  }
}
static int levels_used = 0;
template <int OP, class A> static void scan_pairs(Pairs<A>& p, int level) {      // in place, inclusive
  const int64_t m = (int64_t)p.v.size();
  levels_used = std::max(levels_used, level);
  Pairs<A> out = p;
  auto store = [&](int64_t base, const Pair<A>* e) { for (int j = 0; j < kPerThread; j++) if (base + j < m) { out.v[(size_t)(base + j)] = e[j].v; out.f[(size_t)(base + j)] = e[j].f; } };
  if (m <= kTile) { scan_tiles<OP, A>(p, m, (const Pairs<A>*)nullptr, store); p = out; return; }
  Pairs<A> up = reduce_tiles<OP, A>(p, m);
  scan_pairs<OP, A>(up, level + 1);
  scan_tiles<OP, A>(p, m, &up, store);
  p = out;
}
template <int OP, class A> static std::vector<A> device_scan(const Column<A>& c) {
  std::vector<A> out((size_t)c.n, A());
  if (!c.n) return out;
  Pairs<A> agg = reduce_tiles<OP, A>(c, c.n);
  scan_pairs<OP, A>(agg, 1);
  scan_tiles<OP, A>(c, c.n, &agg, [&](int64_t base, const Pair<A>* e) { store_lane<OP, A>(c, base, e, out); });
  return out;
}

// ---- the sequential loop of the contract ----
// parts: the partitions as row lists in row order; rows of no partition do not exist
template <int OP, class A> static std::vector<A> sequential(const std::vector<A>& x, const std::vector<bool>& ok, const std::vector<std::vector<uint32_t>>& parts, bool reverse, bool count) {
  std::vector<A> out(x.size(), A());
  for (const auto& part : parts) {
    bool any = false;
    A run = A();
    for (size_t q = 0; q < part.size(); q++) {
      const uint32_t r = part[reverse ? part.size() - 1 - q : q];
      if (ok[r]) {
        const A v = count ? (A)1 : x[r];
        if (!any) run = v;
        else if constexpr (OP == PLX_CUM_SUM || OP == PLX_CUM_COUNT) {
          if constexpr (std::is_integral<A>::value) { using U = typename std::make_unsigned<A>::type; run = (A)(U)((U)run + (U)v); } else run = run + v;
        } else if constexpr (std::is_floating_point<A>::value) {
          if (run != run) run = v; else if (v == v) run = OP == PLX_CUM_MIN ? std::min(run, v) : std::max(run, v);
        } else run = OP == PLX_CUM_MIN ? std::min(run, v) : std::max(run, v);
        any = true;
      }
      out[r] = any ? run : A();      // cum_count before the first valid row: 0, which is A()
    }
  }
  return out;
}

// ---- segment patterns: partition lengths that sum to n ----
static std::vector<int64_t> pattern(int which, int64_t n, std::mt19937_64& rng) {
  std::vector<int64_t> len;
  auto rest = [&](int64_t used) { if (used < n) len.push_back(n - used); };
  switch (which) {
    case 0: if (n) len.push_back(n); break;                                              // one partition
    case 1: len.assign((size_t)n, 1); break;                                             // every row its own
    case 2: { int64_t a = std::min<int64_t>(n, 5), b = std::min<int64_t>(n - a, 3 * kTile + 700); if (a) len.push_back(a); if (b) len.push_back(b); rest(a + b); } break;   // the carry through tiles without a head
    case 3: { int64_t a = std::min<int64_t>(n, kTile); if (a) len.push_back(a); rest(a); } break;                               // a head exactly on a tile's first row
    case 4: { int64_t a = std::min<int64_t>(n, kTile - 1), b = std::min<int64_t>(n - a, 1); if (a) len.push_back(a); if (b) len.push_back(b); rest(a + b); } break;   // ... on its last row
    case 5: { int64_t used = 0; while (used < n) { int64_t l = std::min<int64_t>(n - used, (len.size() & 1) ? kPerThread : kPerThread * kWaveLanes - kPerThread); len.push_back(l); used += l; } } break;   // heads on lane 0 and lane 63
    default: { int64_t used = 0; while (used < n) { int64_t l = std::min<int64_t>(n - used, 1 + (int64_t)(rng() % 300)); len.push_back(l); used += l; } } break;
  }
  return len;
}

template <int OP, class A, class Gen>
static void run_case(const char* what, int64_t n, int which, bool permuted, bool reverse, int validity, Gen gen, std::mt19937_64& rng, bool count = false) {
  const std::vector<int64_t> len = permuted ? pattern(which, n, rng) : (n ? std::vector<int64_t>{n} : std::vector<int64_t>{});
  // rows of the partitions: permuted = a random interleaving (each partition's rows ascending), else the rows themselves
  std::vector<uint32_t> owner((size_t)n);
  { size_t at = 0; for (size_t g = 0; g < len.size(); g++) for (int64_t q = 0; q < len[g]; q++) owner[at++] = (uint32_t)g; }
  if (permuted) std::shuffle(owner.begin(), owner.end(), rng);
  std::vector<std::vector<uint32_t>> parts(len.size());
  for (int64_t r = 0; r < n; r++) parts[owner[(size_t)r]].push_back((uint32_t)r);
  Column<A> c;
  c.n = n; c.permuted = permuted; c.reverse = reverse; c.count = count;
  std::vector<bool> ok((size_t)n, true), heads((size_t)n, false);
  for (int64_t r = 0; r < n; r++) ok[(size_t)r] = validity == 0 ? true : validity == 1 ? (rng() % 4 != 0) : true;
  if (validity == 2) for (const auto& p : parts) if (!p.empty()) ok[p[0]] = false;                 // a null at every partition's head
  if (validity == 3 && !parts.empty()) for (uint32_t r : parts[parts.size() / 2]) ok[r] = false;      // a partition that is all null
  c.x.resize((size_t)n);
  for (int64_t r = 0; r < n; r++) c.x[(size_t)r] = gen(r, ok[(size_t)r]);
  c.valid = words_of(ok);
  if (permuted) {
    size_t at = 0;
    c.perm.resize((size_t)n);
    for (const auto& p : parts) { if (!p.empty()) heads[at] = true; for (uint32_t r : p) c.perm[at++] = r; }
    c.heads = words_of(heads);
  }
  const std::vector<A> got = device_scan<OP, A>(c), want = sequential<OP, A>(c.x, ok, parts, reverse, count);
  for (int64_t r = 0; r < n; r++) if (ok[(size_t)r] || count) expect(same<A>(got[(size_t)r], want[(size_t)r]), what, (double)got[(size_t)r], (double)want[(size_t)r], r);
}

// ---- rank ----
static void run_rank(int64_t n, int which, std::mt19937_64& rng) {
  const std::vector<int64_t> len = pattern(which, n, rng);
  // sorted segments: per segment the valid values ascending (few distinct: ties), then its nulls
  std::vector<int> value((size_t)n);
  std::vector<bool> isnull((size_t)n, false), seg_head((size_t)n, false), run_head((size_t)n, false);
  size_t at = 0;
  for (int64_t l : len) {
    const int64_t nulls = l > 1 ? (int64_t)(rng() % 3 == 0) * std::min<int64_t>(l - 1, 1 + (int64_t)(rng() % 3)) : (int64_t)(rng() % 5 == 0);
    std::vector<int> v((size_t)(l - nulls));
    for (auto& z : v) z = (int)(rng() % 7);
    std::sort(v.begin(), v.end());
    for (int64_t q = 0; q < l; q++, at++) {
      isnull[at] = q >= l - nulls;
      value[at] = isnull[at] ? -1 : v[(size_t)q];
      seg_head[at] = q == 0;
      run_head[at] = q == 0 || isnull[at] != isnull[at - 1] || (!isnull[at] && value[at] != value[at - 1]);
    }
  }
  const std::vector<uint64_t> sh = words_of(seg_head), rh = words_of(run_head);
  auto prefix_of = [&](const std::vector<uint64_t>& w) { std::vector<uint64_t> p(w.size() + 1, 0); for (size_t i = 0; i < w.size(); i++) p[i + 1] = p[i] + (uint64_t)__builtin_popcountll(w[i]); return p; };
  auto starts_of = [&](const std::vector<bool>& b) { std::vector<uint32_t> s; for (size_t i = 0; i < b.size(); i++) if (b[i]) s.push_back((uint32_t)i); return s; };
  const std::vector<uint64_t> sp = prefix_of(sh), rp = prefix_of(rh);
  const std::vector<uint32_t> ss = starts_of(seg_head), rs = starts_of(run_head);
  for (int64_t i = 0; i < n; i++) {
    if (isnull[(size_t)i]) continue;
    const RunOf seg = run_of(sp.data(), sh.data(), ss.data(), ss.size(), (uint64_t)n, (uint64_t)i);
    const RunOf run = run_of(rp.data(), rh.data(), rs.data(), rs.size(), (uint64_t)n, (uint64_t)i);
    expect(seg.ok && run.ok && run.start >= seg.start, "rank: run_of", seg.ok, 1, i);
    // counting, from the definitions
    int64_t s0 = i; while (!seg_head[(size_t)s0]) s0--;
    int64_t lo = i; while (lo > s0 && !isnull[(size_t)(lo - 1)] && value[(size_t)(lo - 1)] == value[(size_t)i]) lo--;
    int64_t hi = i; while (hi + 1 < n && !seg_head[(size_t)(hi + 1)] && !isnull[(size_t)(hi + 1)] && value[(size_t)(hi + 1)] == value[(size_t)i]) hi++;
    int64_t dense = 1; for (int64_t q = s0 + 1; q <= i; q++) if (value[(size_t)q] != value[(size_t)(q - 1)]) dense++;
    const uint64_t first = plx::distinct::rank_before(rp.data(), rh.data(), seg.start + 1);
    expect(rank_value(PLX_RANK_ORDINAL, (uint64_t)i, seg.start, run.start, run.end, run.rank, first) == (uint32_t)(i - s0 + 1), "rank ordinal", 0, (double)(i - s0 + 1), i);
    expect(rank_value(PLX_RANK_MIN, (uint64_t)i, seg.start, run.start, run.end, run.rank, first) == (uint32_t)(lo - s0 + 1), "rank min", 0, (double)(lo - s0 + 1), i);
    expect(rank_value(PLX_RANK_MAX, (uint64_t)i, seg.start, run.start, run.end, run.rank, first) == (uint32_t)(hi - s0 + 1), "rank max", 0, (double)(hi - s0 + 1), i);
    expect(rank_value(PLX_RANK_DENSE, (uint64_t)i, seg.start, run.start, run.end, run.rank, first) == (uint32_t)dense, "rank dense", 0, (double)dense, i);
    expect(rank_average(seg.start, run.start, run.end) == 0.5 * (double)((lo - s0 + 1) + (hi - s0 + 1)), "rank average", rank_average(seg.start, run.start, run.end), 0.5 * (double)((lo - s0 + 1) + (hi - s0 + 1)), i);
  }
}

int main() {
  std::mt19937_64 rng(418);
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const int64_t sizes[] = {0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2 * 2048 + 5};
  // generators: a null row carries a payload that would show
  auto gen_i32 = [&](int64_t, bool ok) { return ok ? (int32_t)(rng() % 3 == 0 ? (rng() & 1 ? INT32_MAX : INT32_MIN) : (int32_t)(rng() % 2001) - 1000) : INT32_MAX; };
  auto gen_i64 = [&](int64_t, bool ok) { return ok ? (int64_t)(rng() % 50 == 0 ? (rng() & 1 ? INT64_MAX : INT64_MIN) : (int64_t)(rng() % 2000001) - 1000000) : INT64_MIN; };
  auto gen_f64 = [&](int64_t r, bool ok) { return ok ? (rng() % 40 == 0 ? nan : rng() % 97 == 0 ? (rng() & 1 ? inf : -inf) : rng() % 11 == 0 ? -0.0 : (double)((int64_t)(rng() % 4001) - 2000) / 8.0 + (double)(r % 3)) : nan; };
  auto gen_u32 = [&](int64_t, bool) { return (uint32_t)0xdeadbeefu; };      // cum_count never reads the values
  for (int64_t n : sizes) {
    for (int reverse = 0; reverse < 2; reverse++) {
      for (int validity = 0; validity < 4; validity++) {
        run_case<PLX_CUM_SUM, int32_t>("i32 sum whole", n, 0, false, reverse, validity, gen_i32, rng);
        run_case<PLX_CUM_MAX, double>("f64 max whole", n, 0, false, reverse, validity, gen_f64, rng);
        for (int which = 0; which < 7; which++) {
          if (n < 2 * 2048 && which > 1 && which < 6 && validity > 1) continue;      // the tile patterns matter at the sizes that have tiles
          run_case<PLX_CUM_SUM, int32_t>("i32 sum over", n, which, true, reverse, validity, gen_i32, rng);
          run_case<PLX_CUM_MIN, int64_t>("i64 min over", n, which, true, reverse, validity, gen_i64, rng);
          run_case<PLX_CUM_SUM, double>("f64 sum over", n, which, true, reverse, validity, gen_f64, rng);
          run_case<PLX_CUM_MIN, double>("f64 min over", n, which, true, reverse, validity, gen_f64, rng);
          run_case<PLX_CUM_COUNT, uint32_t>("count over", n, which, true, reverse, validity, gen_u32, rng, true);
        }
      }
    }
    for (int which = 0; which < 7; which++) run_rank(n, which, rng);
  }
  // one size whose tile aggregates need the recursive level: 2048 * 2048 + 3 positions
  const int64_t big = (int64_t)kTile * kTile + 3;
  run_case<PLX_CUM_SUM, int32_t>("i32 sum whole, recursive", big, 0, false, false, 1, gen_i32, rng);
  run_case<PLX_CUM_MAX, int32_t>("i32 max over, recursive", big, 6, true, true, 1, gen_i32, rng);
  expect(levels_used >= 2, "the aggregates' recursive level ran", levels_used, 2, 0);
  // the identities and the mirrored index, by themselves
  expect(identity<PLX_CUM_MIN, int8_t>() == INT8_MAX && identity<PLX_CUM_MAX, int8_t>() == INT8_MIN && identity<PLX_CUM_MAX, uint16_t>() == 0, "integer identities", 0, 0, 0);
  expect(identity<PLX_CUM_MIN, double>() != identity<PLX_CUM_MIN, double>() && identity<PLX_CUM_SUM, double>() == 0.0, "float identities", 0, 0, 0);
  expect(apply<PLX_CUM_SUM, int32_t>(INT32_MAX, 1) == INT32_MIN && apply<PLX_CUM_SUM, int64_t>(INT64_MIN, -1) == INT64_MAX, "sums wrap", 0, 0, 0);
  expect(physical_index(0, 10, true) == 9 && physical_index(9, 10, true) == 0 && physical_index(3, 10, false) == 3, "mirrored index", 0, 0, 0);
  expect(result_dtype(PLX_CUM_SUM, PLX_I8) == PLX_I64 && result_dtype(PLX_CUM_SUM, PLX_BOOL) == PLX_U32 && result_dtype(PLX_CUM_SUM, PLX_F32) == PLX_F32 &&
         result_dtype(PLX_CUM_MIN, PLX_U16) == PLX_U16 && result_dtype(PLX_CUM_COUNT, PLX_F64) == PLX_U32 && result_dtype(7, PLX_I32) == -1 &&
         rank_dtype(PLX_RANK_AVERAGE) == PLX_F64 && rank_dtype(PLX_RANK_ORDINAL) == PLX_U32, "result dtypes", 0, 0, 0);
  expect(op_ok(0) && op_ok(3) && !op_ok(4) && !op_ok(-1) && method_ok(4) && !method_ok(5), "parameter ranges", 0, 0, 0);
  printf("checked=%lld bad=%lld levels=%d\n", checked, bad, levels_used);
  return bad ? 1 : 0;
}
