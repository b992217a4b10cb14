// rolling_main.cpp -- stand-alone driver of the shift / diff / rolling arithmetic (polars_amd/csrc/rolling.hpp: the element and its combine, the restart flags of the
// two scans, window_of's case analysis, the per-lane pieces of a scan in both directions, the tile route's region and LDS slots, the shifted-bitmap funnel: the one
// body of the kernels of kernels_rolling.hip), built with -fsanitize=address,undefined by the tests.  (TEST INFRASTRUCTURE: never linked into libpolars_amd.so.)
//
// Both routes are walked here the way the kernels walk them.  Tile halo: tile by tile, the region's kRegionPerThread positions per lane, the forward scan and the
// backward scan (REV) as lane fold, log2(64) rounds of wave_step over a copy of the wave's registers (what __shfl_up / __shfl_down hand every lane), the four wave
// totals through an array of kWaves entries, then P and S into an "LDS" array allocated at EXACTLY the 2 T + w - 1 entries the layout claims, then the combine of
// every output through s_slot / p_slot.  Two scans: cumulative's 2048-position tiles, forward and mirrored, tile aggregates, their scan in chunks with a carried
// element, the tiles with their carry, P and S in arrays of exactly n entries, then the combine.  Every buffer -- values, validity words, head-mask words, the
// permutation, prefix, starts -- is allocated at its exact size, so a read or write past any of them is an ASan report; a signed overflow is a UBSan one.
//
// What it is checked against is a direct loop over every row's clipped window, written out here from the contract, not from the header:
//   (1) sizes 0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2 * 2048 + 5, whole column and a random interleaving of random partitions;
//   (2) at 2 * 2048 + 5 rows the segment patterns of the GPU tests (one, each, three_tiles, tile_first, tile_last, wave_edges, random, and partitions shorter than
//       the window), permuted;
//   (3) w in 1, 2, 3, 63, 64, 65, 2047, 2048 (the tile route's bound) on both routes, and 2049 and 5000 (larger than the column) on the two scans; both center
//       values; min_samples 1 and w; sum (wrapping i64 at its bounds; f64 with infinities that leave the window, +inf with -inf, NaN), min (i32), max (f64 ignoring
//       NaN); random validity, all-null stretches longer than a window, null rows carrying a payload that would show;
//   (4) shifted_word against bit-by-bit shifting at every bit offset and n across words, with and without a bitmap and a fill; shift_source with run_of's bounds.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>
#include <random>
#include <vector>

#include "../../polars_amd/csrc/rolling.hpp"

using namespace plx::rolling;
namespace cum = plx::cumulative;

static long long bad = 0, checked = 0;
static void expect(bool ok, const char* what, double got, double want, long long at, long long w) {
  checked++;
  if (!ok && bad++ < 20) fprintf(stderr, "%s: got %.17g, want %.17g (at %lld, w=%lld)\n", what, got, want, at, w);
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
  std::vector<A> x;                 // exactly n values, in ROW order
  std::vector<uint64_t> valid;      // exactly ceil(n / 64) words, in row order
  bool permuted = false;
  std::vector<uint32_t> perm;       // permuted: exactly n; sorted position -> row
  std::vector<uint64_t> heads;      // permuted: exactly ceil(n / 64) words over the sorted order
  std::vector<uint64_t> prefix;     // permuted: words + 1
  std::vector<uint32_t> starts;     // permuted: exactly n_segs
  std::vector<int64_t> seg_of;      // the truth: the segment's [start, end) of every sorted position (two entries per position)
};
template <class A> static bool segment_of(const Column<A>& c, int64_t i, int64_t* s0, int64_t* s1) {
  if (!c.permuted) { *s0 = 0; *s1 = c.n; return true; }
  const cum::RunOf r = cum::run_of(c.prefix.data(), c.heads.data(), c.starts.data(), (uint64_t)c.starts.size(), (uint64_t)c.n, (uint64_t)i);
  *s0 = (int64_t)r.start; *s1 = (int64_t)r.end;
  return r.ok;
}
// elem_at of kernels_rolling.hip
template <int OP, class A> static Elem<A> elem_at(const Column<A>& c, int64_t pos, int64_t w) {
  Elem<A> e = neutral<OP, A>();
  const int64_t row = c.permuted ? (int64_t)c.perm[(size_t)pos] : pos;
  if ((c.valid[(size_t)(row >> 6)] >> (row & 63)) & 1) { e.v = c.x[(size_t)row]; e.c = 1u; }
  const bool head = c.permuted ? ((c.heads[(size_t)(pos >> 6)] >> (pos & 63)) & 1) != 0 : pos == 0;
  const bool next_head = c.permuted && pos + 1 < c.n && ((c.heads[(size_t)((pos + 1) >> 6)] >> ((pos + 1) & 63)) & 1);
  e.f = (forward_flag(pos, w, head) ? 1u : 0u) | (backward_flag(pos, c.n, w, next_head) ? 2u : 0u);
  return e;
}

// block_scan of kernels_rolling.hip over the registers of all kThreads lanes: every round of the wave scan reads the registers of the round before
template <int OP, class A, int N, bool REV> static Elem<A> block_scan(std::vector<Elem<A>>& e, const Elem<A>& carry_in) {
  Elem<A> incl[kThreads], excl[kThreads], wave_tot[kWaves];
  for (int t = 0; t < kThreads; t++) incl[t] = fold_thread<OP, A, N, REV>(&e[(size_t)t * N]);
  for (int wv = 0; wv < kWaves; wv++) {
    Elem<A>* t = incl + wv * kWaveLanes;
    for (int s = 1; s < kWaveLanes; s <<= 1) {
      Elem<A> prev[kWaveLanes];
      for (int l = 0; l < kWaveLanes; l++) prev[l] = t[l];
      for (int l = 0; l < kWaveLanes; l++) {
        const int from = REV ? (l + s < kWaveLanes ? l + s : l) : (l >= s ? l - s : l);      // (a lane out of range gets its own value back: __shfl_up / __shfl_down)
        t[l] = wave_step<OP, A, REV>(prev[l], prev[from], l, s);
      }
    }
    for (int l = 0; l < kWaveLanes; l++) {
      const int from = REV ? l + 1 : l - 1;
      excl[wv * kWaveLanes + l] = (from < 0 || from >= kWaveLanes) ? neutral<OP, A>() : t[from];
    }
    wave_tot[wv] = t[REV ? 0 : kWaveLanes - 1];
  }
  for (int t = 0; t < kThreads; t++) {
    const Elem<A> carry = combine<OP, A>(combine<OP, A>(carry_in, fold_waves<OP, A, REV>(wave_tot, t / kWaveLanes)), excl[t]);
    scan_thread<OP, A, N, REV>(carry, &e[(size_t)t * N]);
  }
  return combine<OP, A>(carry_in, fold_waves<OP, A, REV>(wave_tot, REV ? -1 : kWaves));
}

template <class A> struct Result { std::vector<A> v; std::vector<uint32_t> c; };      // per ROW: the window's value and its count of valid values

// one row's window from S[a] and P[b]: emit_outputs of kernels_rolling.hip
template <int OP, class A, class Look> static void emit(const Column<A>& c, const Look& look, int64_t i, int64_t w, int64_t h, Result<A>& out) {
  int64_t s0, s1;
  const bool ok = segment_of(c, i, &s0, &s1);
  expect(ok && s0 == c.seg_of[(size_t)i * 2] && s1 == c.seg_of[(size_t)i * 2 + 1], "segment bounds", (double)s0, (double)c.seg_of[(size_t)i * 2], i, w);
  if (!ok) return;
  const Window win = window_of(i, s0, s1, w, h);
  Elem<A> r;
  if (win.use == (kUseP | kUseS)) r = join<OP, A>(look.S(win.a), look.P(win.b));
  else if (win.use == kUseP) r = look.P(win.b);
  else r = look.S(win.a);
  const int64_t row = c.permuted ? (int64_t)c.perm[(size_t)i] : i;
  out.v[(size_t)row] = r.v; out.c[(size_t)row] = r.c;
}

// ---- the tile-halo route ----
template <class A> struct LdsLook {
  const std::vector<A>* v; const std::vector<uint32_t>* c; int64_t t0, w, h;
  Elem<A> at(int k, const char* what, int64_t pos) const { expect(k >= 0 && k < (int)v->size(), what, k, 0, pos, w); return k >= 0 && k < (int)v->size() ? Elem<A>{(*v)[(size_t)k], (*c)[(size_t)k], 0u} : Elem<A>{A(), 0u, 0u}; }
  Elem<A> S(int64_t pos) const { return at(s_slot(pos, t0, w, h), "S slot", pos); }
  Elem<A> P(int64_t pos) const { return at(p_slot(pos, t0, w, h), "P slot", pos); }
};
template <int OP, class A> static Result<A> tile_route(const Column<A>& c, int64_t w, int64_t h) {
  Result<A> out{std::vector<A>((size_t)c.n, A()), std::vector<uint32_t>((size_t)c.n, 0xdeadu)};
  expect(lds_fits(w), "lds_fits", (double)w, 0, 0, w);
  const int T = tile_rows(w);
  const int region_n = T + (int)w - 1;
  expect(T >= 8 && T % 8 == 0 && region_n <= kRegion && 2 * T + w - 1 <= kLdsEntries, "tile geometry", T, 0, 0, w);
  const int64_t n_tiles = (c.n + T - 1) / T;
  for (int64_t tile = 0; tile < n_tiles; tile++) {
    const int64_t t0 = tile * T, r0 = region_start(t0, w, h);
    std::vector<A> lds_v((size_t)(2 * T + w - 1), A());                 // exactly what the layout claims
    std::vector<uint32_t> lds_c((size_t)(2 * T + w - 1), 0xdeadu);
    std::vector<Elem<A>> e((size_t)kRegion), sc((size_t)kRegion);
    for (int rp = 0; rp < kRegion; rp++) {
      const int64_t pos = r0 + rp;
      e[(size_t)rp] = (rp < region_n && pos >= 0 && pos < c.n) ? elem_at<OP, A>(c, pos, w) : neutral<OP, A>();
    }
    for (int rp = 0; rp < kRegion; rp++) { sc[(size_t)rp] = e[(size_t)rp]; sc[(size_t)rp].f = e[(size_t)rp].f & 1u; }
    block_scan<OP, A, kRegionPerThread, false>(sc, neutral<OP, A>());
    for (int rp = 0; rp < region_n; rp++) { const int k = p_slot(r0 + rp, t0, w, h); if (k >= 0) { lds_v[(size_t)k] = sc[(size_t)rp].v; lds_c[(size_t)k] = sc[(size_t)rp].c; } }
    for (int rp = 0; rp < kRegion; rp++) { sc[(size_t)rp] = e[(size_t)rp]; sc[(size_t)rp].f = (e[(size_t)rp].f >> 1) & 1u; }
    block_scan<OP, A, kRegionPerThread, true>(sc, neutral<OP, A>());
    for (int rp = 0; rp < region_n; rp++) { const int k = s_slot(r0 + rp, t0, w, h); if (k >= 0) { lds_v[(size_t)k] = sc[(size_t)rp].v; lds_c[(size_t)k] = sc[(size_t)rp].c; } }
    const LdsLook<A> look{&lds_v, &lds_c, t0, w, h};
    for (int t = 0; t < kThreads; t++) {
      const int o = t * kOutPerThread;
      if (o >= T) continue;
      for (int j = 0; j < kOutPerThread; j++) if (t0 + o + j < c.n) emit<OP, A>(c, look, t0 + o + j, w, h, out);
    }
  }
  return out;
}

// ---- the two-scan route ----
template <class A> struct Scanned { std::vector<A> v; std::vector<uint32_t> c; };
template <int OP, class A> static Scanned<A> scan_elements(const Column<A>& c, int64_t w, bool backward) {
  const int64_t n = c.n, tiles = (n + kScanTile - 1) / kScanTile;
  auto load = [&](int64_t tile, std::vector<Elem<A>>& e) {
    for (int q = 0; q < kScanTile; q++) {
      const int64_t p = tile * kScanTile + q;
      e[(size_t)q] = neutral<OP, A>();
      if (p < n) { e[(size_t)q] = elem_at<OP, A>(c, cum::physical_index(p, n, backward), w); e[(size_t)q].f = backward ? (e[(size_t)q].f >> 1) & 1u : e[(size_t)q].f & 1u; }
    }
  };
  std::vector<Elem<A>> agg((size_t)tiles), e((size_t)kScanTile);
  for (int64_t tile = 0; tile < tiles; tile++) { load(tile, e); agg[(size_t)tile] = block_scan<OP, A, kScanPerThread, false>(e, neutral<OP, A>()); }
  Elem<A> carry = neutral<OP, A>();                     // rolling_aggscan_kernel: chunks of kScanTile aggregates, a carried element
  for (int64_t chunk = 0; chunk < tiles; chunk += kScanTile) {
    for (int q = 0; q < kScanTile; q++) e[(size_t)q] = chunk + q < tiles ? agg[(size_t)(chunk + q)] : neutral<OP, A>();
    carry = block_scan<OP, A, kScanPerThread, false>(e, carry);
    for (int q = 0; q < kScanTile; q++) if (chunk + q < tiles) agg[(size_t)(chunk + q)] = e[(size_t)q];
  }
  Scanned<A> out{std::vector<A>((size_t)n, A()), std::vector<uint32_t>((size_t)n, 0xdeadu)};
  for (int64_t tile = 0; tile < tiles; tile++) {
    load(tile, e);
    block_scan<OP, A, kScanPerThread, false>(e, tile > 0 ? agg[(size_t)(tile - 1)] : neutral<OP, A>());
    for (int q = 0; q < kScanTile; q++) {
      const int64_t p = tile * kScanTile + q;
      if (p < n) { const int64_t i = cum::physical_index(p, n, backward); out.v[(size_t)i] = e[(size_t)q].v; out.c[(size_t)i] = e[(size_t)q].c; }
    }
  }
  return out;
}
template <class A> struct GlobalLook {
  const Scanned<A>*p, *s;
  Elem<A> S(int64_t pos) const { return Elem<A>{s->v.at((size_t)pos), s->c.at((size_t)pos), 0u}; }
  Elem<A> P(int64_t pos) const { return Elem<A>{p->v.at((size_t)pos), p->c.at((size_t)pos), 0u}; }
};
template <int OP, class A> static Result<A> scans_route(const Column<A>& c, int64_t w, int64_t h) {
  Result<A> out{std::vector<A>((size_t)c.n, A()), std::vector<uint32_t>((size_t)c.n, 0xdeadu)};
  const Scanned<A> P = scan_elements<OP, A>(c, w, false), S = scan_elements<OP, A>(c, w, true);
  const GlobalLook<A> look{&P, &S};
  for (int64_t i = 0; i < c.n; i++) emit<OP, A>(c, look, i, w, h, out);
  return out;
}

// ---- the direct loop ----
template <int OP, class A> static Result<A> direct(const Column<A>& c, int64_t w, int64_t h) {
  Result<A> out{std::vector<A>((size_t)c.n, A()), std::vector<uint32_t>((size_t)c.n, 0)};
  for (int64_t i = 0; i < c.n; i++) {
    const int64_t s0 = c.seg_of[(size_t)i * 2], s1 = c.seg_of[(size_t)i * 2 + 1];
    const int64_t a = std::max(i + h - w + 1, s0), b = std::min(i + h, s1 - 1);
    A acc = cum::identity<OP, A>();
    uint32_t cnt = 0;
    for (int64_t p = a; p <= b; p++) {
      const int64_t row = c.permuted ? (int64_t)c.perm[(size_t)p] : p;
      if (!((c.valid[(size_t)(row >> 6)] >> (row & 63)) & 1)) continue;
      acc = cnt == 0 ? c.x[(size_t)row] : cum::apply<OP, A>(acc, c.x[(size_t)row]);
      cnt++;
    }
    const int64_t row = c.permuted ? (int64_t)c.perm[(size_t)i] : i;
    out.v[(size_t)row] = acc; out.c[(size_t)row] = cnt;
  }
  return out;
}
template <int OP, class A> static void compare(const char* what, const Column<A>& c, const Result<A>& got, const Result<A>& want, int64_t w) {
  for (int64_t r = 0; r < c.n; r++) {
    expect(got.c[(size_t)r] == want.c[(size_t)r], what, got.c[(size_t)r], want.c[(size_t)r], r, w);
    for (uint32_t m : {1u, (uint32_t)w}) expect((got.c[(size_t)r] >= m) == (want.c[(size_t)r] >= m), "validity", got.c[(size_t)r], want.c[(size_t)r], r, w);
    if (want.c[(size_t)r]) expect(same<A>(got.v[(size_t)r], want.v[(size_t)r]), what, (double)got.v[(size_t)r], (double)want.v[(size_t)r], r, w);
  }
}

// ---- inputs ----
static const int kTileRows = 2048;
static std::vector<int64_t> lengths(const char* pattern, int64_t n, std::mt19937_64& rng) {
  std::vector<int64_t> out;
  int64_t used = 0;
  auto fill = [&](std::vector<int64_t> first) { for (int64_t ln : first) { ln = std::min(ln, n - used); if (ln > 0) { out.push_back(ln); used += ln; } } if (used < n) out.push_back(n - used); };
  const std::string p = pattern;
  if (p == "one") fill({n});
  else if (p == "each") out.assign((size_t)n, 1);
  else if (p == "three_tiles") fill({5, 3 * kTileRows + 700});
  else if (p == "tile_first") fill({kTileRows});
  else if (p == "tile_last") fill({kTileRows - 1, 1});
  else if (p == "wave_edges") { while (used < n) { const int64_t ln = std::min<int64_t>(n - used, out.size() & 1 ? 8 : 504); out.push_back(ln); used += ln; } }
  else if (p == "short") { while (used < n) { const int64_t ln = std::min<int64_t>(n - used, 1 + (int64_t)(rng() % 40)); out.push_back(ln); used += ln; } }
  else { while (used < n) { const int64_t ln = std::min<int64_t>(n - used, 1 + (int64_t)(rng() % 300)); out.push_back(ln); used += ln; } }
  return out;
}
template <class A, class Gen> static Column<A> make_column(int64_t n, const char* pattern, bool permuted, int validity, std::mt19937_64& rng, Gen&& gen, A payload) {
  Column<A> c;
  c.n = n; c.permuted = permuted;
  c.x.resize((size_t)n);
  std::vector<bool> ok((size_t)n, true);
  for (int64_t i = 0; i < n; i++) c.x[(size_t)i] = gen();
  c.seg_of.assign((size_t)n * 2, 0);
  if (!permuted) {
    for (int64_t i = 0; i < n; i++) { c.seg_of[(size_t)i * 2] = 0; c.seg_of[(size_t)i * 2 + 1] = n; }
  } else {
    const std::vector<int64_t> lens = lengths(pattern, n, rng);
    std::vector<uint32_t> rows((size_t)n);
    std::iota(rows.begin(), rows.end(), 0u);
    // a random interleaving of the partitions: partition g takes a random subset of the rows, in row order
    std::vector<uint32_t> owner;
    for (size_t g = 0; g < lens.size(); g++) owner.insert(owner.end(), (size_t)lens[g], (uint32_t)g);
    std::shuffle(owner.begin(), owner.end(), rng);
    std::vector<std::vector<uint32_t>> by((size_t)lens.size());
    for (int64_t r = 0; r < n; r++) by[owner[(size_t)r]].push_back((uint32_t)r);
    std::vector<bool> heads((size_t)n, false);
    c.perm.clear();
    for (size_t g = 0; g < lens.size(); g++) {
      const int64_t s0 = (int64_t)c.perm.size();
      heads[(size_t)s0] = true;
      c.starts.push_back((uint32_t)s0);
      for (uint32_t r : by[g]) c.perm.push_back(r);
      for (int64_t i = s0; i < (int64_t)c.perm.size(); i++) { c.seg_of[(size_t)i * 2] = s0; c.seg_of[(size_t)i * 2 + 1] = (int64_t)c.perm.size(); }
    }
    c.heads = words_of(heads);
    c.prefix.assign(c.heads.size() + 1, 0);
    for (size_t k = 0; k < c.heads.size(); k++) c.prefix[k + 1] = c.prefix[k] + (uint64_t)__builtin_popcountll(c.heads[k]);
  }
  if (validity == 1) for (int64_t i = 0; i < n; i++) ok[(size_t)i] = rng() % 10 >= 3;
  if (validity == 2) for (int64_t i = 0; i < n; i++) ok[(size_t)i] = (i / 700) % 2 == 0 && rng() % 10 >= 1;      // all-null stretches of 700 rows
  for (int64_t i = 0; i < n; i++) if (!ok[(size_t)i]) c.x[(size_t)i] = payload;                                   // what a null row carries would show
  c.valid = words_of(ok);
  return c;
}

template <int OP, class A, class Gen> static void run_type(const char* name, Gen&& gen, A payload, std::mt19937_64& rng) {
  static const int64_t sizes[] = {0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2 * 2048 + 5};
  static const int64_t windows[] = {1, 2, 3, 63, 64, 65, 2047, 2048, 2049, 5000};
  static const char* patterns[] = {"one", "each", "three_tiles", "tile_first", "tile_last", "wave_edges", "random", "short"};
  auto run = [&](const Column<A>& c) {
    for (int64_t w : windows) for (int center = 0; center < 2; center++) {
      const int64_t h = half_of(w, center != 0);
      const Result<A> want = direct<OP, A>(c, w, h);
      if (w <= kMaxWindow) compare<OP, A>(name, c, tile_route<OP, A>(c, w, h), want, w);
      else expect(!lds_fits(w), "lds_fits above the bound", (double)w, 0, 0, w);
      compare<OP, A>(name, c, scans_route<OP, A>(c, w, h), want, w);
    }
  };
  for (int64_t n : sizes) {
    run(make_column<A>(n, "one", false, (int)(n % 3), rng, gen, payload));
    if (n > 0) run(make_column<A>(n, "random", true, 1, rng, gen, payload));
  }
  for (const char* p : patterns) run(make_column<A>(2 * 2048 + 5, p, true, p[0] == 'o' ? 2 : 1, rng, gen, payload));
}

// ---- shift ----
static void check_shift(std::mt19937_64& rng) {
  for (int64_t n_bits : {1, 2, 63, 64, 65, 127, 128, 130, 200}) {
    std::vector<bool> bits((size_t)n_bits);
    for (int64_t i = 0; i < n_bits; i++) bits[(size_t)i] = rng() % 3 != 0;
    std::vector<uint64_t> words = words_of(bits);
    words.back() |= (n_bits & 63) ? ~0ull << (n_bits & 63) : 0;      // garbage above the last row must not show
    for (int with_valid = 0; with_valid < 2; with_valid++) for (int fill = 0; fill < 2; fill++) for (int64_t n = -(n_bits + 70); n <= n_bits + 70; n++) {
      const int64_t n_words = (n_bits + 63) / 64;
      for (int64_t wi = 0; wi < n_words; wi++) {
        const uint64_t got = shifted_word(with_valid ? words.data() : nullptr, n_bits, wi, n, fill != 0);
        uint64_t want = 0;
        for (int j = 0; j < 64; j++) {
          const int64_t i = wi * 64 + j, src = i - n;
          if (i >= n_bits) continue;
          const bool in = src >= 0 && src < n_bits;
          if (in ? (!with_valid || bits[(size_t)src]) : fill != 0) want |= 1ull << j;
        }
        expect(got == want, "shifted_word", (double)got, (double)want, wi, n);
      }
    }
  }
  // shift_source inside run_of's bounds: position i reads i - n exactly when the truth says the row n before it in its partition exists
  auto gen = [&]() { return (int64_t)(rng() % 100); };
  const Column<int64_t> c = make_column<int64_t>(1500, "short", true, 0, rng, gen, (int64_t)0);
  for (int64_t n : {0, 1, -1, 5, -5, 39, 40, -41, 1499, 1500, -1505}) for (int64_t i = 0; i < c.n; i++) {
    int64_t s0, s1, src;
    const bool ok = segment_of(c, i, &s0, &s1);
    const bool in = shift_source(i, n, s0, s1, &src);
    const bool want = i - n >= c.seg_of[(size_t)i * 2] && i - n < c.seg_of[(size_t)i * 2 + 1];
    expect(ok && in == want && (!in || src == i - n), "shift_source", in, want, i, n);
  }
  // diff_value: wrapping in the result type
  expect(diff_value<int16_t, uint8_t>(0, 255) == -255, "diff u8", diff_value<int16_t, uint8_t>(0, 255), -255, 0, 0);
  expect(diff_value<int64_t, uint64_t>(0, ~0ull) == 1, "diff u64", (double)diff_value<int64_t, uint64_t>(0, ~0ull), 1, 0, 0);
  expect(diff_value<int64_t, int64_t>(std::numeric_limits<int64_t>::min(), 1) == std::numeric_limits<int64_t>::max(), "diff i64 wraps", 0, 0, 0, 0);
  expect(diff_value<int8_t, int8_t>(-128, 127) == 1, "diff i8 wraps", diff_value<int8_t, int8_t>(-128, 127), 1, 0, 0);
  // the packed parameters
  const Params p = unpack_params(pack_params(2048, 7, true));
  expect(p.window == 2048 && p.min_samples == 7 && p.center && params_ok(p) && !params_ok(unpack_params(pack_params(3, 4, false))) && !params_ok(unpack_params(0)), "params", 0, 0, 0, 0);
}

int main() {
  std::mt19937_64 rng(419);
  check_shift(rng);
  {
    auto gen = [&]() { const uint64_t r = rng(); return r % 11 == 0 ? std::numeric_limits<int64_t>::max() : r % 13 == 0 ? std::numeric_limits<int64_t>::min() : (int64_t)(r % 2001) - 1000; };
    run_type<PLX_CUM_SUM, int64_t>("sum i64", gen, (int64_t)0x5555555555555555ll, rng);
  }
  {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    auto gen = [&]() { const uint64_t r = rng(); return r % 401 == 0 ? inf : r % 409 == 0 ? -inf : r % 997 == 0 ? nan : (double)((int64_t)(r % 2001) - 1000); };      // integer-valued: any association is exact
    run_type<PLX_CUM_SUM, double>("sum f64", gen, nan, rng);
    auto gen2 = [&]() { const uint64_t r = rng(); return r % 7 == 0 ? nan : r % 401 == 0 ? inf : (double)((int64_t)(r % 2001) - 1000) * 0.5; };
    run_type<PLX_CUM_MAX, double>("max f64", gen2, inf, rng);
  }
  {
    auto gen = [&]() { const uint64_t r = rng(); return r % 17 == 0 ? std::numeric_limits<int32_t>::min() : (int32_t)(r % 2001) - 1000; };
    run_type<PLX_CUM_MIN, int32_t>("min i32", gen, std::numeric_limits<int32_t>::min(), rng);
  }
  printf("checked=%lld bad=%lld\n", checked, bad);
  return bad ? 1 : 0;
}
