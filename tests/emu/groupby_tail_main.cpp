// The host side of the group-by tail (polars_amd/csrc/groupby_tail.hpp) as a stand-alone program, built with -fsanitize=address,undefined by
// tests/test_groupby_tail_cpu.py:
//   * the layout of the result block at G = 1, 63, 64, 65, 4096 for every output width (1, 2, 4, 8 bytes, Boolean bitmap), with and without validity, alone and in
//     mixed column lists: offsets 16-byte aligned, pieces disjoint and inside the block, and tail_block_fits true exactly when the block is at most the limit;
//   * every piece written to its last byte in a heap block of exactly `total` bytes (the sanitizer sees a byte too many);
//   * the rank computation the kernel runs (occupied mask -> bases -> rank of a slot, bitmap words over ranks with zero bits beyond n_groups) against a plain loop:
//     the empty mask, the full mask, only slot 0, only the last slot, alternating masks.
// Prints "<checks> checks, <failed> failed"; exit status 1 when any failed.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../../polars_amd/csrc/groupby_tail.hpp"

using namespace plx::gbt;

static long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...) \
  do { g_checks++; if (!(cond)) { g_failed++; if (g_failed < 20) { printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static const size_t kBounce = size_t(1) << 20;      // core.hpp kBounceBytes

// dtype codes of include/polars_amd.h: BOOL 0, I8 1, I16 2, I32 3, I64 4, U8 5, U16 6, U32 7, U64 8, F32 9, F64 10
static const int kDtypes[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10};
static uint32_t width_of(int dt) { static const uint32_t w[] = {0, 1, 2, 4, 8, 1, 2, 4, 8, 4, 8}; return w[dt]; }

static void check_layout(int G, const std::vector<int32_t>& dts, const std::vector<uint8_t>& nul) {
  TailLayout L;
  tail_layout(&L, G, dts.data(), nul.data(), (int)dts.size());
  const uint32_t words = (uint32_t)(G + 63) / 64;
  CHECK(L.n_cols == dts.size() && L.words == words, "G=%d", G);
  std::vector<std::pair<uint32_t, uint32_t>> pieces;      // [begin, end)
  pieces.push_back({0, kTailHeaderBytes});
  for (size_t j = 0; j < dts.size(); j++) {
    const uint32_t w = width_of(dts[j]);
    const uint32_t vb = w ? (uint32_t)G * w : words * 8;
    CHECK(w == tail_dtype_width(dts[j]), "dtype %d", dts[j]);
    CHECK(L.values_bytes[j] == vb, "G=%d col %zu: %u != %u", G, j, L.values_bytes[j], vb);
    CHECK(L.values_off[j] % 16 == 0 && L.values_off[j] >= kTailHeaderBytes, "G=%d col %zu values_off %u", G, j, L.values_off[j]);
    pieces.push_back({L.values_off[j], L.values_off[j] + vb});
    if (nul[j]) {
      CHECK(L.valid_off[j] % 16 == 0 && L.valid_off[j] >= kTailHeaderBytes, "G=%d col %zu valid_off %u", G, j, L.valid_off[j]);
      pieces.push_back({L.valid_off[j], L.valid_off[j] + words * 8});
    } else {
      CHECK(L.valid_off[j] == 0, "G=%d col %zu: validity of a column without one", G, j);
    }
  }
  std::sort(pieces.begin(), pieces.end());
  for (size_t i = 0; i + 1 < pieces.size(); i++) CHECK(pieces[i].second <= pieces[i + 1].first, "G=%d pieces %zu and %zu overlap", G, i, i + 1);
  CHECK(pieces.back().second <= L.total && L.total % 16 == 0, "G=%d total %u", G, L.total);
  CHECK(tail_block_fits(L, kBounce) == ((size_t)L.total <= kBounce), "G=%d fits", G);
  CHECK(tail_block_fits(L, L.total) && !tail_block_fits(L, (uint64_t)L.total - 1), "G=%d fits at the edge", G);
  // write every piece to its last byte in a block of exactly `total` bytes
  uint8_t* block = (uint8_t*)malloc(L.total);
  memset(block, 0, kTailHeaderBytes);
  for (size_t j = 0; j < dts.size(); j++) {
    memset(block + L.values_off[j], 0xa5, L.values_bytes[j]);
    if (nul[j]) memset(block + L.valid_off[j], 0x5a, (size_t)words * 8);
  }
  TailHeader h;
  memcpy(&h, block, sizeof h);
  CHECK(h.n_groups == 0 && sizeof(TailHeader) == kTailHeaderBytes, "header");
  free(block);
}

static void layouts() {
  const int Gs[] = {1, 63, 64, 65, 4096};
  for (int G : Gs) {
    for (int dt : kDtypes)
      for (int n = 0; n < 2; n++) check_layout(G, {dt}, {(uint8_t)n});
    // every dtype together, validity alternating both ways; a full job list of the widest and of the narrowest columns
    std::vector<int32_t> all(kDtypes, kDtypes + 11);
    std::vector<uint8_t> a(11), b(11);
    for (int j = 0; j < 11; j++) { a[j] = j & 1; b[j] = !(j & 1); }
    check_layout(G, all, a);
    check_layout(G, all, b);
    check_layout(G, std::vector<int32_t>(kTailMaxCols, 10), std::vector<uint8_t>(kTailMaxCols, 1));
    check_layout(G, std::vector<int32_t>(kTailMaxCols, 0), std::vector<uint8_t>(kTailMaxCols, 0));
    check_layout(G, std::vector<int32_t>(kTailMaxCols, 5), std::vector<uint8_t>(kTailMaxCols, 1));
  }
  // the host's question at the limit: 24 f64 columns with validity at G = 4096 are 24 * (32768 + 512) + 16 = 798736 bytes, below 2^20; no list of 24 columns exceeds it,
  // so the answer "does not fit" is driven with smaller limits
  TailLayout L;
  std::vector<int32_t> d(kTailMaxCols, 10); std::vector<uint8_t> n(kTailMaxCols, 1);
  tail_layout(&L, 4096, d.data(), n.data(), kTailMaxCols);
  CHECK(L.total == 24u * (32768u + 512u) + 16u && tail_block_fits(L, kBounce) && !tail_block_fits(L, 1u << 19), "largest block %u", L.total);
}

// ---- ranks ----------------------------------------------------------------------------------------------------------------------------------
static void check_ranks(int G, const std::vector<uint8_t>& occupied, const char* what) {
  const uint32_t words = (uint32_t)(G + 63) / 64;
  std::vector<uint64_t> occ(words, 0);
  for (int s = 0; s < G; s++) if (occupied[s]) occ[s >> 6] |= 1ull << (s & 63);
  std::vector<uint32_t> base(words);
  const uint32_t n = tail_rank_bases(occ.data(), words, base.data());
  // the plain loop
  std::vector<uint32_t> slot_of;
  for (int s = 0; s < G; s++) if (occupied[s]) slot_of.push_back((uint32_t)s);
  CHECK(n == slot_of.size(), "%s G=%d: %u groups, expected %zu", what, G, n, slot_of.size());
  std::vector<uint32_t> got(n, ~0u);      // exactly n entries: a rank >= n is a heap overflow the sanitizer reports
  for (int s = 0; s < G; s++)
    if ((occ[s >> 6] >> (s & 63)) & 1) {
      const uint32_t r = tail_rank_of(occ.data(), base.data(), (uint32_t)s);
      CHECK(r < n, "%s G=%d slot %d: rank %u", what, G, s, r);
      if (r < n) got[r] = (uint32_t)s;
    }
  CHECK(got == slot_of, "%s G=%d: ranks differ from ascending slot order", what, G);
  // validity words over ranks: rank r is "valid" iff its slot is a multiple of 3; bits at and beyond n are zero whatever the ballot said
  for (uint32_t w = 0; w < words; w++) {
    uint64_t ballot = 0, want = 0;
    for (uint32_t b = 0; b < 64; b++) {
      const uint32_t r = w * 64 + b;
      if (r < n && slot_of[r] % 3 == 0) { ballot |= 1ull << b; want |= 1ull << b; }
      if (r >= n) ballot |= 1ull << b;      // what a careless lane beyond the last group would add
    }
    CHECK(tail_rank_word(ballot, w, n) == want, "%s G=%d word %u", what, G, w);
  }
}

static void ranks() {
  const int Gs[] = {1, 2, 8, 63, 64, 65, 128, 4096};
  for (int G : Gs) {
    std::vector<uint8_t> m(G, 0);
    check_ranks(G, m, "empty");
    std::fill(m.begin(), m.end(), 1); check_ranks(G, m, "full");
    std::fill(m.begin(), m.end(), 0); m[0] = 1; check_ranks(G, m, "slot 0");
    std::fill(m.begin(), m.end(), 0); m[G - 1] = 1; check_ranks(G, m, "last slot");
    for (int s = 0; s < G; s++) m[s] = (s & 1) == 0; check_ranks(G, m, "even slots");
    for (int s = 0; s < G; s++) m[s] = (s & 1) == 1; check_ranks(G, m, "odd slots");
    for (int s = 0; s < G; s++) m[s] = ((s >> 6) & 1) == 0; check_ranks(G, m, "alternating words");
  }
  const uint64_t xs[] = {0, 1, ~0ull, 0x8000000000000000ull, 0x5555555555555555ull, 0x0123456789abcdefull};
  for (uint64_t x : xs) CHECK(tail_popc64(x) == (uint32_t)__builtin_popcountll(x), "popcount");
}

int main() {
  layouts();
  ranks();
  printf("%ld checks, %ld failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
