// distinct_main.cpp -- stand-alone driver of the n_unique / unique() arithmetic (polars_amd/csrc/distinct.hpp: rank_before, keep_row, the keep check and the bound
// of the bitmap route -- the one body of segment_distinct_kernel, of distinct_keep_kernel and of the host side of the routes), built with
// -fsanitize=address,undefined by the tests.  (TEST INFRASTRUCTURE: never linked into libpolars_amd.so.)
//
// What it is checked against is brute force written out here from the contract, not from the header:
//   (1) n in {0, 1, 63, 64, 65, 4097}: head masks that are empty, full, random at three densities, and with heads exactly at the word boundaries (bits 63, 64, 65,
//       the last bit); the mask and its prefix are allocated at their exact sizes, so a read past either is an ASan report.  rank_before(i) for EVERY i in 0..n
//       (n itself included: a multiple of 64 reads no word behind the mask) against a running count.
//   (2) the distinct values of every segment [a, b) of random cuts = rank_before(b) - rank_before(a), against counting the bits.
//   (3) keep_row for the four strategies over the sorted classes of random keys: the rows kept, mapped back through the (stable) order, are the first / last /
//       only rows of each class in row order; "any" keeps what "first" keeps.
//   (4) the keep check takes 0..3 only; the bitmap bound is max(64 n, 2^20) bits at its edges.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <numeric>
#include <random>
#include <vector>

#include "../../polars_amd/csrc/distinct.hpp"

using namespace plx::distinct;

static long long bad = 0, checked = 0;
static void expect(bool ok, const char* what, long long got, long long want, long long at) {
  checked++;
  if (!ok && bad++ < 20) fprintf(stderr, "%s: got %lld, want %lld (at %lld)\n", what, got, want, at);
}

struct Mask {
  std::vector<uint64_t> words;      // exactly ceil(n / 64) words
  std::vector<uint64_t> prefix;     // exactly words + 1 entries
  size_t n;
};
static Mask build(const std::vector<bool>& bits) {
  Mask m;
  m.n = bits.size();
  m.words.assign((m.n + 63) / 64, 0);
  for (size_t i = 0; i < m.n; i++) if (bits[i]) m.words[i >> 6] |= 1ull << (i & 63);
  m.prefix.assign(m.words.size() + 1, 0);
  for (size_t w = 0; w < m.words.size(); w++) {
    int c = 0;
    for (int b = 0; b < 64; b++) c += (int)((m.words[w] >> b) & 1);      // not the header's popcount
    m.prefix[w + 1] = m.prefix[w] + (uint64_t)c;
  }
  return m;
}

static void check_mask(const std::vector<bool>& bits, std::mt19937_64& rng) {
  const Mask m = build(bits);
  const size_t n = m.n;
  std::vector<uint64_t> run(n + 1, 0);
  for (size_t i = 0; i < n; i++) run[i + 1] = run[i] + (bits[i] ? 1 : 0);
  for (size_t i = 0; i <= n; i++) {
    const uint64_t got = rank_before(m.prefix.data(), m.words.data(), i);
    expect(got == run[i], "rank_before", (long long)got, (long long)run[i], (long long)i);
  }
  // segments: sorted random cuts, first 0, the last one ends at n
  std::vector<size_t> cuts{0};
  for (int k = 0; k < 40 && n; k++) cuts.push_back((size_t)(rng() % (n + 1)));
  for (size_t b : {(size_t)63, (size_t)64, (size_t)65, (size_t)128}) if (b <= n) cuts.push_back(b);
  cuts.push_back(n);
  std::sort(cuts.begin(), cuts.end());
  for (size_t g = 0; g + 1 < cuts.size(); g++) {
    const size_t a = cuts[g], b = cuts[g + 1];
    long long want = 0;
    for (size_t i = a; i < b; i++) want += bits[i] ? 1 : 0;
    const long long got = (long long)(rank_before(m.prefix.data(), m.words.data(), b) - rank_before(m.prefix.data(), m.words.data(), a));
    expect(got == want, "segment distinct", got, want, (long long)a);
  }
}

static void check_keep(size_t n, int n_keys, std::mt19937_64& rng) {
  std::vector<int> key(n);
  for (auto& k : key) k = (int)(rng() % (uint64_t)n_keys);
  std::vector<uint32_t> perm(n);
  std::iota(perm.begin(), perm.end(), 0u);
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
  std::vector<bool> head(n);
  for (size_t i = 0; i < n; i++) head[i] = i == 0 || key[perm[i]] != key[perm[i - 1]];
  // brute force, in row order
  std::map<int, std::vector<size_t>> rows_of;
  for (size_t r = 0; r < n; r++) rows_of[key[r]].push_back(r);
  for (int keep = PLX_UNIQUE_ANY; keep <= PLX_UNIQUE_NONE; keep++) {
    std::vector<bool> want(n, false), got(n, false);
    for (auto& kv : rows_of) {
      const auto& rs = kv.second;
      if (keep == PLX_UNIQUE_LAST) want[rs.back()] = true;
      else if (keep == PLX_UNIQUE_NONE) { if (rs.size() == 1) want[rs[0]] = true; }
      else want[rs.front()] = true;
    }
    for (size_t i = 0; i < n; i++) {
      const bool is_tail = i + 1 == n || head[i + 1];
      if (keep_row(head[i], is_tail, keep)) got[perm[i]] = true;
    }
    for (size_t r = 0; r < n; r++) expect(got[r] == want[r], "keep_row", got[r], want[r], (long long)r * 4 + keep);
  }
}

int main() {
  std::mt19937_64 rng(416);
  const size_t sizes[] = {0, 1, 63, 64, 65, 4097};
  for (size_t n : sizes) {
    check_mask(std::vector<bool>(n, false), rng);
    check_mask(std::vector<bool>(n, true), rng);
    for (int density : {2, 7, 50}) {
      for (int rep = 0; rep < 4; rep++) {
        std::vector<bool> bits(n);
        for (size_t i = 0; i < n; i++) bits[i] = i == 0 || (int)(rng() % 100) < density;
        check_mask(bits, rng);
      }
    }
    {      // heads at the word boundaries only
      std::vector<bool> bits(n, false);
      for (size_t b : {(size_t)0, (size_t)63, (size_t)64, (size_t)65, (size_t)127, (size_t)128, (size_t)4095, (size_t)4096}) if (b < n) bits[b] = true;
      if (n) bits[n - 1] = true;
      check_mask(bits, rng);
    }
    for (int n_keys : {1, 2, 5, 64, 5000}) check_keep(n, n_keys, rng);
  }
  for (int keep = -2; keep <= 6; keep++) expect(keep_ok(keep) == (keep >= 0 && keep <= 3), "keep_ok", keep_ok(keep), keep >= 0 && keep <= 3, keep);
  expect(keep_served(PLX_UNIQUE_ANY) == PLX_UNIQUE_FIRST && keep_served(PLX_UNIQUE_LAST) == PLX_UNIQUE_LAST && keep_served(PLX_UNIQUE_NONE) == PLX_UNIQUE_NONE, "keep_served", 0, 0, 0);
  const uint64_t floor_bits = 1ull << 20;
  expect(!bitmap_route_ok(0, 10), "bound: empty range", 0, 0, 0);
  expect(bitmap_route_ok(floor_bits, 0) && !bitmap_route_ok(floor_bits + 1, 0), "bound: the floor with no rows", 0, 0, 1);
  expect(bitmap_route_ok(floor_bits, 16384) && !bitmap_route_ok(floor_bits + 1, 16384), "bound: 64 n == the floor", 0, 0, 2);
  expect(bitmap_route_ok(64ull * 16385, 16385) && !bitmap_route_ok(64ull * 16385 + 1, 16385), "bound: 64 n above the floor", 0, 0, 3);
  expect(bitmap_route_ok(~0ull, ~0ull >> 2), "bound: 64 n saturates", 0, 0, 4);
  printf("checked=%lld bad=%lld\n", checked, bad);
  return bad ? 1 : 0;
}
