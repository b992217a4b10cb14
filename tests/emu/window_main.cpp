// window_main.cpp -- stand-alone driver of the window arithmetic (polars_amd/csrc/window.hpp: the route rule, the key code of the direct route, slot_store, sorted_group
// and the per-lane body of the broadcast -- the one body of window_slots_kernel, window_group_ids_kernel and window_broadcast_kernel and of the host side of the
// routes), built with -fsanitize=address,undefined by the tests.  (TEST INFRASTRUCTURE: never linked into libpolars_amd.so.)
//
// What it is checked against is brute force written out here from the contract, not from the header:
//   (1) n in {0, 1, 63, 64, 65, 129} rows, one and two key parts of several dtypes, with and without null parts: the brute-force map row -> group is a std::map from
//       the tuple of (is null, value) to the group in first-occurrence order.  Every buffer -- values, validity words, the slot table of exactly R entries, the head
//       mask, its prefix, outputs and their bitmaps -- is allocated at its exact size, so a read or write past any of them is an ASan report.
//   (2) direct route: slot_store for every group, then slot[row_code(r)] for every row == the brute-force group; codes are below R and distinct per group.
//   (3) sorted route: a stable sort of the rows (nulls last), the head mask and its per-word prefix, the groups sorted the same way, sorted_group for every position.
//   (4) broadcast: wave by wave (64 lanes, the tail wave short), lane_bits / copy_value for outputs of width 0, 1, 2, 4, 8 with and without validity; the ballots are
//       assembled the way the kernel's __ballot does and compared with the expected words, pad bits zero.
//   (5) the rule: 4 R <= max(8 n, 4 MiB) at the bound and one beyond it, with no rows, at the floor, above it, saturating; joint_range without overflow; a value
//       outside its declared range and a null without a null code give no code.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <numeric>
#include <random>
#include <vector>

#include "../../polars_amd/csrc/window.hpp"

using namespace plx::window;

static long long bad = 0, checked = 0;
static void expect(bool ok, const char* what, long long got, long long want, long long at) {
  checked++;
  if (!ok && bad++ < 20) fprintf(stderr, "%s: got %lld, want %lld (at %lld)\n", what, got, want, at);
}

struct Col {
  int dtype;
  std::vector<int64_t> v;          // logical values
  std::vector<bool> ok;
  bool nullable;
  std::vector<uint8_t> bytes;      // the physical values at their exact size
  std::vector<uint64_t> valid;     // exactly ceil(n / 64) words (empty: no bitmap)
};
static int width_of(int dt) { return dt == PLX_I8 || dt == PLX_U8 ? 1 : dt == PLX_I16 || dt == PLX_U16 ? 2 : dt == PLX_I32 || dt == PLX_U32 ? 4 : 8; }
static void pack(Col& c) {
  const size_t n = c.v.size();
  if (c.dtype == PLX_BOOL) {
    c.bytes.assign(((n + 63) / 64) * 8, 0);
    for (size_t i = 0; i < n; i++) if (c.v[i]) reinterpret_cast<uint64_t*>(c.bytes.data())[i >> 6] |= 1ull << (i & 63);
  } else {
    const int w = width_of(c.dtype);
    c.bytes.assign(n * (size_t)w, 0);
    for (size_t i = 0; i < n; i++) memcpy(c.bytes.data() + i * (size_t)w, &c.v[i], (size_t)w);      // little endian
  }
  c.valid.clear();
  if (c.nullable) {
    c.valid.assign((n + 63) / 64, 0);
    for (size_t i = 0; i < n; i++) if (c.ok[i]) c.valid[i >> 6] |= 1ull << (i & 63);
  }
}
static Col make_col(int dtype, size_t n, int64_t lo, int64_t hi, bool nullable, std::mt19937_64& rng) {
  Col c;
  c.dtype = dtype; c.nullable = nullable;
  c.v.resize(n); c.ok.assign(n, true);
  for (size_t i = 0; i < n; i++) {
    c.v[i] = dtype == PLX_BOOL ? (int64_t)(rng() & 1) : lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1));
    if (nullable && rng() % 5 == 0) c.ok[i] = false;
  }
  pack(c);
  return c;
}
using Key = std::vector<std::pair<bool, int64_t>>;      // per part (is null, value); nulls last in the order
static Key key_of(const std::vector<Col>& cols, size_t r) {
  Key k;
  for (const Col& c : cols) k.push_back({!c.ok[r], c.ok[r] ? c.v[r] : 0});
  return k;
}

static void check_case(size_t n, std::vector<Col> cols, std::mt19937_64& rng) {
  // ---- brute force: groups in first-occurrence order ----
  std::map<Key, uint32_t> group_of;
  std::vector<uint32_t> want(n);
  std::vector<size_t> first_row;
  for (size_t r = 0; r < n; r++) {
    auto it = group_of.find(key_of(cols, r));
    if (it == group_of.end()) { it = group_of.emplace(key_of(cols, r), (uint32_t)first_row.size()).first; first_row.push_back(r); }
    want[r] = it->second;
  }
  const size_t G = first_row.size();
  // the group frame's key columns
  std::vector<Col> gcols;
  for (const Col& c : cols) {
    Col g; g.dtype = c.dtype; g.nullable = c.nullable;
    for (size_t r : first_row) { g.v.push_back(c.v[r]); g.ok.push_back(c.ok[r]); }
    pack(g);
    gcols.push_back(g);
  }
  // ---- direct ----
  Keys rk{};
  rk.n_parts = (int)cols.size();
  uint64_t ranges[kMaxKeys];
  uint64_t stride = 1;
  for (size_t j = 0; j < cols.size(); j++) {
    const Col& c = cols[j];
    int64_t mn = 0, mx = -1;
    bool any = false;
    for (size_t r = 0; r < n; r++) if (c.ok[r]) { if (!any || c.v[r] < mn) mn = c.v[r]; if (!any || c.v[r] > mx) mx = c.v[r]; any = true; }
    KeyPart& p = rk.part[j];
    p.values = c.bytes.data(); p.validity = c.nullable ? c.valid.data() : nullptr; p.dtype = c.dtype; p.nullable = c.nullable ? 1 : 0;
    p.min = any ? mn : 0; p.span = any ? (uint64_t)(mx - mn) + 1 : 0;
    if (c.dtype == PLX_BOOL) { p.min = 0; p.span = 2; }
    p.stride = stride;
    ranges[j] = p.span + (uint64_t)p.nullable;
    stride *= ranges[j];
  }
  const uint64_t R = joint_range(ranges, rk.n_parts, ~0ull >> 2);
  rk.range = R;
  expect(R == stride || n == 0, "joint_range", (long long)R, (long long)stride, (long long)n);
  if (n && R) {
    Keys gk = rk;
    for (size_t j = 0; j < cols.size(); j++) { gk.part[j].values = gcols[j].bytes.data(); gk.part[j].validity = gcols[j].nullable ? gcols[j].valid.data() : nullptr; }
    std::vector<uint32_t> slot((size_t)R, 0xdeadbeefu);      // exactly R entries, never cleared by the route
    std::vector<bool> taken((size_t)R, false);
    for (size_t g = 0; g < G; g++) {
      uint64_t code = ~0ull;
      const bool ok = row_code(gk, (int64_t)g, &code);
      expect(ok && code < R && !taken[(size_t)code], "group code", (long long)code, (long long)R, (long long)g);
      if (ok && code < R) taken[(size_t)code] = true;
      expect(slot_store(gk, (int64_t)g, slot.data()), "slot_store", 0, 1, (long long)g);
    }
    for (size_t r = 0; r < n; r++) {
      uint64_t code = ~0ull;
      const bool ok = row_code(rk, (int64_t)r, &code);
      expect(ok && code < R, "row code", (long long)code, (long long)R, (long long)r);
      if (ok && code < R) expect(slot[(size_t)code] == want[r], "direct map", slot[(size_t)code], want[r], (long long)r);
    }
  }
  // ---- sorted ----
  std::vector<uint32_t> gid(n, 0xdeadbeefu);
  if (n) {
    std::vector<uint32_t> perm(n), order(G);
    std::iota(perm.begin(), perm.end(), 0u);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return key_of(cols, a) < key_of(cols, b); });
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key_of(gcols, a) < key_of(gcols, b); });
    std::vector<uint64_t> heads((n + 63) / 64, 0), prefix((n + 63) / 64 + 1, 0);
    for (size_t i = 0; i < n; i++) if (i == 0 || key_of(cols, perm[i]) != key_of(cols, perm[i - 1])) heads[i >> 6] |= 1ull << (i & 63);
    for (size_t w = 0; w < heads.size(); w++) {
      int c = 0;
      for (int b = 0; b < 64; b++) c += (int)((heads[w] >> b) & 1);
      prefix[w + 1] = prefix[w] + (uint64_t)c;
    }
    expect(prefix.back() == G, "segments == groups", (long long)prefix.back(), (long long)G, (long long)n);
    for (size_t i = 0; i < n; i++) {
      const uint32_t g = sorted_group(prefix.data(), heads.data(), order.data(), G, i);
      expect(g < G, "sorted_group in range", g, (long long)G, (long long)i);
      gid[perm[i]] = g;
    }
    for (size_t r = 0; r < n; r++) expect(gid[r] == want[r], "sorted map", gid[r], want[r], (long long)r);
    // a segment count that is not G: the answer is "no group", never a read outside order[]
    std::vector<uint32_t> short_order(order.begin(), order.end() - 1);
    const uint32_t g_last = sorted_group(prefix.data(), heads.data(), short_order.data(), G - 1, n - 1);
    expect(G == 1 ? g_last == 0 : g_last == G - 1, "sorted_group past the groups", g_last, (long long)G - 1, (long long)n);
  }
  // ---- broadcast, wave by wave ----
  const int widths[5] = {0, 1, 2, 4, 8};
  for (int wi = 0; wi < 5; wi++) {
    for (int with_valid = 0; with_valid < 2; with_valid++) {
      const int w = widths[wi];
      const size_t gw = std::max<size_t>(G, 1);
      std::vector<uint64_t> gval(gw), gbits((G + 63) / 64, 0), gvalid((G + 63) / 64, 0);
      std::vector<uint8_t> gbytes(G * (size_t)std::max(w, 1), 0);
      std::vector<bool> gok(G, true);
      for (size_t g = 0; g < G; g++) {
        gval[g] = rng();
        if (w) memcpy(gbytes.data() + g * (size_t)w, &gval[g], (size_t)w); else if (gval[g] & 1) gbits[g >> 6] |= 1ull << (g & 63);
        gok[g] = !with_valid || rng() % 3 != 0;
        if (gok[g]) gvalid[g >> 6] |= 1ull << (g & 63);
      }
      const size_t words = (n + 63) / 64;
      std::vector<uint8_t> dst(w ? n * (size_t)w : words * 8, 0xcd);
      std::vector<uint64_t> dvalid(words, 0xcdcdcdcdcdcdcdcdull);
      Output o{};
      o.src = w ? (const void*)gbytes.data() : (const void*)gbits.data();
      o.src_valid = with_valid ? gvalid.data() : nullptr;
      o.dst = dst.data(); o.dst_valid = with_valid ? dvalid.data() : nullptr; o.width = w;
      for (size_t tile = 0; tile < words; tile++) {
        uint64_t ballot_valid = 0, ballot_true = 0;
        for (int lane = 0; lane < 64; lane++) {
          const size_t r = tile * 64 + (size_t)lane;
          const bool ok = r < n;
          const uint64_t g = ok ? want[r] : 0;
          const unsigned b = lane_bits(o, ok, g);
          if (w && ok) copy_value(w, o.src, g, o.dst, (int64_t)r);
          if (b & 1u) ballot_valid |= 1ull << lane;
          if (b & 2u) ballot_true |= 1ull << lane;
        }
        if (!w) reinterpret_cast<uint64_t*>(o.dst)[tile] = ballot_true;
        if (o.dst_valid) o.dst_valid[tile] = ballot_valid;
      }
      for (size_t r = 0; r < n; r++) {
        const size_t g = want[r];
        if (w) {
          uint64_t got = 0, exp = 0;
          memcpy(&got, dst.data() + r * (size_t)w, (size_t)w); memcpy(&exp, &gval[g], (size_t)w);
          expect(got == exp, "broadcast value", (long long)got, (long long)exp, (long long)r);
        } else {
          const bool got = (reinterpret_cast<uint64_t*>(dst.data())[r >> 6] >> (r & 63)) & 1;
          expect(got == (bool)(gval[g] & 1), "broadcast bit", got, (long long)(gval[g] & 1), (long long)r);
        }
        if (with_valid) expect((bool)((dvalid[r >> 6] >> (r & 63)) & 1) == gok[g], "broadcast validity", 0, gok[g], (long long)r);
      }
      if (n & 63) {      // the tail wave's words carry no bit past n
        const uint64_t pad = ~0ull << (n & 63);
        if (with_valid) expect((dvalid[words - 1] & pad) == 0, "validity pad bits", 0, 0, (long long)n);
        if (!w) expect((reinterpret_cast<uint64_t*>(dst.data())[words - 1] & pad) == 0, "value pad bits", 0, 0, (long long)n);
      }
    }
  }
}

int main() {
  std::mt19937_64 rng(417);
  const size_t sizes[] = {0, 1, 63, 64, 65, 129};
  for (size_t n : sizes) {
    for (int nullable = 0; nullable < 2; nullable++) {
      check_case(n, {make_col(PLX_I32, n, -3, 40, nullable, rng)}, rng);
      check_case(n, {make_col(PLX_I64, n, (1ll << 40) - 2, (1ll << 40) + 5, nullable, rng)}, rng);
      check_case(n, {make_col(PLX_I8, n, -128, 127, nullable, rng)}, rng);
      check_case(n, {make_col(PLX_U16, n, 65000, 65535, nullable, rng)}, rng);
      check_case(n, {make_col(PLX_BOOL, n, 0, 1, nullable, rng)}, rng);
      check_case(n, {make_col(PLX_I32, n, 0, 0, nullable, rng)}, rng);                               // one partition (two with nulls)
      check_case(n, {make_col(PLX_I64, n, 0, 1000000, nullable, rng)}, rng);                         // about n partitions
      check_case(n, {make_col(PLX_I32, n, 5, 9, nullable, rng), make_col(PLX_U8, n, 0, 3, !nullable, rng)}, rng);
      check_case(n, {make_col(PLX_I16, n, -2, 2, true, rng), make_col(PLX_BOOL, n, 0, 1, true, rng), make_col(PLX_U32, n, 7, 8, nullable, rng)}, rng);
    }
    {      // a part that is null on every row: the null code alone
      Col c = make_col(PLX_I32, n, 1, 5, true, rng);
      c.ok.assign(n, false);
      pack(c);
      check_case(n, {c, make_col(PLX_I8, n, 0, 2, false, rng)}, rng);
    }
  }
  // ---- no code for what the table has no place for ----
  {
    int32_t vals[3] = {5, 9, 12};
    uint64_t valid = 0b011;
    Keys k{};
    k.n_parts = 1; k.range = 5;
    k.part[0] = KeyPart{vals, &valid, 5, 5, 1, PLX_I32, 0};
    uint64_t code = 0;
    expect(row_code(k, 0, &code) && code == 0, "code of the minimum", (long long)code, 0, 0);
    expect(row_code(k, 1, &code) && code == 4, "code of the maximum", (long long)code, 4, 1);
    expect(!row_code(k, 2, &code), "a null without a null code", 0, 0, 2);
    valid = 0b111;
    expect(!row_code(k, 2, &code), "a value past its declared range", 0, 0, 3);
    vals[2] = 4;
    expect(!row_code(k, 2, &code), "a value below its declared range", 0, 0, 4);
    for (int dt = 0; dt <= 10; dt++) expect(part_ok(dt) == (dt <= PLX_U32), "part_ok", part_ok(dt), dt <= PLX_U32, dt);
  }
  // ---- the rule: 4 R <= max(8 n, 4 MiB) ----
  const uint64_t floor_slots = (4ull << 20) / 4;
  expect(!direct_route_ok(0, 10), "rule: empty range", 0, 0, 0);
  expect(direct_route_ok(floor_slots, 0) && !direct_route_ok(floor_slots + 1, 0), "rule: the floor with no rows", 0, 0, 1);
  expect(direct_route_ok(floor_slots, 1ull << 19) && !direct_route_ok(floor_slots + 1, 1ull << 19), "rule: 8 n == the floor", 0, 0, 2);
  expect(direct_route_ok(2 * ((1ull << 19) + 1), (1ull << 19) + 1) && !direct_route_ok(2 * ((1ull << 19) + 1) + 1, (1ull << 19) + 1), "rule: 8 n above the floor", 0, 0, 3);
  expect(direct_route_ok(2 * 4097, 4097) == (2 * 4097 <= floor_slots), "rule: a small frame under the floor", 0, 0, 4);
  expect(direct_route_ok(~0ull >> 2, ~0ull >> 1), "rule: 8 n saturates", 0, 0, 5);
  {
    const uint64_t big[3] = {1ull << 32, 1ull << 31, 4};
    expect(joint_range(big, 3, ~0ull >> 2) == 0, "joint_range: past the cap", 0, 0, 0);
    expect(joint_range(big, 2, ~0ull) == 1ull << 63, "joint_range: under the cap", 0, 0, 1);
    const uint64_t zero[2] = {7, 0};
    expect(joint_range(zero, 2, ~0ull) == 0, "joint_range: an empty part", 0, 0, 2);
  }
  printf("checked=%lld bad=%lld\n", checked, bad);
  return bad ? 1 : 0;
}
