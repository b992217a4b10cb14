// strmatch_main.cpp -- stand-alone driver of the string predicates' decision function (polars_amd/csrc/strmatch.hpp: match_view, the one body of the device kernel
// and of plx_strview_match_host, and match_views_host, the host twin's loop), built with -fsanitize=address,undefined by the tests.  The case file holds views, their
// data buffer and, per case, a kind, a pattern and the expected answers / validity / flags; views and data are copied into heap blocks of EXACTLY their size, so a
// read past either end aborts the process.  (TEST INFRASTRUCTURE: never linked into libpolars_amd.so.)
//
// file: u64 n, u64 data_len, u64 n_cases, views[16 n], data[data_len], then per case: i32 kind, u32 m, u32 no_data, u32 want_flags, pattern[m], bits[ceil(n/64)] u64, valid[ceil(n/64)] u64
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../polars_amd/csrc/strmatch.hpp"

using namespace plx::strmatch;

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t n = 0, data_len = 0, n_cases = 0;
  if (!rd(f, &n, 8) || !rd(f, &data_len, 8) || !rd(f, &n_cases, 8)) return 3;
  unsigned char* views = (unsigned char*)malloc(n ? 16 * n : 1);
  unsigned char* data = (unsigned char*)malloc(data_len ? data_len : 1);
  if (!rd(f, views, 16 * n) || !rd(f, data, data_len)) return 3;
  const size_t words = (n + 63) / 64;
  int bad = 0;
  for (uint64_t c = 0; c < n_cases; c++) {
    int32_t kind; uint32_t m, no_data, want_flags;
    if (!rd(f, &kind, 4) || !rd(f, &m, 4) || !rd(f, &no_data, 4) || !rd(f, &want_flags, 4) || m > (uint32_t)kMaxPattern) return 3;
    std::vector<uint8_t> pattern(m);
    std::vector<uint64_t> want_bits(words), want_valid(words), bits(words + 1, 0x5a5a5a5a5a5a5a5aull), valid(words + 1, 0x5a5a5a5a5a5a5a5aull);
    if (!rd(f, pattern.data(), m) || !rd(f, want_bits.data(), 8 * words) || !rd(f, want_valid.data(), 8 * words)) return 3;
    const Pattern pat = make_pattern(pattern.data(), m);
    const Pool pool{no_data ? nullptr : data, no_data ? 0 : data_len, 0};
    const uint32_t flags = match_views_host(views, pool, (int64_t)n, kind, pat, bits.data(), valid.data());
    bool ok = flags == want_flags && bits[words] == 0x5a5a5a5a5a5a5a5aull && valid[words] == 0x5a5a5a5a5a5a5a5aull;
    for (size_t w = 0; w < words; w++) ok = ok && bits[w] == want_bits[w] && valid[w] == want_valid[w];
    if (!ok) { fprintf(stderr, "case %llu (kind %d, m %u): flags %u, want %u, or the bitmaps differ\n", (unsigned long long)c, kind, m, flags, want_flags); bad++; }
  }
  free(views); free(data);
  fclose(f);
  printf("cases=%llu bad=%d\n", (unsigned long long)n_cases, bad);
  return bad ? 1 : 0;
}
