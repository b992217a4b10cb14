// groupby_tail.hpp -- what the host and groupby_tail_kernel (kernels_fused.hip) share about the tail of an LDS-table group-by (DESIGN.md 4.11 "One tail kernel"):
// the layout of the result block and the rank computation.  Plain C++ with no HIP type in it: tests/emu/groupby_tail_main.cpp drives it under ASan + UBSan.
//
// The block is ONE device allocation the kernel fills and the host copies in ONE transfer:
//   [0, 16)   TailHeader {n_groups, oob, version, 0}
//   then, per output column in job order, each piece 16-byte aligned:
//     values    G elements of the column's width, or ceil(G / 64) u64 words for a Boolean column (a bitmap); rows [0, n_groups) are written
//     validity  ceil(G / 64) u64 words, nullable columns only; bits at and beyond n_groups are zero
// G is the slot count of the table (the capacity of the result), so the layout is known before the kernel runs.
#pragma once
#include <stdint.h>

#ifndef PLX_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define PLX_HD __host__ __device__
#else
#define PLX_HD
#endif
#endif

namespace plx {
namespace gbt {

constexpr uint32_t kTailLayoutVersion = 1;
constexpr int kTailMaxCols = 24;          // == fused::kMaxFinJobs (asserted where both are seen)
constexpr int kTailMaxSlots = 4096;       // the LDS-table route ends at 12 key bits
constexpr int kTailMaxWords = kTailMaxSlots / 64;
constexpr uint32_t kTailHeaderBytes = 16;

struct TailHeader {
  uint32_t n_groups, oob, version, zero;
};
struct TailLayout {
  uint32_t n_cols;
  uint32_t words;                        // ceil(G / 64): u64 words of every bitmap
  uint32_t values_off[kTailMaxCols];
  uint32_t values_bytes[kTailMaxCols];   // at capacity G
  uint32_t valid_off[kTailMaxCols];      // 0: the column has no validity
  uint32_t total;                        // bytes of the block, a multiple of 16
};

// element width of a dtype code of include/polars_amd.h (plx_dtype); 0 = PLX_BOOL, bit-packed
PLX_HD inline uint32_t tail_dtype_width(int dt) {
  switch (dt) {
    case 1: case 5: return 1;            // PLX_I8, PLX_U8
    case 2: case 6: return 2;            // PLX_I16, PLX_U16
    case 3: case 7: case 9: return 4;    // PLX_I32, PLX_U32, PLX_F32
    case 4: case 8: case 10: return 8;   // PLX_I64, PLX_U64, PLX_F64
    default: return 0;
  }
}
PLX_HD inline uint32_t tail_align16(uint32_t x) { return (x + 15u) & ~15u; }

// THE layout: a pure function of the slot count and, per output column, its dtype and whether it carries validity.  1 <= G <= kTailMaxSlots, n_cols <= kTailMaxCols.
// (written through a pointer: the kernel keeps its copy in LDS, the host on its stack)
PLX_HD inline void tail_layout(TailLayout* L, int G, const int32_t* dtypes, const uint8_t* nullable, int n_cols) {
  if (n_cols > kTailMaxCols) n_cols = kTailMaxCols;
  L->n_cols = (uint32_t)n_cols;
  L->words = ((uint32_t)G + 63u) / 64u;
  uint32_t at = kTailHeaderBytes;
  for (int j = 0; j < n_cols; j++) {
    const uint32_t w = tail_dtype_width(dtypes[j]);
    L->values_off[j] = at;
    L->values_bytes[j] = w ? (uint32_t)G * w : L->words * 8u;
    at = tail_align16(at + L->values_bytes[j]);
    L->valid_off[j] = 0;
    if (nullable[j]) { L->valid_off[j] = at; at = tail_align16(at + L->words * 8u); }
  }
  for (int j = n_cols; j < kTailMaxCols; j++) { L->values_off[j] = 0; L->values_bytes[j] = 0; L->valid_off[j] = 0; }
  L->total = at;
}
// does the block fit a staging buffer of `limit` bytes?  (the host asks this with kBounceBytes before it takes the tail)
PLX_HD inline bool tail_block_fits(const TailLayout& L, uint64_t limit) { return (uint64_t)L.total <= limit; }

// ---- ranks ------------------------------------------------------------------------------------------------------------------------------------------------------
// occ[w]: bit b set iff slot 64 w + b is occupied.  The output position of an occupied slot is its rank among the occupied slots in ascending slot order:
// rank(s) = base[s / 64] + popcount(occ[s / 64] & ((1 << (s % 64)) - 1)), base = the exclusive prefix sum of the words' popcounts.
PLX_HD inline uint32_t tail_popc64(uint64_t x) {
  x = x - ((x >> 1) & 0x5555555555555555ull);
  x = (x & 0x3333333333333333ull) + ((x >> 2) & 0x3333333333333333ull);
  x = (x + (x >> 4)) & 0x0f0f0f0f0f0f0f0full;
  return (uint32_t)((x * 0x0101010101010101ull) >> 56);
}
// base[0 .. words) from occ[0 .. words); returns n_groups.  (the kernel runs this on one lane over at most 64 words in LDS)
PLX_HD inline uint32_t tail_rank_bases(const uint64_t* occ, uint32_t words, uint32_t* base) {
  uint32_t n = 0;
  for (uint32_t w = 0; w < words; w++) { base[w] = n; n += tail_popc64(occ[w]); }
  return n;
}
PLX_HD inline uint32_t tail_rank_of(const uint64_t* occ, const uint32_t* base, uint32_t slot) {
  const uint32_t w = slot >> 6, b = slot & 63u;
  return base[w] + tail_popc64(occ[w] & ((1ull << b) - 1ull));
}
// word w of a bitmap over RANKS whose rows [0, n_groups) carry the bits `bits` of a ballot over ranks 64 w .. 64 w + 63: bits at and beyond n_groups are zero
PLX_HD inline uint64_t tail_rank_word(uint64_t bits, uint32_t w, uint32_t n_groups) {
  const uint64_t lo = (uint64_t)w * 64u;
  if (lo >= n_groups) return 0;
  const uint64_t left = n_groups - lo;
  return left >= 64 ? bits : bits & ((1ull << left) - 1ull);
}

}  // namespace gbt
}  // namespace plx
