// strmatch.hpp -- the per-string decision of str.starts_with / ends_with / contains(literal) over a 16-byte Utf8View / BinaryView, ONE body for the device
// kernel (kernels_strmatch.hip strview_match_kernel) and its host twin (plx_strview_match_host), so that a CPU test of the twin is a test of the kernel's logic.
//
// View layout (crates/polars-arrow/src/array/binview/view.rs:20-29): {len u32, 12 inline bytes} when len <= 12, else {len u32, prefix u32, buffer index u32, offset u32}.
// Comparison is byte-wise; a zero byte is an ordinary byte; the length word decides where a string ends, never the zero padding of an inline view.
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
namespace strmatch {

// Longest pattern the kernels take (bytes).  The pattern travels in the kernel argument struct as kPatternWords little-endian words, zero-padded behind its length; a
// longer one is PLX_ERR_UNSUPPORTED at the entry points.
constexpr int kMaxPattern = 64;
constexpr int kPatternWords = kMaxPattern / 8;
constexpr int kStartsWith = 0, kEndsWith = 1, kContains = 2;      // plx_str_match_kind
// what a row can report besides its answer (OR-ed into one flag word; such a row's answer is false)
constexpr uint32_t kFlagOutside = 1;      // a view points outside its buffer (offset + len beyond the pool, or a buffer index other than 0)
constexpr uint32_t kFlagNoData = 2;       // the decision needs the bytes behind a long view and there is no data buffer

struct Pattern {
  uint64_t w[kPatternWords];
  uint32_t len;
};
// where the bytes of long strings live
struct Pool {
  const unsigned char* data;      // may be null
  uint64_t data_len;              // bytes that may be read at `data`
  uint32_t rebased;               // 1: the second word of a long view is the absolute byte offset into `data` (the views of a device dictionary: StrEncode::dict_views
                                  // has added buf_base[buffer] already); 0: {buffer index, offset} as Arrow has them, over ONE buffer: any index but 0 points outside
};

inline Pattern make_pattern(const uint8_t* bytes, int64_t len) {
  Pattern p{};
  p.len = (uint32_t)len;
  for (int64_t i = 0; i < len && i < kMaxPattern; i++) p.w[i >> 3] |= (uint64_t)bytes[i] << (8 * (i & 7));
  return p;
}

// up to 8 bytes at p (any alignment) as a little-endian word, zero-extended: one 8-byte, or 4 + 2 + 1-byte loads (the load_bytes idiom of kernels_strview.hip)
PLX_HD inline uint64_t load_le(const unsigned char* p, uint32_t n) {
  uint64_t w = 0;
  if (n >= 8) { __builtin_memcpy(&w, p, 8); return w; }
  uint32_t i = 0;
  if (n & 4) { uint32_t x; __builtin_memcpy(&x, p, 4); w = x; i = 4; }
  if (n & 2) { unsigned short x; __builtin_memcpy(&x, p + i, 2); w |= (uint64_t)x << (8 * i); i += 2; }
  if (n & 1) w |= (uint64_t)p[i] << (8 * i);
  return w;
}
// the m bytes at s against the pattern, in words (the pattern is zero behind its length, as load_le's result is).  The trip count is fixed so that every pat.w[j]
// has a constant index: the pattern is read from the kernel arguments by the scalar unit, never copied to scratch.
PLX_HD inline bool eq_pattern(const unsigned char* s, const Pattern& pat, uint32_t m) {
#pragma unroll
  for (int j = 0; j < kPatternWords; j++) {
    const uint32_t at = 8u * (uint32_t)j;
    if (at >= m) break;
    const uint32_t n = m - at < 8u ? m - at : 8u;
    if (load_le(s + at, n) != pat.w[j]) return false;
  }
  return true;
}

// The decision for one non-null string.  w0 / w1: the two words of its view.  *flag collects kFlag* bits (a flagged row answers false).
PLX_HD inline bool match_view(uint64_t w0, uint64_t w1, const Pool& pool, int kind, const Pattern& pat, uint32_t* flag) {
  const uint32_t len = (uint32_t)w0, m = pat.len;
  if (len < m) return false;
  if (m == 0) return true;
  if (len <= 12) {
    // the view is the string: 12 bytes as one 96-bit number, the window at byte o compared under a mask of m bytes (m <= len <= 12; o + m <= len keeps the
    // window inside the string, so the padding is never matched)
    typedef unsigned __int128 u128;
    const u128 s = ((u128)(w1 >> 32) << 64) | (u128)((w0 >> 32) | (w1 << 32));
    const u128 p = ((u128)pat.w[1] << 64) | (u128)pat.w[0];
    const u128 mask = (((u128)1) << (8 * m)) - 1;
    if (kind == kStartsWith) return (s & mask) == p;
    if (kind == kEndsWith) return ((s >> (8 * (len - m))) & mask) == p;
    // every window a 12-byte string can have, with constant shifts (a variable 128-bit shift is a dozen instructions per lane); the guard keeps the ones inside the string
    bool hit = false;
#pragma unroll
    for (uint32_t o = 0; o <= 12; o++) hit |= (o + m <= len) && (((s >> (8 * o)) & mask) == p);
    return hit;
  }
  if (kind == kStartsWith) {
    // the view carries the first four bytes: they decide alone when m <= 4, and reject before the pool is touched otherwise
    const uint32_t prefix = (uint32_t)(w0 >> 32);
    const uint32_t pm = m >= 4 ? 0xffffffffu : ((1u << (8 * m)) - 1u);
    if ((prefix & pm) != (uint32_t)pat.w[0]) return false;
    if (m <= 4) return true;
  }
  if (!pool.data) { *flag |= kFlagNoData; return false; }
  uint64_t at;
  if (pool.rebased) at = w1;
  else {
    if ((uint32_t)w1 != 0u) { *flag |= kFlagOutside; return false; }
    at = w1 >> 32;
  }
  if (at > pool.data_len || (uint64_t)len > pool.data_len - at) { *flag |= kFlagOutside; return false; }
  const unsigned char* s = pool.data + at;
  if (kind == kStartsWith) return eq_pattern(s, pat, m);
  if (kind == kEndsWith) return eq_pattern(s + (len - m), pat, m);
  for (uint32_t o = 0; o + m <= len; o++) if (eq_pattern(s + o, pat, m)) return true;
  return false;
}

// The host twin of strview_match_kernel: the same decision for n views in host memory (16 bytes each, any alignment; a length word of 0xFFFFFFFF is a null row),
// answers and validity as LSB-first bitmaps of ceil(n / 64) words with the bits past n zero.  Returns the kFlag* bits met.
inline uint32_t match_views_host(const void* views, const Pool& pool, int64_t n, int kind, const Pattern& pat, uint64_t* out_bits, uint64_t* out_valid) {
  const unsigned char* vb = (const unsigned char*)views;
  uint32_t flags = 0;
  for (int64_t w = 0; w < (n + 63) / 64; w++) { out_bits[w] = 0; out_valid[w] = 0; }
  for (int64_t i = 0; i < n; i++) {
    uint64_t w0, w1;
    __builtin_memcpy(&w0, vb + 16 * i, 8);
    __builtin_memcpy(&w1, vb + 16 * i + 8, 8);
    if ((uint32_t)w0 == 0xffffffffu) continue;
    out_valid[i >> 6] |= 1ull << (i & 63);
    if (match_view(w0, w1, pool, kind, pat, &flags)) out_bits[i >> 6] |= 1ull << (i & 63);
  }
  return flags;
}

}  // namespace strmatch
}  // namespace plx
