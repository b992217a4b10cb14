// kernels_strmatch.hip -- string predicates on the device: str.starts_with / ends_with / contains(literal) decided per 16-byte view, and the per-node lookup of a
// Boolean bitmap by a code column (the materialising counterpart of the fused programs' OP_BITLOOKUP).
//
// A string predicate on a dictionary column is two steps: the predicate is decided ONCE per dictionary entry (strview_match over the G views of the dictionary: G bits),
// then every row looks its code up in that bitmap -- inside the fused scan (OP_BITLOOKUP) or with bitmap_lookup_kernel.  A raw view column is decided row by row by the
// same kernel.  Both kernels have one shape: a wave owns whole 64-row words of the output bitmaps (lane l decides row 64 w + l, __ballot forms the word, lane 0 stores
// it), so no two waves ever write the same word and the bits past n in the last word are zero because their lanes vote false.
#include <hip/hip_runtime.h>

#include "core.hpp"
#include "dev.hpp"
#include "kernels.hpp"
#include "strmatch.hpp"

namespace plx {
namespace k {

using namespace dev;

namespace {
constexpr int kWordsInFlight = 4;      // 64-row words a wave decides per iteration: their four 16-byte view loads are issued before the first decision

struct StrMatchArgs {
  const unsigned long long* views;      // [n][2]
  const uint64_t* validity;             // may be null
  strmatch::Pool pool;
  int64_t n;
  uint32_t stamps;                      // 1: a view whose length word is kStrviewNullLen is a null row
  unsigned long long* out_bits;         // [ceil(n / 64)]
  unsigned long long* out_valid;        // [ceil(n / 64)]
  unsigned int* flag;                   // strmatch::kFlag* bits, OR-ed
  strmatch::Pattern pat;                // wave-uniform, in the kernel arguments: read by the scalar unit
};

// KIND (plx_str_match_kind) is a template argument: each predicate is a kernel of its own that carries only its own comparison (the thirteen windows of an inline
// `contains` are not in the instruction stream of `starts_with`)
template <int KIND>
__global__ __launch_bounds__(kBlock) void strview_match_kernel(StrMatchArgs a) {
  typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
  const int64_t n_words = (a.n + 63) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int lane = lane_id();
  uint32_t flag = 0;
  for (int64_t w0 = (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * kWordsInFlight; w0 < n_words; w0 += n_waves * kWordsInFlight) {      // (w0: wave-uniform)
    u64x2 v[kWordsInFlight];
#pragma unroll
    for (int r = 0; r < kWordsInFlight; r++) {
      const int64_t row = (w0 + r) * 64 + lane;
      v[r] = (u64x2){0ull, 0ull};
      if (row < a.n) v[r] = __builtin_nontemporal_load(reinterpret_cast<const u64x2*>(a.views) + row);
    }
#pragma unroll
    for (int r = 0; r < kWordsInFlight; r++) {
      const int64_t w = w0 + r, row = w * 64 + lane;
      if (w >= n_words) break;                                                  // (uniform)
      bool valid = row < a.n;
      if (valid && a.validity) valid = (a.validity[w] >> lane) & 1;
      if (valid && a.stamps) valid = (uint32_t)v[r].x != kStrviewNullLen;
      bool hit = false;
      if (valid) hit = strmatch::match_view(v[r].x, v[r].y, a.pool, KIND, a.pat, &flag);
      const uint64_t hb = ballot(hit), vb = ballot(valid);
      if (lane == 0) { a.out_bits[w] = hb; a.out_valid[w] = vb; }
    }
  }
  if (flag) atomicOr(a.flag, flag);
}

// code column -> bit[code] of a lookup bitmap of `range` bits (false at and beyond `range`, and for negative codes); rows the codes' validity marks null answer false
template <class T>
__global__ __launch_bounds__(kBlock) void bitmap_lookup_kernel(const T* __restrict__ codes, const uint64_t* __restrict__ validity, int64_t n, const unsigned long long* __restrict__ lut,
                                                               uint64_t range, unsigned long long* __restrict__ out_bits) {
  const int64_t n_words = (n + 63) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int lane = lane_id();
  for (int64_t w0 = (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * kWordsInFlight; w0 < n_words; w0 += n_waves * kWordsInFlight) {
    T c[kWordsInFlight];
#pragma unroll
    for (int r = 0; r < kWordsInFlight; r++) {
      const int64_t row = (w0 + r) * 64 + lane;
      c[r] = row < n ? __builtin_nontemporal_load(codes + row) : (T)0;
    }
#pragma unroll
    for (int r = 0; r < kWordsInFlight; r++) {
      const int64_t w = w0 + r, row = w * 64 + lane;
      if (w >= n_words) break;
      bool ok = row < n;
      if (ok && validity) ok = (validity[w] >> lane) & 1;
      const uint64_t idx = (uint64_t)(int64_t)c[r];                            // a negative code of a signed type becomes an index beyond every range
      const bool hit = ok && idx < range && ((lut[idx >> 6] >> (idx & 63)) & 1ull);
      const uint64_t hb = ballot(hit);
      if (lane == 0) out_bits[w] = hb;
    }
  }
}

int match_grid(int64_t n) { return grid_for((n + 63) / 64, (kBlock / 64) * kWordsInFlight, 8); }
}  // namespace

uint32_t strview_match(const uint64_t* views, const uint64_t* validity, bool stamps, const uint8_t* data, uint64_t data_len, bool rebased, int64_t n,
                       int kind, const uint8_t* pattern, int64_t pattern_len, uint64_t* out_bits, uint64_t* out_valid) {
  const int64_t n_words = (n + 63) / 64;
  // the pad word behind the last row word (bitmap_bytes) is zero like every bitmap's here
  PLX_HIP(hipMemsetAsync(out_bits + n_words, 0, 8, stream()));
  PLX_HIP(hipMemsetAsync(out_valid + n_words, 0, 8, stream()));
  if (n == 0) return 0;
  Buf flag = dev_alloc_zero(16);
  StrMatchArgs a{};
  a.views = (const unsigned long long*)views; a.validity = validity;
  a.pool = strmatch::Pool{(const unsigned char*)data, data ? data_len : 0, rebased ? 1u : 0u};
  a.n = n; a.stamps = stamps ? 1u : 0u;
  a.out_bits = (unsigned long long*)out_bits; a.out_valid = (unsigned long long*)out_valid; a.flag = flag->as<unsigned int>();
  a.pat = strmatch::make_pattern(pattern, pattern_len);
  {
    ProfileScope ps("strview_match", (uint64_t)n * 16, (uint64_t)n);
    const dim3 grid(match_grid(n)), block(kBlock);
    if (kind == strmatch::kStartsWith) hipLaunchKernelGGL((strview_match_kernel<strmatch::kStartsWith>), grid, block, 0, stream(), a);
    else if (kind == strmatch::kEndsWith) hipLaunchKernelGGL((strview_match_kernel<strmatch::kEndsWith>), grid, block, 0, stream(), a);
    else hipLaunchKernelGGL((strview_match_kernel<strmatch::kContains>), grid, block, 0, stream(), a);
    PLX_HIP(hipGetLastError());
  }
  uint32_t res[4] = {0, 0, 0, 0};
  d2h_sync(res, flag->ptr, 16);
  return res[0];
}

void bitmap_lookup(int dtype, const void* codes, const uint64_t* validity, int64_t n, const uint64_t* lut_bits, uint64_t range, uint64_t* out_bits) {
  const int64_t n_words = (n + 63) / 64;
  PLX_HIP(hipMemsetAsync(out_bits + n_words, 0, 8, stream()));
  if (n == 0) return;
  ProfileScope ps("bitmap_lookup", (uint64_t)n * (uint64_t)dtype_width(dtype) + (uint64_t)n / 8, (uint64_t)n);
  const dim3 grid(match_grid(n)), block(kBlock);
  const unsigned long long* lut = (const unsigned long long*)lut_bits;
  unsigned long long* out = (unsigned long long*)out_bits;
#define PLX_LOOKUP(T) hipLaunchKernelGGL((bitmap_lookup_kernel<T>), grid, block, 0, stream(), (const T*)codes, validity, n, lut, range, out)
  switch (dtype) {
    case PLX_U8: PLX_LOOKUP(uint8_t); break;
    case PLX_U16: PLX_LOOKUP(uint16_t); break;
    case PLX_U32: PLX_LOOKUP(uint32_t); break;
    case PLX_U64: PLX_LOOKUP(uint64_t); break;
    case PLX_I8: PLX_LOOKUP(int8_t); break;
    case PLX_I16: PLX_LOOKUP(int16_t); break;
    case PLX_I32: PLX_LOOKUP(int32_t); break;
    case PLX_I64: PLX_LOOKUP(int64_t); break;
    default: fail(PLX_ERR_INVALID, std::string("bitmap lookup: codes must be an integer column, not ") + dtype_name(dtype));
  }
#undef PLX_LOOKUP
  PLX_HIP(hipGetLastError());
}

}  // namespace k
}  // namespace plx
