// kernels_encode.hip -- one-off passes that build the narrow shadow of a column (encoded_inputs.hpp; engine.cpp decides when).
//
//   affine_gcd      reduction: gcd of (v - min) over the valid rows.  A u64 gcd per lane, wave shuffle tree, LDS across the waves, one partial per workgroup, a one-
//                   workgroup finish kernel.  No atomics.
//   affine_encode   code = (v - base) / stride, eight rows per lane per step: 4 x 16-B loads, ONE 8- / 16-B store of the codes.
//   dict_collect    distinct bit patterns of an 8-byte column: every workgroup keeps an open-addressing set in LDS and gives up past kDictSlots entries by raising a
//                   flag the other workgroups look at once per tile; the sets are merged into one 2 x kDictSlots-slot table in HBM by compare-and-swap.
//   dict_encode     code = position of the row's pattern in the sorted dictionary (eight-step search in an LDS copy), eight rows per lane per step.
// Both encode kernels decode every valid row's code again and compare it with the stored value bit for bit: a shadow that disagrees with its column in one row
// raises the flag and is thrown away by the caller, whatever the reason.
#include "dev.hpp"
#include "encoded_inputs.hpp"
#include "kernels.hpp"
#include "kernels_fused.hpp"

#include <algorithm>

namespace plx {
namespace enc {

using namespace dev;
using k::kBlock;

constexpr int kRowsPerLane = 8;
constexpr unsigned long long kEmpty = ~0ull;
constexpr int kSetSlots = 1024;                        // LDS set of a workgroup: at most kDictSlots + 1 entries ever get in
constexpr int kTableSlots = 2 * fused::kDictSlots;     // the merged table in HBM

__device__ __forceinline__ unsigned long long gcd_u64(unsigned long long a, unsigned long long b) {      // gcd(x, 0) = x
  while (b) { const unsigned long long t = a % b; a = b; b = t; }
  return a;
}

// ---- affine: gcd ---------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void affine_gcd_kernel(const long long* __restrict__ v, const unsigned long long* __restrict__ validity, int64_t n, long long mn,
                                                            unsigned long long* __restrict__ partials) {
  __shared__ unsigned long long red[kBlock / 64];
  unsigned long long g = 0;
  const int64_t pairs = (n + 1) / 2;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < pairs; p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row0 = p * 2;
    long long x[2];
    if (row0 + 2 <= n) { const Pack<long long, 2> pk = load_pack<long long, 2>(v + row0); x[0] = pk.v[0]; x[1] = pk.v[1]; }
    else { x[0] = v[row0]; x[1] = x[0]; }
    unsigned vb = 3u;
    if (validity) vb = (unsigned)(validity[row0 >> 6] >> (row0 & 63)) & 3u;
    if (row0 + 2 > n) vb &= 1u;
#pragma unroll
    for (int r = 0; r < 2; r++) {
      if (!((vb >> r) & 1u)) continue;
      const unsigned long long d = (unsigned long long)x[r] - (unsigned long long)mn;
      if (g == 0 || d % g != 0) g = gcd_u64(g, d);      // (once g has settled this is one remainder per row)
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) g = gcd_u64(g, shfl_xor_u64(g, m));
  if (lane_id() == 0) red[threadIdx.x >> 6] = g;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kBlock / 64; w++) g = gcd_u64(g, red[w]);
    partials[blockIdx.x] = g;
  }
}
__global__ __launch_bounds__(kBlock) void affine_gcd_finish_kernel(const unsigned long long* __restrict__ partials, int np, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long red[kBlock / 64];
  unsigned long long g = 0;
  for (int i = threadIdx.x; i < np; i += blockDim.x) g = gcd_u64(g, partials[i]);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) g = gcd_u64(g, shfl_xor_u64(g, m));
  if (lane_id() == 0) red[threadIdx.x >> 6] = g;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kBlock / 64; w++) g = gcd_u64(g, red[w]);
    out[0] = g;
  }
}

uint64_t affine_gcd(const int64_t* values, const uint64_t* validity, int64_t n, int64_t mn) {
  if (n <= 0) return 0;
  const int grid = k::grid_for((n + 1) / 2, kBlock * 8);
  Buf partials = dev_alloc(sizeof(uint64_t) * (size_t)(grid + 1));
  unsigned long long* pp = partials->as<unsigned long long>();
  {
    ProfileScope ps("encode_affine_gcd", (uint64_t)n * 8, (uint64_t)n);
    hipLaunchKernelGGL(affine_gcd_kernel, dim3(grid), dim3(kBlock), 0, stream(), (const long long*)values, (const unsigned long long*)validity, n, (long long)mn, pp);
    PLX_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(affine_gcd_finish_kernel, dim3(1), dim3(kBlock), 0, stream(), pp, grid, pp + grid);
  PLX_HIP(hipGetLastError());
  uint64_t g = 0;
  d2h_sync(&g, pp + grid, 8);
  return g;
}

// ---- the eight rows of a lane ------------------------------------------------------------------------------------------------------------------------------------
// rows [row0, row0 + 8) of a column widened to 64 bits, row0 a multiple of 8: whole groups as vector loads, the ragged last group row by row (rows past n repeat the
// last row and are masked out of `vb`).  One byte of the bitmap covers the group.
template <class T>
__device__ __forceinline__ void load_rows8(const T* __restrict__ v, const unsigned long long* __restrict__ validity, int64_t row0, int64_t n, unsigned long long x[kRowsPerLane], unsigned& vb) {
  if (row0 + kRowsPerLane <= n) {
    constexpr int kV = sizeof(T) == 8 ? 2 : 4;      // elements of a 16-B load
#pragma unroll
    for (int j = 0; j < kRowsPerLane / kV; j++) {
      const Pack<T, kV> pk = load_pack<T, kV>(v + row0 + j * kV);
#pragma unroll
      for (int r = 0; r < kV; r++) x[j * kV + r] = (unsigned long long)(long long)pk.v[r];      // sign- or zero-extends by T
    }
  } else {
#pragma unroll
    for (int r = 0; r < kRowsPerLane; r++) { int64_t i = row0 + r; if (i > n - 1) i = n - 1; x[r] = (unsigned long long)(long long)v[i]; }
  }
  vb = 0xffu;
  if (validity) vb = (unsigned)reinterpret_cast<const unsigned char*>(validity)[row0 >> 3];
  if (row0 + kRowsPerLane > n) vb &= (1u << (unsigned)(n - row0)) - 1u;
}

// ---- affine: encode ------------------------------------------------------------------------------------------------------------------------------------------------
template <class T, class C>
__global__ __launch_bounds__(kBlock) void affine_encode_kernel(const T* __restrict__ v, const unsigned long long* __restrict__ validity, int64_t n, long long base,
                                                               unsigned long long stride, double inv_stride, C* __restrict__ codes, unsigned int* __restrict__ flag) {
  const int64_t groups = (n + kRowsPerLane - 1) / kRowsPerLane;
  constexpr unsigned long long kTop = sizeof(C) == 1 ? 255ull : 65535ull;
  bool bad = false;
  for (int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gi < groups; gi += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row0 = gi * kRowsPerLane;
    unsigned long long x[kRowsPerLane];
    unsigned vb;
    load_rows8<T>(v, validity, row0, n, x, vb);
    Pack<C, kRowsPerLane> out;
#pragma unroll
    for (int r = 0; r < kRowsPerLane; r++) {
      const unsigned long long d = x[r] - (unsigned long long)base;
      // the quotient by way of a double: exact for the multiples of `stride` an encodable column holds (quotient <= 65535, d < 2^62); anything else fails the check below
      unsigned long long q = stride == 1 ? d : (unsigned long long)__double2ull_rn((double)d * inv_stride);
      if (q > kTop) q = kTop;
      const bool valid = (vb >> r) & 1u;
      if (valid && (unsigned long long)base + q * stride != x[r]) bad = true;
      out.v[r] = valid ? (C)q : (C)0;
    }
    store_pack<C, kRowsPerLane>(codes + row0, out);      // (the buffer holds whole groups)
  }
  if (bad) flag[0] = 1u;
}

bool affine_encode(int dtype, const void* values, const uint64_t* validity, int64_t n, int64_t base, uint64_t stride, int width, void* codes) {
  if (n <= 0) return true;
  PLX_REQUIRE(stride >= 1 && (width == 1 || width == 2), PLX_ERR_INVALID, "affine_encode: stride >= 1, one- or two-byte codes");
  Buf flag = dev_alloc_zero(8);
  const int64_t groups = (n + kRowsPerLane - 1) / kRowsPerLane;
  const int grid = k::grid_for(groups, kBlock * 4);
  const double inv = 1.0 / (double)stride;
  const unsigned long long* vw = (const unsigned long long*)validity;
  unsigned int* f = flag->as<unsigned int>();
  {
    ProfileScope ps("encode_affine", (uint64_t)n * (uint64_t)(dtype_width(dtype) + width), (uint64_t)n);
#define PLX_AFFINE(T, C) hipLaunchKernelGGL((affine_encode_kernel<T, C>), dim3(grid), dim3(kBlock), 0, stream(), (const T*)values, vw, n, (long long)base, (unsigned long long)stride, inv, (C*)codes, f)
    switch (dtype) {
      case PLX_I64: if (width == 1) PLX_AFFINE(long long, uint8_t); else PLX_AFFINE(long long, uint16_t); break;
      case PLX_I32: if (width == 1) PLX_AFFINE(int32_t, uint8_t); else PLX_AFFINE(int32_t, uint16_t); break;
      case PLX_U32: if (width == 1) PLX_AFFINE(uint32_t, uint8_t); else PLX_AFFINE(uint32_t, uint16_t); break;
      default: fail(PLX_ERR_INVALID, "affine_encode: i64, i32 or u32 column required");
    }
#undef PLX_AFFINE
    PLX_HIP(hipGetLastError());
  }
  unsigned int bad = 0;
  d2h_sync(&bad, f, 4);
  return bad == 0;
}

// ---- dictionary: collect -------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned hash_pattern(unsigned long long x) { return (unsigned)((x * 0x9e3779b97f4a7c15ull) >> 40); }

// flags: [0] more than kDictSlots patterns (or the merged table is full), [1] the pattern equal to kEmpty occurs
__global__ __launch_bounds__(kBlock) void dict_collect_kernel(const unsigned long long* __restrict__ v, const unsigned long long* __restrict__ validity, int64_t n_items,
                                                              int64_t step, unsigned long long* __restrict__ table, unsigned int* __restrict__ flags) {
  __shared__ unsigned long long set[kSetSlots];
  __shared__ unsigned int s_count, s_over, s_empty;
  for (int i = threadIdx.x; i < kSetSlots; i += blockDim.x) set[i] = kEmpty;
  if (threadIdx.x == 0) { s_count = 0; s_over = 0; s_empty = 0; }
  __syncthreads();
  constexpr int kTile = 4;      // items per lane between two looks at the flag
  const int64_t per_block = (int64_t)blockDim.x * kTile;
  for (int64_t t0 = (int64_t)blockIdx.x * per_block; t0 < n_items; t0 += (int64_t)gridDim.x * per_block) {
    if (__hip_atomic_load(&flags[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) || lds_ld(&s_over)) break;
#pragma unroll
    for (int j = 0; j < kTile; j++) {
      const int64_t item = t0 + (int64_t)j * blockDim.x + threadIdx.x;
      if (item >= n_items) continue;
      const int64_t row = item * step;
      if (validity && !((validity[row >> 6] >> (row & 63)) & 1ull)) continue;
      const unsigned long long x = v[row];
      if (x == kEmpty) { lds_st(&s_empty, 1u); continue; }
      unsigned h = hash_pattern(x) & (kSetSlots - 1);
      for (int probe = 0; probe < kSetSlots; probe++) {      // (never comes near: the set stops taking patterns at kDictSlots + 1)
        unsigned long long cur = lds_ld(&set[h]);
        if (cur == x) break;
        if (cur == kEmpty) {
          if (lds_ld(&s_over)) break;
          cur = atomicCAS(&set[h], kEmpty, x);
          if (cur == kEmpty) { if (atomicAdd(&s_count, 1u) + 1u > (unsigned)fused::kDictSlots) { lds_st(&s_over, 1u); flags[0] = 1u; } break; }
          if (cur == x) break;
        }
        h = (h + 1) & (kSetSlots - 1);
      }
    }
  }
  __syncthreads();
  if (s_over) return;
  if (threadIdx.x == 0 && s_empty) flags[1] = 1u;
  for (int i = threadIdx.x; i < kSetSlots; i += blockDim.x) {
    const unsigned long long x = set[i];
    if (x == kEmpty) continue;
    unsigned h = hash_pattern(x) & (kTableSlots - 1);
    bool placed = false;
    for (int probe = 0; probe < kTableSlots && !placed; probe++) {
      unsigned long long cur = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cur == kEmpty) cur = atomicCAS(&table[h], kEmpty, x);
      placed = cur == kEmpty || cur == x;
      h = (h + 1) & (kTableSlots - 1);
    }
    if (!placed) flags[0] = 1u;
  }
}

bool dict_collect(const uint64_t* values, const uint64_t* validity, int64_t n, int64_t step, std::vector<uint64_t>* patterns) {
  patterns->clear();
  if (n <= 0) return true;
  PLX_REQUIRE(step >= 1, PLX_ERR_INVALID, "dict_collect: step >= 1");
  const int64_t n_items = (n + step - 1) / step;      // rows 0, step, .. (n_items - 1) * step < n
  Buf table = dev_alloc(sizeof(uint64_t) * kTableSlots + 8);
  k::fill_u64(table->as<uint64_t>(), kTableSlots, kEmpty);
  unsigned int* flags = reinterpret_cast<unsigned int*>(table->as<uint64_t>() + kTableSlots);
  PLX_HIP(hipMemsetAsync(flags, 0, 8, stream()));
  const int grid = k::grid_for(n_items, kBlock * 16);
  {
    ProfileScope ps(step == 1 ? "encode_dict_collect" : "encode_dict_sample", (uint64_t)n_items * 8, (uint64_t)n_items);
    hipLaunchKernelGGL(dict_collect_kernel, dim3(grid), dim3(kBlock), 0, stream(), (const unsigned long long*)values, (const unsigned long long*)validity, n_items, step,
                       table->as<unsigned long long>(), flags);
    PLX_HIP(hipGetLastError());
  }
  std::vector<uint64_t> host(kTableSlots + 1);
  d2h_sync(host.data(), table->ptr, sizeof(uint64_t) * kTableSlots + 8);
  const uint32_t over = (uint32_t)host[kTableSlots], has_empty = (uint32_t)(host[kTableSlots] >> 32);
  if (over) return false;
  for (int i = 0; i < kTableSlots; i++) if (host[i] != kEmpty) patterns->push_back(host[i]);
  if (has_empty) patterns->push_back(kEmpty);
  std::sort(patterns->begin(), patterns->end());
  return patterns->size() <= (size_t)fused::kDictSlots;
}

// ---- dictionary: encode --------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void dict_encode_kernel(const unsigned long long* __restrict__ v, const unsigned long long* __restrict__ validity, int64_t n,
                                                             const unsigned long long* __restrict__ dict, int n_dict, uint8_t* __restrict__ codes, unsigned int* __restrict__ flag) {
  __shared__ unsigned long long d[fused::kDictSlots];
  for (int i = threadIdx.x; i < fused::kDictSlots; i += blockDim.x) d[i] = dict[i < n_dict ? i : n_dict - 1];      // (padded with the largest pattern: stays sorted)
  __syncthreads();
  const int64_t groups = (n + kRowsPerLane - 1) / kRowsPerLane;
  bool bad = false;
  for (int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gi < groups; gi += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row0 = gi * kRowsPerLane;
    unsigned long long x[kRowsPerLane];
    unsigned vb;
    load_rows8<unsigned long long>(v, validity, row0, n, x, vb);
    Pack<uint8_t, kRowsPerLane> out;
#pragma unroll
    for (int r = 0; r < kRowsPerLane; r++) {
      int lo = 0;      // the last position whose pattern is <= x (position 0 when none is)
#pragma unroll
      for (int s = fused::kDictSlots / 2; s >= 1; s >>= 1) if (lo + s < n_dict && d[lo + s] <= x[r]) lo += s;
      const bool valid = (vb >> r) & 1u;
      if (valid && d[lo] != x[r]) bad = true;
      out.v[r] = valid ? (uint8_t)lo : (uint8_t)0;
    }
    store_pack<uint8_t, kRowsPerLane>(codes + row0, out);
  }
  if (bad) flag[0] = 1u;
}

bool dict_encode(const uint64_t* values, const uint64_t* validity, int64_t n, const unsigned long long* dict, int n_dict, uint8_t* codes) {
  if (n <= 0) return true;
  PLX_REQUIRE(n_dict >= 1 && n_dict <= fused::kDictSlots, PLX_ERR_INVALID, "dict_encode: 1 .. 256 dictionary entries");
  Buf flag = dev_alloc_zero(8);
  const int64_t groups = (n + kRowsPerLane - 1) / kRowsPerLane;
  const int grid = k::grid_for(groups, kBlock * 4);
  unsigned int* f = flag->as<unsigned int>();
  {
    ProfileScope ps("encode_dict", (uint64_t)n * 9, (uint64_t)n);
    hipLaunchKernelGGL(dict_encode_kernel, dim3(grid), dim3(kBlock), 0, stream(), (const unsigned long long*)values, (const unsigned long long*)validity, n, dict, n_dict, codes, f);
    PLX_HIP(hipGetLastError());
  }
  unsigned int bad = 0;
  d2h_sync(&bad, f, 4);
  return bad == 0;
}

// ---- decimal: statistics -------------------------------------------------------------------------------------------------------------------------------------------
// decimal::Stats of the items `0, step, ..`: every lane keeps its own, a wave shuffle tree and the workgroup's LDS merge them, one partial per workgroup goes to HBM and
// the host merges those.  A lane whose exponents have all failed does no more arithmetic (stats_row skips them): a column of arbitrary doubles costs one load a row.
__device__ __forceinline__ decimal::Stats stats_shfl_xor(const decimal::Stats& s, int m) {
  decimal::Stats o;
  o.fail = (uint32_t)__shfl_xor((int)s.fail, m, 64); o.any = (uint32_t)__shfl_xor((int)s.any, m, 64);
#pragma unroll
  for (int e = 0; e < decimal::kNumExp; e++) { o.mn[e] = (int64_t)shfl_xor_u64((uint64_t)s.mn[e], m); o.mx[e] = (int64_t)shfl_xor_u64((uint64_t)s.mx[e], m); }
  return o;
}
__global__ __launch_bounds__(kBlock) void decimal_stats_kernel(const double* __restrict__ v, const unsigned long long* __restrict__ validity, int64_t n_items, int64_t step,
                                                               int e_lo, int e_hi, decimal::Stats* __restrict__ partials) {
  __shared__ decimal::Stats red[kBlock / 64];
  decimal::Stats st;
  decimal::stats_init(st);
  for (int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; item < n_items; item += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = item * step;
    if (validity && !((validity[row >> 6] >> (row & 63)) & 1ull)) continue;
    decimal::stats_row(st, v[row], e_lo, e_hi);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) decimal::stats_merge(st, stats_shfl_xor(st, m));
  if (lane_id() == 0) red[threadIdx.x >> 6] = st;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kBlock / 64; w++) decimal::stats_merge(st, red[w]);
    partials[blockIdx.x] = st;
  }
}

decimal::Stats decimal_stats(const double* values, const uint64_t* validity, int64_t n, int64_t step, int e_lo, int e_hi) {
  decimal::Stats st;
  decimal::stats_init(st);
  if (n <= 0) return st;
  PLX_REQUIRE(step >= 1 && e_lo >= 0 && e_hi <= decimal::kMaxExp, PLX_ERR_INVALID, "decimal_stats: step >= 1, exponents 0..9");
  const int64_t n_items = (n + step - 1) / step;      // rows 0, step, .. (n_items - 1) * step < n
  const int grid = k::grid_for(n_items, kBlock * 16);
  Buf partials = dev_alloc(sizeof(decimal::Stats) * (size_t)grid);
  {
    ProfileScope ps(step == 1 ? "encode_decimal_stats" : "encode_decimal_sample", (uint64_t)n_items * 8, (uint64_t)n_items);
    hipLaunchKernelGGL(decimal_stats_kernel, dim3(grid), dim3(kBlock), 0, stream(), values, (const unsigned long long*)validity, n_items, step, e_lo, e_hi, partials->as<decimal::Stats>());
    PLX_HIP(hipGetLastError());
  }
  std::vector<decimal::Stats> host((size_t)grid);
  d2h_sync(host.data(), partials->ptr, sizeof(decimal::Stats) * (size_t)grid);
  for (const decimal::Stats& p : host) decimal::stats_merge(st, p);
  return st;
}

// ---- decimal: encode -----------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void decimal_encode_kernel(const unsigned long long* __restrict__ v, const unsigned long long* __restrict__ validity, int64_t n, long long base,
                                                                int e, uint32_t* __restrict__ codes, unsigned int* __restrict__ flag) {
  const int64_t groups = (n + kRowsPerLane - 1) / kRowsPerLane;
  bool bad = false;
  for (int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; gi < groups; gi += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row0 = gi * kRowsPerLane;
    unsigned long long x[kRowsPerLane];
    unsigned vb;
    load_rows8<unsigned long long>(v, validity, row0, n, x, vb);
    Pack<uint32_t, kRowsPerLane> out;
#pragma unroll
    for (int r = 0; r < kRowsPerLane; r++) {
      const bool valid = (vb >> r) & 1u;
      uint32_t code = 0;
      const bool ok = decimal::encode_row(__longlong_as_double((long long)x[r]), base, e, &code);      // (compares the decoded bits with the row's)
      if (valid && !ok) bad = true;
      out.v[r] = valid && ok ? code : 0u;
    }
    store_pack<uint32_t, kRowsPerLane>(codes + row0, out);      // (the buffer holds whole groups)
  }
  if (bad) flag[0] = 1u;
}

bool decimal_encode(const double* values, const uint64_t* validity, int64_t n, int64_t base, int e, uint32_t* codes) {
  if (n <= 0) return true;
  PLX_REQUIRE(e >= 0 && e <= decimal::kMaxExp, PLX_ERR_INVALID, "decimal_encode: exponent 0..9");
  Buf flag = dev_alloc_zero(8);
  const int64_t groups = (n + kRowsPerLane - 1) / kRowsPerLane;
  const int grid = k::grid_for(groups, kBlock * 4);
  unsigned int* f = flag->as<unsigned int>();
  {
    ProfileScope ps("encode_decimal", (uint64_t)n * 12, (uint64_t)n);
    hipLaunchKernelGGL(decimal_encode_kernel, dim3(grid), dim3(kBlock), 0, stream(), (const unsigned long long*)values, (const unsigned long long*)validity, n, (long long)base, e, codes, f);
    PLX_HIP(hipGetLastError());
  }
  unsigned int bad = 0;
  d2h_sync(&bad, f, 4);
  return bad == 0;
}

}  // namespace enc
}  // namespace plx
