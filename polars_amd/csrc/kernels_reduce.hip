// kernels_reduce.hip -- whole-column reductions (sum / mean / min / max / count).
// One streaming pass computes every aggregate of a column at once (the kernel is
// HBM-bound, the extra VALU work is free): 16-B loads per lane, per-thread
// accumulators, wave64 shuffle tree, LDS across the 4 waves of a workgroup, one
// partial per workgroup, then a single-workgroup finish kernel.  No float atomics:
// results are deterministic for a given grid.
//
// Reference semantics: polars-compute/src/sum.rs:173-203 (wrapping integer sums),
// float_sum.rs:193-313 (f64 accumulation; the reference's pairwise order is not
// reproduced -- float sums are compared at 1e-6 relative), min_max/scalar.rs:23-73
// (NaN ignored unless all values are NaN), aggregate/mod.rs:240-246 (mean).
#include "dev.hpp"
#include "kernels.hpp"
#include "variance.hpp"

namespace plx {
namespace k {

using namespace dev;

struct Partial {
  uint64_t isum;
  double fsum;
  uint64_t mn, mx;  // bit patterns of T widened (ints: sign/zero extended; floats: f64)
  uint64_t n_valid, n_ordered;
};

template <class T> struct Wide { using type = long long; };
template <> struct Wide<uint8_t> { using type = unsigned long long; };
template <> struct Wide<uint16_t> { using type = unsigned long long; };
template <> struct Wide<uint32_t> { using type = unsigned long long; };
template <> struct Wide<uint64_t> { using type = unsigned long long; };
template <> struct Wide<float> { using type = double; };
template <> struct Wide<double> { using type = double; };

template <class W> __device__ __forceinline__ uint64_t to_bits(W w) {
  if constexpr (is_fp<W>::value) return (uint64_t)__double_as_longlong((double)w); else return (uint64_t)w;
}
template <class W> __device__ __forceinline__ W from_bits(uint64_t b) {
  if constexpr (is_fp<W>::value) return (W)__longlong_as_double((long long)b); else return (W)b;
}

template <class W>
struct Acc {
  uint64_t isum = 0; double fsum = 0.0; W mn, mx; uint64_t nv = 0, no = 0; bool have = false;
  __device__ __forceinline__ void add(W x) {
    nv++;
    if constexpr (is_fp<W>::value) { fsum += x; if (x == x) { no++; if (!have) { mn = mx = x; have = true; } else { mn = x < mn ? x : mn; mx = x > mx ? x : mx; } } }
    else { isum += (uint64_t)x; fsum += (double)x; no++; if (!have) { mn = mx = x; have = true; } else { mn = x < mn ? x : mn; mx = x > mx ? x : mx; } }
  }
  __device__ __forceinline__ void merge(uint64_t oisum, double ofsum, W omn, W omx, uint64_t onv, uint64_t ono) {
    isum += oisum; fsum += ofsum; nv += onv;
    if (ono) { if (!no) { mn = omn; mx = omx; } else { mn = omn < mn ? omn : mn; mx = omx > mx ? omx : mx; } }
    no += ono; have = no > 0;
  }
};

template <class W>
__device__ __forceinline__ void block_reduce_store(Acc<W>& acc, Partial* out) {
  // wave tree
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    uint64_t oi = shfl_xor_u64(acc.isum, m);
    double of = shfl_xor_f64(acc.fsum, m);
    uint64_t omn = shfl_xor_u64(to_bits<W>(acc.no ? acc.mn : (W)0), m);
    uint64_t omx = shfl_xor_u64(to_bits<W>(acc.no ? acc.mx : (W)0), m);
    uint64_t onv = shfl_xor_u64(acc.nv, m);
    uint64_t ono = shfl_xor_u64(acc.no, m);
    acc.merge(oi, of, from_bits<W>(omn), from_bits<W>(omx), onv, ono);
  }
  __shared__ Partial sh[kBlock / 64];
  const int wave = threadIdx.x >> 6;
  if (lane_id() == 0) {
    sh[wave].isum = acc.isum; sh[wave].fsum = acc.fsum; sh[wave].mn = to_bits<W>(acc.no ? acc.mn : (W)0); sh[wave].mx = to_bits<W>(acc.no ? acc.mx : (W)0);
    sh[wave].n_valid = acc.nv; sh[wave].n_ordered = acc.no;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    Acc<W> t;
    for (int w = 0; w < (int)(blockDim.x >> 6); w++) t.merge(sh[w].isum, sh[w].fsum, from_bits<W>(sh[w].mn), from_bits<W>(sh[w].mx), sh[w].n_valid, sh[w].n_ordered);
    out->isum = t.isum; out->fsum = t.fsum; out->mn = to_bits<W>(t.no ? t.mn : (W)0); out->mx = to_bits<W>(t.no ? t.mx : (W)0);
    out->n_valid = t.nv; out->n_ordered = t.no;
  }
}

// Each wave owns runs of 64*V rows so the validity word(s) of a run are wave-uniform.
template <class T>
__global__ __launch_bounds__(kBlock) void reduce_kernel(const T* __restrict__ v, const uint64_t* __restrict__ valid, int64_t n,
                                                        Partial* __restrict__ partials) {
  using W = typename Wide<T>::type;
  constexpr int V = 16 / sizeof(T);
  Acc<W> acc;
  const int lane = lane_id();
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t run = 64 * V;              // rows per wave-iteration
  const int64_t nruns = n / run;
  for (int64_t r = wave; r < nruns; r += nwaves) {
    const int64_t base = r * run + (int64_t)lane * V;
    Pack<T, V> p = load_pack<T, V>(v + base);
    if (valid) {
      // rows base..base+V-1 live in one 64-bit word (V divides 64)
      uint64_t word = valid[base >> 6] >> (base & 63);
#pragma unroll
      for (int j = 0; j < V; j++) if ((word >> j) & 1) acc.add((W)p.v[j]);
    } else {
#pragma unroll
      for (int j = 0; j < V; j++) acc.add((W)p.v[j]);
    }
  }
  // tail rows
  for (int64_t i = nruns * run + ((int64_t)blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (!valid || ((valid[i >> 6] >> (i & 63)) & 1)) acc.add((W)v[i]);
  }
  block_reduce_store<W>(acc, partials + blockIdx.x);
}

template <class W>
__global__ __launch_bounds__(kBlock) void reduce_finish_kernel(const Partial* __restrict__ partials, int np, Partial* __restrict__ out) {
  Acc<W> acc;
  for (int i = threadIdx.x; i < np; i += blockDim.x) {
    const Partial& p = partials[i];
    acc.merge(p.isum, p.fsum, from_bits<W>(p.mn), from_bits<W>(p.mx), p.n_valid, p.n_ordered);
  }
  block_reduce_store<W>(acc, out);
}

template <class T>
static ReduceResult reduce_typed(const void* values, const uint64_t* validity, int64_t n) {
  using W = typename Wide<T>::type;
  constexpr int V = 16 / sizeof(T);
  int grid = grid_for(n, kBlock * V * 4);
  Buf partials = dev_alloc(sizeof(Partial) * (size_t)(grid + 1));
  hipLaunchKernelGGL((reduce_kernel<T>), dim3(grid), dim3(kBlock), 0, stream(), (const T*)values, validity, n, partials->as<Partial>());
  hipLaunchKernelGGL((reduce_finish_kernel<W>), dim3(1), dim3(kBlock), 0, stream(), partials->as<Partial>(), grid, partials->as<Partial>() + grid);
  PLX_HIP(hipGetLastError());
  Partial h;
  d2h_sync(&h, partials->as<Partial>() + grid, sizeof(Partial));
  ReduceResult r;
  r.isum = h.isum; r.fsum = h.fsum; r.minmax_lo = h.mn; r.minmax_hi = h.mx; r.n_valid = h.n_valid; r.n_ordered = h.n_ordered;
  return r;
}

ReduceResult reduce_all(int dtype, const void* values, const uint64_t* validity, int64_t n) {
  ProfileScope ps("reduce_all", (uint64_t)n * dtype_width(dtype) + (validity ? (uint64_t)n / 8 : 0), (uint64_t)n);
  if (n == 0) { ReduceResult r; memset(&r, 0, sizeof(r)); return r; }
  switch (dtype) {
    case PLX_I8: return reduce_typed<int8_t>(values, validity, n);
    case PLX_I16: return reduce_typed<int16_t>(values, validity, n);
    case PLX_I32: return reduce_typed<int32_t>(values, validity, n);
    case PLX_I64: return reduce_typed<int64_t>(values, validity, n);
    case PLX_U8: return reduce_typed<uint8_t>(values, validity, n);
    case PLX_U16: return reduce_typed<uint16_t>(values, validity, n);
    case PLX_U32: return reduce_typed<uint32_t>(values, validity, n);
    case PLX_U64: return reduce_typed<uint64_t>(values, validity, n);
    case PLX_F32: return reduce_typed<float>(values, validity, n);
    case PLX_F64: return reduce_typed<double>(values, validity, n);
    default: fail(PLX_ERR_UNSUPPORTED, "reduce: unsupported dtype");
  }
}

// ---- var / std -------------------------------------------------------------------------------------------------------------
// reduce_kernel's shape (16-B loads, wave-uniform validity words, runs + tail, one partial per workgroup, a single-workgroup finish kernel, no atomics), another
// accumulator: a lane sums d = x - p and d * d about ITS OWN first valid value p (no division per element, and no cancellation whatever offset the column carries),
// converts once (variance::from_shifted) and from there on every combination -- wave tree, LDS, finish kernel -- is Chan's merge (variance.hpp).
// The means that the merges subtract are kept RELATIVE TO THE COLUMN'S FIRST VALID VALUE p0 (var_pivot_kernel, one workgroup in front): a mean near 1e15 is only
// representable to 0.06, and a merge that saw such means would err by n * 0.06^2 -- relative to p0 they are as small as the column's range and carry its precision.
// Only the finish kernel's output is absolute again.
struct VarAcc {
  double p = 0.0, s1 = 0.0, s2 = 0.0;
  uint64_t n = 0;
  __device__ __forceinline__ void add(double x) {
    if (n == 0) p = x;
    const double d = x - p;
    s1 += d; s2 += d * d; n++;
  }
  // n, mean - origin, m2
  __device__ __forceinline__ variance::Moments moments(double origin) const {
    variance::Moments m;
    m.n = (double)n;
    m.mean = n ? (p - origin) + s1 / (double)n : 0.0;
    m.m2 = variance::from_shifted((double)n, s1, s2);
    return m;
  }
};

__device__ __forceinline__ void block_merge_store(variance::Moments m, variance::Moments* out, double add_to_mean) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    variance::Moments o;
    o.n = shfl_xor_f64(m.n, s); o.mean = shfl_xor_f64(m.mean, s); o.m2 = shfl_xor_f64(m.m2, s);
    // both lanes of a pair combine (low lane, high lane) in that order: every lane of the wave ends with the same bits
    m = (lane_id() & s) ? variance::merge(o, m) : variance::merge(m, o);
  }
  __shared__ variance::Moments sh[kBlock / 64];
  if (lane_id() == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    variance::Moments t = sh[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); w++) t = variance::merge(t, sh[w]);
    if (t.n > 0.0) t.mean += add_to_mean;
    *out = t;
  }
}

// *p0 = the first valid value among the column's first kVarOriginRows rows as f64 (0 when there is none).  One workgroup walks the validity words kBlock at a time
// and stops at the first stretch that holds a set bit -- the first word of nearly every column -- and after kVarOriginSteps stretches at the latest: the search is
// serial (two barriers a step), and a column that opens with 2^27 nulls must not pay 16 000 of them in front of a 0.4 ms kernel.  Any origin is CORRECT; one near the
// data is what makes the result robust to a common offset, so a column with more than 2^20 leading nulls gets the accuracy of plain f64 means (origin 0) instead
template <class T>
__global__ __launch_bounds__(kBlock) void var_pivot_kernel(const T* __restrict__ v, const uint64_t* __restrict__ valid, int64_t n, double* __restrict__ p0) {
  using W = typename Wide<T>::type;
  constexpr unsigned long long kNoRow = ~0ull;
  constexpr int64_t kVarOriginSteps = 64;      // x kBlock words x 64 rows = the first 2^20 rows
  __shared__ unsigned long long sh_first[kBlock / 64];
  unsigned long long found = valid ? kNoRow : 0ull;
  if (valid) {
    const int64_t nwords = (n + 63) >> 6;
    const int64_t wend = nwords < kVarOriginSteps * (int64_t)blockDim.x ? nwords : kVarOriginSteps * (int64_t)blockDim.x;
    for (int64_t w0 = 0; w0 < wend; w0 += blockDim.x) {      // (block-uniform trip count and exit)
      const int64_t w = w0 + threadIdx.x;
      uint64_t word = w < nwords ? valid[w] : 0ull;
      if (w == nwords - 1 && (n & 63)) word &= (1ull << (n & 63)) - 1ull;      // pad bits of the last word
      unsigned long long cand = word ? (unsigned long long)w * 64ull + (unsigned long long)(__ffsll((long long)word) - 1) : kNoRow;
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) { const unsigned long long o = shfl_xor_u64(cand, s); cand = o < cand ? o : cand; }
      if (lane_id() == 0) sh_first[threadIdx.x >> 6] = cand;
      __syncthreads();
      for (int k2 = 0; k2 < (int)(blockDim.x >> 6); k2++) found = sh_first[k2] < found ? sh_first[k2] : found;
      __syncthreads();
      if (found != kNoRow) break;
    }
  }
  if (threadIdx.x == 0) *p0 = (found != kNoRow && (int64_t)found < n) ? (double)(W)v[found] : 0.0;
}

template <class T>
__global__ __launch_bounds__(kBlock) void var_kernel(const T* __restrict__ v, const uint64_t* __restrict__ valid, int64_t n, const double* __restrict__ p0,
                                                     variance::Moments* __restrict__ partials) {
  using W = typename Wide<T>::type;
  constexpr int V = 16 / sizeof(T);
  VarAcc acc;
  const int lane = lane_id();
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t run = 64 * V;
  const int64_t nruns = n / run;
  for (int64_t r = wave; r < nruns; r += nwaves) {
    const int64_t base = r * run + (int64_t)lane * V;
    Pack<T, V> p = load_pack<T, V>(v + base);
    if (valid) {
      uint64_t word = valid[base >> 6] >> (base & 63);
#pragma unroll
      for (int j = 0; j < V; j++) if ((word >> j) & 1) acc.add((double)(W)p.v[j]);
    } else {
#pragma unroll
      for (int j = 0; j < V; j++) acc.add((double)(W)p.v[j]);
    }
  }
  for (int64_t i = nruns * run + ((int64_t)blockIdx.x * blockDim.x + threadIdx.x); i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (!valid || ((valid[i >> 6] >> (i & 63)) & 1)) acc.add((double)(W)v[i]);
  }
  block_merge_store(acc.moments(*p0), partials + blockIdx.x, 0.0);
}

// partials hold means relative to *p0; the one Moments this writes holds the absolute mean
__global__ __launch_bounds__(kBlock) void var_finish_kernel(const variance::Moments* __restrict__ partials, int np, const double* __restrict__ p0, variance::Moments* __restrict__ out) {
  variance::Moments m{0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < np; i += blockDim.x) m = variance::merge(m, partials[i]);
  block_merge_store(m, out, *p0);
}

template <class T>
static variance::Moments var_typed(const void* values, const uint64_t* validity, int64_t n) {
  constexpr int V = 16 / sizeof(T);
  const int grid = grid_for(n, kBlock * V * 4);
  Buf partials = dev_alloc(sizeof(variance::Moments) * (size_t)(grid + 2));      // [grid] partials, the result, p0 (in the first word of one more entry)
  variance::Moments* pp = partials->as<variance::Moments>();
  double* p0 = reinterpret_cast<double*>(pp + grid + 1);
  hipLaunchKernelGGL((var_pivot_kernel<T>), dim3(1), dim3(kBlock), 0, stream(), (const T*)values, validity, n, p0);
  hipLaunchKernelGGL((var_kernel<T>), dim3(grid), dim3(kBlock), 0, stream(), (const T*)values, validity, n, (const double*)p0, pp);
  hipLaunchKernelGGL(var_finish_kernel, dim3(1), dim3(kBlock), 0, stream(), (const variance::Moments*)pp, grid, (const double*)p0, pp + grid);
  PLX_HIP(hipGetLastError());
  variance::Moments h;
  d2h_sync(&h, partials->as<variance::Moments>() + grid, sizeof(h));
  return h;
}

variance::Moments reduce_var(int dtype, const void* values, const uint64_t* validity, int64_t n) {
  ProfileScope ps("reduce_var", (uint64_t)n * dtype_width(dtype) + (validity ? (uint64_t)n / 8 : 0), (uint64_t)n);
  if (n == 0) return variance::Moments{0.0, 0.0, 0.0};
  switch (dtype) {
    case PLX_I8: return var_typed<int8_t>(values, validity, n);
    case PLX_I16: return var_typed<int16_t>(values, validity, n);
    case PLX_I32: return var_typed<int32_t>(values, validity, n);
    case PLX_I64: return var_typed<int64_t>(values, validity, n);
    case PLX_U8: return var_typed<uint8_t>(values, validity, n);
    case PLX_U16: return var_typed<uint16_t>(values, validity, n);
    case PLX_U32: return var_typed<uint32_t>(values, validity, n);
    case PLX_U64: return var_typed<uint64_t>(values, validity, n);
    case PLX_F32: return var_typed<float>(values, validity, n);
    case PLX_F64: return var_typed<double>(values, validity, n);
    default: fail(PLX_ERR_UNSUPPORTED, std::string("var / std: unsupported dtype ") + dtype_name(dtype));
  }
}

}  // namespace k
}  // namespace plx
