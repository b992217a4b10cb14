// kernels_asof.hip -- join_asof on the device (the arithmetic and the contract: asof.hpp).
//
// The right side is prepared once: rows with a null key part are compacted away (the filter's route), the rest are checked for order in one pass and sorted by
// (by parts, on) -- sort::sort_indices, stable, so equal tuples keep right row order -- only when that fails.  asof_encode_kernel then writes the sorted tuples as W
// arrays of order-preserving codes, code[w][M], and every stride-th tuple as sample[w][ns].
//
// asof_search_kernel, the hot path: one lane per left row.  A workgroup copies the samples into LDS once and walks its share of the left rows 256 at a time.  A lane
// encodes its own tuple from the typed columns, finds its bound among the samples in LDS, finishes inside one stride of the global arrays, applies asof::pick and the
// tolerance, and stores the matched right row (through the map of sorted positions to right rows when there is one).  The validity goes out by ballot: lane 0 of
// every wave stores the wave's 64-bit word.  Nothing is shared between workgroups: no atomics, no waiting.  The <false> instantiation skips the sample stage and
// holds no LDS (PLX_ASOF_ROUTE=global).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "asof.hpp"
#include "dev.hpp"
#include "kernels.hpp"
#include "ops.hpp"
#include "sort.hpp"

namespace plx {
namespace asof {

using namespace dev;

// the key parts of one side as they are: typed columns
struct Part { const void* values; const uint64_t* valid; int dtype; };
template <int W> struct Parts { Part p[W]; };

template <int W> __device__ __forceinline__ bool row_valid(const Parts<W>& k, int64_t r) {
  bool ok = true;
#pragma unroll
  for (int w = 0; w < W; w++) if (k.p[w].valid) ok = ok && ((k.p[w].valid[r >> 6] >> (r & 63)) & 1);
  return ok;
}
template <int W> __device__ __forceinline__ Tuple<W> encode_row(const Parts<W>& k, int64_t r) {
  Tuple<W> t;
#pragma unroll
  for (int w = 0; w < W; w++) t.w[w] = quantile::encode_value(k.p[w].dtype, k.p[w].values, r);
  return t;
}

// flags[0]: some row sorts before the row in front of it; flags[1]: some key part holds a null.  Every writer stores the same value: no atomics.
template <int W>
__global__ __launch_bounds__(kThreads) void asof_order_check_kernel(Parts<W> k, int64_t m, unsigned int* __restrict__ flags) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
    if (!row_valid<W>(k, i)) flags[1] = 1u;
    if (i + 1 < m && tuple_less<W>(encode_row<W>(k, i + 1), encode_row<W>(k, i))) flags[0] = 1u;
  }
}

// position p of the sorted order is row perm[p] (null: row p) of the key columns
template <int W>
__global__ __launch_bounds__(kThreads) void asof_encode_kernel(Parts<W> k, const uint32_t* __restrict__ perm, int64_t m, uint64_t* __restrict__ code, uint64_t* __restrict__ sample,
                                                              int64_t stride, int64_t ns) {
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < m; p += (int64_t)gridDim.x * blockDim.x) {
    const Tuple<W> t = encode_row<W>(k, perm ? (int64_t)perm[p] : p);
    const bool is_sample = stride > 0 && p % stride == 0 && p / stride < ns;
#pragma unroll
    for (int w = 0; w < W; w++) {
      code[(int64_t)w * m + p] = t.w[w];
      if (is_sample) sample[(int64_t)w * ns + p / stride] = t.w[w];
    }
  }
}

template <int W> struct SearchArgs {
  Parts<W> left;
  const uint64_t* code;      // [W][m]
  const uint64_t* sample;    // [W][ns]
  const uint32_t* map;       // sorted position -> right row; null: the position is the row
  uint32_t* out;             // [n]
  uint64_t* out_valid;       // ceil(n / 64) words
  int64_t n, m, ns, stride;
  int how, is_float;
  Tolerance tol;
};
template <int W, bool LDS>
__global__ __launch_bounds__(kThreads) void asof_search_kernel(SearchArgs<W> a) {
  const uint64_t* sample_base = nullptr;
  int64_t ns = 0;
  if constexpr (LDS) {
    __shared__ uint64_t lds[kLdsWords];
    ns = a.ns;
    for (int64_t i = threadIdx.x; i < (int64_t)W * ns; i += kThreads) lds[i] = a.sample[i];      // ns <= samples_for(W): W * ns <= kLdsWords
    __syncthreads();
    sample_base = lds;
  }
  const Words samples{sample_base, ns}, codes{a.code, a.m};
  const int64_t tiles = (a.n + kThreads - 1) / kThreads;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t row = tile * kThreads + threadIdx.x;
    int64_t p = kNone;
    if (row < a.n && row_valid<W>(a.left, row)) p = match_row<W>(a.how, samples, ns, a.stride, codes, a.m, encode_row<W>(a.left, row), a.is_float != 0, a.tol);
    const bool hit = p != kNone;
    if (row < a.n) a.out[row] = hit ? (a.map ? a.map[p] : (uint32_t)p) : 0u;
    const uint64_t word = ballot(hit);
    const int64_t wave_row = tile * kThreads + (threadIdx.x & ~(kWaveLanes - 1));
    if ((threadIdx.x & (kWaveLanes - 1)) == 0 && wave_row < a.n) a.out_valid[wave_row >> 6] = word;
  }
}

// ---- the host route ----
namespace {
bool lds_route() {
  const char* r = std::getenv("PLX_ASOF_ROUTE");      // read per call: "global" skips the LDS sample stage, "lds" (or nothing) names the default
  return !(r && std::strcmp(r, "global") == 0);
}

template <int W> Parts<W> parts_of(const std::vector<ColumnPtr>& cols, bool with_validity) {
  Parts<W> k;
  for (int w = 0; w < W; w++) k.p[w] = Part{cols[w]->data(), with_validity ? cols[w]->valid_words() : nullptr, cols[w]->dtype};
  return k;
}

struct Prepared {
  Buf code, sample;
  ColumnPtr map;             // null: the sorted position is the right row
  int64_t m = 0, ns = 0, stride = 0, dropped = 0;
  bool sorted = false;
  std::string sort_desc;
};

// out-of-order / null flags of the rows of `cols`
template <int W> void order_check(const std::vector<ColumnPtr>& cols, bool with_validity, int64_t m, unsigned int flags[2]) {
  Buf f = dev_alloc_zero(8);
  {
    ProfileScope ps("asof_order_check", (uint64_t)m * 8 * W, (uint64_t)m);
    hipLaunchKernelGGL((asof_order_check_kernel<W>), dim3(k::grid_for(m, kThreads * 4)), dim3(kThreads), 0, stream(), parts_of<W>(cols, with_validity), m, f->as<unsigned int>());
    PLX_HIP(hipGetLastError());
  }
  d2h_sync(flags, f->ptr, 8);
}

template <int W> Prepared prepare_right(std::vector<ColumnPtr> keys, int samples) {
  Prepared pr;
  const int64_t m0 = keys[0]->len;
  unsigned int flags[2] = {0, 0};
  order_check<W>(keys, true, m0, flags);
  ColumnPtr rows;            // the usable rows' ids, when some were dropped
  if (flags[1]) {
    // AND the validities of the key parts, then the filter's compaction of the row ids and of every key column
    auto mask = std::make_shared<Column>();
    mask->dtype = PLX_BOOL; mask->len = m0; mask->null_count = 0;
    mask->values = dev_alloc_zero(bitmap_bytes(m0));
    const uint64_t* acc = nullptr;
    for (int w = 0; w < W; w++) {
      if (!keys[w]->valid_words()) continue;
      k::bitmap_and3(acc, keys[w]->valid_words(), nullptr, m0, mask->values->as<uint64_t>());
      acc = mask->values->as<uint64_t>();
    }
    auto pm = ops::prepare_mask(mask);
    const int64_t kept = ops::prepared_rows(*pm);
    pr.dropped = m0 - kept;
    if (kept == 0) return pr;
    auto iota = std::make_shared<Column>();
    iota->dtype = PLX_U32; iota->len = m0; iota->null_count = 0;
    iota->values = dev_alloc(values_bytes(PLX_U32, m0) + 16);
    k::fill_iota_u32(iota->values->as<uint32_t>(), m0);
    rows = ops::filter_prepared(iota, *pm);
    for (auto& c : keys) c = ops::filter_prepared(c, *pm);
    order_check<W>(keys, false, kept, flags);
  }
  const int64_t m = keys[0]->len;
  pr.m = m;
  ColumnPtr perm;
  if (flags[0]) {
    std::vector<sort::SortKey> sk;
    for (auto& c : keys) { sort::SortKey s; s.col = c; s.descending = false; s.nulls_last = true; sk.push_back(s); }
    perm = sort::sort_indices(sk, -1, &pr.sort_desc);
    pr.sorted = true;
  }
  pr.map = perm && rows ? ops::gather(rows, perm) : perm ? perm : rows;
  pr.stride = stride_for(m, samples);
  pr.ns = sample_count(m, pr.stride);
  pr.code = dev_alloc((size_t)W * m * 8);
  pr.sample = dev_alloc((size_t)std::max<int64_t>(W * pr.ns, 1) * 8);
  {
    ProfileScope ps("asof_encode", (uint64_t)m * 16 * W, (uint64_t)m);
    hipLaunchKernelGGL((asof_encode_kernel<W>), dim3(k::grid_for(m, kThreads * 4)), dim3(kThreads), 0, stream(), parts_of<W>(keys, false), perm ? (const uint32_t*)perm->values->as<uint32_t>() : nullptr,
                       m, pr.code->as<uint64_t>(), pr.sample->as<uint64_t>(), pr.stride, pr.ns);
    PLX_HIP(hipGetLastError());
  }
  PLX_HIP(hipStreamSynchronize(stream()));      // the compacted key columns live until the encode is done
  return pr;
}

ColumnPtr all_null(int64_t n) {
  auto out = std::make_shared<Column>();
  out->dtype = PLX_U32; out->len = n;
  out->values = dev_alloc_zero(values_bytes(PLX_U32, std::max<int64_t>(n, 1)));
  if (n > 0) { out->validity = dev_alloc_zero(bitmap_bytes(n)); out->null_count = n; } else out->null_count = 0;
  return out;
}

template <int W>
ColumnPtr match_typed(int how, const std::vector<ColumnPtr>& left, const std::vector<ColumnPtr>& right, const Tolerance& tol, std::string* desc) {
  const int64_t n = left[0]->len, m0 = right[0]->len;
  const bool lds = lds_route();
  const int samples = lds ? samples_for(W) : 0;
  const std::string head = std::string("asof[") + strategy_name(how) + (strict_of(how) ? " strict" : "") + ", by=" + std::to_string(W - 1);
  if (n == 0 || m0 == 0) { if (desc) *desc = "asof[empty]"; return all_null(n); }
  Prepared pr = prepare_right<W>(right, samples);
  if (desc) {
    *desc = head + ", right=" + (pr.sorted ? "sorted: " + pr.sort_desc : std::string("in order")) + (pr.dropped ? ", dropped null keys=" + std::to_string(pr.dropped) : "") +
            ", rows=" + std::to_string(n) + " x " + std::to_string(pr.m) + ", samples=" + std::to_string(samples) + "]";
  }
  if (pr.m == 0) return all_null(n);
  auto out = std::make_shared<Column>();
  out->dtype = PLX_U32; out->len = n;
  out->values = dev_alloc(values_bytes(PLX_U32, n) + 16);
  out->validity = dev_alloc_zero(bitmap_bytes(n));
  out->null_count = -1;
  SearchArgs<W> a;
  a.left = parts_of<W>(left, true);
  a.code = pr.code->as<uint64_t>(); a.sample = pr.sample->as<uint64_t>();
  a.map = pr.map ? pr.map->values->as<uint32_t>() : nullptr;
  a.out = out->values->as<uint32_t>(); a.out_valid = out->validity->as<uint64_t>();
  a.n = n; a.m = pr.m; a.ns = lds ? pr.ns : 0; a.stride = lds ? pr.stride : 0;
  a.how = how; a.is_float = dtype_is_float(left[W - 1]->dtype) ? 1 : 0;
  a.tol = tol;
  {
    // what the search must move: the left key parts and the index column once, and per row about log2(stride) + 1 lines of the code arrays
    ProfileScope ps(lds ? "asof_search" : "asof_search_global", (uint64_t)n * (8 * W + 4) + (uint64_t)n / 8, (uint64_t)n);
    const int grid = (int)std::min<int64_t>((n + kThreads - 1) / kThreads, (int64_t)device().cu_count * (lds ? 2 : 8));
    if (lds) hipLaunchKernelGGL((asof_search_kernel<W, true>), dim3(grid), dim3(kThreads), 0, stream(), a);
    else hipLaunchKernelGGL((asof_search_kernel<W, false>), dim3(grid), dim3(kThreads), 0, stream(), a);
    PLX_HIP(hipGetLastError());
  }
  if (column_null_count(out) == 0) out->validity = nullptr;      // (synchronises: the codes, samples and the map live until the search is done)
  return out;
}
}  // namespace

ColumnPtr match(int how, const std::vector<ColumnPtr>& left_by, const std::vector<ColumnPtr>& right_by, const ColumnPtr& left_on, const ColumnPtr& right_on, const plx_scalar* tolerance,
                std::string* desc) {
  PLX_REQUIRE(how_ok(how), PLX_ERR_INVALID, "join_asof: strategy " + std::to_string(how) + " is no plx_asof_strategy (0 = backward, 1 = forward, 2 = nearest), optionally OR'd with PLX_ASOF_STRICT (4)");
  PLX_REQUIRE(left_by.size() == right_by.size(), PLX_ERR_INVALID, "join_asof: " + std::to_string(left_by.size()) + " left by parts against " + std::to_string(right_by.size()) + " right by parts");
  PLX_REQUIRE((int)left_by.size() <= kMaxBy, PLX_ERR_UNSUPPORTED, "join_asof: " + std::to_string(left_by.size()) + " by parts; an as-of join takes 0.." + std::to_string(kMaxBy) + " by parts on this path");
  PLX_REQUIRE(left_on && right_on, PLX_ERR_INVALID, "join_asof: needs an `on` column on both sides");
  if (!on_dtype_ok(left_on->dtype) || !on_dtype_ok(right_on->dtype))
    fail(PLX_ERR_UNSUPPORTED, std::string("join_asof: `on` of dtype ") + dtype_name(on_dtype_ok(left_on->dtype) ? right_on->dtype : left_on->dtype) + "; integer, float, Date and Datetime columns only");
  PLX_REQUIRE(left_on->dtype == right_on->dtype, PLX_ERR_INVALID, std::string("join_asof: `on` is ") + dtype_name(left_on->dtype) + " on the left and " + dtype_name(right_on->dtype) + " on the right");
  std::vector<ColumnPtr> left = left_by, right = right_by;
  left.push_back(left_on); right.push_back(right_on);
  for (size_t j = 0; j + 1 < left.size(); j++) {
    PLX_REQUIRE(left[j] && right[j], PLX_ERR_INVALID, "join_asof: null by column");
    if (!by_dtype_ok(left[j]->dtype) || !by_dtype_ok(right[j]->dtype)) fail(PLX_ERR_UNSUPPORTED, "join_asof: by part " + std::to_string(j) + " is neither integer, float nor Boolean");
    PLX_REQUIRE(left[j]->dtype == right[j]->dtype, PLX_ERR_INVALID,
                "join_asof: by part " + std::to_string(j) + " is " + dtype_name(left[j]->dtype) + " on the left and " + dtype_name(right[j]->dtype) + " on the right");
    PLX_REQUIRE(left[j]->len == left_on->len && right[j]->len == right_on->len, PLX_ERR_SHAPE, "join_asof: by part " + std::to_string(j) + " and `on` have different lengths");
  }
  PLX_REQUIRE(left_on->len < 0xffffffffll && right_on->len < 0xffffffffll, PLX_ERR_UNSUPPORTED, "join_asof: more rows than u32 IdxSize");
  Tolerance tol{kNoTolerance, 0, 0.0};
  if (tolerance) {
    if (dtype_is_float(left_on->dtype)) {
      PLX_REQUIRE(tolerance->f64 >= 0.0, PLX_ERR_INVALID, "join_asof: tolerance must be a number >= 0, got " + std::to_string(tolerance->f64));
      tol = Tolerance{kFloatTolerance, 0, tolerance->f64};
    } else tol = Tolerance{kIntTolerance, tolerance->u, 0.0};
  }
  switch ((int)left.size()) {
    case 1: return match_typed<1>(how, left, right, tol, desc);
    case 2: return match_typed<2>(how, left, right, tol, desc);
    case 3: return match_typed<3>(how, left, right, tol, desc);
    case 4: return match_typed<4>(how, left, right, tol, desc);
    case 5: return match_typed<5>(how, left, right, tol, desc);
    case 6: return match_typed<6>(how, left, right, tol, desc);
    case 7: return match_typed<7>(how, left, right, tol, desc);
    default: return match_typed<8>(how, left, right, tol, desc);
  }
}

}  // namespace asof
}  // namespace plx
