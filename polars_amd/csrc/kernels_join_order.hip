// kernels_join_order.hip -- the row order of a join's pair list (plx_ir.maintain_order of PLX_IR_JOIN, JoinArgs::maintain_order of the reference).
//
// Both join paths end in a pair list (probe_idx, build_idx) that is then gathered; order_pairs puts that list into the requested order BEFORE the gathers, so the
// payload columns are touched once.  What is known about the incoming list decides the work (PairProps):
//   P  probe index non-decreasing        join_indices (emit at scanned offsets); join_pairs over every probe row / ballot candidates / filter candidates.
//                                        NOT the candidates of the partitioned probes (partition order) unless restore_candidate_order ran first.
//   C  build index increasing inside     unique build keys (at most one pair per probe row).  NOT chains (atomicExch heads: newest first, no fixed order).
//      one probe row
//   primary = probe side, P, (C or no secondary order asked)   nothing to do
//   primary = probe side, P, secondary asked, not C            every run of one probe row is ordered in place (insertion sort, runs <= kRunBound);
//                                                              a longer run anywhere -> the packed sort below on all 8 digits
//   primary = build side, P                                    STABLE key-only LSD radix of (build << 32 | probe) on the build digits only (4 passes at most): the
//                                                              probe side is increasing inside one build row because the input was in probe order
//   anything else                                              the same radix on all 8 digits of (primary << 32 | secondary)
// The radix is sort::sort_keys_u64 (kernels_sort.hip: count / scan / scatter without a permutation, 8 B read + 8 B written per pair and pass, uniform digits skipped);
// pack / unpack, the run ordering and the candidate restore are the kernels of this file.  A left join's unmatched rows carry kNoRow in build_idx; build is only ever
// the secondary side of a left join (polars_amd.h), kNoRow travels through the sort like any row index and the validity bitmap is rebuilt afterwards.
#include "dev.hpp"
#include "join.hpp"
#include "kernels.hpp"
#include "ops.hpp"
#include "sort.hpp"

namespace plx {
namespace join {

using namespace dev;
using k::kBlock;

namespace {
constexpr uint32_t kNoRowIdx = 0xffffffffu;
constexpr int kRunBound = 32;      // longest run the in-place insertion sort takes (<= 32 * 31 / 2 moves of one lane); the project's joins have runs of 1..7
}

// out[i] = hi[i] << 32 | lo[i]   (lo null: 0)
__global__ __launch_bounds__(kBlock) void pair_pack_kernel(const uint32_t* __restrict__ hi, const uint32_t* __restrict__ lo, int64_t n, uint64_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = ((uint64_t)hi[i] << 32) | (lo ? (uint64_t)lo[i] : 0ull);
}
__global__ __launch_bounds__(kBlock) void pair_unpack_kernel(const uint64_t* __restrict__ in, int64_t n, uint32_t* __restrict__ hi, uint32_t* __restrict__ lo) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t v = in[i];
    hi[i] = (uint32_t)(v >> 32);
    if (lo) lo[i] = (uint32_t)v;
  }
}
// primary[] non-decreasing: the lane at the first pair of a run (equal primary) orders the run's secondary values in place.  Runs are disjoint, so lanes never touch
// each other's pairs; a run longer than `bound` is left alone and reported through too_long[0].
__global__ __launch_bounds__(kBlock) void run_order_kernel(const uint32_t* __restrict__ primary, uint32_t* secondary, int64_t n, int bound, unsigned int* __restrict__ too_long) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t p = primary[i];
    if (i > 0 && primary[i - 1] == p) continue;
    int64_t end = i + 1;
    while (end < n && end - i <= bound && primary[end] == p) end++;
    if (end - i > bound) { too_long[0] = 1u; continue; }
    for (int64_t a = i + 1; a < end; a++) {
      const uint32_t v = secondary[a];
      int64_t b = a;
      while (b > i && secondary[b - 1] > v) { secondary[b] = secondary[b - 1]; b--; }
      if (b != a) secondary[b] = v;
    }
  }
}

static ColumnPtr mk_idx(int64_t n) {
  auto c = std::make_shared<Column>();
  c->dtype = PLX_U32; c->len = n; c->values = dev_alloc(values_bytes(PLX_U32, std::max<int64_t>(n, 1))); c->null_count = 0;
  return c;
}
// sorts the pairs by digits first_digit..7 of (hi << 32 | lo); lo may be null (hi only).  Returns the digit passes run.
static int packed_sort(ColumnPtr& hi, ColumnPtr* lo, int first_digit) {
  const int64_t n = hi->len;
  PLX_REQUIRE(n < 0xffffffffll, PLX_ERR_UNSUPPORTED, "join order: pair count exceeds u32 IdxSize");
  PLX_REQUIRE(!lo || (*lo)->len == n, PLX_ERR_SHAPE, "join order: pair columns have different lengths");
  Buf packed = dev_alloc((size_t)n * 8);
  {
    ProfileScope ps("join_order_pack", (uint64_t)n * (lo ? 16 : 12), (uint64_t)n);
    hipLaunchKernelGGL(pair_pack_kernel, dim3(k::grid_for(n, kBlock * 4)), dim3(kBlock), 0, stream(), hi->values->as<uint32_t>(), lo ? (*lo)->values->as<uint32_t>() : (const uint32_t*)nullptr, n,
                       packed->as<uint64_t>());
    PLX_HIP(hipGetLastError());
  }
  int passes = 0;
  Buf sorted = sort::sort_keys_u64(packed, n, first_digit, &passes, nullptr);
  if (passes == 0) return 0;                     // every digit uniform: the list is as it was
  ColumnPtr nhi = mk_idx(n), nlo = lo ? mk_idx(n) : nullptr;
  {
    ProfileScope ps("join_order_unpack", (uint64_t)n * (lo ? 16 : 12), (uint64_t)n);
    hipLaunchKernelGGL(pair_unpack_kernel, dim3(k::grid_for(n, kBlock * 4)), dim3(kBlock), 0, stream(), sorted->as<uint64_t>(), n, nhi->values->as<uint32_t>(),
                       nlo ? nlo->values->as<uint32_t>() : (uint32_t*)nullptr);
    PLX_HIP(hipGetLastError());
  }
  PLX_HIP(hipStreamSynchronize(stream()));       // `packed` / `sorted` are released on return
  hi = nhi;
  if (lo) *lo = nlo;
  return passes;
}

const char* join_order_name(int order) {
  switch (order) {
    case PLX_JOIN_ORDER_NONE: return "none";
    case PLX_JOIN_ORDER_LEFT: return "left";
    case PLX_JOIN_ORDER_RIGHT: return "right";
    case PLX_JOIN_ORDER_LEFT_RIGHT: return "left_right";
    case PLX_JOIN_ORDER_RIGHT_LEFT: return "right_left";
  }
  return "?";
}

bool join_order_needs_probe_order(int order, bool probe_is_left) {
  if (order == PLX_JOIN_ORDER_NONE) return false;
  const bool primary_left = order == PLX_JOIN_ORDER_LEFT || order == PLX_JOIN_ORDER_LEFT_RIGHT;
  const bool secondary = order == PLX_JOIN_ORDER_LEFT_RIGHT || order == PLX_JOIN_ORDER_RIGHT_LEFT;
  return primary_left == probe_is_left || secondary;
}

void restore_candidate_order(ColumnPtr& cand, std::string* desc) {
  PLX_REQUIRE(cand && cand->dtype == PLX_U32 && !cand->validity, PLX_ERR_INVALID, "restore_candidate_order: a non-null PLX_U32 row list");
  const int passes = cand->len > 1 ? packed_sort(cand, nullptr, 4) : 0;
  if (desc) *desc = "candidates back in row order (radix, " + std::to_string(passes) + " passes)";
}

void order_pairs(int order, bool probe_is_left, PairProps props, ColumnPtr& probe_idx, ColumnPtr& build_idx, std::string* desc) {
  PLX_REQUIRE(order >= PLX_JOIN_ORDER_NONE && order <= PLX_JOIN_ORDER_RIGHT_LEFT, PLX_ERR_INVALID, "join maintain_order outside 0..4");
  if (order == PLX_JOIN_ORDER_NONE) { if (desc) desc->clear(); return; }
  const bool primary_left = order == PLX_JOIN_ORDER_LEFT || order == PLX_JOIN_ORDER_LEFT_RIGHT;
  const bool secondary = order == PLX_JOIN_ORDER_LEFT_RIGHT || order == PLX_JOIN_ORDER_RIGHT_LEFT;
  const bool primary_probe = primary_left == probe_is_left;
  const bool nullable_build = build_idx->validity != nullptr;
  PLX_REQUIRE(!nullable_build || primary_probe, PLX_ERR_UNSUPPORTED, "join maintain_order: the nullable side of a left join cannot be the primary order");
  PLX_REQUIRE(probe_idx->len == build_idx->len, PLX_ERR_SHAPE, "join order: pair columns have different lengths");
  const int64_t n = probe_idx->len;
  const std::string head = std::string("order=") + join_order_name(order) + ": ";
  std::string how;
  bool moved = false;
  if (n <= 1) how = "already ordered";
  else if (primary_probe && props.probe_ordered && (!secondary || props.runs_ordered)) how = "already ordered";
  else {
    int first_digit = 0;
    bool sort_needed = true;
    if (primary_probe && props.probe_ordered) {
      // chains: order the build rows of every probe row in place
      Buf flag = dev_alloc_zero(16);
      {
        ProfileScope ps("join_order_runs", (uint64_t)n * 12, (uint64_t)n);
        hipLaunchKernelGGL(run_order_kernel, dim3(k::grid_for(n, kBlock * 2)), dim3(kBlock), 0, stream(), probe_idx->values->as<uint32_t>(), build_idx->values->as<uint32_t>(), n, kRunBound,
                           flag->as<unsigned int>());
        PLX_HIP(hipGetLastError());
      }
      uint32_t f = 0;
      d2h_sync(&f, flag->ptr, 4);
      if (!f) { sort_needed = false; how = "runs of one " + std::string(probe_is_left ? "left" : "right") + " row ordered in place (insertion sort, runs <= " + std::to_string(kRunBound) + ")"; }
      else how = "a run longer than " + std::to_string(kRunBound) + ", ";
    } else if (primary_probe) first_digit = (secondary && !props.runs_ordered) ? 0 : 4;
    else first_digit = (props.probe_ordered || !secondary) ? 4 : 0;
    if (sort_needed) {
      ColumnPtr& prim = primary_probe ? probe_idx : build_idx;
      ColumnPtr& sec = primary_probe ? build_idx : probe_idx;
      const int passes = packed_sort(prim, &sec, first_digit);
      moved = passes > 0;
      how += std::string("radix by ") + (first_digit == 4 ? (primary_probe ? "probe row" : "build row") : (primary_probe ? "(probe row, build row)" : "(build row, probe row)")) + ", " +
             std::to_string(passes) + " passes";
    }
  }
  if (nullable_build && moved) {
    // unmatched rows of a left join carry the kNoRow sentinel -> validity bitmap (as join_pairs leaves it)
    plx_scalar s; s.u = kNoRowIdx;
    ColumnPtr ok = ops::cmp_scalar(PLX_NE, build_idx, s);
    build_idx->validity = ok->values; build_idx->null_count = -1;
    if (column_null_count(build_idx) == 0) { build_idx->validity = nullptr; build_idx->null_count = 0; }
  }
  if (desc) *desc = head + how;
}

}  // namespace join
}  // namespace plx
