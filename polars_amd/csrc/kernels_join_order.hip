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
// the secondary side of a left / right join (polars_amd.h), kNoRow travels through the sort like any row index and the validity bitmap is rebuilt afterwards.
// Full joins (PairProps::build_tail >= 0): the list is the probe side's left join followed by the tail (kNoRow, unmatched build row) in build row order, and kNoRow can
// sit on the primary side; rows without a primary index go last, in increasing index of the other side:
//   primary = probe side    the head is ordered as above and the tail stays where it is -- the run of kNoRow primaries is never shown to run_order_kernel (its run
//                           bound would send every full join into the 8-digit sort) nor to the radix
//   primary = build side    the radix runs over the whole list: kNoRow is the largest build index, so the probe-only rows end up last (in probe order: the sort is
//                           stable and they arrived in probe order, or the probe digits are sorted too), and a tail row takes its place among the matched build rows
#include "dev.hpp"
#include "join.hpp"
#include "join_keys.hpp"
#include "kernels.hpp"
#include "ops.hpp"
#include "sort.hpp"

namespace plx {
namespace join {

using namespace dev;
using k::kBlock;

namespace {
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
// sorts the pairs by digits first_digit..7 of (hi << 32 | lo); lo may be null (hi only).  n_sort (>= 0): only the first n_sort pairs, the rest stay behind them as
// they are.  Returns the digit passes run.
static int packed_sort(ColumnPtr& hi, ColumnPtr* lo, int first_digit, int64_t n_sort = -1) {
  const int64_t len = hi->len, n = n_sort >= 0 ? n_sort : len;
  PLX_REQUIRE(len < 0xffffffffll && n <= len, PLX_ERR_UNSUPPORTED, "join order: pair count exceeds u32 IdxSize");
  PLX_REQUIRE(!lo || (*lo)->len == len, PLX_ERR_SHAPE, "join order: pair columns have different lengths");
  if (n <= 1) return 0;
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
  ColumnPtr nhi = mk_idx(len), nlo = lo ? mk_idx(len) : nullptr;
  if (len > n) {
    PLX_HIP(hipMemcpyAsync(nhi->values->as<uint32_t>() + n, hi->values->as<uint32_t>() + n, (size_t)(len - n) * 4, hipMemcpyDeviceToDevice, stream()));
    if (lo) PLX_HIP(hipMemcpyAsync(nlo->values->as<uint32_t>() + n, (*lo)->values->as<uint32_t>() + n, (size_t)(len - n) * 4, hipMemcpyDeviceToDevice, stream()));
  }
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
  const bool full = props.build_tail >= 0;
  const bool nullable_build = build_idx->validity != nullptr;
  PLX_REQUIRE(full || !nullable_build || primary_probe, PLX_ERR_UNSUPPORTED, "join maintain_order: the nullable side of a left / right join cannot be the primary order");
  PLX_REQUIRE(probe_idx->len == build_idx->len, PLX_ERR_SHAPE, "join order: pair columns have different lengths");
  const int64_t n = probe_idx->len, tail = full ? props.build_tail : 0;
  PLX_REQUIRE(tail <= n, PLX_ERR_SHAPE, "join order: more unmatched build rows than pairs");
  const int64_t n_head = primary_probe ? n - tail : n;      // the pairs that are ordered: all but the tail when the probe side leads
  const std::string head = std::string("order=") + join_order_name(order) + ": ";
  std::string how;
  bool moved = false;
  if (n_head <= 1) how = "already ordered";
  else if (primary_probe && props.probe_ordered && (!secondary || props.runs_ordered)) how = "already ordered";
  else {
    int first_digit = 0;
    bool sort_needed = true;
    if (primary_probe && props.probe_ordered) {
      // chains: order the build rows of every probe row in place
      Buf flag = dev_alloc_zero(16);
      {
        ProfileScope ps("join_order_runs", (uint64_t)n_head * 12, (uint64_t)n_head);
        hipLaunchKernelGGL(run_order_kernel, dim3(k::grid_for(n_head, kBlock * 2)), dim3(kBlock), 0, stream(), probe_idx->values->as<uint32_t>(), build_idx->values->as<uint32_t>(), n_head, kRunBound,
                           flag->as<unsigned int>());
        PLX_HIP(hipGetLastError());
      }
      uint32_t f = 0;
      d2h_sync(&f, flag->ptr, 4);
      if (!f) { sort_needed = false; how = "runs of one " + std::string(probe_is_left ? "left" : "right") + " row ordered in place (insertion sort, runs <= " + std::to_string(kRunBound) + ")"; }
      else how = "a run longer than " + std::to_string(kRunBound) + ", ";
    } else if (primary_probe) first_digit = (secondary && !props.runs_ordered) ? 0 : 4;
    else if (full) first_digit = props.probe_ordered ? 4 : 0;      // the probe-only rows (kNoRow build index) go last in probe order, whether a secondary order is asked or not
    else first_digit = (props.probe_ordered || !secondary) ? 4 : 0;
    if (sort_needed) {
      ColumnPtr& prim = primary_probe ? probe_idx : build_idx;
      ColumnPtr& sec = primary_probe ? build_idx : probe_idx;
      const int passes = packed_sort(prim, &sec, first_digit, n_head);
      moved = passes > 0;
      how += std::string("radix by ") + (first_digit == 4 ? (primary_probe ? "probe row" : "build row") : (primary_probe ? "(probe row, build row)" : "(build row, probe row)")) + ", " +
             std::to_string(passes) + " passes";
    }
  }
  if (full) how += primary_probe ? "; unmatched build rows=" + std::to_string(tail) + " stay behind, in build row order"
                                 : "; unmatched build rows=" + std::to_string(tail) + " in their place, probe-only rows last";
  if (moved) {
    // rows without a partner carry the kNoRow sentinel -> validity bitmap (as join_indices / join_pairs leave it)
    if (nullable_build || full) null_out_no_row(build_idx);
    if (full) null_out_no_row(probe_idx);
  }
  if (desc) *desc = head + how;
}

}  // namespace join
}  // namespace plx
