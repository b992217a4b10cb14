// kernels_window.hip -- the way back from a group frame to the rows: `expr.over(keys)` (the arithmetic: window.hpp).
//
// Reference behaviour (restated, not ported): WindowExpr with mapping group_to_rows evaluates the function per group and scatters the group values back through the
// groups' row lists (polars-expr/src/expressions/window.rs).  GPU shape: the group-by has run already (engine.cpp groupby_columns); what is left is a map row -> group
// and one streaming pass that writes every window column of the node.
//   direct : the keys' joint code range R is dense: window_slots_kernel writes slot[code(keys of group g)] = g (one lane per group, no memset: every code among the
//            rows occurs among the groups) and the broadcast computes the row's code and reads slot[code].  4 R bytes of table, L2-sized or row-proportional by the
//            route rule (window::direct_route_ok).
//   sorted : everything else: one sort_indices of the rows by the keys, the segment heads and their per-word prefix (sort::segment_head_ranks), the group frame's keys
//            sorted the same way, and window_group_ids_kernel writes gid[perm[i]] = order[segment of i].
//   broadcast: a lane owns a row, a wave 64 consecutive rows; the row's group is found once, then every output copies the 1-, 2-, 4- or 8-byte value of that group
//            (coalesced full-width stores).  A validity word (and a Boolean output's value word) is the wave's ballot, stored whole by one lane: no atomics, no
//            read-modify-write of bitmaps; lanes past the last row vote 0, which masks the tail wave's words.  Up to window::kMaxOutputs columns per launch.
// A row whose group is not below G (keys outside the bounds a caller declared) raises a device flag that the host reads once after the launches.
#include <algorithm>

#include "dev.hpp"
#include "kernels.hpp"
#include "ops.hpp"
#include "sort.hpp"
#include "window.hpp"

namespace plx {
namespace window {

using namespace dev;
using k::kBlock;

__global__ __launch_bounds__(kBlock) void window_slots_kernel(Keys gk, int64_t n_groups, uint32_t* __restrict__ slot, unsigned int* __restrict__ flag) {
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n_groups; g += (int64_t)gridDim.x * blockDim.x)
    if (!slot_store(gk, g, slot)) *flag = 1u;
}

__global__ __launch_bounds__(kBlock) void window_group_ids_kernel(const uint32_t* __restrict__ perm, const uint64_t* __restrict__ prefix, const uint64_t* __restrict__ heads,
                                                                  const uint32_t* __restrict__ order, int64_t n, int64_t n_groups, uint32_t* __restrict__ gid,
                                                                  unsigned int* __restrict__ flag) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t r = perm[i];
    const uint32_t g = sorted_group(prefix, heads, order, (uint64_t)n_groups, (uint64_t)i);
    if ((int64_t)r < n && (int64_t)g < n_groups) gid[r] = g; else *flag = 1u;
  }
}

// kDirect: `table` = slot[R], the row's group is slot[code(row)]; else `table` = gid[n]
template <bool kDirect>
__global__ __launch_bounds__(kBlock) void window_broadcast_kernel(Keys keys, const uint32_t* __restrict__ table, int64_t n, int64_t n_groups, Outputs outs,
                                                                  unsigned int* __restrict__ flag) {
  const int64_t n_tiles = (n + 63) >> 6;
  const int lane = threadIdx.x & 63;
  constexpr int kWaves = kBlock / kWave;
  for (int64_t tile = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); tile < n_tiles; tile += (int64_t)gridDim.x * kWaves) {
    const int64_t r = tile * 64 + lane;
    uint64_t g = 0;
    bool ok = false;
    if (r < n) {
      if constexpr (kDirect) {
        uint64_t code;
        if (row_code(keys, r, &code)) { g = table[code]; ok = g < (uint64_t)n_groups; }
      } else {
        g = table[r];
        ok = g < (uint64_t)n_groups;
      }
      if (!ok) *flag = 1u;
    }
#pragma unroll
    for (int j = 0; j < kMaxOutputs; j++) {
      if (j < outs.n) {
        const Output& o = outs.o[j];
        const unsigned b = lane_bits(o, ok, g);
        if (o.width) { if (ok) copy_value(o.width, o.src, g, o.dst, r); }
        else {
          const uint64_t m = ballot((b & 2u) != 0);
          if (lane == 0) reinterpret_cast<uint64_t*>(o.dst)[tile] = m;
        }
        if (o.dst_valid) {
          const uint64_t m = ballot((b & 1u) != 0);
          if (lane == 0) o.dst_valid[tile] = m;
        }
      }
    }
  }
}

static bool force_sorted_route() {
  const char* e = getenv("PLX_WINDOW_ROUTE");      // read at every call: the tests switch it.  "direct" asks for what the rule gives already
  return e && std::string(e) == "sort";
}

static unsigned int* new_flag(Buf& keep) { keep = dev_alloc_zero(8); return keep->as<unsigned int>(); }

RowMap map_rows(const std::vector<ColumnPtr>& keys, const std::vector<ColumnPtr>& group_keys) {
  PLX_REQUIRE(!keys.empty() && (int)keys.size() <= kMaxKeys, PLX_ERR_UNSUPPORTED, "window: " + std::to_string(keys.size()) + " keys; a window takes 1.." + std::to_string(kMaxKeys) + " keys on this path");
  PLX_REQUIRE(group_keys.size() == keys.size(), PLX_ERR_INVALID, "window: the group frame has another number of keys");
  RowMap m;
  const int64_t n = m.n = keys[0]->len, G = m.n_groups = group_keys[0]->len;
  PLX_REQUIRE(n < 0xffffffffll - 1, PLX_ERR_UNSUPPORTED, "window: more rows than u32 IdxSize");
  for (size_t j = 0; j < keys.size(); j++) {
    PLX_REQUIRE(keys[j]->len == n && group_keys[j]->len == G, PLX_ERR_SHAPE, "window: key columns have different lengths");
    PLX_REQUIRE(keys[j]->dtype == group_keys[j]->dtype, PLX_ERR_INVALID, "window: the group frame's keys differ in dtype from the rows' keys");
    PLX_REQUIRE(keys[j]->values || n == 0, PLX_ERR_INVALID, "placeholder column has no data");
  }
  m.flag_ptr = new_flag(m.flag);
  if (n == 0) { m.desc = "window[empty]"; return m; }
  // ---- direct: every part an integer / Boolean with a known range, the joint range inside the rule ----
  bool direct = !force_sorted_route();
  uint64_t ranges[kMaxKeys];
  Keys rk{};
  rk.n_parts = (int)keys.size();
  for (size_t j = 0; j < keys.size() && direct; j++) {
    const ColumnPtr& c = keys[j];
    KeyPart& p = rk.part[j];
    if (!part_ok(c->dtype)) { direct = false; break; }
    p.values = c->data(); p.validity = c->valid_words(); p.dtype = c->dtype; p.nullable = c->validity ? 1 : 0;
    if (c->dtype == PLX_BOOL) { p.min = 0; p.span = 2; }
    else {
      int64_t mn = 0, mx = 0;
      if (ops::int_range(c, &mn, &mx)) {      // the cached statistics; one min / max pass when nobody knows them yet
        p.min = mn; p.span = (uint64_t)mx - (uint64_t)mn + 1;
        if (p.span == 0) { direct = false; break; }      // all of i64
      } else { p.min = 0; p.span = 0; }                   // no valid row: the null code alone
    }
    ranges[j] = p.span + (uint64_t)p.nullable;
  }
  if (direct) {
    const uint64_t R = joint_range(ranges, rk.n_parts, ~0ull >> 2);
    direct = direct_route_ok(R, (uint64_t)n);
    rk.range = R;
  }
  if (direct) {
    uint64_t stride = 1;
    for (int j = 0; j < rk.n_parts; j++) { rk.part[j].stride = stride; stride *= ranges[j]; }
    Keys gk = rk;
    for (int j = 0; j < rk.n_parts; j++) { gk.part[j].values = group_keys[j]->data(); gk.part[j].validity = group_keys[j]->valid_words(); }
    m.table = dev_alloc((size_t)rk.range * 4);
    {
      ProfileScope ps("window_slots", (uint64_t)G * 12, (uint64_t)G);
      hipLaunchKernelGGL(window_slots_kernel, dim3(k::grid_for(G, kBlock)), dim3(kBlock), 0, stream(), gk, G, m.table->as<uint32_t>(), m.flag_ptr);
      PLX_HIP(hipGetLastError());
    }
    m.direct = true;
    m.keys = rk;
    m.key_cols = keys;
    m.desc = "window[direct range=" + std::to_string(rk.range) + "]";
    return m;
  }
  // ---- sorted ----
  std::vector<sort::SortKey> sk, gk;
  for (const ColumnPtr& c : keys) { sort::SortKey s; s.col = c; s.nulls_last = true; sk.push_back(s); }
  for (const ColumnPtr& c : group_keys) { sort::SortKey s; s.col = c; s.nulls_last = true; gk.push_back(s); }
  std::string sd;
  ColumnPtr perm = sort::sort_indices(sk, -1, &sd);
  const sort::HeadRanks hr = sort::segment_head_ranks(keys, perm);
  PLX_REQUIRE(hr.n_segments == G, PLX_ERR_INVALID, "window: segment count mismatch (" + std::to_string(hr.n_segments) + " segments, " + std::to_string(G) + " groups)");
  ColumnPtr order = sort::sort_indices(gk, -1, nullptr);
  m.table = dev_alloc((size_t)n * 4);
  {
    ProfileScope ps("window_group_ids", (uint64_t)n * 8 + (uint64_t)n / 4, (uint64_t)n);
    hipLaunchKernelGGL(window_group_ids_kernel, dim3(k::grid_for(n, kBlock * 4)), dim3(kBlock), 0, stream(), perm->values->as<uint32_t>(), hr.prefix->as<uint64_t>(), hr.heads->as<uint64_t>(),
                       order->values->as<uint32_t>(), n, G, m.table->as<uint32_t>(), m.flag_ptr);
    PLX_HIP(hipGetLastError());
  }
  PLX_HIP(hipStreamSynchronize(stream()));      // perm, the heads and the order live until the kernel that reads them is done
  m.desc = "window[sorted rows: " + sd + "]";
  return m;
}

std::vector<ColumnPtr> broadcast(const RowMap& m, const std::vector<ColumnPtr>& group_cols) {
  const int64_t n = m.n, G = m.n_groups;
  std::vector<ColumnPtr> out;
  for (const ColumnPtr& gc : group_cols) {
    PLX_REQUIRE(gc->len == G, PLX_ERR_SHAPE, "window: a group column of " + std::to_string(gc->len) + " rows for " + std::to_string(G) + " groups");
    const int w = dtype_width(gc->dtype);
    PLX_REQUIRE(gc->dtype == PLX_BOOL || w == 1 || w == 2 || w == 4 || w == 8, PLX_ERR_UNSUPPORTED, std::string("window: a ") + dtype_name(gc->dtype) + " group column");
    auto c = std::make_shared<Column>();
    c->dtype = gc->dtype; c->len = n;
    c->values = dev_alloc(values_bytes(gc->dtype, std::max<int64_t>(n, 1)));
    const bool nulls = gc->validity && column_null_count(gc) > 0;
    if (nulls) { c->validity = dev_alloc(bitmap_bytes(n)); c->null_count = -1; } else c->null_count = 0;
    out.push_back(c);
  }
  if (n == 0) return out;
  const int64_t n_tiles = (n + 63) >> 6;
  const int grid = k::grid_for(n_tiles, kBlock / kWave);
  for (size_t b0 = 0; b0 < group_cols.size(); b0 += (size_t)kMaxOutputs) {
    Outputs o{};
    uint64_t bytes = 0;
    for (size_t j = b0; j < group_cols.size() && j < b0 + (size_t)kMaxOutputs; j++) {
      Output& x = o.o[o.n++];
      x.src = group_cols[j]->data(); x.src_valid = out[j]->validity ? group_cols[j]->valid_words() : nullptr;
      x.dst = out[j]->values->ptr; x.dst_valid = out[j]->validity ? out[j]->validity->as<uint64_t>() : nullptr;
      x.width = dtype_width(group_cols[j]->dtype);
      bytes += (uint64_t)n * (uint64_t)std::max(x.width, 1);
    }
    ProfileScope ps("window_broadcast", bytes + (uint64_t)n * 8, (uint64_t)n);
    if (m.direct) hipLaunchKernelGGL(window_broadcast_kernel<true>, dim3(grid), dim3(kBlock), 0, stream(), m.keys, m.table->as<uint32_t>(), n, G, o, m.flag_ptr);
    else hipLaunchKernelGGL(window_broadcast_kernel<false>, dim3(grid), dim3(kBlock), 0, stream(), m.keys, m.table->as<uint32_t>(), n, G, o, m.flag_ptr);
    PLX_HIP(hipGetLastError());
  }
  unsigned int bad = 0;
  d2h_sync(&bad, m.flag_ptr, 4);      // read once, after the launches
  PLX_REQUIRE(!bad, PLX_ERR_INVALID, "window: a row has no group among the " + std::to_string(G) + " groups (key values outside the bounds declared for their column?)");
  return out;
}

}  // namespace window
}  // namespace plx
