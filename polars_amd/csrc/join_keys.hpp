// join_keys.hpp -- how the join kernels read a key column, and the host helpers of kernels_join.hip that every join route calls (shared by kernels_join.hip,
// kernels_join_wide.hip and kernels_join_order.hip; the table, the row loops and the driver the two hash-join routes share are join_driver.hpp).
// A key is read in its physical dtype and widened to one 64-bit word in registers (no materialised 64-bit key copy); floats are
// canonicalised (-0 -> +0, one NaN: total_ord.rs:40-48) so that equal keys have equal words.
#pragma once
#include "dev.hpp"
#include "core.hpp"

namespace plx {
namespace join {

constexpr uint64_t kEmpty = ~0ull;
constexpr uint32_t kNoRow = 0xffffffffu;
constexpr uint64_t kRandomOdd = 0x55fbfd6bfc5458e9ull;

struct KeyCol {
  const void* values;
  const uint64_t* validity;
  int dtype;
  int64_t n;
};

__device__ __forceinline__ uint64_t load_key(const KeyCol& kc, int64_t i) {
  switch (kc.dtype) {
    case PLX_I8: return (uint64_t)(long long)reinterpret_cast<const int8_t*>(kc.values)[i];
    case PLX_I16: return (uint64_t)(long long)reinterpret_cast<const int16_t*>(kc.values)[i];
    case PLX_I32: return (uint64_t)(long long)reinterpret_cast<const int32_t*>(kc.values)[i];
    case PLX_U8: return reinterpret_cast<const uint8_t*>(kc.values)[i];
    case PLX_U16: return reinterpret_cast<const uint16_t*>(kc.values)[i];
    case PLX_U32: return reinterpret_cast<const uint32_t*>(kc.values)[i];
    case PLX_F32: { float f = reinterpret_cast<const float*>(kc.values)[i]; double d = (double)f; return (d != d) ? 0x7ff8000000000000ull : (uint64_t)__double_as_longlong(d + 0.0); }
    case PLX_F64: { double d = reinterpret_cast<const double*>(kc.values)[i]; return (d != d) ? 0x7ff8000000000000ull : (uint64_t)__double_as_longlong(d + 0.0); }
    case PLX_BOOL: return (reinterpret_cast<const uint64_t*>(kc.values)[i >> 6] >> (i & 63)) & 1;
    default: return reinterpret_cast<const uint64_t*>(kc.values)[i];
  }
}
__device__ __forceinline__ bool key_valid(const KeyCol& kc, int64_t i) { return !kc.validity || ((kc.validity[i >> 6] >> (i & 63)) & 1); }

inline KeyCol key_col(const ColumnPtr& c) { KeyCol kc; kc.values = c->data(); kc.validity = c->valid_words(); kc.dtype = c->dtype; kc.n = c->len; return kc; }
inline int ceil_log2(uint64_t x) { int b = 0; while ((1ull << b) < x) b++; return b; }

// semi / anti: out_probe[offsets[i]] = i for every probe row with counts[i] != 0 (join_emit_kept_kernel, kernels_join.hip), on the current stream
void emit_kept_rows(const uint32_t* counts, const uint64_t* offsets, int64_t n, uint32_t* out_probe);
// full join (kernels_join.hip; both key routes): the build rows whose byte in matched[nb] the count pass left 0, ascending (ballots -> selection words -> the row-id
// compaction of kernels_filter.hip; *n_out of them; synchronises), and (kNoRow, row) for them written behind the first `at` pairs of the two index columns
Buf unmatched_build_rows(const uint8_t* matched, int64_t nb, int64_t* n_out);
void append_unmatched(const Buf& rows, int64_t n, int64_t at, const ColumnPtr& probe_idx, const ColumnPtr& build_idx);
// a PLX_U32 index column of n rows without nulls, values uninitialised (room for at least min_alloc_rows)
ColumnPtr make_idx_column(int64_t n, int64_t min_alloc_rows = 0);
// the kNoRow entries of an index column become nulls (validity bitmap; none when no entry is kNoRow)
void null_out_no_row(ColumnPtr& idx);

}  // namespace join
}  // namespace plx
