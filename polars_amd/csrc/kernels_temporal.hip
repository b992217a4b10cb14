// kernels_temporal.hip -- the parts of a Date / Datetime column per node (dt.year(), dt.month(), ...): the materialising counterpart of the fused programs'
// OP_DATEPART, for select / with_columns / Series.dt and for plans that do not fuse.  The arithmetic is temporal.hpp's (one body with the fused programs and the host
// entry); this file only moves the data.
//
// One kernel per (unit, part): the unit fixes the input width and every divisor, the part the output width, so each instantiation carries one part's multiply-high
// chain and nothing else.  A lane owns 4 consecutive rows per step: one 16-byte load of a Date column (two of a Datetime column) and ONE store of the 4 narrow
// results (4 B of Int8, 8 B of Int16, 16 B of Int32).  No validity is read: the result shares the input's bitmap (ops::temporal_part), and the value under a null is
// whatever the arithmetic makes of the bytes there -- it is defined for every input.  The up to 3 rows behind the last whole quad go to the first lanes one by one.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "core.hpp"
#include "dev.hpp"
#include "kernels.hpp"
#include "temporal.hpp"

namespace plx {
namespace k {

using namespace dev;

namespace {
template <int PART> struct PartOut { using type = int8_t; };
template <> struct PartOut<temporal::kYear> { using type = int32_t; };
template <> struct PartOut<temporal::kDatePart> { using type = int32_t; };
template <> struct PartOut<temporal::kOrdinalDay> { using type = int16_t; };

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef long long i64x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

template <int UNIT, int PART>
__global__ __launch_bounds__(kBlock) void temporal_part_kernel(const void* __restrict__ in, int64_t n, void* __restrict__ out, int aligned) {
  using In = std::conditional_t<UNIT == temporal::kUnitDate, int32_t, int64_t>;
  using Out = typename PartOut<PART>::type;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
  if (!aligned) {      // values borrowed from the caller at an address that is no multiple of 16 (plx_column_from_device): row by row
    for (int64_t i = t; i < n; i += nt) reinterpret_cast<Out*>(out)[i] = (Out)temporal::part_static<UNIT, PART>((int64_t)reinterpret_cast<const In*>(in)[i]);
    return;
  }
  const int64_t n_quads = n >> 2;
  for (int64_t q = t; q < n_quads; q += nt) {
    int64_t v[4];
    if constexpr (UNIT == temporal::kUnitDate) {
      const i32x4 x = reinterpret_cast<const i32x4*>(in)[q];
      v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
      const i64x2 x0 = reinterpret_cast<const i64x2*>(in)[2 * q], x1 = reinterpret_cast<const i64x2*>(in)[2 * q + 1];
      v[0] = x0.x; v[1] = x0.y; v[2] = x1.x; v[3] = x1.y;
    }
    int32_t r[4];
#pragma unroll
    for (int j = 0; j < 4; j++) r[j] = (int32_t)temporal::part_static<UNIT, PART>(v[j]);
    if constexpr (sizeof(Out) == 1) {
      reinterpret_cast<uint32_t*>(out)[q] = ((uint32_t)r[0] & 0xffu) | (((uint32_t)r[1] & 0xffu) << 8) | (((uint32_t)r[2] & 0xffu) << 16) | ((uint32_t)r[3] << 24);
    } else if constexpr (sizeof(Out) == 2) {
      u32x2 o;
      o.x = ((uint32_t)r[0] & 0xffffu) | ((uint32_t)r[1] << 16);
      o.y = ((uint32_t)r[2] & 0xffffu) | ((uint32_t)r[3] << 16);
      reinterpret_cast<u32x2*>(out)[q] = o;
    } else {
      i32x4 o;
      o.x = r[0]; o.y = r[1]; o.z = r[2]; o.w = r[3];
      reinterpret_cast<i32x4*>(out)[q] = o;
    }
  }
  if (t < (n & 3)) {
    const int64_t i = (n_quads << 2) + t;      // i < n: t < n - 4 n_quads
    reinterpret_cast<Out*>(out)[i] = (Out)temporal::part_static<UNIT, PART>((int64_t)reinterpret_cast<const In*>(in)[i]);
  }
}

template <int UNIT>
void launch_unit(int part, const void* in, int64_t n, void* out) {
  const dim3 grid(grid_for((n + 3) / 4, kBlock, 8)), block(kBlock);
  const int aligned = (((uintptr_t)in | (uintptr_t)out) & 15) == 0 ? 1 : 0;
#define PLX_PART(P) case P: hipLaunchKernelGGL((temporal_part_kernel<UNIT, P>), grid, block, 0, stream(), in, n, out, aligned); break
  switch (part) {
    PLX_PART(temporal::kYear); PLX_PART(temporal::kMonth); PLX_PART(temporal::kDay); PLX_PART(temporal::kQuarter); PLX_PART(temporal::kWeekday);
    PLX_PART(temporal::kOrdinalDay);
    default:
      if constexpr (UNIT != temporal::kUnitDate) {
        switch (part) {
          PLX_PART(temporal::kHour); PLX_PART(temporal::kMinute); PLX_PART(temporal::kSecond); PLX_PART(temporal::kDatePart);
          default: break;
        }
      }
  }
#undef PLX_PART
}
}  // namespace

void temporal_part(int unit, int part, const void* in, int64_t n, void* out) {
  if (!temporal::part_ok(part, unit)) fail(PLX_ERR_INVALID, "temporal part: part " + std::to_string(part) + " of unit " + std::to_string(unit) + " (the time of day and date() exist for a Datetime only)");
  if (n == 0) return;
  ProfileScope ps("temporal_part", (uint64_t)n * (uint64_t)((unit == temporal::kUnitDate ? 4 : 8) + temporal::part_width(part)), (uint64_t)n);
  switch (unit) {
    case temporal::kUnitDate: launch_unit<temporal::kUnitDate>(part, in, n, out); break;
    case temporal::kUnitMs: launch_unit<temporal::kUnitMs>(part, in, n, out); break;
    case temporal::kUnitUs: launch_unit<temporal::kUnitUs>(part, in, n, out); break;
    default: launch_unit<temporal::kUnitNs>(part, in, n, out); break;
  }
  PLX_HIP(hipGetLastError());
}

}  // namespace k
}  // namespace plx
