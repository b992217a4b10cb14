// encoded_inputs.hpp -- narrow "shadows" of low-cardinality columns for the fused aggregate scans.
//
// A fact table stores dates, small integers and enum-like floats in 8-byte columns; the fused scans are bound by the bytes they read.  A shadow is an exact copy of
// such a column as one- or two-byte codes, built once (Column::shadow, see EncodedShadow in core.hpp) and read by every later register / LDS aggregate scan of that
// column in its place:
//   affine  integer column, value = base + stride * code          -> OP_LOAD(u8 | u16), [OP_MUL_I CONST stride], [OP_ADD_I CONST base]
//   dict    f64 column by BIT PATTERN, value = dict[code]         -> OP_LOAD(u8), OP_DICT
//   decimal f64 column of decimals, value = (base + code) / 10^e  -> OP_LOAD(u32), [OP_ADD_I CONST base], OP_DEC10(e)   (decimal.hpp)
// This header holds the host-side pieces with no device dependency: the affine chooser and the rewrite of a compiled program (both pure functions, exposed through the
// C ABI for the tests), and the launchers of the encoder kernels (kernels_encode.hip).
#pragma once
#include "core.hpp"
#include "decimal.hpp"
#include "fused.hpp"

namespace plx {
namespace enc {

// ---- affine chooser ----------------------------------------------------------------------------------------------------------------------------------------------
// From the EXACT minimum / maximum of the valid rows and g = gcd(v - min) over them (0: not computed, or every valid row equals min).
struct AffineChoice { bool ok; int width; int64_t base; uint64_t stride; };
inline uint64_t affine_span(int64_t mn, int64_t mx) { return (uint64_t)mx - (uint64_t)mn; }
inline bool affine_rejects_span(int64_t mn, int64_t mx) { return mx < mn || affine_span(mn, mx) >= (1ull << 62); }
inline bool affine_needs_gcd(int64_t mn, int64_t mx) { return !affine_rejects_span(mn, mx) && affine_span(mn, mx) > 65535; }
inline AffineChoice choose_affine(int64_t mn, int64_t mx, uint64_t g) {
  AffineChoice c{false, 0, mn, 1};
  if (affine_rejects_span(mn, mx)) return c;
  const uint64_t span = affine_span(mn, mx);
  uint64_t stride = 1;
  if (span > 65535) {
    if (g == 0 || span % g != 0) return c;      // (g divides max - min by construction; anything else is a caller's mistake, answered by not encoding)
    stride = g;
  }
  const uint64_t top = span / stride;
  if (top > 65535) return c;
  c.ok = true; c.width = top <= 255 ? 1 : 2; c.stride = stride;
  return c;
}

// ---- program rewrite ---------------------------------------------------------------------------------------------------------------------------------------------
struct InputEncoding {
  int kind = 0;                                 // EncodedShadow::Kind
  int width = 0;
  int64_t base = 0;
  uint64_t stride = 1;                          // decimal: the exponent
  const void* codes = nullptr;
  const unsigned long long* dict = nullptr;
};
// The plain program `sh` / `a` with the inputs that have an encoding read from their codes.  The loads stay where they are (the host compiler emits them first, one
// per input: fused_device.hpp relies on it), only their dtype and pointer change; the decode steps follow the last load and work IN PLACE on the slot the load wrote,
// so no later op changes.  Constants go through one slot the plain program never touches.  Returns false, and leaves the outputs alone, when nothing is encoded or
// the longer program does not fit (kMaxOps, kSlots, kMaxDicts): the caller then runs the plain program.  `taken`, when given, gets bit i set for every input encoded.
inline bool encode_program(const fused::Shape& sh, const fused::Args& a, const InputEncoding* e, fused::Shape* osh, fused::Args* oa, uint32_t* taken = nullptr) {
  using namespace fused;
  int nl = 0;
  while (nl < sh.n_ops && sh.ops[nl].code == OP_LOAD) nl++;
  for (int pc = nl; pc < sh.n_ops; pc++) if (sh.ops[pc].code == OP_LOAD) return false;
  int load_of[kMaxInputs];
  for (int i = 0; i < kMaxInputs; i++) load_of[i] = -1;
  for (int pc = 0; pc < nl; pc++) { const int i = sh.ops[pc].a; if (i >= sh.n_inputs || load_of[i] >= 0) return false; load_of[i] = pc; }
  const uint32_t temp = program_slots(sh);
  Shape s = sh; Args x = a;
  int n = nl, dicts = 0;
  uint32_t did = 0;
  for (int i = 0; i < sh.n_inputs; i++) {
    const InputEncoding& ei = e[i];
    if (!ei.kind || load_of[i] < 0 || (ei.kind == 3 ? ei.width != 4 || ei.stride > (uint64_t)decimal::kMaxExp : ei.width != 1 && ei.width != 2)) continue;
    const uint8_t slot = sh.ops[load_of[i]].dst;
    const bool mul = ei.kind == 1 && ei.stride != 1, add = ei.kind != 2 && ei.base != 0;
    const int extra = ei.kind == 2 ? 1 : 2 * ((mul ? 1 : 0) + (add ? 1 : 0)) + (ei.kind == 3 ? 1 : 0);
    if (n + extra + (sh.n_ops - nl) > kMaxOps) continue;
    if (ei.kind == 3) {      // in place on the load's slot, like the affine decode: decimal::decode op by op
      if (add && temp >= (uint32_t)kSlots) continue;
      if (add) { x.imm[n] = (uint64_t)ei.base; s.ops[n++] = Op{OP_CONST, (uint8_t)temp, 0, 0, 0, {0, 0, 0}}; s.ops[n++] = Op{OP_ADD_I, slot, slot, (uint8_t)temp, 0, {0, 0, 0}}; }
      s.ops[n++] = Op{OP_DEC10, slot, slot, slot, (uint8_t)ei.stride, {0, 0, 0}};
    } else if (ei.kind == 2) {
      if (dicts >= kMaxDicts || ei.width != 1) continue;
      x.dict[dicts] = ei.dict;
      s.ops[n++] = Op{OP_DICT, slot, slot, slot, (uint8_t)dicts, {0, 0, 0}};
      dicts++;
    } else {
      if ((mul || add) && temp >= (uint32_t)kSlots) continue;
      if (mul) { x.imm[n] = ei.stride; s.ops[n++] = Op{OP_CONST, (uint8_t)temp, 0, 0, 0, {0, 0, 0}}; s.ops[n++] = Op{OP_MUL_I, slot, slot, (uint8_t)temp, 0, {0, 0, 0}}; }
      if (add) { x.imm[n] = (uint64_t)ei.base; s.ops[n++] = Op{OP_CONST, (uint8_t)temp, 0, 0, 0, {0, 0, 0}}; s.ops[n++] = Op{OP_ADD_I, slot, slot, (uint8_t)temp, 0, {0, 0, 0}}; }
    }
    s.in_dtype[i] = ei.width == 1 ? PLX_U8 : ei.width == 2 ? PLX_U16 : PLX_U32;
    x.in[i].values = ei.codes;
    did |= 1u << i;
  }
  if (!did) return false;
  for (int pc = nl; pc < sh.n_ops; pc++, n++) { s.ops[n] = sh.ops[pc]; x.imm[n] = a.imm[pc]; }
  for (int pc = n; pc < kMaxOps; pc++) { s.ops[pc] = Op{}; x.imm[pc] = 0; }
  s.n_ops = (uint8_t)n;
  *osh = s; *oa = x;
  if (taken) *taken = did;
  return true;
}

// ---- encoder kernels (kernels_encode.hip) ------------------------------------------------------------------------------------------------------------------------
// gcd of (v - mn) over the valid rows of an i64 column (0 when they all equal mn); synchronises
uint64_t affine_gcd(const int64_t* values, const uint64_t* validity, int64_t n, int64_t mn);
// codes[i] = (v[i] - base) / stride as u8 / u16 (null rows: 0); every valid row decodes its code again and compares: returns false when any row did not come back
// bit for bit (the codes are then garbage).  `codes` holds n rounded up to a multiple of 8 codes.  dtype: PLX_I64 | PLX_I32 | PLX_U32.  Synchronises.
bool affine_encode(int dtype, const void* values, const uint64_t* validity, int64_t n, int64_t base, uint64_t stride, int width, void* codes);
// distinct bit patterns of the valid rows `0, step, 2 * step, ..` of an 8-byte column, sorted as u64: false when there are more than kDictSlots.  Synchronises.
bool dict_collect(const uint64_t* values, const uint64_t* validity, int64_t n, int64_t step, std::vector<uint64_t>* patterns);
// codes[i] = index of v[i] in the sorted dictionary `dict` (device, kDictSlots words, n_dict in use); self-checking like affine_encode.  Synchronises.
bool dict_encode(const uint64_t* values, const uint64_t* validity, int64_t n, const unsigned long long* dict, int n_dict, uint8_t* codes);
// decimal::Stats of the valid rows `0, step, 2 * step, ..` of an f64 column at the exponents e_lo .. e_hi.  Synchronises.
decimal::Stats decimal_stats(const double* values, const uint64_t* validity, int64_t n, int64_t step, int e_lo, int e_hi);
// codes[i] = decimal::encode_row(v[i]) as u32 (null rows: 0), eight rows per lane and one 32-byte store; false when any valid row has no code that decodes to its bits
// (the codes are then garbage).  `codes` holds n rounded up to a multiple of 8 codes.  Synchronises.
bool decimal_encode(const double* values, const uint64_t* validity, int64_t n, int64_t base, int e, uint32_t* codes);

}  // namespace enc
}  // namespace plx
