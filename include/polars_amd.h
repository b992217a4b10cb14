/*
 * polars_amd.h -- C ABI of the MI355X-native columnar execution backend for the
 * Polars hot path (filter / gather, primitive compare + arithmetic, whole-column
 * and grouped aggregation, hash join), built for gfx950.
 *
 * This header is the drop-in boundary (seam B1).  Every entry
 * point is `extern "C"`, takes plain pointers / sizes / opaque integer handles and
 * returns an `int` status (0 = ok).  No torch / C++ types cross it.  A Rust
 * `extern "C"` block in polars-mem-engine binds these 1:1.
 *
 * Reference interfaces each group of entry points replaces (paths relative to
 * the pola-rs/polars tree):
 *
 *   plx_version / plx_last_error
 *       pyo3-polars/pyo3-polars/src/derive.rs:26-66
 *       (_polars_plugin_get_version, _polars_plugin_get_last_error_message)
 *       crates/polars-ffi/src/lib.rs:12-13 (MAJOR=0, MINOR=1)
 *   plx_series_export, plx_column_import_series / plx_column_export_series
 *       crates/polars-ffi/src/version_0.rs:7-16 (SeriesExport), :61-107
 *       (export_series / import_series)
 *   ArrowSchema / ArrowArray, plx_column_import_arrow / plx_column_export_arrow
 *       crates/polars-arrow/src/ffi/generated.rs:6-34 (Arrow C Data Interface)
 *   plx_cmp / plx_cmp_scalar
 *       crates/polars-compute/src/comparisons/mod.rs:4-75 (TotalEqKernel/TotalOrdKernel)
 *       null rule crates/polars-core/src/chunked_array/ops/arity.rs:203-214,430-454
 *   plx_bitmap_binop / plx_bitmap_not
 *       crates/polars-expr/src/expressions/binary.rs:110-118
 *   plx_arith / plx_arith_scalar
 *       crates/polars-compute/src/arithmetic/mod.rs:8-150 (ArithmeticKernel)
 *   plx_cast
 *       crates/polars-expr/src/expressions/cast.rs (numeric casts only)
 *   plx_if_then_else
 *       crates/polars-expr/src/expressions/ternary.rs (TernaryExpr), crates/polars-core/src/chunked_array/ops/zip.rs (zip_with)
 *   plx_temporal_part
 *       crates/polars-time/src/chunkedarray/date.rs, datetime.rs (DateMethods / DatetimeMethods: year, month, day, quarter, weekday, ordinal, hour, minute, second)
 *   plx_filter
 *       crates/polars-compute/src/filter/mod.rs:18-28 (filter)
 *   plx_gather
 *       crates/polars-compute/src/gather/primitive.rs:9-78 (take_primitive_unchecked)
 *   plx_reduce
 *       crates/polars-core/src/chunked_array/ops/aggregate/mod.rs:86-137,240-246,307-316
 *   plx_groupby_agg
 *       crates/polars-core/src/frame/group_by/mod.rs:29-98 (group_by_with_series)
 *       + crates/polars-core/src/frame/group_by/aggregations/mod.rs:854-1018
 *   plx_join_indices
 *       crates/polars-ops/src/frame/join/hash_join/single_keys_dispatch.rs:234-357
 *       (hash_join_inner / hash_join_left -> (left_idx, right_idx))
 *   plx_join_asof_indices / PLX_IR_JOIN_ASOF
 *       crates/polars-ops/src/frame/join/asof/{mod.rs, default.rs, groups.rs} (join_asof, join_asof_by; AsofStrategy, the backward / forward / nearest scans)
 *   plx_hash_partition
 *       crates/polars-utils/src/hashing.rs:72-121 (HashPartitioner) and
 *       crates/polars-expr/src/hash_keys.rs:263-314 (gen_idxs_per_partition)
 *   plx_ir / plx_aexpr / plx_execute_plan
 *       crates/polars-plan/src/plans/ir/mod.rs:53-187 (IR arena),
 *       crates/polars-plan/src/plans/aexpr/mod.rs:150-259 (AExpr arena),
 *       crates/polars-mem-engine/src/planner/lp.rs:75-100,326-878 (create_physical_plan)
 *       crates/polars-mem-engine/src/executors/executor.rs:10-16 (Executor::execute)
 *   plx_profile_*
 *       crates/polars-expr/src/state/node_timer.rs:14-70 (NodeTimer)
 *
 * Threading: every call is thread-safe (the reference calls plugins from rayon workers,
 * crates/polars-ffi/src/version_0.rs:136-162).  A thread that wants its own HIP stream installs it
 * with plx_set_stream; device buffers recycled by the library's pool between threads are ordered
 * behind the releasing stream (event recorded at release, waited for on re-use).  A column handed
 * to another thread must only be used there after the producing thread synchronised
 * (plx_synchronize) -- the same rule a SeriesExport hand-over obeys.  Errors never unwind across
 * the ABI; a non-zero status means `plx_last_error()` (thread-local) holds the message.
 */
#ifndef POLARS_AMD_H
#define POLARS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLX_ABI_MAJOR 0
#define PLX_ABI_MINOR 1

/* ---- status codes ------------------------------------------------------ */
#define PLX_OK 0
#define PLX_ERR_INVALID 1      /* bad argument / dtype mismatch (PolarsError::InvalidOperation) */
#define PLX_ERR_HIP 2          /* HIP runtime error; message has hipGetErrorString */
#define PLX_ERR_UNSUPPORTED 3  /* node/dtype outside the hot path -> caller falls back to CPU */
#define PLX_ERR_OOM 4
#define PLX_ERR_SHAPE 5        /* length mismatch (PolarsError::ShapeMismatch) */
#define PLX_ERR_NOT_FOUND 6    /* unknown column (PolarsError::ColumnNotFound) */
#define PLX_ERR_CANCELLED 7    /* host cancel flag raised (ExecutionState::should_stop) */

/* ---- physical dtypes (Arrow primitive layouts) --------------------------- */
typedef enum plx_dtype {
  PLX_BOOL = 0, /* bit-packed LSB-first values bitmap */
  PLX_I8 = 1,
  PLX_I16 = 2,
  PLX_I32 = 3, /* also Date */
  PLX_I64 = 4, /* also Datetime / Duration */
  PLX_U8 = 5,
  PLX_U16 = 6,
  PLX_U32 = 7, /* also IdxSize, Categorical physical */
  PLX_U64 = 8,
  PLX_F32 = 9,
  PLX_F64 = 10
} plx_dtype;

/* comparison operators: polars_plan::dsl::Operator (dsl/expr/mod.rs:683-707) */
typedef enum plx_cmp_op { PLX_EQ = 0, PLX_NE = 1, PLX_LT = 2, PLX_LE = 3, PLX_GT = 4, PLX_GE = 5 } plx_cmp_op;

/* arithmetic operators */
typedef enum plx_arith_op {
  PLX_ADD = 0,
  PLX_SUB = 1,
  PLX_MUL = 2,
  PLX_TRUE_DIV = 3,  /* ints -> f64, floats stay */
  PLX_FLOOR_DIV = 4, /* ints: by zero -> null */
  PLX_MOD = 5        /* ints: by zero -> null */
} plx_arith_op;

typedef enum plx_bitmap_op { PLX_AND = 0, PLX_OR = 1, PLX_XOR = 2 } plx_bitmap_op;

/* aggregations: IRAggExpr (plans/aexpr/mod.rs) subset on the hot path */
typedef enum plx_agg_op {
  PLX_AGG_SUM = 0,
  PLX_AGG_MEAN = 1,
  PLX_AGG_MIN = 2,
  PLX_AGG_MAX = 3,
  PLX_AGG_COUNT = 4, /* non-null count, u32 (IdxSize) */
  PLX_AGG_LEN = 5,   /* row count incl. nulls, u32 */
  PLX_AGG_FIRST = 6, /* first row of each group (group_by only; used for key columns) */
  /* Variance / standard deviation of the valid rows with `ddof` delta degrees of freedom: f64 (f32 stays f32), null when valid rows <= ddof; a NaN or an
   * infinity among the values gives NaN.  A PLX_AE_AGG node of these kinds carries ddof (0..255) in lit.u; plx_groupby_agg uses ddof = 1, plx_groupby_agg_ddof
   * takes one per aggregate; a whole column goes through plx_reduce_var (plx_reduce refuses the two kinds).  Numeric operands only: a Boolean operand is
   * PLX_ERR_UNSUPPORTED.  Fused scans accumulate sums about a pivot: the accuracy contract is DESIGN.md 4.14. */
  PLX_AGG_VAR = 7,
  PLX_AGG_STD = 8,
  /* An order statistic of the valid rows (median = quantile 0.5, linear): f64 (f32 stays f32), null when no row is valid.  Values rank in the sort's total order
   * (NaN greatest, -0 == +0).  A PLX_AE_AGG node of this kind carries q (a real number in [0, 1]) in lit.f64 and the plx_quantile_interpolation in its dtype slot;
   * plx_groupby_agg_params takes one pair per aggregate (plx_groupby_agg / plx_groupby_agg_ddof refuse the kind); a whole column goes through plx_reduce_quantile
   * (plx_reduce refuses the kind).  Integer and float operands only: a Boolean operand is PLX_ERR_UNSUPPORTED.  It is no sum of cells: fused scans decline it, a
   * whole column runs a radix select and a group-by sorted segments. */
  PLX_AGG_QUANTILE = 9,
  /* The number of distinct values of the rows, a null counting as one value of its own: PLX_U32, never null; 0 for an empty column, at least 1 for a group.  Values
   * are equal by the sort's equality (every NaN equals every NaN, -0 == +0, integers exactly).  No parameters: plx_groupby_agg, plx_groupby_agg_ddof and
   * plx_groupby_agg_params all take it; a whole column goes through plx_reduce_n_unique (plx_reduce refuses the kind).  Any integer, float or Boolean operand (Date,
   * Datetime and Categorical columns are integers here).  It is no sum of cells: fused scans decline it, a whole column runs one of three routes and a group-by the
   * sorted segments of the quantiles. */
  PLX_AGG_N_UNIQUE = 10
} plx_agg_op;

/* Which row of every class of equal rows PLX_IR_DISTINCT / plx_distinct_mask keep: FIRST the first in row order, LAST the last, NONE only the rows of classes of one
 * row; ANY leaves the choice to the engine, which serves it as FIRST (the plan description says so). */
typedef enum plx_unique_keep {
  PLX_UNIQUE_ANY = 0,
  PLX_UNIQUE_FIRST = 1,
  PLX_UNIQUE_LAST = 2,
  PLX_UNIQUE_NONE = 3
} plx_unique_keep;

/* The cumulative functions (PLX_AE_CUMULATIVE, plx_cumulative): each keeps one value per row.  A null row stays null (COUNT has no nulls) and adds nothing; the
 * running value carries over it.  SUM: the sum aggregate's dtype (narrow integers -> PLX_I64, PLX_BOOL -> PLX_U32), integers wrap, PLX_F32 accumulates in f64 like
 * the sum aggregate; MIN / MAX keep the dtype and ignore a NaN unless every valid value so far is NaN (the min / max aggregates' rule); COUNT: PLX_U32, the number of
 * non-null values up to and including the row. */
typedef enum plx_cum_op {
  PLX_CUM_SUM = 0,
  PLX_CUM_MIN = 1,
  PLX_CUM_MAX = 2,
  PLX_CUM_COUNT = 3
} plx_cum_op;

/* The ranking methods (PLX_AE_RANK, plx_rank).  Values rank in the sort's order (NaN greatest, all NaNs tie, -0 == +0); a null row's rank is null and nulls take no
 * part.  Among equal values AVERAGE gives the mean of their ordinal ranks (PLX_F64), MIN the smallest, MAX the largest, DENSE the number of distinct values up to
 * theirs, ORDINAL their ordinal ranks in row order (also when descending); the last four are PLX_U32. */
typedef enum plx_rank_method {
  PLX_RANK_AVERAGE = 0,
  PLX_RANK_MIN = 1,
  PLX_RANK_MAX = 2,
  PLX_RANK_DENSE = 3,
  PLX_RANK_ORDINAL = 4
} plx_rank_method;

/* The fixed-window rolling functions (PLX_AE_ROLLING, plx_rolling).  The window of row i is the rows [i + h - w + 1, i + h] of its partition, h = 0 or, centered,
 * (w - 1) / 2, clipped to the partition; the result is null where the window holds fewer than min_samples non-null values, else the function of its non-null values.
 * SUM: the dtype of PLX_CUM_SUM (narrow integers -> PLX_I64, PLX_BOOL -> PLX_U32, integers wrap, PLX_F32 accumulates in f64); MEAN: PLX_F64 (PLX_F32 for a PLX_F32
 * operand), accumulated in f64; MIN / MAX keep the dtype and ignore a NaN unless every valid value of the window is NaN. */
typedef enum plx_rolling_op {
  PLX_ROLLING_SUM = 0,
  PLX_ROLLING_MEAN = 1,
  PLX_ROLLING_MIN = 2,
  PLX_ROLLING_MAX = 3
} plx_rolling_op;

/* With pos = (n - 1) * q over the n valid values in order and a, b the values at ranks floor(pos), ceil(pos): NEAREST = the value at rank floor(pos + 0.5),
 * LOWER = a, HIGHER = b, MIDPOINT = a == b ? a : (a + b) / 2, LINEAR = a == b ? a : (pos - floor(pos)) * (b - a) + a. */
typedef enum plx_quantile_interpolation {
  PLX_QUANTILE_NEAREST = 0,
  PLX_QUANTILE_LOWER = 1,
  PLX_QUANTILE_HIGHER = 2,
  PLX_QUANTILE_MIDPOINT = 3,
  PLX_QUANTILE_LINEAR = 4
} plx_quantile_interpolation;

/* Null keys match nothing (nulls_equal is not on this path).  PLX_JOIN_FULL: every pair of the inner join, one row per unmatched left row (null right index) and one
 * row per unmatched right row (null left index); null-key rows of either side count as unmatched.  PLX_JOIN_RIGHT: the left join with the sides exchanged -- every
 * right row appears, the left index is nullable.  (The reference tree was not at hand when FULL and RIGHT were added: their contract here and at plx_ir.coalesce /
 * plx_join_order is the maintainers' reading of polars >= 1.0 and is what the tests pin.) */
typedef enum plx_join_how { PLX_JOIN_INNER = 0, PLX_JOIN_LEFT = 1, PLX_JOIN_SEMI = 2, PLX_JOIN_ANTI = 3, PLX_JOIN_FULL = 4, PLX_JOIN_RIGHT = 5 } plx_join_how;

/* As-of joins (plx_join_asof_indices, PLX_IR_JOIN_ASOF): which candidate a left row takes.  OR PLX_ASOF_STRICT into the strategy for allow_exact_matches = false:
 * every comparison becomes strict, for NEAREST as well.  The contract is stated at plx_join_asof_indices. */
typedef enum plx_asof_strategy { PLX_ASOF_BACKWARD = 0, PLX_ASOF_FORWARD = 1, PLX_ASOF_NEAREST = 2 } plx_asof_strategy;
#define PLX_ASOF_STRICT 4

/* A 64-bit scalar passed by bit pattern; interpreted according to a plx_dtype. */
typedef union plx_scalar {
  int64_t i;
  uint64_t u;
  double f64;
  float f32;
} plx_scalar;

/* Opaque handles (0 is never valid). */
typedef uint64_t plx_column; /* device-resident Arrow-layout column */
typedef uint64_t plx_frame;  /* ordered set of named columns of equal length */

/* ---- Arrow C Data Interface (standard layout) ------------------------- */
#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE
struct ArrowSchema {
  const char* format;
  const char* name;
  const char* metadata;
  int64_t flags;
  int64_t n_children;
  struct ArrowSchema** children;
  struct ArrowSchema* dictionary;
  void (*release)(struct ArrowSchema*);
  void* private_data;
};
struct ArrowArray {
  int64_t length;
  int64_t null_count;
  int64_t offset;
  int64_t n_buffers;
  int64_t n_children;
  const void** buffers;
  struct ArrowArray** children;
  struct ArrowArray* dictionary;
  void (*release)(struct ArrowArray*);
  void* private_data;
};
#endif

/* Mirror of polars_ffi::version_0::SeriesExport (a chunked Arrow array). */
typedef struct plx_series_export {
  struct ArrowSchema* field;
  struct ArrowArray** arrays;
  size_t len;
  void (*release)(struct plx_series_export*);
  void* private_data;
} plx_series_export;

/* ---- library / device -------------------------------------------------- */
/* (major << 16) | minor, same packing as _polars_plugin_get_version. */
uint32_t plx_version(void);
/* Thread-local message of the last failing call on this thread ("" if none). */
const char* plx_last_error(void);
/* Bind the calling process to one GPU (one process per GPU). Idempotent. */
int plx_init(int device_ordinal);
int plx_shutdown(void);
/* Launch all subsequent work of this thread on `hip_stream` (hipStream_t as void*;
 * NULL = the library's own stream). */
int plx_set_stream(void* hip_stream);
int plx_synchronize(void);
/* Cooperative cancel flag checked between kernel launches. */
int plx_set_cancel(int flag);
/* name (<=255 chars), CU count, HBM bytes of the bound device. */
int plx_device_info(char* name_out, size_t name_cap, int32_t* cu_count, uint64_t* hbm_bytes);
/* bytes currently held by the library's device pool / high-water mark */
int plx_memory_stats(uint64_t* in_use, uint64_t* high_water);
/* return cached free blocks to the driver */
int plx_memory_trim(void);
/* Pre-grows the device memory pool: after the call its cache holds a free block of at least `bytes`.  Mapping device memory costs ~30 ms per GB
 * (hipMalloc); an executor that expects queries with large intermediates (the record pool of a partitioned group-by over 1e9 rows: 12-25 GB) sizes the
 * pool once at start-up, the way the reference's GPU engine sizes its RMM pool, instead of paying inside its first query. */
int plx_memory_reserve(uint64_t bytes);

/* ---- columns ----------------------------------------------------------- */
/* Copy a host Arrow-layout buffer pair to HBM. `validity` may be NULL (no nulls);
 * `bit_offset` applies to both a PLX_BOOL values bitmap and the validity bitmap
 * (Arrow `offset`); for non-bool values the caller passes the already-offset
 * values pointer. */
int plx_column_from_host(plx_dtype dtype, const void* values, const uint8_t* validity,
                         int64_t bit_offset, int64_t len, plx_column* out);
/* Wrap device buffers owned by the caller (e.g. a torch tensor): no copy; the
 * caller keeps them alive until plx_column_free. validity may be NULL.
 * Alignment: dev_values is a multiple of the element width (8 for PLX_BOOL, whose
 * values are a bitmap); it need NOT be a multiple of 16 -- a window that starts
 * anywhere inside a larger buffer is fine.  dev_validity is a multiple of 8 and
 * covers whole 64-bit words, (len + 63) / 64 of them, with bit 0 of word 0 the
 * first row: every kernel loads validity (and Boolean values) as uint64_t.
 * A pointer below that returns PLX_ERR_INVALID before anything is launched. */
int plx_column_from_device(plx_dtype dtype, void* dev_values, void* dev_validity, int64_t len,
                           plx_column* out);
/* Planning-only column: dtype / length / nullability (/ integer range statistics) but NO
 * device memory.  Lets plx_describe_fusion run without a GPU; every compute entry point
 * rejects it. */
int plx_column_placeholder(plx_dtype dtype, int64_t len, int nullable, int has_range, int64_t range_min, int64_t range_max,
                           plx_column* out);
/* Planning-only: declares the encoded shadow a placeholder column would have (kind 1 = affine, value = base + stride * code; 2 = dictionary; width = bytes per
 * code, 1 | 2), so that plx_describe_fusion / plx_debug_program_json show the program a scan of the encoded column runs.  Placeholder columns only. */
int plx_column_placeholder_encoding(plx_column col, int32_t kind, int32_t width, int64_t base, uint64_t stride);
/* The affine chooser of the encoded shadows, a pure function: from the exact minimum / maximum of a column's valid rows and gcd = gcd(v - min) over them (0: not
 * computed) -> whether the column encodes, code width in bytes, base and stride.  needs_gcd: the span alone does not decide, the gcd pass has to run. */
int plx_encoding_choose_affine(int64_t min, int64_t max, uint64_t gcd, int32_t* ok, int32_t* width, int64_t* base, uint64_t* stride, int32_t* needs_gcd);
/* The decimal shadow of an f64 column (kind 3, four-byte codes): value = (double)(int64)(base + code) / 10^e, e in 0..9.  plx_column_placeholder_encoding takes kind 3
 * with width 4, the exponent in `stride` and the base as is.  The three functions below are the host twins of what the device runs (one shared header), pure
 * functions over host memory:
 *   choose_decimal  the chooser over the valid rows of `values` (validity: LSB-first bitmap or null): the smallest exponent at which every row is k / 10^e bit for
 *                   bit, base 0 when every k lies in [0, 2^32), else the minimum; ok = 0 for NaN, +-inf, -0.0, |k| >= 2^53, a span of 2^32 or a non-decimal;
 *   decimal_decode  out[i] = the value of codes[i];
 *   decimal_encode  codes[i] / ok[i] = the code of values[i] under (base, e), or ok[i] = 0 when the row has none (the encoder's mismatch). */
int plx_encoding_choose_decimal(const double* values, const uint8_t* validity, int64_t n, int32_t* ok, int32_t* e, int64_t* base);
int plx_encoding_decimal_decode(int64_t base, int32_t e, const uint32_t* codes, int64_t n, double* out);
int plx_encoding_decimal_encode(const double* values, int64_t n, int64_t base, int32_t e, uint32_t* codes, uint8_t* ok);
/* f64 columns of at least min_rows rows may get a decimal shadow (it takes half the column's bytes; default 2^22, environment PLX_ENCODED_DECIMAL_MIN_ROWS). */
int plx_encoded_set_decimal_min_rows(int64_t min_rows);
int64_t plx_encoded_decimal_min_rows(void);
/* Caller-provided value bounds of an integer column (dictionary size of a Categorical, Parquet column-chunk min / max
 * statistics): every valid value lies in [lo, hi].  The planner uses them the way the reference uses sortedness flags and
 * metadata statistics -- to choose dense / direct-address group tables without a pass over the data.  Kernels that rely on
 * the bounds check them per row and fail the query (PLX_ERR_INVALID) if a value lies outside. */
int plx_column_set_bounds(plx_column col, int64_t lo, int64_t hi);
/* Forgets what the library has LEARNED about the column (value range computed by a statistics pass or as a by-product of a scan, the group-by
 * planner's key sample and heavy hitters, the sampled sortedness): the next query pays for them again, as the first query on a fresh column
 * does.  The column's encoded shadow and the count of scans towards one go too.  Bounds declared with plx_column_set_bounds stay.  Measurement support (bench.py `one_shot_ms`); never changes a result. */
int plx_column_drop_statistics(plx_column col);
/* Arrow C Data Interface import: copies to HBM, then calls array->release and
 * schema->release (callee takes ownership: plugin.rs:122-125 convention). */
int plx_column_import_arrow(struct ArrowArray* array, struct ArrowSchema* schema, plx_column* out);
/* Chunked import (SeriesExport): chunks are concatenated on device. Takes ownership. */
int plx_column_import_series(plx_series_export* series, plx_column* out);
/* Export to host memory owned by the returned structs (released via ->release). */
int plx_column_export_arrow(plx_column col, struct ArrowArray* out_array, struct ArrowSchema* out_schema);
int plx_column_export_series(plx_column col, const char* name, plx_series_export* out);
/* Plain download. values_out must hold len*width bytes (BOOL: (len+7)/8);
 * validity_out (may be NULL) must hold (len+7)/8 bytes; *has_validity_out tells
 * whether the column carries a validity bitmap (if not, validity_out is all ones). */
int plx_column_to_host(plx_column col, void* values_out, uint8_t* validity_out, int32_t* has_validity_out);
/* Device-to-device copy into caller-owned HBM (e.g. a torch tensor): values (len*width bytes;
 * BOOL: (len+7)/8) and, if dev_validity_out != NULL, (len+7)/8 validity bytes (all ones when the
 * column has no bitmap).  Synchronises the library stream before returning. */
int plx_column_copy_to_device(plx_column col, void* dev_values_out, void* dev_validity_out);
int plx_column_info(plx_column col, plx_dtype* dtype, int64_t* len, int64_t* null_count);
int plx_column_device_ptrs(plx_column col, void** values, void** validity);
int plx_column_retain(plx_column col);
int plx_column_free(plx_column col);

/* ---- kernel-level entry points (one reference kernel family each) -------- */
/* out: PLX_BOOL, validity = lhs.validity AND rhs.validity. Total-order float
 * semantics (NaN == NaN, NaN greatest). */
int plx_cmp(plx_cmp_op op, plx_column lhs, plx_column rhs, plx_column* out);
int plx_cmp_scalar(plx_cmp_op op, plx_column lhs, plx_scalar rhs, plx_column* out);
/* Boolean columns: values op, validity AND (binary.rs:110-118). */
int plx_bitmap_binop(plx_bitmap_op op, plx_column lhs, plx_column rhs, plx_column* out);
int plx_bitmap_not(plx_column col, plx_column* out);
/* Same-dtype operands (type coercion happens in the optimizer). */
int plx_arith(plx_arith_op op, plx_column lhs, plx_column rhs, plx_column* out);
/* Row-wise select (the reference's zip_with): out[i] = mask[i] is valid and true ? if_true[i] : if_false[i], value and validity of the chosen side; a null mask row
 * selects if_false.  mask is Boolean, if_true / if_false have one dtype (any fixed-width dtype or Boolean); a length-1 operand broadcasts.  The result carries a
 * validity bitmap only when a side can be null. */
int plx_if_then_else(plx_column mask, plx_column if_true, plx_column if_false, plx_column* out);
/* scalar_on_left: computes scalar OP col instead of col OP scalar. */
int plx_arith_scalar(plx_arith_op op, plx_column col, plx_scalar scalar, int scalar_on_left, plx_column* out);
/* numeric -> numeric cast (non-strict: out-of-range -> null like polars cast(strict=False)). */
int plx_cast(plx_column col, plx_dtype to, plx_column* out);
/* Stream compaction by a PLX_BOOL mask; null mask values are false. */
int plx_filter(plx_column col, plx_column mask, plx_column* out);
/* out[i] = col[idx[i]]; idx is PLX_U32 (IdxSize); null idx -> null. */
int plx_gather(plx_column col, plx_column idx, plx_column* out);
/* Whole-column reduction. *out_value receives the scalar in the output dtype
 * *out_dtype (sum: SumCast rule; mean: f64, f32 stays f32; count/len: u32);
 * *out_valid = 0 when the result is null (mean/min/max of empty or all-null). */
int plx_reduce(plx_agg_op op, plx_column col, plx_scalar* out_value, plx_dtype* out_dtype, int32_t* out_valid);
/* Whole-column variance (want_std != 0: standard deviation) with ddof 0..255 delta degrees of freedom.  *out_dtype is f64 (f32 for an f32 column);
 * *out_valid = 0 when the column has at most ddof valid rows.  One streaming pass of Chan merges, no atomics: the same column gives the same bits every time, and
 * a common offset of any size costs no digits.  Numeric columns only (PLX_ERR_UNSUPPORTED names the dtype otherwise). */
int plx_reduce_var(plx_column col, int32_t ddof, int32_t want_std, plx_scalar* out_value, plx_dtype* out_dtype, int32_t* out_valid);
/* Whole-column quantile q in [0, 1] (NaN or outside: PLX_ERR_INVALID) with a plx_quantile_interpolation; the median is (0.5, PLX_QUANTILE_LINEAR).  *out_dtype is
 * f64 (f32 for an f32 column); *out_valid = 0 when the column has no valid row.  A radix select over the sort's value codes: the column is never sorted, and the
 * same column gives the same bits every time.  plx_last_plan_description() names the digit rounds.  Integer and float columns only (PLX_ERR_UNSUPPORTED names the
 * dtype otherwise); at most 2^32 - 2 rows. */
int plx_reduce_quantile(plx_column col, double q, int32_t interpolation, plx_scalar* out_value, plx_dtype* out_dtype, int32_t* out_valid);
/* Whole-column distinct count (PLX_AGG_N_UNIQUE): *out = the number of distinct values, a null counting as one; 0 for an empty column.  Three routes, named by
 * plx_last_plan_description(): "n_unique[boolean]" (popcounts), "n_unique[bitmap range=R]" (integer columns whose exact value range R = max - min + 1 is at most
 * max(64 * rows, 2^20): one bit per value, vector atomic OR) and "n_unique[sorted codes: passes=P, skipped=S]" (everything else: a key-only radix sort of the value
 * codes and a count of the run heads).  PLX_NUNIQUE_ROUTE=sort in the environment forces the sorted-codes route (=bitmap is the default rule: the bitmap wherever it is legal).  Integer atomics only: the same column
 * gives the same count every time.  At most 2^32 - 2 rows. */
int plx_reduce_n_unique(plx_column col, uint32_t* out);

/* Hash group-by with in-place aggregation.  n_keys >= 1 key columns (integer,
 * bool or float; a null key forms its own group; floats canonicalised).
 * aggs[i] applies to values[i] (ignored for PLX_AGG_LEN, may be 0).
 * Outputs: out_keys[n_keys] (one row per group) and out_aggs[n_aggs].
 * Row order of groups is unspecified unless maintain_order != 0 (then groups are
 * ordered by first occurrence). */
int plx_groupby_agg(const plx_column* keys, int32_t n_keys, const plx_column* values,
                    const plx_agg_op* aggs, int32_t n_aggs, int32_t maintain_order,
                    plx_column* out_keys, plx_column* out_aggs);
/* The same with ddof[i] (0..255) for aggregate i: read for PLX_AGG_VAR / PLX_AGG_STD, ignored for every other kind.  ddof == NULL: 1 everywhere. */
int plx_groupby_agg_ddof(const plx_column* keys, int32_t n_keys, const plx_column* values,
                         const plx_agg_op* aggs, int32_t n_aggs, int32_t maintain_order, const int32_t* ddof,
                         plx_column* out_keys, plx_column* out_aggs);
/* The same with q[i] / interpolation[i] (plx_quantile_interpolation) for aggregate i as well: read for PLX_AGG_QUANTILE, ignored for every other kind.  A NULL array
 * means the defaults: ddof 1, q 0.5, PLX_QUANTILE_LINEAR (the median).  Quantiles run over sorted segments, every other kind as in plx_groupby_agg; the group order
 * is that of the same call without the quantiles. */
int plx_groupby_agg_params(const plx_column* keys, int32_t n_keys, const plx_column* values,
                           const plx_agg_op* aggs, int32_t n_aggs, int32_t maintain_order, const int32_t* ddof,
                           const double* q, const int32_t* interpolation, plx_column* out_keys, plx_column* out_aggs);
/* Window aggregates (PLX_AE_WINDOW as a column call): aggregate i of `aggs` over values[i] per partition of the n_keys (1..8: more is PLX_ERR_UNSUPPORTED) key columns,
 * given back on every row -- out_cols[i] has the height and row order of the keys, the dtype and validity the aggregate has in plx_groupby_agg_params.  keys, values,
 * aggs, ddof, q and interpolation follow plx_groupby_agg_params (values[i] may be 0 for PLX_AGG_LEN; NULL ddof / q / interpolation: the defaults).  One group-by, one
 * row -> group map and one broadcast launch per 8 outputs.  The map takes one of two routes, named by plx_last_plan_description(): "window[direct range=R]" (integer,
 * Boolean, temporal and Categorical keys but PLX_U64 whose joint code range R keeps 4 R <= max(8 rows, 4 MiB): a table of R group ids) and "window[sorted rows: ...]"
 * (everything else: one sort of the rows).  PLX_WINDOW_ROUTE=sort in the environment forces the sorted route (=direct is the default rule: the direct route wherever it
 * is legal).  At most 2^32 - 2 rows. */
int plx_window_agg(const plx_column* keys, int32_t n_keys, const plx_column* values, const plx_agg_op* aggs, int32_t n_aggs, const int32_t* ddof,
                   const double* q, const int32_t* interpolation, plx_column* out_cols);
/* Cumulative functions and ranks over plain columns (PLX_AE_CUMULATIVE / PLX_AE_RANK as column calls).  n_keys == 0 (keys may be NULL): the whole
 * column is one partition; 1..8 key columns (more is PLX_ERR_UNSUPPORTED): the partitions of a window over them, each scanned / ranked in row order.  op is a
 * plx_cum_op, method a plx_rank_method, reverse / descending 0 or 1: anything else is PLX_ERR_INVALID naming the parameter, checked before anything runs, an empty
 * input included.  The result has the height and row order of `value`, the dtype of plx_cum_op / plx_rank_method and the validity of `value` (PLX_CUM_COUNT: none).
 * plx_last_plan_description() names the route: "Cumulative{... route=cumulative[whole column] | cumulative[sorted rows: ...]}" (a segmented inclusive scan in three
 * launches: tile aggregates, their scan, the tiles with their carry) and "Rank{... route=rank[sorted segments: ...]}" (one sort by (keys, value), two head masks, O(1) per row).
 * At most 2^32 - 2 rows. */
int plx_cumulative(const plx_column* keys, int32_t n_keys, plx_column value, int32_t op, int32_t reverse, plx_column* out);
int plx_rank(const plx_column* keys, int32_t n_keys, plx_column value, int32_t method, int32_t descending, plx_column* out);
/* shift / diff and the rolling functions over plain columns (PLX_AE_SHIFT / PLX_AE_ROLLING as column calls).  keys / n_keys as for plx_cumulative.
 * plx_shift: row i takes row i - n of its partition (any n; |n| >= the partition length vacates every row); vacated rows are null, or hold *fill (a value of the
 * column's dtype) and are valid when fill is not NULL.  diff != 0: the result is value[i] - value[i - n] in the widened dtype (PLX_U8 -> PLX_I16, PLX_U16 -> PLX_I32,
 * PLX_U32 / PLX_U64 -> PLX_I64, else unchanged; integers wrap), null where either row is null or row i - n lies outside the partition; fill must be NULL and a
 * PLX_BOOL column is PLX_ERR_UNSUPPORTED.  plx_rolling: op is a plx_rolling_op, window_size >= 1, min_samples in 1..window_size, center 0 or 1.  Anything else is
 * PLX_ERR_INVALID naming the parameter, checked before anything runs, an empty input included.  plx_last_plan_description() names the route:
 * "Shift{... route=shift[whole column] | shift[sorted rows: ...]}", "Rolling{... route=rolling[tile halo: w=.., lds=..] | rolling[two scans: ...]}".  The environment
 * variable PLX_ROLLING_ROUTE=scans (read per call) forces the two-scan route at every window size; "tile" or unset: the tile route up to a window of 1024 rows.
 * At most 2^32 - 2 rows. */
int plx_shift(const plx_column* keys, int32_t n_keys, plx_column value, int64_t n, const plx_scalar* fill, int32_t diff, plx_column* out);
int plx_rolling(const plx_column* keys, int32_t n_keys, plx_column value, int32_t op, int64_t window_size, int64_t min_samples, int32_t center, plx_column* out);
/* Row-order Boolean mask (no nulls) of the rows that unique() keeps: the n_keys (1..8: more is PLX_ERR_UNSUPPORTED) key columns of integer, float or Boolean dtype
 * are sorted stably once, so the head of every run of equal rows is its first occurrence and the tail its last; keep is a plx_unique_keep (outside 0..3:
 * PLX_ERR_INVALID).  Two rows are equal when every key is equal by the sort's equality, null == null.  Filtering any column of the same height by the mask
 * (plx_filter) gives the distinct rows in row order. */
int plx_distinct_mask(const plx_column* keys, int32_t n_keys, int32_t keep, plx_column* out_mask);

/* Equi-join on one key column pair -> row-index pairs (PLX_U32). For LEFT joins the
 * right index column carries nulls for unmatched left rows. Null keys never match.
 * Pair order is unspecified (sort before comparing), as in the reference.
 * SEMI / ANTI (single_keys_semi_anti.rs): *out_left_idx = the left rows with (without) a match on the right, in
 * left order; *out_right_idx = 0 (no column).  A null left key never matches (kept by ANTI, dropped by SEMI). */
int plx_join_indices(plx_join_how how, plx_column left_key, plx_column right_key,
                     plx_column* out_left_idx, plx_column* out_right_idx);

/* As-of join -> one right row index (or null) per left row, in left row order (*out_right_idx: PLX_U32, len(left_on) rows, a validity bitmap only when some row
 * is unmatched).  The reference tree was not at hand: this contract is the maintainers' reading of py-polars join_asof and polars-ops/src/frame/join/asof/, and
 * is what the tests pin.
 *   strategy_and_flags   a plx_asof_strategy, OR'd with PLX_ASOF_STRICT for allow_exact_matches = false; anything else is PLX_ERR_INVALID.
 *   groups     the candidates of a left row are the right rows whose n_by (0..7: more is PLX_ERR_UNSUPPORTED) `by` parts all equal the left row's, by the sort's
 *              equality (NaN == NaN, -0 == +0).  A null in any by part, or a null `on`, on either side makes that row match nothing; a left row whose group has
 *              no right row gets null.  by parts: integer, float or Boolean columns, part j of one dtype on both sides.
 *   order      the candidates of a group are taken in (on, right row) order.  Neither side needs to be sorted: the usable right rows are checked for order in
 *              one pass and sorted (stable, by parts then on) only when that fails; left rows are searched independently.
 *   backward   the last candidate with on_r <= on_l;  forward: the first candidate with on_r >= on_l;  nearest: the candidate at the smallest distance, among
 *              several at that distance the LAST in candidate order -- an equidistant pair goes to the forward value, a duplicated forward value to its last
 *              row, an exact match to the last of its duplicates.  PLX_ASOF_STRICT makes every comparison strict (nearest then skips exact matches).
 *   tolerance  NULL, or the largest distance a match may have: read as .u for an integer `on` (Date / Datetime: in the column's own unit), as .f64 (>= 0, not
 *              NaN: PLX_ERR_INVALID) for a float `on`.  The match found without the tolerance is kept only if its distance is at most the tolerance; there is
 *              no fallback to another candidate.  Integer distances are exact in 64 unsigned bits (Int64 min against max is 2^64 - 1, not an overflow);
 *              float distances are |a - b| in f64, equal values (NaN against NaN, inf against inf) are distance 0, a NaN distance is within no tolerance
 *              and loses against any number under nearest.
 *   on         any integer dtype, PLX_F32 or PLX_F64, the same dtype on both sides (PLX_BOOL: PLX_ERR_UNSUPPORTED).
 * plx_last_plan_description(): "asof[backward, by=2, right=in order, rows=N x M, samples=S]", "asof[..., right=sorted: <sort>, dropped null keys=K, ...]" or
 * "asof[empty]".  PLX_ASOF_ROUTE=global in the environment (read per call) searches without the LDS sample stage: samples=0. */
int plx_join_asof_indices(int32_t strategy_and_flags, const plx_column* left_by, const plx_column* right_by, int32_t n_by,
                          plx_column left_on, plx_column right_on, const plx_scalar* tolerance, plx_column* out_right_idx);

/* Stable multi-key arg-sort (arg_sort_multiple; polars-core/src/chunked_array/ops/sort/arg_sort_multiple.rs,
 * SortExec polars-mem-engine/src/executors/sort.rs).  descending / nulls_last: n_by flags each, NULL = all 0.
 * nulls_last is an absolute position (not flipped by descending); floats in total order (NaN greatest,
 * -0.0 == +0.0); ties keep input order.  limit >= 0 returns only the first `limit` indices of that order
 * (sort + slice -> top-k, slice_pushdown_lp.rs / polars-stream top_k.rs) without sorting the whole input.
 * *out_idx: PLX_U32 row indices. */
int plx_sort_indices(const plx_column* by, int32_t n_by, const uint8_t* descending, const uint8_t* nulls_last, int64_t limit,
                     plx_column* out_idx);

/* Key-hash partitioning for the multi-GPU exchange: partition p of row i is
 * mulhi(dirty_hash(key[i]) * seed', n_partitions) (HashPartitioner; nulls -> 0).
 * out_perm (PLX_U32, len rows) lists row indices grouped by partition;
 * counts_out[n_partitions] (host) receives rows per partition. */
int plx_hash_partition(plx_column key, int32_t n_partitions, uint64_t seed, plx_column* out_perm,
                       int64_t* counts_out);

/* ---- frames ------------------------------------------------------------- */
int plx_frame_new(const char* const* names, const plx_column* cols, int32_t n_cols, plx_frame* out);
int plx_frame_free(plx_frame f);
/* Vertical concatenation (polars.concat(how="vertical"), crates/polars-core/src/frame/mod.rs:609 vstack_mut): same column names and dtypes in
 * every frame; columns are copied device-to-device, validity bitmaps merged at bit granularity.  Used by multi-file scans. */
int plx_frame_concat(const plx_frame* frames, int32_t n_frames, plx_frame* out);
int plx_frame_shape(plx_frame f, int64_t* height, int32_t* width);
/* name_out points into library-owned storage valid until the frame is freed. */
int plx_frame_column(plx_frame f, int32_t i, const char** name_out, plx_column* col_out);
/* dtypes_out[width] (plx_dtype) of the frame's columns. */
int plx_frame_dtypes(plx_frame f, int32_t* dtypes_out);
/* Download every column with one stream synchronisation: values_out[i] / validity_out[i] as in
 * plx_column_to_host (validity_out[i] may be NULL), has_validity_out[width]. */
int plx_frame_to_host(plx_frame f, void* const* values_out, uint8_t* const* validity_out, int32_t* has_validity_out);

/* ---- plan execution (Executor seam) ------------------------------------ */
typedef enum plx_aexpr_kind {
  PLX_AE_COLUMN = 0,  /* name */
  PLX_AE_LITERAL = 1, /* dtype, lit, is_null */
  PLX_AE_BINARY = 2,  /* op = plx_operator, lhs, rhs */
  PLX_AE_CAST = 3,    /* lhs, dtype */
  PLX_AE_AGG = 4,     /* op = plx_agg_op, lhs */
  PLX_AE_LEN = 5,     /* pl.len() */
  PLX_AE_ALIAS = 6,   /* lhs, name */
  PLX_AE_NOT = 7,     /* lhs (boolean) */
  PLX_AE_IS_NULL = 8,     /* lhs -> Boolean, never null (FunctionExpr::Boolean(IsNull)) */
  PLX_AE_IS_NOT_NULL = 9, /* lhs -> Boolean, never null */
  PLX_AE_FILL_NULL = 10,  /* lhs, rhs = non-null literal of the same dtype (fill_null(literal)); inside fused pipelines only */
  PLX_AE_TERNARY = 11,    /* when(cond).then(lhs).otherwise(rhs): cond Boolean, lhs / rhs of one dtype (type coercion casts upstream).  A row takes lhs where cond is
                           * valid and true and rhs everywhere else (a null cond selects rhs); value and validity are those of the chosen side.  Output name: that of lhs */
  PLX_AE_BITMAP_LOOKUP = 12, /* lhs = an integer expression, lit.u = a plx_column of dtype PLX_BOOL without nulls (the lookup bitmap; the caller keeps the handle alive until
                           * the plan has run).  Result: Boolean, bit `value` of the bitmap, false outside [0, len(bitmap)), null where lhs is null: set membership over a
                           * dense code range.  Fused pipelines test the bit inside their scan (at most 2 bitmaps per program, semi-join membership bitmaps included; a
                           * plan that needs more runs per node), the per-node path with plx_bitmap_lookup's kernel.  Output name: that of lhs */
  PLX_AE_TEMPORAL = 13,   /* lhs = a Date (PLX_I32 days) or Datetime (PLX_I64 ticks) expression, op = the part (plx_temporal_part), lit.u = the unit (plx_time_unit).
                           * Result: the part in its own dtype (plx_temporal_part), null exactly where lhs is null.  Fused pipelines compute it inside their scan
                           * (OP_DATEPART), the per-node path with plx_temporal_part's kernel.  As a group key month, day, quarter, weekday, ordinal_day, hour, minute and
                           * second have a range known without a pass over the data; year and date take theirs from the operand column's range, which costs one min / max
                           * pass over that column (cached on it) when nobody knows it yet.  Output name: that of lhs */
  PLX_AE_WINDOW = 14,     /* lhs = the function, rhs = arena index of the first PLX_AE_WINDOW_KEY link (Expr.over with mapping_strategy "group_to_rows").  The function reduces
                           * to one value per partition: it holds at least one PLX_AE_AGG / PLX_AE_LEN and every column reference in it sits below one (anything else is
                           * PLX_ERR_UNSUPPORTED: window functions that do not aggregate are not built).  Result: on every row the value of the row's partition, with that
                           * value's validity, in the dtype the aggregate has in a group-by; height and row order are the input's.  Partitions form as group-by groups do
                           * (a null key is a partition of its own, NaN == NaN, -0 == +0).  Legal in the expressions of PLX_IR_SELECT / PLX_IR_HSTACK and in the predicate
                           * of PLX_IR_FILTER, anywhere inside them; in the keys or aggregates of a PLX_IR_GROUPBY it is PLX_ERR_INVALID.  Windows of one node that share
                           * their key list run one group-by, one row -> group map and one broadcast; fused pipelines decline the kind by name.  Output name: that of lhs */
  PLX_AE_WINDOW_KEY = 15, /* one link of a window's key list: lhs = a key expression (no aggregate inside: PLX_ERR_INVALID), rhs = the next link or -1.  1..8 links
                           * (more is PLX_ERR_UNSUPPORTED).  A link anywhere but below a PLX_AE_WINDOW, and a window without a link, are PLX_ERR_INVALID at plan import */
  PLX_AE_CUMULATIVE = 16, /* lhs = a row-level operand (no aggregate, window, cumulative or ranking node inside: PLX_ERR_UNSUPPORTED naming it), op = the plx_cum_op
                           * (outside 0..3: PLX_ERR_INVALID at import), lit.u = reverse (0 / 1: the scan runs from the last row to the first).  Result: one value per
                           * row in the dtype of plx_cum_op, the operand's validity (COUNT: none), height and row order the input's.  The partition is the whole column, or,
                           * as the lhs of a PLX_AE_WINDOW, each partition of its keys in the frame's row order.  Legal where a window is; in the keys or aggregates of a
                           * PLX_IR_GROUPBY it is PLX_ERR_INVALID.  Nodes of one select / with_columns / filter that share their key list share one stable sort of the
                           * rows and one head mask; fused pipelines decline the kind by name.  Output name: that of lhs */
  PLX_AE_RANK = 17,       /* lhs = a row-level operand (as for PLX_AE_CUMULATIVE), op = the plx_rank_method (outside 0..4: PLX_ERR_INVALID at import), lit.u = descending
                           * (0 / 1).  Result: PLX_F64 (AVERAGE) or PLX_U32 with the operand's validity; whole column, or per partition as the lhs of a PLX_AE_WINDOW.
                           * Nodes that share (keys, operand, descending) share one sort.  Output name: that of lhs */
  PLX_AE_SHIFT = 18,      /* lhs = a row-level operand (as for PLX_AE_CUMULATIVE), op = 0 (shift) or 1 (diff), lit.i = n (any int64), rhs = the arena index of the fill
                           * literal (a non-null PLX_AE_LITERAL of the operand's dtype; shift only) or -1: vacated rows are null.  Result: shift keeps the dtype, diff
                           * widens unsigned operands (plx_shift); one value per row.  Whole column, or per partition as the lhs of a PLX_AE_WINDOW.  Legal where
                           * PLX_AE_CUMULATIVE is; shares that kind's stable sort and head mask per key list.  Output name: that of lhs */
  PLX_AE_ROLLING = 19     /* lhs = a row-level operand, op = the plx_rolling_op (outside 0..3: PLX_ERR_INVALID at import), lit.u = window_size in bits 0..31,
                           * min_samples in bits 32..62, center in bit 63 (window_size < 1 or min_samples outside 1..window_size: PLX_ERR_INVALID at import).  Result:
                           * the dtype of plx_rolling_op, a validity of its own.  Placement and sharing as for PLX_AE_SHIFT.  Output name: that of lhs */
} plx_aexpr_kind;

/* polars_plan::dsl::Operator subset */
typedef enum plx_operator {
  PLX_OP_EQ = 0, PLX_OP_NE = 1, PLX_OP_LT = 2, PLX_OP_LE = 3, PLX_OP_GT = 4, PLX_OP_GE = 5,
  PLX_OP_PLUS = 6, PLX_OP_MINUS = 7, PLX_OP_MULTIPLY = 8, PLX_OP_TRUE_DIVIDE = 9,
  PLX_OP_FLOOR_DIVIDE = 10, PLX_OP_MODULUS = 11, PLX_OP_AND = 12, PLX_OP_OR = 13, PLX_OP_XOR = 14
} plx_operator;

typedef struct plx_aexpr {
  int32_t kind; /* plx_aexpr_kind */
  int32_t op;   /* plx_operator or plx_agg_op; PLX_AE_CUMULATIVE: plx_cum_op; PLX_AE_RANK: plx_rank_method; PLX_AE_SHIFT: 0 shift / 1 diff; PLX_AE_ROLLING: plx_rolling_op */
  int32_t lhs;  /* arena index of the (left) input, -1 if none */
  int32_t rhs;  /* arena index of the right input, -1 if none */
  int32_t dtype; /* literal dtype / cast target (plx_dtype) */
  int32_t is_null; /* literal is NULL */
  plx_scalar lit;   /* PLX_AE_LITERAL: the value; PLX_AE_BITMAP_LOOKUP: lit.u = the lookup bitmap's plx_column handle; PLX_AE_TEMPORAL: lit.u = the plx_time_unit;
                     * PLX_AE_AGG of PLX_AGG_VAR / PLX_AGG_STD: lit.u = ddof; of PLX_AGG_QUANTILE: lit.f64 = q (and dtype = the plx_quantile_interpolation); PLX_AGG_N_UNIQUE carries nothing;
                     * PLX_AE_CUMULATIVE: lit.u = reverse; PLX_AE_RANK: lit.u = descending; PLX_AE_SHIFT: lit.i = n; PLX_AE_ROLLING: lit.u = the packed parameters;
                     * read for those kinds only */
  const char* name; /* column name / alias */
  int32_t cond;     /* PLX_AE_TERNARY: arena index of the predicate; read for that kind only (appended last: arenas of earlier callers never carry the kind) */
} plx_aexpr;

typedef enum plx_ir_kind {
  PLX_IR_SCAN = 0,    /* frame */
  PLX_IR_FILTER = 1,  /* input, predicate */
  PLX_IR_SELECT = 2,  /* input, exprs */
  PLX_IR_HSTACK = 3,  /* input, exprs (with_columns) */
  PLX_IR_GROUPBY = 4, /* input, keys, exprs (aggs), maintain_order */
  PLX_IR_JOIN = 5,    /* input, input_right, keys (left_on), keys_right (right_on), how, suffix, maintain_order (plx_join_order), coalesce.  Key shapes that are joined:
                       * 1 key column; 2..8 key columns of integer, Boolean or float dtype, where column j has the same dtype on both sides (more than 8:
                       * PLX_ERR_UNSUPPORTED naming the limit).  A null in any key part makes the row's key null: it matches nothing.  Floats compare in the
                       * total order (NaN == NaN, -0 == +0).  The route is visible in the plan description: "packed N key columns into Int64; hash_join[...]"
                       * when the joint value ranges bit-pack into 63 bits, "wide_hash_join[words=N (why), ...]" / wide_hash_semi_join / wide_hash_anti_join
                       * otherwise (a table of row ids whose key words are compared column by column: any dtype mix, any value range). */
  PLX_IR_SORT = 6,    /* input, keys (by), sort_descending[n_keys], sort_nulls_last[n_keys] (IR::Sort; always stable) */
  PLX_IR_SLICE = 7,   /* input, slice_offset (negative: from the end), slice_len (IR::Slice); directly above a Sort it becomes top-k */
  PLX_IR_DISTINCT = 8, /* input, keys (the subset as column expressions, 1..8: more is PLX_ERR_UNSUPPORTED), how = the plx_unique_keep (outside 0..3: PLX_ERR_INVALID at
                       * plan import), maintain_order 0 / 1 (IR::Distinct).  The rows that are distinct over the keys, ALWAYS in the input's row order: one stable sort of
                       * the keys, a Boolean row mask, one filter of every column -- so maintain_order = 1 is honoured and 0 loses nothing. */
  PLX_IR_JOIN_ASOF = 9 /* input, input_right, keys / keys_right (the by parts, then `on` LAST; n_keys == n_keys_right, 1..8: more is PLX_ERR_UNSUPPORTED), how = a
                       * plx_asof_strategy OR'd with PLX_ASOF_STRICT, predicate = the arena index of a non-null, non-negative PLX_AE_LITERAL holding the tolerance in
                       * the `on` dtype's family (an integer literal for integer / Date / Datetime, a float literal for floats) or -1, suffix and coalesce as in
                       * PLX_IR_JOIN (the rules of a left join), maintain_order must be 0.  A bad strategy, mismatched key counts, a tolerance that is no literal or
                       * is negative and maintain_order != 0 are PLX_ERR_INVALID at plan import.  Output: one row per left row in left order; the left columns are
                       * the input's own (not gathered), each right column is gathered at the matched row (plx_join_asof_indices states the match). */
} plx_ir_kind;

/* Row order of a PLX_IR_JOIN's output (plx_ir.maintain_order of a join node; JoinArgs::maintain_order / MaintainOrderJoin of the reference).
 *   NONE        unspecified: whatever the route produces (partition order on the partitioned probes, the other side's order when the
 *               requested side became the build side, newest row first among duplicate build keys).
 *   LEFT        output rows are in non-decreasing left row index; the order among the rows of one left row is unspecified.
 *   LEFT_RIGHT  sorted by (left row index, right row index): a total order, the output is unique.
 *   RIGHT, RIGHT_LEFT  the mirror image.
 * PLX_JOIN_LEFT: LEFT and LEFT_RIGHT (an unmatched left row is one output row at its left position, right columns null); RIGHT and
 * RIGHT_LEFT return PLX_ERR_UNSUPPORTED with a message that names maintain_order (where the rows without a right index would go is not
 * defined here).  PLX_JOIN_RIGHT is the mirror image: NONE, RIGHT and RIGHT_LEFT; LEFT and LEFT_RIGHT return PLX_ERR_UNSUPPORTED with a
 * message that names maintain_order.
 * PLX_JOIN_FULL takes all five.  A side's "primary" rows are the rows that carry an index of that side.  LEFT / LEFT_RIGHT: the rows with a
 * left index come first, in the order defined above; the rows without one (unmatched right rows) follow after all of them, in increasing
 * right row index -- so LEFT_RIGHT and RIGHT_LEFT stay total orders with a unique output.  RIGHT / RIGHT_LEFT: the mirror image.  The "no
 * row" sentinel can therefore sit on the primary side of a full join's pair list; the pair list still holds fewer than 2^32 - 1 pairs.
 * PLX_JOIN_SEMI / PLX_JOIN_ANTI return left order whatever the value.  A value outside 0..4 is PLX_ERR_INVALID; the
 * option is never silently ignored.  The join feeding a fused join -> group-by is the one exception: its groups are unordered. */
typedef enum plx_join_order {
  PLX_JOIN_ORDER_NONE = 0,
  PLX_JOIN_ORDER_LEFT = 1,
  PLX_JOIN_ORDER_RIGHT = 2,
  PLX_JOIN_ORDER_LEFT_RIGHT = 3,
  PLX_JOIN_ORDER_RIGHT_LEFT = 4
} plx_join_order;

typedef struct plx_ir {
  int32_t kind; /* plx_ir_kind */
  int32_t input;
  int32_t input_right;
  int32_t predicate;
  plx_frame frame;
  const int32_t* exprs;
  int32_t n_exprs;
  const int32_t* keys;
  int32_t n_keys;
  const int32_t* keys_right;
  int32_t n_keys_right;
  int32_t how; /* PLX_IR_JOIN: plx_join_how; PLX_IR_DISTINCT: plx_unique_keep; PLX_IR_JOIN_ASOF: plx_asof_strategy | PLX_ASOF_STRICT */
  int32_t maintain_order; /* PLX_IR_GROUPBY / PLX_IR_SORT / PLX_IR_DISTINCT: 0 / 1; PLX_IR_JOIN: plx_join_order */
  const char* suffix; /* join suffix, NULL = "_right" */
  const uint8_t* sort_descending; /* PLX_IR_SORT: n_keys flags, NULL = ascending */
  const uint8_t* sort_nulls_last; /* PLX_IR_SORT: n_keys flags, NULL = nulls first */
  int64_t slice_offset;           /* PLX_IR_SLICE */
  int64_t slice_len;              /* PLX_IR_SLICE: rows kept (clamped to the input; slice_offsets, polars-core/src/utils/mod.rs:340-358) */
  int32_t coalesce;               /* PLX_IR_JOIN (JoinArgs::coalesce): 0 = the join kind's default (inner, left and right coalesce; full keeps both keys), 1 = coalesce,
                                   * 2 = keep both key columns; anything else is PLX_ERR_INVALID at plan import; semi / anti ignore it.  A key pair is "plain" when both key
                                   * expressions are plain columns; only plain pairs coalesce.  Output columns:
                                   *   inner / left, coalesce   left columns, then right columns without the plain right keys
                                   *   full, coalesce           the same, each plain left key column holding the left value where the row has a left index, the right key's otherwise
                                   *   right, coalesce          left columns without the plain left keys, then all right columns
                                   *   keep both                all left columns, then all right columns (a key is null where its side has no row)
                                   * A right name that (still) clashes with a left name gets the suffix: a full join on k yields k and k_right.
                                   * The coalesced key of a FULL join is built for key columns of 1, 2, 4 or 8 bytes per value; a Boolean key column (a bitmap) coalesced
                                   * on a full join is PLX_ERR_UNSUPPORTED at execution (keep both keys, or cast the key). */
} plx_ir;

/* plan flags */
#define PLX_PLAN_NO_FUSION 1u /* force one kernel per node (reference-shaped execution) */
#define PLX_PLAN_NO_PARTITION 4u /* high-cardinality group-by: always the HBM-table sink, never the partitioned LDS path */
#define PLX_PLAN_NO_DIRECT_JOIN 2u /* fused join->aggregate: always use the hash table, never the direct-address table */

/* Build the physical plan for IR node `root` and execute it. The output frame is
 * owned by the caller (plx_frame_free). PLX_ERR_UNSUPPORTED means: run this
 * subtree on the CPU engine instead (same contract as docs/user-guide/gpu-support.md). */
int plx_execute_plan(const plx_ir* ir, int32_t n_ir, const plx_aexpr* exprs, int32_t n_exprs, int32_t root,
                     uint32_t flags, plx_frame* out);
/* Compile-only: lowers the `[Filter]* -> Select | GroupBy` pipeline rooted at `root`
 * into its fused register program without launching anything (works on placeholder
 * columns, no GPU needed).  *fusable = 0 with a reason in why_not if the plan needs the
 * one-kernel-per-node path; *static_shape_id >= 0 if a pre-instantiated (AOT) kernel
 * matches.  plx_last_plan_description() then returns a dump of the program. */
int plx_describe_fusion(const plx_ir* ir, int32_t n_ir, const plx_aexpr* exprs, int32_t n_exprs, int32_t root, int32_t* fusable,
                        int32_t* static_shape_id, char* why_not, size_t why_cap);
/* Compile-only, no GPU needed: the complete compiled form of the fusable pipeline rooted at `root` (same arguments as
 * plx_describe_fusion) as a JSON document in buf (NUL-terminated, truncated to cap): register program with immediates,
 * input columns, aggregate cells, key packing / decoding, finalisation of every output.  The CPU tests interpret it row by
 * row (tests/program_eval.py).  PLX_ERR_UNSUPPORTED with the reason in plx_last_error() if not fusable. */
int plx_debug_program_json(const plx_ir* ir, int32_t n_ir, const plx_aexpr* exprs, int32_t n_exprs, int32_t root, char* buf, size_t cap);
/* Run-time kernel specialisation (hiprtc): query shapes without a pre-instantiated kernel get one compiled on
 * first use (inputs of >= PLX_JIT_MIN_ROWS rows, default 2^22; PLX_JIT=0 disables; failures fall back to the
 * generic interpreter).  plx_jit_selftest compiles (does not run: no GPU needed) the kernels of the fused pipeline
 * rooted at `root` -- same arguments as plx_describe_fusion -- and returns PLX_OK, or PLX_ERR_INVALID with the
 * compiler log in plx_last_error().  plx_jit_stats: kernels compiled so far / total compile milliseconds. */
int plx_jit_selftest(const plx_ir* ir, int32_t n_ir, const plx_aexpr* exprs, int32_t n_exprs, int32_t root);
int plx_jit_stats(int32_t* compiled, double* compile_ms);
/* Inputs of at least min_rows rows use the JIT (default 2^22); min_rows < 0 disables it. */
int plx_jit_set_min_rows(int64_t min_rows);
/* Human-readable physical plan (which fused pipeline / kernels were chosen) of the
 * last plx_execute_plan on this thread. */
const char* plx_last_plan_description(void);
/* The inputs that the fused aggregate scans of the calling thread's last plx_execute_plan read through their encoded shadows, one
 * "encoded{l_shipdate:affine16,l_discount:dict8}; " per scan; "" when every scan read its columns as stored.  Kept beside the plan description, not in
 * it: the description names the route, and the route of a query is the same whether its inputs are read plain or encoded. */
const char* plx_last_plan_encodings(void);
/* Rows per wave tile of the process's last fused aggregate scan (whole-frame aggregates or the LDS group table): 512 when it ran over wide tiles, 128 when it did
 * not, 0 before the first.  For tests; the plan description does not say. */
int32_t plx_last_scan_tile_rows(void);
/* LDS cells per group that the process's last LDS-table scan held: the program's aggregate count, or fewer when aggregates share cells (count, integer sum and the
 * f64 sum behind a mean of one small non-negative integer input: 5 for TPC-H Q1's 7 aggregates); 0 before the first.  plx_set_shared_cells(0) keeps one cell per
 * aggregate, like PLX_SHARED_CELLS=0 in the environment (read once, at the first scan). */
int32_t plx_last_lds_cells(void);
void plx_set_shared_cells(int32_t on);
/* The tail of a group-by on the LDS-table route: one kernel compacts the table, finalises every output column and writes one result block, which the host fetches
 * in one copy behind one synchronisation and keeps as host mirrors of the result columns.  plx_set_groupby_tail(0) keeps the separate compaction, finalisation and
 * download steps, like PLX_GROUPBY_TAIL=0 in the environment (read once, at the first such group-by).  plx_last_groupby_tail: 1 when the calling thread's last fused
 * group-by finished through the tail kernel, else 0.  plx_last_download_mirrored: 1 when the calling thread's last plx_column_to_host / plx_frame_to_host was served
 * from host mirrors without a device call (every requested column had one), else 0. */
void plx_set_groupby_tail(int32_t on);
int32_t plx_last_groupby_tail(void);
int32_t plx_last_download_mirrored(void);
/* The cell plan as a pure function (no GPU needed).  The program is AOT shape `static_shape_id`, or (-1) the arrays: ops = n_ops x {code, dst, a, b, c}, aggs =
 * n_aggs x {kind, src}.  known / lo / hi: per aggregate, the bound lo <= v <= hi on its source; wg_rows: rows one workgroup can add to its table.  out gets
 * {cells per group, shift, cell[k] for every aggregate, the aggregate whose cell k is read from or -1 for every aggregate}; returns the aggregate count, -1 on bad
 * arguments.  plx_lds_wg_rows: the row bound for a grid of `grid` workgroups over 512-row wide tiles (wide != 0) or 128-row tiles. */
int32_t plx_cell_plan(int32_t static_shape_id, int32_t n_inputs, const int32_t* dtypes, const int32_t* nullable, int32_t n_ops, const uint8_t* ops, int32_t n_aggs, const uint8_t* aggs,
                      const uint8_t* known, const int64_t* lo, const int64_t* hi, uint64_t wg_rows, uint64_t n_rows, int32_t* out);
uint64_t plx_lds_wg_rows(int64_t n_rows, int32_t grid, int32_t wide);
/* The launchers' choice between the two tile sizes, as a pure function (no GPU needed): 1 = 512-row wide tiles.  They are chosen exactly when the program is compiled
 * (ahead of time or at run time), a row is at most 16 bytes of integer or f64 columns (no Boolean, no f32), one of them narrower than eight bytes, no input is nullable or carries a bitmap, n_rows holds one whole tile,
 * every values pointer is aligned to eight rows of its column, and the knob (PLX_WIDE_TILES, default on) is on.  dtypes / nullable / values / validity: n_inputs
 * entries each, pointers as integers.  -1: bad arguments. */
int32_t plx_wide_tiles_choice(int32_t compiled, int32_t knob_on, int64_t n_rows, int32_t n_inputs, const int32_t* dtypes, const int32_t* nullable, const uint64_t* values,
                              const uint64_t* validity);

/* ---- synthetic benchmark data (no reference counterpart: dbgen lives outside the reference tree) -------
 * Fills n_rows of the TPC-H Q1 lineitem columns directly in HBM with a counter-based generator (row i is a pure
 * function of (seed, i): polars_amd/csrc/datagen_device.hpp), so bench.py gets its 25 GB SF100 input without
 * depending on another library's kernels.  out_cols[7], in this order: l_shipdate (PLX_I64, Datetime[us]),
 * l_returnflag (PLX_U8, codes 0..2 = A,N,R), l_linestatus (PLX_U8, 0..1 = F,O), l_quantity (PLX_I64, 1..50),
 * l_extendedprice (PLX_F64), l_discount (PLX_F64, 0..0.10), l_tax (PLX_F64, 0..0.08). */
int plx_datagen_lineitem_q1(int64_t n_rows, uint64_t seed, plx_column* out_cols);
/* The same generator evaluated on the host for rows [row0, row0 + n) (no GPU needed): pins the kernel's arithmetic
 * in the CPU tests and lets callers spot-check a device table.  Plain host arrays, any may be NULL. */
int plx_datagen_lineitem_q1_host(int64_t row0, int64_t n, uint64_t seed, int64_t* shipdate, uint8_t* returnflag, uint8_t* linestatus,
                                 int64_t* quantity, double* extendedprice, double* discount, double* tax);

/* TPC-H Q3 inputs in dbgen row order (both tables ascending in orderkey; sparse keys: 8 of every 32 used; 1-7 lines per
 * order; l_shipdate = o_orderdate + 1..121 days).  out_orders[4]: o_orderkey, o_custkey, o_orderdate (Datetime[us]),
 * o_shippriority (all PLX_I64); out_lineitem[4]: l_orderkey (I64), l_extendedprice (F64), l_discount (F64), l_shipdate (I64). */
int plx_datagen_orders_lineitem(int64_t n_orders, uint64_t seed, plx_column* out_orders, plx_column* out_lineitem);
/* Host twin for orders [order0, order0 + n) of a table of n_orders_total orders: per-order arrays (n entries, n_lines = lines
 * of each order) and the lines of those orders in order (line_cap = capacity of the line arrays; *n_lines_out = lines written,
 * PLX_ERR_INVALID if they do not fit).  Any output may be NULL. */
int plx_datagen_orders_lineitem_host(int64_t order0, int64_t n, int64_t n_orders_total, uint64_t seed, int64_t* orderkey, int64_t* custkey,
                                     int64_t* orderdate, uint32_t* n_lines, int64_t line_cap, int64_t* l_orderkey, double* l_extendedprice,
                                     double* l_discount, int64_t* l_shipdate, int64_t* n_lines_out);
/* One uniform column of n rows: value i = lo + floor(U_i * (hi - lo)), U_i from stream `stream` (0..7) of row i;
 * dtype PLX_I64 / PLX_U32: the integer; PLX_F64: the integer times `scale`.  plx_datagen_uniform_host: rows
 * [row0, row0 + n) into a host array of that dtype. */
/* customer (TPC-H Q3 columns): out_cols[2] = c_custkey (PLX_I64, 1..n in order), c_mktsegment (PLX_U8 codes 0..4 =
 * AUTOMOBILE, BUILDING, FURNITURE, HOUSEHOLD, MACHINERY); plx_datagen_customer_host: rows [row0, row0 + n) on the CPU. */
int plx_datagen_customer(int64_t n_customers, uint64_t seed, plx_column* out_cols);
int plx_datagen_customer_host(int64_t row0, int64_t n, uint64_t seed, int64_t* custkey, uint8_t* segment);
int plx_datagen_uniform(int32_t dtype, int64_t n_rows, uint64_t seed, uint32_t stream, int64_t lo, int64_t hi, double scale, plx_column* out);
int plx_datagen_uniform_host(int32_t dtype, int64_t row0, int64_t n, uint64_t seed, uint32_t stream, int64_t lo, int64_t hi, double scale, void* out);
/* One heavy-tailed PLX_I64 key column in [0, n_keys) (BASELINE config 3's "Zipf s = 1.1" variant): key i = floor(1 / x_i^10) - 1, x_i uniform in
 * [x0, 1) from stream `stream` of row i, x0 = n_keys^(-1/10) handed over as x0_q62 = round(x0 * 2^62); integer fixed-point arithmetic only, so
 * plx_datagen_zipf_host (rows [row0, row0 + n) on the CPU) is bit-identical. */
int plx_datagen_zipf(int64_t n_rows, uint64_t seed, uint32_t stream, uint64_t x0_q62, int64_t n_keys, plx_column* out);
int plx_datagen_zipf_host(int64_t row0, int64_t n, uint64_t seed, uint32_t stream, uint64_t x0_q62, int64_t n_keys, int64_t* out);

/* ---- raw Utf8View / BinaryView keys: device-side dictionary encoding -----------------------------
 * The reference hashes and compares the 16-byte views directly (crates/polars-expr/src/hash_keys.rs:413-452 BinviewKeys,
 * crates/polars-compute/src/binview_index_map.rs; view layout crates/polars-arrow/src/array/binview/view.rs:20-29,55:
 * {len u32, 12 inline bytes} or {len u32, prefix u32, buffer index u32, offset u32}).  plx_strview_dict_encode builds that
 * index map on the device once, when the column enters: `views` = n 16-byte views (host), `data_buffers` = the array's variadic
 * data buffers (host; may be empty when every string is <= 12 bytes).  out_codes = a PLX_U32 column of dictionary codes (validity
 * = the input's; bounds [0, n_distinct) declared), out_dict = the dictionary (code -> string), kept on the device.
 * plx_strview_dict_encode_device: the same for views already in HBM (a PLX_U64 column of 2 n words; `data` a PLX_U8 column or 0).
 * Nulls of a view column in HBM: the raw-view entry points (plx_strview_dict_encode_device, plx_strview_groupby, plx_ipc_read_string_views) carry no bitmap --
 * a null entry is a view whose length word is 0xFFFFFFFF (no Arrow view has it: lengths are non-negative int32; the other 12 bytes zero).
 * plx_strview_stamp_nulls(views, valid) writes those stamps into the column from the array's validity (valid: a PLX_BOOL column of n rows, true = valid -- the
 * BinaryViewArray's validity bitmap, crates/polars-arrow/src/array/binview/mod.rs, imported as Boolean values; a NULL entry of `valid` itself counts as not valid);
 * encode gives such rows null codes.  A view buffer the caller lent (plx_column_from_device) or that another column shares is copied first: the COLUMN behind the
 * handle is stamped, never memory somebody else can see.
 * plx_strdict_to_host: offsets[n_strings + 1] + the concatenated bytes, in code order. */
typedef uint64_t plx_strdict;
int plx_strview_dict_encode(const void* views, const uint8_t* validity, int64_t bit_offset, int64_t n, const void* const* data_buffers, const int64_t* data_sizes,
                            int32_t n_data_buffers, plx_column* out_codes, plx_strdict* out_dict);
int plx_strview_dict_encode_device(plx_column views_u64_pairs, plx_column data_u8, plx_column* out_codes, plx_strdict* out_dict);
int plx_strview_stamp_nulls(plx_column views_u64_pairs, plx_column valid_bool);
/* group_by(<raw Utf8View key>).agg(sum, count, len of ONE numeric column), the key never dictionary-encoded first (kernels_strgroup.hip; the reference's
 * BinviewKeys group-by: crates/polars-expr/src/hash_keys.rs:413-452, crates/polars-compute/src/binview_index_map.rs).  views: a PLX_U64 column of 2 n words in
 * HBM (inline strings: <= 12 bytes each); value: a PLX_F64 / PLX_I64 column of n rows, nulls allowed.  Outputs, one row per distinct string, in no particular
 * order: out_codes = 0 .. G-1 (PLX_U32) with *out_dict holding the G strings in that order; out_sum (the value's dtype; 0 for a group without a valid value),
 * out_count (valid values, PLX_U32), out_len (rows, PLX_U32) -- mean = sum / count.  Rows with a null key (stamped views, above) form one group of their own,
 * as in the reference (a null is a key: hash_keys.rs:413-452 keeps the validity in the key): that group's code is null, its dictionary entry empty.  Returns PLX_ERR_UNSUPPORTED when the input is outside the fast path (a
 * string longer than 12 bytes, more distinct strings than the LDS tables hold, fewer than ~4096 of them): the caller then encodes (plx_strview_dict_encode_device) and groups on the codes. */
int plx_strview_groupby(plx_column views_u64_pairs, plx_column value, plx_column* out_codes, plx_strdict* out_dict, plx_column* out_sum, plx_column* out_count, plx_column* out_len);
/* ---- string predicates: str.starts_with / ends_with / contains(literal) -------------------------------
 * The pattern is `pattern_len` bytes (the UTF-8 bytes of a string, or any bytes for binary data) of at most PLX_STR_MATCH_MAX_PATTERN = 64; a longer one is
 * PLX_ERR_UNSUPPORTED.  Comparison is byte-wise, a zero byte is an ordinary byte, the view's length word decides where a string ends.  A string shorter than the
 * pattern never matches; the empty pattern matches every non-null string.
 *   plx_strdict_match      the predicate for each of the dictionary's n_strings entries, in code order: a PLX_BOOL column without nulls, decided on the device (the
 *                          dictionary is not downloaded).  Together with plx_bitmap_lookup / PLX_AE_BITMAP_LOOKUP over the code column this is the predicate on a
 *                          dictionary-encoded string column: one decision per distinct string, one bit lookup per row.
 *   plx_strview_match      the predicate for each of n raw views in HBM (views_u64_pairs: PLX_U64, 2 n words; data_u8: the bytes behind views over 12 bytes -- buffer
 *                          index 0 -- or 0): a PLX_BOOL column of n rows, null where the view is a null stamp (length word 0xFFFFFFFF).  The column is not encoded.
 *                          A validity bitmap with nulls on views_u64_pairs itself is PLX_ERR_INVALID (it would count words, not views): stamp the nulls.
 *                          A view that points outside data_u8 is PLX_ERR_INVALID ("a view points outside its buffer"), a decision that needs bytes with data_u8 = 0
 *                          is PLX_ERR_INVALID ("needs the data buffer"); the kernel reads nothing out of bounds either way.  Strings of <= 12 bytes, and starts_with
 *                          of <= 4 bytes on any string, are decided from the views alone.
 *   plx_strview_match_host the same decision function on the CPU over host memory (views: n x 16 bytes, data / data_len may be NULL / 0; out_bits / out_valid:
 *                          ceil(n / 64) words each, bits past n zero).  Needs no GPU and no plx_init.
 *   plx_bitmap_lookup      out[i] = lut[codes[i]] for an integer code column (false outside [0, len(lut))); the validity is the codes'.  lut: PLX_BOOL without nulls. */
#define PLX_STR_MATCH_MAX_PATTERN 64
typedef enum plx_str_match_kind { PLX_STR_STARTS_WITH = 0, PLX_STR_ENDS_WITH = 1, PLX_STR_CONTAINS = 2 } plx_str_match_kind;
int plx_strdict_match(plx_strdict dict, int32_t kind, const uint8_t* pattern, int64_t pattern_len, plx_column* out_bool);
int plx_strview_match(plx_column views_u64_pairs, plx_column data_u8, int32_t kind, const uint8_t* pattern, int64_t pattern_len, plx_column* out_bool);
int plx_strview_match_host(const void* views, const uint8_t* data, int64_t data_len, int64_t n, int32_t kind, const uint8_t* pattern, int64_t pattern_len,
                           uint64_t* out_bits, uint64_t* out_valid);
int plx_bitmap_lookup(plx_column codes, plx_column lut_bool, plx_column* out_bool);
int plx_strdict_info(plx_strdict dict, int64_t* n_strings, int64_t* total_bytes);

/* ---- date parts (the reference's dt namespace: crates/polars-time/src/chunkedarray/{date,datetime}.rs) ----
 * A Date is PLX_I32 days since 1970-01-01, a Datetime PLX_I64 ticks since 1970-01-01T00:00 in the unit given; the calendar is the proleptic Gregorian one and the
 * day of an instant is floor(ticks / ticks per day), so instants before the epoch land on their own day.  Defined for every i32 day count and every i64 tick count.
 *   part            output dtype   values
 *   YEAR            PLX_I32
 *   MONTH           PLX_I8         1..12
 *   DAY             PLX_I8         1..31
 *   QUARTER         PLX_I8         1..4
 *   WEEKDAY         PLX_I8         ISO: Monday = 1 .. Sunday = 7
 *   ORDINAL_DAY     PLX_I16        1..366
 *   HOUR MINUTE SECOND  PLX_I8     0..23, 0..59, 0..59; a Datetime only
 *   DATE            PLX_I32        the day count (a Date); a Datetime only.  (A ms Datetime beyond +-5.8e6 years keeps the low 32 bits, as the cast does.)
 *   plx_temporal_part       one kernel over the column (PLX_I32 with PLX_UNIT_DATE, PLX_I64 with a Datetime unit; anything else is PLX_ERR_INVALID); the result shares
 *                           the input's validity bitmap: null exactly where the input is null.
 *   plx_temporal_part_host  the same arithmetic on the CPU over host memory (values: n x i32 for PLX_UNIT_DATE, n x i64 otherwise; out: n values of the part's
 *                           dtype).  Needs no GPU and no plx_init. */
typedef enum plx_time_unit { PLX_UNIT_DATE = 0, PLX_UNIT_MS = 1, PLX_UNIT_US = 2, PLX_UNIT_NS = 3 } plx_time_unit;
typedef enum plx_temporal_part_kind {
  PLX_PART_YEAR = 0, PLX_PART_MONTH = 1, PLX_PART_DAY = 2, PLX_PART_QUARTER = 3, PLX_PART_WEEKDAY = 4, PLX_PART_ORDINAL_DAY = 5,
  PLX_PART_HOUR = 6, PLX_PART_MINUTE = 7, PLX_PART_SECOND = 8, PLX_PART_DATE = 9
} plx_temporal_part_kind;
int plx_temporal_part(plx_column col, int part, int unit, plx_column* out);
int plx_temporal_part_host(const void* values, int unit, int part, int64_t n, void* out);

int plx_strdict_to_host(plx_strdict dict, int64_t* offsets, uint8_t* bytes);
int plx_strdict_free(plx_strdict dict);
/* synthetic Utf8View column (benchmark support, BASELINE config 5 from raw strings): 2 n PLX_U64 words = the inline views of
 * "id%010d" % (lo + floor(U * (hi - lo))) with the same counter-based U as plx_datagen_uniform(stream) */
int plx_datagen_id_views(int64_t n_rows, uint64_t seed, uint32_t stream, int64_t lo, int64_t hi, plx_column* out_views);
/* the same for keys the view does NOT hold: 20-byte strings "id%010d-longkey"; out_views = 2 n PLX_U64 words {length 20 | 4-byte prefix, buffer 0 | offset}, out_data = the
 * (hi - lo) * 20 bytes of the distinct strings, each once, at (value - lo) * 20 -- rows with equal keys share their bytes, as after a gather of a string column
 * (the reference compares such keys through the buffers: crates/polars-compute/src/binview_index_map.rs:106-117 get_long_key) */
int plx_datagen_long_id_views(int64_t n_rows, uint64_t seed, uint32_t stream, int64_t lo, int64_t hi, plx_column* out_views, plx_column* out_data);

/* ---- Parquet scan -> device columns ------------------------------------
 * The scan in front of the hot path: the reference decodes Parquet on the CPU (crates/polars-parquet/src/parquet/read/page/reader.rs:183-300
 * page walk, parquet/read/compression.rs:70-135 decompress, arrow/read/deserialize/{primitive,boolean,dictionary_encoded,binview} decode;
 * driven by crates/polars-io/src/parquet/read/read_impl.rs and crates/polars-stream/src/nodes/io_sources/parquet).  Here the host reads
 * METADATA only (footer, page headers, string dictionary pages); the column-chunk bytes travel to HBM as stored -- compressed and
 * encoded, one DMA per chunk -- and are decoded by kernels: Snappy, RLE / bit-packed hybrid levels and dictionary indices, PLAIN
 * values, null expansion, integer narrowing.
 *   plx_parquet_open            footer + schema; works without a GPU (planning / row-group pruning on any machine)
 *   plx_parquet_column_info     leaf column -> name, plx_dtype (-1: outside the hot path's dtypes: nested, decimal, ...),
 *                               logical kind (0 none, 1 Date = days in PLX_I32, 2 / 5 / 6 Datetime[us / ms / ns] in PLX_I64 -- the stored
 *                               unit is kept; INT96 columns come out as ns like the reference's default --, 3 String / 4 Binary =
 *                               PLX_U32 dictionary codes + plx_parquet_categories), nullable.  `name` stays valid until the next
 *                               call on the same thread.
 *   plx_parquet_chunk_info      codec, bit mask of the page encodings, sizes, and the chunk statistics as scalars of the column's
 *                               dtype (has_min_max = 0 when absent or not usable, e.g. strings); null_count -1 = unknown
 *   plx_parquet_read            row_groups x columns -> frame (rows in row-group order as given).  Codecs: UNCOMPRESSED, SNAPPY and ZSTD (device
 *                               kernels), GZIP and LZ4_RAW (pages inflated by host threads with the library's own decoders, then the same kernels);
 *                               encodings: PLAIN (strings: see plx_parquet_column_strdict), PLAIN_DICTIONARY / RLE_DICTIONARY, RLE levels;
 *                               DELTA_BINARY_PACKED / BYTE_STREAM_SPLIT / DELTA_*_BYTE_ARRAY / INT96 (decoded by host threads);
 *                               data pages v1 and v2; anything else
 *                               is PLX_ERR_UNSUPPORTED naming what it met (the caller decodes that file on the host), a malformed
 *                               file is PLX_ERR_INVALID.  Needs plx_init: there is no host decode path in the library.
 *   plx_parquet_categories*     dictionary of a String / Binary column as of its last read: offsets[n + 1] + concatenated bytes,
 *                               index = code (first-appearance order over the chunk dictionaries read) */
typedef uint64_t plx_parquet;
int plx_parquet_open(const char* path, plx_parquet* out);
int plx_parquet_close(plx_parquet file);
int plx_parquet_shape(plx_parquet file, int64_t* num_rows, int32_t* num_row_groups, int32_t* num_columns);
int plx_parquet_column_info(plx_parquet file, int32_t column, const char** name, int32_t* dtype, int32_t* logical, int32_t* nullable);
/* time zone of a Datetime column: "UTC" when the file marks the timestamps as instants (isAdjustedToUTC; the reference then reads
 * Datetime(unit, "UTC"), crates/polars-parquet/src/arrow/read/schema/convert.rs), "" otherwise.  Valid until the next call on the thread. */
int plx_parquet_column_timezone(plx_parquet file, int32_t column, const char** timezone);
int plx_parquet_row_group_info(plx_parquet file, int32_t row_group, int64_t* num_rows, int64_t* compressed_bytes);
int plx_parquet_chunk_info(plx_parquet file, int32_t row_group, int32_t column, int32_t* codec, uint32_t* encodings, int64_t* compressed_bytes,
                           int64_t* uncompressed_bytes, int32_t* has_min_max, plx_scalar* min, plx_scalar* max, int64_t* null_count);
int plx_parquet_read(plx_parquet file, const int32_t* row_groups, int32_t n_row_groups, const int32_t* columns, int32_t n_columns, plx_frame* out);
int plx_parquet_categories(plx_parquet file, int32_t column, int64_t* n_strings, int64_t* total_bytes);
int plx_parquet_categories_to_host(plx_parquet file, int32_t column, int64_t* offsets, uint8_t* bytes);
/* String columns holding PLAIN (not dictionary-encoded) pages: host threads assemble 16-byte views over the page payloads, the dictionary is
 * built on the device (plx_strview_dict_encode); this hands its handle over (caller frees it with plx_strdict_free).  PLX_ERR_NOT_FOUND
 * when the column's last read went through the chunk dictionaries (plx_parquet_categories*). */
int plx_parquet_column_strdict(plx_parquet file, int32_t column, plx_strdict* out);

/* ---- Arrow IPC file (Feather V2) scan -> device columns -------------------------
 * The reference reads IPC files with crates/polars-arrow/src/io/ipc/read/{file.rs,common.rs,read_basic.rs,schema.rs} (driven by
 * crates/polars-io/src/ipc/ipc_file.rs and crates/polars-stream/src/nodes/io_sources/ipc.rs): FlatBuffers footer + one message per
 * record batch whose body holds the column buffers in Arrow layout.  An uncompressed file needs no decoding at all: the host parses
 * the metadata, every selected buffer goes file -> page-locked staging -> HBM in one DMA, record batches are concatenated in place.
 *   plx_ipc_open / _shape / _column_info / _batch_info   metadata; work without a GPU.  dtype / logical as for plx_parquet_column_info.
 *   plx_ipc_read                batches x columns -> frame.  LZ4_FRAME / ZSTD compressed bodies are inflated per buffer by host threads
 *                               (the library's own decoders); nested columns, non-us timestamps -> PLX_ERR_UNSUPPORTED naming what it met.
 *   strings                     dictionary-encoded in the file: indices become PLX_U32 codes (widened on the device), values through
 *                               plx_ipc_categories*.  Utf8 / LargeUtf8 / Utf8View columns: views are assembled on the host, the
 *                               dictionary is built on the device (plx_strview_dict_encode); plx_ipc_column_strdict hands its handle
 *                               over (caller frees it with plx_strdict_free). */
typedef uint64_t plx_ipc;
int plx_ipc_open(const char* path, plx_ipc* out);
int plx_ipc_close(plx_ipc file);
int plx_ipc_shape(plx_ipc file, int64_t* num_rows, int32_t* num_batches, int32_t* num_columns);
int plx_ipc_column_info(plx_ipc file, int32_t column, const char** name, int32_t* dtype, int32_t* logical, int32_t* nullable);
int plx_ipc_column_timezone(plx_ipc file, int32_t column, const char** timezone);      /* the Timestamp type's timezone string, "" = none */
int plx_ipc_batch_info(plx_ipc file, int32_t batch, int64_t* num_rows, int64_t* body_bytes, int32_t* compressed);
int plx_ipc_read(plx_ipc file, const int32_t* batches, int32_t n_batches, const int32_t* columns, int32_t n_columns, plx_frame* out);
/* One Utf8 / LargeUtf8 / Binary column of the selected record batches as it is needed for a group-by ON THE VIEWS (plx_strview_groupby): *out_views = a PLX_U64 column of
 * 2 n words (16-byte views built on the device from the file's offsets + bytes), *out_data = the bytes behind the views of strings over 12 bytes (PLX_U8; the pair is what
 * plx_strview_dict_encode_device takes when the column has to be encoded after all); null entries are stamped views.  PLX_ERR_UNSUPPORTED: a Utf8View column, a column that is
 * dictionary-encoded in the file -- read those through plx_ipc_read.  (The reference reads string columns as views and hashes them per operator:
 * crates/polars-io/src/ipc/ipc_file.rs, crates/polars-expr/src/hash_keys.rs:413-452.) */
int plx_ipc_read_string_views(plx_ipc file, const int32_t* batches, int32_t n_batches, int32_t column, plx_column* out_views, plx_column* out_data);
int plx_ipc_categories(plx_ipc file, int32_t column, int64_t* n_strings, int64_t* total_bytes);
int plx_ipc_categories_to_host(plx_ipc file, int32_t column, int64_t* offsets, uint8_t* bytes);
int plx_ipc_column_strdict(plx_ipc file, int32_t column, plx_strdict* out);

/* ---- multi-GPU exchange (one process per GPU, RCCL over xGMI) -----------------------------
 * The exchange step of the sharded operators; shape of the reference's in-process exchange:
 * crates/polars-utils/src/hashing.rs:72-121 (HashPartitioner), crates/polars-stream/src/nodes/group_by.rs:252-497
 * (combine_locals).  A communicator wraps an RCCL communicator created from a 128-byte unique id that rank 0 obtains
 * (plx_comm_unique_id) and hands to the other ranks by any means (torch.distributed / MPI / a file).  librccl is
 * loaded with dlopen on first use.
 *   plx_exchange_by_key  every row of `frame` goes to rank plx_hash_partition(key) -- rows with a NULL key to rank 0
 *                        (null_partition(), hashing.rs:111-115); all columns travel in ONE grouped ncclSend / ncclRecv
 *                        all-to-all(v) on the library's stream (nullable and Boolean columns included: validity bitmaps and
 *                        bit-packed values cross as one byte per row and are re-packed on receipt); ONE host round trip
 *                        (the [world x world] row counts, for the receive allocations) and ONE stream synchronisation at the end
 *                        (the gathered per-destination buffers return to the pool only after RCCL is done with them);
 *                        *out = the rows this rank received.  rows_sent / bytes_sent: what left this rank over the fabric.
 *                        The sharded group-by calls it on PARTIAL aggregate rows (polars_amd/dist.py sharded_groupby:
 *                        local pre-aggregation first, group_by.rs:140-497), the sharded join on rows.
 *   plx_allgather_frame  concatenation of every rank's (small) frame in rank order, on every rank (same column kinds).  */
typedef uint64_t plx_comm;
int plx_comm_unique_id(uint8_t* out_128_bytes);
int plx_comm_init(const uint8_t* unique_id_128_bytes, int32_t rank, int32_t world_size, plx_comm* out);
int plx_comm_info(plx_comm comm, int32_t* rank, int32_t* world_size);
int plx_comm_free(plx_comm comm);
int plx_exchange_by_key(plx_comm comm, plx_frame frame, const char* key, uint64_t seed, plx_frame* out, uint64_t* rows_sent, uint64_t* bytes_sent);
int plx_allgather_frame(plx_comm comm, plx_frame frame, plx_frame* out);

/* ---- tracing (NodeTimer equivalent) --------------------------------------- */
typedef struct plx_profile_record {
  char name[48];      /* kernel / node name */
  double start_us;    /* hipEvent time relative to plx_profile_enable */
  double end_us;
  uint64_t algo_bytes; /* algorithmic bytes of this launch (0 if n/a) */
  uint64_t rows;
} plx_profile_record;
int plx_profile_enable(int on);
/* Resolves pending events (synchronises), copies up to cap records, returns count in *n. */
int plx_profile_fetch(plx_profile_record* out, int32_t cap, int32_t* n);
int plx_profile_clear(void);

/* ---- the reference's expression-plugin entry points ------------------------------------
 * What an UNMODIFIED Polars dlopens (crates/polars-plan/src/plans/aexpr/function_expr/plugin.rs:23-137
 * call_plugin, :139-227 plugin_field; normally generated by pyo3-polars-derive/src/lib.rs:140-163):
 *   _polars_plugin_get_version()                 (major << 16) | minor, here (0, 1)   [pyo3-polars derive.rs:56-66]
 *   _polars_plugin_get_last_error_message()      thread-local C string of the last failure   [derive.rs:26-45]
 *   _polars_plugin_<name>(inputs, n, kwargs, kwargs_len, out, ctx)
 *       inputs: n SeriesExport values (crates/polars-ffi/src/version_0.rs:7-16) the CALLEE takes ownership of and
 *       releases (plugin.rs:122-125); out: written on success, out->private_data == NULL on failure; kwargs: pickled
 *       dict (only the key "op" is read); ctx: CallerContext (version_0.rs:136-162), bit 0 = the caller is already
 *       parallel -> the call runs on a HIP stream private to the calling thread.  A length-1 input is a broadcast literal.
 *   _polars_plugin_field_<name>(fields, n, out, kwargs, kwargs_len)   output field (minor 1 signature, plugin.rs:186-207)
 * Functions: plx_cmp / plx_arith (kwargs {"op": "gt" | ... | "add" | ...}) and one symbol per operator for callers
 * without kwargs: plx_eq ne lt le gt ge, plx_add sub mul truediv floordiv mod, plx_filter(values, mask),
 * plx_when_then_otherwise(mask, then, otherwise), plx_dt_part(values; kwargs part, unit), plx_sum mean min max (length-1 result), plx_var / plx_std (length-1 result; kwargs ddof), plx_median (length-1 result), plx_n_unique (length-1 result).  Python side: polars.plugins.register_plugin_function(
 *     plugin_path=".../libpolars_amd.so", function_name="plx_gt", args=[pl.col("a"), pl.lit(3)]).           */
typedef struct plx_caller_context { uint64_t bitflags; } plx_caller_context;
uint32_t _polars_plugin_get_version(void);
char* _polars_plugin_get_last_error_message(void);
#define PLX_DECLARE_PLUGIN(name)                                                                                            \
  void _polars_plugin_##name(const plx_series_export* inputs, size_t n_inputs, const uint8_t* kwargs, size_t kwargs_len,    \
                             plx_series_export* out, const void* ctx);                                                      \
  void _polars_plugin_field_##name(const struct ArrowSchema* fields, size_t n_fields, struct ArrowSchema* out,              \
                                   const uint8_t* kwargs, size_t kwargs_len);
PLX_DECLARE_PLUGIN(plx_cmp) PLX_DECLARE_PLUGIN(plx_arith) PLX_DECLARE_PLUGIN(plx_filter)
PLX_DECLARE_PLUGIN(plx_eq) PLX_DECLARE_PLUGIN(plx_ne) PLX_DECLARE_PLUGIN(plx_lt) PLX_DECLARE_PLUGIN(plx_le) PLX_DECLARE_PLUGIN(plx_gt) PLX_DECLARE_PLUGIN(plx_ge)
PLX_DECLARE_PLUGIN(plx_add) PLX_DECLARE_PLUGIN(plx_sub) PLX_DECLARE_PLUGIN(plx_mul) PLX_DECLARE_PLUGIN(plx_truediv) PLX_DECLARE_PLUGIN(plx_floordiv) PLX_DECLARE_PLUGIN(plx_mod)
PLX_DECLARE_PLUGIN(plx_sum) PLX_DECLARE_PLUGIN(plx_mean) PLX_DECLARE_PLUGIN(plx_min) PLX_DECLARE_PLUGIN(plx_max)
PLX_DECLARE_PLUGIN(plx_when_then_otherwise)   /* (mask, then, otherwise): plx_if_then_else; the field is the `then` input's */
PLX_DECLARE_PLUGIN(plx_dt_part)               /* (values): plx_temporal_part; kwargs {"part": "year" | ..., "unit": "date" | "ms" | "us" | "ns"}; the field is the part's dtype */
/* plx_var / plx_std (values): plx_reduce_var; kwargs {"ddof": 0..255} (absent: 1); a length-1 result; the field is Float64, Float32 for a Float32 input */
void _polars_plugin_plx_var(const plx_series_export* inputs, size_t n_inputs, const uint8_t* kwargs, size_t kwargs_len, plx_series_export* out, const void* ctx);
void _polars_plugin_field_plx_var(const struct ArrowSchema* fields, size_t n_fields, struct ArrowSchema* out, const uint8_t* kwargs, size_t kwargs_len);
void _polars_plugin_plx_std(const plx_series_export* inputs, size_t n_inputs, const uint8_t* kwargs, size_t kwargs_len, plx_series_export* out, const void* ctx);
void _polars_plugin_field_plx_std(const struct ArrowSchema* fields, size_t n_fields, struct ArrowSchema* out, const uint8_t* kwargs, size_t kwargs_len);
/* plx_median (values): plx_reduce_quantile(0.5, PLX_QUANTILE_LINEAR); no kwargs; a length-1 result; the field is Float64, Float32 for a Float32 input */
void _polars_plugin_plx_median(const plx_series_export* inputs, size_t n_inputs, const uint8_t* kwargs, size_t kwargs_len, plx_series_export* out, const void* ctx);
void _polars_plugin_field_plx_median(const struct ArrowSchema* fields, size_t n_fields, struct ArrowSchema* out, const uint8_t* kwargs, size_t kwargs_len);
/* plx_n_unique (values): plx_reduce_n_unique; no kwargs; a length-1 result; the field is UInt32 under the input's name */
void _polars_plugin_plx_n_unique(const plx_series_export* inputs, size_t n_inputs, const uint8_t* kwargs, size_t kwargs_len, plx_series_export* out, const void* ctx);
void _polars_plugin_field_plx_n_unique(const struct ArrowSchema* fields, size_t n_fields, struct ArrowSchema* out, const uint8_t* kwargs, size_t kwargs_len);
/* plx_window_agg (values, key, key...): plx_window_agg of one aggregate; kwargs {"agg": "sum" | "mean" | "min" | "max" | "count" | "len" | "var" | "std" | "quantile" |
 * "median" | "n_unique", "ddof": 0..255, "q": [0, 1], "interpolation": "nearest" | ...}; a result of the inputs' height; the field is the aggregate's group-by dtype
 * under the first input's name */
void _polars_plugin_plx_window_agg(const plx_series_export* inputs, size_t n_inputs, const uint8_t* kwargs, size_t kwargs_len, plx_series_export* out, const void* ctx);
void _polars_plugin_field_plx_window_agg(const struct ArrowSchema* fields, size_t n_fields, struct ArrowSchema* out, const uint8_t* kwargs, size_t kwargs_len);
/* plx_cum (values, key...): plx_cumulative; kwargs {"op": "sum" | "min" | "max" | "count", "reverse": bool}; zero keys: the whole column.  A result of the inputs'
 * height; the field is the plx_cum_op dtype under the first input's name */
void _polars_plugin_plx_cum(const plx_series_export* inputs, size_t n_inputs, const uint8_t* kwargs, size_t kwargs_len, plx_series_export* out, const void* ctx);
void _polars_plugin_field_plx_cum(const struct ArrowSchema* fields, size_t n_fields, struct ArrowSchema* out, const uint8_t* kwargs, size_t kwargs_len);
/* plx_rank (values, key...): plx_rank; kwargs {"method": "average" | "min" | "max" | "dense" | "ordinal", "descending": bool}; the field is Float64 for "average",
 * UInt32 otherwise, under the first input's name */
void _polars_plugin_plx_rank(const plx_series_export* inputs, size_t n_inputs, const uint8_t* kwargs, size_t kwargs_len, plx_series_export* out, const void* ctx);
void _polars_plugin_field_plx_rank(const struct ArrowSchema* fields, size_t n_fields, struct ArrowSchema* out, const uint8_t* kwargs, size_t kwargs_len);
/* plx_shift / plx_diff (values, key...): plx_shift; kwargs {"n": int} (absent: 1; an integer that fits 32 bits).  Vacated rows are null.  The field is the input's
 * (plx_shift) or the widened difference dtype (plx_diff; a Boolean or temporal series is refused) under the first input's name */
void _polars_plugin_plx_shift(const plx_series_export* inputs, size_t n_inputs, const uint8_t* kwargs, size_t kwargs_len, plx_series_export* out, const void* ctx);
void _polars_plugin_field_plx_shift(const struct ArrowSchema* fields, size_t n_fields, struct ArrowSchema* out, const uint8_t* kwargs, size_t kwargs_len);
void _polars_plugin_plx_diff(const plx_series_export* inputs, size_t n_inputs, const uint8_t* kwargs, size_t kwargs_len, plx_series_export* out, const void* ctx);
void _polars_plugin_field_plx_diff(const struct ArrowSchema* fields, size_t n_fields, struct ArrowSchema* out, const uint8_t* kwargs, size_t kwargs_len);
/* plx_rolling (values, key...): plx_rolling; kwargs {"op": "sum" | "mean" | "min" | "max", "window_size": int, "min_samples": int (absent: window_size), "center":
 * bool}; the field is the plx_rolling_op dtype under the first input's name */
void _polars_plugin_plx_rolling(const plx_series_export* inputs, size_t n_inputs, const uint8_t* kwargs, size_t kwargs_len, plx_series_export* out, const void* ctx);
void _polars_plugin_field_plx_rolling(const struct ArrowSchema* fields, size_t n_fields, struct ArrowSchema* out, const uint8_t* kwargs, size_t kwargs_len);

#ifdef __cplusplus
}
#endif
#endif /* POLARS_AMD_H */
