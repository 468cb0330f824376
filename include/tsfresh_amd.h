/*
 * tsfresh_amd C-ABI  --  MI355X (gfx950) feature-extraction hot path.
 *
 * The reference (blue-yonder/tsfresh) is pure Python and has no FFI of its own.  Its plug points for
 * this path are:
 *   - tsfresh/feature_extraction/extraction.py:308  _do_extraction_on_chunk(chunk, fc_parameters)
 *       one (id, kind) series  x  the FCParameters dict  ->  [(id, "kind__calc__params", value), ...]
 *   - tsfresh/feature_extraction/extraction.py:193  _do_extraction  (adapter -> map_reduce -> pivot)
 *   - tsfresh/utilities/distribution.py:74          DistributorBaseClass.map_reduce
 * This header is what a ctypes binding for that path binds instead: the FCParameters dict is compiled
 * to a flat list of "feature specs" (one per output column), the list of series is handed over as one
 * ragged buffer (values + offsets), and the result is the dense [n_series x n_cols] float64 matrix
 * that tsfresh/feature_extraction/data.py:86 (pivot) would otherwise assemble from tuples.
 *
 * Plain C, plain pointers and sizes, no torch types.  All functions return 0 on success or a
 * negative tsfa_status; the message is available from tsfa_last_error() (thread-local).
 */
#ifndef TSFRESH_AMD_H
#define TSFRESH_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSFA_VERSION 100 /* 0.1.0 */

typedef enum tsfa_status {
    TSFA_OK = 0,
    TSFA_ERR_INVALID = -1,     /* bad argument */
    TSFA_ERR_UNSUPPORTED = -2, /* calculator / parameter not implemented natively */
    TSFA_ERR_NO_DEVICE = -3,   /* no HIP device: the library never falls back to the CPU */
    TSFA_ERR_HIP = -4,         /* HIP runtime error */
    TSFA_ERR_TOO_LONG = -5     /* a series of more than 33 554 431 samples (every calculator takes any length up to there; since
                                  round 6 also sample_entropy / approximate_entropy, which used to stop at 65 535) */
} tsfa_status;

/* element type of the ragged value buffer */
/* (tsfa_extract* take TSFA_F32 / TSFA_F64 samples; the integer types and TSFA_BOOL name id / sort-key columns and the value
 * columns tsfa_pack_device converts to float64; TSFA_F16 / TSFA_BF16 are accepted by tsfa_pack_dense ONLY, which converts them
 * to float32 -- every other entry point refuses them as it refuses an unknown type) */
typedef enum tsfa_dtype {
    TSFA_F32 = 0, TSFA_F64 = 1, TSFA_I64 = 2, TSFA_I32 = 3,
    TSFA_I8 = 4, TSFA_I16 = 5, TSFA_U8 = 6, TSFA_U16 = 7, TSFA_U32 = 8, TSFA_U64 = 9, TSFA_BOOL = 10, /* one byte, 0 | 1 */
    TSFA_F16 = 11,  /* IEEE binary16 */
    TSFA_BF16 = 12  /* bfloat16: the upper half of a binary32 */
} tsfa_dtype;

/* where the caller's buffers live */
typedef enum tsfa_memspace { TSFA_HOST = 0, TSFA_DEVICE = 1 } tsfa_memspace;

/*
 * One output column: a calculator of tsfresh/feature_extraction/feature_calculators.py plus one
 * parameter combination of the FCParameters dict (tsfresh/feature_extraction/settings.py:165-280).
 * `calc` comes from tsfa_calc_id("<calculator name>"); the meaning of p[] per calculator is listed in
 * tsfresh_amd/csrc/tsfa_specs.h (string-valued parameters such as attr / f_agg are enum codes).
 * matrix_profile (feature_calculators.py:2385) is served for one explicit integer window: p[0] = windows >= 4,
 * p[1] = min / max / mean / median / 25 / 75 as 0 .. 5; columns of one window share one profile per series.
 */
typedef struct tsfa_feature_spec {
    int32_t calc;
    int32_t reserved;
    double p[4];
} tsfa_feature_spec;

typedef struct tsfa_plan tsfa_plan; /* opaque; owned by the library */

/* ---- library / device ---- */
int tsfa_version(void);
/* number of visible HIP devices (0 if none; never fails) */
int tsfa_device_count(void);
/* thread-local message of the last failing call on this thread ("" if none) */
const char *tsfa_last_error(void);

/* ---- calculator registry ---- */
/* id of a feature calculator by its tsfresh name (feature_calculators.py), or -1 if not native */
int tsfa_calc_id(const char *name);
/* inverse of tsfa_calc_id; NULL if out of range */
const char *tsfa_calc_name(int calc);
/* number of native calculators */
int tsfa_calc_count(void);

/* ---- plan: the compiled FCParameters dict for one kind ---- */
/*
 * specs[i] describes output column i.  `device` is the HIP device ordinal.  Replaces the Python loop
 * over fc_parameters.items() in extraction.py:339-378.  Returns TSFA_ERR_UNSUPPORTED (and names the
 * offender in tsfa_last_error) for a calculator/parameter combination that has no kernel.
 */
int tsfa_plan_create(const tsfa_feature_spec *specs, int32_t n_specs, int32_t device, tsfa_plan **out_plan);
/*
 * tsfa_plan_create for FCParameters whose parameter values include ARRAYS: `data` is a pool of n_data float64 (copied; the
 * caller keeps ownership) that such specs point into.  Today one calculator has an array parameter: query_similarity_count
 * (feature_calculators.py:2475-2519, {"query": Q, "threshold": thr, "normalize": norm}) --
 *     p[0] = thr, p[1] = norm (0 | 1), p[2] = offset of Q in the pool, p[3] = len(Q)  (0: query=None, the column is NaN).
 * TSFA_ERR_INVALID if a spec points outside the pool.  tsfa_plan_create is the case n_data = 0.
 */
int tsfa_plan_create_with_data(const tsfa_feature_spec *specs, int32_t n_specs, const double *data, int64_t n_data,
                               int32_t device, tsfa_plan **out_plan);
int32_t tsfa_plan_n_cols(const tsfa_plan *plan);
void tsfa_plan_destroy(tsfa_plan *plan);

/*
 * Extract all planned features for n_series ragged series.  Replaces distributor.map_reduce(
 * _do_extraction_on_chunk, ...) + pivot (extraction.py:294-304) for one kind.
 *
 *   values   concatenated samples, series s occupies [offsets[s], offsets[s+1]);  dtype per `dtype`
 *   offsets  n_series+1 int64, offsets[0] may be non-zero (a view into a larger buffer)
 *   out      row-major [n_series x ld_out] float64, ld_out >= n_cols; caller-allocated, caller-owned;
 *            NaN where the reference yields NaN
 *   space    TSFA_HOST: values/offsets/out are host pointers; the batch is staged through HBM in row chunks, copy-in
 *            of chunk c + 1 and copy-out of chunk c - 1 overlapping the kernels of chunk c (three streams);
 *            TSFA_DEVICE: all three are device pointers on the plan's device
 * A batch whose lengths span more than a factor of two is launched by length class (each class with the LDS carve and
 * workgroup size of ITS longest series), so one long series does not slow a batch of short ones down.
 *   stream   a hipStream_t (or NULL = the plan's own stream).  With TSFA_DEVICE and a non-NULL
 *            stream the call returns after enqueueing; otherwise it is synchronous.
 *
 * One plan may be used by one host thread at a time; plans on different devices are independent.
 */
int tsfa_extract(tsfa_plan *plan, const void *values, int32_t dtype, const int64_t *offsets,
                 int64_t n_series, double *out, int64_t ld_out, int32_t space, void *stream);

/*
 * tsfa_extract plus the per-sample abscissa that linear_trend_timewise regresses on
 * (feature_calculators.py:2274: hours since the series' first timestamp, taken from the DatetimeIndex
 * the reference hands the calculator as x.index, extraction.py:345-360).
 *
 *   times    float64, laid out exactly like `values` (same offsets, same memory space); NULL is allowed
 *            only for plans without linear_trend_timewise columns (TSFA_ERR_INVALID otherwise).
 */
int tsfa_extract_timed(tsfa_plan *plan, const void *values, int32_t dtype, const double *times,
                       const int64_t *offsets, int64_t n_series, double *out, int64_t ld_out,
                       int32_t space, void *stream);

/*
 * The window form: series s is the view values[starts[s] .. ends[s]) of one shared buffer; views may overlap.
 * This is what tsfresh/utilities/dataframe_functions.py:340-372 (_roll_out_time_series, called by
 * roll_time_series :377) produces by COPYING every window into a new DataFrame before extract_features is
 * called on it (the forecasting workflow, BASELINE configs[4]); here the windows stay views.
 * tsfa_extract / tsfa_extract_timed are the special case ends = starts + 1 (a ragged batch).
 *
 *   starts, ends   n_series int64 each (same memory space as values); 1 <= ends[s] - starts[s] <= 33554431 (TSFA_ERR_TOO_LONG)
 *   times          as in tsfa_extract_timed, indexed like values; the kernel regresses on
 *                  times[i] - times[starts[s]], i.e. hours since the window's own first stamp
 */
int tsfa_extract_windows(tsfa_plan *plan, const void *values, int32_t dtype, const double *times,
                         const int64_t *starts, const int64_t *ends, int64_t n_series, double *out,
                         int64_t ld_out, int32_t space, void *stream);

/*
 * The row chunks into which the TSFA_HOST form of tsfa_extract* cuts a batch of n_series series on this plan (at least 4096
 * series each, at most 16; the plan's "host_chunks" option and profiling change them): cuts[c] .. cuts[c + 1] is chunk c.
 * A launch sizes its workgroups by the lengths of ITS batch, and the workgroup size decides the association of the
 * reductions: a caller that extracts the same series chunk by chunk with TSFA_DEVICE pointers gets, with these cuts, the
 * launches of the TSFA_HOST form and bit-equal features.  cap: entries of `cuts` (>= n_chunks + 1, 17 always suffice).
 * Returns the number of chunks (0 for n_series == 0) or a negative tsfa_status.
 */
int tsfa_extract_chunks(const tsfa_plan *plan, int64_t n_series, int64_t *cuts, int32_t cap);

/*
 * Timing of the kernels of the last tsfa_extract on this plan, measured with HIP events on the
 * stream the kernels were launched on.  names[i] / ms[i] for i < returned count (<= cap).
 * Only recorded when tsfa_plan_set_profiling(plan, 1) was called before the extract.
 */
int tsfa_plan_set_profiling(tsfa_plan *plan, int32_t enable);
int32_t tsfa_plan_last_timings(const tsfa_plan *plan, const char **names, float *ms, int32_t cap);

/*
 * What the last tsfa_extract* on this plan launched: one record per (kernel family, launch group), in launch order, written
 * just before the family's launch when every launch parameter has its final value.  Read-only diagnostics (the tests read
 * which build, workgroup size and scratch layout a length was routed to); recording changes no launch.  The list is cleared at
 * the start of every extract; the TSFA_HOST form appends the records of its row chunks one after the other.
 *   family        0 BASIC, 1 SORT, 2 SPECTRAL, 3 AR, 4 ENTROPY, 5 CWT (number_cwt_peaks), 6 SEQ, 7 TREND, 8 MPROFILE
 *   length_class  index of the launch group (0 when the batch is one group)
 *   max_len       longest series of the group: what the carve is sized for
 *   n_series      series of the group
 *   threads       workgroup size of the family kernel
 *   lds_bytes     the family's carve for max_len with 8-byte samples, the number the route is decided by: bytes of LDS in the
 *                 LDS build, bytes of a workgroup's HBM scratch slot (before rounding to 256) in the long-series build
 *                 (SORT, LDS build: what the launch really carves, in the input precision)
 *   long_build    1: the HBM-scratch build (tsfa_kernels_long.hip) runs, 0: the LDS build
 *   variant       ENTROPY: the sweep (0 / 1 pair sweeps, 2 / 3 bit-matrix sweeps, 4 the bit-matrix sweep over HBM)
 *                 CWT: bit 0 the row values are kept in LDS, bit 1 the matrix-core convolutions
 *                 SEQ: `bins` values parsed per launch | (symbol rows in HBM) << 8
 *                 SPECTRAL: 1 chirp-z scratch attached
 *                 SORT: bit 0 a k_perm launch is queued for the group, bit 1 one wavefront per series with a sorted copy,
 *                       bit 2 one wavefront per series with the entropy kernel's 16-bit order in its place
 *                 AR: 1 the second pass works in HBM scratch    others: 0
 * Returns the number of records; at most `cap` are written to `out` (cap = 0 or out = NULL only counts).
 */
typedef struct tsfa_launch_info {
    int32_t family;
    int32_t length_class;
    int32_t max_len;
    int32_t threads;
    int64_t n_series;
    int64_t lds_bytes;
    int32_t long_build;
    int32_t variant;
} tsfa_launch_info;
int32_t tsfa_plan_last_launches(const tsfa_plan *plan, tsfa_launch_info *out, int32_t cap);

/*
 * Launch options of one plan, set by the caller who owns it.  The library reads NO environment variable; what used to be
 * debugging switches of the environment are named options here, each an alternative ROUTE to the same numbers (the tests
 * compare both ways) or a diagnostic pre-fill:
 *   "length_classes" 0|1   launch a batch whose lengths span more than 2x class by class (default 1)
 *   "stats_share"    0|1   k_basic's per-series statistics serve the other families (1)
 *   "select"         0|1   median / quantile-only plans by selection instead of a sort (1)
 *   "fused_minimal"  0     MinimalFCParameters-shaped plans through the family kernels instead of k_stream
 *   "perm_fused"     0     permutation_entropy inside k_sort instead of k_perm
 *   "bluestein"      0|1   chirp-z transform for long spectra of non-power-of-two length (1); "bluestein_min" n: its crossover
 *   "gscratch_slots" n     cap of the chirp-z scratch slots (several launches per group)
 *   "entropy_route"  0|1|2 bit-matrix sweep | windowed pair sweep | general kernel
 *   "force_long"     0|1   the HBM-scratch build of the family kernels whatever the length
 *   "row_form"       0|1   BASIC / TREND columns of series of <= 256 samples four series to a wavefront (1)
 *   "sort_waves"     1|2   k_sort up to 2048 samples: one wavefront per series (1), or the two-wavefront form it replaced (2)
 *   "seq_rows"       -1|0|1 lempel_ziv_complexity's symbol rows in LDS (0), in HBM (1), or in HBM where that puts more series on a CU (-1, default)
 *   "cwt_links"      0|1   number_cwt_peaks with n <= 5: ridge lines linked column by column (1), or by the general linker of the wider plans (0)
 *   "host_chunks"    n     row chunks of the TSFA_HOST pipeline (0: by batch size)
 *   "side_lane"      mask  two lanes: bit f = family f (enum tsfa_family) runs on a low-priority side stream beside the others,
 *                          behind the main lane's ENTROPY family; 0 = one lane.  Default: SEQ | TREND.  BASIC, SORT and ENTROPY
 *                          are refused (they carry the shared statistics and the shared sample order).  Never while profiling,
 *                          beyond 4096 samples
 *   "fail_after"     f     test hook: the batch returns an error after family f's launches (-1: off)
 *   "fill"           v     pre-fill the result matrix with v before the kernels run (audits: every cell is written anyway)
 * plan == NULL: library-wide options ("relevance_batch" n: columns per sort batch of tsfa_relevance_*).
 * Unknown names return TSFA_ERR_INVALID.  The reference has no counterpart (its knobs are n_jobs / chunksize).
 */
int tsfa_plan_set_option(tsfa_plan *plan, const char *name, double value);

/* Optional: promise that every series of the following tsfa_extract* calls on this plan has min_len <= length <=
 * max_len.  The calls then skip their length scan and the host synchronisation it needs, so device-pointer calls on one
 * stream (e.g. the row chunks of a shard whose results are exchanged chunk by chunk) are enqueued back to back.  A batch
 * outside the promised range is undefined behaviour.  (0, 0) withdraws the promise.  The reference has no counterpart:
 * its per-series dispatch (extraction.py:308) sizes nothing ahead. */
int tsfa_plan_set_length_hint(tsfa_plan *plan, int64_t min_len, int64_t max_len);

/* Host-side packer helper.  The reference groups a long DataFrame into per-(id, kind) pd.Series with a pandas groupby
 * (data.py:233-291, LongTsFrameAdapter); for the usual layout -- rows already grouped by ascending id, every group already
 * in sort order -- the ragged buffer tsfa_extract wants is the value column itself, and all that is needed is ONE
 * multi-threaded pass that (a) proves the layout, (b) finds the group boundaries, (c) performs the reference's NaN check
 * of the value column (data.py:148-167).
 *   ids / sort / values: the columns (sort and values may be NULL), element types per tsfa_dtype
 *   *flags:    TSFA_PACK_UNSORTED  the layout is something else (the caller falls back to a sorting packer)
 *              TSFA_PACK_VALUE_NAN a value is NaN (the caller raises the reference's ValueError)
 *   *n_groups: number of series; tsfa_pack_offsets then writes the n_groups + 1 row offsets (same thread). */
#define TSFA_PACK_UNSORTED 1
#define TSFA_PACK_VALUE_NAN 2
int tsfa_pack_scan(const void *ids, int32_t id_type, const void *sort, int32_t sort_type, const void *values,
                   int32_t value_type, int64_t n_rows, int32_t *flags, int64_t *n_groups);
int tsfa_pack_offsets(int64_t *offsets, int64_t n_groups, int64_t n_rows);

/* Device packer: the same grouping for a frame in ANY row order (rows in time order with the ids interleaved -- the usual
 * sensor log --, tsfresh's long format, a shuffled frame), on the GPU.  Replaces the pandas groupby of LongTsFrameAdapter
 * (data.py:233-291) and WideTsFrameAdapter (:181-230) and the host's factorize + lexsort + gather.  The three columns go to
 * HBM as they are (space: TSFA_HOST pointers are staged, TSFA_DEVICE pointers are used in place), the rows are sorted stably
 * by (id, sort) with an LSD radix sort of order-preserving keys (passes whose digit is constant over all rows are skipped;
 * a frame that is already in order is not sorted at all), group boundaries are found, and the values are gathered into the
 * ragged buffer tsfa_extract* takes with TSFA_DEVICE pointers.  The handle owns that buffer, the int64 offsets
 * (n_groups + 1), the unique ids (ascending, the id column's own element type) and, with TSFA_PACK_KEEP_SORT, the sort
 * column in packed order; tsfa_pack_device_destroy frees all of them.
 *   ids         any integer type of tsfa_dtype except TSFA_BOOL
 *   sort        NULL (stable sort by id alone) or any integer type, TSFA_F32, TSFA_F64 (no NaN; -0.0 equals +0.0)
 *   values      TSFA_F32 stays float32, TSFA_F64 stays float64, TSFA_BOOL and every integer type become float64 exactly as
 *               numpy's astype(float64) (64-bit integers beyond 2^53 round to nearest even)
 *   options     TSFA_PACK_KEEP_SORT or 0
 * Scratch while the call runs: 40 bytes per row (two buffers of 16-byte composite key + 4-byte row index) + 1 KiB per 4096
 * rows + the staged columns; an allocation that fails is TSFA_ERR_HIP with the byte count in the message.  More than
 * 2^32 - 1 rows: TSFA_ERR_TOO_LONG.  No HIP device: TSFA_ERR_NO_DEVICE (there is no CPU route in the library).
 * Synchronous; the handle may be destroyed from any thread.
 *   tsfa_pack_device_flags: TSFA_PACK_VALUE_NAN (a float value is NaN: the caller raises the reference's ValueError,
 *                           data.py:148-167) | TSFA_PACK_IN_ORDER (the rows were already in order: nothing was sorted)
 *   tsfa_pack_device_n_passes: radix passes that ran (0 .. 16)
 *   tsfa_pack_device_values: device pointer and element type (TSFA_F32 | TSFA_F64) of the ragged buffer (n_rows elements)
 *   tsfa_pack_device_offsets: device pointer of the int64 offsets
 *   tsfa_pack_device_copy_ids / _offsets / _sort: copies to host arrays of n_groups ids / n_groups + 1 int64 / n_rows sort
 *                           keys (TSFA_ERR_INVALID without TSFA_PACK_KEEP_SORT) */
#define TSFA_PACK_IN_ORDER 4
#define TSFA_PACK_KEEP_SORT 1
typedef struct tsfa_pack tsfa_pack; /* opaque; owned by the library */
int tsfa_pack_device(const void *ids, int32_t id_type, const void *sort, int32_t sort_type, const void *values,
                     int32_t value_type, int64_t n_rows, int32_t space, int32_t options, int32_t device, tsfa_pack **out_pack);
int64_t tsfa_pack_device_n_rows(const tsfa_pack *pack);
int64_t tsfa_pack_device_n_groups(const tsfa_pack *pack);
int32_t tsfa_pack_device_flags(const tsfa_pack *pack);
int32_t tsfa_pack_device_n_passes(const tsfa_pack *pack);
int tsfa_pack_device_values(const tsfa_pack *pack, const void **values, int32_t *dtype);
const int64_t *tsfa_pack_device_offsets(const tsfa_pack *pack);
/* Device pointer of the pack's unique ids (n_groups elements of the id column's own type, ascending): what
 * tsfa_pack_device_copy_ids copies, for a caller that keeps the ids in HBM.  Valid while the pack (or, for a view, any holder
 * of the set's id buffer) lives. */
const void *tsfa_pack_device_ids(const tsfa_pack *pack);
int tsfa_pack_device_copy_ids(const tsfa_pack *pack, void *ids_host);
int tsfa_pack_device_copy_offsets(const tsfa_pack *pack, int64_t *offsets_host);
int tsfa_pack_device_copy_sort(const tsfa_pack *pack, void *sort_host);
void tsfa_pack_device_destroy(tsfa_pack *pack);

/* Pack set: a frame of several kinds -- tsfresh's long format (one kind column), or a wide frame with several value columns
 * -- is sorted ONCE and hands out one ordinary tsfa_pack per kind.  Replaces, for those two formats, the host's per-kind
 * selection (factorize, nonzero, three gathers per kind) and the K uploads and K sorts of K tsfa_pack_device calls.
 *   tsfa_pack_set_create   sorts the rows stably by (kind, id, sort), the kind being the most significant key, with the keys,
 *                          the LSD radix sort and the pass-skipping rule of tsfa_pack_device.
 *       kinds      NULL (one kind: a wide frame) or any integer type of tsfa_dtype except TSFA_BOOL (callers with string
 *                  kinds pass factorized codes; dense codes below 256 cost one pass, a constant column none)
 *       options    TSFA_PACK_KEEP_SORT or 0
 *     Shortcuts: rows already in (id, sort) order with the kinds interleaved (the usual long frame) run ONLY the kind passes
 *     (the sort is stable); rows already in (kind, id, sort) order run none and the set reports TSFA_PACK_IN_ORDER.
 *     A row heads a series when its (kind, id) differs from its predecessor's: the last series of one kind and the first of
 *     the next may carry the same id.  Kinds may hold different id sets.
 *     Bytes per row: the kind key is not part of the sort's scratch record, a kind pass reads its digit through the row index
 *     (kinds[perm[i]]), so the scratch while the call runs is tsfa_pack_device's 40 bytes per row + 1 KiB per 4096 rows + the
 *     staged id / sort / kind columns.  The set keeps 4 bytes per row (the permutation), the int64 offsets of the whole sorted
 *     frame (n_groups + 1), with several kinds every kind's offsets rebased to its first row (n_groups + n_kinds int64), the
 *     unique ids of every (kind, id) group and, with TSFA_PACK_KEEP_SORT, the sort column in packed order.
 *   tsfa_pack_set_n_kinds  distinct kind values (1 when kinds == NULL)
 *   tsfa_pack_set_copy_kinds  the distinct kind values, ascending, in the kind column's own element type (n_kinds elements);
 *                          TSFA_ERR_INVALID for a set without a kind column
 *   tsfa_pack_set_flags    TSFA_PACK_IN_ORDER;  tsfa_pack_set_n_passes: radix passes that ran (0 .. 24)
 *   tsfa_pack_set_values   gathers ONE value column (n_rows elements, row-aligned with the key columns; conversions and the
 *                          TSFA_PACK_VALUE_NAN flag as in tsfa_pack_device) through the stored permutation into one new buffer
 *                          and writes n_kinds tsfa_pack handles, kind k (ascending) at out_packs[k].  Each handle is a view:
 *                          its values are the kind's row range of that buffer, its offsets start at 0, its ids are the kind's
 *                          own, and every tsfa_pack_device_* accessor and tsfa_extract* work on it unchanged.  A wide frame
 *                          calls it once per value column (one handle per call; the handles share the set's offsets and ids),
 *                          a long frame once.  Scratch: the staged value column.
 * Ownership is reference-counted: the set and the packs may be destroyed in any order (each with its own destroy function);
 * a shared buffer is freed with its last holder, a value buffer with its last view.  More than 2^31 - 1 kinds:
 * TSFA_ERR_TOO_LONG.  Otherwise the errors of tsfa_pack_device. */
typedef struct tsfa_pack_set tsfa_pack_set; /* opaque; owned by the library */
int tsfa_pack_set_create(const void *ids, int32_t id_type, const void *sort, int32_t sort_type, const void *kinds,
                         int32_t kind_type, int64_t n_rows, int32_t space, int32_t options, int32_t device,
                         tsfa_pack_set **out_set);
int32_t tsfa_pack_set_n_kinds(const tsfa_pack_set *set);
int tsfa_pack_set_copy_kinds(const tsfa_pack_set *set, void *kinds_host);
int32_t tsfa_pack_set_flags(const tsfa_pack_set *set);
int32_t tsfa_pack_set_n_passes(const tsfa_pack_set *set);
int tsfa_pack_set_values(tsfa_pack_set *set, const void *values, int32_t value_type, int32_t space, tsfa_pack **out_packs);
/* Row packer: a value MATRIX through a set's permutation in one pass.  For a set made WITHOUT a kind column (a wide frame) whose
 * n_cols value columns are one array in device memory of logical shape (n_rows, n_cols), row-aligned with the key columns,
 * with any non-negative element strides stride_row / stride_col (row-major, column-major, sliced and expanded views).
 * Replaces n_cols tsfa_pack_set_values calls, each of which re-reads the permutation and, on a row-major matrix, touches
 * n_cols times the bytes it uses.
 *   values, value_type   TSFA_DEVICE pointers only; the element types, conversions and NaN test of tsfa_pack_device
 *   out_packs            n_cols handles; out_packs[c] is a view of column c: elements [c * n_rows, (c + 1) * n_rows) of ONE new
 *                        buffer of n_cols * n_rows output elements, the set's offsets and ids, TSFA_PACK_VALUE_NAN raised per
 *                        column; every tsfa_pack_device_* accessor and tsfa_extract* work on it, ownership as in
 *                        tsfa_pack_set_values
 * Two kernels, chosen from the strides: stride_col == 1 with several columns turns [position x column] tiles through LDS (the
 * tile geometry of tsfa_pack_dense's channels-last route; the permutation is read once per row, the loads of a gathered row
 * and the stores of a column are both unit-stride); anything else is a strided gather with one lane per (column, position).
 * Grid-stride over the tiles, at most 2048 workgroups; no atomic but the OR into a column's flag.  Scratch: 4 bytes per column.
 * Synchronous.  TSFA_ERR_INVALID: a null pointer, a set with a kind column, an unknown element type, n_cols outside
 * [1, 2^31 - 1], a negative stride, an extent beyond 2^59 cells.  Otherwise the errors of tsfa_pack_set_values. */
int tsfa_pack_set_rows(tsfa_pack_set *set, const void *values, int32_t value_type, int64_t n_cols, int64_t stride_row,
                       int64_t stride_col, tsfa_pack **out_packs);
/* Hours packer of a set: the per-sample `times` of tsfa_extract_timed for a frame whose stamps are a row-aligned array in
 * device memory (the frame's DatetimeIndex), written in the set's packed order for ALL kinds at once:
 *     hours_out[p] = hours between stamp t[perm[p] * stride] and the stamp of the first sorted row of p's (kind, id) group
 * for every sorted position p in [0, n_rows); kind k's stretch starts at its first row, where tsfa_pack_set_values' views start.
 *   t, t_type, ticks_per_second   TSFA_I64 ticks or TSFA_F64 seconds, exactly as tsfa_pack_times takes them, with its
 *                        arithmetic (one int64 subtraction, one conversion, two IEEE divisions: pandas >= 2 bit for bit);
 *                        stamps need not ascend
 *   hours_out            n_rows float64 (a device pointer)
 *   flags_out            one int32 the call ORs TSFA_DENSE_BAD_TIME into (the caller clears it): a NaT tick or NaN second; its
 *                        hours are NaN, and so are those of a whole group whose FIRST stamp is missing
 * One kernel over work items of 4096 sorted positions: one bisection of the set's offsets per work item, the offsets of the
 * groups that start inside it staged in LDS, where the lanes bisect; at most 1024 workgroups, grid-stride.  Nothing is
 * allocated.  Synchronous.  This is what a frame with a DatetimeIndex lacks to be packed on the device; the frame entries do
 * not use it yet.
 * TSFA_ERR_INVALID: a null pointer, another type, a ticks_per_second outside the four values, a negative stride. */
int tsfa_pack_set_hours(const tsfa_pack_set *set, const void *t, int32_t t_type, int64_t ticks_per_second, int64_t stride,
                        double *hours_out, int32_t *flags_out);
void tsfa_pack_set_destroy(tsfa_pack_set *set);

/* Dense packer: the ragged layout for a batch that already IS an array in device memory -- (n_batch, n_channels, n_time) with
 * any non-negative element strides: [B, C, n], the channels-last [B, n, C] of a multivariate recording, [B, n] (one channel,
 * stride_channel 0), sliced, stepped and expanded (stride 0) views.  Replaces WideTsFrameAdapter (data.py:181-230: one
 * groupby of the id column per value column) for a container that is already an array: there is nothing to group or to sort,
 * series b of channel c is row (b, c), and the only work is the copy into the layout tsfa_extract* reads, fused with the
 * conversion of the element type.
 *   x, x_type        TSFA_F64 stays float64, TSFA_F32 stays float32, TSFA_F16 and TSFA_BF16 become float32 (both exact:
 *                    subnormals and +-inf keep their value)
 *   lengths          NULL, or n_batch entries of lengths_type (TSFA_I32 | TSFA_I64): series b is its first lengths[b] samples,
 *                    1 <= lengths[b] <= n_time (a right-padded batch)
 *   values_out       channel c occupies elements [c * channel_stride_out, c * channel_stride_out + T) of the output type,
 *                    T = sum of the lengths (n_batch * n_time without lengths), the series back to back in batch order;
 *                    channel_stride_out >= n_batch * n_time
 *   offsets_out      n_batch + 1 int64 shared by every channel: b * n_time without lengths, else the exclusive scan of the
 *                    lengths (one workgroup, 64 bits wide; no workgroup waits on another)
 *   flags_out        one int32 the call ORs into (the caller clears it): TSFA_PACK_VALUE_NAN a sample that was copied is NaN
 *                    (the caller raises the reference's ValueError, data.py:148-167); TSFA_DENSE_BAD_LENGTH a length is
 *                    outside [1, n_time] -- it was clamped into [0, n_time] before use, so whatever `lengths` holds nothing
 *                    outside x is read and nothing outside [0, T) of a channel is written
 * Channel c of the result goes to tsfa_extract* as (values_out + c * channel_stride_out, offsets_out, n_batch, TSFA_DEVICE).
 * Three kernels, chosen from the strides: stride_time == 1 copies rows with consecutive lanes on consecutive samples;
 * stride_channel == 1 with several channels turns [time x channel] tiles through LDS so that both the reads and the writes
 * are unit-stride; anything else is a strided gather.  All pointers are device pointers on `device`; nothing is allocated.
 *   stream           a hipStream_t: the call returns after enqueueing.  NULL: the library's own (the null) stream, and the
 *                    call returns when the work is done.
 * TSFA_ERR_INVALID: a null pointer, a type outside the lists above, a negative stride, a dimension below 1,
 * channel_stride_out below n_batch * n_time, or an extent beyond 2^62 elements.  TSFA_ERR_TOO_LONG: n_time > 33 554 431.
 * TSFA_ERR_NO_DEVICE: no HIP device (there is no CPU route in the library). */
#define TSFA_DENSE_BAD_LENGTH 8
int tsfa_pack_dense(const void *x, int32_t x_type, int64_t n_batch, int64_t n_channels, int64_t n_time, int64_t stride_batch,
                    int64_t stride_channel, int64_t stride_time, const void *lengths, int32_t lengths_type, void *values_out,
                    int64_t channel_stride_out, int64_t *offsets_out, int32_t *flags_out, int32_t device, void *stream);

/* Times packer: the per-sample `times` of tsfa_extract_timed / tsfa_extract_windows (float64 hours since the series' first
 * stamp, what linear_trend_timewise regresses on) for a batch whose clock is an array in device memory, written in the
 * ragged layout tsfa_pack_dense wrote for the samples of the same batch.  Replaces the host's pandas arithmetic on a
 * DatetimeIndex (feature_extraction/data.py: _hours_since_first) for a batch that is an array.
 *   t, t_type        logical (n_batch, n_time) stamps with non-negative element strides; stride_batch 0: one clock shared by
 *                    every series.  TSFA_I64: integer ticks since any epoch, ticks_per_second of them per second (1, 10^3,
 *                    10^6 or 10^9: numpy's datetime64[s|ms|us|ns] viewed as int64).  TSFA_F64: seconds, ticks_per_second is
 *                    ignored.
 *   offsets          the n_batch + 1 int64 tsfa_pack_dense wrote (a device pointer).  A series' length is the difference of
 *                    its offsets (clamped into [0, n_time]); no stamp at or beyond a series' length is read.
 *   hours_out        hours_out[offsets[b] + i], i < len(b); nothing outside [offsets[0], offsets[n_batch]) is written.
 *                      ticks:   (double)(t[b,i] - t[b,0]) / (double)ticks_per_second / 3600.0
 *                      seconds: (t[b,i] - t[b,0]) / 3600.0
 *                    The subtraction is in int64, there is one correctly rounded int64 -> float64 conversion and two IEEE
 *                    divisions, no reciprocal multiply: bit for bit pandas >= 2's
 *                    `(index - index[0]).total_seconds() / 3600.0`, where total_seconds is `asi8 / periods_per_second`
 *                    (pandas 1.x multiplied by 1e-9 and differs in the last bits).  Stamps need not ascend: the hours of an
 *                    earlier stamp are negative.  A tick difference that overflows int64 wraps: stamps further apart than
 *                    2^63 - 1 ticks are the caller's problem, as are infinite seconds.
 *   flags_out        one int32 the call ORs into (the caller clears it; it may be the word tsfa_pack_dense used):
 *                    TSFA_DENSE_BAD_TIME a NaT tick (INT64_MIN) or a NaN second inside a series' length; its hours are NaN,
 *                    and every sample of a series whose FIRST stamp is missing has NaN hours.
 *   stream           as in tsfa_pack_dense.  All pointers are device pointers on `device`; nothing is allocated.
 * One kernel: PD_ROW_CHUNK stamps of one series per work item, consecutive lanes on consecutive stamps, no LDS, no barrier,
 * one atomic OR per wavefront at most.
 * TSFA_ERR_INVALID: a null pointer, another type, a ticks_per_second outside the four values, a negative stride, a
 * dimension below 1 or an extent beyond 2^62 elements.  TSFA_ERR_TOO_LONG: n_time > 33 554 431.  TSFA_ERR_NO_DEVICE: no HIP
 * device. */
#define TSFA_DENSE_BAD_TIME 16
int tsfa_pack_times(const void *t, int32_t t_type, int64_t ticks_per_second, int64_t n_batch, int64_t n_time,
                    int64_t stride_batch, int64_t stride_time, const int64_t *offsets, double *hours_out, int32_t *flags_out,
                    int32_t device, void *stream);

/* Valid-step packer: tsfa_pack_dense for a batch with gaps -- what the wide frame of the same batch holds after `dropna()`.
 * Step t of series b is dropped FOR EVERY CHANNEL when any channel's sample x[b, :, t] is NaN, and, with stamps, when its
 * stamp is NaT (INT64_MIN ticks) or a NaN second; +-inf is a value and stays (dropna keeps it).  Steps at or beyond
 * lengths[b] are never read.  The kept steps of a series keep their order.
 *   x .. lengths_type   as in tsfa_pack_dense (the same element types, strides, conversions and clamping of the lengths)
 *   t, t_type           NULL, or logical (n_batch, n_time) stamps with non-negative element strides t_stride_batch (0: one
 *                       clock shared by every series) and t_stride_time; TSFA_I64 ticks or TSFA_F64 seconds, as
 *                       tsfa_pack_times takes them
 *   values_out          channel c occupies elements [c * channel_stride_out, c * channel_stride_out + T) of the output type,
 *                       T = the kept steps of the batch, the series back to back; channel_stride_out >= n_batch * n_time
 *   offsets_out         n_batch + 1 int64 shared by every channel: the exclusive scan of the kept counts (one workgroup, 64
 *                       bits wide, a carry across its trips; no workgroup waits on another)
 *   steps_out           int32[T <= n_batch * n_time]: steps_out[offsets[b] + k] = the original step index of the k-th kept
 *                       step of series b
 *   stamps_out          NULL without t; else (n_batch, n_time) elements of t's type, right-padded:
 *                       stamps_out[b * n_time + k] = the stamp of the k-th kept step of series b; cells at or beyond a
 *                       series' kept count are not written.  tsfa_pack_times(stamps_out, t_type, ticks_per_second, n_batch,
 *                       n_time, n_time, 1, offsets_out, ...) gives the hours since each series' first KEPT stamp.
 *   scratch             scratch_bytes >= 200 * n_batch * ceil(n_time / 1024) bytes of device memory, aligned to 8 (the kept
 *                       counts, the keep masks and the per-round prefixes of the work items); the caller's, free to reuse
 *                       when the call is done
 *   flags_out           one int32 the call ORs into (the caller clears it): TSFA_DENSE_BAD_LENGTH as in tsfa_pack_dense;
 *                       TSFA_DENSE_EMPTY_SERIES a series has no kept step (offsets_out[b + 1] == offsets_out[b]: the frame
 *                       after dropna() has no row for it; the first such b is the caller's to find in offsets_out).
 *                       TSFA_PACK_VALUE_NAN is never raised: no NaN is copied.
 *   stream              as in tsfa_pack_dense.  All pointers are device pointers on `device`; nothing is allocated.
 * Three launches over work items of 1024 steps of one series: a count pass (a 64-lane ballot per 64 steps is the keep mask,
 * its population count the kept steps), the scan, and a compaction pass (a lane's cell is the work item's base + the kept
 * steps of the work item's earlier rounds + the population count of its mask below the lane) that writes every channel,
 * steps_out and stamps_out.  One route for every layout, the time stride a compile-time 1 when it is 1.  No atomic on a position: the
 * result is deterministic.
 * TSFA_ERR_INVALID: what tsfa_pack_dense refuses, a null steps_out or scratch, stamps of another type or without stamps_out,
 * a negative stamp stride, a scratch that is too small or misaligned.  TSFA_ERR_TOO_LONG: n_time > 33 554 431.
 * TSFA_ERR_NO_DEVICE: no HIP device. */
#define TSFA_DENSE_EMPTY_SERIES 32
int tsfa_pack_dense_valid(const void *x, int32_t x_type, int64_t n_batch, int64_t n_channels, int64_t n_time,
                          int64_t stride_batch, int64_t stride_channel, int64_t stride_time, const void *lengths,
                          int32_t lengths_type, const void *t, int32_t t_type, int64_t t_stride_batch, int64_t t_stride_time,
                          void *values_out, int64_t channel_stride_out, int64_t *offsets_out, int32_t *steps_out,
                          void *stamps_out, void *scratch, int64_t scratch_bytes, int32_t *flags_out, int32_t device,
                          void *stream);

/* Window builder: the rolled (forecasting) layout of one pack, built on the device from the pack's offsets.  Replaces, for a
 * frame packed by tsfa_pack_device / tsfa_pack_set_*, the host's enumeration of n_series x n_shifts window candidates
 * (tsfresh/utilities/dataframe_functions.py:340-358, _roll_out_time_series, for all shifts at once) and the upload of the
 * starts and ends: the windows go from here to tsfa_extract_windows as TSFA_DEVICE pointers next to the pack's value buffer.
 *   pack               a handle of tsfa_pack_device or a view of tsfa_pack_set_values
 *   rolling_direction  != 0; its magnitude is the stride of the timeshifts
 *   max_timeshift      > 0, or 0 for none
 *   min_timeshift      >= 0
 *   steps              the reference's prediction_steps (:546): the longest series of the whole FRAME over all kinds (of one
 *                      entry for a dict container); the caller passes it because another kind may own the longest series
 * The windows are those of the reference, in (series, ascending timeshift) order.  Series of `len` samples, a = |direction|,
 * mts = max_timeshift or steps; no window when mts < min_timeshift; otherwise
 *   direction > 0: every ts with ts = steps (mod a) and min_timeshift + 1 <= ts <= len gives [max(ts - mts - 1, 0), ts)
 *   direction < 0: every frm = k a <= len - min_timeshift - 1 gives [frm, min(frm + mts + 1, len)), ts = frm + 1
 * Three launches: a per-series count (O(1) per series), the packer's exclusive scan, a fill in which window w finds its series
 * by bisection over the scanned counts.  A series has at most `len` windows, so a pack has fewer than 2^32 of them; every
 * index is int64.  The handle owns, in device memory, n_windows int64 each of
 *   starts / ends      indices into the pack's value buffer (offsets[s] + frm, offsets[s] + until)
 *   series             the series index s of the window (row of the pack's ids)
 *   timeshifts         ts
 *   tsfa_windows_n_windows, tsfa_windows_starts / _ends (device pointers, NULL when there is no window)
 *   tsfa_windows_copy_series / _timeshifts / _starts / _ends: copies to host arrays of n_windows int64
 *   tsfa_roll_shift_values  the value of the pack's kept sort column that names each window -- sort[ends - 1] for a positive
 *                      direction, sort[starts] for a negative one -- gathered on the device in the column's own element type;
 *                      n_windows elements are copied to out_host.  `pack` is the pack the windows were built on.
 *                      TSFA_ERR_INVALID for a pack without TSFA_PACK_KEEP_SORT.
 * Synchronous.  TSFA_ERR_NO_DEVICE without a HIP device; TSFA_ERR_INVALID for direction 0, a negative max_timeshift or
 * min_timeshift, or steps below the pack's longest series.  The windows do not keep the pack alive: destroy them first or
 * not, but hand tsfa_extract_windows only live buffers. */
typedef struct tsfa_windows tsfa_windows; /* opaque; owned by the library */
int tsfa_roll_windows(const tsfa_pack *pack, int32_t rolling_direction, int64_t max_timeshift, int64_t min_timeshift,
                      int64_t steps, tsfa_windows **out_windows);
int64_t tsfa_windows_n_windows(const tsfa_windows *windows);
const int64_t *tsfa_windows_starts(const tsfa_windows *windows);
const int64_t *tsfa_windows_ends(const tsfa_windows *windows);
int tsfa_windows_copy_series(const tsfa_windows *windows, int64_t *series_host);
int tsfa_windows_copy_timeshifts(const tsfa_windows *windows, int64_t *timeshifts_host);
int tsfa_windows_copy_starts(const tsfa_windows *windows, int64_t *starts_host);
int tsfa_windows_copy_ends(const tsfa_windows *windows, int64_t *ends_host);
int tsfa_roll_shift_values(const tsfa_windows *windows, const tsfa_pack *pack, void *out_host);
void tsfa_windows_destroy(tsfa_windows *windows);

/* The same windows, in the same order and with the same meaning of every roll argument, for a batch that is no pack: the
 * offsets tsfa_pack_dense wrote (or any n_series + 1 ascending int64 in device memory) in, caller-owned device buffers out.
 * All pointers are device pointers on `device`; nothing is allocated beyond one counter word inside tsfa_roll_count.
 * Two routes, chosen by `scanned`:
 *   scanned != NULL  a ragged batch.  tsfa_roll_count writes every series' window count into scanned[n_series], scans it in
 *                    place (exclusive) and returns the total in *n_windows_host; tsfa_roll_fill finds window w's series by
 *                    bisection over `scanned`.  series_len is ignored.
 *   scanned == NULL  a uniform batch: every series has series_len samples, offsets[s] = offsets[0] + s * series_len (offsets
 *                    may be NULL for offsets[0] = 0).  The count per series is a closed form the host evaluates:
 *                    tsfa_roll_count launches nothing and reads nothing back, tsfa_roll_fill is one launch in which window w
 *                    belongs to series w / c with shift index w % c.  tsfa_roll_fill refuses an n_windows that is not the
 *                    one tsfa_roll_count returns for the same arguments.
 *   starts / ends / series / timeshifts   n_windows int64 each, as the handle of tsfa_roll_windows holds them; cells beyond
 *                    n_windows are not written.  With n_windows == 0 nothing is launched and the pointers may be NULL.
 *   stream           a hipStream_t: tsfa_roll_fill returns after enqueueing; tsfa_roll_count's ragged route enqueues on it and
 *                    then waits for it, because the total is its result.  NULL: the null stream, and both return when the work
 *                    is done.
 * TSFA_ERR_TOO_LONG, before anything is launched: a batch of 2^32 samples or more -- offsets[n_series] - offsets[0] (two words
 * read back) or n_series * series_len; the counts are 32 bits wide, which suffices because no series has more windows than
 * samples.  TSFA_ERR_INVALID: direction 0, a negative max_timeshift or min_timeshift, steps below the longest series
 * (below series_len), a null pointer that is needed.  TSFA_ERR_NO_DEVICE without a HIP device. */
int tsfa_roll_count(const int64_t *offsets, int64_t n_series, int64_t series_len, int32_t rolling_direction,
                    int64_t max_timeshift, int64_t min_timeshift, int64_t steps, uint32_t *scanned, int64_t *n_windows_host,
                    int32_t device, void *stream);
int tsfa_roll_fill(const int64_t *offsets, int64_t n_series, const uint32_t *scanned, int64_t series_len, int64_t n_windows,
                   int32_t rolling_direction, int64_t max_timeshift, int64_t min_timeshift, int64_t steps, int64_t *starts,
                   int64_t *ends, int64_t *series, int64_t *timeshifts, int32_t device, void *stream);

/* Page-locked host memory for the TSFA_HOST form.  tsfa_extract* accepts ANY host pointer; from pageable memory the HIP
 * runtime stages every transfer through its own bounce buffers, from memory obtained here the copy engines read and
 * write it directly, so the chunked copy-in / compute / copy-out pipeline of tsfa_extract runs at PCIe rate.  The
 * Python host allocates the packed sample buffer and the result matrix (the future DataFrame's block) this way.  The
 * reference has no counterpart (its matrix is assembled by data.pivot, data.py:86-121, from Python tuples). */
int tsfa_host_alloc(void **ptr, size_t bytes);
int tsfa_host_free(void *ptr);

/* Device-resident matrices: the chain extract -> impute -> select (tsfresh/convenience/relevant_extraction.py:18,
 * SURVEY.md 8f N3) hands a float64 [n_ids x n_features] matrix from step to step.  tsfa_extract, tsfa_impute and
 * tsfa_relevance_* accept TSFA_DEVICE pointers; with the four entry points below a host in any language keeps that
 * matrix in HBM for the whole chain and fetches only the selected columns (the reference's `X.loc[:, relevant]`,
 * feature_selection/selection.py:181).  tsfa_device_copy: to_device != 0 copies host -> device, else device -> host.
 * tsfa_gather_columns: out_host[r * n_sel + c] = X[r * ld + cols[c]].
 * tsfa_scatter_columns: dst[r * ld_dst + cols[c]] = src[r * n_src + c], dst and src in device memory, cols on the host: the
 * columns of ONE native plan of a settings object that needs several (augmented_dickey_fuller with several autolag values,
 * more than 128 cwt_coefficients columns) land in their places of the caller's matrix without leaving the device. */
int tsfa_device_alloc(void **ptr, size_t bytes, int32_t device);
int tsfa_device_free(void *ptr, int32_t device);
int tsfa_device_copy(void *dst, const void *src, size_t bytes, int32_t to_device, int32_t device);
int tsfa_gather_columns(const double *X, int64_t n_rows, int64_t ld, const int32_t *cols, int64_t n_sel, double *out_host,
                        int32_t device);
int tsfa_scatter_columns(double *dst, int64_t ld_dst, const int32_t *cols, const double *src, int64_t n_rows, int64_t n_src,
                         int32_t device);

/* ---- feature selection: relevance statistics of the extracted matrix ----
 * Replaces the per-feature loop of tsfresh/feature_selection/relevance.py:214-322 (calculate_relevance_table ->
 * _calculate_relevance_table_for_implicit_target) for classification targets: one call yields, for EVERY column of
 * X, what the reference's univariate tests need
 *   significance_tests.py:84  target_binary_feature_real_test  (scipy.stats.mannwhitneyu): the mid-rank sum of the
 *                             rows of each class and the tie term sum(t^3 - t) of the normal approximation,
 *   significance_tests.py:43  target_binary_feature_binary_test (scipy.stats.fisher_exact): for a column with two
 *                             distinct values, the rows of each class that hold the larger one,
 *   relevance.py:396          get_feature_type: the number of distinct values (1 constant, 2 binary, more: real).
 * X: row-major float64 [n_rows x n_cols], leading dimension ld, host or device memory (`space`), no NaNs.
 * y_codes: host int32[n_rows], class codes 0 .. n_classes-1 (<= 256).  Outputs are host arrays:
 * cols[n_cols], rank_sums[n_cols * n_classes], hi_counts[n_cols * n_classes].  Synchronous. */
typedef struct tsfa_relevance_col {
    int64_t n_unique;  /* distinct values of the column */
    double v_lo, v_hi; /* smallest / largest value */
    double tie_term;   /* sum over tie groups of t^3 - t */
} tsfa_relevance_col;
int tsfa_relevance_classes(const double *X, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t space,
                           const int32_t *y_codes, int32_t n_classes, int32_t device, tsfa_relevance_col *cols,
                           double *rank_sums, int64_t *hi_counts);

/* ... plus, for the 'smir' option (significance_tests.py:121, scipy.stats.ks_2samp of the column split by the label),
 * ks_d[n_cols * n_classes]: the Kolmogorov-Smirnov distance of every column for every label against the rest. */
int tsfa_relevance_classes_ks(const double *X, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t space,
                              const int32_t *y_codes, int32_t n_classes, int32_t device, tsfa_relevance_col *cols,
                              double *rank_sums, int64_t *hi_counts, double *ks_d);

/* The same for real-valued targets (relevance.py:303-316):
 *   significance_tests.py:170 target_real_feature_real_test   (scipy.stats.kendalltau, asymptotic): discordant pairs
 *                             and the tie statistics of the column and of the (column, target) pairs,
 *   significance_tests.py:135 target_real_feature_binary_test (scipy.stats.ks_2samp): for a two-valued column the
 *                             Kolmogorov-Smirnov distance of the target split by the column.
 * y_rank: host int32[n_rows], dense ranks of the target (equal targets share a rank); y_perm: host int32[n_rows], the
 * rows in ascending target order; y_end: host uint8[n_rows], 1 where position p of that order ends a tie group.
 * cols: host array [n_cols].  Synchronous. */
typedef struct tsfa_relevance_real_col {
    int64_t n_unique;   /* distinct values of the column */
    double v_lo, v_hi;  /* smallest / largest value */
    int64_t dis;        /* discordant pairs */
    int64_t xtie, ntie; /* tied pairs of the column / of (column, target) */
    double x0, x1;      /* sum t(t-1)(t-2), sum t(t-1)(2t+5) over the column's tie groups */
    int64_t n_hi;       /* two-valued column: rows holding v_hi */
    double ks_d;        /* two-valued column: sup |F_hi - F_lo| of the target */
} tsfa_relevance_real_col;
int tsfa_relevance_real(const double *X, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t space, const int32_t *y_rank,
                        const int32_t *y_perm, const unsigned char *y_end, int32_t device, tsfa_relevance_real_col *cols);
/* Pr(D >= h / lcm(m, n)), two-sided two-sample Kolmogorov-Smirnov, m != n, g = gcd(m, n): the exact lattice-path tail of
 * scipy.stats.ks_2samp(method="exact") -- a scalar function of four integers (host arithmetic, no device needed). */
double tsfa_ks_outer_prob(int64_t m, int64_t n, int64_t g, int64_t h);

/* ---- impute: tsfresh/utilities/dataframe_functions.py:49-214 on the feature matrix ----
 * Per column: the largest / smallest / median FINITE value (get_range_values_per_column :142-180; a column without a
 * finite value counts as zeros); then, in place, +inf -> max, -inf -> min, NaN -> median (impute_dataframe_range
 * :96-139).  X: row-major float64 [n_rows x n_cols], leading dimension ld, host or device memory (`space`).
 * col_max / col_min / col_median / finite_count: optional host arrays [n_cols] receiving the statistics and the number
 * of finite cells per column (0: the reference warns and fills with zeros).  Synchronous. */
int tsfa_impute(double *X, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t space, int32_t device, double *col_max,
                double *col_min, double *col_median, int32_t *finite_count);

/* ---- selection on the device: p-value tails, FDR step-up, mask, gather (csrc/rel_tails.h) ----
 * The chain impute -> relevance table -> selection for a matrix that stays in HBM: the statistics of tsfa_relevance_*
 * are not copied out but turned into p-values where they are, the Benjamini-Hochberg / Benjamini-Yekutieli step-up runs
 * on the p-value array, and the selected columns are gathered into another device matrix.  What comes back to the host is
 * the count of host-route cells, the count of selected columns, and whatever the caller asks for.
 *
 * Every p-value cell has a route: who evaluates its tail (significance_tests.py mannwhitney_pvalue / fisher_exact_pvalue /
 * kendall_pvalue restated in float64; Fisher by one wavefront per cell, the closed forms by one lane per cell).  The two
 * HOST routes are left to the caller: the kernel writes NaN, counts the cell, and the caller overwrites p before
 * tsfa_relevance_fdr -- the exact Mann-Whitney distribution (a class or its complement with <= 8 rows, no ties) and every
 * Kolmogorov-Smirnov tail (with_ks, and two-valued columns under a real target) -- unless the *_ks variants below are asked
 * to serve the exact Kolmogorov-Smirnov tail on the device (TSFA_ROUTE_KS_EXACT). */
enum tsfa_route {
    TSFA_ROUTE_NONE = 0,           /* constant column: p = NaN */
    TSFA_ROUTE_MWU_NORMAL = 1,
    TSFA_ROUTE_FISHER = 2,
    TSFA_ROUTE_KENDALL = 3,
    TSFA_ROUTE_HOST_MWU_EXACT = 4,
    TSFA_ROUTE_HOST_KS = 5,
    TSFA_ROUTE_KS_EXACT = 6        /* a Kolmogorov-Smirnov cell whose exact tail the device served (ks_tail, below) */
};
/* X, y_codes, n_classes as tsfa_relevance_classes; with_ks != 0 additionally runs the sweep of tsfa_relevance_classes_ks and
 * routes every real cell to TSFA_ROUTE_HOST_KS.  Device outputs: p[n_cols * n_classes], route[n_cols * n_classes],
 * type[n_cols] (0 constant, 1 binary, 2 real).  Optional host outputs (NULL: not copied): cols, rank_sums, hi_counts, ks_d
 * (only with with_ks) as tsfa_relevance_classes_ks fills them, and n_host_cells, the number of HOST-route cells.
 * Synchronous, on the null stream. */
int tsfa_relevance_tails_classes(const double *X, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t space,
                                 const int32_t *y_codes, int32_t n_classes, int32_t with_ks, int32_t device, double *p,
                                 unsigned char *route, unsigned char *type, tsfa_relevance_col *cols, double *rank_sums,
                                 int64_t *hi_counts, double *ks_d, int64_t *n_host_cells);
/* The same for a real target (y_rank, y_perm, y_end as tsfa_relevance_real; ytie, y0, y1: the target's tied pairs,
 * sum t(t-1)(t-2) and sum t(t-1)(2t+5) over its tie groups).  Device outputs p[n_cols], route[n_cols], type[n_cols]; optional
 * host outputs cols[n_cols] and n_host_cells. */
int tsfa_relevance_tails_real(const double *X, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t space, const int32_t *y_rank,
                              const int32_t *y_perm, const unsigned char *y_end, int64_t ytie, double y0, double y1,
                              int32_t device, double *p, unsigned char *route, unsigned char *type,
                              tsfa_relevance_real_col *cols, int64_t *n_host_cells);

/* ---- the exact Kolmogorov-Smirnov tail on the device (csrc/rel_ks.h) ----
 * significance_tests.py ks_2samp_pvalue(n1, n2, d) for max(n1, n2) <= 10 000, bit for bit: g = gcd, lcm = (n1 / g) * n2,
 * h = rint(d * lcm); h == 0 gives 1.0; n1 == n2 the Horner form of the closed sum (a lane per cell); n1 != n2 the lattice
 * walk of tsfa_ks_outer_prob by anti-diagonals (a wavefront per cell).  A cell is NOT served, and stays with the caller,
 * when max(n1, n2) > 10 000 (scipy's kstwo.sf), when n1 < 1, n2 < 1 or d is not in [0, 1], and when the exact value is not
 * inside [0, 1] (rounding can leave it an ulp above 1: the Python text then falls through to kstwo, and so must the caller).
 *
 * tsfa_ks_tails: n1[n_cells], n2[n_cells], d[n_cells] and the outputs p[n_cells], route[n_cells] are DEVICE arrays.  A served
 * cell gets its p and TSFA_ROUTE_KS_EXACT, every other cell NaN and TSFA_ROUTE_HOST_KS.  Synchronous, on the null stream. */
int tsfa_ks_tails(const int64_t *n1, const int64_t *n2, const double *d, int64_t n_cells, int32_t device, double *p,
                  unsigned char *route);
enum tsfa_ks_tail {
    TSFA_KS_TAIL_HOST = 0,  /* every Kolmogorov-Smirnov cell is TSFA_ROUTE_HOST_KS: what tsfa_relevance_tails_* do */
    TSFA_KS_TAIL_DEVICE = 1 /* the cells tsfa_ks_tails serves get their p and TSFA_ROUTE_KS_EXACT; the rest stay HOST_KS */
};
/* tsfa_relevance_tails_classes / tsfa_relevance_tails_real with the choice of ks_tail: with TSFA_KS_TAIL_DEVICE the
 * Kolmogorov-Smirnov cells (with_ks: the real columns of every class table; real target: the two-valued columns) are
 * evaluated from the statistics the sweep left in HBM, and n_host_cells counts what is left.  ks_d_device (class tables:
 * [n_cols * n_classes], only with with_ks) and n_hi_device / ks_d_device (real target: [n_cols]) are optional caller-owned
 * DEVICE arrays that receive the statistics of the Kolmogorov-Smirnov cells, so that a caller with a few cells left fetches
 * those triples instead of the host copies (cols, ks_d).  Everything else as the functions above. */
int tsfa_relevance_tails_classes_ks(const double *X, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t space,
                                    const int32_t *y_codes, int32_t n_classes, int32_t with_ks, int32_t ks_tail, int32_t device,
                                    double *p, unsigned char *route, unsigned char *type, tsfa_relevance_col *cols,
                                    double *rank_sums, int64_t *hi_counts, double *ks_d, double *ks_d_device,
                                    int64_t *n_host_cells);
int tsfa_relevance_tails_real_ks(const double *X, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t space, const int32_t *y_rank,
                                 const int32_t *y_perm, const unsigned char *y_end, int64_t ytie, double y0, double y1,
                                 int32_t ks_tail, int32_t device, double *p, unsigned char *route, unsigned char *type,
                                 tsfa_relevance_real_col *cols, int64_t *n_hi_device, double *ks_d_device,
                                 int64_t *n_host_cells);
/* statsmodels' multipletests "fdr_bh" / "fdr_by" per table and relevance.py's combination of the tables.  All pointers are
 * device pointers.  p[n_cols * n_tables] (n_tables <= 256: the classes, or 1), type[n_cols].  Per table the columns whose type
 * is not 0 are tested (m of them); their p-values are sorted (NaN last, never rejected) and everything up to the largest
 * sorted position k with  p_(k) <= ((k / (double)m) / c_m) * alpha  is rejected.  c_m: 1.0 for Benjamini-Hochberg,
 * sum_{i=1..m} 1/i (as the caller's arithmetic adds it) for Benjamini-Yekutieli.
 * Outputs: relevant_per_table[n_cols * n_tables], n_significant_out[n_cols] (tables that reject the column), p_min[n_cols]
 * (smallest p-value over the tables, NaN when there is none), relevant[n_cols]: n_significant_out >= n_significant with
 * multiclass != 0, n_significant_out > 0 otherwise.  Synchronous. */
int tsfa_relevance_fdr(const double *p, const unsigned char *type, int64_t n_cols, int32_t n_tables, double alpha, double c_m,
                       int32_t n_significant, int32_t multiclass, int32_t device, unsigned char *relevant_per_table,
                       unsigned char *relevant, int32_t *n_significant_out, double *p_min);
/* indices[0 .. *count) = the positions of the non-zero bytes of mask[n], ascending (mask and indices: device memory,
 * indices has room for n entries and is written only up to *count; count: host). */
int tsfa_compact_mask(const unsigned char *mask, int64_t n, int32_t *indices, int64_t *count, int32_t device);
/* tsfa_gather_columns within HBM: out[r * ld_out + c] = X[r * ld + cols[c]], cols in device memory. */
int tsfa_gather_columns_device(const double *X, int64_t n_rows, int64_t ld, const int32_t *cols, int64_t n_sel, double *out,
                               int64_t ld_out, int32_t device);

#ifdef __cplusplus
}
#endif
#endif /* TSFRESH_AMD_H */
