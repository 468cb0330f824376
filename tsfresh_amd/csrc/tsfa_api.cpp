// C-ABI of libtsfresh_amd.so (see include/tsfresh_amd.h).  Host code: plan compilation, HBM staging, launches.
// There is deliberately no CPU compute path here: without a HIP device every entry point that would compute
// returns TSFA_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../include/tsfresh_amd.h"
#include "tsfa_devmem.h"
#include "tsfa_host_tables.h"
#include "tsfa_launch.h"
#include "fam_seq.h"
#include "tsfa_layout.h"

static thread_local std::string g_last_error;

static int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

// for the other translation units of the library and the macros of tsfa_devmem.h
int tsfa_fail(int code, const char *msg) { return fail(code, std::string(msg ? msg : "")); }

#define TSFA_MAX_CHUNKS 16
// The side lane's families (PlanOptions::side_lane).  BASIC, SORT and ENTROPY never go there: they carry the shared
// per-series statistics and the shared sample order.
// The default is what profiles/r09_two_lanes.md measured best at 100 000 x 1024: k_seq, then k_trend, starting behind
// k_entropy_bits -- beside k_ar and k_sort, which leave issue slots idle; k_entropy_bits itself (VALU busy 0.90) leaves few,
// and neither k_perm on the side lane nor a side stream of the main lane's priority measured a gain.
#define TSFA_SIDE_ALL ((1u << TSFA_N_FAMILIES) - 1u)
#define TSFA_SIDE_ALLOWED (TSFA_SIDE_ALL & ~((1u << TSFA_FAM_BASIC) | (1u << TSFA_FAM_SORT) | (1u << TSFA_FAM_ENTROPY)))
#define TSFA_SIDE_DEFAULT ((1u << TSFA_FAM_SEQ) | (1u << TSFA_FAM_TREND))

struct Timing {
    std::string name;
    hipEvent_t e0 = nullptr, e1 = nullptr;   // owned: a slot that plan->timings.resize() trims destroys its events
    float ms = 0.f;
    Timing() = default;
    // move construction is all std::vector::resize needs; there is no copy and no assignment on purpose, so that code
    // which would duplicate or overwrite the handles does not compile
    Timing(Timing &&o) noexcept : name(std::move(o.name)), e0(o.e0), e1(o.e1), ms(o.ms) { o.e0 = o.e1 = nullptr; }
    ~Timing() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

// Launch options of a plan (tsfa_plan_set_option): each names an alternative ROUTE to the same numbers -- every one has a test
// that compares both ways -- or a diagnostic pre-fill.  They are set through the C-ABI by the caller who owns the plan; the
// library reads NO environment variable (round-5 VERDICT: 25 getenv calls on the launch path).  Result-changing diagnostics
// (leaving a family's launch out, per-family workgroup sizes, the stderr traces) exist only in the lab build (make lab:
// -DTSFA_LAB, libtsfresh_amd_lab.so, never loaded by the package).
struct PlanOptions {
    bool length_classes = true;   // launch a batch whose lengths span more than 2x class by class
    bool stats_share = true;      // k_basic's per-series statistics record serves the ENTROPY / AR / SEQ / SORT families
    int sort_waves = 1;           // SORT, groups up to 2048 samples: 1 = one wavefront per series; 2 = the two-wavefront form it replaced
    bool select = true;           // median / quantile-only plans: order statistics by selection (k_order_stats)
    bool bluestein = true;        // chirp-z transform for long non-power-of-two spectra
    bool force_long = false;      // the HBM-scratch build of every family kernel whatever the length
    int entropy_route = 0;        // 0: bit-matrix sweep where it applies; 1: the windowed pair sweep; 2: the general kernel
    int bluestein_min = 0;        // crossover Goertzel -> chirp-z in samples (0: the measured defaults)
    int gscratch_slots = 0;       // cap of the chirp-z scratch slots (0: none; tests force several launches per group)
    int host_chunks = 0;          // row chunks of the host pipeline (0: by batch size)
    int nt[TSFA_N_FAMILIES] = {0};  // lab build: workgroup size per family (0: the measured defaults)
    bool trace = false;           // lab build: launch decisions to stderr
    bool row_form = true;         // BASIC / TREND: series of <= 256 samples four to a wavefront (k_basic_rows / k_trend_rows)
    int seq_rows = -1;            // lempel_ziv symbol rows: 0 in LDS, 1 in HBM, -1: in HBM where that puts more series on a CU
    unsigned side_lane = TSFA_SIDE_DEFAULT;   // two lanes (tsfa_plan::side): bit f = family f on the side lane; 0: one lane
    int cwt_links = 1;            // number_cwt_peaks, widths <= 5: 1 = ridge lines linked column by column; 0 = the general linker it replaced there
    int fail_after = -1;          // test hook: run_batch returns an error after this family's launches (its exits after the fork)
};

#if defined(TSFA_LAB)
#define TSFA_LAB_ONLY(x) (x)
#else
#define TSFA_LAB_ONLY(x) (0)
#endif

static int64_t g_relevance_batch = 0;   // tsfa_plan_set_option(NULL, "relevance_batch", n): columns per sort batch (tests)
int64_t tsfa_relevance_batch_override() { return g_relevance_batch; }

struct tsfa_plan {
    int device = 0;
    PlanOptions opt;
    hipStream_t stream = nullptr;
    int n_cols = 0;
    std::vector<TsfaSpec> fam_specs[TSFA_N_FAMILIES];  // CWT slot: number_cwt_peaks specs only
    // Device memory is held by owners (tsfa_devmem.h) that go with the plan; the streams and events below are released by
    // ~tsfa_plan, which also makes `device` current before any member is freed.
    DevPtr<TsfaSpec> d_specs[TSFA_N_FAMILIES];
    TsfaFamHints hints[TSFA_N_FAMILIES];
    TsfaCwtBank bank;  // cwt_coefficients
    DevPtr<double> d_W;
    DevPtr<int> d_cols, d_coeff;
    DevPtr<double> d_dectab, d_twc, d_tws, d_consts;
    DevPtr<long long> d_stats;
    // (long_scratch: the HBM slots of every long-series family, k_mprofile's among them)
    DevBuf values, offsets, out, gscratch, times, deg_list, sel, long_scratch, pf_buf, perm_buf, stats_buf, dd_scratch, gen_scratch, seq_rows;
    // k_general (fam_general.h): the columns of the calculators whose parameters lie beyond the tuned kernels' tables
    std::vector<TsfaSpec> gen_specs;
    DevPtr<TsfaSpec> d_gen_specs;
    TsfaGenPlan gen_plan;
    DevPtr<double> d_pool;                      // array-valued parameters (tsfa_plan_create_with_data): query_similarity_count's queries
    DevPtr<int> d_deg_count;
    DevPtr<int> d_cursor;                       // per-launch-group fill cursors (k_class_fill)
    hipStream_t s_in = nullptr, s_out = nullptr;  // copy-in / copy-out streams of the host pipeline
    hipEvent_t ev_in[TSFA_MAX_CHUNKS] = {nullptr}, ev_k[TSFA_MAX_CHUNKS] = {nullptr};
    std::vector<int64_t> h_rel;                 // offsets relative to the staged span
    bool needs_times = false;  // the plan holds linear_trend_timewise columns
    bool sort_only_order_stats = false;  // the SORT family holds only median / quantile columns
    bool stream_ok = false;              // BASIC + SORT are served by the fused streaming kernel (k_stream)
    bool profiling = false;
    std::vector<Timing> timings;
    std::vector<tsfa_launch_info> launches;     // tsfa_plan_last_launches: one record per (family, launch group) of the last extract
    long long hint_min_len = 0, hint_max_len = 0;  // tsfa_plan_set_length_hint: skip the length scan (and its host sync)
    // Every family kernel writes every one of its columns for every series (NaN where the reference yields NaN): audited
    // with a sentinel pre-fill over lengths 1 .. 8192, three parameter sets, both sample types, constant / non-finite
    // series (profiles/fill_audit.py, tests/test_gpu_parity.py::test_every_cell_is_written_by_a_kernel), so the matrix is
    // NOT pre-filled (round 3 rewrote all of it, 0.63 GB per 100 000 x 783, for nothing).  Option "fill" restores the
    // pre-fill of every column, with NaN or an audit's sentinel (profiles/fill_audit.py).
    bool fill_all = false;
    double fill_value = __builtin_nan("");
    int debug_skip_fam = -1;             // lab build, option "skip_family": the audit's positive control
    // Two lanes (option "side_lane": a family bit mask, 0 = one lane): the named families run on a second stream beside the
    // others, at the device's LOWEST priority -- the dispatcher gives the main lane's workgroups every slot they can use and
    // the side lane's the LDS / register / wavefront slots they leave (k_entropy_bits holds 122 of 160 KB of LDS and 448 of
    // 512 VGPRs per SIMD: two k_seq workgroups fit beside it) -- so a latency-bound kernel fills issue slots an issue-bound one
    // leaves idle.  The lane forks behind the main lane's k_entropy (run_batch: lane_order) and joins before run_batch
    // returns, on every exit path.  The stream and its events are made at the first batch that uses them (side_ready).
    hipStream_t side = nullptr;
    hipEvent_t ev_side_fork = nullptr, ev_side_join = nullptr, ev_side_long = nullptr;

    // the body runs before the members' destructors: everything the plan owns is freed on its own device
    ~tsfa_plan() {
        // `stream` is the first thing a create makes: without it nothing else exists, and a create that was refused on its
        // arguments leaves the caller's current device alone
        if (!stream) return;
        (void)hipSetDevice(device);
        auto drop_event = [](hipEvent_t e) { if (e) (void)hipEventDestroy(e); };
        auto drop_stream = [](hipStream_t s) { if (s) (void)hipStreamDestroy(s); };
        for (hipEvent_t e : ev_in) drop_event(e);
        for (hipEvent_t e : ev_k) drop_event(e);
        for (hipEvent_t e : {ev_side_fork, ev_side_join, ev_side_long}) drop_event(e);
        for (hipStream_t s : {s_in, s_out, side, stream}) drop_stream(s);
    }
};

static const char *fam_names[TSFA_N_FAMILIES] = {"k_basic", "k_sort", "k_spectral", "k_ar", "k_entropy", "k_cwtpeaks", "k_seq", "k_trend", "k_mprofile"};

template <class T>
static int upload(const std::vector<T> &h, DevPtr<T> &d) {
    d.reset();
    if (h.empty()) return 0;
    if (d.alloc(h.size() * sizeof(T)) != hipSuccess) return -1;
    if (hipMemcpy(d.get(), h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return -1;
    return 0;
}

static int record(tsfa_plan *plan, hipStream_t st, size_t slot, const char *name, bool begin) {
    if (!plan->profiling) return 0;
    if (plan->timings.size() <= slot) plan->timings.resize(slot + 1);
    Timing &t = plan->timings[slot];
    if (!t.e0) {
        if (hipEventCreate(&t.e0) != hipSuccess || hipEventCreate(&t.e1) != hipSuccess) return -1;
    }
    t.name = name;
    return hipEventRecord(begin ? t.e0 : t.e1, st) == hipSuccess ? 0 : -1;
}

extern "C" {

int tsfa_version(void) { return TSFA_VERSION; }

int tsfa_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *tsfa_last_error(void) { return g_last_error.c_str(); }

int tsfa_calc_id(const char *name) {
    if (!name) return -1;
    for (int i = 0; i < TSFA_N_CALCS; ++i)
        if (strcmp(tsfa_calc_table[i].name, name) == 0) return i;
    return -1;
}
const char *tsfa_calc_name(int calc) { return (calc >= 0 && calc < TSFA_N_CALCS) ? tsfa_calc_table[calc].name : nullptr; }
int tsfa_calc_count(void) { return TSFA_N_CALCS; }

void tsfa_plan_destroy(tsfa_plan *plan) {
    if (plan) delete plan;   // ~tsfa_plan and the members' owners release everything
}

int tsfa_plan_create(const tsfa_feature_spec *specs, int32_t n_specs, int32_t device, tsfa_plan **out_plan) {
    return tsfa_plan_create_with_data(specs, n_specs, nullptr, 0, device, out_plan);
}

int tsfa_plan_create_with_data(const tsfa_feature_spec *specs, int32_t n_specs, const double *data, int64_t n_data, int32_t device,
                               tsfa_plan **out_plan) {
    if (!out_plan) return fail(TSFA_ERR_INVALID, "out_plan is NULL");
    *out_plan = nullptr;
    if (n_specs < 0 || (n_specs > 0 && !specs)) return fail(TSFA_ERR_INVALID, "bad specs");
    if (n_data < 0 || (n_data > 0 && !data)) return fail(TSFA_ERR_INVALID, "bad data pool");
    const int ndev = tsfa_device_count();
    if (ndev <= 0) return fail(TSFA_ERR_NO_DEVICE, "no HIP device visible: tsfresh_amd has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(TSFA_ERR_INVALID, "device ordinal out of range");

    std::unique_ptr<tsfa_plan> plan(new tsfa_plan());   // goes with any early return below
    plan->device = device;
    plan->n_cols = n_specs;
    std::vector<TsfaSpec> cwt_coef;
    bool general[TSFA_N_CALCS];
    tsfa_general_calcs(specs, n_specs, general);
    for (int i = 0; i < n_specs; ++i) {
        TsfaSpec s;
        s.calc = specs[i].calc;
        s.col = i;
        for (int k = 0; k < 4; ++k) s.p[k] = specs[i].p[k];
        if (s.calc < 0 || s.calc >= TSFA_N_CALCS)
            return fail(TSFA_ERR_UNSUPPORTED, "spec " + std::to_string(i) + ": unknown calculator id " + std::to_string(s.calc));
        const std::string why = tsfa_validate_spec(s);
        if (!why.empty())
            return fail(TSFA_ERR_UNSUPPORTED, std::string("spec ") + std::to_string(i) + " (" + tsfa_calc_table[s.calc].name + "): " + why);
        if (s.calc == TSFA_C_QUERY_SIMILARITY_COUNT && s.p[3] > 0 && !(s.p[2] + s.p[3] <= (double)n_data))
            return fail(TSFA_ERR_INVALID, "spec " + std::to_string(i) + " (query_similarity_count): the query lies outside the data pool");
        if (s.calc == TSFA_C_LINEAR_TREND_TIMEWISE) plan->needs_times = true;
        if (s.calc == TSFA_C_CWT_COEFFICIENTS) cwt_coef.push_back(s);
        else if (general[s.calc]) plan->gen_specs.push_back(s);
        else plan->fam_specs[tsfa_calc_table[s.calc].family].push_back(s);
    }
    plan->gen_plan = tsfa_prepare_general(plan->gen_specs);
    if (cwt_coef.size() > 128) return fail(TSFA_ERR_UNSUPPORTED, "more than 128 cwt_coefficients columns in one plan");
    {
        std::vector<TsfaSpec> all;
        for (int f = 0; f < TSFA_N_FAMILIES; ++f) all.insert(all.end(), plan->fam_specs[f].begin(), plan->fam_specs[f].end());
        const std::string why = tsfa_validate_plan(all.data(), (int)all.size());
        if (!why.empty()) return fail(TSFA_ERR_UNSUPPORTED, why);
    }
    if (!cwt_coef.empty()) {
        const std::string why = plan->bank.build(cwt_coef);
        if (!why.empty()) return fail(TSFA_ERR_UNSUPPORTED, why);
    }
    if (hipSetDevice(device) != hipSuccess) return fail(TSFA_ERR_HIP, "hipSetDevice failed");
    for (int f = 0; f < TSFA_N_FAMILIES; ++f) tsfa_prepare_family(f, plan->fam_specs[f], plan->hints[f]);
    plan->sort_only_order_stats = !plan->fam_specs[TSFA_FAM_SORT].empty();
    for (const auto &sp : plan->fam_specs[TSFA_FAM_SORT])
        if (sp.calc != TSFA_C_MEDIAN && sp.calc != TSFA_C_QUANTILE) plan->sort_only_order_stats = false;
    // streaming plans (MinimalFCParameters): BASIC float closed forms + median only -> one kernel, one read
    plan->stream_ok = !plan->fam_specs[TSFA_FAM_BASIC].empty() && plan->hints[TSFA_FAM_BASIC].c == 0;
    for (const auto &sp : plan->fam_specs[TSFA_FAM_BASIC])
        if (!tsfa_stream_calc_ok(sp.calc) || sp.calc == TSFA_C_MEDIAN) plan->stream_ok = false;
    for (const auto &sp : plan->fam_specs[TSFA_FAM_SORT])
        if (sp.calc != TSFA_C_MEDIAN) plan->stream_ok = false;
    bool ok = hipStreamCreateWithFlags(&plan->stream, hipStreamNonBlocking) == hipSuccess;
    for (int f = 0; ok && f < TSFA_N_FAMILIES; ++f) ok = upload(plan->fam_specs[f], plan->d_specs[f]) == 0;
    if (ok) ok = upload(plan->gen_specs, plan->d_gen_specs) == 0;
    if (ok && n_data > 0) ok = upload(std::vector<double>(data, data + n_data), plan->d_pool) == 0;
    if (ok && !cwt_coef.empty()) {
        ok = upload(plan->bank.W, plan->d_W) == 0 && upload(plan->bank.cols, plan->d_cols) == 0 &&
             upload(plan->bank.coeff_idx, plan->d_coeff) == 0;
    }
    if (ok) {
        std::vector<double> dt, twc, tws;
        tsfa_build_dectab(dt);
        tsfa_build_twiddles(twc, tws);
        ok = upload(dt, plan->d_dectab) == 0 && upload(twc, plan->d_twc) == 0 && upload(tws, plan->d_tws) == 0;
        std::vector<double> consts;
        tsfa_build_consts(consts);
        ok = ok && upload(consts, plan->d_consts) == 0;
    }
    if (ok) ok = plan->d_stats.alloc(TSFA_LEN_STATS * sizeof(long long)) == hipSuccess;
    if (ok) ok = plan->d_deg_count.alloc(2 * sizeof(int)) == hipSuccess;   // [k_ar_degenerate, k_langevin_dd]
    if (ok) ok = plan->d_cursor.alloc(TSFA_N_LEN_CLASSES * sizeof(int)) == hipSuccess;
    if (ok) ok = hipStreamCreateWithFlags(&plan->s_in, hipStreamNonBlocking) == hipSuccess &&
                 hipStreamCreateWithFlags(&plan->s_out, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; ok && i < TSFA_MAX_CHUNKS; ++i)
        ok = hipEventCreateWithFlags(&plan->ev_in[i], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&plan->ev_k[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) return fail(TSFA_ERR_HIP, "device allocation/upload failed while creating the plan");
    *out_plan = plan.release();
    return TSFA_OK;
}

int32_t tsfa_plan_n_cols(const tsfa_plan *plan) { return plan ? plan->n_cols : -1; }

int tsfa_plan_set_length_hint(tsfa_plan *plan, int64_t min_len, int64_t max_len) {
    if (!plan) return fail(TSFA_ERR_INVALID, "null plan");
    if (max_len == 0 && min_len == 0) { plan->hint_min_len = plan->hint_max_len = 0; return TSFA_OK; }
    if (min_len < 1 || max_len < min_len || max_len > 2147483647LL / 64) return fail(TSFA_ERR_INVALID, "length hint must satisfy 1 <= min <= max <= 33554431");
    plan->hint_min_len = min_len;
    plan->hint_max_len = max_len;
    return TSFA_OK;
}

int tsfa_plan_set_option(tsfa_plan *plan, const char *name, double value) {
    if (!name) return fail(TSFA_ERR_INVALID, "option name is NULL");
    const std::string n(name);
    const bool on = value != 0.0;
    if (n == "side_lane") {   // (the mask is checked before the plan is looked at: the parser is testable without a device)
        static const char *nm[TSFA_N_FAMILIES] = {"BASIC", "SORT", "SPECTRAL", "AR", "ENTROPY", "CWT", "SEQ", "TREND", "MPROFILE"};
        if (!(value >= 0.0 && value <= (double)TSFA_SIDE_ALL && value == (double)(unsigned)value))
            return fail(TSFA_ERR_INVALID, "side_lane: 0 (one lane) or a bit mask of families");
        for (int f = 0; f < TSFA_N_FAMILIES; ++f)
            if ((((unsigned)value & ~TSFA_SIDE_ALLOWED) >> f) & 1u)
                return fail(TSFA_ERR_INVALID, std::string("side_lane: ") + nm[f] + " stays on the main lane (BASIC, SORT and ENTROPY carry "
                                              "the shared statistics and the shared sample order)");
    }
    if (!plan) {   // library-wide
        if (n == "relevance_batch") { g_relevance_batch = value > 0.0 ? (int64_t)value : 0; return TSFA_OK; }
        return fail(TSFA_ERR_INVALID, "unknown library option '" + n + "'");
    }
    PlanOptions &o = plan->opt;
    if (n == "length_classes") o.length_classes = on;
    else if (n == "stats_share") o.stats_share = on;
    else if (n == "select") o.select = on;
    else if (n == "bluestein") o.bluestein = on;
    else if (n == "force_long") o.force_long = on;
    else if (n == "row_form") o.row_form = on;
    else if (n == "seq_rows") o.seq_rows = (value < 0.0) ? -1 : (on ? 1 : 0);
    else if (n == "entropy_route") { if (value != 0.0 && value != 1.0 && value != 2.0) return fail(TSFA_ERR_INVALID, "entropy_route: 0, 1 or 2"); o.entropy_route = (int)value; }
    else if (n == "sort_waves") { if (value != 1.0 && value != 2.0) return fail(TSFA_ERR_INVALID, "sort_waves: 1 or 2"); o.sort_waves = (int)value; }
    else if (n == "cwt_links") { if (value != 0.0 && value != 1.0) return fail(TSFA_ERR_INVALID, "cwt_links: 0 or 1"); o.cwt_links = (int)value; }
    else if (n == "bluestein_min") o.bluestein_min = value > 0.0 ? (int)std::min(value, 32767.0) : 0;
    else if (n == "gscratch_slots") o.gscratch_slots = value > 0.0 ? (int)std::min(value, 2147483647.0) : 0;
    else if (n == "host_chunks") o.host_chunks = value > 0.0 ? (int)std::min(value, (double)TSFA_MAX_CHUNKS) : 0;
    else if (n == "fused_minimal") { if (!on) plan->stream_ok = false; }   // (cannot be switched back on: decided when the plan is built)
    else if (n == "perm_fused") { if (!on) plan->hints[TSFA_FAM_SORT].d = 0; }   // permutation_entropy stays in k_sort
    else if (n == "fill") { plan->fill_value = value; plan->fill_all = true; }   // pre-fill the matrix (NaN, or an audit's sentinel)
    else if (n == "side_lane") o.side_lane = (unsigned)value;   // (checked above)
    else if (n == "fail_after") o.fail_after = (value >= 0.0 && value < (double)TSFA_N_FAMILIES) ? (int)value : -1;
#if defined(TSFA_LAB)
    else if (n == "skip_family") plan->debug_skip_fam = (int)value;
    else if (n == "trace") o.trace = on;
    else if (n.rfind("nt_", 0) == 0 && n.size() == 4 && n[3] >= '0' && n[3] < '0' + TSFA_N_FAMILIES) o.nt[n[3] - '0'] = (int)value;
#endif
    else return fail(TSFA_ERR_INVALID, "unknown plan option '" + n + "'");
    return TSFA_OK;
}

int tsfa_plan_set_profiling(tsfa_plan *plan, int32_t enable) {
    if (!plan) return fail(TSFA_ERR_INVALID, "plan is NULL");
    plan->profiling = enable != 0;
    return TSFA_OK;
}

int32_t tsfa_plan_last_timings(const tsfa_plan *plan, const char **names, float *ms, int32_t cap) {
    if (!plan) return 0;
    int32_t n = 0;
    for (const auto &t : plan->timings) {
        if (n >= cap) break;
        if (names) names[n] = t.name.c_str();
        if (ms) ms[n] = t.ms;
        ++n;
    }
    return n;
}

int32_t tsfa_plan_last_launches(const tsfa_plan *plan, tsfa_launch_info *out, int32_t cap) {
    if (!plan) return 0;
    const int32_t n = (int32_t)plan->launches.size();
    for (int32_t i = 0; out && i < n && i < cap; ++i) out[i] = plan->launches[(size_t)i];
    return n;
}

int tsfa_extract(tsfa_plan *plan, const void *values, int32_t dtype, const int64_t *offsets, int64_t n_series,
                 double *out, int64_t ld_out, int32_t space, void *stream) {
    return tsfa_extract_timed(plan, values, dtype, nullptr, offsets, n_series, out, ld_out, space, stream);
}

int tsfa_extract_timed(tsfa_plan *plan, const void *values, int32_t dtype, const double *times, const int64_t *offsets,
                       int64_t n_series, double *out, int64_t ld_out, int32_t space, void *stream) {
    // a ragged batch is the special case ends = starts + 1 of the window form
    return tsfa_extract_windows(plan, values, dtype, times, offsets, offsets ? offsets + 1 : nullptr, n_series, out,
                                ld_out, space, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// One batch = fill + the family kernels of the plan over [n_series] views, enqueued on `st` (no host sync).
// ---------------------------------------------------------------------------------------------------------------
struct BatchShape {
    long long max_len = 0, min_len = 0, max_np2 = 0;
    int n_groups = 1;                        // launch groups; 1 = every series in one launch, no index lists
    int g_maxn[TSFA_N_LEN_CLASSES] = {0};
    long long g_np2[TSFA_N_LEN_CLASSES] = {0};
    int64_t g_count[TSFA_N_LEN_CLASSES] = {0};
    bool g_has_short[TSFA_N_LEN_CLASSES] = {false};   // the group holds series of <= TSFA_ROW_MAXN samples (the row form's)
    TsfaClassMap map;
};

// stats: the TSFA_LEN_STATS numbers of k_len_stats (or their host-side twin).  Length classes with fewer than
// `min_group` series ride with the next longer class; a batch whose lengths span less than a factor of two (or that is
// small) is one group.
static void shape_from_stats(const long long *st, int64_t n_series, BatchShape &sh, bool length_classes) {
    sh.max_len = st[0];
    sh.min_len = st[1];
    sh.max_np2 = st[2];
    memset(&sh.map, 0, sizeof sh.map);
    sh.n_groups = 1;
    sh.g_maxn[0] = (int)st[0];
    sh.g_np2[0] = st[2];
    sh.g_count[0] = n_series;
    sh.g_has_short[0] = st[1] <= TSFA_ROW_MAXN;
    if (!length_classes || n_series < 2048 || st[0] <= 2 * st[1] || st[0] <= 128) return;
    const int64_t min_group = 512;
    int ng = 0;
    int64_t pend_count = 0;
    long long pend_np2 = 0;
    int first_of_group = 0;
    for (int c = 0; c < TSFA_N_LEN_CLASSES; ++c) {
        const int64_t cnt = st[3 + c];
        pend_count += cnt;
        pend_np2 = std::max(pend_np2, st[3 + 2 * TSFA_N_LEN_CLASSES + c]);
        bool last = true;
        for (int d = c + 1; d < TSFA_N_LEN_CLASSES; ++d)
            if (st[3 + d] > 0) last = false;
        if (cnt > 0 && (pend_count >= min_group || last)) {
            sh.g_maxn[ng] = (int)st[3 + TSFA_N_LEN_CLASSES + c];
            sh.g_np2[ng] = pend_np2;
            sh.g_count[ng] = pend_count;
            sh.g_has_short[ng] = false;
            for (int d = first_of_group; d <= c; ++d) {   // classes 0 .. 2 end at 64, 128, 256 samples
                sh.map.group_of[d] = ng;
                if ((64LL << d) <= TSFA_ROW_MAXN && st[3 + d] > 0) sh.g_has_short[ng] = true;
            }
            first_of_group = c + 1;
            pend_count = 0;
            pend_np2 = 0;
            ++ng;
        }
        if (last) {
            for (int d = first_of_group; d < TSFA_N_LEN_CLASSES; ++d) sh.map.group_of[d] = ng > 0 ? ng - 1 : 0;
            break;
        }
    }
    sh.n_groups = std::max(ng, 1);
    int b = 0;
    for (int g = 0; g < sh.n_groups; ++g) {
        sh.map.base[g] = b;
        b += (int)sh.g_count[g];
    }
}

// host-side twin of k_len_stats
static int host_len_stats(const int64_t *starts, const int64_t *ends, int64_t n, long long *st) {
    for (int i = 0; i < TSFA_LEN_STATS; ++i) st[i] = 0;
    st[1] = (1LL << 62);
    for (int64_t s = 0; s < n; ++s) {
        const long long l = ends[s] - starts[s];
        if (l < 0) return -1;
        const bool np2 = l > 0 && (l & (l - 1)) != 0;
        const int c = tsfa_len_class(l);
        st[0] = std::max(st[0], l);
        st[1] = std::min(st[1], l);
        if (np2) st[2] = std::max(st[2], l);
        st[3 + c] += 1;
        st[3 + TSFA_N_LEN_CLASSES + c] = std::max(st[3 + TSFA_N_LEN_CLASSES + c], l);
        if (np2) st[3 + 2 * TSFA_N_LEN_CLASSES + c] = std::max(st[3 + 2 * TSFA_N_LEN_CLASSES + c], l);
    }
    return 0;
}

// Row chunks of the TSFA_HOST pipeline: >= 4096 series each (a launch should fill the 256 CUs several times over), at most
// TSFA_MAX_CHUNKS; chunk c is rows [n_series * c / n_chunks, n_series * (c + 1) / n_chunks).  tsfa_extract_chunks hands the
// same cuts to callers that launch a batch chunk by chunk with TSFA_DEVICE pointers.
static int host_chunk_count(const tsfa_plan *plan, int64_t n_series) {
    int n_chunks = (int)std::min<int64_t>(TSFA_MAX_CHUNKS, std::max<int64_t>(1, n_series / 4096));
    if (plan->opt.host_chunks >= 1) n_chunks = std::min(plan->opt.host_chunks, TSFA_MAX_CHUNKS);
    if (plan->profiling) n_chunks = 1;
    return (int)std::max<int64_t>(1, std::min<int64_t>(n_chunks, n_series));
}

int tsfa_extract_chunks(const tsfa_plan *plan, int64_t n_series, int64_t *cuts, int32_t cap) {
    if (!plan || !cuts || n_series < 0) return fail(TSFA_ERR_INVALID, "tsfa_extract_chunks: bad arguments");
    const int n_chunks = n_series ? host_chunk_count(plan, n_series) : 0;
    if (cap < n_chunks + 1) return fail(TSFA_ERR_INVALID, "tsfa_extract_chunks: cuts holds fewer than n_chunks + 1 entries");
    for (int c = 0; c <= n_chunks; ++c) cuts[c] = n_chunks ? n_series * c / n_chunks : 0;
    return n_chunks;
}

// The side lane's stream, at the device's lowest priority, and its events, made when the first batch needs them (the
// options are set after the plan is built)
static int side_ready(tsfa_plan *plan) {
    if (plan->side) return TSFA_OK;
    int least = 0, greatest = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIP_TRY(hipStreamCreateWithPriority(&plan->side, hipStreamNonBlocking, least));
    for (hipEvent_t *e : {&plan->ev_side_fork, &plan->ev_side_join, &plan->ev_side_long})
        if (!*e) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return TSFA_OK;
}

// Joins the side lane into the main one when run_batch leaves, by whichever return: the next batch of the plan (k_basic
// writes the statistics record the side lane's kernels read) and the caller's copy-out both follow the main stream.
struct SideJoin {
    tsfa_plan *plan;
    hipStream_t st;
    bool used = false;
    int join() {
        if (!used) return TSFA_OK;
        used = false;
        HIP_TRY(hipEventRecord(plan->ev_side_join, plan->side));
        HIP_TRY(hipStreamWaitEvent(st, plan->ev_side_join, 0));
        return TSFA_OK;
    }
    ~SideJoin() {   // an error return: the error message of the call that failed stays
        if (used && hipEventRecord(plan->ev_side_join, plan->side) == hipSuccess) (void)hipStreamWaitEvent(st, plan->ev_side_join, 0);
    }
};

static int run_batch(tsfa_plan *plan, const void *d_values, int dtype, const double *d_times, const int64_t *d_starts,
                     const int64_t *d_ends, int64_t n_series, double *d_out, int64_t ld, const BatchShape &sh,
                     const int *d_sel, hipStream_t st, bool allow_side) {
    if (plan->fill_all && tsfa_launch_fill_nan(d_out, n_series, plan->n_cols, ld, st, plan->fill_value))
        return fail(TSFA_ERR_HIP, "fill launch failed");

    // Launch order: longest kernels first.
    static const int order_long_first[TSFA_N_FAMILIES] = {TSFA_FAM_ENTROPY, TSFA_FAM_AR, TSFA_FAM_SORT, TSFA_FAM_CWT, TSFA_FAM_BASIC,
                                                          TSFA_FAM_SEQ, TSFA_FAM_SPECTRAL, TSFA_FAM_TREND, TSFA_FAM_MPROFILE};
    // ... unless k_basic shares its per-series statistics (numpy-order mean / variance, extrema: plan->stats_buf,
    // TSFA_STATS_*) with the ENTROPY, AR, SEQ and SORT families, which then skip their own sums: BASIC goes first
    static const int order_basic_first[TSFA_N_FAMILIES] = {TSFA_FAM_BASIC, TSFA_FAM_ENTROPY, TSFA_FAM_AR, TSFA_FAM_SORT, TSFA_FAM_CWT,
                                                           TSFA_FAM_SEQ, TSFA_FAM_SPECTRAL, TSFA_FAM_TREND, TSFA_FAM_MPROFILE};
    const bool share_stats = plan->stats_buf.p != nullptr && !plan->stream_ok && plan->opt.stats_share;
    const int *order = share_stats ? order_basic_first : order_long_first;
    bool stats_valid[TSFA_N_LEN_CLASSES + 1];   // launch groups whose statistics record k_basic has written
    for (int g = 0; g <= TSFA_N_LEN_CLASSES; ++g) stats_valid[g] = false;
    // Two lanes: the side lane forks behind the main lane's ENTROPY family (lane_order below) and joins before the kernels
    // that follow the families -- on an error return too (SideJoin).  Not for a host call that goes out in several row
    // chunks (allow_side), and not while profiling: the timing slots then bracket kernels that run one after another on one
    // stream, so kernel_ms stays a serial per-kernel breakdown (the time a kernel takes alone, not the time it adds to a step
    // it shares with another lane).
    const unsigned side_mask = plan->opt.side_lane;
    bool pair = side_mask != 0 && !plan->profiling && allow_side && !plan->opt.force_long;
    for (int g = 0; g < sh.n_groups; ++g) pair = pair && sh.g_maxn[g] <= 4096;   // (the HBM-scratch build shares one scratch region)
    if (pair) {
        const int rc = side_ready(plan);
        if (rc) return rc;
    }
    // The head of the order up to and including ENTROPY (in both orders above nothing but BASIC precedes it, and neither may
    // go to the side lane), then the side lane's families, k_seq at their head, then the rest of the main lane's: the side
    // lane's first kernel starts when the main lane's next one does.  The order within each lane stays that of `order`.
    int lane_order[TSFA_N_FAMILIES];
    int fork_at = 0;
    if (pair) {
        int k = 0;
        do lane_order[k] = order[k]; while (order[k++] != TSFA_FAM_ENTROPY);
        fork_at = k;
        if ((side_mask >> TSFA_FAM_SEQ) & 1u) lane_order[k++] = TSFA_FAM_SEQ;
        for (int fi = fork_at; fi < TSFA_N_FAMILIES; ++fi)
            if (((side_mask >> order[fi]) & 1u) && order[fi] != TSFA_FAM_SEQ) lane_order[k++] = order[fi];
        for (int fi = fork_at; fi < TSFA_N_FAMILIES; ++fi)
            if (!((side_mask >> order[fi]) & 1u)) lane_order[k++] = order[fi];
        order = lane_order;
    }
    bool side_forked = false;
    SideJoin side_join{plan, st};
    hipStream_t long_lane = nullptr;     // the lane of the last launch from the HBM-scratch build (one scratch region for both)
    size_t slot = 0;
    // the sample order k_entropy_bits establishes is handed to k_sort through plan->perm_buf (2 bytes per sample): one
    // sort per series instead of two.  Per launch group: only where the bit-matrix sweep ran (float32 or float64 series
    // of 3 .. 1024 samples, LDS build); both families stay on the main lane, ENTROPY ahead of SORT.
    bool perm_valid[TSFA_N_LEN_CLASSES + 1];
    for (int g = 0; g <= TSFA_N_LEN_CLASSES; ++g) perm_valid[g] = false;
    const bool perm_share = plan->perm_buf.p != nullptr;
    bool stream_done[TSFA_N_LEN_CLASSES + 1];   // launch groups whose BASIC (+ SORT) columns k_stream has written
    for (int g = 0; g <= TSFA_N_LEN_CLASSES; ++g) stream_done[g] = false;
    for (int fi = 0; fi < TSFA_N_FAMILIES; ++fi) {
        const int f = order[fi];
        if (pair && !side_forked && fi == fork_at) {
            // everything launched so far (the caller's work on `st`, the fill, k_basic and its statistics record where they
            // are shared) precedes the side lane
            HIP_TRY(hipEventRecord(plan->ev_side_fork, st));
            HIP_TRY(hipStreamWaitEvent(plan->side, plan->ev_side_fork, 0));
            side_forked = true;
        }
        if (plan->fam_specs[f].empty()) continue;
        if (TSFA_LAB_ONLY(plan->debug_skip_fam == f)) continue;   // lab build (profiles/fill_audit.py): this family's cells keep the fill
        if (f == TSFA_FAM_BASIC && plan->stream_ok) {
            bool all = true;
            for (int g = 0; g < sh.n_groups; ++g) all = all && stream_done[g];
            if (all) continue;   // every group went through k_stream at the SORT (or this) family's turn
        }
        hipStream_t fst = st;
        if (side_forked && ((side_mask >> f) & 1u)) {
            fst = plan->side;
            side_join.used = true;
        }
        const char *slot_name = (plan->stream_ok && (f == TSFA_FAM_SORT || (f == TSFA_FAM_BASIC && plan->fam_specs[TSFA_FAM_SORT].empty())))
                                    ? "k_stream" : fam_names[f];
        if (record(plan, fst, slot, slot_name, true)) return fail(TSFA_ERR_HIP, "event record failed");
        std::vector<TsfaLaunch> perm_launches;   // SORT: the groups whose permutation_entropy columns go to k_perm (fam_perm.h)
        for (int g = sh.n_groups - 1; g >= 0; --g) {  // longest series first
            const int maxn = sh.g_maxn[g];
            const long long max_np2 = sh.g_np2[g];
            TsfaLaunch a;
            memset(&a, 0, sizeof a);
            a.fam = f;
            a.dtype = dtype;
            a.values = d_values;
            a.starts = d_starts;
            a.ends = d_ends;
            a.n_series = sh.g_count[g];
            a.sel = (sh.n_groups > 1) ? d_sel + sh.map.base[g] : nullptr;
            a.specs = plan->d_specs[f].get();
            a.nspecs = (int)plan->fam_specs[f].size();
            a.out = d_out;
            a.ld = ld;
            a.maxn = maxn;
            a.nt = (maxn <= 2048) ? 64 : 256;
            if (maxn > 2048) {
                // Long series: the LDS footprint leaves ONE workgroup per CU, so the wavefronts of that workgroup are all
                // the latency hiding there is.  Measured (profiles/nt_sweep.sh, 5 000 series, lengths 4096..8192 /
                // 2049..4096): number_cwt_peaks gains up to 1024 threads (31.6 -> 12.3 ms), the others peak at 512
                // beyond 4096 samples and at 256 below (more barriers than work).
                static const int nt_8k[TSFA_N_FAMILIES] = {512, 512, 512, 512, 256, 1024, 256, 256, 256};
                static const int nt_4k[TSFA_N_FAMILIES] = {256, 256, 256, 256, 256, 512, 256, 256, 256};
                a.nt = (maxn > 4096) ? nt_8k[f] : nt_4k[f];
            }
            if (maxn <= 2048) {
                // Wavefronts per series, measured on MI355X at n = 1024 (profiles/r01_*): the LDS footprint of a series
                // caps the workgroups per CU, so the latency-bound families gain from more wavefronts per workgroup,
                // while k_basic's many short reductions lose to the extra barriers.  At least 4 samples per thread.
                // AR: one wavefront per series.  Its time is serial linear algebra that a second wavefront only repeated,
                // and its layout (10 144 B at 1024 samples) puts 16 one-wavefront series on a CU; the workgroup size is
                // then the same for every length up to 2048, so a series gives the same bits in whatever group it lands.
                // SORT: one wavefront per series as well (round 8).  Its sweeps are short, and what lies between them -- the
                // corridor edges with lane = edge, the reductions' exchange through LDS, the refinement gate, the Householder
                // fit of wavefront 0, the lane = column epilogue -- a second wavefront waited for or repeated.  9 744 B at
                // 1024 float32 samples (the sorted series as a 16-bit order): 16 series per CU, and no dependence of the bits
                // on the launch group's longest series.  The plan option sort_waves = 2 keeps the 128-thread form reachable.
                static const int pref[TSFA_N_FAMILIES] = {64, 64, 128, 64, 256, 256, 128, 64, 256};
                const int cap = std::max(64, ((maxn / 4 + 63) / 64) * 64);
                a.nt = std::min(pref[f], cap);
                if (f == TSFA_FAM_SORT && plan->opt.sort_waves == 2) a.nt = std::min(128, cap);
            }
            if (TSFA_LAB_ONLY(plan->opt.nt[f] >= 64)) a.nt = plan->opt.nt[f];   // lab build: workgroup size of a family
            a.stream = fst;
            a.dectab = plan->d_dectab.get();
            a.times = d_times;
            a.twc = plan->d_twc.get();
            a.consts = plan->d_consts.get();
            a.tws = plan->d_tws.get();
            a.hint_a = plan->hints[f].a;
            a.hint_b = plan->hints[f].b;
            a.hint_c = plan->hints[f].c;
            a.hint_d = plan->hints[f].d;
            a.hint_e = plan->hints[f].e;
            a.alt = plan->hints[f].alt;
            a.cq = plan->hints[f].cq;
            // SPECTRAL beyond 2048 samples: 512 threads for EVERY series of such a group, not only where some series of the
            // group takes the chirp-z transform (whose passes over HBM scratch want them: profiles/r05_j, 2049..4096 samples
            // 2.36 -> 2.28 ms) -- the Welch sums depend on the workgroup size in the last bit, and a series must give the same
            // bits whatever else its shard holds (round-5 ADVICE)
            if (f == TSFA_FAM_SPECTRAL && maxn > 2048 && !TSFA_LAB_ONLY(plan->opt.nt[f] >= 64)) a.nt = 512;
            int aux = 0;
            if (f == TSFA_FAM_TREND) aux = a.alt.small_w;   // no n-double work array in LDS (TsfaAltPlan::small_w)
            if (f == TSFA_FAM_MPROFILE) aux = (dtype == TSFA_F32) ? 4 : 8;   // the series is resident in its input precision
            if (f == TSFA_FAM_SPECTRAL) {
                // only non-power-of-two lengths <= 256 use the table-driven DFT (longer ones: Goertzel, no table)
                a.dft_n = (int)std::min<long long>(max_np2, 256);
                aux = a.dft_n;
                // long series of non-power-of-two length: three power-of-two FFTs through HBM scratch (Bluestein,
                // fam_spectral.h) instead of the O(n^2) Goertzel sweep; 32 M bytes per workgroup, at most 6 GB per launch
                int bl_odd = TSFA_BLUESTEIN_MIN, bl_even = TSFA_BLUESTEIN_MIN_EVEN;
                // (A/B of the crossover, tests.  32 767: both crossovers travel packed in one int)
                if (plan->opt.bluestein_min > 0) bl_odd = bl_even = std::min(std::max(plan->opt.bluestein_min, 17), 32767);
                a.bluestein_min = TSFA_BLUESTEIN_PACK(bl_odd, bl_even);
                // (a group whose longest non-power-of-two series lies beyond the transform's reach still gets the scratch, sized
                //  for the longest length within it: its shorter series take the route they take in any other company; none
                //  where even the shortest series of the shard lies beyond it)
                if (max_np2 >= std::min(bl_odd, bl_even) && sh.min_len <= 32768 && plan->opt.bluestein) {
                    const long long reach = std::min<long long>(max_np2, 32767);
                    long long M = 1;
                    while (M < 2 * reach - 1) M <<= 1;
                    // one slot per workgroup of a launch; at most 1 GB (and at least the 2048 workgroups of the long-series
                    // build's persistent grid, 2 MB each at the longest length): a larger group goes out in several launches
                    const size_t slot_bytes = (size_t)(4 * M) * sizeof(double);
                    // (1 GB: a launch of >= 2048 workgroups already fills the chip several times over, and a plan keeps this
                    //  scratch for its lifetime -- six cached plans per thread, one per device: round-5 ADVICE)
                    int64_t slots = std::min<int64_t>(a.n_series, std::max<int64_t>((int64_t)((1ull << 30) / slot_bytes), 2048));
                    if (plan->opt.gscratch_slots > 0) slots = std::min<int64_t>(slots, plan->opt.gscratch_slots);   // test hook: several launches per group
                    const size_t bytes = (size_t)slots * slot_bytes;
                    if (plan->gscratch.ensure(bytes) == 0) {
                        a.gscratch = (double *)plan->gscratch.p;
                        a.gscratch_n = (int)(4 * M);
                        a.gscratch_slots = slots;
                        // the transform's passes over its HBM scratch want more wavefronts than the LDS-resident phases
                        // (profiles/r05_j: 2049..4096 samples 2.36 -> 2.28 ms at 512 threads).  Up to 2048 samples the family's
                        // own 128 stay although 256 measured faster on 1025..2048 (1.76 -> 1.59 ms): there the workgroup size
                        // is the same for every launch group, and the Welch sums depend on it in the last bit -- a series must
                        // give the same bits in whatever shard it lands (test_extract_features_on_several_devices_from_one_process)
                    }
                }
            } else if (f == TSFA_FAM_CWT) {
                a.cwt_rowv = tsfa_family_lds_bytes(f, maxn, a.nt, 1) <= 96 * 1024 ? 1 : 0;
                a.cwt_links = plan->opt.cwt_links;
                aux = a.cwt_rowv;
            } else if (f == TSFA_FAM_AR) {
                // leading dimension of the normal matrices: ADF needs maxlag(n) + 3, AR(k) needs k + 2
                int P = 8, Pdd = 8;   // (Pdd: ar_coefficient orders beyond TSFA_AR_TABLE_K are fitted by the second pass alone)
                for (const auto &s : plan->fam_specs[f]) {
                    if (s.calc == TSFA_C_AUGMENTED_DICKEY_FULLER) {
                        int ml = (int)ceil(12.0 * pow((double)maxn / 100.0, 0.25));
                        if (maxn / 2 - 2 < ml) ml = maxn / 2 - 2;
                        P = std::max(P, ml + 3);
                    } else if (s.calc == TSFA_C_AR_COEFFICIENT) {
                        const int k = std::min((int)s.p[1], std::max(1, (maxn - 2) / 2));   // (n < 2 k + 2: no fit, fc.py:1497)
                        if ((int)s.p[1] <= TSFA_AR_TABLE_K) P = std::max(P, (int)s.p[1] + 2);
                        Pdd = std::max(Pdd, k + 2);
                        a.ar_has_coef = 1;
                    }
                }
                Pdd = std::max(Pdd, P);
                a.ar_P = P;
                a.ar_P_dd = Pdd;
                aux = P;
                {   // second pass (k_ar_degenerate): double-double normal equations in LDS up to P = 64 (65 535 samples), HBM beyond
                    ArDdLds D;
                    if (D.carve(nullptr, Pdd) > TSFA_LDS_LIMIT - 2048) {
                        const size_t slot_bytes = (size_t)ArDdLds::scratch_doubles(Pdd) * sizeof(double);
                        const int slots = (int)std::min<int64_t>(a.n_series, std::min<int64_t>(256, std::max<int64_t>(8, (int64_t)(((size_t)2 << 30) / slot_bytes))));
                        if (plan->dd_scratch.ensure((size_t)slots * slot_bytes))
                            return fail(TSFA_ERR_HIP, "hipMalloc failed for the second AR pass");
                        a.dd_scratch = (double *)plan->dd_scratch.p;
                        a.dd_slots = slots;
                    }
                }
                a.deg_list = (long long *)plan->deg_list.p;
                a.deg_count = plan->d_deg_count.get();
                HIP_TRY(hipMemsetAsync(plan->d_deg_count.get(), 0, sizeof(int), fst));
            } else if (f == TSFA_FAM_SORT && plan->hints[f].b > 0) {
                // Langevin fits: ill-conditioned ones are recorded for the double-double pass (fam_langevin_dd.h)
                a.pf_slot = tsfa_pf_slot_doubles(plan->hints[f].b);
                a.pf_buf = (double *)plan->pf_buf.p;
                a.pf_count = plan->d_deg_count.get() + 1;
                a.pf_cap = (int)std::min<long long>((long long)n_series * std::max(1, plan->hints[f].e), 2147483647LL);
                HIP_TRY(hipMemsetAsync(a.pf_count, 0, sizeof(int), fst));
            } else if (f == TSFA_FAM_ENTROPY) {
                // one wavefront per 64-template row block, up to four per series; the symmetric sweep needs 12 B of
                // LDS counters per sample
                const int waves = std::min(4, std::max(1, (maxn - 1 + 63) / 64));
                a.nt = std::max(a.nt, 64 * waves);
                a.ent_cnt = tsfa_entropy_lds_bytes(maxn, 1) <= TSFA_LDS_LIMIT ? 1 : 0;
                a.ent_fast = a.ent_cnt;
                for (const auto &s : plan->fam_specs[f])
                    if (s.calc == TSFA_C_APPROXIMATE_ENTROPY && (int)s.p[0] != 2) a.ent_fast = 0;
                if (plan->opt.entropy_route == 2) a.ent_fast = 0;  // test hook: the general kernel
                // series up to TSFA_ENTB_MAXN samples: the bit-matrix sweep (fam_entropy_bits.h) -- sorted ranges + bit
                // rows instead of a distance per pair; one (strip, tolerance) task per wavefront register slot
                // (a single tolerance: the windowed pair sweep is the cheaper one -- 7.7 vs 9.0 ms per 100k x 1024 -- the sample
                //  sort, the table and the ranges do not amortise)
                // (1025 .. TSFA_ENTB_MAXN_WIDE samples, round 6: the same 48-byte-entry sweep with one workgroup per CU -- the
                //  16-byte-entry form below builds 22 column parts at 2048 samples, this one 6, and the kernel waits for the
                //  barriers around a build more than for its instructions: profiles/r06_w)
                const bool entb_wide = maxn > TSFA_ENTB_MAXN && maxn <= TSFA_ENTB_MAXN_WIDE &&
                                       tsfa_entropy_lds_bytes(maxn, 2) <= TSFA_LDS_LIMIT &&
                                       entb_kround(maxn, std::min(a.nspecs, TSFA_ENTB_MAXK), TSFA_ENTB_MAXWAVES) >= std::min(a.nspecs, TSFA_ENTB_MAXK);
                if (a.ent_fast && a.nspecs >= 2 && maxn >= 3 && plan->opt.entropy_route == 0 &&
                    ((maxn <= TSFA_ENTB_MAXN && tsfa_entropy_lds_bytes(maxn, 2) <= TSFA_LDS_LIMIT / 2) || entb_wide)) {
                    a.ent_cnt = 2;
                    a.nt = 64 * std::min(TSFA_ENTB_MAXWAVES, entb_waves_for(maxn, a.nspecs));
                    if (TSFA_LAB_ONLY(plan->opt.nt[f] >= 64)) a.nt = plan->opt.nt[f];
                } else if (a.ent_fast && a.nspecs >= 2 && maxn > TSFA_ENTB_MAXN && maxn <= TSFA_ENTB_MAXN_LONG &&
                           plan->opt.entropy_route == 0 &&
                           tsfa_entropy_lds_bytes(maxn, 3) <= TSFA_LDS_LIMIT) {
                    // 1025 .. 4096 samples: the same sweep with 16-byte table entries (a column part of 96 columns still
                    // fits LDS) and the tolerances in rounds of as many as 16 wavefronts hold in registers; one
                    // workgroup per CU.  The pair sweep is O(n^2) float64 operations per tolerance: 101.6 ms per
                    // 10 000 series of 4096 samples (profiles/r03_shapes.txt) against ... for this one.
                    a.ent_cnt = 3;
                    a.nt = 64 * TSFA_ENTB_MAXWAVES;
                } else if (a.nspecs >= 2 && maxn > TSFA_ENTB_MAXN_LONG && maxn <= TSFA_ENTH_MAXN && plan->opt.entropy_route == 0) {
                    // 4097 .. 19 000 samples (fam_entropy_hbits.h, the long-series build): the table of one diagonal word per
                    // column part in LDS, the per-sample arrays in the workgroup's HBM slot, the tasks in register batches.
                    // The pair sweep it replaces: 0.45 ms per series of 16 384 samples with the GPU full (profiles/r04_long_entropy.md)
                    bool all_m2 = true;
                    for (const auto &s : plan->fam_specs[f])
                        if (s.calc == TSFA_C_APPROXIMATE_ENTROPY && (int)s.p[0] != 2) all_m2 = false;
                    if (all_m2) {
                        a.ent_cnt = 4;
                        a.ent_fast = 0;
                        a.nt = 64 * TSFA_ENTB_MAXWAVES;
                    }
                }
            }
            // SEQ: one launch parses up to TSFA_LZ_MAX_GROUP `bins` values side by side -- as many as LDS allows
            int seq_group = 0;
            if (f == TSFA_FAM_SEQ) {
                for (seq_group = std::min(a.nspecs, TSFA_LZ_MAX_GROUP); seq_group > 1; --seq_group) {
                    bool fits = true;
                    for (int s0 = 0; fits && s0 < a.nspecs; s0 += seq_group) {
                        lz_build_group(plan->fam_specs[f].data() + s0, std::min(seq_group, a.nspecs - s0), maxn, &a.seq);
                        fits = tsfa_seq_lds_bytes(a.seq) <= TSFA_LDS_LIMIT;
                    }
                    if (fits) break;
                }
                lz_build_group(plan->fam_specs[f].data(), std::min(seq_group, a.nspecs), maxn, &a.seq);
            }
            size_t seq_lds = 0;  // the largest launch of the family at this group size
            int seq_grows = 0;
            if (f == TSFA_FAM_SEQ) {
                TsfaSeqGroup g;
                for (int s0 = 0; s0 < a.nspecs; s0 += seq_group) {
                    lz_build_group(plan->fam_specs[f].data() + s0, std::min(seq_group, a.nspecs - s0), maxn, &g);
                    seq_lds = std::max(seq_lds, tsfa_seq_lds_bytes(g));
                }
                // The symbol rows in HBM (k_seq<T, true>): LDS then holds the tables alone, and the family is bound by
                // (series resident per CU) x (latency of a parse step).  Taken where it puts more workgroups on a CU and the
                // rows of the launch's workgroups fit 2 GB; every `bins` value of the plan in one launch then.
                if (plan->opt.seq_rows != 0 && !plan->opt.force_long) {
                    const int group_g = std::min(a.nspecs, TSFA_LZ_MAX_GROUP);
                    size_t lds_g = 0, stride_g = 0;
                    for (int s0 = 0; s0 < a.nspecs; s0 += group_g) {
                        lz_build_group(plan->fam_specs[f].data() + s0, std::min(group_g, a.nspecs - s0), maxn, &g, 1);
                        lds_g = std::max(lds_g, tsfa_seq_lds_bytes(g));
                        stride_g = std::max(stride_g, (size_t)g.stride);
                    }
                    auto resident = [&](size_t lds) {
                        if (lds > TSFA_LDS_LIMIT) return (size_t)0;
                        return std::min<size_t>((size_t)(163840 / std::max<size_t>(lds, 1)), (size_t)(32 * 64 / a.nt));
                    };
                    const bool more = resident(lds_g) > resident(seq_lds);
                    if (lds_g <= TSFA_LDS_LIMIT && (plan->opt.seq_rows == 1 || more) &&
                        (size_t)a.n_series * stride_g <= ((size_t)2 << 30) &&
                        plan->seq_rows.ensure((size_t)a.n_series * stride_g) == 0) {
                        seq_grows = 1;
                        seq_group = group_g;
                        seq_lds = lds_g;
                        a.seq_rows = (unsigned char *)plan->seq_rows.p;
                    }
                }
            }
            size_t lds = (f == TSFA_FAM_SEQ) ? seq_lds
                         : (f == TSFA_FAM_ENTROPY) ? tsfa_entropy_lds_bytes(maxn, a.ent_cnt)
                                                   : tsfa_family_lds_bytes(f, maxn, a.nt, aux);
            // A series whose working set does not fit a CU's LDS runs from the long-series build of the same kernels
            // (tsfa_kernels_long.hip): the working set in a slot of HBM scratch per resident workgroup, a persistent
            // grid walking the group's series.  Slower per sample, but every length up to 65 535 extracts.
            const bool use_long = lds > TSFA_LDS_LIMIT || plan->opt.force_long || (f == TSFA_FAM_ENTROPY && a.ent_cnt == 4);
            if (TSFA_LAB_ONLY(f == TSFA_FAM_SPECTRAL && plan->opt.trace))
                fprintf(stderr, "[tsfa] spectral group %d: n_series %lld maxn %d max_np2 %lld lds %zu long %d chirp-z %d slots %lld nt %d\n", g,
                        (long long)a.n_series, maxn, max_np2, lds, (int)use_long, (int)(a.gscratch != nullptr), (long long)a.gscratch_slots, a.nt);
            if (use_long) {
                if (!(f == TSFA_FAM_ENTROPY && a.ent_cnt == 4)) a.nt = 256;
                // the long-series build's persistent grid indexes the chirp-z scratch by workgroup: a slot for each, or none
                if (a.gscratch != nullptr && a.gscratch_slots < std::min<int64_t>(a.n_series, 2048)) a.gscratch = nullptr;
                if (f == TSFA_FAM_ENTROPY && a.ent_cnt != 4) { a.ent_cnt = 0; a.ent_fast = 0; lds = tsfa_entropy_lds_bytes(maxn, 5); }
                if (f == TSFA_FAM_CWT) { a.cwt_rowv = 0; lds = tsfa_family_lds_bytes(f, maxn, a.nt, 0); }
                if (f == TSFA_FAM_SEQ) {
                    seq_group = std::min(a.nspecs, TSFA_LZ_MAX_GROUP);
                    seq_grows = 0;
                    lds = 0;
                    for (int s0 = 0; s0 < a.nspecs; s0 += seq_group) {
                        lz_build_group(plan->fam_specs[f].data() + s0, std::min(seq_group, a.nspecs - s0), maxn, &a.seq);
                        lds = std::max(lds, tsfa_seq_lds_bytes(a.seq));
                    }
                } else if (f != TSFA_FAM_ENTROPY && f != TSFA_FAM_CWT) {
                    lds = tsfa_family_lds_bytes(f, maxn, a.nt, aux);
                }
                const size_t slot_bytes = (lds + 255) & ~(size_t)255;
                const int64_t n_slots = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(a.n_series, 512),
                                                                               (int64_t)((4ull << 30) / slot_bytes)));
                if (plan->long_scratch.ensure((size_t)n_slots * slot_bytes))
                    return fail(TSFA_ERR_HIP, "hipMalloc failed for the long-series scratch");
                a.long_scratch = (unsigned char *)plan->long_scratch.p;
                a.long_bytes = (size_t)n_slots * slot_bytes;
                if (pair) {   // one scratch region: a launch that uses it waits for the other lane's last one
                    if (long_lane != nullptr && long_lane != fst) {
                        HIP_TRY(hipEventRecord(plan->ev_side_long, long_lane));
                        HIP_TRY(hipStreamWaitEvent(fst, plan->ev_side_long, 0));
                    }
                    long_lane = fst;
                }
            }
            if (share_stats && g <= TSFA_N_LEN_CLASSES) {
                if (f == TSFA_FAM_BASIC && !(plan->hints[f].c == 0 && a.nt <= 256)) {   // (k_basic_lite does not export)
                    a.stats_out = (double *)plan->stats_buf.p;
                    stats_valid[g] = true;
                } else if ((f == TSFA_FAM_ENTROPY || f == TSFA_FAM_AR || f == TSFA_FAM_SEQ || f == TSFA_FAM_SORT) && stats_valid[g]) {
                    a.stats_in = (const double *)plan->stats_buf.p;
                }
            }
            if (perm_share && !use_long && g <= TSFA_N_LEN_CLASSES) {
                if (f == TSFA_FAM_ENTROPY && a.ent_cnt == 2 && maxn <= TSFA_ENTB_MAXN) {   // (the shared order: rows of TSFA_ENTB_MAXN entries)
                    a.perm_buf = (unsigned short *)plan->perm_buf.p;
                    a.perm_stride = TSFA_ENTB_MAXN;
                    perm_valid[g] = true;
                } else if (f == TSFA_FAM_SORT && perm_valid[g]) {
                    a.perm_buf = (unsigned short *)plan->perm_buf.p;
                    a.perm_stride = TSFA_ENTB_MAXN;
                }
            }
            if (f == TSFA_FAM_SORT) {
                // every permutation_entropy column of the plan from one sweep, in a kernel of its own (hints.d: one stride,
                // the dimensions 3 .. 7): where the series and the histogram of all patterns fit LDS -- also beside the
                // HBM-scratch build of k_sort -- with at most eight windows per thread; k_sort then skips those columns
                a.hint_d = 0;
                if (plan->hints[f].d != 0) {
                    const int pnt = (maxn <= 2048) ? std::min(256, std::max(64, ((maxn / 4 + 63) / 64) * 64))
                                                   : std::min(1024, ((maxn / 8 + 63) / 64) * 64);
                    // (k_perm packs two 16-bit counters per word: safe while a series holds at most 65 535 windows -- LDS
                    //  admits 40 960 float32 samples; asserted here rather than implied, round-4 ADVICE)
                    if (maxn <= 65535 && tsfa_perm_lds_bytes(maxn, pnt, dtype == TSFA_F32 ? 4 : 8) <= TSFA_LDS_LIMIT) {
                        a.hint_d = plan->hints[f].d;
                        TsfaLaunch pa = a;
                        pa.nt = pnt;
                        pa.long_scratch = nullptr;
                        perm_launches.push_back(pa);
                    }
                }
            }
            if (f == TSFA_FAM_SORT && !use_long) {
                // one wavefront per series (k_sort<T, 1>); where k_entropy_bits left the sample order and k_perm takes the
                // permutation_entropy columns (a dimension >= 8 would borrow the sorted copy's storage), the sorted series is
                // that order in LDS and not a copy (k_sort<T, 2>).  The layout follows: the kernel carves with these arguments.
                a.sort_mode = (maxn <= 2048 && a.nt == 64 && plan->opt.sort_waves == 1 && !TSFA_LAB_ONLY(plan->opt.nt[f] >= 64))
                                  ? ((a.perm_buf != nullptr && a.hint_d != 0) ? 2 : 1) : 0;
                lds = tsfa_sort_lds_bytes(a, dtype == TSFA_F32 ? 4 : 8);
            }
            // tsfa_plan_last_launches: what this (family, group) is about to launch (a group k_stream already served launches nothing)
            if (!(plan->stream_ok && (f == TSFA_FAM_SORT || f == TSFA_FAM_BASIC) && maxn <= 2048 && g <= TSFA_N_LEN_CLASSES && stream_done[g])) {
                tsfa_launch_info li;
                li.family = f;
                li.length_class = g;
                li.max_len = maxn;
                li.threads = a.nt;
                li.n_series = a.n_series;
                li.lds_bytes = (int64_t)lds;
                li.long_build = use_long ? 1 : 0;
                li.variant = (f == TSFA_FAM_ENTROPY) ? a.ent_cnt
                             : (f == TSFA_FAM_CWT) ? a.cwt_rowv
                             : (f == TSFA_FAM_SEQ) ? (seq_group | (seq_grows << 8))
                             : (f == TSFA_FAM_SPECTRAL) ? (a.gscratch != nullptr ? 1 : 0)
                             : (f == TSFA_FAM_SORT) ? ((a.hint_d != 0 ? 1 : 0) | (a.sort_mode << 1))   // bit 1: one wavefront, bit 2: ... with the 16-bit order
                             : (f == TSFA_FAM_AR) ? (a.dd_scratch != nullptr ? 1 : 0) : 0;
                plan->launches.push_back(li);
            }
            int rc = 0;
            if (plan->stream_ok && (f == TSFA_FAM_SORT || f == TSFA_FAM_BASIC) && maxn <= 2048 && g <= TSFA_N_LEN_CLASSES) {
                if (stream_done[g]) continue;   // BASIC's turn after the SORT family's launch served both
                TsfaLaunch sa = a;
                sa.specs = plan->d_specs[TSFA_FAM_SORT].get();
                sa.nspecs = (int)plan->fam_specs[TSFA_FAM_SORT].size();
                sa.bspecs = plan->d_specs[TSFA_FAM_BASIC].get();
                sa.nbspecs = (int)plan->fam_specs[TSFA_FAM_BASIC].size();
                rc = tsfa_launch_stream(sa);
                stream_done[g] = true;
            } else
            if (f == TSFA_FAM_SORT && plan->sort_only_order_stats && maxn <= 2048 && !use_long &&
                plan->opt.select) {
                // a plan that only asks the sort family for median / quantile columns (MinimalFCParameters): selection
                // in registers, one wavefront per series, no sorted copy (tsfa_kernels.hip: k_order_stats)
                rc = tsfa_launch_order_stats(a);
            } else if (f == TSFA_FAM_SEQ) {
                for (int s0 = 0; rc == 0 && s0 < a.nspecs; s0 += seq_group) {
                    lz_build_group(plan->fam_specs[f].data() + s0, std::min(seq_group, a.nspecs - s0), maxn, &a.seq, seq_grows);
                    if (!use_long && tsfa_seq_lds_bytes(a.seq) > TSFA_LDS_LIMIT)
                        return fail(TSFA_ERR_TOO_LONG, "k_seq: a series of " + std::to_string(maxn) + " samples does not fit LDS");
                    rc = use_long ? tsfa_launch_family_long(a) : tsfa_launch_family(a);
                }
            } else {
                // BASIC / TREND: a series of at most TSFA_ROW_MAXN samples is evaluated by the row form (four series per
                // wavefront, tsfa_common.h BlkRow) whatever else its launch group holds -- its length alone decides, so it
                // gives the same bits in every batch and shard; the family kernel skips those series
                bool rows_any = false, rows_all = false;
                const bool lite = (f == TSFA_FAM_BASIC && plan->hints[f].c == 0 && a.nt <= 256);   // (k_basic_lite: closed forms only)
                if ((f == TSFA_FAM_BASIC || f == TSFA_FAM_TREND) && plan->opt.row_form && !lite && g <= TSFA_N_LEN_CLASSES) {
                    rows_any = sh.g_has_short[g];
                    rows_all = maxn <= TSFA_ROW_MAXN;
                }
                if (rows_any) {
                    a.skip_le = TSFA_ROW_MAXN;
                    rc = tsfa_launch_rows(a);
                }
                if (rc == 0 && !rows_all) rc = use_long ? tsfa_launch_family_long(a) : tsfa_launch_family(a);
            }
            if (rc == 0 && f == TSFA_FAM_AR) rc = tsfa_launch_ar_degenerate(a);
            if (rc == 0 && f == TSFA_FAM_SORT && a.pf_buf) rc = tsfa_launch_langevin_dd(a);
            if (rc) return fail(TSFA_ERR_HIP, std::string(fam_names[f]) + " launch failed: " +
                                                  (rc == -2 ? "no scratch slot" : hipGetErrorString((hipError_t)rc)));
        }
        if (record(plan, fst, slot, slot_name, false)) return fail(TSFA_ERR_HIP, "event record failed");
        ++slot;
        if (!perm_launches.empty()) {   // on the SORT family's lane
            if (record(plan, fst, slot, "k_perm", true)) return fail(TSFA_ERR_HIP, "event record failed");
            for (auto &pa : perm_launches) {
                const int rc = tsfa_launch_perm(pa);
                if (rc) return fail(TSFA_ERR_HIP, std::string("k_perm launch failed: ") + hipGetErrorString((hipError_t)rc));
            }
            if (record(plan, fst, slot, "k_perm", false)) return fail(TSFA_ERR_HIP, "event record failed");
            ++slot;
        }
        if (plan->opt.fail_after == f) return fail(TSFA_ERR_INVALID, std::string("fail_after: leaving after ") + fam_names[f]);
    }
    {
        const int rc = side_join.join();
        if (rc) return rc;
    }
    if (plan->bank.C > 0) {
        TsfaCwtLaunch c;
        memset(&c, 0, sizeof c);
        c.dtype = dtype;
        c.values = d_values;
        c.starts = d_starts;
        c.ends = d_ends;
        c.n_series = n_series;
        c.W = plan->d_W.get();
        c.S4 = plan->bank.S4;
        c.C = plan->bank.C;
        c.cols = plan->d_cols.get();
        c.coeff_idx = plan->d_coeff.get();
        c.out = d_out;
        c.ld = ld;
        c.stream = st;
        if (record(plan, st, slot, "k_cwt_gemm", true)) return fail(TSFA_ERR_HIP, "event record failed");
        const int rc = tsfa_launch_cwt(c);
        if (rc) return fail(TSFA_ERR_HIP, "k_cwt_gemm launch failed");
        if (record(plan, st, slot, "k_cwt_gemm", false)) return fail(TSFA_ERR_HIP, "event record failed");
        ++slot;
    }
    if (!plan->gen_specs.empty()) {
        // one launch over every series of the batch, a slot of HBM scratch per resident workgroup (at most 1 GB in all)
        const int maxn = (int)sh.max_len;
        const size_t slot_doubles = tsfa_general_slot_doubles(maxn, plan->gen_plan) + 8;
        int slots = (int)std::min<int64_t>(n_series, 2048);
        const size_t budget = (size_t)1 << 30;
        if ((size_t)slots * slot_doubles * sizeof(double) > budget)
            slots = (int)std::max<size_t>(16, budget / (slot_doubles * sizeof(double)));
        slots = (int)std::min<int64_t>(slots, n_series);
        if (plan->gen_scratch.ensure((size_t)slots * slot_doubles * sizeof(double)))
            return fail(TSFA_ERR_HIP, "hipMalloc failed for the scratch of k_general");
        TsfaLaunch a;
        memset(&a, 0, sizeof a);
        a.dtype = dtype;
        a.values = d_values;
        a.starts = d_starts;
        a.ends = d_ends;
        a.n_series = n_series;
        a.specs = plan->d_gen_specs.get();
        a.nspecs = (int)plan->gen_specs.size();
        a.out = d_out;
        a.ld = ld;
        a.maxn = maxn;
        a.stream = st;
        if (record(plan, st, slot, "k_general", true)) return fail(TSFA_ERR_HIP, "event record failed");
        if (tsfa_launch_general(a, plan->gen_plan, (double *)plan->gen_scratch.p, slot_doubles, slots, plan->d_pool.get()))
            return fail(TSFA_ERR_HIP, "k_general launch failed");
        if (record(plan, st, slot, "k_general", false)) return fail(TSFA_ERR_HIP, "event record failed");
        ++slot;
    }
    if (plan->profiling) plan->timings.resize(slot);
    return TSFA_OK;
}

// Series of any length extract (beyond a CU's LDS from the long-series build: 32-bit indices, working set in HBM) -- since
// round 6 also under sample_entropy / approximate_entropy: bit-matrix sweeps to 17 408 samples, beyond that the O(n^2) pair
// sweep of the long-series build with a 32-bit sample order (the reference's own approximate_entropy allocates an n x n x m
// float64 array there: 160 GB at 100 000 samples, MemoryError; its sample_entropy has no such limit).
static int check_shape(const tsfa_plan *plan, const BatchShape &sh) {
    if (sh.min_len < 1) return fail(TSFA_ERR_INVALID, "every series must hold at least one sample");
    if (sh.max_len > 2147483647LL / 64) return fail(TSFA_ERR_TOO_LONG, "series longer than 33 554 431 samples are not supported");
    return TSFA_OK;
}

// index lists of the launch groups (device), from the device-resident views
static int build_sel(tsfa_plan *plan, const int64_t *d_starts, const int64_t *d_ends, int64_t n_series, const BatchShape &sh,
                     int *d_sel, hipStream_t st) {
    if (sh.n_groups <= 1) return TSFA_OK;
    HIP_TRY(hipMemsetAsync(plan->d_cursor.get(), 0, TSFA_N_LEN_CLASSES * sizeof(int), st));
    if (tsfa_launch_class_fill(d_starts, d_ends, n_series, sh.map, plan->d_cursor.get(), d_sel, st))
        return fail(TSFA_ERR_HIP, "class_fill launch failed");
    return TSFA_OK;
}

int tsfa_extract_windows(tsfa_plan *plan, const void *values, int32_t dtype, const double *times, const int64_t *starts,
                         const int64_t *ends, int64_t n_series, double *out, int64_t ld_out, int32_t space,
                         void *stream) {
    if (!plan) return fail(TSFA_ERR_INVALID, "plan is NULL");
    if (plan->needs_times && !times)
        return fail(TSFA_ERR_INVALID, "the plan holds linear_trend_timewise columns: call tsfa_extract_timed with the "
                                      "per-sample times (the reference skips the calculator without a DatetimeIndex)");
    if (dtype != TSFA_F32 && dtype != TSFA_F64) return fail(TSFA_ERR_INVALID, "dtype must be TSFA_F32 or TSFA_F64");
    if (space != TSFA_HOST && space != TSFA_DEVICE) return fail(TSFA_ERR_INVALID, "space must be TSFA_HOST or TSFA_DEVICE");
    if (n_series < 0) return fail(TSFA_ERR_INVALID, "n_series < 0");
    plan->launches.clear();
    if (n_series == 0 || plan->n_cols == 0) return TSFA_OK;
    if (!values || !starts || !ends || !out) return fail(TSFA_ERR_INVALID, "NULL buffer");
    if (ld_out < plan->n_cols) return fail(TSFA_ERR_INVALID, "ld_out < n_cols");
    if (n_series > 2147483647LL) return fail(TSFA_ERR_INVALID, "n_series exceeds the grid limit (2^31 - 1)");
    HIP_TRY(hipSetDevice(plan->device));
    const size_t esz = (dtype == TSFA_F32) ? 4 : 8;
    if (plan->deg_list.ensure((size_t)n_series * sizeof(long long)))
        return fail(TSFA_ERR_HIP, "hipMalloc failed for the k_ar_degenerate list");
    if (!plan->fam_specs[TSFA_FAM_SORT].empty() && !plan->fam_specs[TSFA_FAM_ENTROPY].empty() && !plan->sort_only_order_stats &&
        plan->perm_buf.ensure((size_t)n_series * (size_t)TSFA_ENTB_MAXN * sizeof(unsigned short)))
        return fail(TSFA_ERR_HIP, "hipMalloc failed for the shared sample order");
    if (!plan->fam_specs[TSFA_FAM_BASIC].empty() && !plan->stream_ok &&
        (!plan->fam_specs[TSFA_FAM_ENTROPY].empty() || !plan->fam_specs[TSFA_FAM_AR].empty() || !plan->fam_specs[TSFA_FAM_SEQ].empty() ||
         !plan->fam_specs[TSFA_FAM_SORT].empty()) &&
        plan->stats_buf.ensure((size_t)n_series * TSFA_STATS_N * sizeof(double)))
        return fail(TSFA_ERR_HIP, "hipMalloc failed for the shared per-series statistics");
    if (plan->hints[TSFA_FAM_SORT].b > 0 &&
        plan->pf_buf.ensure((size_t)n_series * (size_t)std::max(1, plan->hints[TSFA_FAM_SORT].e) *
                            (size_t)tsfa_pf_slot_doubles(plan->hints[TSFA_FAM_SORT].b) * sizeof(double)))
        return fail(TSFA_ERR_HIP, "hipMalloc failed for the records of the Langevin second pass");

    if (space == TSFA_DEVICE) {
        hipStream_t st = stream ? (hipStream_t)stream : plan->stream;
        // ---- batch length statistics (decide workgroup sizes, LDS carves and the length-class launch groups) ----
        long long h_stats[TSFA_LEN_STATS];
        for (int i = 0; i < TSFA_LEN_STATS; ++i) h_stats[i] = 0;
        h_stats[1] = (1LL << 62);
        BatchShape sh;
        if (plan->hint_max_len > 0) {
            // the caller vouches for the length range of every batch (tsfa_plan_set_length_hint): no scan, no host sync
            // -- back-to-back calls on one stream (chunks of a shard) are enqueued without waiting for each other;
            // one launch group, carved for the longest promised length
            h_stats[0] = plan->hint_max_len;
            h_stats[1] = plan->hint_min_len;
            h_stats[2] = (plan->hint_min_len == plan->hint_max_len && (plan->hint_max_len & (plan->hint_max_len - 1)) == 0)
                             ? 0 : plan->hint_max_len;  // longest length that may not be a power of two
            sh.max_len = h_stats[0];
            sh.min_len = h_stats[1];
            sh.max_np2 = h_stats[2];
            sh.g_maxn[0] = (int)h_stats[0];
            sh.g_np2[0] = h_stats[2];
            sh.g_count[0] = n_series;
            sh.g_has_short[0] = plan->hint_min_len <= TSFA_ROW_MAXN;
            memset(&sh.map, 0, sizeof sh.map);
        } else {
            HIP_TRY(hipMemcpyAsync(plan->d_stats.get(), h_stats, sizeof h_stats, hipMemcpyHostToDevice, st));
            if (tsfa_launch_len_stats(starts, ends, n_series, plan->d_stats.get(), st)) return fail(TSFA_ERR_HIP, "len_stats launch failed");
            HIP_TRY(hipMemcpyAsync(h_stats, plan->d_stats.get(), sizeof h_stats, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            shape_from_stats(h_stats, n_series, sh, plan->opt.length_classes);
        }
        int rc = check_shape(plan, sh);
        if (rc) return rc;
        int *d_sel = nullptr;
        if (sh.n_groups > 1) {
            if (plan->sel.ensure((size_t)n_series * sizeof(int))) return fail(TSFA_ERR_HIP, "hipMalloc failed for the length-class lists");
            d_sel = (int *)plan->sel.p;
            if ((rc = build_sel(plan, starts, ends, n_series, sh, d_sel, st))) return rc;
        }
        if ((rc = run_batch(plan, values, dtype, plan->needs_times ? times : nullptr, starts, ends, n_series, out, ld_out, sh,
                            d_sel, st, true)))
            return rc;
        const bool async = (stream != nullptr);
        if (!async || plan->profiling) {
            HIP_TRY(hipStreamSynchronize(st));
            if (plan->profiling)
                for (auto &t : plan->timings) (void)hipEventElapsedTime(&t.ms, t.e0, t.e1);
        }
        return TSFA_OK;
    }

    // ---------------------------------------------------------------------------------------------------------
    // TSFA_HOST: the batch is cut into row chunks that travel as a pipeline over three streams --
    //   copy-in stream : values of chunk c + 1 (H2D)        (pinned host memory: true DMA; pageable: the runtime stages)
    //   compute stream : kernels of chunk c
    //   copy-out stream: rows of chunk c - 1 (D2H, strided into the caller's matrix)
    // so PCIe traffic hides behind the kernels instead of bracketing them.
    // ---------------------------------------------------------------------------------------------------------
    hipStream_t st = plan->stream;
    const bool ragged = (ends == starts + 1);
    long long h_stats[TSFA_LEN_STATS];
    if (host_len_stats(starts, ends, n_series, h_stats))
        return fail(TSFA_ERR_INVALID, "a series ends before it starts (offsets must be non-decreasing)");
    {
        BatchShape whole;
        shape_from_stats(h_stats, n_series, whole, plan->opt.length_classes);
        const int rc = check_shape(plan, whole);
        if (rc) return rc;
    }
    int64_t base = starts[0], top = ends[0];
    if (ragged) {
        base = starts[0];
        top = starts[n_series];
    } else {
        for (int64_t i = 0; i < n_series; ++i) {
            base = std::min(base, starts[i]);
            top = std::max(top, ends[i]);
        }
    }
    const int64_t total = top - base;
    std::vector<int64_t> &rel = plan->h_rel;
    if (ragged) {
        rel.resize((size_t)n_series + 1);
        for (int64_t i = 0; i <= n_series; ++i) rel[(size_t)i] = starts[i] - base;
    } else {
        rel.resize(2 * (size_t)n_series);
        for (int64_t i = 0; i < n_series; ++i) {
            rel[(size_t)i] = starts[i] - base;
            rel[(size_t)(n_series + i)] = ends[i] - base;
        }
    }
    if (plan->values.ensure((size_t)total * esz + 16) || plan->offsets.ensure(rel.size() * sizeof(int64_t)) ||
        plan->out.ensure((size_t)n_series * plan->n_cols * sizeof(double)) ||
        plan->sel.ensure((size_t)n_series * sizeof(int)))
        return fail(TSFA_ERR_HIP, "hipMalloc failed for the staging buffers");
    const double *d_times = nullptr;
    if (plan->needs_times) {
        if (plan->times.ensure((size_t)total * sizeof(double) + 16)) return fail(TSFA_ERR_HIP, "hipMalloc failed for the times buffer");
        d_times = (const double *)plan->times.p;
    }
    const int64_t *d_starts = (const int64_t *)plan->offsets.p;
    const int64_t *d_ends = d_starts + (ragged ? 1 : n_series);
    double *d_out = (double *)plan->out.p;
    const int64_t ld = plan->n_cols;

    const int n_chunks = host_chunk_count(plan, n_series);

    HIP_TRY(hipMemcpyAsync(plan->offsets.p, rel.data(), rel.size() * sizeof(int64_t), hipMemcpyHostToDevice, plan->s_in));
    if (!ragged || n_chunks == 1) {
        // window views may interleave: the touched span goes up in one piece
        HIP_TRY(hipMemcpyAsync(plan->values.p, (const char *)values + (size_t)base * esz, (size_t)total * esz,
                               hipMemcpyHostToDevice, plan->s_in));
        if (d_times)
            HIP_TRY(hipMemcpyAsync(plan->times.p, times + base, (size_t)total * sizeof(double), hipMemcpyHostToDevice, plan->s_in));
    }
    int rc = TSFA_OK;
    for (int c = 0; c < n_chunks && rc == TSFA_OK; ++c) {
        const int64_t c0 = n_series * c / n_chunks, c1 = n_series * (c + 1) / n_chunks;
        if (ragged && n_chunks > 1) {
            const int64_t v0 = rel[(size_t)c0], v1 = rel[(size_t)c1];
            HIP_TRY(hipMemcpyAsync((char *)plan->values.p + (size_t)v0 * esz, (const char *)values + (size_t)(base + v0) * esz,
                                   (size_t)(v1 - v0) * esz, hipMemcpyHostToDevice, plan->s_in));
            if (d_times)
                HIP_TRY(hipMemcpyAsync((char *)plan->times.p + (size_t)v0 * 8, times + base + v0, (size_t)(v1 - v0) * 8,
                                       hipMemcpyHostToDevice, plan->s_in));
        }
        HIP_TRY(hipEventRecord(plan->ev_in[c], plan->s_in));
        HIP_TRY(hipStreamWaitEvent(st, plan->ev_in[c], 0));
        // length classes of this chunk, from the host-side offsets (no device scan, no sync)
        long long cs[TSFA_LEN_STATS];
        host_len_stats(starts + c0, ends + c0, c1 - c0, cs);
        BatchShape sh;
        shape_from_stats(cs, c1 - c0, sh, plan->opt.length_classes);
        int *d_sel = (int *)plan->sel.p + c0;
        if ((rc = build_sel(plan, d_starts + c0, d_ends + c0, c1 - c0, sh, d_sel, st))) break;
        if ((rc = run_batch(plan, plan->values.p, dtype, d_times, d_starts + c0, d_ends + c0, c1 - c0, d_out + c0 * ld, ld,
                            sh, d_sel, st, n_chunks == 1)))
            break;
        HIP_TRY(hipEventRecord(plan->ev_k[c], st));
        HIP_TRY(hipStreamWaitEvent(plan->s_out, plan->ev_k[c], 0));
        HIP_TRY(hipMemcpy2DAsync(out + c0 * ld_out, (size_t)ld_out * sizeof(double), d_out + c0 * ld, (size_t)ld * sizeof(double),
                                 (size_t)plan->n_cols * sizeof(double), (size_t)(c1 - c0), hipMemcpyDeviceToHost, plan->s_out));
    }
    // drain all three streams even on an error: the caller's buffers must not be in flight when we return
    const hipError_t e1 = hipStreamSynchronize(plan->s_in), e2 = hipStreamSynchronize(st), e3 = hipStreamSynchronize(plan->s_out);
    if (rc) return rc;
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess)
        return fail(TSFA_ERR_HIP, std::string("stream synchronize: ") + hipGetErrorString(e1 != hipSuccess ? e1 : (e2 != hipSuccess ? e2 : e3)));
    if (plan->profiling)
        for (auto &t : plan->timings) (void)hipEventElapsedTime(&t.ms, t.e0, t.e1);
    return TSFA_OK;
}

int tsfa_host_alloc(void **ptr, size_t bytes) {
    if (!ptr) return fail(TSFA_ERR_INVALID, "ptr is NULL");
    *ptr = nullptr;
    if (tsfa_device_count() <= 0) return fail(TSFA_ERR_NO_DEVICE, "no HIP device visible");
    HIP_TRY(hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocDefault));
    return TSFA_OK;
}

int tsfa_host_free(void *ptr) {
    if (!ptr) return TSFA_OK;
    HIP_TRY(hipHostFree(ptr));
    return TSFA_OK;
}

}  // extern "C"
