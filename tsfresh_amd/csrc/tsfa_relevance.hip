// Relevance statistics for feature selection: for every column of the extracted feature matrix the
// sufficient statistics of the reference's univariate tests against a class-coded target
//   tsfresh/feature_selection/significance_tests.py:84  target_binary_feature_real_test   (Mann-Whitney U: rank sums
//                                                        with mid-ranks + the tie term of the normal approximation)
//   tsfresh/feature_selection/significance_tests.py:43  target_binary_feature_binary_test (Fisher: 2 x 2 counts)
//   tsfresh/feature_selection/relevance.py:396          get_feature_type                  (1 / 2 / more distinct values)
// in ONE batched sweep: a workgroup owns a column, sorts its (value, row) pairs in HBM scratch (bitonic network:
// 4096-element tiles finished in LDS, only the strides >= 4096 as global passes), then ranks them (ties found by
// binary search in the sorted column) and accumulates rank sums / counts per class with LDS atomics.  The sums are
// exact (mid-ranks are multiples of 0.5, totals < 2^53), so the order of the atomics does not matter.
// The p-value tails are the host's for the frame entry points (tsfresh_amd/feature_selection/significance_tests.py) and
// device code for the tensor entry points (rel_tails.h, tsfa_relevance_tails_* below).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../include/tsfresh_amd.h"
#include "rel_tails.h"
#include "rel_ks.h"
#include "tsfa_devmem.h"

#define REL_NT 1024
#define REL_TILE 4096
#define REL_MAXC 256

__global__ void __launch_bounds__(REL_NT) k_rel_stage(const double *__restrict__ X, int64_t n, int64_t ld, int64_t c0,
                                                       double *__restrict__ keys, uint32_t *__restrict__ idx, int64_t np2) {
    const int64_t c = blockIdx.x;
    double *K = keys + c * np2;
    uint32_t *I = idx + c * np2;
    const double *col = X + c0 + c;
    for (int64_t r = threadIdx.x; r < np2; r += REL_NT) {
        K[r] = (r < n) ? col[r * ld] : __builtin_inf();
        I[r] = (uint32_t)r;
    }
}

// compare-exchange stages j = jmax, jmax/2, .. 1 of merge level k on one LDS tile whose first element has global index base
__device__ __forceinline__ void rel_lds_stages(double *sk, uint32_t *si, int tile, int64_t base, int64_t k, int jmax) {
    for (int j = jmax; j > 0; j >>= 1) {
        __syncthreads();
        for (int t = threadIdx.x; t < (tile >> 1); t += REL_NT) {
            const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
            const int l = i | j;
            const bool up = (((base + i) & k) == 0);
            const double a = sk[i], b = sk[l];
            const uint32_t ia = si[i], ib = si[l];
            // ties by row: a total order, so the +inf pads (rows >= n) stay behind real +inf values
            if (((a > b) || (a == b && ia > ib)) == up) {
                sk[i] = b; sk[l] = a;
                si[i] = ib; si[l] = ia;
            }
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(REL_NT) k_rel_sort(double *__restrict__ keys, uint32_t *__restrict__ idx, int64_t np2, int tile) {
    extern __shared__ unsigned char rel_smem[];
    double *sk = (double *)rel_smem;
    uint32_t *si = (uint32_t *)(rel_smem + (size_t)tile * sizeof(double));
    double *K = keys + (int64_t)blockIdx.x * np2;
    uint32_t *I = idx + (int64_t)blockIdx.x * np2;
    // phase A: every tile fully sorted in LDS (direction from the element's global index, as the network requires)
    for (int64_t base = 0; base < np2; base += tile) {
        for (int t = threadIdx.x; t < tile; t += REL_NT) { sk[t] = K[base + t]; si[t] = I[base + t]; }
        for (int64_t k = 2; k <= tile; k <<= 1) rel_lds_stages(sk, si, tile, base, k, (int)(k >> 1));
        for (int t = threadIdx.x; t < tile; t += REL_NT) { K[base + t] = sk[t]; I[base + t] = si[t]; }
        __syncthreads();
    }
    // phase B: merge levels above the tile size: strides >= tile in HBM (L2-resident), the rest of the level in LDS
    for (int64_t k = 2 * (int64_t)tile; k <= np2; k <<= 1) {
        for (int64_t j = k >> 1; j >= tile; j >>= 1) {
            __syncthreads();
            for (int64_t t = threadIdx.x; t < (np2 >> 1); t += REL_NT) {
                const int64_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int64_t l = i | j;
                const bool up = ((i & k) == 0);
                const double a = K[i], b = K[l];
                const uint32_t ia = I[i], ib = I[l];
                if (((a > b) || (a == b && ia > ib)) == up) {
                    K[i] = b; K[l] = a;
                    I[i] = ib; I[l] = ia;
                }
            }
        }
        __syncthreads();
        for (int64_t base = 0; base < np2; base += tile) {
            for (int t = threadIdx.x; t < tile; t += REL_NT) { sk[t] = K[base + t]; si[t] = I[base + t]; }
            rel_lds_stages(sk, si, tile, base, k, tile >> 1);
            for (int t = threadIdx.x; t < tile; t += REL_NT) { K[base + t] = sk[t]; I[base + t] = si[t]; }
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(REL_NT) k_rel_stats(const double *__restrict__ keys, const uint32_t *__restrict__ idx, int64_t np2, int64_t n,
                                                       const int32_t *__restrict__ y, int n_classes, int64_t c0,
                                                       tsfa_relevance_col *__restrict__ cols, double *__restrict__ rank_sums,
                                                       int64_t *__restrict__ hi_counts) {
    __shared__ double s_rs[REL_MAXC];
    __shared__ unsigned long long s_hc[REL_MAXC];
    __shared__ double s_tie;
    __shared__ unsigned long long s_uniq;
    const double *K = keys + (int64_t)blockIdx.x * np2;
    const uint32_t *I = idx + (int64_t)blockIdx.x * np2;
    for (int k = threadIdx.x; k < REL_MAXC; k += REL_NT) { s_rs[k] = 0.0; s_hc[k] = 0ull; }
    if (threadIdx.x == 0) { s_tie = 0.0; s_uniq = 0ull; }
    __syncthreads();
    const double vhi = K[n - 1];
    double tie = 0.0;
    unsigned long long uniq = 0ull;
    for (int64_t i = threadIdx.x; i < n; i += REL_NT) {
        const double key = K[i];
        const bool start = (i == 0) || (K[i - 1] != key);
        const bool end = (i == n - 1) || (K[i + 1] != key);
        int64_t lb = i, ub = i + 1;
        if (!start) {  // first position of the tie group
            int64_t lo = 0, hi = i;
            while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (K[mid] < key) lo = mid + 1; else hi = mid; }
            lb = lo;
        }
        if (!end) {    // one past its last position
            int64_t lo = i + 1, hi = n;
            while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (K[mid] <= key) lo = mid + 1; else hi = mid; }
            ub = lo;
        }
        const double midrank = 0.5 * (double)(lb + ub + 1);  // mean of the 1-based ranks lb + 1 .. ub
        if (start) {
            const double t = (double)(ub - lb);
            tie += t * t * t - t;
            ++uniq;
        }
        const int cls = y[I[i]];
        atomicAdd(&s_rs[cls], midrank);
        if (key == vhi) atomicAdd(&s_hc[cls], 1ull);
    }
    atomicAdd(&s_tie, tie);
    atomicAdd(&s_uniq, uniq);
    __syncthreads();
    const int64_t c = c0 + blockIdx.x;
    for (int k = threadIdx.x; k < n_classes; k += REL_NT) {
        rank_sums[c * n_classes + k] = s_rs[k];
        hi_counts[c * n_classes + k] = (int64_t)s_hc[k];
    }
    if (threadIdx.x == 0) {
        cols[c].n_unique = (int64_t)s_uniq;
        cols[c].v_lo = K[0];
        cols[c].v_hi = vhi;
        cols[c].tie_term = s_tie;
    }
}

// The two-sample Kolmogorov-Smirnov walk of both KS kernels below, by one workgroup over positions 0 .. n - 1 of an
// ordered sample: hit(p) says whether position p belongs to the first sample, end(p) whether a tie group ends at p.
// Per-thread chunk counts, their exclusive scan (thread 0, serially), then k1 / n1 - (p + 1 - k1) / n0 at every group
// end -- searchsorted(side="right") / n, as scipy -- and the min / max reduction (thread 0, serially).  The order of
// these operations is the result's bits: do not reorder.  Every thread of the workgroup calls it (the leading barrier lets
// a caller loop over it).  Returns the hit total in *total -- the word it is broadcast through, in LDS or in the column's
// record -- and, on thread 0, the distance.
template <class Hit, class End>
__device__ __forceinline__ double rel_ks_walk(int64_t n, Hit hit, End end, long long *s_cnt, double *s_max, double *s_min,
                                              int64_t *total) {
    const int64_t chunk = (n + REL_NT - 1) / REL_NT;
    const int64_t p0 = (int64_t)threadIdx.x * chunk, p1 = (p0 + chunk < n) ? p0 + chunk : n;
    long long c = 0;
    for (int64_t p = p0; p < p1; ++p) c += hit(p) ? 1 : 0;
    __syncthreads();
    s_cnt[threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long acc = 0;
        for (int t = 0; t < REL_NT; ++t) { const long long v = s_cnt[t]; s_cnt[t] = acc; acc += v; }
        *total = acc;
    }
    __syncthreads();
    const double n1 = (double)*total, n0 = (double)(n - *total);
    long long k1 = s_cnt[threadIdx.x];
    double mx = -__builtin_inf(), mn = __builtin_inf();
    for (int64_t p = p0; p < p1; ++p) {
        k1 += hit(p) ? 1 : 0;
        if (end(p)) {
            const double d = (double)k1 / n1 - (double)(p + 1 - k1) / n0;
            mx = fmax(mx, d);
            mn = fmin(mn, d);
        }
    }
    s_max[threadIdx.x] = mx; s_min[threadIdx.x] = mn;
    __syncthreads();
    if (threadIdx.x != 0) return 0.0;
    for (int t = 1; t < REL_NT; ++t) { mx = fmax(mx, s_max[t]); mn = fmin(mn, s_min[t]); }
    double mins = -mn;
    mins = (mins < 0.0) ? 0.0 : ((mins > 1.0) ? 1.0 : mins);
    return (mins > mx) ? mins : mx;
}

// 'smir' option (significance_tests.py:121: scipy.stats.ks_2samp(x[y == label], x[y != label])): the Kolmogorov-Smirnov
// distance of the column split by each class label, walked along the sorted column (evaluated where a tie group of the
// column ends).
__global__ void __launch_bounds__(REL_NT) k_rel_ks_classes(const double *__restrict__ keys, const uint32_t *__restrict__ idx, int64_t np2, int64_t n,
                                                            const int32_t *__restrict__ y, int n_classes, int64_t c0,
                                                            double *__restrict__ ks_d) {
    __shared__ long long s_cnt[REL_NT];
    __shared__ double s_max[REL_NT], s_min[REL_NT];
    __shared__ int64_t s_total;
    const double *K = keys + (int64_t)blockIdx.x * np2;
    const uint32_t *I = idx + (int64_t)blockIdx.x * np2;
    for (int k = 0; k < n_classes; ++k) {
        const double d = rel_ks_walk(
            n, [&](int64_t p) { return y[I[p]] == k; }, [&](int64_t p) { return p == n - 1 || K[p + 1] != K[p]; }, s_cnt, s_max, s_min,
            &s_total);
        if (threadIdx.x == 0) ks_d[(c0 + blockIdx.x) * n_classes + k] = d;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Real-valued targets (significance_tests.py:170 target_real_feature_real_test = scipy.stats.kendalltau, :135
// target_real_feature_binary_test = scipy.stats.ks_2samp).  The column is sorted by (value, dense rank of y) -- the
// payload of the sort is the y rank instead of the row -- which is the order scipy's kendalltau establishes; then
//   k_rel_xties       tie statistics of x and of the (x, y) pairs (group ends by binary search),
//   k_rel_inversions  discordant pairs = strict inversions of the y-rank sequence: bottom-up merge sort, runs up to 4096
//                     in LDS (rank of every element in the sibling run by binary search), longer runs by merge-path
//                     segments in HBM scratch (each thread merges one contiguous output segment and counts, for every
//                     element taken from the right run, the left elements still waiting),
//   k_rel_ks          for two-valued columns: the two-sample Kolmogorov-Smirnov distance of y split by the column,
//                     walked in y order (prefix counts by a block scan, evaluated where a y tie group ends).
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(REL_NT) k_rel_stage_real(const double *__restrict__ X, int64_t n, int64_t ld, int64_t c0,
                                                            const int32_t *__restrict__ yrank, double *__restrict__ keys,
                                                            uint32_t *__restrict__ idx, int64_t np2) {
    const int64_t c = blockIdx.x;
    double *K = keys + c * np2;
    uint32_t *I = idx + c * np2;
    const double *col = X + c0 + c;
    for (int64_t r = threadIdx.x; r < np2; r += REL_NT) {
        K[r] = (r < n) ? col[r * ld] : __builtin_inf();
        I[r] = (r < n) ? (uint32_t)yrank[r] : 0xFFFFFFFFu;
    }
}

__global__ void __launch_bounds__(REL_NT) k_rel_xties(const double *__restrict__ keys, const uint32_t *__restrict__ idx, int64_t np2, int64_t n,
                                                       int64_t c0, tsfa_relevance_real_col *__restrict__ cols) {
    __shared__ unsigned long long s_xtie, s_ntie, s_uniq;
    __shared__ double s_x0, s_x1;
    const double *K = keys + (int64_t)blockIdx.x * np2;
    const uint32_t *I = idx + (int64_t)blockIdx.x * np2;
    if (threadIdx.x == 0) { s_xtie = 0ull; s_ntie = 0ull; s_uniq = 0ull; s_x0 = 0.0; s_x1 = 0.0; }
    __syncthreads();
    unsigned long long xtie = 0ull, ntie = 0ull, uniq = 0ull;
    double x0 = 0.0, x1 = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += REL_NT) {
        const double key = K[i];
        const uint32_t yr = I[i];
        const bool xstart = (i == 0) || (K[i - 1] != key);
        const bool jstart = xstart || (I[i - 1] != yr);
        if (xstart) {
            ++uniq;
            if (i + 1 < n && K[i + 1] == key) {  // a tie group of x starts here: its end by binary search
                int64_t lo = i + 1, hi = n;
                while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (K[mid] <= key) lo = mid + 1; else hi = mid; }
                const unsigned long long t = (unsigned long long)(lo - i);
                xtie += t * (t - 1ull) / 2ull;
                const double td = (double)t;
                x0 += td * (td - 1.0) * (td - 2.0);
                x1 += td * (td - 1.0) * (2.0 * td + 5.0);
            }
        }
        if (jstart && i + 1 < n && K[i + 1] == key && I[i + 1] == yr) {  // joint tie group of (x, y)
            int64_t lo = i + 1, hi = n;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                const double km = K[mid];
                if (km < key || (km == key && I[mid] <= yr)) lo = mid + 1; else hi = mid;
            }
            const unsigned long long t = (unsigned long long)(lo - i);
            ntie += t * (t - 1ull) / 2ull;
        }
    }
    atomicAdd(&s_xtie, xtie); atomicAdd(&s_ntie, ntie); atomicAdd(&s_uniq, uniq);
    atomicAdd(&s_x0, x0); atomicAdd(&s_x1, x1);
    __syncthreads();
    if (threadIdx.x == 0) {
        tsfa_relevance_real_col &o = cols[c0 + blockIdx.x];
        o.n_unique = (int64_t)s_uniq;
        o.v_lo = K[0];
        o.v_hi = K[n - 1];
        o.xtie = (int64_t)s_xtie;
        o.ntie = (int64_t)s_ntie;
        o.x0 = s_x0;
        o.x1 = s_x1;
        o.dis = 0;
        o.n_hi = 0;
        o.ks_d = 0.0;
    }
}

// strict inversions of seq[0 .. np2) (padded with 0xFFFFFFFF); tmp: a second buffer of np2 words; both are clobbered
__global__ void __launch_bounds__(REL_NT) k_rel_inversions(uint32_t *__restrict__ idx, uint32_t *__restrict__ tmpbuf, int64_t np2, int tile,
                                                            int64_t c0, tsfa_relevance_real_col *__restrict__ cols) {
    extern __shared__ unsigned char rel_smem[];
    uint32_t *sa = (uint32_t *)rel_smem, *sb = sa + tile;
    __shared__ unsigned long long s_inv;
    uint32_t *A = idx + (int64_t)blockIdx.x * np2;
    uint32_t *B = tmpbuf + (int64_t)blockIdx.x * np2;
    if (threadIdx.x == 0) s_inv = 0ull;
    unsigned long long inv = 0ull;
    for (int64_t base = 0; base < np2; base += tile) {
        __syncthreads();
        for (int t = threadIdx.x; t < tile; t += REL_NT) sa[t] = A[base + t];
        uint32_t *src = sa, *dst = sb;
        for (int run = 1; run < tile; run <<= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < tile; t += REL_NT) {
                const int off = t & (2 * run - 1), lbase = t - off, rbase = lbase + run;
                const uint32_t v = src[t];
                int pos;
                if (off < run) {  // left run: elements of the right run that are smaller go first
                    int lo = 0, hi = run;
                    while (lo < hi) { const int mid = (lo + hi) >> 1; if (src[rbase + mid] < v) lo = mid + 1; else hi = mid; }
                    pos = off + lo;
                } else {          // right run: elements of the left run that are <= v go first; the others are inversions
                    int lo = 0, hi = run;
                    while (lo < hi) { const int mid = (lo + hi) >> 1; if (src[lbase + mid] <= v) lo = mid + 1; else hi = mid; }
                    pos = (off - run) + lo;
                    inv += (unsigned long long)(run - lo);
                }
                dst[lbase + pos] = v;
            }
            uint32_t *sw = src; src = dst; dst = sw;
        }
        __syncthreads();
        for (int t = threadIdx.x; t < tile; t += REL_NT) A[base + t] = src[t];
    }
    // merge levels above the tile: one contiguous output segment per thread (merge path), ping-pong A <-> B
    const int64_t seg = np2 / REL_NT;  // np2 >= 2048: >= 2
    uint32_t *src = A, *dst = B;
    for (int64_t run = tile; run < np2; run <<= 1) {
        __syncthreads();
        const int64_t o0 = (int64_t)threadIdx.x * seg;
        const int64_t pbase = o0 & ~(2 * run - 1), diag = o0 - pbase;
        const uint32_t *L = src + pbase, *R = src + pbase + run;
        int64_t lo = (diag > run) ? diag - run : 0, hi = (diag < run) ? diag : run;
        while (lo < hi) {  // smallest li with L[li] > R[diag - li - 1]  (ties: the left element goes first)
            const int64_t mid = (lo + hi) >> 1;
            if (L[mid] <= R[diag - mid - 1]) lo = mid + 1; else hi = mid;
        }
        int64_t li = lo, ri = diag - lo;
        for (int64_t k = 0; k < seg; ++k) {
            const bool take_left = (li < run) && (ri >= run || L[li] <= R[ri]);
            if (take_left) { dst[o0 + k] = L[li]; ++li; }
            else { dst[o0 + k] = R[ri]; ++ri; inv += (unsigned long long)(run - li); }
        }
        uint32_t *sw = src; src = dst; dst = sw;
    }
    atomicAdd(&s_inv, inv);
    __syncthreads();
    if (threadIdx.x == 0) cols[c0 + blockIdx.x].dis = (int64_t)s_inv;
}

// two-valued columns: sup |F_hi - F_lo| of y over the rows with the larger / the smaller value of the column
__global__ void __launch_bounds__(REL_NT) k_rel_ks(const double *__restrict__ X, int64_t n, int64_t ld, const int32_t *__restrict__ yperm,
                                                    const unsigned char *__restrict__ yend, tsfa_relevance_real_col *__restrict__ cols) {
    __shared__ long long s_cnt[REL_NT];
    __shared__ double s_max[REL_NT], s_min[REL_NT];
    tsfa_relevance_real_col &o = cols[blockIdx.x];
    if (o.n_unique != 2) return;
    const double vhi = o.v_hi;
    const double *col = X + blockIdx.x;
    const double d = rel_ks_walk(
        n, [&](int64_t p) { return col[(int64_t)yperm[p] * ld] == vhi; }, [&](int64_t p) { return yend[p] != 0; }, s_cnt, s_max, s_min,
        &o.n_hi);
    if (threadIdx.x == 0) o.ks_d = d;
}

// ---------------------------------------------------------------------------------------------------------------------
// What every host driver below starts with: the device check, the staged input matrix, the column sorter.
// ---------------------------------------------------------------------------------------------------------------------
#define REL_NO_CPU_PATH " (there is no CPU path)"   // the note of the entry points that compute on the device

static int rel_check_device(int32_t device, const char *who, const char *note = "") {
    return tsfa_check_device(who, device, note);
}

// The n_rows x n_cols input matrix as the kernels read it: the caller's pointer and leading dimension (TSFA_DEVICE), or
// a device copy that this object owns (TSFA_HOST).  A host matrix may be a row-strided VIEW (ld > n_cols) that ends with
// its last row: only the n_cols-wide rows are the caller's -- the device copy is dense (leading dimension n_cols) and
// the columns between the rows are never read nor written back.
struct RelMatrix {
    const double *X = nullptr;
    int64_t ld = 0;
    DevPtr<double> own;

    int stage(const double *Xc, int64_t n_rows, int64_t n_cols, int64_t ldc, int32_t space) {
        X = Xc;
        ld = ldc;
        if (space != TSFA_HOST) return TSFA_OK;
        HIP_TRY_MALLOC(own, (size_t)n_rows * n_cols * sizeof(double));
        HIP_TRY(hipMemcpy2D(own.get(), (size_t)n_cols * sizeof(double), Xc, (size_t)ldc * sizeof(double), (size_t)n_cols * sizeof(double),
                            (size_t)n_rows, hipMemcpyHostToDevice));
        X = own.get();
        ld = n_cols;
        return TSFA_OK;
    }
    // the owned copy back into the host matrix it was staged from (tsfa_impute); nothing to do for a device matrix
    int write_back(double *Xc, int64_t n_rows, int64_t n_cols, int64_t ldc) const {
        if (!own) return TSFA_OK;
        HIP_TRY(hipMemcpy2D(Xc, (size_t)ldc * sizeof(double), own.get(), (size_t)n_cols * sizeof(double), (size_t)n_cols * sizeof(double),
                            (size_t)n_rows, hipMemcpyDeviceToHost));
        return TSFA_OK;
    }
};

int64_t tsfa_relevance_batch_override();

// The staged HBM sort of n_columns key columns of n_keys keys each, in batches of columns: the geometry k_rel_sort and the
// kernels behind it are launched with, and the (key, payload) scratch of one batch.
struct RelSorter {
    int64_t np2 = 0, batch = 0;
    int tile = 0;
    size_t lds = 0;   // dynamic LDS of k_rel_sort: one tile of keys and payloads
    DevPtr<double> keys;
    DevPtr<uint32_t> idx;

    // n_keys < 2^31 (every caller has refused more): the payload is 32 bits wide
    int init(int64_t n_keys, int64_t n_columns) {
        // np2: a power of two >= 2048 = 2 * REL_NT, so that k_rel_inversions' seg = np2 / REL_NT is >= 2
        static_assert(2048 >= 2 * REL_NT && (REL_TILE & (REL_TILE - 1)) == 0 && REL_TILE >= 2048, "sort geometry");
        np2 = 2048;
        while (np2 < n_keys) np2 <<= 1;
        // tile: a power of two that divides np2 (both are powers of two, tile <= np2), as k_rel_sort's phases need
        tile = (int)((np2 < REL_TILE) ? np2 : REL_TILE);
        // columns per batch: bound the scratch (12 B per padded key and column) to ~4 GB; tsfa_plan_set_option(NULL,
        // "relevance_batch", n) overrides (tests)
        batch = (int64_t)(4.0e9 / (12.0 * (double)np2));
        if (tsfa_relevance_batch_override() > 0) batch = tsfa_relevance_batch_override();
        if (batch < 1) batch = 1;
        if (batch > n_columns) batch = n_columns;
        lds = (size_t)tile * (sizeof(double) + sizeof(uint32_t));
        HIP_TRY_MALLOC(keys, (size_t)batch * np2 * sizeof(double));
        HIP_TRY_MALLOC(idx, (size_t)batch * np2 * sizeof(uint32_t));
        HIP_TRY(hipFuncSetAttribute((const void *)k_rel_sort, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        return TSFA_OK;
    }

    // per batch of nb columns from c0 on, on the null stream: stage(c0, nb) fills keys / idx (np2 entries per column),
    // k_rel_sort orders them, consume(c0, nb) reads the sorted columns.  The staging kernels stay apart on purpose
    // (k_rel_stage pads the payload with the row, k_rel_stage_real with 0xFFFFFFFF, k_imp_stage also counts the finite
    // cells): the tie-break of rel_lds_stages depends on those pads.
    template <class Stage, class Consume>
    int run(int64_t n_columns, Stage stage, Consume consume) const {
        for (int64_t c0 = 0; c0 < n_columns; c0 += batch) {
            const int64_t nb = (n_columns - c0 < batch) ? (n_columns - c0) : batch;
            stage(c0, nb);
            k_rel_sort<<<dim3((unsigned)nb), REL_NT, lds, 0>>>(keys.get(), idx.get(), np2, tile);
            consume(c0, nb);
            HIP_TRY(hipGetLastError());
        }
        return TSFA_OK;
    }
};

// The device side of one statistics sweep: what the sweep allocates, and what it leaves in HBM for the caller -- the
// host copies of tsfa_relevance_classes*, or the tails kernels of tsfa_relevance_tails_classes.
struct RelClassesDev {
    RelMatrix dX;
    RelSorter sort;
    DevPtr<double> drs, dks;
    DevPtr<int32_t> dy;
    DevPtr<int64_t> dhc;
    DevPtr<tsfa_relevance_col> dcols;
};

// validates, allocates and runs the sweep on the null stream; on return (any status) the caller owns `d`, and what the
// sweep allocated goes with it.  With TSFA_OK and n_cols > 0 the kernels are queued (not waited for) and d.dcols / d.drs /
// d.dhc (/ d.dks) will hold the statistics.
static int rel_classes_sweep(const double *X, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t space, const int32_t *y_codes,
                             int32_t n_classes, int32_t device, bool with_ks, RelClassesDev &d) {
    if (!X || !y_codes || n_rows < 1 || n_cols < 0 || ld < n_cols)
        return tsfa_fail(TSFA_ERR_INVALID, "tsfa_relevance_classes: null pointer or bad shape");
    if (n_classes < 1 || n_classes > REL_MAXC) return tsfa_fail(TSFA_ERR_UNSUPPORTED, "tsfa_relevance_classes: 1 .. 256 classes");
    if (n_rows >= (1ll << 31)) return tsfa_fail(TSFA_ERR_TOO_LONG, "tsfa_relevance_classes: more than 2^31 rows");
    for (int64_t r = 0; r < n_rows; ++r)
        if (y_codes[r] < 0 || y_codes[r] >= n_classes) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_relevance_classes: class code out of range");
    int rc = rel_check_device(device, "tsfa_relevance_classes", REL_NO_CPU_PATH);
    if (rc || n_cols == 0) return rc;
    HIP_TRY(hipSetDevice(device));
    if ((rc = d.dX.stage(X, n_rows, n_cols, ld, space))) return rc;
    if ((rc = d.sort.init(n_rows, n_cols))) return rc;
    HIP_TRY_MALLOC(d.dy, (size_t)n_rows * sizeof(int32_t));
    HIP_TRY_MALLOC(d.drs, (size_t)n_cols * n_classes * sizeof(double));
    HIP_TRY_MALLOC(d.dhc, (size_t)n_cols * n_classes * sizeof(int64_t));
    HIP_TRY_MALLOC(d.dcols, (size_t)n_cols * sizeof(tsfa_relevance_col));
    if (with_ks) HIP_TRY_MALLOC(d.dks, (size_t)n_cols * n_classes * sizeof(double));
    HIP_TRY(hipMemcpy(d.dy.get(), y_codes, (size_t)n_rows * sizeof(int32_t), hipMemcpyHostToDevice));
    const RelSorter &s = d.sort;
    return s.run(
        n_cols,
        [&](int64_t c0, int64_t nb) {
            k_rel_stage<<<dim3((unsigned)nb), REL_NT, 0, 0>>>(d.dX.X, n_rows, d.dX.ld, c0, s.keys.get(), s.idx.get(), s.np2);
        },
        [&](int64_t c0, int64_t nb) {
            k_rel_stats<<<dim3((unsigned)nb), REL_NT, 0, 0>>>(s.keys.get(), s.idx.get(), s.np2, n_rows, d.dy.get(), n_classes, c0,
                                                              d.dcols.get(), d.drs.get(), d.dhc.get());
            if (with_ks)
                k_rel_ks_classes<<<dim3((unsigned)nb), REL_NT, 0, 0>>>(s.keys.get(), s.idx.get(), s.np2, n_rows, d.dy.get(), n_classes, c0,
                                                                       d.dks.get());
        });
}

static int relevance_classes_impl(const double *X, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t space,
                                  const int32_t *y_codes, int32_t n_classes, int32_t device, tsfa_relevance_col *cols,
                                  double *rank_sums, int64_t *hi_counts, double *ks_d) {
    if (!cols || !rank_sums || !hi_counts) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_relevance_classes: null pointer or bad shape");
    RelClassesDev d;
    int rc = rel_classes_sweep(X, n_rows, n_cols, ld, space, y_codes, n_classes, device, ks_d != nullptr, d);
    if (rc != TSFA_OK || n_cols == 0) return rc;
    HIP_TRY(hipMemcpy(cols, d.dcols.get(), (size_t)n_cols * sizeof(tsfa_relevance_col), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(rank_sums, d.drs.get(), (size_t)n_cols * n_classes * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hi_counts, d.dhc.get(), (size_t)n_cols * n_classes * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (ks_d) HIP_TRY(hipMemcpy(ks_d, d.dks.get(), (size_t)n_cols * n_classes * sizeof(double), hipMemcpyDeviceToHost));
    return TSFA_OK;
}

extern "C" int tsfa_relevance_classes(const double *X, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t space,
                                      const int32_t *y_codes, int32_t n_classes, int32_t device, tsfa_relevance_col *cols,
                                      double *rank_sums, int64_t *hi_counts) {
    return relevance_classes_impl(X, n_rows, n_cols, ld, space, y_codes, n_classes, device, cols, rank_sums, hi_counts, nullptr);
}

extern "C" int tsfa_relevance_classes_ks(const double *X, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t space,
                                         const int32_t *y_codes, int32_t n_classes, int32_t device, tsfa_relevance_col *cols,
                                         double *rank_sums, int64_t *hi_counts, double *ks_d) {
    if (!ks_d) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_relevance_classes_ks: null ks_d");
    return relevance_classes_impl(X, n_rows, n_cols, ld, space, y_codes, n_classes, device, cols, rank_sums, hi_counts, ks_d);
}

// The device side of tsfa_relevance_real's sweep, as RelClassesDev
struct RelRealDev {
    RelMatrix dX;
    RelSorter sort;
    DevPtr<int32_t> dyr, dyp;
    DevPtr<unsigned char> dye;
    DevPtr<tsfa_relevance_real_col> dcols;
};

static int rel_real_sweep(const double *X, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t space, const int32_t *y_rank,
                          const int32_t *y_perm, const unsigned char *y_end, int32_t device, RelRealDev &d) {
    if (!X || !y_rank || !y_perm || !y_end || n_rows < 1 || n_cols < 0 || ld < n_cols)
        return tsfa_fail(TSFA_ERR_INVALID, "tsfa_relevance_real: null pointer or bad shape");
    if (n_rows >= (1ll << 31)) return tsfa_fail(TSFA_ERR_TOO_LONG, "tsfa_relevance_real: more than 2^31 rows");
    int rc = rel_check_device(device, "tsfa_relevance_real", REL_NO_CPU_PATH);
    if (rc || n_cols == 0) return rc;
    HIP_TRY(hipSetDevice(device));
    if ((rc = d.dX.stage(X, n_rows, n_cols, ld, space))) return rc;
    if ((rc = d.sort.init(n_rows, n_cols))) return rc;
    HIP_TRY_MALLOC(d.dyr, (size_t)n_rows * sizeof(int32_t));
    HIP_TRY_MALLOC(d.dyp, (size_t)n_rows * sizeof(int32_t));
    HIP_TRY_MALLOC(d.dye, (size_t)n_rows);
    HIP_TRY_MALLOC(d.dcols, (size_t)n_cols * sizeof(tsfa_relevance_real_col));
    HIP_TRY(hipMemcpy(d.dyr.get(), y_rank, (size_t)n_rows * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.dyp.get(), y_perm, (size_t)n_rows * sizeof(int32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.dye.get(), y_end, (size_t)n_rows, hipMemcpyHostToDevice));
    const RelSorter &s = d.sort;
    const size_t lds_inv = (size_t)s.tile * 2 * sizeof(uint32_t);
    HIP_TRY(hipFuncSetAttribute((const void *)k_rel_inversions, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_inv));
    rc = s.run(
        n_cols,
        [&](int64_t c0, int64_t nb) {
            k_rel_stage_real<<<dim3((unsigned)nb), REL_NT, 0, 0>>>(d.dX.X, n_rows, d.dX.ld, c0, d.dyr.get(), s.keys.get(), s.idx.get(), s.np2);
        },
        [&](int64_t c0, int64_t nb) {
            k_rel_xties<<<dim3((unsigned)nb), REL_NT, 0, 0>>>(s.keys.get(), s.idx.get(), s.np2, n_rows, c0, d.dcols.get());
            // the sorted values are dead now: their storage is the second buffer of the merge sort (np2 words per column
            // out of the np2 doubles)
            k_rel_inversions<<<dim3((unsigned)nb), REL_NT, lds_inv, 0>>>(s.idx.get(), (uint32_t *)s.keys.get(), s.np2, s.tile, c0, d.dcols.get());
        });
    if (rc) return rc;
    k_rel_ks<<<dim3((unsigned)n_cols), REL_NT, 0, 0>>>(d.dX.X, n_rows, d.dX.ld, d.dyp.get(), d.dye.get(), d.dcols.get());
    HIP_TRY(hipGetLastError());
    return TSFA_OK;
}

extern "C" int tsfa_relevance_real(const double *X, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t space,
                                   const int32_t *y_rank, const int32_t *y_perm, const unsigned char *y_end, int32_t device,
                                   tsfa_relevance_real_col *cols) {
    if (!cols) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_relevance_real: null pointer or bad shape");
    RelRealDev d;
    int rc = rel_real_sweep(X, n_rows, n_cols, ld, space, y_rank, y_perm, y_end, device, d);
    if (rc != TSFA_OK || n_cols == 0) return rc;
    HIP_TRY(hipMemcpy(cols, d.dcols.get(), (size_t)n_cols * sizeof(tsfa_relevance_real_col), hipMemcpyDeviceToHost));
    return TSFA_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// p-value tails, FDR step-up, mask compaction and the device gather (rel_tails.h): the decision of the selection -- a
// mask over the columns -- is taken where the statistics are, so the device-resident chain reads back the constant
// columns' names and one count.  A wavefront serves a Fisher cell, a lane every closed-form cell; the two host routes
// (exact Mann-Whitney, Kolmogorov-Smirnov) get NaN and are counted for the caller.
// ---------------------------------------------------------------------------------------------------------------------
#define RT_THREADS 256

// closed forms and routes of the class tables: thread = cell (column, class); also the column types
__global__ void __launch_bounds__(RT_THREADS) k_tails_classes(const tsfa_relevance_col *__restrict__ cols, const double *__restrict__ rank_sums,
                                                              const int64_t *__restrict__ class_n, int64_t n_rows, int64_t n_cols,
                                                              int n_classes, int with_ks, double *__restrict__ p,
                                                              unsigned char *__restrict__ route, unsigned char *__restrict__ type,
                                                              unsigned long long *__restrict__ n_host) {
    const int64_t cell = (int64_t)blockIdx.x * RT_THREADS + threadIdx.x;
    if (cell >= n_cols * n_classes) return;
    if (rt_tails_classes_cell(cols, rank_sums, class_n, n_rows, n_classes, with_ks, cell, p, route, type)) atomicAdd(n_host, 1ull);
}

// Fisher cells: wavefront = cell; cells of other routes leave at once (wave-uniform)
__global__ void __launch_bounds__(RT_THREADS) k_tails_fisher(const tsfa_relevance_col *__restrict__ cols, const int64_t *__restrict__ hi_counts,
                                                             const int64_t *__restrict__ class_n, int64_t n_rows, int64_t n_cols,
                                                             int n_classes, double *__restrict__ p) {
    const int64_t cell = (int64_t)blockIdx.x * (RT_THREADS / 64) + (threadIdx.x >> 6);
    if (cell >= n_cols * n_classes) return;
    rt_tails_fisher_cell(cols, hi_counts, class_n, n_rows, n_classes, cell, p);
}

__global__ void __launch_bounds__(RT_THREADS) k_tails_real(const tsfa_relevance_real_col *__restrict__ cols, int64_t n_rows, int64_t n_cols,
                                                           int64_t ytie, double y0, double y1, double *__restrict__ p,
                                                           unsigned char *__restrict__ route, unsigned char *__restrict__ type,
                                                           unsigned long long *__restrict__ n_host) {
    const int64_t c = (int64_t)blockIdx.x * RT_THREADS + threadIdx.x;
    if (c >= n_cols) return;
    if (rt_tails_real_cell(cols, n_rows, ytie, y0, y1, c, p, route, type)) atomicAdd(n_host, 1ull);
}

// ---- the exact Kolmogorov-Smirnov tail (rel_ks.h): the TSFA_ROUTE_HOST_KS cells of a table, where the device serves them ----
// closed forms (h == 0, the Horner form of n1 == n2): thread = cell.  cnt[0]: cells served, cnt[1] / cnt[2]: lattice cells
// whose ring fits the LDS slice / needs the scratch
__global__ void __launch_bounds__(RT_THREADS) k_ks_closed(RkCells s, int64_t n_cells, double *__restrict__ p, unsigned char *__restrict__ route,
                                                          unsigned long long *__restrict__ cnt) {
    const int64_t cell = (int64_t)blockIdx.x * RT_THREADS + threadIdx.x;
    if (cell >= n_cells) return;
    const int r = rk_closed_cell(s, cell, p, route);
    if (r != RK_CELL_NONE) atomicAdd(cnt + (r - 1), 1ull);
}

// lattice cells: wavefront = cell, in a grid-stride loop, so that the rings (LDS: 8 KB a wavefront; scratch: 128 KB a
// wavefront, null when no cell needs it) are sized by the launch and not by the table.  The wavefronts of a workgroup never
// meet: no barrier.
__global__ void __launch_bounds__(RT_THREADS) k_ks_lattice(RkCells s, int64_t n_cells, double *__restrict__ scratch, double *__restrict__ p,
                                                           unsigned char *__restrict__ route, unsigned long long *__restrict__ cnt) {
    __shared__ double rings[(RT_THREADS / 64) * RK_LDS_CHUNKS * 64];
    const int w = (int)(threadIdx.x >> 6);
    const int64_t wave = (int64_t)blockIdx.x * (RT_THREADS / 64) + w, n_waves = (int64_t)gridDim.x * (RT_THREADS / 64);
    double *lds = rings + w * (RK_LDS_CHUNKS * 64);
    double *hbm = scratch ? scratch + wave * (RK_HBM_CHUNKS * 64) : nullptr;
    for (int64_t cell = wave; cell < n_cells; cell += n_waves)
        if (rk_lattice_cell(s, cell, lds, hbm, p, route) == RK_CELL_SERVED && (threadIdx.x & 63) == 0) atomicAdd(cnt, 1ull);
}

__global__ void __launch_bounds__(RT_THREADS) k_ks_init(int64_t n_cells, double *__restrict__ p, unsigned char *__restrict__ route) {
    const int64_t cell = (int64_t)blockIdx.x * RT_THREADS + threadIdx.x;
    if (cell >= n_cells) return;
    p[cell] = RT_NAN;
    route[cell] = TSFA_ROUTE_HOST_KS;
}

// the real table's n_hi and ks_d, out of the sweep's records into the caller's device arrays
__global__ void __launch_bounds__(RT_THREADS) k_ks_handout_real(const tsfa_relevance_real_col *__restrict__ cols, int64_t n_cols,
                                                                int64_t *__restrict__ n_hi, double *__restrict__ ks_d) {
    const int64_t c = (int64_t)blockIdx.x * RT_THREADS + threadIdx.x;
    if (c >= n_cols) return;
    if (n_hi) n_hi[c] = cols[c].n_hi;
    if (ks_d) ks_d[c] = cols[c].ks_d;
}

#define RK_MAX_WORKGROUPS 512   // of 4 wavefronts: at most 256 MB of scratch, and only when a cell needs it

// The KS stage on the null stream of the current device: every TSFA_ROUTE_HOST_KS cell of route[n_cells] that rel_ks.h serves
// gets its p and TSFA_ROUTE_KS_EXACT.  Synchronous; *served: how many.
static int ks_tails_run(const RkCells &s, int64_t n_cells, double *p, unsigned char *route, int64_t *served) {
    *served = 0;
    if (n_cells == 0) return TSFA_OK;
    unsigned long long cnt[3] = {0ull, 0ull, 0ull};
    DevPtr<unsigned long long> dcnt;
    DevPtr<double> dscratch;
    HIP_TRY_MALLOC(dcnt, sizeof(cnt));
    HIP_TRY(hipMemset(dcnt.get(), 0, sizeof(cnt)));
    k_ks_closed<<<dim3((unsigned)((n_cells + RT_THREADS - 1) / RT_THREADS)), RT_THREADS, 0, 0>>>(s, n_cells, p, route, dcnt.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(cnt, dcnt.get(), sizeof(cnt), hipMemcpyDeviceToHost));
    if (cnt[1] + cnt[2] > 0) {
        int64_t nwg = (n_cells + RT_THREADS / 64 - 1) / (RT_THREADS / 64);
        if (nwg > RK_MAX_WORKGROUPS) nwg = RK_MAX_WORKGROUPS;
        if (cnt[2] > 0) HIP_TRY_MALLOC(dscratch, (size_t)nwg * (RT_THREADS / 64) * RK_HBM_CHUNKS * 64 * sizeof(double));
        k_ks_lattice<<<dim3((unsigned)nwg), RT_THREADS, 0, 0>>>(s, n_cells, dscratch.get(), p, route, dcnt.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(cnt, dcnt.get(), sizeof(cnt[0]), hipMemcpyDeviceToHost));
    }
    *served = (int64_t)cnt[0];
    return TSFA_OK;
}

extern "C" int tsfa_ks_tails(const int64_t *n1, const int64_t *n2, const double *d, int64_t n_cells, int32_t device, double *p,
                             unsigned char *route) {
    if (n_cells < 0 || (n_cells > 0 && (!n1 || !n2 || !d || !p || !route)))
        return tsfa_fail(TSFA_ERR_INVALID, "tsfa_ks_tails: null pointer or bad shape");
    int rc = rel_check_device(device, "tsfa_ks_tails");
    if (rc || n_cells == 0) return rc;
    HIP_TRY(hipSetDevice(device));
    k_ks_init<<<dim3((unsigned)((n_cells + RT_THREADS - 1) / RT_THREADS)), RT_THREADS, 0, 0>>>(n_cells, p, route);
    HIP_TRY(hipGetLastError());
    RkCells s = {};
    s.n1 = n1;
    s.n2 = n2;
    s.d = d;
    int64_t served = 0;
    rc = ks_tails_run(s, n_cells, p, route, &served);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return TSFA_OK;
}

static int ks_tail_check(int32_t ks_tail, const char *who) {
    if (ks_tail == TSFA_KS_TAIL_HOST || ks_tail == TSFA_KS_TAIL_DEVICE) return TSFA_OK;
    return tsfa_fail(TSFA_ERR_INVALID, (std::string(who) + ": ks_tail must be TSFA_KS_TAIL_HOST or TSFA_KS_TAIL_DEVICE").c_str());
}

static int relevance_tails_classes_impl(const double *X, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t space,
                                        const int32_t *y_codes, int32_t n_classes, int32_t with_ks, int32_t ks_tail, int32_t device,
                                        double *p, unsigned char *route, unsigned char *type, tsfa_relevance_col *cols,
                                        double *rank_sums, int64_t *hi_counts, double *ks_d, double *ks_d_device,
                                        int64_t *n_host_cells) {
    if (n_host_cells) *n_host_cells = 0;
    if (n_cols > 0 && (!p || !route || !type)) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_relevance_tails_classes: null output pointer");
    if ((ks_d || ks_d_device) && !with_ks) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_relevance_tails_classes: ks_d without with_ks");
    RelClassesDev d;
    unsigned long long nh = 0ull;
    std::vector<int64_t> class_n;
    int rc = rel_classes_sweep(X, n_rows, n_cols, ld, space, y_codes, n_classes, device, with_ks != 0, d);
    if (rc != TSFA_OK || n_cols == 0) return rc;
    class_n.assign((size_t)n_classes, 0);
    for (int64_t r = 0; r < n_rows; ++r) ++class_n[(size_t)y_codes[r]];
    DevPtr<int64_t> dcn;
    DevPtr<unsigned long long> dnh;
    HIP_TRY_MALLOC(dcn, (size_t)n_classes * sizeof(int64_t));
    HIP_TRY_MALLOC(dnh, sizeof(unsigned long long));
    HIP_TRY(hipMemcpy(dcn.get(), class_n.data(), (size_t)n_classes * sizeof(int64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(dnh.get(), 0, sizeof(unsigned long long)));
    const int64_t cells = n_cols * n_classes;
    {
        k_tails_classes<<<dim3((unsigned)((cells + RT_THREADS - 1) / RT_THREADS)), RT_THREADS, 0, 0>>>(
            d.dcols.get(), d.drs.get(), dcn.get(), n_rows, n_cols, n_classes, with_ks, p, route, type, dnh.get());
        HIP_TRY(hipGetLastError());
        k_tails_fisher<<<dim3((unsigned)((cells + RT_THREADS / 64 - 1) / (RT_THREADS / 64))), RT_THREADS, 0, 0>>>(
            d.dcols.get(), d.dhc.get(), dcn.get(), n_rows, n_cols, n_classes, p);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpy(&nh, dnh.get(), sizeof(nh), hipMemcpyDeviceToHost));
    if (with_ks && ks_tail == TSFA_KS_TAIL_DEVICE && nh > 0) {
        RkCells s = {};
        s.d = d.dks.get();
        s.class_n = dcn.get();
        s.n_rows = n_rows;
        s.n_classes = n_classes;
        int64_t served = 0;
        rc = ks_tails_run(s, cells, p, route, &served);
        if (rc) return rc;
        nh -= (unsigned long long)served;
    }
    if (n_host_cells) *n_host_cells = (int64_t)nh;
    if (cols) HIP_TRY(hipMemcpy(cols, d.dcols.get(), (size_t)n_cols * sizeof(tsfa_relevance_col), hipMemcpyDeviceToHost));
    if (rank_sums) HIP_TRY(hipMemcpy(rank_sums, d.drs.get(), (size_t)n_cols * n_classes * sizeof(double), hipMemcpyDeviceToHost));
    if (hi_counts) HIP_TRY(hipMemcpy(hi_counts, d.dhc.get(), (size_t)n_cols * n_classes * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (ks_d) HIP_TRY(hipMemcpy(ks_d, d.dks.get(), (size_t)n_cols * n_classes * sizeof(double), hipMemcpyDeviceToHost));
    if (ks_d_device) HIP_TRY(hipMemcpy(ks_d_device, d.dks.get(), (size_t)n_cols * n_classes * sizeof(double), hipMemcpyDeviceToDevice));
    return TSFA_OK;
}

extern "C" int tsfa_relevance_tails_classes(const double *X, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t space,
                                            const int32_t *y_codes, int32_t n_classes, int32_t with_ks, int32_t device, double *p,
                                            unsigned char *route, unsigned char *type, tsfa_relevance_col *cols, double *rank_sums,
                                            int64_t *hi_counts, double *ks_d, int64_t *n_host_cells) {
    return relevance_tails_classes_impl(X, n_rows, n_cols, ld, space, y_codes, n_classes, with_ks, TSFA_KS_TAIL_HOST, device, p, route,
                                        type, cols, rank_sums, hi_counts, ks_d, nullptr, n_host_cells);
}

extern "C" int tsfa_relevance_tails_classes_ks(const double *X, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t space,
                                               const int32_t *y_codes, int32_t n_classes, int32_t with_ks, int32_t ks_tail,
                                               int32_t device, double *p, unsigned char *route, unsigned char *type,
                                               tsfa_relevance_col *cols, double *rank_sums, int64_t *hi_counts, double *ks_d,
                                               double *ks_d_device, int64_t *n_host_cells) {
    if (n_host_cells) *n_host_cells = 0;
    if (int rc = ks_tail_check(ks_tail, "tsfa_relevance_tails_classes_ks")) return rc;
    return relevance_tails_classes_impl(X, n_rows, n_cols, ld, space, y_codes, n_classes, with_ks, ks_tail, device, p, route, type, cols,
                                        rank_sums, hi_counts, ks_d, ks_d_device, n_host_cells);
}

static int relevance_tails_real_impl(const double *X, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t space, const int32_t *y_rank,
                                     const int32_t *y_perm, const unsigned char *y_end, int64_t ytie, double y0, double y1,
                                     int32_t ks_tail, int32_t device, double *p, unsigned char *route, unsigned char *type,
                                     tsfa_relevance_real_col *cols, int64_t *n_hi_device, double *ks_d_device, int64_t *n_host_cells) {
    if (n_host_cells) *n_host_cells = 0;
    if (n_cols > 0 && (!p || !route || !type)) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_relevance_tails_real: null output pointer");
    RelRealDev d;
    unsigned long long nh = 0ull;
    int rc = rel_real_sweep(X, n_rows, n_cols, ld, space, y_rank, y_perm, y_end, device, d);
    if (rc != TSFA_OK || n_cols == 0) return rc;
    DevPtr<unsigned long long> dnh;
    HIP_TRY_MALLOC(dnh, sizeof(unsigned long long));
    HIP_TRY(hipMemset(dnh.get(), 0, sizeof(unsigned long long)));
    k_tails_real<<<dim3((unsigned)((n_cols + RT_THREADS - 1) / RT_THREADS)), RT_THREADS, 0, 0>>>(d.dcols.get(), n_rows, n_cols, ytie, y0, y1, p,
                                                                                              route, type, dnh.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(&nh, dnh.get(), sizeof(nh), hipMemcpyDeviceToHost));
    if (ks_tail == TSFA_KS_TAIL_DEVICE && nh > 0) {
        RkCells s = {};
        s.rcols = d.dcols.get();
        s.n_rows = n_rows;
        int64_t served = 0;
        rc = ks_tails_run(s, n_cols, p, route, &served);
        if (rc) return rc;
        nh -= (unsigned long long)served;
    }
    if (n_host_cells) *n_host_cells = (int64_t)nh;
    if (cols) HIP_TRY(hipMemcpy(cols, d.dcols.get(), (size_t)n_cols * sizeof(tsfa_relevance_real_col), hipMemcpyDeviceToHost));
    if (n_hi_device || ks_d_device) {
        k_ks_handout_real<<<dim3((unsigned)((n_cols + RT_THREADS - 1) / RT_THREADS)), RT_THREADS, 0, 0>>>(d.dcols.get(), n_cols, n_hi_device,
                                                                                                       ks_d_device);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
    }
    return TSFA_OK;
}

extern "C" int tsfa_relevance_tails_real(const double *X, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t space,
                                         const int32_t *y_rank, const int32_t *y_perm, const unsigned char *y_end, int64_t ytie,
                                         double y0, double y1, int32_t device, double *p, unsigned char *route, unsigned char *type,
                                         tsfa_relevance_real_col *cols, int64_t *n_host_cells) {
    return relevance_tails_real_impl(X, n_rows, n_cols, ld, space, y_rank, y_perm, y_end, ytie, y0, y1, TSFA_KS_TAIL_HOST, device, p, route,
                                     type, cols, nullptr, nullptr, n_host_cells);
}

extern "C" int tsfa_relevance_tails_real_ks(const double *X, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t space,
                                            const int32_t *y_rank, const int32_t *y_perm, const unsigned char *y_end, int64_t ytie,
                                            double y0, double y1, int32_t ks_tail, int32_t device, double *p, unsigned char *route,
                                            unsigned char *type, tsfa_relevance_real_col *cols, int64_t *n_hi_device,
                                            double *ks_d_device, int64_t *n_host_cells) {
    if (n_host_cells) *n_host_cells = 0;
    if (int rc = ks_tail_check(ks_tail, "tsfa_relevance_tails_real_ks")) return rc;
    return relevance_tails_real_impl(X, n_rows, n_cols, ld, space, y_rank, y_perm, y_end, ytie, y0, y1, ks_tail, device, p, route, type, cols,
                                     n_hi_device, ks_d_device, n_host_cells);
}

// masked sort keys of the p-value matrix (rt_fdr_key): what k_rel_stage / k_rel_sort then order, one key column per table
__global__ void __launch_bounds__(RT_THREADS) k_fdr_keys(const double *__restrict__ p, const unsigned char *__restrict__ type, int64_t n_cols,
                                                         int n_tables, double *__restrict__ keys) {
    const int64_t cell = (int64_t)blockIdx.x * RT_THREADS + threadIdx.x;
    if (cell >= n_cols * n_tables) return;
    keys[cell] = rt_fdr_key(p[cell], type[cell / n_tables]);
}

// one workgroup per sorted key column (table t0 + blockIdx.x): m = the columns that are not constant, the largest sorted
// position that meets its threshold, and the flag of every column of the table
__global__ void __launch_bounds__(REL_NT) k_fdr_stepup(const double *__restrict__ keys, const uint32_t *__restrict__ idx, int64_t np2,
                                                        const unsigned char *__restrict__ type, int64_t n_cols, int n_tables, int t0,
                                                        double alpha, double c_m, unsigned char *__restrict__ rel_t) {
    __shared__ unsigned long long s_m;
    __shared__ long long s_last;
    const double *K = keys + (int64_t)blockIdx.x * np2;
    const uint32_t *I = idx + (int64_t)blockIdx.x * np2;
    if (threadIdx.x == 0) { s_m = 0ull; s_last = -1ll; }
    __syncthreads();
    unsigned long long cnt = 0ull;
    for (int64_t c = threadIdx.x; c < n_cols; c += REL_NT) cnt += (type[c] != 0) ? 1ull : 0ull;
    atomicAdd(&s_m, cnt);
    __syncthreads();
    const int64_t m = (int64_t)s_m;
    long long last = -1ll;
    for (int64_t i = threadIdx.x; i < m; i += REL_NT)   // (positions m .. n_cols - 1 hold the constant columns' +inf)
        if (K[i] <= rt_fdr_threshold(i + 1, m, c_m, alpha)) last = i;
    atomicMax(&s_last, last);
    __syncthreads();
    last = s_last;
    for (int64_t i = threadIdx.x; i < n_cols; i += REL_NT) rel_t[(int64_t)I[i] * n_tables + t0 + blockIdx.x] = (i <= last) ? 1 : 0;
}

__global__ void __launch_bounds__(RT_THREADS) k_fdr_combine(const double *__restrict__ p, const unsigned char *__restrict__ rel_t,
                                                            const unsigned char *__restrict__ type, int64_t n_cols, int n_tables,
                                                            int multiclass, int n_significant, unsigned char *__restrict__ relevant,
                                                            int32_t *__restrict__ n_sig, double *__restrict__ p_min) {
    const int64_t c = (int64_t)blockIdx.x * RT_THREADS + threadIdx.x;
    if (c >= n_cols) return;
    rt_fdr_combine(p + c * n_tables, rel_t + c * n_tables, n_tables, type[c], multiclass, n_significant, relevant + c, n_sig + c, p_min + c);
}

extern "C" int tsfa_relevance_fdr(const double *p, const unsigned char *type, int64_t n_cols, int32_t n_tables, double alpha,
                                  double c_m, int32_t n_significant, int32_t multiclass, int32_t device,
                                  unsigned char *relevant_per_table, unsigned char *relevant, int32_t *n_significant_out,
                                  double *p_min) {
    if (n_cols < 0 || n_tables < 1 || n_tables > REL_MAXC || !(c_m > 0.0) ||
        (n_cols > 0 && (!p || !type || !relevant_per_table || !relevant || !n_significant_out || !p_min)))
        return tsfa_fail(TSFA_ERR_INVALID, "tsfa_relevance_fdr: null pointer, bad shape, more than 256 tables or c_m <= 0");
    if (n_cols >= (1ll << 31)) return tsfa_fail(TSFA_ERR_TOO_LONG, "tsfa_relevance_fdr: more than 2^31 columns");
    int rc = rel_check_device(device, "tsfa_relevance_fdr");
    if (rc || n_cols == 0) return rc;
    const int64_t cells = n_cols * n_tables;
    HIP_TRY(hipSetDevice(device));
    DevPtr<double> dmask;
    RelSorter s;
    HIP_TRY_MALLOC(dmask, (size_t)cells * sizeof(double));
    if ((rc = s.init(n_cols, n_tables))) return rc;
    k_fdr_keys<<<dim3((unsigned)((cells + RT_THREADS - 1) / RT_THREADS)), RT_THREADS, 0, 0>>>(p, type, n_cols, n_tables, dmask.get());
    HIP_TRY(hipGetLastError());
    // the key matrix is [n_cols, n_tables]: a table is a column of it, its rows are the feature columns
    rc = s.run(
        n_tables,
        [&](int64_t t0, int64_t nb) {
            k_rel_stage<<<dim3((unsigned)nb), REL_NT, 0, 0>>>(dmask.get(), n_cols, n_tables, t0, s.keys.get(), s.idx.get(), s.np2);
        },
        [&](int64_t t0, int64_t nb) {
            k_fdr_stepup<<<dim3((unsigned)nb), REL_NT, 0, 0>>>(s.keys.get(), s.idx.get(), s.np2, type, n_cols, n_tables, (int)t0, alpha, c_m,
                                                              relevant_per_table);
        });
    if (rc) return rc;
    k_fdr_combine<<<dim3((unsigned)((n_cols + RT_THREADS - 1) / RT_THREADS)), RT_THREADS, 0, 0>>>(
        p, relevant_per_table, type, n_cols, n_tables, multiclass, n_significant, relevant, n_significant_out, p_min);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return TSFA_OK;
}

// one workgroup: slice counts, their exclusive scan (thread 0, as the KS kernels above), the writes
__global__ void __launch_bounds__(REL_NT) k_compact_mask(const unsigned char *__restrict__ mask, int64_t n, int32_t *__restrict__ indices,
                                                          long long *__restrict__ count) {
    __shared__ int32_t s_cnt[REL_NT];
    s_cnt[threadIdx.x] = rt_compact_count(mask, n, (int)threadIdx.x, REL_NT);
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t acc = 0;
        for (int t = 0; t < REL_NT; ++t) { const int32_t v = s_cnt[t]; s_cnt[t] = acc; acc += v; }
        *count = acc;
    }
    __syncthreads();
    rt_compact_write(mask, n, (int)threadIdx.x, REL_NT, s_cnt[threadIdx.x], indices);
}

extern "C" int tsfa_compact_mask(const unsigned char *mask, int64_t n, int32_t *indices, int64_t *count, int32_t device) {
    if (!count || n < 0 || (n > 0 && (!mask || !indices))) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_compact_mask: null pointer or bad shape");
    *count = 0;
    if (n >= (1ll << 31)) return tsfa_fail(TSFA_ERR_TOO_LONG, "tsfa_compact_mask: more than 2^31 entries");
    int rc = rel_check_device(device, "tsfa_compact_mask");
    if (rc || n == 0) return rc;
    long long got = 0;
    HIP_TRY(hipSetDevice(device));
    DevPtr<long long> dcount;
    HIP_TRY_MALLOC(dcount, sizeof(long long));
    k_compact_mask<<<1, REL_NT, 0, 0>>>(mask, n, indices, dcount.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(&got, dcount.get(), sizeof(got), hipMemcpyDeviceToHost));
    *count = (int64_t)got;
    return TSFA_OK;
}

// k_gather_columns with the indices read from HBM, a leading dimension of the destination, and a flag for an index
// outside [0, ld) (nothing is read or written for it)
__global__ void __launch_bounds__(256) k_gather_columns_device(const double *__restrict__ X, int64_t n_rows, int64_t ld,
                                                                const int32_t *__restrict__ cols, int64_t n_sel,
                                                                double *__restrict__ out, int64_t ld_out, int *__restrict__ bad) {
    const int64_t total = n_rows * n_sel;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / n_sel, c = i - r * n_sel;
        const int32_t src = cols[c];
        if (src < 0 || src >= ld) { *bad = 1; continue; }
        out[r * ld_out + c] = X[r * ld + src];
    }
}

extern "C" int tsfa_gather_columns_device(const double *X, int64_t n_rows, int64_t ld, const int32_t *cols, int64_t n_sel,
                                          double *out, int64_t ld_out, int32_t device) {
    if (n_rows < 0 || n_sel < 0 || ld_out < n_sel || ((n_rows && n_sel) && (!X || !cols || !out)))
        return tsfa_fail(TSFA_ERR_INVALID, "tsfa_gather_columns_device: null pointer or bad shape");
    int rc = rel_check_device(device, "tsfa_gather_columns_device");
    if (rc || n_rows == 0 || n_sel == 0) return rc;
    int bad = 0;
    HIP_TRY(hipSetDevice(device));
    DevPtr<int> dbad;
    HIP_TRY_MALLOC(dbad, sizeof(int));
    HIP_TRY(hipMemset(dbad.get(), 0, sizeof(int)));
    k_gather_columns_device<<<2048, 256, 0, 0>>>(X, n_rows, ld, cols, n_sel, out, ld_out, dbad.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(&bad, dbad.get(), sizeof(int), hipMemcpyDeviceToHost));
    if (bad) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_gather_columns_device: column index out of range");
    return TSFA_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// impute (tsfresh/utilities/dataframe_functions.py:49-214): per column the largest / smallest / median FINITE value
// (get_range_values_per_column :142-180: np.ma.masked_invalid + np.max / np.min / np.ma.median; a column without any
// finite value counts as all zeros), then +inf -> max, -inf -> min, NaN -> median (impute_dataframe_range :96-139).
// The column statistics come from the same staged HBM sort as the relevance tests: non-finite cells are staged as +inf
// and therefore sort behind the `cnt` finite ones.
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(REL_NT) k_imp_stage(const double *__restrict__ X, int64_t n, int64_t ld, int64_t c0,
                                                       double *__restrict__ keys, uint32_t *__restrict__ idx, int64_t np2,
                                                       int *__restrict__ finite_cnt) {
    const int64_t c = blockIdx.x;
    double *K = keys + c * np2;
    uint32_t *I = idx + c * np2;
    const double *col = X + c0 + c;
    int cnt = 0;
    for (int64_t r = threadIdx.x; r < np2; r += REL_NT) {
        double v = __builtin_inf();
        if (r < n) {
            const double x = col[r * ld];
            if (x == x && x != __builtin_inf() && x != -__builtin_inf()) { v = x; ++cnt; }
        }
        K[r] = v;
        I[r] = (uint32_t)r;
    }
    __shared__ int red[REL_NT / 64];
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < REL_NT / 64; ++w) t += red[w];
        finite_cnt[c0 + c] = t;
    }
}

__global__ void k_imp_stats(const double *__restrict__ keys, int64_t np2, const int *__restrict__ finite_cnt, int64_t c0, int64_t nb,
                            double *__restrict__ cmax, double *__restrict__ cmin, double *__restrict__ cmed) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nb) return;
    const double *K = keys + c * np2;
    const int cnt = finite_cnt[c0 + c];
    double mx = 0.0, mn = 0.0, md = 0.0;
    if (cnt > 0) {
        mn = K[0];
        mx = K[cnt - 1];
        md = (cnt & 1) ? K[cnt / 2] : (K[cnt / 2 - 1] + K[cnt / 2]) / 2.0;  // np.ma.median: mean of the two middle values
    }
    cmax[c0 + c] = mx;
    cmin[c0 + c] = mn;
    cmed[c0 + c] = md;
}

__global__ void __launch_bounds__(256) k_imp_apply(double *__restrict__ X, int64_t n, int64_t ld, int64_t n_cols,
                                                   const double *__restrict__ cmax, const double *__restrict__ cmin,
                                                   const double *__restrict__ cmed) {
    const int64_t total = n * n_cols;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / n_cols, c = i - r * n_cols;
        const double v = X[r * ld + c];
        if (v != v) X[r * ld + c] = cmed[c];
        else if (v == __builtin_inf()) X[r * ld + c] = cmax[c];
        else if (v == -__builtin_inf()) X[r * ld + c] = cmin[c];
    }
}

extern "C" int tsfa_impute(double *X, int64_t n_rows, int64_t n_cols, int64_t ld, int32_t space, int32_t device,
                           double *col_max, double *col_min, double *col_median, int32_t *finite_count) {
    if (!X || n_rows < 0 || n_cols < 0 || ld < n_cols) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_impute: null pointer or bad shape");
    if (n_rows >= (1ll << 31)) return tsfa_fail(TSFA_ERR_TOO_LONG, "tsfa_impute: more than 2^31 rows");
    int rc = rel_check_device(device, "tsfa_impute", REL_NO_CPU_PATH);
    if (rc || n_cols == 0 || n_rows == 0) return rc;
    RelMatrix m;
    RelSorter s;
    DevPtr<double> dstat;
    DevPtr<int> dcnt;
    HIP_TRY(hipSetDevice(device));
    if ((rc = m.stage(X, n_rows, n_cols, ld, space))) return rc;
    if ((rc = s.init(n_rows, n_cols))) return rc;
    HIP_TRY_MALLOC(dcnt, (size_t)n_cols * sizeof(int));
    HIP_TRY_MALLOC(dstat, (size_t)3 * n_cols * sizeof(double));
    double *cmax = dstat.get(), *cmin = cmax + n_cols, *cmed = cmin + n_cols;
    rc = s.run(
        n_cols,
        [&](int64_t c0, int64_t nb) {
            k_imp_stage<<<dim3((unsigned)nb), REL_NT, 0, 0>>>(m.X, n_rows, m.ld, c0, s.keys.get(), s.idx.get(), s.np2, dcnt.get());
        },
        [&](int64_t c0, int64_t nb) {
            k_imp_stats<<<dim3((unsigned)((nb + 63) / 64)), 64, 0, 0>>>(s.keys.get(), s.np2, dcnt.get(), c0, nb, cmax, cmin, cmed);
        });
    if (rc) return rc;
    // the matrix that is patched: the staged copy of a host matrix (written back below), or the caller's device matrix
    k_imp_apply<<<2048, 256, 0, 0>>>(m.own ? m.own.get() : X, n_rows, m.ld, n_cols, cmax, cmin, cmed);
    HIP_TRY(hipGetLastError());
    if (col_max) HIP_TRY(hipMemcpy(col_max, cmax, (size_t)n_cols * sizeof(double), hipMemcpyDeviceToHost));
    if (col_min) HIP_TRY(hipMemcpy(col_min, cmin, (size_t)n_cols * sizeof(double), hipMemcpyDeviceToHost));
    if (col_median) HIP_TRY(hipMemcpy(col_median, cmed, (size_t)n_cols * sizeof(double), hipMemcpyDeviceToHost));
    if (finite_count) HIP_TRY(hipMemcpy(finite_count, dcnt.get(), (size_t)n_cols * sizeof(int), hipMemcpyDeviceToHost));
    if ((rc = m.write_back(X, n_rows, n_cols, ld))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return TSFA_OK;
}

// ---------------------------------------------------------------------------------------------
// Device-resident matrices: extract -> impute -> select without the feature matrix crossing PCIe
// between the steps.  tsfa_extract / tsfa_impute / tsfa_relevance_* take TSFA_DEVICE pointers; these four entry points
// give a host in any language the buffer, the transfers and the final gather of the selected columns.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_gather_columns(const double *__restrict__ X, int64_t n_rows, int64_t ld,
                                                         const int32_t *__restrict__ cols, int64_t n_sel,
                                                         double *__restrict__ out) {
    const int64_t total = n_rows * n_sel;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / n_sel, c = i - r * n_sel;
        out[i] = X[r * ld + cols[c]];
    }
}

__global__ void __launch_bounds__(256) k_scatter_columns(double *__restrict__ dst, int64_t ld_dst, const int32_t *__restrict__ cols,
                                                          const double *__restrict__ src, int64_t n_rows, int64_t n_src) {
    const int64_t total = n_rows * n_src;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / n_src, c = i - r * n_src;
        dst[r * ld_dst + cols[c]] = src[i];
    }
}

extern "C" int tsfa_device_alloc(void **ptr, size_t bytes, int32_t device) {
    if (!ptr) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_device_alloc: ptr is NULL");
    *ptr = nullptr;
    int rc = rel_check_device(device, "tsfa_device_alloc");
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMalloc(ptr, bytes ? bytes : 1));
    return TSFA_OK;
}

extern "C" int tsfa_device_free(void *ptr, int32_t device) {
    if (!ptr) return TSFA_OK;
    int rc = rel_check_device(device, "tsfa_device_free");
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipFree(ptr));
    return TSFA_OK;
}

extern "C" int tsfa_device_copy(void *dst, const void *src, size_t bytes, int32_t to_device, int32_t device) {
    if ((!dst || !src) && bytes) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_device_copy: null pointer");
    int rc = rel_check_device(device, "tsfa_device_copy");
    if (rc || !bytes) return rc;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMemcpy(dst, src, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost));
    return TSFA_OK;
}

extern "C" int tsfa_gather_columns(const double *X, int64_t n_rows, int64_t ld, const int32_t *cols, int64_t n_sel,
                                   double *out_host, int32_t device) {
    if (n_rows < 0 || n_sel < 0 || ((n_rows && n_sel) && (!X || !cols || !out_host)))
        return tsfa_fail(TSFA_ERR_INVALID, "tsfa_gather_columns: null pointer or bad shape");
    int rc = rel_check_device(device, "tsfa_gather_columns");
    if (rc || n_rows == 0 || n_sel == 0) return rc;
    for (int64_t c = 0; c < n_sel; ++c)
        if (cols[c] < 0 || cols[c] >= ld) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_gather_columns: column index out of range");
    DevPtr<int32_t> dcols;
    DevPtr<double> dout;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY_MALLOC(dcols, (size_t)n_sel * sizeof(int32_t));
    HIP_TRY_MALLOC(dout, (size_t)n_rows * n_sel * sizeof(double));
    HIP_TRY(hipMemcpy(dcols.get(), cols, (size_t)n_sel * sizeof(int32_t), hipMemcpyHostToDevice));
    k_gather_columns<<<2048, 256, 0, 0>>>(X, n_rows, ld, dcols.get(), n_sel, dout.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out_host, dout.get(), (size_t)n_rows * n_sel * sizeof(double), hipMemcpyDeviceToHost));
    return TSFA_OK;
}

extern "C" int tsfa_scatter_columns(double *dst, int64_t ld_dst, const int32_t *cols, const double *src, int64_t n_rows,
                                    int64_t n_src, int32_t device) {
    if (n_rows < 0 || n_src < 0 || ((n_rows && n_src) && (!dst || !cols || !src)))
        return tsfa_fail(TSFA_ERR_INVALID, "tsfa_scatter_columns: null pointer or bad shape");
    int rc = rel_check_device(device, "tsfa_scatter_columns");
    if (rc || n_rows == 0 || n_src == 0) return rc;
    for (int64_t c = 0; c < n_src; ++c)
        if (cols[c] < 0 || cols[c] >= ld_dst) return tsfa_fail(TSFA_ERR_INVALID, "tsfa_scatter_columns: column index out of range");
    DevPtr<int32_t> dcols;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY_MALLOC(dcols, (size_t)n_src * sizeof(int32_t));
    HIP_TRY(hipMemcpy(dcols.get(), cols, (size_t)n_src * sizeof(int32_t), hipMemcpyHostToDevice));
    k_scatter_columns<<<2048, 256, 0, 0>>>(dst, ld_dst, dcols.get(), src, n_rows, n_src);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return TSFA_OK;
}

// Pr(D >= h / lcm(m, n)) for the two-sided two-sample Kolmogorov-Smirnov statistic, m != n: the proportion of lattice
// paths (0,0) -> (m,n) that do not stay strictly inside |x/m - y/n| < h/lcm (Hodges 1958; the column recurrence scipy
// uses in ks_2samp(method="exact"), computed on the complement so small probabilities keep their relative accuracy).
// A scalar function of four integers: no data passes through it.
extern "C" double tsfa_ks_outer_prob(int64_t m, int64_t n, int64_t g, int64_t h) {
    if (m < n) { const int64_t t = m; m = n; n = t; }
    const int64_t mg = m / g, ng = n / g;
    int64_t minj = 0, maxj = (h + mg - 1) / mg;
    if (maxj > n + 1) maxj = n + 1;
    int64_t curlen = maxj - minj;
    int64_t lenA = 2 * maxj + 2;
    if (lenA > n + 1) lenA = n + 1;
    std::vector<double> A((size_t)lenA + 2, 1.0);
    for (int64_t j = minj; j < maxj; ++j) A[(size_t)j] = 0.0;
    for (int64_t i = 1; i <= m; ++i) {
        const int64_t lastminj = minj, lastlen = curlen;
        // floor((ng * i - h) / mg) + 1 and ceil((ng * i + h) / mg) in exact integer arithmetic
        const int64_t num = ng * i - h;
        int64_t fl = num / mg;
        if (num % mg != 0 && num < 0) --fl;
        minj = fl + 1;
        if (minj < 0) minj = 0;
        if (minj > n) minj = n;
        maxj = (ng * i + h + mg - 1) / mg;
        if (maxj > n + 1) maxj = n + 1;
        if (maxj <= minj) return 1.0;
        double val = (minj == 0) ? 0.0 : 1.0;
        for (int64_t jj = 0; jj < maxj - minj; ++jj) {
            const int64_t j = jj + minj;
            val = (A[(size_t)(jj + minj - lastminj)] * (double)i + val * (double)j) / (double)(i + j);
            A[(size_t)jj] = val;
        }
        curlen = maxj - minj;
        if (lastlen > curlen)
            for (int64_t q = maxj - minj; q < maxj - minj + (lastlen - curlen); ++q) A[(size_t)q] = 1.0;
    }
    return A[(size_t)(maxj - minj - 1)];
}
