// sample_entropy / approximate_entropy (m = 2), the tiled route (TSFA_FAM_ENTROPY, launch record variant 5): the ordered-pair
// sweep of ONE series spread over the chip.  k_entropy of the long-series build gives a series to one workgroup
// (entropy_sweep_m2, fam_entropy.h): a single recording of 100 000 samples then runs its 10^10 pair tests on one of 256 CUs.
// The per-row results of that sweep are integer counts, so any split of the columns gives the same counts; here the working
// arrays of every series of a launch group lie in HBM scratch of the plan and five kernels run:
//
//   k_ent_prologue  one workgroup per series, once: the standard deviation by fam_entropy_series' own expressions (the numpy-order
//                   sums, or the k_basic record), the order of the length-2 templates by entropy_sort_templates<.., unsigned int>,
//                   and the SORTED triples (x[p], x[p+1], x[p+2]) as three arrays (+inf beyond the series): the sweep reads
//                   consecutive addresses on both sides and never gathers through the order.
//   then per batch of TSFA_ENT_MAXK tolerances (the batches of fam_entropy_series), on the same scratch:
//   k_ent_windows   one workgroup per series: the batch's tolerances (ent_tolerance), the column window [jlo, jhi) of every block
//                   of 256 sorted rows -- entropy_sweep_m2's band +- rmax with its margin, bisected in the sorted first samples --
//                   the block's tile count ceil((jhi - jlo) / ENT_C), and zeroed counters.
//   k_ent_scan      one workgroup: the tile table, the exclusive prefix of the tile counts over (series, row block).
//   k_ent_sweep     the hot path, a persistent grid.  A tile index becomes (series, row block, column chunk) by a binary search
//                   in the table.  The workgroup stages the chunk's triples in LDS (3 x 2048 doubles, 48 KB: three workgroups
//                   per CU); a lane owns one row, keeps its triple and the tolerances in registers and walks the columns by
//                   broadcast LDS reads, four columns per step and the next four in flight (ent_eval_group: three subtractions
//                   and two maxima per pair, then per tolerance two compares whose masks enter the counters as carry-in).  It
//                   ends with one 32-bit atomicAdd per (row, tolerance, m | m + 1) into the series' counters: counts stay
//                   below 2^32.  Matrix instructions do not fit: max-norm compares, no dot product.
//   k_ent_epilogue  one workgroup of 256 threads per series: the counters in the pair sweep's own order (row pass * 256 + tid,
//                   ent_acc_row per row, blk_sum, ent_m2_value) -- the functions and the workgroup size of kl_entropy, so every
//                   cell equals that route's bit for bit.
//
// This file is built like the long-series build: its barriers order global memory (the order is sorted in HBM).
#define TSFA_LONG 1
#include <hip/hip_runtime.h>

#include "fam_entropy.h"
#include "tsfa_launch.h"

#include <algorithm>

#define ENT_ROWS 256     // sorted rows of a row block = threads of the sweep and of the epilogue (kl_entropy's workgroup)
#define ENT_C 2048       // columns of a tile
#define ENT_HDR 16       // doubles of a series' record: the batch's tolerances [0, TSFA_ENT_MAXK), the standard deviation [15]
#define ENT_PRO_NT 1024  // threads of the prologue (the sort and the numpy-order sums do not depend on the workgroup size)
static_assert(ENT_C % (2 * TSFA_ENT_G) == 0 && TSFA_ENT_G == 4, "k_ent_sweep: two groups of four columns per step");

// Scratch of a chunk of ns series whose longest has maxn samples: the tile table (ns * nblk + 1 prefix entries), the windows
// (jlo, jhi per row block), the records, then per series a slot of the sorted triples (3 x stride doubles), the order (np2
// words) and the counters (2 x TSFA_ENT_MAXK x stride words: C_m of tolerance k at [k * stride], C_{m+1} at [(8 + k) * stride]).
struct EntLayout {
    int stride, np2, nblk;
    size_t slot;
    __host__ __device__ explicit EntLayout(int maxn) {
        const int rows = maxn > 1 ? maxn - 1 : 1;
        stride = ((rows + ENT_ROWS - 1) / ENT_ROWS) * ENT_ROWS;
        np2 = 64;
        while (np2 < rows) np2 <<= 1;
        nblk = stride / ENT_ROWS;
        slot = (size_t)stride * (24 + 8 * TSFA_ENT_MAXK) + (size_t)np2 * 4;
    }
    static __host__ __device__ size_t r256(size_t b) { return (b + 255) & ~(size_t)255; }
    __host__ __device__ size_t pre_bytes(int64_t ns) const { return r256(((size_t)ns * nblk + 1) * sizeof(long long)); }
    __host__ __device__ size_t win_bytes(int64_t ns) const { return r256((size_t)ns * nblk * 2 * sizeof(int)); }
    __host__ __device__ size_t head_bytes(int64_t ns) const { return pre_bytes(ns) + win_bytes(ns) + r256((size_t)ns * ENT_HDR * sizeof(double)); }
    __host__ __device__ size_t bytes(int64_t ns) const { return head_bytes(ns) + (size_t)ns * slot; }
};

struct EntView {   // the arrays of series k of the chunk
    long long *pre;
    int *win;
    double *hdr, *s0, *s1, *s2;
    unsigned int *perm, *cnt;
};
__device__ __forceinline__ EntView ent_view(unsigned char *scratch, const EntLayout &L, int64_t ns, int64_t k) {
    EntView v;
    v.pre = (long long *)scratch;
    v.win = (int *)(scratch + L.pre_bytes(ns)) + (size_t)k * L.nblk * 2;
    v.hdr = (double *)(scratch + L.pre_bytes(ns) + L.win_bytes(ns)) + (size_t)k * ENT_HDR;
    unsigned char *p = scratch + L.head_bytes(ns) + (size_t)k * L.slot;
    v.s0 = (double *)p;
    v.s1 = v.s0 + L.stride;
    v.s2 = v.s1 + L.stride;
    v.perm = (unsigned int *)(v.s2 + L.stride);
    v.cnt = v.perm + L.np2;
    return v;
}

struct EntSeries {
    int64_t sidx, off;
    int n;
};
__device__ __forceinline__ EntSeries ent_series(const int64_t *starts, const int64_t *ends, const int *sel, int64_t first, int64_t k) {
    EntSeries s;
    s.sidx = sel ? (int64_t)sel[k] : first + k;
    s.off = starts[s.sidx];
    s.n = (int)(ends[s.sidx] - s.off);
    return s;
}

template <typename T>
__global__ void __launch_bounds__(ENT_PRO_NT) k_ent_prologue(const T *__restrict__ values, const int64_t *__restrict__ starts,
                                                              const int64_t *__restrict__ ends, const int *__restrict__ sel, int64_t first,
                                                              int64_t ns, int maxn, const double *__restrict__ stats_in,
                                                              unsigned char *__restrict__ scratch) {
    __shared__ double red[TSFA_RED_DOUBLES];
    __shared__ NpScratch nps;
    const Blk b{(int)threadIdx.x, (int)blockDim.x, red, &nps};
    const EntLayout L(maxn);
    const EntSeries s = ent_series(starts, ends, sel, first, blockIdx.x);
    const EntView V = ent_view(scratch, L, ns, blockIdx.x);
    const int n = s.n;
    if (n < 3) return;   // (no template pair: the epilogue writes the closed forms)
    const T *__restrict__ xs = values + s.off;
    const double *stats = stats_in ? stats_in + s.sidx * TSFA_STATS_N : nullptr;
    // np.std(x) as in fam_entropy_series: the tolerances are then the same bits
    const double dn = (double)n;
    const double mean = stats ? stats[TSFA_STATS_MEAN] : np_sum(b, n, [=](int i) { return (double)xs[i]; }) / dn;
    const double var = stats ? stats[TSFA_STATS_VAR] : np_sum(b, n, [=](int i) { const double d = (double)xs[i] - mean; return d * d; }) / dn;
    if (b.tid == 0) V.hdr[ENT_HDR - 1] = sqrt(var);
    entropy_sort_templates(b, xs, n, V.perm, next_pow2(n - 1));
    const int rows = n - 1, padded = ((rows + ENT_ROWS - 1) / ENT_ROWS) * ENT_ROWS;   // (<= L.stride)
    for (int q = b.tid; q < padded; q += b.nt) {
        double x0 = TSFA_INF, x1 = TSFA_INF, x2 = TSFA_INF;
        if (q < rows) {
            const int p = (int)V.perm[q];
            x0 = (double)xs[p];
            x1 = (double)xs[p + 1];
            if (p + 2 < n) x2 = (double)xs[p + 2];
        }
        V.s0[q] = x0;
        V.s1[q] = x1;
        V.s2[q] = x2;
    }
}

// the tolerances of the batch specs[0 .. nk) at standard deviation sd; unused slots never match
__device__ __forceinline__ void ent_batch_tolerances(const TsfaSpec *__restrict__ specs, int nk, double sd, double *r) {
#pragma unroll
    for (int k = 0; k < TSFA_ENT_MAXK; ++k) {
        r[k] = -1.0;
        if (k < nk) r[k] = ent_tolerance((specs[k].calc == TSFA_C_SAMPLE_ENTROPY) ? 0.2 * sd : specs[k].p[1] * sd);
    }
}

__global__ void __launch_bounds__(ENT_ROWS) k_ent_windows(const int64_t *__restrict__ starts, const int64_t *__restrict__ ends,
                                                           const int *__restrict__ sel, int64_t first, int64_t ns, int maxn,
                                                           const TsfaSpec *__restrict__ specs, int nk, unsigned char *__restrict__ scratch) {
    const int tid = (int)threadIdx.x;
    const EntLayout L(maxn);
    const EntSeries s = ent_series(starts, ends, sel, first, blockIdx.x);
    const EntView V = ent_view(scratch, L, ns, blockIdx.x);
    long long *tiles = V.pre + (size_t)blockIdx.x * L.nblk;   // counts here, k_ent_scan turns them into the prefix
    const int n = s.n, rows = n - 1;
    if (n < 3) {
        for (int rb = tid; rb < L.nblk; rb += ENT_ROWS) tiles[rb] = 0;
        return;
    }
    double r[TSFA_ENT_MAXK];
    ent_batch_tolerances(specs, nk, V.hdr[ENT_HDR - 1], r);
    double rmax = 0.0;   // (entropy_sweep_m2's: the largest tolerance, 0 at least)
#pragma unroll
    for (int k = 0; k < TSFA_ENT_MAXK; ++k) {
        rmax = fmax(rmax, r[k]);
        if (tid == k) V.hdr[k] = r[k];
    }
    const double *__restrict__ s0 = V.s0;
    for (int rb = tid; rb < L.nblk; rb += ENT_ROWS) {
        const int q0 = rb * ENT_ROWS;
        long long nt = 0;
        if (q0 < rows) {
            const int q1 = (q0 + ENT_ROWS < rows) ? (q0 + ENT_ROWS) : rows;
            // entropy_sweep_m2's window of the rows [q0, q1): first samples within rmax of the band, widened by a rounding margin
            const double band_lo = s0[q0], band_hi = s0[q1 - 1];
            const double margin = 1e-9 * (fabs(band_lo) + fabs(band_hi) + rmax);
            const double key_lo = band_lo - rmax - margin, key_hi = band_hi + rmax + margin;
            int lo = 0, hi = rows;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (s0[mid] < key_lo) lo = mid + 1; else hi = mid; }
            const int jlo = lo;
            hi = rows;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (s0[mid] <= key_hi) lo = mid + 1; else hi = mid; }
            V.win[2 * rb] = jlo;
            V.win[2 * rb + 1] = lo;
            nt = (lo - jlo + ENT_C - 1) / ENT_C;
        }
        tiles[rb] = nt;
    }
    for (int k = 0; k < nk; ++k)
        for (int q = tid; q < rows; q += ENT_ROWS) {
            V.cnt[(size_t)k * L.stride + q] = 0u;
            V.cnt[(size_t)(TSFA_ENT_MAXK + k) * L.stride + q] = 0u;
        }
}

// pre[0 .. E): tile counts -> their exclusive prefix; pre[E] = all tiles
__global__ void __launch_bounds__(1024) k_ent_scan(long long *__restrict__ pre, long long E) {
    __shared__ long long part[1024];
    const int tid = (int)threadIdx.x;
    const long long per = (E + 1023) / 1024;
    const long long lo = std::min<long long>(E, tid * per), hi = std::min<long long>(E, lo + per);
    long long acc = 0;
    for (long long e = lo; e < hi; ++e) acc += pre[e];
    part[tid] = acc;
    __syncthreads();
    if (tid == 0) {
        long long run = 0;
        for (int t = 0; t < 1024; ++t) {
            const long long v = part[t];
            part[t] = run;
            run += v;
        }
    }
    __syncthreads();
    acc = part[tid];
    for (long long e = lo; e < hi; ++e) {
        const long long v = pre[e];
        pre[e] = acc;
        acc += v;
    }
    if (tid == 1023) pre[E] = acc;   // (its span is the last one, or empty behind the last one)
}

__device__ __forceinline__ void ent_tile_group(const double *c0, const double *c1, const double *c2, int c, EntCol *g) {
#pragma unroll
    for (int u = 0; u < TSFA_ENT_G; ++u) { g[u].x0 = c0[c + u]; g[u].x1 = c1[c + u]; g[u].x2 = c2[c + u]; }
}

// NK: tolerances compared (the batch's, rounded up; the slots beyond the batch hold -1 and count nothing)
template <int NK>
__global__ void __launch_bounds__(ENT_ROWS) k_ent_sweep(const int64_t *__restrict__ starts, const int64_t *__restrict__ ends,
                                                         const int *__restrict__ sel, int64_t first, int64_t ns, int maxn,
                                                         unsigned char *__restrict__ scratch) {
    // (one group past the chunk: the double-buffered loop loads it and never evaluates it)
    __shared__ __attribute__((aligned(16))) double c0[ENT_C + TSFA_ENT_G], c1[ENT_C + TSFA_ENT_G], c2[ENT_C + TSFA_ENT_G];
    const int tid = (int)threadIdx.x;
    const EntLayout L(maxn);
    const long long *__restrict__ pre = (const long long *)scratch;
    const long long E = (long long)ns * L.nblk;
    const long long total = pre[E];
    for (long long t = blockIdx.x; t < total; t += gridDim.x) {
        long long lo = 0, hi = E;   // pre[lo] <= t < pre[hi]
        while (hi - lo > 1) {
            const long long mid = (lo + hi) >> 1;
            if (pre[mid] <= t) lo = mid; else hi = mid;
        }
        const int64_t k = lo / L.nblk;
        const int rb = (int)(lo % L.nblk);
        const EntView V = ent_view(scratch, L, ns, k);
        const int rows = ent_series(starts, ends, sel, first, k).n - 1;
        const int cb = V.win[2 * rb] + (int)(t - pre[lo]) * ENT_C;           // first column of the chunk
        const int len = std::min(ENT_C, V.win[2 * rb + 1] - cb);             // 1 .. ENT_C columns, all below `rows`
        const int len8 = (len + 2 * TSFA_ENT_G - 1) & ~(2 * TSFA_ENT_G - 1);  // padded with +inf: matches nothing
        for (int c = tid; c < len8; c += ENT_ROWS) {
            const bool in = c < len;
            c0[c] = in ? V.s0[cb + c] : TSFA_INF;
            c1[c] = in ? V.s1[cb + c] : TSFA_INF;
            c2[c] = in ? V.s2[cb + c] : TSFA_INF;
        }
        const int q = rb * ENT_ROWS + tid;   // (< L.stride; beyond the series the prologue left +inf: such a lane counts nothing)
        const double xi0 = V.s0[q], xi1 = V.s1[q], xi2 = V.s2[q];
        double r[NK];
#pragma unroll
        for (int j = 0; j < NK; ++j) r[j] = V.hdr[j];
        int n2[NK], n3[NK];
#pragma unroll
        for (int j = 0; j < NK; ++j) { n2[j] = 0; n3[j] = 0; }
        __syncthreads();
        EntCol ca[TSFA_ENT_G], cbuf[TSFA_ENT_G];
        unsigned int colv = 0u;
        ent_tile_group(c0, c1, c2, 0, ca);
        for (int c = 0; c < len8; c += 2 * TSFA_ENT_G) {
            ent_tile_group(c0, c1, c2, c + TSFA_ENT_G, cbuf);
            ent_eval_group<NK, false>(xi0, xi1, xi2, ca, r, n2, n3, colv, nullptr);
            ent_tile_group(c0, c1, c2, c + 2 * TSFA_ENT_G, ca);
            ent_eval_group<NK, false>(xi0, xi1, xi2, cbuf, r, n2, n3, colv, nullptr);
        }
        if (q < rows) {
#pragma unroll
            for (int j = 0; j < NK; ++j) {
                if (n2[j] != 0) (void)atomicAdd(&V.cnt[(size_t)j * L.stride + q], (unsigned int)n2[j]);
                if (n3[j] != 0) (void)atomicAdd(&V.cnt[(size_t)(TSFA_ENT_MAXK + j) * L.stride + q], (unsigned int)n3[j]);
            }
        }
        __syncthreads();
    }
}

// the columns specs[0 .. nk) of the batch
__global__ void __launch_bounds__(ENT_ROWS) k_ent_epilogue(const int64_t *__restrict__ starts, const int64_t *__restrict__ ends,
                                                            const int *__restrict__ sel, int64_t first, int64_t ns, int maxn,
                                                            const TsfaSpec *__restrict__ specs, int nk, unsigned char *__restrict__ scratch,
                                                            double *__restrict__ out, int64_t ld) {
    __shared__ double red[TSFA_RED_DOUBLES];
    __shared__ NpScratch nps;
    const Blk b{(int)threadIdx.x, (int)blockDim.x, red, &nps};
    const EntLayout L(maxn);
    const EntSeries s = ent_series(starts, ends, sel, first, blockIdx.x);
    const EntView V = ent_view(scratch, L, ns, blockIdx.x);
    const int n = s.n, nrow_m = n - 1, nrow_m1 = n - 2;
    const double dm = (double)nrow_m, dm1 = (double)nrow_m1;
    const int npass = (n >= 3) ? (nrow_m + b.nt - 1) / b.nt : 0;
    for (int k = 0; k < nk; ++k) {
        const unsigned int *__restrict__ cm = V.cnt + (size_t)k * L.stride, *__restrict__ cm1 = V.cnt + (size_t)(TSFA_ENT_MAXK + k) * L.stride;
        double slm = 0.0, slm1 = 0.0, scm = 0.0, scm1 = 0.0;
        for (int pass = 0; pass < npass; ++pass) {
            const int qi = pass * b.nt + b.tid;
            const bool row_m = (qi < nrow_m);
            const bool row_m1 = row_m && ((int)V.perm[qi] < nrow_m1);
            ent_acc_row(row_m, row_m1, row_m ? (int)cm[qi] : 0, row_m ? (int)cm1[qi] : 0, dm, dm1, slm, slm1, scm, scm1);
        }
        EntAcc a;
        a.sum_log_m = blk_sum(b, slm);
        a.sum_log_m1 = blk_sum(b, slm1);
        a.sum_cnt_m = blk_sum(b, scm);
        a.sum_cnt_m1 = blk_sum(b, scm1);
        const double v = ent_m2_value(specs[k].calc, a, n);
        if (b.tid == 0) out[s.sidx * ld + specs[k].col] = v;
    }
}

size_t tsfa_entropy_tiles_scratch(int64_t n_series, int maxn, size_t cap) {
    const EntLayout L(maxn);
    int64_t ns = std::max<int64_t>(1, n_series);
    while (ns > 1 && L.bytes(ns) > cap) ns = (ns + 1) / 2;   // (a chunk of the group: the launcher cuts it)
    return L.bytes(ns);
}

template <typename T>
static int launch_tiles_t(const TsfaLaunch &a, const T *values, unsigned char *scratch, size_t bytes) {
    hipStream_t st = (hipStream_t)a.stream;
    const EntLayout L(a.maxn);
    int64_t chunk = std::min<int64_t>(a.n_series, (int64_t)(bytes / L.slot));
    while (chunk > 0 && L.bytes(chunk) > bytes) --chunk;
    if (!scratch || chunk < 1) return -2;
    for (int64_t c0 = 0; c0 < a.n_series; c0 += chunk) {
        const int64_t ns = std::min<int64_t>(chunk, a.n_series - c0);
        const int *sel = a.sel ? a.sel + c0 : nullptr;
        const dim3 per_series((unsigned)ns);
        k_ent_prologue<T><<<per_series, ENT_PRO_NT, 0, st>>>(values, a.starts, a.ends, sel, c0, ns, a.maxn, a.stats_in, scratch);
        // a persistent grid: three workgroups of 48 KB per CU; never more than the tiles of full windows
        const long long most = (long long)ns * L.nblk * ((L.stride + ENT_C - 1) / ENT_C);
        const dim3 grid((unsigned)std::min<long long>(most, 256 * 3));
        for (int s0 = 0; s0 < a.nspecs; s0 += TSFA_ENT_MAXK) {   // the batches of fam_entropy_series, on the same scratch
            const int nk = std::min(TSFA_ENT_MAXK, a.nspecs - s0);
            k_ent_windows<<<per_series, ENT_ROWS, 0, st>>>(a.starts, a.ends, sel, c0, ns, a.maxn, a.specs + s0, nk, scratch);
            k_ent_scan<<<1, 1024, 0, st>>>((long long *)scratch, (long long)ns * L.nblk);
            if (nk <= 1) k_ent_sweep<1><<<grid, ENT_ROWS, 0, st>>>(a.starts, a.ends, sel, c0, ns, a.maxn, scratch);
            else if (nk <= 2) k_ent_sweep<2><<<grid, ENT_ROWS, 0, st>>>(a.starts, a.ends, sel, c0, ns, a.maxn, scratch);
            else if (nk <= 4) k_ent_sweep<4><<<grid, ENT_ROWS, 0, st>>>(a.starts, a.ends, sel, c0, ns, a.maxn, scratch);
            else if (nk <= 6) k_ent_sweep<6><<<grid, ENT_ROWS, 0, st>>>(a.starts, a.ends, sel, c0, ns, a.maxn, scratch);
            else k_ent_sweep<8><<<grid, ENT_ROWS, 0, st>>>(a.starts, a.ends, sel, c0, ns, a.maxn, scratch);
            k_ent_epilogue<<<per_series, ENT_ROWS, 0, st>>>(a.starts, a.ends, sel, c0, ns, a.maxn, a.specs + s0, nk, scratch, a.out, a.ld);
        }
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

int tsfa_launch_entropy_tiles(const TsfaLaunch &a, unsigned char *scratch, size_t bytes) {
    if (a.dtype == 0) return launch_tiles_t<float>(a, (const float *)a.values, scratch, bytes);
    return launch_tiles_t<double>(a, (const double *)a.values, scratch, bytes);
}
