// matrix_profile, the tiled route (TSFA_FAM_MPROFILE, launch record variant 1): the diagonal sweep of ONE series spread over
// the chip.  fam_mprofile.h gives a series to one workgroup; a single long recording then runs on one of 256 CUs.  Here the
// working arrays of every series of a launch group lie in HBM scratch of the plan (40 bytes per window position: mu, inv,
// df | dg, key -- MpWork with every array `stride` entries long) and three kernels run per distinct window of the plan:
//
//   k_mpt_prologue  one thread per (series, window index): mu, inv, df, dg by fam_mprofile.h's per-window arithmetic, key = 0.
//                   One more workgroup writes the tile table: the exclusive prefix of the series' tile counts.
//   k_mpt_sweep     the hot path.  The triangle of cells (row i, diagonal d >= ceil(w/4) + 1) is cut into tiles of
//                   TSFA_MP_RESTART rows, aligned to multiples of it, by TSFA_MP_TILE_D = 1024 neighbouring diagonals.  Every
//                   diagonal of a tile starts from mp_cov_direct at the tile's first row -- the row at which mp_sweep
//                   recomputes it too -- and advances by mp_sweep's recurrence, so a cell has the bits it has there.
//                   A persistent grid walks the tiles; a tile index becomes (series, diagonal block, row block) by a binary
//                   search in the table and a closed form within the series (only tiles that hold a cell are counted).
//   k_mpt_epilogue  one workgroup per series: mp_epilogue and mp_feature of fam_mprofile.h on the HBM arrays.
//
// The tile kernel.  A workgroup stages the row side (inv, df, dg of 256 rows) and the column side (j = i + d: one span of
// 256 + 1024 - 1 entries) in LDS, with zeroed row and column keys: 48 KB, three workgroups per CU, three wavefronts per SIMD.
// Entries beyond the series are staged with inv = NaN: such a cell fails the NaN rule like a flat window's, so the loop has
// no bounds test.  A lane holds FOUR NEIGHBOURING diagonals in registers.  From one row to the next its four columns move on
// by one, so per row it loads ONE new column entry, not four (the row loop is unrolled by four: the register names rotate),
// and a column's maximum over the lane's four diagonals is kept in a register and leaves with one ds_max_u64 when the
// column drops out of the lane's window.  The row side -- 45 of the 79 vector instructions per row of 64 cells in mp_sweep --
// is reduced in the lane first (three v_max_f64), then as an integer key over the 16 lanes of a DPP row, and the four rows
// of a wavefront meet in one ds_max_u64: once per 256 cells.  The maxima are order-free, so the regrouping keeps the bits.
// The column arrays are stored as four sub-arrays by (column mod 4): the lanes of a wavefront, four columns apart, read
// consecutive addresses.  At its end a tile merges every touched key into the series' HBM keys, one global atomicMax per
// entry, not per cell.  Matrix instructions do not fit: the direct covariances keep mp_cov_direct's summation order.
//
// This file is built like the long-series build: its barriers order global memory (the epilogue's arrays are in HBM).
#define TSFA_LONG 1
#include <hip/hip_runtime.h>

#include "fam_mprofile.h"
#include "tsfa_launch.h"

#include <algorithm>

#define MPT_ROWS TSFA_MP_RESTART
#define MPT_Q (TSFA_MP_TILE_D / MPT_ROWS)        // row blocks a diagonal block is wide
#define MPT_COLS (MPT_ROWS + TSFA_MP_TILE_D)     // column entries staged: >= MPT_ROWS + TSFA_MP_TILE_D - 1, a multiple of 4
#define MPT_SUB (MPT_COLS / TSFA_MP_LANE_D)      // entries of a sub-array (column mod 4)
static_assert(TSFA_MP_LANE_D == 4 && TSFA_MP_TILE_D == 4 * 64 * TSFA_MP_LANE_D && MPT_ROWS == 256 && MPT_ROWS % 4 == 0,
              "k_mpt_sweep: four wavefronts, four diagonals per lane, row loop unrolled by four");

struct MptSeries {
    int64_t sidx, off;
    int n, L, nd;   // nd: diagonals that hold a cell, L - ceil(w/4) - 1 (0: no admissible pair)
};

__device__ __forceinline__ MptSeries mpt_series(const int64_t *starts, const int64_t *ends, const int *sel, int64_t first, int64_t k,
                                                int w) {
    MptSeries s;
    s.sidx = sel ? (int64_t)sel[k] : first + k;
    s.off = starts[s.sidx];
    s.n = (int)(ends[s.sidx] - s.off);
    s.L = s.n - w + 1;
    const int nd = s.L - mp_excl(w) - 1;
    s.nd = (w >= TSFA_MP_MIN_W && nd > 0) ? nd : 0;
    return s;
}

__device__ __forceinline__ MpWork mpt_work(unsigned char *slots, int64_t k, int stride) {
    double *p = (double *)slots + (size_t)k * 5 * (size_t)stride;
    MpWork W;
    W.mu = p;
    W.inv = p + stride;
    W.df = p + 2 * (size_t)stride;
    W.dg = p + 3 * (size_t)stride;
    W.key = (mp_key_t *)(p + 4 * (size_t)stride);
    return W;
}

// Tiles of a series with nd diagonals, diagonal block major: block db holds the diagonals from dmin + db TSFA_MP_TILE_D on,
// whose cells lie in the rows below nd - db TSFA_MP_TILE_D, that is in NR - MPT_Q db row blocks (NR = ceil(nd / MPT_ROWS)).
__host__ __device__ inline long long mpt_tiles(int nd) {
    if (nd <= 0) return 0;
    const long long NR = (nd + MPT_ROWS - 1) / MPT_ROWS, NB = (NR + MPT_Q - 1) / MPT_Q;
    return NB * NR - MPT_Q * (NB * (NB - 1) / 2);
}

template <typename T>
__global__ void __launch_bounds__(256) k_mpt_prologue(const T *__restrict__ values, const int64_t *__restrict__ starts,
                                                       const int64_t *__restrict__ ends, const int *__restrict__ sel, int64_t first,
                                                       int64_t ns, int w, int stride, int nblk, unsigned char *__restrict__ slots,
                                                       long long *__restrict__ pre) {
    const int tid = (int)threadIdx.x;
    if ((int64_t)blockIdx.x == ns * nblk) {   // the tile table: pre[k] = tiles of the series before k, pre[ns] = all
        __shared__ long long part[256];
        const int64_t per = (ns + 255) / 256;
        const int64_t lo = std::min<int64_t>(ns, tid * per), hi = std::min<int64_t>(ns, lo + per);
        long long acc = 0;
        for (int64_t k = lo; k < hi; ++k) acc += mpt_tiles(mpt_series(starts, ends, sel, first, k, w).nd);
        part[tid] = acc;
        __syncthreads();
        if (tid == 0) {
            long long run = 0;
            for (int t = 0; t < 256; ++t) {
                const long long v = part[t];
                part[t] = run;
                run += v;
            }
        }
        __syncthreads();
        acc = part[tid];
        for (int64_t k = lo; k < hi; ++k) {
            pre[k] = acc;
            acc += mpt_tiles(mpt_series(starts, ends, sel, first, k, w).nd);
        }
        if (tid == 255) pre[ns] = acc;   // (its span is the last one, or empty behind the last one)
        return;
    }
    const int64_t k = (int64_t)blockIdx.x / nblk;
    const int i = (int)((int64_t)blockIdx.x % nblk) * 256 + tid;
    const MptSeries s = mpt_series(starts, ends, sel, first, k, w);
    if (s.nd == 0 || i >= s.L) return;
    const XsView<T> x{values + s.off};
    const MpWork W = mpt_work(slots, k, stride);
    bool flat, flat1;
    const double m = mp_window_mean(x, i, w, &flat);
    const double m1 = (i + 1 < s.L) ? mp_window_mean(x, i + 1, w, &flat1) : 0.0;
    W.mu[i] = m;
    W.inv[i] = mp_window_inv(x, i, w, m, flat);
    mp_window_diffs(x, i, w, s.L, m, m1, &W.df[i], &W.dg[i]);
    W.key[i] = 0ull;
}

template <int CTRL>
__device__ __forceinline__ mp_key_t mpt_dpp_key(mp_key_t v) {
    const int lo = __builtin_amdgcn_update_dpp((int)(unsigned)v, (int)(unsigned)v, CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(unsigned)(v >> 32), (int)(unsigned)(v >> 32), CTRL, 0xf, 0xf, false);
    return ((mp_key_t)(unsigned)hi << 32) | (mp_key_t)(unsigned)lo;
}
// the largest key of the 16 lanes of a DPP row, in every one of them
__device__ __forceinline__ mp_key_t mpt_row16_max(mp_key_t k) {
    mp_key_t o;
    o = mpt_dpp_key<TSFA_DPP_QUAD_XOR1>(k); k = o > k ? o : k;
    o = mpt_dpp_key<TSFA_DPP_QUAD_XOR2>(k); k = o > k ? o : k;
    o = mpt_dpp_key<TSFA_DPP_ROW_HALF_MIRROR>(k); k = o > k ? o : k;
    o = mpt_dpp_key<TSFA_DPP_ROW_MIRROR>(k); k = o > k ? o : k;
    return k;
}

template <typename T>
__global__ void __launch_bounds__(256) k_mpt_sweep(const T *__restrict__ values, const int64_t *__restrict__ starts,
                                                    const int64_t *__restrict__ ends, const int *__restrict__ sel, int64_t first, int64_t ns,
                                                    int w, int stride, unsigned char *__restrict__ slots,
                                                    const long long *__restrict__ pre) {
    __shared__ double r_inv[MPT_ROWS], r_df[MPT_ROWS], r_dg[MPT_ROWS];
    __shared__ double c_inv[MPT_COLS], c_df[MPT_COLS], c_dg[MPT_COLS];   // entry of column c: (c & 3) * MPT_SUB + (c >> 2)
    __shared__ mp_key_t r_key[MPT_ROWS], c_key[MPT_COLS];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int dmin = mp_excl(w) + 1;
    const long long total = pre[ns];
    for (long long t = blockIdx.x; t < total; t += gridDim.x) {
        int64_t lo = 0, hi = ns;   // pre[lo] <= t < pre[hi]
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (pre[mid] <= t) lo = mid; else hi = mid;
        }
        const MptSeries s = mpt_series(starts, ends, sel, first, lo, w);
        const int NR = (s.nd + MPT_ROWS - 1) / MPT_ROWS;
        long long rem = t - pre[lo];
        int db = 0;
        while (NR - MPT_Q * db > 0 && rem >= NR - MPT_Q * db) {
            rem -= NR - MPT_Q * db;
            ++db;
        }
        const int L = s.L;
        const int i0 = (int)rem * MPT_ROWS, d0 = dmin + db * TSFA_MP_TILE_D, j0 = i0 + d0;
        const MpWork W = mpt_work(slots, lo, stride);
        for (int r = tid; r < MPT_ROWS; r += 256) {
            const bool in = i0 + r < L;
            r_inv[r] = in ? W.inv[i0 + r] : TSFA_NAN;
            r_df[r] = in ? W.df[i0 + r] : 0.0;
            r_dg[r] = in ? W.dg[i0 + r] : 0.0;
            r_key[r] = 0ull;
        }
        for (int c = tid; c < MPT_COLS; c += 256) {
            const bool in = j0 + c < L;
            const int p = (c & 3) * MPT_SUB + (c >> 2);
            c_inv[p] = in ? W.inv[j0 + c] : TSFA_NAN;
            c_df[p] = in ? W.df[j0 + c] : 0.0;
            c_dg[p] = in ? W.dg[j0 + c] : 0.0;
            c_key[p] = 0ull;
        }
        __syncthreads();
        // the wavefront's diagonals: d0 + 256 wv + (4 lane .. 4 lane + 3); its rows: those of its first diagonal
        const int g = wv * 64 + lane;
        const int rows = std::min(MPT_ROWS, L - (d0 + 256 * wv) - i0);
        if (rows > 0) {
            const XsView<T> x{values + s.off};
            const int jl = j0 + 4 * g;   // column of the lane's first diagonal at the tile's first row
            double cv[4], mj[4];
            bool ok[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ok[r] = jl + r < L;
                mj[r] = ok[r] ? W.mu[jl + r] : 0.0;
                cv[r] = 0.0;
            }
            const double mi = W.mu[i0];
            for (int k = 0; k < w; ++k) {   // mp_cov_direct of the four diagonals, each in its order over k
                const double xi = x[i0 + k] - mi;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double xj = ok[r] ? x[jl + r + k] : 0.0;
                    cv[r] += xi * (xj - mj[r]);
                }
            }
            // slot s of ci / cf / cg / cm: the column of the lane's window that is s mod 4 (relative to its first column)
            double ci[4], cf[4], cg[4], cm[4];
#pragma unroll
            for (int sl = 0; sl < 3; ++sl) {
                ci[sl] = c_inv[sl * MPT_SUB + g];
                cf[sl] = c_df[sl * MPT_SUB + g];
                cg[sl] = c_dg[sl * MPT_SUB + g];
                cm[sl] = -TSFA_INF;
            }
            const int nq = (rows + 3) >> 2;
            for (int q = 0; q < nq; ++q) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int row = 4 * q + u;
                    {   // the column that enters the window: relative column row + 3
                        const int sn = (u + 3) & 3, e = sn * MPT_SUB + q + g + ((u + 3) >> 2);
                        ci[sn] = c_inv[e];
                        cf[sn] = c_df[e];
                        cg[sn] = c_dg[e];
                        cm[sn] = -TSFA_INF;
                    }
                    const double ri = r_inv[row], rf = r_df[row], rg = r_dg[row];
                    double m = -TSFA_INF;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int sl = (u + r) & 3;
                        double v = cv[r] * ri * ci[sl];
                        cv[r] = cv[r] + rf * cg[sl] + cf[sl] * rg;
                        if (v > 1.0) v = 1.0;
                        const double rho = (v == v) ? v : -TSFA_INF;   // (a flat window, or an entry beyond the series: NaN)
                        cm[sl] = __builtin_fmax(cm[sl], rho);
                        m = __builtin_fmax(m, rho);
                    }
                    // the column that leaves the window: relative column row, slot u
                    if (cm[u] > -TSFA_INF) (void)atomicMax(&c_key[u * MPT_SUB + q + g], mp_enc(cm[u]));
                    const mp_key_t rk = mpt_row16_max(m > -TSFA_INF ? mp_enc(m) : 0ull);
                    if ((lane & 15) == 0 && rk != 0ull) (void)atomicMax(&r_key[row], rk);
                }
            }
#pragma unroll
            for (int sl = 0; sl < 3; ++sl)   // the columns still in the window behind the last row
                if (cm[sl] > -TSFA_INF) (void)atomicMax(&c_key[sl * MPT_SUB + nq + g], mp_enc(cm[sl]));
        }
        __syncthreads();
        for (int r = tid; r < MPT_ROWS; r += 256) {
            const mp_key_t k = r_key[r];
            if (k != 0ull && i0 + r < L) (void)atomicMax(&W.key[i0 + r], k);
        }
        for (int p = tid; p < MPT_COLS; p += 256) {
            const mp_key_t k = c_key[p];
            const int c = ((p % MPT_SUB) << 2) | (p / MPT_SUB);
            if (k != 0ull && j0 + c < L) (void)atomicMax(&W.key[j0 + c], k);
        }
        __syncthreads();
    }
}

// the columns specs[s0 .. s1) of one window
__global__ void __launch_bounds__(256) k_mpt_epilogue(const int64_t *__restrict__ starts, const int64_t *__restrict__ ends,
                                                       const int *__restrict__ sel, int64_t first, int w, int stride,
                                                       unsigned char *__restrict__ slots, const TsfaSpec *__restrict__ specs, int s0, int s1,
                                                       double *__restrict__ out, int64_t ld) {
    __shared__ double red[TSFA_RED_DOUBLES];
    __shared__ NpScratch nps;
    const Blk b{(int)threadIdx.x, (int)blockDim.x, red, &nps};
    const MptSeries s = mpt_series(starts, ends, sel, first, blockIdx.x, w);
    const MpWork W = mpt_work(slots, blockIdx.x, stride);
    int m = 0;
    double mean = TSFA_NAN;
    if (s.nd > 0) m = mp_epilogue(b, s.L, w, W, &mean);
    for (int c = s0; c < s1; ++c) {
        const double v = mp_feature((int)specs[c].p[1], W.df, m, mean);
        if (b.tid == 0) out[s.sidx * ld + specs[c].col] = v;
    }
}

// the table ahead of the series' slots: (series + 1) prefix entries, rounded to 256 bytes
static size_t mpt_table_bytes(int64_t ns) { return (((size_t)ns + 1) * sizeof(long long) + 255) & ~(size_t)255; }

size_t tsfa_mprofile_tiles_scratch(int64_t n_series, int maxn, size_t cap) {
    const size_t slot = (size_t)40 * (size_t)maxn;
    int64_t ns = std::max<int64_t>(1, n_series);
    while (ns > 1 && mpt_table_bytes(ns) + (size_t)ns * slot > cap) ns = (ns + 1) / 2;   // (a chunk of the group: the launcher cuts it)
    return mpt_table_bytes(ns) + (size_t)ns * slot;
}

template <typename T>
static int launch_tiles_t(const TsfaLaunch &a, const T *values, const TsfaSpec *h_specs, unsigned char *scratch, size_t bytes) {
    hipStream_t st = (hipStream_t)a.stream;
    const int stride = a.maxn;
    const size_t slot = (size_t)40 * (size_t)stride;
    int64_t chunk = std::min<int64_t>(a.n_series, (int64_t)(bytes / (slot + sizeof(long long))));
    while (chunk > 0 && mpt_table_bytes(chunk) + (size_t)chunk * slot > bytes) --chunk;
    if (!scratch || chunk < 1) return -2;
    long long *pre = (long long *)scratch;
    unsigned char *slots = scratch + mpt_table_bytes(chunk);
    for (int64_t c0 = 0; c0 < a.n_series; c0 += chunk) {
        const int64_t ns = std::min<int64_t>(chunk, a.n_series - c0);
        const int *sel = a.sel ? a.sel + c0 : nullptr;
        for (int s0 = 0; s0 < a.nspecs;) {   // the windows one after another on the same scratch
            const int w = (int)h_specs[s0].p[0];
            int s1 = s0 + 1;
            while (s1 < a.nspecs && (int)h_specs[s1].p[0] == w) ++s1;
            const int Lmax = a.maxn - w + 1;
            const int nd = (w >= TSFA_MP_MIN_W) ? Lmax - (w + 3) / 4 - 1 : 0;   // (mp_excl: device code) of the longest series
            if (nd > 0) {
                const int nblk = (Lmax + 255) / 256;
                k_mpt_prologue<T><<<dim3((unsigned)(ns * nblk + 1)), 256, 0, st>>>(values, a.starts, a.ends, sel, c0, ns, w, stride, nblk, slots, pre);
                // a persistent grid: three workgroups of 48 KB per CU
                const long long most = (long long)ns * mpt_tiles(nd);
                k_mpt_sweep<T><<<dim3((unsigned)std::min<long long>(most, 256 * 3)), 256, 0, st>>>(values, a.starts, a.ends, sel, c0, ns, w, stride, slots, pre);
            }
            k_mpt_epilogue<<<dim3((unsigned)ns), 256, 0, st>>>(a.starts, a.ends, sel, c0, w, stride, slots, a.specs, s0, s1, a.out, a.ld);
            s0 = s1;
        }
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

int tsfa_launch_mprofile_tiles(const TsfaLaunch &a, const TsfaSpec *h_specs, unsigned char *scratch, size_t bytes) {
    if (a.dtype == 0) return launch_tiles_t<float>(a, (const float *)a.values, h_specs, scratch, bytes);
    return launch_tiles_t<double>(a, (const double *)a.values, h_specs, scratch, bytes);
}
