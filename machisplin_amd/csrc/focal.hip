// Window statistics of one plane at any radius (include/machisplin_hip.h, section "focal", states the rules; focal_rule.h holds
// them): blocked prefix sums along the rows, then -- square windows -- down the columns of the row-window sums, or -- circular
// windows -- a sum of 2 R + 1 row-window sums.  No window is held in LDS, so nothing limits the radius; no atomics.
//
// focal_rows_kernel (once per call, whatever the radii).  A workgroup of 256 threads takes whole rows, FOC_CHUNK = 64 blocks of
// B = 64 cells at a time.  The chunk is loaded with 64 consecutive elements per wave load, converted and centred, into LDS
// (65 doubles per block: lane b's run starts in another bank than lane b + 1's); lane b of wave 0 then runs down block b for the
// in-block prefix of z - offset, wave 1 for its square, wave 2 for the valid count -- chains of 64 steps; lane 0 of each of these
// waves adds the 64 block totals to its running offset, which it carries from chunk to chunk of the row -- ceil(ncol / 64) steps
// per row; and all four waves write offset + in-block prefix with 64 consecutive elements per store.
// focal_cols_kernel (per radius, square).  Lane = column, so every load and store of a wave is 64 consecutive elements by
// itself: a thread forms the row-window sums W of its column for the 64 rows of one aligned block from the row prefixes and
// writes their in-block prefix and the block's total.  focal_col_offsets_kernel runs a thread down the block totals of a
// column (ceil(nrow / 64) steps), starting from the offsets a host band carries in.  focal_square_kernel forms the window's
// sums from two prefix values per plane and makes the statistics; focal_circle_kernel adds the 2 R + 1 row-window sums, the
// half widths from a table made on the device once per radius.  The min / max family of a square window has kernels of its own,
// further down: running minima on the same aligned blocks, exact in any order.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <mutex>
#include "ensemble_int.h"
#include "focal_rule.h"

namespace mhs {

constexpr int FOC_NT = 256;
constexpr int FOC_B = FOCAL_B;                       // 64: one block per lane of a wave
constexpr int FOC_PAD = FOC_B + 1;                   // LDS doubles per block
constexpr int FOC_CHUNK = 64 * FOC_B;                // cells of a row a workgroup stages at a time
constexpr size_t FOC_LDS = (size_t)64 * FOC_PAD * (3 * sizeof(double) + sizeof(int));
static_assert(FOC_B == 64, "a lane owns a block: B is the wave size");
static_assert(FOCAL_B == MHS_FOCAL_BLOCK && FOCAL_SQUARE == MHS_FOCAL_SQUARE && FOCAL_CIRCLE == MHS_FOCAL_CIRCLE, "focal_rule.h restates the header's constants");
static_assert(FOC_LDS <= LDS_LIMIT, "the chunk and its three prefixes must fit");

struct FocalPlane {
    const void *plane;       // element (0, 0) of the raster's plane (a row band's buffer: moved back to absolute row 0)
    int64_t ld;
    int nrow, ncol;
    double nodata;
    int has_nodata;
    double offset;
};

// the row prefixes of the raster's rows [row0, ...), all columns: element (r, c) at (r - row0) * ncol + c
struct FocalRows {
    double *p1, *p2;
    int *pn;
    int row0;
};

// the column phase of one radius: rows [qa, qb), qa a multiple of B, columns [c0, c0 + nc); element (r, c) at (r - qa) * nc + c - c0,
// block k's entry of column c at (k - qa / B) * nc + c - c0
struct FocalCols {
    double *q1, *q2, *t1, *t2, *o1, *o2;
    int64_t *qn, *tn, *on;
    int qa, qb, c0, nc;
};

template <typename T>
__global__ __launch_bounds__(FOC_NT) void focal_rows_kernel(const FocalPlane g, const FocalRows P, const int ra, const int rb) {
    extern __shared__ __align__(16) unsigned char focal_sm[];
    double *X = (double *)focal_sm, *I1 = X + 64 * FOC_PAD, *I2 = I1 + 64 * FOC_PAD;
    int *In = (int *)(I2 + 64 * FOC_PAD);
    __shared__ double tot_d[2][64], off_d[2][64];
    __shared__ int tot_n[64], off_n[64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool has_nd = g.has_nodata != 0;
    const T *plane = (const T *)g.plane;
    for (int r = ra + (int)blockIdx.x; r < rb; r += (int)gridDim.x) {
        double run_d = 0.0;                                       // lane 0 of waves 0 and 1: the offset of the next block
        int run_n = 0;                                            // lane 0 of wave 2
        const T *row = plane + (int64_t)r * g.ld;
        const int64_t at = (int64_t)(r - P.row0) * g.ncol;
        for (int ch0 = 0; ch0 < g.ncol; ch0 += FOC_CHUNK) {
            const int nblk = min(64, (g.ncol - ch0 + FOC_B - 1) / FOC_B);
            for (int e = threadIdx.x; e < FOC_CHUNK; e += FOC_NT) {
                const int col = ch0 + e;
                double v = (double)NAN;                           // NA, and what lies past the row's end
                if (col < g.ncol) {
                    const double z = (double)row[col];
                    if (!focal_na(z, has_nd, g.nodata)) v = z - g.offset;
                }
                X[(e >> 6) * FOC_PAD + (e & 63)] = v;
            }
            __syncthreads();
            if (lane < nblk) {
                const double *x = X + lane * FOC_PAD;
                if (wave == 0) {
                    double s = 0.0;
                    for (int i = 0; i < FOC_B; ++i) {
                        const double v = x[i], a = v == v ? v : 0.0;
                        s = i == 0 ? a : s + a;
                        I1[lane * FOC_PAD + i] = s;
                    }
                    tot_d[0][lane] = s;
                } else if (wave == 1) {
                    double s = 0.0;
                    for (int i = 0; i < FOC_B; ++i) {
                        const double v = x[i], a = v == v ? v * v : 0.0;
                        s = i == 0 ? a : s + a;
                        I2[lane * FOC_PAD + i] = s;
                    }
                    tot_d[1][lane] = s;
                } else if (wave == 2) {
                    int s = 0;
                    for (int i = 0; i < FOC_B; ++i) {
                        const double v = x[i];
                        s += v == v ? 1 : 0;
                        In[lane * FOC_PAD + i] = s;
                    }
                    tot_n[lane] = s;
                }
            }
            __syncthreads();
            if (lane == 0 && wave < 2) {
                for (int k = 0; k < nblk; ++k) { off_d[wave][k] = run_d; run_d = run_d + tot_d[wave][k]; }
            } else if (lane == 0 && wave == 2) {
                for (int k = 0; k < nblk; ++k) { off_n[k] = run_n; run_n += tot_n[k]; }
            }
            __syncthreads();
            for (int e = threadIdx.x; e < FOC_CHUNK; e += FOC_NT) {
                const int col = ch0 + e;
                if (col < g.ncol) {
                    const int b = e >> 6, i = b * FOC_PAD + (e & 63);
                    P.p1[at + col] = off_d[0][b] + I1[i];
                    P.p2[at + col] = off_d[1][b] + I2[i];
                    P.pn[at + col] = off_n[b] + In[i];
                }
            }
            __syncthreads();                                      // the next chunk overwrites the LDS
        }
    }
}

// the sums of row r's columns max(c - w, 0) .. min(c + w, ncol - 1)
struct RowSums { double s1, s2; int n; };
__device__ inline RowSums focal_row_sums(const FocalRows &P, int ncol, int r, int c, int w) {
    const int64_t at = (int64_t)(r - P.row0) * ncol;
    const int hi = min((int64_t)c + w, (int64_t)ncol - 1), lo = (int64_t)c - w > 0 ? c - w : 0;
    RowSums s{P.p1[at + hi], P.p2[at + hi], P.pn[at + hi]};
    if (lo > 0) { s.s1 = s.s1 - P.p1[at + lo - 1]; s.s2 = s.s2 - P.p2[at + lo - 1]; s.n -= P.pn[at + lo - 1]; }
    else { s.s1 = s.s1 - 0.0; s.s2 = s.s2 - 0.0; }
    return s;
}

__global__ __launch_bounds__(FOC_NT) void focal_cols_kernel(const FocalRows P, const FocalCols Q, const int ncol, const int R) {
    const int tiles_x = (Q.nc + FOC_NT - 1) / FOC_NT;
    const int64_t n_items = (int64_t)tiles_x * ((Q.qb - Q.qa + FOC_B - 1) / FOC_B);
    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int kb = (int)(item / tiles_x), x = (int)(item % tiles_x) * FOC_NT + (int)threadIdx.x;
        if (x >= Q.nc) continue;
        const int c = Q.c0 + x, r_lo = Q.qa + kb * FOC_B, r_hi = min(Q.qb, r_lo + FOC_B);
        double s1 = 0.0, s2 = 0.0;
        int64_t sn = 0;
        for (int r = r_lo; r < r_hi; ++r) {
            const RowSums w = focal_row_sums(P, ncol, r, c, R);
            s1 = r == r_lo ? w.s1 : s1 + w.s1;
            s2 = r == r_lo ? w.s2 : s2 + w.s2;
            sn += w.n;
            const int64_t at = (int64_t)(r - Q.qa) * Q.nc + x;
            Q.q1[at] = s1; Q.q2[at] = s2; Q.qn[at] = sn;
        }
        const int64_t bt = (int64_t)kb * Q.nc + x;
        Q.t1[bt] = s1; Q.t2[bt] = s2; Q.tn[bt] = sn;
    }
}

// carry: the offsets of the first block, three arrays of nc (double, double, int64) one behind the other, or NULL: zero
__global__ __launch_bounds__(FOC_NT) void focal_col_offsets_kernel(const FocalCols Q, const char *carry) {
    const int x = (int)(blockIdx.x * FOC_NT + threadIdx.x);
    if (x >= Q.nc) return;
    const int nblk = (Q.qb - Q.qa + FOC_B - 1) / FOC_B;
    double r1 = 0.0, r2 = 0.0;
    int64_t rn = 0;
    if (carry) {
        r1 = ((const double *)carry)[x];
        r2 = ((const double *)carry)[Q.nc + x];
        rn = ((const int64_t *)carry)[2 * (int64_t)Q.nc + x];
    }
    for (int k = 0; k < nblk; ++k) {
        const int64_t at = (int64_t)k * Q.nc + x;
        Q.o1[at] = r1; Q.o2[at] = r2; Q.on[at] = rn;
        r1 = r1 + Q.t1[at]; r2 = r2 + Q.t2[at]; rn += Q.tn[at];
    }
}

// ---- the min / max family of a square window: focal_rule.h's running minimum on two channels, z and -z (+inf at NA cells), so
// the maximum is minus the minimum of the second.  Rows first (radius-independent tables, then the row-window minima of a radius),
// then the same down the columns of those.
constexpr int FOCM_BLK = 32;                         // blocks of a row a workgroup stages at a time: five arrays of them in LDS
constexpr int FOCM_CHUNK = FOCM_BLK * FOC_B;
constexpr size_t FOCM_LDS = (size_t)5 * FOCM_BLK * FOC_PAD * sizeof(double);
static_assert(FOCM_LDS <= LDS_LIMIT, "the chunk and its four running minima must fit");

// along the rows [row0, ...), all columns: pm / sm of channel ch at ch * ch_stride + (r - row0) * ncol + c; the table's level j at
// j * tab_lev + ch * tab_ch + (r - row0) * nb + k
struct FocalMmRows {
    double *pm, *sm, *tab;
    int64_t ch_stride, tab_ch, tab_lev;
    int row0, nb;
};
// of one radius, rows [qa, qb) and the window's columns: rm (the row-window minima), pm, sm of channel ch at ch * ch_stride +
// (r - qa) * nc + x; the table's level j at j * tab_lev + ch * tab_ch + k * nc + x
struct FocalMmCols {
    double *rm, *pm, *sm, *tab;
    int64_t ch_stride, tab_ch, tab_lev;
    int qa, qb, c0, nc;
};

template <typename T>
__global__ __launch_bounds__(FOC_NT) void focal_mm_rows_kernel(const FocalPlane g, const FocalMmRows M, const int ra, const int rb) {
    extern __shared__ __align__(16) unsigned char focal_sm[];
    double *X = (double *)focal_sm;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double *mine = X + (1 + wave) * FOCM_BLK * FOC_PAD;           // wave 0: pm of z, 1: sm of z, 2: pm of -z, 3: sm of -z
    const bool has_nd = g.has_nodata != 0;
    const double inf = (double)INFINITY;
    for (int r = ra + (int)blockIdx.x; r < rb; r += (int)gridDim.x) {
        const T *row = (const T *)g.plane + (int64_t)r * g.ld;
        const int64_t at = (int64_t)(r - M.row0) * g.ncol;
        for (int ch0 = 0; ch0 < g.ncol; ch0 += FOCM_CHUNK) {
            const int nblk = min(FOCM_BLK, (g.ncol - ch0 + FOC_B - 1) / FOC_B);
            for (int e = threadIdx.x; e < FOCM_CHUNK; e += FOC_NT) {
                const int col = ch0 + e;
                double v = (double)NAN;
                if (col < g.ncol) {
                    const double z = (double)row[col];
                    if (!focal_na(z, has_nd, g.nodata)) v = z;
                }
                X[(e >> 6) * FOC_PAD + (e & 63)] = v;
            }
            __syncthreads();
            if (lane < nblk) {
                const double *x = X + lane * FOC_PAD;
                double *o = mine + lane * FOC_PAD;
                const bool neg = wave >= 2, back = wave & 1;
                double m = inf;
                for (int i = 0; i < FOC_B; ++i) {
                    const int ii = back ? FOC_B - 1 - i : i;
                    const double v = x[ii], val = v == v ? (neg ? -v : v) : inf;
                    m = val < m ? val : m;
                    o[ii] = m;
                }
                if (!back) M.tab[(neg ? M.tab_ch : 0) + (int64_t)(r - M.row0) * M.nb + ch0 / FOC_B + lane] = m;
            }
            __syncthreads();
            for (int e = threadIdx.x; e < FOCM_CHUNK; e += FOC_NT) {
                const int col = ch0 + e;
                if (col < g.ncol) {
                    const int i = (e >> 6) * FOC_PAD + (e & 63);
                    const double *a = X + FOCM_BLK * FOC_PAD;
                    M.pm[at + col] = a[i];
                    M.sm[at + col] = a[FOCM_BLK * FOC_PAD + i];
                    M.pm[M.ch_stride + at + col] = a[2 * FOCM_BLK * FOC_PAD + i];
                    M.sm[M.ch_stride + at + col] = a[3 * FOCM_BLK * FOC_PAD + i];
                }
            }
            __syncthreads();
        }
    }
}

// one level of a table from the level below: element (o, k, i) of outer x nk x inner takes the minimum with element (o, k + half, i)
__global__ __launch_bounds__(FOC_NT) void focal_mm_level_kernel(const double *__restrict__ prev, double *__restrict__ next, const int64_t total,
                                                                const int nk, const int64_t inner, const int half) {
    for (int64_t idx = (int64_t)blockIdx.x * FOC_NT + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * FOC_NT) {
        const int k = (int)(idx / inner % nk);
        double a = prev[idx];
        if (k + half < nk) { const double b = prev[idx + (int64_t)half * inner]; a = b < a ? b : a; }
        next[idx] = a;
    }
}

template <typename T>
struct MmRowAcc {
    const double *pm_, *sm_, *tab_;
    int64_t tab_lev;
    const T *row;
    bool neg, has_nd;
    double nodata;
    __device__ double pm(int64_t i) const { return pm_[i]; }
    __device__ double sm(int64_t i) const { return sm_[i]; }
    __device__ double table(int j, int64_t k) const { return tab_[(int64_t)j * tab_lev + k]; }
    __device__ double raw(int64_t i) const {
        const double z = (double)row[i];
        return focal_na(z, has_nd, nodata) ? (double)INFINITY : neg ? -z : z;
    }
};
struct MmColAcc {
    const double *pm_, *sm_, *rm_, *tab_;
    int64_t stride, tab_lev;
    __device__ double pm(int64_t i) const { return pm_[i * stride]; }
    __device__ double sm(int64_t i) const { return sm_[i * stride]; }
    __device__ double raw(int64_t i) const { return rm_[i * stride]; }
    __device__ double table(int j, int64_t k) const { return tab_[(int64_t)j * tab_lev + k * stride]; }
};

// the row-window minima of one radius: tiles of 4 rows x 64 columns of the rows [qa, qb) and the window's columns
template <typename T>
__global__ __launch_bounds__(FOC_NT) void focal_mm_rowwin_kernel(const FocalPlane g, const FocalMmRows M, const FocalMmCols C, const int R) {
    const int tiles_x = (C.nc + 63) / 64, nr = C.qb - C.qa;
    const int64_t n_tiles = (int64_t)tiles_x * ((nr + 3) / 4);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int row = (int)(tile / tiles_x) * 4 + (int)(threadIdx.x >> 6), x = (int)(tile % tiles_x) * 64 + (int)(threadIdx.x & 63);
        if (row >= nr || x >= C.nc) continue;
        const int r = C.qa + row, c = C.c0 + x;
        const int64_t hi = min((int64_t)c + R, (int64_t)g.ncol - 1), lo = max((int64_t)c - R, (int64_t)0);
        const int64_t at = (int64_t)(r - M.row0) * g.ncol, tat = (int64_t)(r - M.row0) * M.nb;
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) {
            const MmRowAcc<T> acc{M.pm + ch * M.ch_stride + at, M.sm + ch * M.ch_stride + at, M.tab + ch * M.tab_ch + tat, M.tab_lev,
                                  (const T *)g.plane + (int64_t)r * g.ld, ch == 1, g.has_nodata != 0, g.nodata};
            C.rm[ch * C.ch_stride + (int64_t)row * C.nc + x] = focal_range_min(acc, g.ncol, lo, hi);
        }
    }
}

// lane = column: the running minima down the 64 rows of one aligned block of the row-window minima, and the block's minimum
__global__ __launch_bounds__(FOC_NT) void focal_mm_cols_kernel(const FocalMmCols C) {
    const int tiles_x = (C.nc + FOC_NT - 1) / FOC_NT;
    const int64_t n_items = (int64_t)tiles_x * ((C.qb - C.qa + FOC_B - 1) / FOC_B);
    const double inf = (double)INFINITY;
    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int kb = (int)(item / tiles_x), x = (int)(item % tiles_x) * FOC_NT + (int)threadIdx.x;
        if (x >= C.nc) continue;
        const int i_lo = kb * FOC_B, i_hi = min(C.qb - C.qa, i_lo + FOC_B);
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) {
            const int64_t base = ch * C.ch_stride + x;
            double m = inf;
            for (int i = i_lo; i < i_hi; ++i) {
                const double v = C.rm[base + (int64_t)i * C.nc];
                m = v < m ? v : m;
                C.pm[base + (int64_t)i * C.nc] = m;
            }
            C.tab[ch * C.tab_ch + (int64_t)kb * C.nc + x] = m;
            m = inf;
            for (int i = i_hi - 1; i >= i_lo; --i) {
                const double v = C.rm[base + (int64_t)i * C.nc];
                m = v < m ? v : m;
                C.sm[base + (int64_t)i * C.nc] = m;
            }
        }
    }
}

// what the two output kernels share: the statistics of one cell into the planes of the mask
template <typename O>
__device__ inline void focal_emit(unsigned mask, bool fill_na, int64_t n, double s1, double s2, double offset, bool has_e, double e,
                                  double mn, double mx, O *dst, int64_t plane_stride) {
    double o[FS_NSTATS];
    const bool made = has_e || fill_na;
    if (made) focal_stats(mask, n, s1, s2, offset, has_e, e, mn, mx, o);
#pragma unroll
    for (int k = 0; k < FS_NSTATS; ++k)
        if (mask & (1u << k)) {
            const bool na = !made || (!has_e && (FS_NEEDS_CENTRE >> k & 1u));
            *dst = (O)(na ? (double)NAN : o[k]);
            dst += plane_stride;
        }
}

struct FocalOut { int r0, nr, c0, nc; unsigned mask; int fill_na; };

template <typename T>
__device__ inline bool focal_centre(const FocalPlane &g, int r, int c, double &e) {
    e = (double)((const T *)g.plane)[(int64_t)r * g.ld + c];
    return !focal_na(e, g.has_nodata != 0, g.nodata);
}

// tiles of 4 rows x 64 columns: wave w the row w of the tile
template <typename T, typename O>
__global__ __launch_bounds__(FOC_NT) void focal_square_kernel(const FocalPlane g, const FocalCols Q, const FocalMmCols C, const FocalOut w, const int R,
                                                              O *__restrict__ out, const int64_t ld_out, const int64_t plane_stride) {
    const int tiles_x = (w.nc + 63) / 64;
    const int64_t n_tiles = (int64_t)tiles_x * ((w.nr + 3) / 4);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int row = (int)(tile / tiles_x) * 4 + (int)(threadIdx.x >> 6), col = (int)(tile % tiles_x) * 64 + (int)(threadIdx.x & 63);
        if (row >= w.nr || col >= w.nc) continue;
        const int r = w.r0 + row, c = w.c0 + col, x = c - Q.c0;
        const int rh = min((int64_t)r + R, (int64_t)g.nrow - 1), rl = (int64_t)r - R > 0 ? r - R : 0;
        const int64_t ah = (int64_t)(rh - Q.qa) * Q.nc + x, bh = (int64_t)((rh - Q.qa) / FOC_B) * Q.nc + x;
        double s1 = Q.o1[bh] + Q.q1[ah], s2 = Q.o2[bh] + Q.q2[ah];
        int64_t n = Q.on[bh] + Q.qn[ah];
        if (rl > 0) {
            const int64_t al = (int64_t)(rl - 1 - Q.qa) * Q.nc + x, bl = (int64_t)((rl - 1 - Q.qa) / FOC_B) * Q.nc + x;
            s1 = s1 - (Q.o1[bl] + Q.q1[al]); s2 = s2 - (Q.o2[bl] + Q.q2[al]); n -= Q.on[bl] + Q.qn[al];
        } else { s1 = s1 - 0.0; s2 = s2 - 0.0; }
        double mn = 0.0, mx = 0.0;
        if (w.mask & FS_MINMAX_FAMILY) {
            const MmColAcc a0{C.pm + x, C.sm + x, C.rm + x, C.tab + x, C.nc, C.tab_lev};
            const MmColAcc a1{C.pm + C.ch_stride + x, C.sm + C.ch_stride + x, C.rm + C.ch_stride + x, C.tab + C.tab_ch + x, C.nc, C.tab_lev};
            mn = focal_range_min(a0, C.qb - C.qa, rl - C.qa, rh - C.qa);
            mx = -focal_range_min(a1, C.qb - C.qa, rl - C.qa, rh - C.qa);
        }
        double e;
        const bool has_e = focal_centre<T>(g, r, c, e);
        focal_emit<O>(w.mask, w.fill_na != 0, n, s1, s2, g.offset, has_e, e, mn, mx, out + (int64_t)row * ld_out + col, plane_stride);
    }
}

__global__ void focal_half_width_kernel(const int R, const int n, int *hw) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) hw[i] = focal_half_width(R, i);
}

// hw[0 .. min(R, nrow - 1)]: the half widths of the rows that can lie inside the raster
template <typename T, typename O>
__global__ __launch_bounds__(FOC_NT) void focal_circle_kernel(const FocalPlane g, const FocalRows P, const FocalOut w, const int R,
                                                              const int *__restrict__ hw, O *__restrict__ out, const int64_t ld_out,
                                                              const int64_t plane_stride) {
    const int tiles_x = (w.nc + 63) / 64;
    const int64_t n_tiles = (int64_t)tiles_x * ((w.nr + 3) / 4);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int row = (int)(tile / tiles_x) * 4 + (int)(threadIdx.x >> 6), col = (int)(tile % tiles_x) * 64 + (int)(threadIdx.x & 63);
        if (row >= w.nr || col >= w.nc) continue;
        const int r = w.r0 + row, c = w.c0 + col;
        const int rh = min((int64_t)r + R, (int64_t)g.nrow - 1), rl = (int64_t)r - R > 0 ? r - R : 0;
        double s1 = 0.0, s2 = 0.0;
        int64_t n = 0;
        for (int rr = rl; rr <= rh; ++rr) {
            const RowSums s = focal_row_sums(P, g.ncol, rr, c, hw[rr < r ? r - rr : rr - r]);
            s1 = s1 + s.s1; s2 = s2 + s.s2; n += s.n;
        }
        double e;
        const bool has_e = focal_centre<T>(g, r, c, e);
        focal_emit<O>(w.mask, w.fill_na != 0, n, s1, s2, g.offset, has_e, e, 0.0, 0.0, out + (int64_t)row * ld_out + col, plane_stride);
    }
}

// what a call makes
struct FocalJob {
    FocalPlane g;
    int dtype;
    int r0, r1, c0, c1;      // the output window
    int n_rad, radius[MHS_FOCAL_MAX_RADII];
    int shape;
    unsigned mask;
    int n_stats, fill_na, out_dtype;
    size_t out_esz;
};

static int focal_popcount(unsigned m) { int n = 0; for (; m; m &= m - 1) ++n; return n; }
static size_t foc_up(size_t b) { return (b + 255) & ~(size_t)255; }
static unsigned foc_grid(int64_t items) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(items, (int64_t)1 << 20)); }
static size_t focal_carry_bytes(const FocalJob &job) { return foc_up((size_t)(job.c1 - job.c0) * 24); }      // of one radius

// first row of the column phase of the output rows from b0: row 0, or -- carried offsets -- the start of the block of row
// b0 - R - 1, the row whose prefix the window of row b0 subtracts
static int focal_qa(int b0, int R, bool carried) { return carried ? (int)(std::max<int64_t>(0, (int64_t)b0 - R - 1) / FOC_B) * FOC_B : 0; }
static int focal_qb(const FocalJob &job, int b1, int R) { return (int)std::min<int64_t>(job.g.nrow, (int64_t)b1 + R); }
// the rows of the plane the output rows [b0, b1) read
static void focal_rows_read(const FocalJob &job, int b0, int b1, bool carried, int *ra, int *rb) {
    *ra = job.g.nrow; *rb = 0;
    for (int k = 0; k < job.n_rad; ++k) {
        const int R = job.radius[k];
        const int a = job.shape == FOCAL_SQUARE ? focal_qa(b0, R, carried) : (int)std::max<int64_t>(0, (int64_t)b0 - R);
        *ra = std::min(*ra, a); *rb = std::max(*rb, focal_qb(job, b1, R));
    }
}

template <typename T, typename O>
static void focal_launch_out(const FocalJob &job, const FocalRows &P, const FocalCols &Q, const FocalMmCols &C, const FocalOut &w, int R, const int *hw,
                             void *out, int64_t ld, int64_t ps, hipStream_t st) {
    const int64_t n_tiles = (int64_t)((w.nc + 63) / 64) * ((w.nr + 3) / 4);
    if (job.shape == FOCAL_SQUARE)
        hipLaunchKernelGGL((focal_square_kernel<T, O>), dim3(foc_grid(n_tiles)), dim3(FOC_NT), 0, st, job.g, Q, C, w, R, (O *)out, ld, ps);
    else
        hipLaunchKernelGGL((focal_circle_kernel<T, O>), dim3(foc_grid(n_tiles)), dim3(FOC_NT), 0, st, job.g, P, w, R, hw, (O *)out, ld, ps);
}

template <typename T>
static int focal_launch_rows(const FocalJob &job, const FocalRows &P, int ra, int rb, hipStream_t st) {
    if (FOC_LDS > (size_t)64 * 1024)
        MHS_HIP(hipFuncSetAttribute((const void *)focal_rows_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FOC_LDS));
    const int n_cu = ctx().n_cu > 0 ? ctx().n_cu : 256;
    hipLaunchKernelGGL((focal_rows_kernel<T>), dim3((unsigned)std::min<int64_t>(rb - ra, (int64_t)n_cu * 4)), dim3(FOC_NT), FOC_LDS, st, job.g, P, ra, rb);
    return MHS_OK;
}

template <typename T>
static int focal_launch_mm_rows(const FocalJob &job, const FocalMmRows &M, int ra, int rb, hipStream_t st) {
    if (FOCM_LDS > (size_t)64 * 1024)
        MHS_HIP(hipFuncSetAttribute((const void *)focal_mm_rows_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FOCM_LDS));
    const int n_cu = ctx().n_cu > 0 ? ctx().n_cu : 256;
    hipLaunchKernelGGL((focal_mm_rows_kernel<T>), dim3((unsigned)std::min<int64_t>(rb - ra, (int64_t)n_cu * 4)), dim3(FOC_NT), FOCM_LDS, st, job.g, M, ra, rb);
    return MHS_OK;
}

// The output rows [b0, b1) of the window's columns, every radius, into out; job.g.plane is the plane moved back to absolute row
// 0 and holds the rows focal_rows_read names.  carry_in / carry_out (host bands, square): the column offsets of block
// focal_qa(b0) / B per radius as they come in (NULL: this piece starts at row 0) and those of block focal_qa(next_b0) / B to hand on.
static int focal_run(const FocalJob &job, int b0, int b1, void *out, int64_t ld, int64_t ps, hipStream_t st, const char *carry_in,
                     char *carry_out, int next_b0, bool carried) {
    const int nc = job.c1 - job.c0, ncol = job.g.ncol;
    if (b1 <= b0 || nc == 0) return MHS_OK;
    int ra, rb;
    focal_rows_read(job, b0, b1, carried, &ra, &rb);
    const bool square = job.shape == FOCAL_SQUARE;
    size_t q_rows = 0, q_blk = 0, hw_n = 0;
    for (int k = 0; k < job.n_rad; ++k) {
        if (square) {
            const size_t rows = (size_t)(focal_qb(job, b1, job.radius[k]) - focal_qa(b0, job.radius[k], carried));
            q_rows = std::max(q_rows, rows); q_blk = std::max(q_blk, (rows + FOC_B - 1) / FOC_B);
        } else hw_n = std::max(hw_n, (size_t)std::min(job.radius[k], job.g.nrow - 1) + 1);
    }
    const size_t cells = (size_t)(rb - ra) * ncol;
    const size_t b_p8 = foc_up(cells * 8), b_p4 = foc_up(cells * 4), b_q = foc_up(q_rows * nc * 8), b_t = foc_up(q_blk * nc * 8), b_hw = foc_up(hw_n * 4);
    const bool mm = (job.mask & FS_MINMAX_FAMILY) != 0;          // square only (focal_check)
    const int nbc = (ncol + FOC_B - 1) / FOC_B, lev_r = focal_levels(nbc), lev_c = focal_levels((int64_t)q_blk);
    const size_t b_m = mm ? foc_up(2 * cells * 8) : 0, b_mt = mm ? foc_up((size_t)lev_r * 2 * (rb - ra) * nbc * 8) : 0;
    const size_t b_mq = mm ? foc_up(2 * q_rows * nc * 8) : 0, b_ct = mm ? foc_up((size_t)lev_c * 2 * q_blk * nc * 8) : 0;
    const size_t total = 2 * b_p8 + b_p4 + 3 * b_q + 6 * b_t + b_hw + 2 * b_m + b_mt + 3 * b_mq + b_ct;
    char *base = nullptr;
    MHS_HIP(hipMallocAsync((void **)&base, total, st));
    struct Release { char *p; hipStream_t s; ~Release() { (void)hipFreeAsync(p, s); } } release{base, st};      // behind the last kernel
    char *at = base;
    auto take = [&](size_t b) { char *p = at; at += b; return p; };
    FocalRows P{(double *)take(b_p8), (double *)take(b_p8), (int *)take(b_p4), ra};
    FocalCols Q{};
    Q.q1 = (double *)take(b_q); Q.q2 = (double *)take(b_q); Q.qn = (int64_t *)take(b_q);
    Q.t1 = (double *)take(b_t); Q.t2 = (double *)take(b_t); Q.tn = (int64_t *)take(b_t);
    Q.o1 = (double *)take(b_t); Q.o2 = (double *)take(b_t); Q.on = (int64_t *)take(b_t);
    int *hw = (int *)take(b_hw);
    FocalMmRows M{(double *)take(b_m), (double *)take(b_m), (double *)take(b_mt), (int64_t)cells, (int64_t)(rb - ra) * nbc, 2 * (int64_t)(rb - ra) * nbc, ra, nbc};
    FocalMmCols C{};
    C.rm = (double *)take(b_mq); C.pm = (double *)take(b_mq); C.sm = (double *)take(b_mq); C.tab = (double *)take(b_ct);
    int rc = job.dtype == MHS_F64 ? focal_launch_rows<double>(job, P, ra, rb, st)
           : job.dtype == MHS_F32 ? focal_launch_rows<float>(job, P, ra, rb, st) : focal_launch_rows<short>(job, P, ra, rb, st);
    if (rc) return rc;
    if (mm) {
        rc = job.dtype == MHS_F64 ? focal_launch_mm_rows<double>(job, M, ra, rb, st)
           : job.dtype == MHS_F32 ? focal_launch_mm_rows<float>(job, M, ra, rb, st) : focal_launch_mm_rows<short>(job, M, ra, rb, st);
        if (rc) return rc;
        for (int j = 1; j < lev_r; ++j)
            hipLaunchKernelGGL(focal_mm_level_kernel, dim3(foc_grid((M.tab_lev + FOC_NT - 1) / FOC_NT)), dim3(FOC_NT), 0, st, M.tab + (j - 1) * M.tab_lev,
                               M.tab + j * M.tab_lev, M.tab_lev, nbc, (int64_t)1, 1 << (j - 1));
    }
    const FocalOut w{b0, b1 - b0, job.c0, nc, job.mask, job.fill_na};
    const bool f64 = job.out_dtype == MHS_F64;
    for (int k = 0; k < job.n_rad; ++k) {
        const int R = job.radius[k];
        if (square) {
            Q.qa = focal_qa(b0, R, carried); Q.qb = focal_qb(job, b1, R); Q.c0 = job.c0; Q.nc = nc;
            const int nblk = (Q.qb - Q.qa + FOC_B - 1) / FOC_B;
            hipLaunchKernelGGL(focal_cols_kernel, dim3(foc_grid((int64_t)((nc + FOC_NT - 1) / FOC_NT) * nblk)), dim3(FOC_NT), 0, st, P, Q, ncol, R);
            hipLaunchKernelGGL(focal_col_offsets_kernel, dim3((unsigned)((nc + FOC_NT - 1) / FOC_NT)), dim3(FOC_NT), 0, st, Q,
                               carry_in ? carry_in + (size_t)k * focal_carry_bytes(job) : nullptr);
            if (carry_out) {                                     // the offsets of the block the next piece starts in
                const size_t blk = (size_t)(focal_qa(next_b0, R, true) - Q.qa) / FOC_B * nc;
                char *dst = carry_out + (size_t)k * focal_carry_bytes(job);
                MHS_HIP(hipMemcpyAsync(dst, Q.o1 + blk, (size_t)nc * 8, hipMemcpyDeviceToDevice, st));
                MHS_HIP(hipMemcpyAsync(dst + (size_t)nc * 8, Q.o2 + blk, (size_t)nc * 8, hipMemcpyDeviceToDevice, st));
                MHS_HIP(hipMemcpyAsync(dst + (size_t)nc * 16, Q.on + blk, (size_t)nc * 8, hipMemcpyDeviceToDevice, st));
            }
            if (mm) {
                const int rows = Q.qb - Q.qa;
                C.qa = Q.qa; C.qb = Q.qb; C.c0 = job.c0; C.nc = nc;
                C.ch_stride = (int64_t)rows * nc; C.tab_ch = (int64_t)nblk * nc; C.tab_lev = 2 * C.tab_ch;
                const unsigned tiles = foc_grid((int64_t)((nc + 63) / 64) * ((rows + 3) / 4));
                if (job.dtype == MHS_F64) hipLaunchKernelGGL(focal_mm_rowwin_kernel<double>, dim3(tiles), dim3(FOC_NT), 0, st, job.g, M, C, R);
                else if (job.dtype == MHS_F32) hipLaunchKernelGGL(focal_mm_rowwin_kernel<float>, dim3(tiles), dim3(FOC_NT), 0, st, job.g, M, C, R);
                else hipLaunchKernelGGL(focal_mm_rowwin_kernel<short>, dim3(tiles), dim3(FOC_NT), 0, st, job.g, M, C, R);
                hipLaunchKernelGGL(focal_mm_cols_kernel, dim3(foc_grid((int64_t)((nc + FOC_NT - 1) / FOC_NT) * nblk)), dim3(FOC_NT), 0, st, C);
                for (int j = 1; j < focal_levels(nblk); ++j)
                    hipLaunchKernelGGL(focal_mm_level_kernel, dim3(foc_grid((C.tab_lev + FOC_NT - 1) / FOC_NT)), dim3(FOC_NT), 0, st, C.tab + (j - 1) * C.tab_lev,
                                       C.tab + j * C.tab_lev, C.tab_lev, nblk, (int64_t)nc, 1 << (j - 1));
            }
        } else {
            const int n = std::min(R, job.g.nrow - 1) + 1;
            hipLaunchKernelGGL(focal_half_width_kernel, dim3((unsigned)((n + FOC_NT - 1) / FOC_NT)), dim3(FOC_NT), 0, st, R, n, hw);
        }
        void *dst = (char *)out + (size_t)k * job.n_stats * (size_t)ps * job.out_esz;
        if (job.dtype == MHS_F64) f64 ? focal_launch_out<double, double>(job, P, Q, C, w, R, hw, dst, ld, ps, st) : focal_launch_out<double, float>(job, P, Q, C, w, R, hw, dst, ld, ps, st);
        else if (job.dtype == MHS_F32) f64 ? focal_launch_out<float, double>(job, P, Q, C, w, R, hw, dst, ld, ps, st) : focal_launch_out<float, float>(job, P, Q, C, w, R, hw, dst, ld, ps, st);
        else f64 ? focal_launch_out<short, double>(job, P, Q, C, w, R, hw, dst, ld, ps, st) : focal_launch_out<short, float>(job, P, Q, C, w, R, hw, dst, ld, ps, st);
    }
    MHS_HIP(hipGetLastError());
    return MHS_OK;
}

#define FOC_REQUIRE(cond, ...)                                             \
    do {                                                                   \
        if (!(cond)) { set_error(__VA_ARGS__); return MHS_ERR_INVALID; }    \
    } while (0)

// every check of a focal call, before any device call
static int focal_check(const char *fn, const mhs_grid *grid, const mhs_stack *s, int layer, const int *radii, int n_radii, int shape,
                       unsigned stats, int fill_na, double offset, int64_t r0, int64_t r1, int64_t c0, int64_t c1, const void *out, int out_dtype,
                       int64_t ld, int64_t plane_stride, FocalJob *job) {
    FOC_REQUIRE(grid && s, "%s: NULL argument (grid or stack)", fn);
    FOC_REQUIRE(grid->nrow > 0 && grid->ncol > 0 && grid->nrow < (1LL << 30) && grid->ncol < (1LL << 30), "%s: bad grid geometry (nrow, ncol must be in 1 .. 2^30)", fn);
    FOC_REQUIRE(0 <= r0 && r0 <= r1 && r1 <= grid->nrow && 0 <= c0 && c0 <= c1 && c1 <= grid->ncol, "%s: window outside the grid", fn);
    FOC_REQUIRE(s->data, "%s: stack data is NULL", fn);
    FOC_REQUIRE(s->dtype == MHS_F64 || s->dtype == MHS_F32 || s->dtype == MHS_I16, "%s: bad stack dtype", fn);
    FOC_REQUIRE(layer >= 0 && layer < s->n_layers, "%s: layer %d is not one of the stack's %d layers", fn, layer, s->n_layers);
    FOC_REQUIRE(s->ld >= grid->ncol && (s->n_layers == 1 || s->plane_stride >= s->ld * (grid->nrow - 1) + grid->ncol), "%s: stack strides smaller than the grid", fn);
    FOC_REQUIRE(radii, "%s: radii is NULL", fn);
    FOC_REQUIRE(n_radii >= 1 && n_radii <= MHS_FOCAL_MAX_RADII, "%s: n_radii must be in 1 .. %d (MHS_FOCAL_MAX_RADII), got %d", fn, MHS_FOCAL_MAX_RADII, n_radii);
    const int64_t r_max = std::max(grid->nrow, grid->ncol);
    for (int k = 0; k < n_radii; ++k)
        FOC_REQUIRE(radii[k] >= 1 && radii[k] <= r_max, "%s: radius must be in 1 .. %lld (max(nrow, ncol)), got radii[%d] = %d", fn, (long long)r_max, k, radii[k]);
    FOC_REQUIRE(shape == FOCAL_SQUARE || shape == FOCAL_CIRCLE, "%s: shape must be MHS_FOCAL_SQUARE or MHS_FOCAL_CIRCLE, got %d", fn, shape);
    FOC_REQUIRE(stats != 0 && (stats >> FS_NSTATS) == 0, "%s: stats mask 0x%x selects nothing or unknown bits", fn, stats);
    if (shape == FOCAL_CIRCLE)
        FOC_REQUIRE((stats & FS_MINMAX_FAMILY) == 0, "%s: a circle window gives the sum family only (stats mask 0x%x asks for min / max): mhs_relief has them in a "
                    "circle for radius <= %d, a square window is meant for them beyond", fn, stats, MHS_TERRAIN_MAX_RADIUS);
    FOC_REQUIRE(std::isfinite(offset), "%s: offset must be finite", fn);
    FOC_REQUIRE(out_dtype == MHS_F64 || out_dtype == MHS_F32, "%s: out_dtype must be MHS_F64 or MHS_F32", fn);
    FOC_REQUIRE(out, "%s: out is NULL", fn);
    FOC_REQUIRE(ld >= c1 - c0, "%s: ld smaller than the window width", fn);
    const int n_stats = focal_popcount(stats);
    if (n_stats * n_radii > 1) FOC_REQUIRE(plane_stride >= ld * (r1 - r0 - 1) + (c1 - c0), "%s: plane_stride smaller than an output plane", fn);
    job->g = FocalPlane{nullptr, s->ld, (int)grid->nrow, (int)grid->ncol, s->nodata, !std::isnan(s->nodata), offset};
    job->dtype = s->dtype;
    job->r0 = (int)r0; job->r1 = (int)r1; job->c0 = (int)c0; job->c1 = (int)c1;
    job->n_rad = n_radii;
    for (int k = 0; k < n_radii; ++k) job->radius[k] = radii[k];
    job->shape = shape; job->mask = stats; job->n_stats = n_stats; job->fill_na = fill_na != 0; job->out_dtype = out_dtype;
    job->out_esz = out_dtype == MHS_F64 ? 8 : 4;
    return MHS_OK;
}

// Host planes in, host planes out: row bands of the window, top to bottom, on one stream of the library's host-pointer pipeline.
// A band sends up the rows focal_rows_read names; the column offsets of the block its successor starts in stay on the device.
static int focal_host(FocalJob job, const mhs_stack *s, int layer, void *out_host) {
    if (int rc = require_ready()) return rc;
    const int64_t nr = job.r1 - job.r0, nc = job.c1 - job.c0;
    if (nr == 0 || nc == 0) return MHS_OK;
    const size_t esz = dtype_bytes(s->dtype);
    const int n_out = job.n_stats * job.n_rad;
    const bool square = job.shape == FOCAL_SQUARE;
    const size_t row_bytes = (size_t)s->ld * esz + (size_t)nc * job.out_esz * n_out;
    int64_t rows_per = std::max<int64_t>(1, std::min<int64_t>(nr, (int64_t)(((size_t)256 << 20) / row_bytes)));
    if (const char *e = getenv("MHS_HOST_BANDS")) {
        const int64_t nb = std::max<int64_t>(1, std::min<int64_t>(nr, atoll(e)));
        rows_per = (nr + nb - 1) / nb;
    }
    size_t in_rows = 0;                                          // the most rows a band sends up
    for (int64_t b0 = job.r0; b0 < job.r1; b0 += rows_per) {
        int ra, rb;
        focal_rows_read(job, (int)b0, (int)std::min<int64_t>(job.r1, b0 + rows_per), b0 > job.r0, &ra, &rb);
        in_rows = std::max(in_rows, (size_t)(rb - ra));
    }
    const size_t in_bytes = foc_up(in_rows * s->ld * esz);
    const size_t plane_out = (size_t)rows_per * nc;
    const size_t out_bytes = foc_up(plane_out * job.out_esz * n_out);
    const size_t carry_bytes = square ? focal_carry_bytes(job) * job.n_rad : 0;
    std::lock_guard<std::mutex> lk(pipe_mutex());
    if (int rc = host_pipe(in_bytes + out_bytes + 2 * carry_bytes)) return rc;
    Context &c = ctx();
    hipStream_t st = c.pipe_comp;
    char *in = c.pipe_arena, *outb = in + in_bytes, *carry[2] = {outb + out_bytes, outb + out_bytes + carry_bytes};
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{st};   // no copy is left in flight, whatever the exit
    const char *src = (const char *)s->data + (size_t)layer * s->plane_stride * esz;
    int band = 0;
    for (int64_t b0 = job.r0; b0 < job.r1; b0 += rows_per, ++band) {
        const int64_t b1 = std::min<int64_t>(job.r1, b0 + rows_per);
        const bool carried = band > 0, more = b1 < job.r1;
        int ra, rb;
        focal_rows_read(job, (int)b0, (int)b1, carried, &ra, &rb);
        MHS_HIP(hipMemcpyAsync(in, src + (size_t)ra * s->ld * esz, ((size_t)(rb - ra - 1) * s->ld + job.g.ncol) * esz, hipMemcpyHostToDevice, st));
        job.g.plane = in - (size_t)ra * s->ld * esz;
        if (int rc = focal_run(job, (int)b0, (int)b1, outb, nc, (int64_t)plane_out, st, square && carried ? carry[band & 1] : nullptr,
                               square && more ? carry[(band + 1) & 1] : nullptr, (int)b1, carried))
            return rc;
        for (int p = 0; p < n_out; ++p)
            MHS_HIP(hipMemcpyAsync((char *)out_host + ((size_t)p * nr * nc + (size_t)(b0 - job.r0) * nc) * job.out_esz, outb + (size_t)p * plane_out * job.out_esz,
                                   (size_t)(b1 - b0) * nc * job.out_esz, hipMemcpyDeviceToHost, st));
        MHS_HIP(hipStreamSynchronize(st));       // the next band reuses the buffers
    }
    return MHS_OK;
}

}  // namespace mhs

using namespace mhs;

extern "C" {

int mhs_focal_dev(const mhs_grid *g, const mhs_stack *stack, int layer, const int *radii, int n_radii, int shape, unsigned stats, int fill_na,
                  double offset, int64_t r0, int64_t r1, int64_t c0, int64_t c1, void *out_dev, int out_dtype, int64_t ld, int64_t plane_stride,
                  void *stream) {
    FocalJob job;
    if (int rc = focal_check(__func__, g, stack, layer, radii, n_radii, shape, stats, fill_na, offset, r0, r1, c0, c1, out_dev, out_dtype, ld, plane_stride, &job)) return rc;
    if (int rc = require_ready()) return rc;
    job.g.plane = (const char *)stack->data + (size_t)layer * stack->plane_stride * dtype_bytes(stack->dtype);
    return focal_run(job, job.r0, job.r1, out_dev, ld, plane_stride, pick_stream(stream), nullptr, nullptr, 0, false);
}

int mhs_focal(const mhs_grid *g, const mhs_stack *stack, int layer, const int *radii, int n_radii, int shape, unsigned stats, int fill_na,
              double offset, int64_t r0, int64_t r1, int64_t c0, int64_t c1, void *out_host, int out_dtype) {
    FocalJob job;
    if (int rc = focal_check(__func__, g, stack, layer, radii, n_radii, shape, stats, fill_na, offset, r0, r1, c0, c1, out_host, out_dtype, c1 - c0,
                             (r1 - r0) * (c1 - c0), &job)) return rc;
    return focal_host(job, stack, layer, out_host);
}

}  // extern "C"
