// Standard errors of thin-plate-spline predictions on gfx950: fields::predictSE.Krig for a fitted spline, at points,
// on every cell centre of a raster window and on the tiles of Step 3 (terra::interpolate(r, fit, fun = predictSE)).
//
// With M = [[K + lambda W^-1, T], [T', 0]] the saddle-point matrix of the fit (fields' Krig notation) and
// z(x) = [phi(|(u,v) - u_j|^2)_j ; 1 ; u ; v], predictSE.Krig's
//     var(x) = rho phi(0) - 2 rho k(x)'a(x) + a(x)' (rho K + sigma^2 W^-1) a(x)
// reduces, for rho = sigma^2 / lambda (fields' MLE pair satisfies it), to
//     var(x) = (sigma^2 / lambda) z(x)' Q z(x),   Q = -M^-1 .
// Q does not depend on the data or on sigma^2: it is built once per spline (O(n^3), block formula on the fit's own
// weighted QR: on the host, below, or on the device, tps_se_build.hip -- mhs_tps_se_build_mode) and kept on the device
// in the handle.  Per cell the work is one quadratic form with a fixed (n+3)^2 matrix: a batched GEMM  Z_block Q
// (v_mfma_f64_16x16x4f64) followed by a row-wise dot with Z_block.
//
// Kernel layout (tps_se_kernel): a workgroup = 4 waves = 128 cells of one window (a wave owns two 16-cell tiles).
// The columns of Q are walked in chunks of 64; for each chunk the rows of Q stream through LDS in slabs of 16 x 64
// (double-buffered, one global read per workgroup), every wave multiplies its z rows into 2 x 4 accumulator tiles, and
// the chunk's part of z'Qz is folded in before the next chunk.  z is never stored: the A operand (one z entry per
// lane) is computed where it is consumed, with the table log of the direct evaluation (devmath.h), and the cell centres
// and range scaling are those of tps_eval.hip, so the SE plane and the estimate plane describe the same cells.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>
#include "common.h"
#include "devmath.h"
#include "step3_plan.h"
#include "tps_host.h"
#include "tps_se.h"

namespace mhs {

constexpr int SE_WAVES = 4;                        // waves per workgroup
constexpr int SE_CT = 2;                           // 16-cell tiles per wave
constexpr int SE_CELLS = SE_WAVES * SE_CT * 16;    // cells per workgroup
constexpr int SE_JB = 4;                           // 16-column tiles per chunk of Q
constexpr int SE_KS = 16;                          // rows of Q per LDS slab
constexpr int SE_LD = 80;                          // LDS row stride (doubles): consecutive rows 128 B apart in the banks

// one window (or one point set) of one spline
struct SeWindow {
    const double *q;          // np x np, Q with PHI_K folded in (zero padding beyond n + 3)
    const Knot *knots;        // the handle's knots (u, v read)
    const double *px, *py;    // points mode: coordinates; NULL = grid window
    double *out;
    double xmin, ymax, xres, yres, cx, cy, sx, sy;
    double rho;               // sigma^2 / lambda
    int64_t r0, c0, ld, ncell;
    int64_t block0;           // first workgroup of this window
    int nc, n, np, pad;       // n = 0: no spline (a zero tile): NaN
};

typedef double d4v __attribute__((ext_vector_type(4)));

// z_k for a cell at scaled (u, v): phi without its constant for k < n, then 1, u, v, then zeros (padding)
__device__ __forceinline__ double se_z(const Knot *__restrict__ knots, int n, double u, double v, int k, const double2 *tab) {
    const Knot kn = knots[min(k, n - 1)];
    const double dx = u - kn.u;
    const double dx2 = dx * dx;
    const double dy = v - kn.v;
    const double dd = fma(dy, dy, dx2);
    const double ph = r2logr2(dd, tab);
    return k < n ? ph : (k == n ? 1.0 : (k == n + 1 ? u : (k == n + 2 ? v : 0.0)));
}

// scaled coordinates of cell i of the window, with exactly the operations of tps_eval.hip
__device__ __forceinline__ void se_cell(const SeWindow &W, int64_t i, double &u, double &v) {
    if (W.px) {
        u = (W.px[i] - W.cx) / W.sx;
        v = (W.py[i] - W.cy) / W.sy;
        return;
    }
    const int64_t row = i / W.nc, col = i - row * W.nc;
    const double x = W.xmin + ((double)(W.c0 + col) + 0.5) * W.xres;
    const double y = W.ymax - ((double)(W.r0 + row) + 0.5) * W.yres;
    u = (x - W.cx) / W.sx;
    v = (y - W.cy) / W.sy;
}

__device__ __forceinline__ void se_store(const SeWindow &W, int64_t i, double val) {
    if (i >= W.ncell) return;
    if (W.px) { W.out[i] = val; return; }
    const int64_t row = i / W.nc, col = i - row * W.nc;
    W.out[row * W.ld + col] = val;
}

__global__ __launch_bounds__(64 * SE_WAVES) __attribute__((amdgpu_waves_per_eu(2))) void tps_se_kernel(const SeWindow *__restrict__ wins, int nwin,
                                                                const double2 *__restrict__ gtab) {
    __shared__ double2 tab[LOG_TAB_N];
    __shared__ double slab[2][SE_KS * SE_LD];
    // the window of this workgroup (uniform): last window whose first block <= blockIdx.x
    int lo = 0, hi = nwin - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (wins[mid].block0 <= (int64_t)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const SeWindow W = wins[lo];
    const int64_t cell0 = ((int64_t)blockIdx.x - W.block0) * SE_CELLS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    if (W.n == 0) {     // a tile without a spline
        for (int c = threadIdx.x; c < SE_CELLS; c += 64 * SE_WAVES) se_store(W, cell0 + c, __builtin_nan(""));
        return;
    }
    stage_log_table(tab, gtab);
    const int n = W.n, np = W.np;
    const int64_t last = W.ncell - 1;
    // A-operand cells of this lane (row l15 of each tile) and the cells of its accumulator rows (l4 + 4 r)
    double ua[SE_CT], va[SE_CT], part[SE_CT][4];
#pragma unroll
    for (int t = 0; t < SE_CT; ++t) {
        se_cell(W, min(cell0 + (wave * SE_CT + t) * 16 + l15, last), ua[t], va[t]);
#pragma unroll
        for (int r = 0; r < 4; ++r) part[t][r] = 0.0;
    }
    const int nslab = np / SE_KS;
    for (int j0 = 0; j0 < np; j0 += 16 * SE_JB) {
        const int njb = min(SE_JB, (np - j0) >> 4);
        d4v acc[SE_CT][SE_JB];
#pragma unroll
        for (int t = 0; t < SE_CT; ++t)
#pragma unroll
            for (int jb = 0; jb < SE_JB; ++jb) acc[t][jb] = d4v{0.0, 0.0, 0.0, 0.0};
        // slab s = rows [16 s, 16 s + 16) x columns [j0, j0 + 64) of Q; 4 elements per thread
        double pre[SE_KS * 64 / (64 * SE_WAVES)];
        auto load = [&](int s) {
#pragma unroll
            for (int q = 0; q < SE_KS * 64 / (64 * SE_WAVES); ++q) {
                const int idx = threadIdx.x + q * 64 * SE_WAVES, r = idx >> 6, c = idx & 63;
                pre[q] = (j0 + c < np) ? W.q[(int64_t)(s * SE_KS + r) * np + j0 + c] : 0.0;
            }
        };
        auto put = [&](int b) {
#pragma unroll
            for (int q = 0; q < SE_KS * 64 / (64 * SE_WAVES); ++q) {
                const int idx = threadIdx.x + q * 64 * SE_WAVES, r = idx >> 6, c = idx & 63;
                slab[b][r * SE_LD + c] = pre[q];
            }
        };
        __syncthreads();          // the previous chunk's last slab is no longer read
        load(0);
        put(0);
        __syncthreads();
        for (int s = 0; s < nslab; ++s) {
            if (s + 1 < nslab) load(s + 1);
            const double *S = slab[s & 1];
#pragma unroll
            for (int kk = 0; kk < SE_KS; kk += 4) {
                const int k = s * SE_KS + kk + l4;
                double a[SE_CT];
#pragma unroll
                for (int t = 0; t < SE_CT; ++t) a[t] = se_z(W.knots, n, ua[t], va[t], k, tab);
#pragma unroll
                for (int jb = 0; jb < SE_JB; ++jb) {
                    if (jb < njb) {
                        const double b = S[(kk + l4) * SE_LD + jb * 16 + l15];
#pragma unroll
                        for (int t = 0; t < SE_CT; ++t) acc[t][jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], b, acc[t][jb], 0, 0, 0);
                    }
                }
            }
            if (s + 1 < nslab) put((s + 1) & 1);
            __syncthreads();
        }
        // acc[t][jb][r] = (Z Q)[cell l4 + 4 r of tile t][column j0 + 16 jb + l15]: fold in z of that cell and column
#pragma unroll
        for (int t = 0; t < SE_CT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double ue, ve;
                se_cell(W, min(cell0 + (wave * SE_CT + t) * 16 + l4 + 4 * r, last), ue, ve);
#pragma unroll
                for (int jb = 0; jb < SE_JB; ++jb)
                    if (jb < njb) part[t][r] = fma(acc[t][jb][r], se_z(W.knots, n, ue, ve, j0 + jb * 16 + l15, tab), part[t][r]);
            }
    }
    // sum over the 16 lanes of a row group, then one lane per cell writes sqrt(max(rho z'Qz, 0))
#pragma unroll
    for (int t = 0; t < SE_CT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double x = part[t][r];
            x += __shfl_xor(x, 1);
            x += __shfl_xor(x, 2);
            x += __shfl_xor(x, 4);
            x += __shfl_xor(x, 8);
            if (l15 == 0) {
                const double var = W.rho * x;
                se_store(W, cell0 + (wave * SE_CT + t) * 16 + l4 + 4 * r, sqrt(var > 0.0 ? var : 0.0));
            }
        }
}

// process-wide settings (mhs_tps_se_max_n, mhs_tps_se_build_mode): they apply to every Q built after them
static std::atomic<int64_t> g_se_max_n{MHS_TPS_SE_MAX_N};
static std::atomic<int> g_se_build_mode{MHS_SE_BUILD_AUTO};

// ------------------------------------------------------------------------------------------------ Q on the host --
void se_state_free(SeState *s) {
    if (!s) return;
    pool_release(s->q_dev);
    delete s;
}

template <typename F>
static void parallel_for(int threads, int64_t count, F fn) {
    threads = (int)std::max<int64_t>(1, std::min<int64_t>(threads, count));
    if (threads == 1) { for (int64_t i = 0; i < count; ++i) fn(i); return; }
    std::atomic<int64_t> next{0};
    auto work = [&]() { for (;;) { const int64_t i = next.fetch_add(1); if (i >= count) break; fn(i); } };
    std::vector<std::thread> th;
    for (int q = 1; q < threads; ++q) th.emplace_back(work);
    work();
    for (std::thread &t : th) t.join();
}

// G <- Q' G (n x n column-major, every column), Q = H0 H1 H2 of the weighted QR; rev applies Q instead
static void reflect_columns(std::vector<double> &G, int64_t n, int64_t ncols, const std::vector<double> *hv, const double *htau,
                            bool rev) {
    for (int64_t j = 0; j < ncols; ++j)
        for (int q = 0; q < 3; ++q) {
            const int k = rev ? 2 - q : q;
            apply_reflector(hv[k], htau[k], G.data() + j * n, n);
        }
}
static void transpose_square(std::vector<double> &G, int64_t n) {
    for (int64_t j = 0; j < n; ++j)
        for (int64_t i = j + 1; i < n; ++i) std::swap(G[i + j * n], G[j + i * n]);
}

// Q = -M^-1 by the block formula on the weighted QR  S T = [Q1 Q2] [R; 0]  (S = W^1/2):  with F = [Q1 Q2]' (S K S) [Q1 Q2]
// + lambda I and X = F22^-1 = (B + lambda I)^-1,
//   M^-1 = diag(S, I) [[Q2 X Q2',  (Q1 - Q2 X F21) R^-T], [., -R^-1 (F11 - F12 X F21) R^-T]] diag(S, I).
// Also trA = n - lambda tr X and RSS_w = lambda^2 |X Q2' S yM|^2 (the weighted residual of the fit is lambda W^-1 c).
static int se_build(const mhs_tps *t, int threads, std::vector<double> &Qh, SeState &st) {
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t n = t->n, m = n - 3;
    const double lam = t->lambda;
    const TpsPrep *P = t->prep.get();
    std::vector<double> sw((size_t)n, 1.0), hvl[3];
    double htl[3], Rl[9];
    const std::vector<double> *hv = hvl;
    const double *htau = htl, *R = Rl;
    const double *uv = t->knots_uv.data();
    if (P) { sw = P->sw; hv = P->hv; htau = P->htau; R = P->R; }
    else {   // mhs_tps_from_coef: unit weights, the QR of [1 u v]
        std::vector<double> T((size_t)(3 * n));
        for (int64_t i = 0; i < n; ++i) { T[i] = 1.0; T[n + i] = uv[i]; T[2 * n + i] = uv[n + i]; }
        qr_n3(T, n, hvl, htl, Rl);
        if (!(fabs(Rl[8]) > 1e-10 * fabs(Rl[0]) && fabs(Rl[4]) > 1e-10 * fabs(Rl[0]))) {
            set_error("mhs_tps_predict_se: collinear knots");
            return MHS_ERR_NUMERIC;
        }
    }
    // F = Q' (S K S) Q + lambda I, K with the exact log (phi(0) = 0)
    std::vector<double> G((size_t)(n * n));
    parallel_for(threads, n, [&](int64_t j) {
        for (int64_t i = 0; i < n; ++i) {
            const double dx = uv[i] - uv[j], dy = uv[n + i] - uv[n + j];
            const double d2 = dx * dx + dy * dy;
            G[i + j * n] = d2 > 0 ? sw[i] * sw[j] * (PHI_K * d2 * log(d2)) : 0.0;
        }
    });
    reflect_columns(G, n, n, hv, htau, false);
    transpose_square(G, n);
    reflect_columns(G, n, n, hv, htau, false);
    for (int64_t i = 0; i < n; ++i) G[i + i * n] += lam;
    // Cholesky of F22 (left-looking, column-major m x m)
    std::vector<double> L((size_t)(m * m), 0.0);
    for (int64_t j = 0; j < m; ++j)
        for (int64_t i = j; i < m; ++i) L[i + j * m] = G[(3 + i) + (3 + j) * n];
    for (int64_t j = 0; j < m; ++j) {
        double *cj = L.data() + j * m;
        for (int64_t k = 0; k < j; ++k) {
            const double *ck = L.data() + k * m;
            const double a = ck[j];
            for (int64_t i = j; i < m; ++i) cj[i] -= a * ck[i];
        }
        if (!(cj[j] > 0)) { set_error("mhs_tps_predict_se: B + lambda I is not positive definite"); return MHS_ERR_NUMERIC; }
        const double d = sqrt(cj[j]);
        cj[j] = d;
        for (int64_t i = j + 1; i < m; ++i) cj[i] /= d;
    }
    // Li = L^-1 column by column (independent), then X = Li' Li
    std::vector<double> Li((size_t)(m * m), 0.0), X((size_t)(m * m));
    parallel_for(threads, m, [&](int64_t c) {
        double *x = Li.data() + c * m;
        x[c] = 1.0;
        for (int64_t k = c; k < m; ++k) {
            const double *lk = L.data() + k * m;
            x[k] /= lk[k];
            const double a = x[k];
            for (int64_t i = k + 1; i < m; ++i) x[i] -= a * lk[i];
        }
    });
    parallel_for(threads, m, [&](int64_t j) {
        const double *lj = Li.data() + j * m;
        for (int64_t i = 0; i <= j; ++i) {
            const double *li = Li.data() + i * m;
            double s = 0.0;
            for (int64_t k = j; k < m; ++k) s += li[k] * lj[k];
            X[i + j * m] = s;
            X[j + i * m] = s;
        }
    });
    // Y = X F21, S3 = F11 - F21' Y, tr X, RSS_w
    std::vector<double> Y((size_t)(m * 3));
    for (int c = 0; c < 3; ++c)
        for (int64_t i = 0; i < m; ++i) {
            double s = 0.0;
            for (int64_t k = 0; k < m; ++k) s += X[i + k * m] * G[(3 + k) + c * n];
            Y[i + c * m] = s;
        }
    double S3[9];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            double s = G[a + b * n];
            for (int64_t k = 0; k < m; ++k) s -= G[(3 + k) + a * n] * Y[k + b * m];
            S3[a + 3 * b] = s;
        }
    double trX = 0.0;
    for (int64_t i = 0; i < m; ++i) trX += X[i + i * m];
    st.eff_df = (double)n - lam * trX;
    if (P) {
        double rss = 0.0;
        for (int64_t i = 0; i < m; ++i) {
            double s = 0.0;
            for (int64_t k = 0; k < m; ++k) s += X[i + k * m] * P->wv[3 + k];
            rss += s * s;
        }
        st.rss_w = lam * lam * rss;
        st.sigma2 = (st.rss_w + P->pure_ss) / ((double)P->N - st.eff_df);
    }
    // R^-1 (upper triangular)
    double Ri[9] = {0};
    for (int c = 0; c < 3; ++c) {
        Ri[c + 3 * c] = 1.0 / R[c + 3 * c];
        for (int r = c - 1; r >= 0; --r) {
            double s = 0.0;
            for (int k = r + 1; k <= c; ++k) s += R[r + 3 * k] * Ri[k + 3 * c];
            Ri[r + 3 * c] = -s / R[r + 3 * r];
        }
    }
    // top-left: S Q [[0, 0], [0, X]] Q' S
    std::vector<double> TL((size_t)(n * n), 0.0);
    for (int64_t j = 0; j < m; ++j)
        for (int64_t i = 0; i < m; ++i) TL[(3 + i) + (3 + j) * n] = X[i + j * m];
    reflect_columns(TL, n, n, hv, htau, true);
    transpose_square(TL, n);
    reflect_columns(TL, n, n, hv, htau, true);
    // top-right: S Q [[I], [-Y]] R^-T
    std::vector<double> TR((size_t)(n * 3), 0.0);
    for (int c = 0; c < 3; ++c) {
        for (int a = 0; a < 3; ++a) TR[a + c * n] = Ri[c + 3 * a];                     // (R^-T)[a][c] = Ri[c][a]
        for (int64_t i = 0; i < m; ++i) {
            double s = 0.0;
            for (int a = 0; a < 3; ++a) s += Y[i + a * m] * Ri[c + 3 * a];
            TR[(3 + i) + c * n] = -s;
        }
    }
    reflect_columns(TR, n, 3, hv, htau, true);
    // bottom-right: -R^-1 S3 R^-T
    double BR[9];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            double s = 0.0;
            for (int p = 0; p < 3; ++p)
                for (int q = 0; q < 3; ++q) s += Ri[a + 3 * p] * S3[p + 3 * q] * Ri[b + 3 * q];
            BR[a + 3 * b] = -s;
        }
    // Q = -M^-1, phi's constant folded in (the kernel's z holds d2 log d2), zero-padded to np
    const int64_t np = (n + 3 + 15) / 16 * 16;
    Qh.assign((size_t)(np * np), 0.0);
    const double k2 = PHI_K * PHI_K;
    for (int64_t j = 0; j < n; ++j)
        for (int64_t i = 0; i < n; ++i) Qh[i * np + j] = -k2 * sw[i] * sw[j] * TL[i + j * n];
    for (int c = 0; c < 3; ++c)
        for (int64_t i = 0; i < n; ++i) {
            const double v = -PHI_K * sw[i] * TR[i + c * n];
            Qh[i * np + n + c] = v;
            Qh[(n + c) * np + i] = v;
        }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) Qh[(n + a) * np + n + b] = -BR[a + 3 * b];
    st.n = n; st.np = np; st.lambda = lam;
    st.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return MHS_OK;
}

// the handle's SE state, built and uploaded on first use (under the handle's mutex)
static int se_state(const mhs_tps *t, int threads, const SeState **out) {
    mhs_tps *tm = const_cast<mhs_tps *>(t);
    std::lock_guard<std::mutex> lk(tm->mu);
    if (!tm->se) {
        const int64_t max_n = g_se_max_n.load();
        if (t->n > max_n) {
            set_error("mhs_tps_predict_se: %lld distinct stations; standard errors are limited to %d (Q = -M^-1 is dense, "
                      "O(n^2) per cell)", (long long)t->n, (int)max_n);
            return MHS_ERR_INVALID;
        }
        if (!(t->lambda > 0)) {
            set_error("mhs_tps_predict_se: lambda must be positive (rho = sigma^2 / lambda)");
            return MHS_ERR_INVALID;
        }
        SeState *s = new SeState();
        // AUTO: the host build -- the bits every earlier release gave -- up to the default limit, the device build above it
        const int mode = g_se_build_mode.load();
        if (mode == MHS_SE_BUILD_DEVICE || (mode == MHS_SE_BUILD_AUTO && t->n > MHS_TPS_SE_MAX_N)) {
            if (int rc = se_build_device(t, *s)) { delete s; return rc; }
        } else {
            std::vector<double> Qh;
            if (int rc = se_build(t, threads, Qh, *s)) { delete s; return rc; }
            s->built_on = MHS_SE_BUILD_HOST;
            s->q_dev = (double *)pool_alloc(sizeof(double) * Qh.size());
            if (!s->q_dev) { delete s; return MHS_ERR_ALLOC; }
            if (int rc = h2d_sync(s->q_dev, Qh.data(), sizeof(double) * Qh.size())) { se_state_free(s); return rc; }
        }
        tm->se = s;
    }
    *out = tm->se;
    return MHS_OK;
}

static int resolve_sigma2(const mhs_tps *t, const SeState *s, double sigma2, double *rho) {
    if (std::isnan(sigma2)) {
        if (!t->prep) {
            set_error("mhs_tps_predict_se: a spline built from coefficients has no observations: sigma2 must be given");
            return MHS_ERR_INVALID;
        }
        sigma2 = s->sigma2;
    }
    if (!(sigma2 >= 0) || std::isinf(sigma2)) { set_error("mhs_tps_predict_se: sigma2 must be >= 0 or NaN"); return MHS_ERR_INVALID; }
    *rho = sigma2 / s->lambda;
    return MHS_OK;
}

static SeWindow se_window(const mhs_tps *t, const SeState *s, double rho) {
    SeWindow w;
    memset(&w, 0, sizeof(w));
    w.q = s ? s->q_dev : nullptr;
    w.knots = t ? t->knots_dev : nullptr;
    w.n = t ? (int)t->n : 0;
    w.np = s ? (int)s->np : 0;
    w.rho = rho;
    if (t) { w.cx = t->center[0]; w.cy = t->center[1]; w.sx = t->scale[0]; w.sy = t->scale[1]; }
    return w;
}

static void se_grid_geom(SeWindow &w, const mhs_grid *g, int64_t r0, int64_t r1, int64_t c0, int64_t c1, double *out, int64_t ld) {
    w.xmin = g->xmin; w.ymax = g->ymax; w.xres = g->xres; w.yres = g->yres;
    w.r0 = r0; w.c0 = c0; w.nc = (int)(c1 - c0); w.ncell = (r1 - r0) * (c1 - c0);
    w.out = out; w.ld = ld;
}

// one launch over every window (their first blocks assigned here); the descriptors travel in a pool block that is
// released after the stream has been synchronised by the caller (*desc_out)
static int se_launch(std::vector<SeWindow> &wins, hipStream_t s, void **desc_out) {
    *desc_out = nullptr;
    int64_t blocks = 0;
    std::vector<SeWindow> live;
    for (SeWindow &w : wins) {
        if (w.ncell <= 0) continue;
        w.block0 = blocks;
        blocks += (w.ncell + SE_CELLS - 1) / SE_CELLS;
        live.push_back(w);
    }
    if (live.empty()) return MHS_OK;
    MHS_REQUIRE(blocks < (1LL << 31), "too many cells for one launch");
    void *d = pool_alloc(sizeof(SeWindow) * live.size());
    if (!d) return MHS_ERR_ALLOC;
    *desc_out = d;
    if (int rc = h2d_sync(d, live.data(), sizeof(SeWindow) * live.size())) return rc;
    hipLaunchKernelGGL(tps_se_kernel, dim3((unsigned)blocks), dim3(64 * SE_WAVES), 0, s, (const SeWindow *)d, (int)live.size(),
                       ctx().log_tab);
    MHS_HIP(hipGetLastError());
    return MHS_OK;
}

// The SE plane of the plan's tiles: the windows, the stations and the packed layout are the Step3Plan's (step3_plan.h), the ones
// the estimate's own driver (run_tiles, tps_surface.hip) works from; the fits are materialised handles here (mhs_tps_fit_many)
static int surface_se_tiles(const mhs_grid *g, const Step3Plan &P, const double *xy, const double *resid, int64_t n, const double *cov1,
                            double lambda, int gcv_mode, double *out_dev, int64_t ld, hipStream_t s) {
    const int64_t nt = P.nt;
    std::vector<int64_t> rows((size_t)n), cols((size_t)n);
    if (int rc = mhs_cells_from_xy(g, xy, n, rows.data(), cols.data())) return rc;
    std::vector<std::vector<double>> txy((size_t)nt), ty((size_t)nt);
    std::vector<int64_t> todo;
    for (int64_t h = 0; h < nt; ++h) {
        step3_stations(P, h, rows.data(), cols.data(), xy, resid, cov1, n, txy[(size_t)h], ty[(size_t)h]);
        if ((int64_t)ty[(size_t)h].size() >= STEP3_MIN_STATIONS) todo.push_back(h);     // V73:710-721: no spline below that
    }
    // the tiles' fits in one call (what mhs_tps_fit_many gives a caller that composes the same steps)
    const int64_t nf = (int64_t)todo.size();
    std::vector<const double *> pxy((size_t)nf), py((size_t)nf);
    std::vector<int64_t> pn((size_t)nf);
    std::vector<mhs_tps *> fits((size_t)nf, nullptr);
    std::vector<int> status((size_t)nf, MHS_OK);
    for (int64_t q = 0; q < nf; ++q) {
        const int64_t h = todo[(size_t)q];
        pxy[(size_t)q] = txy[(size_t)h].data(); py[(size_t)q] = ty[(size_t)h].data(); pn[(size_t)q] = (int64_t)ty[(size_t)h].size();
    }
    struct Drop { std::vector<mhs_tps *> &f; ~Drop() { for (mhs_tps *t : f) tps_free_quiet(t); } } drop{fits};
    if (nf > 0)
        if (int rc = mhs_tps_fit_many(pxy.data(), py.data(), pn.data(), nf, lambda, gcv_mode, fits.data(), status.data())) return rc;
    for (int64_t q = 0; q < nf; ++q)
        if (!fits[(size_t)q]) {
            set_error("mhs_tps_surface_se_dev: the spline of tile %lld could not be fitted", (long long)todo[(size_t)q]);
            return status[(size_t)q] ? status[(size_t)q] : MHS_ERR_NUMERIC;
        }
    // Q of every tile from the host threads: host builds run side by side, device builds (MHS_SE_BUILD_DEVICE) one after the other
    std::vector<const SeState *> st((size_t)nf, nullptr);
    std::vector<int> rcs((size_t)nf, MHS_OK);
    std::vector<std::string> errs((size_t)nf);
    const int slot = current_slot();
    parallel_for(std::min(cpu_budget(), 16), nf, [&](int64_t q) {
        SlotBind bind(slot);
        rcs[(size_t)q] = se_state(fits[(size_t)q], 1, &st[(size_t)q]);
        if (rcs[(size_t)q]) errs[(size_t)q] = mhs_last_error();
    });
    for (int64_t q = 0; q < nf; ++q)
        if (rcs[(size_t)q]) { set_error("%s", errs[(size_t)q].c_str()); return rcs[(size_t)q]; }
    // the tiles' keep windows, then ONE launch for all of them
    const std::vector<size_t> off = P.pack();
    DevBuf<double> buf;
    MHS_HIP(buf.alloc(off[(size_t)nt]));
    std::vector<SeWindow> wins;
    std::vector<const double *> ptrs((size_t)nt);
    int64_t q = 0;
    for (int64_t h = 0; h < nt; ++h) {
        double *o = buf.p + off[(size_t)h];
        ptrs[(size_t)h] = o;
        const mhs_grid gf = P.fit_grid(g, h);      // terra::rast(rb): the fit raster, evaluated on the keep window (V73:726)
        int64_t r0, r1, c0, c1;
        P.keep_in_fit(h, &r0, &r1, &c0, &c1);
        SeWindow w;
        if (q < nf && todo[(size_t)q] == h) {
            double rho = 0;
            if (int rc = resolve_sigma2(fits[(size_t)q], st[(size_t)q], NAN, &rho)) return rc;
            w = se_window(fits[(size_t)q], st[(size_t)q], rho);
            ++q;
        } else w = se_window(nullptr, nullptr, 0.0);
        se_grid_geom(w, &gf, r0, r1, c0, c1, o, c1 - c0);
        wins.push_back(w);
    }
    void *desc = nullptr;
    int rc = se_launch(wins, s, &desc);
    if (!rc) rc = mosaic_feather_impl(g, P.nRx, P.nCx, P.keep.data(), ptrs.data(), 0, out_dev, ld, nullptr, s, false);  // NA-aware
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = MHS_ERR_HIP;
    pool_release(desc);
    return rc;
}

}  // namespace mhs

using namespace mhs;

extern "C" {

int mhs_tps_se_max_n(int64_t max_n, int64_t *previous) {
    MHS_REQUIRE(max_n >= 1 && max_n <= MHS_TPS_SE_HARD_MAX_N, "max_n must lie in 1 .. MHS_TPS_SE_HARD_MAX_N");
    const int64_t prev = g_se_max_n.exchange(max_n);
    if (previous) *previous = prev;
    return MHS_OK;
}

int mhs_tps_se_build_mode(int mode) {
    MHS_REQUIRE(mode == MHS_SE_BUILD_AUTO || mode == MHS_SE_BUILD_HOST || mode == MHS_SE_BUILD_DEVICE, "mode must be 0, 1 or 2");
    g_se_build_mode.store(mode);
    return MHS_OK;
}

int mhs_tps_se_info(const mhs_tps *t, int *built_on, double *build_ms, int64_t *q_bytes) {
    MHS_REQUIRE(t != nullptr, "NULL argument");
    mhs_tps *tm = const_cast<mhs_tps *>(t);
    std::lock_guard<std::mutex> lk(tm->mu);
    MHS_REQUIRE(tm->se != nullptr, "this spline has no Q yet (no standard error has been asked of it)");
    if (built_on) *built_on = tm->se->built_on;
    if (build_ms) *build_ms = tm->se->build_ms;
    if (q_bytes) *q_bytes = (int64_t)sizeof(double) * tm->se->np * tm->se->np;
    return MHS_OK;
}

int mhs_tps_sigma2(const mhs_tps *t, double *sigma2) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(t && sigma2, "NULL argument");
    MHS_REQUIRE(t->prep != nullptr, "a spline built from coefficients has no observations");
    const SeState *s = nullptr;
    if (int rc = se_state(t, cpu_budget(), &s)) return rc;
    *sigma2 = s->sigma2;
    return MHS_OK;
}

int mhs_tps_predict_se_grid_dev(const mhs_tps *t, const mhs_grid *g, int64_t r0, int64_t r1, int64_t c0, int64_t c1,
                                double sigma2, double *out_dev, int64_t ld, void *stream) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(t && g && out_dev, "NULL argument");
    MHS_REQUIRE(g->nrow > 0 && g->ncol > 0 && g->xres > 0 && g->yres > 0, "bad grid geometry");
    MHS_REQUIRE(0 <= r0 && r0 <= r1 && r1 <= g->nrow && 0 <= c0 && c0 <= c1 && c1 <= g->ncol, "window outside the grid");
    MHS_REQUIRE(ld >= c1 - c0, "ld smaller than the window width");
    MHS_REQUIRE(c1 - c0 < (1LL << 30), "window too wide");
    const SeState *s = nullptr;
    if (int rc = se_state(t, cpu_budget(), &s)) return rc;
    double rho = 0;
    if (int rc = resolve_sigma2(t, s, sigma2, &rho)) return rc;
    if (r1 == r0 || c1 == c0) return MHS_OK;
    std::vector<SeWindow> wins(1, se_window(t, s, rho));
    se_grid_geom(wins[0], g, r0, r1, c0, c1, out_dev, ld);
    hipStream_t st = pick_stream(stream);
    void *desc = nullptr;
    int rc = se_launch(wins, st, &desc);
    // the descriptor block goes back to the pool only once the kernel has read it
    if (desc) { if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = MHS_ERR_HIP; pool_release(desc); }
    return rc;
}

int mhs_tps_predict_se_grid(const mhs_tps *t, const mhs_grid *g, int64_t r0, int64_t r1, int64_t c0, int64_t c1, double sigma2,
                            double *out_host) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(t && g && out_host, "NULL argument");
    MHS_REQUIRE(0 <= r0 && r0 <= r1 && 0 <= c0 && c0 <= c1, "bad window");
    const int64_t nr = r1 - r0, nc = c1 - c0;
    return plane_to_host(nr, nc, out_host, [&](double *buf, hipStream_t s) {      // an empty window is still validated by the _dev twin
        return mhs_tps_predict_se_grid_dev(t, g, r0, r1, c0, c1, sigma2, buf, std::max<int64_t>(nc, 1), s); });
}

int mhs_tps_predict_se_points(const mhs_tps *t, const double *xy, int64_t n, double sigma2, double *out_host) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(t && out_host && (xy || n == 0), "NULL argument");
    MHS_REQUIRE(n >= 0, "negative n");
    const SeState *s = nullptr;
    if (int rc = se_state(t, cpu_budget(), &s)) return rc;
    double rho = 0;
    if (int rc = resolve_sigma2(t, s, sigma2, &rho)) return rc;
    if (n == 0) return MHS_OK;
    DevBuf<double> dxy, dout;
    MHS_HIP(dxy.alloc((size_t)(2 * n)));
    MHS_HIP(dout.alloc((size_t)n));
    hipStream_t st = ctx().stream;
    MHS_HIP(hipMemcpyAsync(dxy.p, xy, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, st));
    std::vector<SeWindow> wins(1, se_window(t, s, rho));
    wins[0].px = dxy.p; wins[0].py = dxy.p + n; wins[0].out = dout.p; wins[0].ncell = n;
    void *desc = nullptr;
    int rc = se_launch(wins, st, &desc);
    if (!rc && hipMemcpyAsync(out_host, dout.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st) != hipSuccess) rc = MHS_ERR_HIP;
    if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = MHS_ERR_HIP;
    pool_release(desc);
    return rc;
}

int mhs_tps_surface_se_dev(const mhs_grid *g, const double *xy, const double *resid, int64_t n, const double *cov1_at_stations,
                           int64_t tile_edge, double lambda, int gcv_mode, double *out_dev, int64_t ld, int64_t *tiles_out,
                           void *stream) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(g && xy && resid && out_dev && n > 0 && ld >= g->ncol, "bad arguments");
    Step3Plan P;
    if (int rc = step3_plan(g, tile_edge, P)) return rc;
    if (tiles_out) { tiles_out[0] = P.nRx; tiles_out[1] = P.nCx; }
    hipStream_t s = pick_stream(stream);
    if (P.nt == 1) {  // V73:748-753: the global fit
        mhs_tps *t = nullptr;
        if (int rc = mhs_tps_fit(xy, resid, n, lambda, gcv_mode, &t)) return rc;
        int rc = mhs_tps_predict_se_grid_dev(t, g, 0, g->nrow, 0, g->ncol, NAN, out_dev, ld, s);
        if (!rc) rc = (hipStreamSynchronize(s) == hipSuccess) ? MHS_OK : MHS_ERR_HIP;
        mhs_tps_free(t);
        return rc;
    }
    return surface_se_tiles(g, P, xy, resid, n, cov1_at_stations, lambda, gcv_mode, out_dev, ld, s);
}

int mhs_tps_surface_se(const mhs_grid *g, const double *xy, const double *resid, int64_t n, const double *cov1_at_stations,
                       int64_t tile_edge, double lambda, int gcv_mode, double *out_host, int64_t *tiles_out) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(g && out_host && g->nrow > 0 && g->ncol > 0, "bad arguments");
    return plane_to_host(g->nrow, g->ncol, out_host, [&](double *out, hipStream_t s) {
        return mhs_tps_surface_se_dev(g, xy, resid, n, cov1_at_stations, tile_edge, lambda, gcv_mode, out, g->ncol, tiles_out, s); });
}

}  // extern "C"
