// Thin-plate-spline fit on gfx950: fields::Tps(x, Y) (V73:722, V73:751).
//
//   host   collapse replicates, range-scale, Householder QR of T~ = W^1/2 [1 u v]   O(n)         tps_prepare
//   GPU    Gram  A = W^1/2 K W^1/2,  K_ij = (1/8pi) 0.5 log(r2) r2                    n^2 logs     build_A
//   GPU    A <- Q' A Q  (three two-sided Householder updates); B = A[3:,3:] is SPD, order m = n - 3
//   then one of four routes to c2 = (B + lambda I)^-1 Q2'y~ (tps_fit_lane picks; each is one solve_* function here):
//     fixed     lambda given: blocked Cholesky of B + lambda I (FP64 MFMA trailing update) + triangular solves, n^3/3
//               (tps_chol.hip)
//     tridiag   GCV, m <= 256: Householder tridiagonalisation in ONE block, lambda by GCV on the tridiagonal on the host,
//               one-block back-transform (kernels below; TridiagGcv in tps_gcv_host.hip)
//     band32    GCV, 320 <= m <= 32 768 (the default for large fits): reduction to a band of width 32 by 32-column panels,
//               lambda by GCV on the band on the GPU, back-transform (tps_band32.hip)
//     band8     GCV, everything else -- 256 < m < 320, m beyond the 32-column route, MHS_FIT_LEGACY_BAND=1, and a fit whose
//               32-column reduction broke down: reduction to a band of width 8 by 8-column panels, lambda by GCV on the band
//               on the host (BandGcv), back-transform (tps_band8.hip)
//     A GCV route reduces B = Q Bb Q' once per station set, rotates g = Q'Q2'y~ along, solves q = (Bb + lambda I)^-1 g and
//     back-transforms c2 = Q q (4n^3/3); the reduction cache below keeps a reduction for the other response layers.
//   host   c = W^1/2 Q [0; c2],  d = R^-1 (Q1'y~ - A[0:3,3:] c2)                                  make_spline
//
// A is n x n, full symmetric storage, column-major with leading dimension ld.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <unordered_map>
#include <memory>
#include <mutex>
#include <vector>
#include "common.h"
#include "devmath.h"
#include "tps_host.h"
#include "tps_chol.h"
#include "tps_band32.h"
#include "tps_band8.h"

namespace mhs {

// ------------------------------------------------------------------ Gram matrix --

// The null-space projection A <- Q'KQ, Q = H1 H2 H3 = I - V T V' (the three reflectors of the QR of [1 u v]), WITHOUT
// ever storing K: Q'KQ = K - W V' - V W' with W = Y T - 1/2 V S, Y = K V, S = T'(V'Y)T.  Pass 1 forms Y from kernel
// entries computed on the fly (row blocks x column splits, partial sums); the host turns Y into W (3 columns); pass 2
// computes the entries again and writes the projected matrix directly.  Two passes of n^2 logs and ONE write of the
// matrix instead of a write and three read-modify-write passes (memory-bound: 7.8 -> 2.5 ms at n = 20 000).
constexpr int GY_MAXSPLIT = 16;
__global__ __launch_bounds__(256) void gram_y_kernel(const double *__restrict__ u, const double *__restrict__ v,
                                                     const double *__restrict__ sw, int n, const double *__restrict__ V3,
                                                     const double2 *__restrict__ gtab, double *__restrict__ Ypart /* [split][3][n] */) {
    __shared__ double2 tab[LOG_TAB_N];
    __shared__ double red[4][3][64];
    stage_log_table(tab, gtab);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + lane;
    const int per = ((n + (int)gridDim.y - 1) / (int)gridDim.y + 3) & ~3;
    const int j0 = blockIdx.y * per, j1 = min(n, j0 + per);
    const bool ok = i < n;
    const int ii = ok ? i : 0;
    const double ui = u[ii], vi = v[ii], si = sw[ii] * (0.5 / (8.0 * M_PI));
    double y0 = 0.0, y1 = 0.0, y2 = 0.0;
    for (int j = j0 + wave; j < j1; j += 4) {
        const double dx = ui - u[j], dy = vi - v[j];
        const double d2 = fma(dy, dy, dx * dx);
        const double k = si * sw[j] * r2logr2(d2, tab);
        y0 = fma(k, V3[j], y0); y1 = fma(k, V3[n + j], y1); y2 = fma(k, V3[2 * (int64_t)n + j], y2);
    }
    red[wave][0][lane] = y0; red[wave][1][lane] = y1; red[wave][2][lane] = y2;
    __syncthreads();
    if (threadIdx.x < 192) {
        const int a = threadIdx.x >> 6;
        const double t = (red[0][a][lane] + red[1][a][lane]) + (red[2][a][lane] + red[3][a][lane]);
        if (ok) Ypart[((int64_t)blockIdx.y * 3 + a) * n + i] = t;
    }
}

__global__ __launch_bounds__(256) void gram_proj_kernel(const double *__restrict__ u, const double *__restrict__ v,
                                                        const double *__restrict__ sw, int n, int64_t ld,
                                                        const double2 *__restrict__ gtab, const double *__restrict__ V3,
                                                        const double *__restrict__ W3, double *__restrict__ A) {
    __shared__ double2 tab[LOG_TAB_N];
    stage_log_table(tab, gtab);
    const int i = blockIdx.x * 64 + (threadIdx.x & 63);
    const int j0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * 16;
    if (i >= n) return;
    const double ui = u[i], vi = v[i], si = sw[i] * (0.5 / (8.0 * M_PI));
    const double v0 = V3[i], v1 = V3[n + i], v2 = V3[2 * (int64_t)n + i];
    const double w0 = W3[i], w1 = W3[n + i], w2 = W3[2 * (int64_t)n + i];
    for (int j = j0; j < j0 + 16 && j < n; ++j) {
        const double dx = ui - u[j], dy = vi - v[j];
        const double d2 = fma(dy, dy, dx * dx);
        double a = si * sw[j] * r2logr2(d2, tab);
        a -= w0 * V3[j] + v0 * W3[j];
        a -= w1 * V3[n + j] + v1 * W3[n + j];
        a -= w2 * V3[2 * (int64_t)n + j] + v2 * W3[2 * (int64_t)n + j];
        A[i + (int64_t)j * ld] = a;
    }
}

__global__ void add_diag_kernel(double *A, int64_t ld, int off, int m, double lam) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) A[(int64_t)(off + i) * ld + off + i] += lam;
}

// =============================================================================================
// Small matrices (the reference-tiled mode fits 130-750 stations per tile, V73:690-722): the blocked
// band reduction of tps_band8.hip is four launches and two events per panel, and with several tiles being fitted
// side by side the HIP launch path itself becomes the bottleneck.  Up to TRI_SMALL_CUT the whole
// Householder TRIDIAGONALISATION runs in ONE block (matrix in L2, reflectors kept below the subdiagonal,
// g <- Q'g carried along) and the GCV search uses the tridiagonal criterion on the host (TridiagGcv);
// a second single-block kernel applies Q to the solution.  Three launches per fit.
// Thread layout: rows over the low bits, up to 1024 / rows column groups over the high bits.
// =============================================================================================
constexpr int TRI_SMALL_MAX = 768;   // rows the kernel can hold
constexpr int TRI_SMALL_CUT = 256;   // largest order it is used for: one CU's bandwidth bounds it (~m^3 x 8 B through
                                     // a single block), the band reduction overtakes it near m = 300

__global__ __launch_bounds__(1024) void tridiag_small_kernel(double *__restrict__ A, int64_t ld, int off, int m,
                                                             double *__restrict__ d, double *__restrict__ e,
                                                             double *__restrict__ tau, double *__restrict__ g) {
    __shared__ double vs[TRI_SMALL_MAX], ws[TRI_SMALL_MAX], part[1024];
    __shared__ double pbuf[2][16][BW];   // per-wave partials of the two reductions of a column
    __shared__ double alpha_s;
    double *B = A + (int64_t)off * ld + off;
    for (int k = 0; k < m - 1; ++k) {
        const int t = m - k - 1;                       // order of the trailing block B22 = B[k+1:, k+1:]
        double *x = B + (int64_t)k * ld + (k + 1);     // column k below the diagonal
        double *B22 = B + (int64_t)(k + 1) * ld + (k + 1);
        if (threadIdx.x == 0) d[k] = B[(int64_t)k * ld + k];
        if (t == 1) {
            if (threadIdx.x == 0) { e[k] = x[0]; tau[k] = 0.0; }
            break;
        }
        const int rows_pad = (t + 63) & ~63;
        const int G = max(1, 1024 / rows_pad);         // column groups
        const int ii = threadIdx.x % rows_pad, jg = threadIdx.x / rows_pad;
        const bool act = jg < G && ii < t;
        // Householder vector of x (dlarfg).  Reductions as in the panel kernel: lane-swap / DPP partials, one
        // barrier, every wave adds the 16 partials itself (alternating buffers): 6 barriers per column, not 11.
        const double xi = (threadIdx.x < t) ? x[threadIdx.x] : 0.0;
        double red1[1] = {threadIdx.x >= 1 && threadIdx.x < t ? xi * xi : 0.0};
        wave_publish<1>(red1, pbuf[0]);
        if (threadIdx.x == 0) alpha_s = xi;
        __syncthreads();
        const double ss = lane_value(block_total<1, 16>(pbuf[0]), 0);
        const double alpha = alpha_s;
        double beta = alpha, tk = 0.0, scal = 0.0;
        if (ss != 0.0) {
            beta = -copysign(sqrt(alpha * alpha + ss), alpha);
            tk = (beta - alpha) / beta;
            scal = 1.0 / (alpha - beta);
        }
        if (threadIdx.x < t) {
            const double v = threadIdx.x == 0 ? 1.0 : xi * scal;
            vs[threadIdx.x] = v;
            if (threadIdx.x > 0) x[threadIdx.x] = v;   // reflector kept for the back-transform
        }
        if (threadIdx.x == 0) { e[k] = beta; tau[k] = tk; }
        __syncthreads();
        // p = tau B22 v (partial sums per column group), w = p - 1/2 tau (p'v) v ; g <- H g
        double acc = 0.0;
        if (act) {
            const double *row = B22 + ii;
#pragma unroll 4
            for (int j = jg; j < t; j += G) acc = fma(row[(int64_t)j * ld], vs[j], acc);
        }
        part[threadIdx.x] = acc;
        __syncthreads();
        double pi = 0.0, vi = 0.0, gi = 0.0;
        if (threadIdx.x < t) {
            for (int q = 0; q < G; ++q) pi += part[q * rows_pad + threadIdx.x];
            pi *= tk;
            vi = vs[threadIdx.x];
            gi = g[k + 1 + threadIdx.x];
        }
        double red2[2] = {pi * vi, vi * gi};
        wave_publish<2>(red2, pbuf[1]);
        __syncthreads();
        const double tot2 = block_total<2, 16>(pbuf[1]);
        const double pv = lane_value(tot2, 0), vg = lane_value(tot2, 1);
        if (threadIdx.x < t) {
            ws[threadIdx.x] = pi - 0.5 * tk * pv * vi;
            g[k + 1 + threadIdx.x] = gi - tk * vg * vi;
        }
        __syncthreads();
        // B22 <- B22 - v w' - w v'
        if (act) {
            double *row = B22 + ii;
            const double vi2 = vs[ii], wi2 = ws[ii];
#pragma unroll 4
            for (int j = jg; j < t; j += G) row[(int64_t)j * ld] -= vi2 * ws[j] + wi2 * vs[j];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) d[m - 1] = B[(int64_t)(m - 1) * ld + (m - 1)];
}

// q <- Q q = H_0 H_1 ... H_{m-3} q with the reflectors tridiag_small_kernel left below the subdiagonal
// NW waves: 16, or 4 when m <= 256 (a row per thread is all the kernel uses; the waves beyond the rows contribute exact
// zeros to every sum, so both sizes give the same bits) -- a 256-thread block finds a slot beside grid-filling kernels
// as soon as ONE of their blocks retires, a 1024-thread block needs a whole CU to drain
template <int NW>
__global__ __launch_bounds__(NW * 64) void tridiag_back_kernel(const double *__restrict__ A, int64_t ld, int off, int m,
                                                               const double *__restrict__ tau, double *__restrict__ q) {
    __shared__ double pbuf[2][NW][BW];
    const double *B = A + (int64_t)off * ld + off;
    int ph = 0;
    // the next reflector's element and tau are requested a step ahead: a step is two barriers, not a trip to L2 as well
    double xn = 0.0, tn = 0.0;
    if (m >= 3) {
        const int k0 = m - 3;
        if (threadIdx.x >= 1 && (int)threadIdx.x < m - k0 - 1) xn = B[(int64_t)k0 * ld + (k0 + 1) + threadIdx.x];
        tn = tau[k0];
    }
    for (int k = m - 3; k >= 0; --k) {
        const int t = m - k - 1;
        const double tk = tn, xk = xn;
        if (k > 0) {
            if (threadIdx.x >= 1 && (int)threadIdx.x < t + 1) xn = B[(int64_t)(k - 1) * ld + k + threadIdx.x];
            tn = tau[k - 1];
        }
        double vi = 0.0, qi = 0.0;
        if (threadIdx.x < t) { vi = threadIdx.x == 0 ? 1.0 : xk; qi = q[k + 1 + threadIdx.x]; }
        double red[1] = {vi * qi};
        wave_publish<1>(red, pbuf[ph]);
        __syncthreads();
        const double vq = lane_value(block_total<1, NW>(pbuf[ph]), 0);
        ph ^= 1;
        if (threadIdx.x < t) q[k + 1 + threadIdx.x] = qi - tk * vq * vi;
        __syncthreads();
    }
}

// g <- Q' g = H_{m-3} ... H_0 g with the reflectors tridiag_small_kernel left: the updates that kernel applies to g while it
// reduces the matrix, in the same order and through the same reduction tree (the second slot of its two-value
// reduction), so a right-hand side sent through here equals bit for bit one that was carried through the reduction.
// Used when the reduction of a station set is reused for another response layer (mhs_tps_reduction_cache).
template <int NW>      // 16 waves, or 4 when m <= 256: see tridiag_back_kernel
__global__ __launch_bounds__(NW * 64) void tridiag_qt_kernel(const double *__restrict__ A, int64_t ld, int off, int m,
                                                             const double *__restrict__ tau, double *__restrict__ g) {
    __shared__ double pbuf[2][NW][BW];
    const double *B = A + (int64_t)off * ld + off;
    int ph = 0;
    double xn = 0.0, tn = 0.0;
    if (m >= 3) {
        if (threadIdx.x >= 1 && (int)threadIdx.x < m - 1) xn = B[1 + threadIdx.x];
        tn = tau[0];
    }
    for (int k = 0; k < m - 2; ++k) {
        const int t = m - k - 1;
        const double tk = tn, xk = xn;
        if (k + 1 < m - 2) {
            if (threadIdx.x >= 1 && (int)threadIdx.x < t - 1) xn = B[(int64_t)(k + 1) * ld + (k + 2) + threadIdx.x];
            tn = tau[k + 1];
        }
        double vi = 0.0, gi = 0.0;
        if ((int)threadIdx.x < t) { vi = threadIdx.x == 0 ? 1.0 : xk; gi = g[k + 1 + threadIdx.x]; }
        double red2[2] = {0.0, vi * gi};
        wave_publish<2>(red2, pbuf[ph]);
        __syncthreads();
        const double vg = lane_value(block_total<2, NW>(pbuf[ph]), 1);
        ph ^= 1;
        if ((int)threadIdx.x < t) g[k + 1 + threadIdx.x] = gi - tk * vg * vi;
        __syncthreads();
    }
}

// The four ways a fit is solved once A = Q'KQ stands (tps_fit_lane picks one by size, lambda and environment)
enum class Route { fixed, tridiag, band32, band8 };

// The reduction of one station set, kept for the other response layers of the same table.  Tridiagonal route: reflectors +
// tau on the device, the tridiagonal and the three projected rows on the host.  Band routes: the reduced matrix (band +
// reflectors, n x ld) and the panels' records on the device (8-column: T factors and (tau, G); 32-column: B32_PANEL_REC),
// the band and the projected rows on the host.  Entries are shared_ptr-owned: a fit keeps its hit alive while
// mhs_tps_reduction_cache(0) -- or mhs_shutdown -- empties the map from another thread.
struct ReductionEntry {
    int64_t n = 0;
    int m = 0;
    Route kind = Route::tridiag;                 // the route that made the reduction
    std::vector<double> uv, sw, td, te, Atop;
    double *refl = nullptr, *tau = nullptr;      // device: m x m (ld = m), m
    // band routes
    int64_t ld = 0;
    int npanels = 0;
    double *Ared = nullptr, *Tall = nullptr, *aux = nullptr;   // device
    std::vector<double> ab;                                    // host: m x (BW + 1), or m x 33 on the 32-column route
    bool broke = false;                                        // NEGATIVE entry (no buffers): the 32-column route broke down on this station set
    size_t bytes = 0;                                          // device bytes held (the cache's budget counts them)
    uint64_t stamp = 0;                                        // last use (least recently used entries are evicted first)
    ReductionEntry(const TpsPrep &P, Route k) : n(P.n), m((int)(P.n - 3)), kind(k), uv(P.uv), sw(P.sw) {}
    bool same_stations(const TpsPrep &P) const { return n == P.n && uv == P.uv && sw == P.sw; }
    ~ReductionEntry() {
        for (double *q : {refl, tau, Ared, Tall, aux}) if (q) (void)hipFree(q);
        (void)hipGetLastError();
    }
};
struct ReductionCache {
    std::mutex mu;
    bool enabled = false;
    std::unordered_multimap<uint64_t, std::shared_ptr<ReductionEntry>> map;
    size_t bytes = 0;
    uint64_t clock = 0;
};
static ReductionCache g_rcache_slots[MAX_SLOTS];      // one per device slot: entries hold device pointers
#define g_rcache (g_rcache_slots[current_slot()])
// Device bytes the cache may pin (MHS_RCACHE_MAX_MB, default 4096): a band-route entry is a full copy of the reduced matrix
// (200 MB at n = 5 000), and a tiled Step 3 adds one per tile spline above 259 stations -- unbounded, they would compete
// with the arenas, whose own hipMalloc failures are hard errors (round-3 advisor finding).
static size_t rcache_budget() {
    static const size_t b = [] { const char *e = getenv("MHS_RCACHE_MAX_MB"); const long long mb = e ? atoll(e) : 4096; return (size_t)std::max(0LL, mb) << 20; }();
    return b;
}
// insert under the lock: evicts least-recently-used entries until the new one fits; an entry larger than the whole budget
// is not kept at all
static void rcache_insert(uint64_t key, const std::shared_ptr<ReductionEntry> &e) {
    std::vector<std::shared_ptr<ReductionEntry>> dead;      // freed after the lock is released (hipFree synchronises)
    {
        std::lock_guard<std::mutex> lk(g_rcache.mu);
        if (!g_rcache.enabled || e->bytes > rcache_budget()) return;
        while (g_rcache.bytes + e->bytes > rcache_budget() && !g_rcache.map.empty()) {
            auto victim = g_rcache.map.begin();
            for (auto it = g_rcache.map.begin(); it != g_rcache.map.end(); ++it) if (it->second->stamp < victim->second->stamp) victim = it;
            g_rcache.bytes -= victim->second->bytes;
            dead.push_back(std::move(victim->second));
            g_rcache.map.erase(victim);
        }
        e->stamp = ++g_rcache.clock;
        g_rcache.bytes += e->bytes;
        g_rcache.map.emplace(key, e);
    }
}
void reduction_cache_clear() {      // mhs_shutdown / mhs_init on another device: nothing of the old device survives
    std::vector<std::shared_ptr<ReductionEntry>> dead;
    {
        std::lock_guard<std::mutex> lk(g_rcache.mu);
        g_rcache.enabled = false;
        for (auto &kv : g_rcache.map) dead.push_back(std::move(kv.second));
        g_rcache.map.clear();
        g_rcache.bytes = 0;
    }
}
static uint64_t fnv1a(const void *p, size_t bytes, uint64_t h) {
    const unsigned char *c = (const unsigned char *)p;
    for (size_t i = 0; i < bytes; ++i) { h ^= c[i]; h *= 1099511628211ull; }
    return h;
}

// What a fit carries through its cache calls: whether the slot's cache is on, and then the hash of the station set
struct RcacheKey {
    bool on = false;
    uint64_t h = 0;
};
static RcacheKey rcache_key(const TpsPrep &P) {
    RcacheKey k;
    {
        std::lock_guard<std::mutex> lk(g_rcache.mu);
        k.on = g_rcache.enabled;
    }
    if (k.on) k.h = fnv1a(P.sw.data(), sizeof(double) * P.sw.size(), fnv1a(P.uv.data(), sizeof(double) * P.uv.size(), 1469598103934665603ull ^ (uint64_t)P.n));
    return k;
}
// find: the reduction of these stations made by route `kind`, or null.  With `broke` the negative entries are looked at
// first: an earlier layer's 32-column reduction broke down on these stations (round-4 advisor finding: every further layer
// repeated the failing reduction, the matrix rebuild and an uncached legacy reduction) -- then *broke is set and nothing
// is returned.
static std::shared_ptr<ReductionEntry> rcache_find(const RcacheKey &key, const TpsPrep &P, Route kind, bool *broke = nullptr) {
    if (!key.on) return nullptr;
    std::lock_guard<std::mutex> lk(g_rcache.mu);
    const auto range = g_rcache.map.equal_range(key.h);
    if (broke)
        for (auto it = range.first; it != range.second; ++it)
            if (it->second->broke && it->second->same_stations(P)) { *broke = true; return nullptr; }
    for (auto it = range.first; it != range.second; ++it)
        if (!it->second->broke && it->second->kind == kind && it->second->same_stations(P)) {
            it->second->stamp = ++g_rcache.clock;
            return it->second;
        }
    return nullptr;
}
// store: allocate the entry's device buffers, fill them on the fit's stream, wait, insert -- or drop the entry on any HIP
// failure.  One copy = rows x width doubles into the entry's member dst; src_ld != 0: the source rows are src_ld doubles
// apart.  need_headroom (the 32-column route's full-matrix copies): only with twice the entry's size free on the device.
struct RcacheCopy {
    double *ReductionEntry::*dst;
    const double *src;
    size_t width, rows, src_ld;
};
static void rcache_store(const RcacheKey &key, const std::shared_ptr<ReductionEntry> &e, hipStream_t s, std::initializer_list<RcacheCopy> copies,
                         bool need_headroom = false) {
    for (const RcacheCopy &c : copies) e->bytes += sizeof(double) * c.width * c.rows;
    bool ok = true;
    if (need_headroom) {
        size_t free_b = 0, total_b = 0;
        ok = e->bytes <= rcache_budget() && hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 2 * e->bytes;
    }
    for (const RcacheCopy &c : copies) ok = ok && hipMalloc((void **)&((*e).*c.dst), sizeof(double) * c.width * c.rows) == hipSuccess;
    for (const RcacheCopy &c : copies) {
        double *dst = (*e).*c.dst;
        ok = ok && (c.src_ld ? hipMemcpy2DAsync(dst, sizeof(double) * c.width, c.src, sizeof(double) * c.src_ld, sizeof(double) * c.width, c.rows, hipMemcpyDeviceToDevice, s)
                             : hipMemcpyAsync(dst, c.src, sizeof(double) * c.width * c.rows, hipMemcpyDeviceToDevice, s)) == hipSuccess;
    }
    ok = ok && hipStreamSynchronize(s) == hipSuccess;
    if (ok) rcache_insert(key.h, e);
    else (void)hipGetLastError();
}
// remember a breakdown of the 32-column route: the other layers on these stations go straight to the 8-column route
static void rcache_remember_breakdown(const RcacheKey &key, const TpsPrep &P) {
    auto e = std::make_shared<ReductionEntry>(P, Route::band32);
    e->broke = true;
    rcache_insert(key.h, e);
}

// fields' Krig.replicates: unique locations (first-appearance order), means, counts
static void collapse_replicates(const double *xy, const double *y, int64_t N, std::vector<double> &xm,
                                std::vector<double> &ym_out, std::vector<double> &w, double &pure_ss) {
    std::map<std::pair<double, double>, int64_t> seen;
    std::vector<int64_t> gid((size_t)N);
    std::vector<double> ux, uy, sum, cnt;
    for (int64_t i = 0; i < N; ++i) {
        const auto key = std::make_pair(xy[i], xy[N + i]);
        auto it = seen.find(key);
        if (it == seen.end()) {
            it = seen.emplace(key, (int64_t)ux.size()).first;
            ux.push_back(key.first); uy.push_back(key.second); sum.push_back(0.0); cnt.push_back(0.0);
        }
        gid[i] = it->second;
        sum[it->second] += y[i];
        cnt[it->second] += 1.0;
    }
    const int64_t n = (int64_t)ux.size();
    xm.resize(2 * n);
    ym_out.resize(n);
    w = cnt;
    for (int64_t k = 0; k < n; ++k) { xm[k] = ux[k]; xm[n + k] = uy[k]; ym_out[k] = sum[k] / cnt[k]; }
    pure_ss = 0.0;
    for (int64_t i = 0; i < N; ++i) { const double r = y[i] - ym_out[gid[i]]; pure_ss += r * r; }
}

int tps_prepare(const double *xy, const double *y, int64_t N, TpsPrep &P) {
    for (int64_t i = 0; i < N; ++i)
        if (!std::isfinite(xy[i]) || !std::isfinite(xy[N + i]) || !std::isfinite(y[i])) {
            set_error("mhs_tps_fit: non-finite input at row %lld (drop NA rows first, V73:706)", (long long)i);
            return MHS_ERR_INVALID;
        }
    P.N = N;
    collapse_replicates(xy, y, N, P.xm, P.ym, P.w, P.pure_ss);
    const int64_t n = P.n = (int64_t)P.ym.size();
    if (n <= 3) { set_error("mhs_tps_fit: need more than 3 distinct locations"); return MHS_ERR_NUMERIC; }

    // range scaling (fields scale.type = "range")
    P.uv.resize(2 * n); P.sw.resize(n);
    for (int d = 0; d < 2; ++d) {
        double lo = P.xm[d * n], hi = P.xm[d * n];
        for (int64_t i = 0; i < n; ++i) { lo = std::min(lo, P.xm[d * n + i]); hi = std::max(hi, P.xm[d * n + i]); }
        P.center[d] = lo; P.scale[d] = hi - lo;
        if (!(P.scale[d] > 0)) { set_error("mhs_tps_fit: degenerate station coordinates (zero range)"); return MHS_ERR_NUMERIC; }
        for (int64_t i = 0; i < n; ++i) P.uv[d * n + i] = (P.xm[d * n + i] - P.center[d]) / P.scale[d];
    }
    for (int64_t i = 0; i < n; ++i) P.sw[i] = sqrt(P.w[i]);

    // QR of T~ = W^1/2 [1 u v]
    std::vector<double> T(3 * n);
    for (int64_t i = 0; i < n; ++i) { T[i] = P.sw[i]; T[n + i] = P.sw[i] * P.uv[i]; T[2 * n + i] = P.sw[i] * P.uv[n + i]; }
    qr_n3(T, n, P.hv, P.htau, P.R);
    if (fabs(P.R[8]) < 1e-10 * fabs(P.R[0]) || fabs(P.R[4]) < 1e-10 * fabs(P.R[0])) {
        set_error("mhs_tps_fit: collinear station coordinates");
        return MHS_ERR_NUMERIC;
    }
    P.wv.resize(n);  // Q' y~
    for (int64_t i = 0; i < n; ++i) P.wv[i] = P.sw[i] * P.ym[i];
    for (int k = 0; k < 3; ++k) apply_reflector(P.hv[k], P.htau[k], P.wv.data(), n);
    return MHS_OK;
}

}  // namespace mhs

using namespace mhs;

// carves the work buffers of one fit out of the lane's arena (256-byte aligned); a dry run sizes it
struct ArenaCarver {
    char *base;
    size_t off = 0;
    template <typename T>
    T *take(size_t count) {
        off = (off + 255) & ~(size_t)255;
        T *p = base ? (T *)(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
};

// the device buffers every route shares, and the two band routes' work spaces
struct FitBufs {
    double *A, *duv, *dsw, *v3buf, *w3buf, *ypbuf, *vbuf, *pbuf, *wbuf, *gbuf, *chw, *tau;
    char *b8base, *b32base;
    int *info_dev;
};

// One fit on its way through the routes: what tps_fit_lane decided (sizes, streams, buffers, cache key), and the MHS_TIMING laps
struct FitJob {
    FitLane &L;
    const TpsPrep &prep;
    int64_t n, ld;      // stations; leading dimension of A (n x n, B = A[3:, 3:] of order m)
    int m;
    // mhs_fit_reserve_cus active: a GCV fit stays on the compute units the ensemble's masked member leaves free
    // (the Cholesky route takes its two streams from the lane itself)
    bool confined;
    hipStream_t s, s2, s2_b32;      // main stream, second stream, second stream of the 32-column reduction
    FitBufs b;
    int gcv_mode, gcv_threads;
    RcacheKey key;
    std::vector<double> Atop;       // rows 0..2 of the projected matrix, columns 3..n-1 (by symmetry: columns 0..2, rows 3..)
    bool timing;
    std::chrono::steady_clock::time_point t_last;
    void lap(const char *what) {
        if (!timing) return;
        (void)hipStreamSynchronize(s);
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[mhs_tps_fit n=%lld] %-28s %8.3f ms\n", (long long)n, what,
                std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    }
};
// what a route hands back: c2 = (B + lambda I)^-1 Q2'y~ and the criterion at lambda
struct FitSolution {
    std::vector<double> c2;
    double lam = NAN, gcv = NAN, eff_df = NAN;
};

// The matrix is allocated with room for the Cholesky's identity padding (up to one panel of rows and columns) and
// shifted by one double, so that row 3 -- where B = Q2'KQ2 starts -- sits on a 16-byte boundary in every column.
static void carve(ArenaCarver &ar, FitBufs &b, int64_t n, int m, int64_t ld, bool fixed, bool b32) {
    const int m_pad = chol_padded(m);
    b.A = ar.take<double>((size_t)(ld * (3 + m_pad)) + 2);
    if (b.A) b.A += 1;
    b.duv = ar.take<double>((size_t)(2 * n));
    b.dsw = ar.take<double>((size_t)n);
    b.v3buf = ar.take<double>(3 * (size_t)n);
    b.w3buf = ar.take<double>(3 * (size_t)n);
    b.ypbuf = ar.take<double>((size_t)GY_MAXSPLIT * 3 * n);
    b.vbuf = ar.take<double>((size_t)n);
    b.pbuf = ar.take<double>((size_t)n);
    b.wbuf = ar.take<double>((size_t)n);
    b.gbuf = ar.take<double>((size_t)m_pad + 8);
    b.chw = ar.take<double>(fixed ? chol_work_doubles(m) : 1);
    b.tau = ar.take<double>((size_t)n + 3);
    b.b8base = ar.take<char>(band8_workspace_bytes(m, n, !fixed));      // every fit: the 32-column route may hand its fit back
    b.info_dev = ar.take<int>(1);
    b.b32base = ar.take<char>(b32 ? band32_workspace_bytes(m, n) : 1);
}

// W = Y T - 1/2 V S, S = T'(1/2 (M + M'))T, M = V'Y, for the three reflectors V of the polynomial block (host, 3 columns)
static void projection_w(const TpsPrep &P, const std::vector<double> &Y, std::vector<double> &W) {
    const int64_t n = P.n;
    const std::vector<double> *hv = P.hv;
    double G[3][3], Tm3[3][3] = {{0}}, M3[3][3], S3[3][3], TM[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            double g = 0.0, mm = 0.0;
            for (int64_t i = 0; i < n; ++i) { g += hv[a][i] * hv[b][i]; mm += hv[a][i] * Y[(size_t)b * n + i]; }
            G[a][b] = g; M3[a][b] = mm;
        }
    for (int j = 0; j < 3; ++j) {      // larft (forward, columnwise): Q = H1 H2 H3 = I - V T V'
        Tm3[j][j] = P.htau[j];
        for (int i = 0; i < j; ++i) {
            double sum = 0.0;
            for (int l = i; l < j; ++l) sum += Tm3[i][l] * G[l][j];
            Tm3[i][j] = -P.htau[j] * sum;
        }
    }
    for (int a = 0; a < 3; ++a)        // S = T' (1/2 (M + M')) T
        for (int b = 0; b < 3; ++b) { double t = 0.0; for (int c = 0; c < 3; ++c) t += 0.5 * (M3[a][c] + M3[c][a]) * Tm3[c][b]; TM[a][b] = t; }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) { double t = 0.0; for (int c = 0; c < 3; ++c) t += Tm3[c][a] * TM[c][b]; S3[a][b] = t; }
    for (int64_t i = 0; i < n; ++i)
        for (int b = 0; b < 3; ++b) {
            double t = 0.0;
            for (int c = 0; c < 3; ++c) t += Y[(size_t)c * n + i] * Tm3[c][b] - 0.5 * hv[c][i] * 0.5 * (S3[c][b] + S3[b][c]);
            W[(size_t)b * n + i] = t;
        }
}

// The projected matrix A = Q'KQ = K - W V' - V W' in two passes over kernel entries computed on the fly (see gram_y_kernel);
// needs the stations in b.duv / b.dsw.  Run again when the 32-column route hands the fit back.
static int build_A(FitJob &J) {
    const int64_t n = J.n;
    const FitBufs &b = J.b;
    hipStream_t s = J.s;
    for (int k = 0; k < 3; ++k)
        MHS_HIP(hipMemcpyAsync(b.v3buf + (size_t)k * n, J.prep.hv[k].data(), sizeof(double) * n, hipMemcpyHostToDevice, s));
    const unsigned rb = (unsigned)((n + 63) / 64);
    const unsigned nsp = (unsigned)std::min<int64_t>(GY_MAXSPLIT, std::max<int64_t>(1, (1024 + rb - 1) / rb));
    hipLaunchKernelGGL(gram_y_kernel, dim3(rb, nsp), dim3(256), 0, s, b.duv, b.duv + n, b.dsw, (int)n, b.v3buf, ctx().log_tab, b.ypbuf);
    MHS_HIP(hipGetLastError());
    std::vector<double> Yp((size_t)nsp * 3 * n), Y(3 * (size_t)n, 0.0), W(3 * (size_t)n);
    MHS_HIP(hipMemcpyAsync(Yp.data(), b.ypbuf, sizeof(double) * Yp.size(), hipMemcpyDeviceToHost, s));
    MHS_HIP(hipStreamSynchronize(s));
    for (unsigned sp = 0; sp < nsp; ++sp)
        for (size_t e = 0; e < 3 * (size_t)n; ++e) Y[e] += Yp[(size_t)sp * 3 * n + e];
    projection_w(J.prep, Y, W);
    MHS_HIP(hipMemcpyAsync(b.w3buf, W.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice, s));
    dim3 grid((unsigned)((n + 63) / 64), (unsigned)((n + 63) / 64));
    hipLaunchKernelGGL(gram_proj_kernel, grid, dim3(256), 0, s, b.duv, b.duv + n, b.dsw, (int)n, J.ld, ctx().log_tab, b.v3buf, b.w3buf, b.A);
    MHS_HIP(hipGetLastError());
    MHS_HIP(hipStreamSynchronize(s));      // W (host vector) is read by the copy above
    return MHS_OK;
}

// fixed lambda: Cholesky of B + lambda I, solve for c2 = (B + lambda I)^-1 w2 (tps_chol.hip)
static int solve_fixed(FitJob &J, FitSolution &out) {
    const int m = J.m;
    const FitBufs &b = J.b;
    hipStream_t s = J.s;
    hipLaunchKernelGGL(add_diag_kernel, dim3((m + 255) / 256), dim3(256), 0, s, b.A, J.ld, 3, m, out.lam);
    MHS_HIP(hipMemcpyAsync(b.gbuf, J.prep.wv.data() + 3, sizeof(double) * m, hipMemcpyHostToDevice, s));
    if (int rc = cholesky_solve_mfma(J.L, b.A, J.ld, 3, m, b.gbuf, b.chw, b.info_dev)) return rc;
    MHS_HIP(hipMemcpyAsync(out.c2.data(), b.gbuf, sizeof(double) * m, hipMemcpyDeviceToHost, s));
    MHS_HIP(hipStreamSynchronize(s));
    return MHS_OK;
}

// small matrix: single-block tridiagonalisation + tridiagonal GCV on the host + single-block back-transform
static int solve_tridiag(FitJob &J, const ReductionEntry *hit, FitSolution &out) {
    const int m = J.m;
    const FitBufs &b = J.b;
    hipStream_t s = J.s;
    MHS_HIP(hipMemcpyAsync(b.gbuf, J.prep.wv.data() + 3, sizeof(double) * m, hipMemcpyHostToDevice, s));
    double *dd_dev = b.pbuf, *ee_dev = b.wbuf;
    std::vector<double> td((size_t)m), te((size_t)m), g((size_t)m), q((size_t)m);
    const double *refl = b.A;
    const double *tau_dev = b.tau;
    int64_t refl_ld = J.ld;
    int refl_off = 3;
    if (hit) {
        refl = hit->refl; tau_dev = hit->tau; refl_ld = m; refl_off = 0;
        td = hit->td; te = hit->te;
        if (m <= 256) hipLaunchKernelGGL(tridiag_qt_kernel<4>, dim3(1), dim3(256), 0, s, refl, refl_ld, refl_off, m, tau_dev, b.gbuf);
        else hipLaunchKernelGGL(tridiag_qt_kernel<16>, dim3(1), dim3(1024), 0, s, refl, refl_ld, refl_off, m, tau_dev, b.gbuf);
        MHS_HIP(hipGetLastError());
    } else {
        hipLaunchKernelGGL(tridiag_small_kernel, dim3(1), dim3(1024), 0, s, b.A, J.ld, 3, m, dd_dev, ee_dev, b.tau, b.gbuf);
        MHS_HIP(hipGetLastError());
        MHS_HIP(hipMemcpyAsync(td.data(), dd_dev, sizeof(double) * m, hipMemcpyDeviceToHost, s));
        MHS_HIP(hipMemcpyAsync(te.data(), ee_dev, sizeof(double) * (m - 1), hipMemcpyDeviceToHost, s));
    }
    MHS_HIP(hipMemcpyAsync(g.data(), b.gbuf, sizeof(double) * m, hipMemcpyDeviceToHost, s));
    MHS_HIP(hipStreamSynchronize(s));
    J.lap(hit ? "Q'g with the cached reflectors" : "tridiagonalisation (GPU, one block)");
    if (!hit && J.key.on) {      // keep the reduction for the next response layer on these stations
        auto e = std::make_shared<ReductionEntry>(J.prep, Route::tridiag);
        e->td = td; e->te = te; e->Atop = J.Atop;
        rcache_store(J.key, e, s, {{&ReductionEntry::refl, b.A + (int64_t)3 * J.ld + 3, (size_t)m, (size_t)m, (size_t)J.ld},
                                   {&ReductionEntry::tau, b.tau, (size_t)m, 1, 0}});
    }
    TridiagGcv tg;
    tg.a = td.data(); tg.b = te.data(); tg.g = g.data(); tg.m = m; tg.n = J.n; tg.N = J.prep.N; tg.pure_ss = J.prep.pure_ss;
    out.lam = tg.find_lambda(J.gcv_mode);
    if (std::isnan(out.lam) || out.lam < 0) { set_error("mhs_tps_fit: GCV search failed"); return MHS_ERR_NUMERIC; }
    tg.eval(out.lam, &out.gcv, &out.eff_df, q.data());
    J.lap("GCV search (host, tridiagonal)");
    MHS_HIP(hipMemcpyAsync(b.gbuf, q.data(), sizeof(double) * m, hipMemcpyHostToDevice, s));
    if (m <= 256) hipLaunchKernelGGL(tridiag_back_kernel<4>, dim3(1), dim3(256), 0, s, refl, refl_ld, refl_off, m, tau_dev, b.gbuf);
    else hipLaunchKernelGGL(tridiag_back_kernel<16>, dim3(1), dim3(1024), 0, s, refl, refl_ld, refl_off, m, tau_dev, b.gbuf);
    MHS_HIP(hipGetLastError());
    MHS_HIP(hipMemcpyAsync(out.c2.data(), b.gbuf, sizeof(double) * m, hipMemcpyDeviceToHost, s));
    MHS_HIP(hipStreamSynchronize(s));
    J.lap("solve + back-transform");
    return MHS_OK;
}

// 32-column panels, GCV on the band on the GPU (tps_band32.hip).  *broke: a panel was numerically rank deficient (its
// Cholesky-QR needs cond(P)^2 < 1 / eps) -- A is spent and `out` untouched
static int solve_band32(FitJob &J, const ReductionEntry *hit, FitSolution &out, bool *broke) {
    const int m = J.m;
    const FitBufs &b = J.b;
    hipStream_t s = J.s;
    Band32Ws w32;
    band32_carve(w32, b.b32base, m, J.n);
    double *pin = nullptr;
    if (int rc = band32_pinned(J.L, &pin)) return rc;
    MHS_HIP(hipMemcpyAsync(b.gbuf, J.prep.wv.data() + 3, sizeof(double) * m, hipMemcpyHostToDevice, s));
    const double *redA = b.A, *redT = w32.Tall;      // what the back-transform reads: this fit's reduction, or the cached one
    int64_t red_ld = J.ld;
    std::vector<double> ab32((size_t)m * (B32_NB + 1)), g((size_t)m), q((size_t)m);
    int breakdown = 0;
    if (hit) {
        redA = hit->Ared; redT = hit->Tall; red_ld = hit->ld;
        ab32 = hit->ab;
        MHS_HIP(hipMemcpyAsync(w32.ab, ab32.data(), sizeof(double) * ab32.size(), hipMemcpyHostToDevice, s));
        if (int rc = band32_qt(s, redA, red_ld, m, redT, b.gbuf, w32.sgp)) return rc;
    } else {
        if (int rc = band32_reduce(J.L, s, J.s2_b32, b.A, J.ld, m, J.n, b.gbuf, w32, &breakdown)) return rc;
    }
    if (breakdown) { *broke = true; return MHS_OK; }
    if (!hit) MHS_HIP(hipMemcpyAsync(ab32.data(), w32.ab, sizeof(double) * ab32.size(), hipMemcpyDeviceToHost, s));
    MHS_HIP(hipMemcpyAsync(g.data(), b.gbuf, sizeof(double) * m, hipMemcpyDeviceToHost, s));
    MHS_HIP(hipStreamSynchronize(s));
    J.lap(hit ? "Q'g with the cached 32-column reduction" : "band reduction (GPU, 32-column panels)");
    if (!hit && J.key.on) {      // keep the reduction for the next response layer on these stations
        const int np32 = band32_npanels(m);
        auto e = std::make_shared<ReductionEntry>(J.prep, Route::band32);
        e->Atop = J.Atop; e->ld = J.ld; e->npanels = np32; e->ab = ab32;
        rcache_store(J.key, e, s, {{&ReductionEntry::Ared, b.A, (size_t)J.ld * (size_t)(3 + m), 1, 0},
                                   {&ReductionEntry::Tall, w32.Tall, (size_t)np32 * B32_PANEL_REC, 1, 0}}, true);
    }
    Band32Search bs;
    bs.s = s; bs.s_aux = J.s2; bs.ab_dev = w32.ab; bs.g_dev = b.gbuf; bs.ab_host = ab32.data(); bs.g_host = g.data(); bs.m = m; bs.n = J.n; bs.N = J.prep.N;
    bs.pure_ss = J.prep.pure_ss; bs.ws = &w32; bs.pin = pin;
    if (int rc = bs.find_lambda(J.gcv_mode, &out.lam)) return rc;
    if (std::isnan(out.lam)) { set_error("mhs_tps_fit: GCV search failed"); return MHS_ERR_NUMERIC; }
    J.lap("GCV search (GPU, band of 32)");
    if (int rc = bs.solve(out.lam, &out.gcv, &out.eff_df, q.data())) return rc;
    MHS_HIP(hipMemcpyAsync(b.gbuf, q.data(), sizeof(double) * m, hipMemcpyHostToDevice, s));
    if (int rc = band32_backtransform(s, redA, red_ld, m, redT, b.gbuf, w32.btpart)) return rc;
    MHS_HIP(hipMemcpyAsync(out.c2.data(), b.gbuf, sizeof(double) * m, hipMemcpyDeviceToHost, s));
    MHS_HIP(hipStreamSynchronize(s));
    J.lap("solve + back-transform");
    return MHS_OK;
}

// 8-column panels, GCV on the band on the host (tps_band8.hip, BandGcv): B is reduced to bandwidth BW in place, g = Q'w2
// rotated along
static int solve_band8(FitJob &J, const ReductionEntry *hit, FitSolution &out) {
    const int m = J.m;
    const FitBufs &b = J.b;
    hipStream_t s = J.s;
    Band8Ws w8;
    band8_carve(w8, b.b8base, m, J.n, true);
    MHS_HIP(hipMemcpyAsync(b.gbuf, J.prep.wv.data() + 3, sizeof(double) * m, hipMemcpyHostToDevice, s));
    const bool keep = !hit && J.key.on && band8_cacheable(m);
    const double *redA = b.A, *redT = w8.Tall;      // what the back-transform reads: this fit's reduction, or the cached one
    int64_t red_ld = J.ld;
    std::vector<double> ab((size_t)m * (BW + 1)), g((size_t)m), q((size_t)m);
    struct Lease { GcvPool *p = nullptr; ~Lease() { gcv_pool_release(p); } } lease;
    if (hit) {
        // another response layer on a station set reduced before: only the right-hand side goes through the panels
        redA = hit->Ared; redT = hit->Tall; red_ld = hit->ld;
        ab = hit->ab;
        if (int rc = band8_qt(s, redA, red_ld, m, hit->aux, b.gbuf)) return rc;
        MHS_HIP(hipMemcpyAsync(g.data(), b.gbuf, sizeof(double) * m, hipMemcpyDeviceToHost, s));
        lease.p = gcv_pool_lease(J.gcv_threads);
        MHS_HIP(hipStreamSynchronize(s));
        J.lap("Q'g with the cached band reduction");
    } else {
        hipEvent_t wake = nullptr;
        if (int rc = band8_reduce(J.L, s, J.s2, b.A, J.ld, m, J.n, b.gbuf, w8, keep, &wake)) return rc;
        MHS_HIP(hipMemcpyAsync(ab.data(), w8.ab, sizeof(double) * ab.size(), hipMemcpyDeviceToHost, s));
        MHS_HIP(hipMemcpyAsync(g.data(), b.gbuf, sizeof(double) * m, hipMemcpyDeviceToHost, s));
        // wake the GCV workers while the last panels are still running
        if (wake) MHS_HIP(hipEventSynchronize(wake));
        lease.p = gcv_pool_lease(J.gcv_threads);
        MHS_HIP(hipStreamSynchronize(s));
        J.lap("band reduction (GPU)");
        if (keep) {      // keep the reduction for the next response layer on these stations (200 MB at n = 5 000)
            const int np = band8_npanels(m);
            auto e = std::make_shared<ReductionEntry>(J.prep, Route::band8);
            e->Atop = J.Atop; e->ld = J.ld; e->npanels = np; e->ab = ab;
            // no 16-byte row alignment needed for the matrix: only band8_qt and the back-transform read it
            rcache_store(J.key, e, s, {{&ReductionEntry::Ared, b.A, (size_t)J.ld * (size_t)(3 + m), 1, 0},
                                       {&ReductionEntry::Tall, w8.Tall, (size_t)np * BW * BW, 1, 0},
                                       {&ReductionEntry::aux, w8.aux, (size_t)np * PANEL_AUX, 1, 0}});
        }
    }
    BandGcv bg;
    bg.ab = ab.data(); bg.g = g.data(); bg.m = m; bg.n = J.n; bg.N = J.prep.N; bg.bw = BW; bg.pure_ss = J.prep.pure_ss; bg.threads = J.gcv_threads;
    bg.pool = lease.p;
    out.lam = bg.find_lambda(J.gcv_mode);
    if (std::isnan(out.lam)) { set_error("mhs_tps_fit: GCV search failed"); return MHS_ERR_NUMERIC; }
    J.lap("GCV search (host, banded)");
    BandGcv::Work wk;
    if (!bg.eval(out.lam, &out.gcv, &out.eff_df, q.data(), wk)) { set_error("mhs_tps_fit: band matrix not positive definite"); return MHS_ERR_NUMERIC; }
    MHS_HIP(hipMemcpyAsync(b.gbuf, q.data(), sizeof(double) * m, hipMemcpyHostToDevice, s));
    if (int rc = band8_backtransform(s, redA, red_ld, m, redT, b.gbuf, w8.Gp)) return rc;
    MHS_HIP(hipMemcpyAsync(out.c2.data(), b.gbuf, sizeof(double) * m, hipMemcpyDeviceToHost, s));
    MHS_HIP(hipStreamSynchronize(s));
    J.lap("solve + back-transform");
    return MHS_OK;
}

// d = R^-1 (w1 - Atop c2) ; c~ = Q [0; c2] ; c = W^1/2 c~ ; the spline's handle.  (The batched fits of tps_batch.hip do
// this algebra on the device with wave-wide sums, a different summation order: the two are not shared.)
static int make_spline(const TpsPrep &prep, const std::vector<double> &Atop, const FitSolution &sol, mhs_tps **out) {
    const int64_t n = prep.n;
    const int m = (int)(n - 3);
    const double *R = prep.R;
    double rhs[3];
    for (int k = 0; k < 3; ++k) {
        double sdot = 0.0;
        for (int j = 0; j < m; ++j) sdot += Atop[(size_t)k * m + j] * sol.c2[j];
        rhs[k] = prep.wv[k] - sdot;
    }
    double dd[3];
    dd[2] = rhs[2] / R[8];
    dd[1] = (rhs[1] - R[1 + 3 * 2] * dd[2]) / R[4];
    dd[0] = (rhs[0] - R[0 + 3 * 1] * dd[1] - R[0 + 3 * 2] * dd[2]) / R[0];
    std::vector<double> ct((size_t)n, 0.0);
    for (int j = 0; j < m; ++j) ct[3 + j] = sol.c2[j];
    for (int k = 2; k >= 0; --k) apply_reflector(prep.hv[k], prep.htau[k], ct.data(), n);

    mhs_tps *t = new mhs_tps();
    t->n = n;
    t->lambda = sol.lam; t->eff_df = sol.eff_df; t->gcv = sol.gcv;
    memcpy(t->center, prep.center, sizeof(t->center));
    memcpy(t->scale, prep.scale, sizeof(t->scale));
    memcpy(t->d, dd, sizeof(dd));
    t->c.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) t->c[i] = prep.sw[i] * ct[i];
    t->knots_uv = prep.uv;
    t->prep = std::make_shared<const TpsPrep>(prep);
    if (int rc = upload_knots(t)) { mhs_tps_free(t); return rc; }
    *out = t;
    return MHS_OK;
}

// Round 4: the GCV route of fits with 320+ unknowns is the 32-column one; MHS_FIT_LEGACY_BAND=1 (read per fit: the tests
// switch it) keeps them on the 8-column route, which also takes a fit whose 32-column reduction breaks down.
static Route pick_route(bool fixed, int m) {
    if (fixed) return Route::fixed;
    if (m <= TRI_SMALL_CUT && m >= 3) return Route::tridiag;
    if (!getenv("MHS_FIT_LEGACY_BAND") && m >= B32_MIN_M && m <= B32_MAX_M) return Route::band32;
    return Route::band8;
}

namespace mhs {
int tps_fit_lane(FitLane &L, const double *xy, const double *y, int64_t N, double lambda, int gcv_mode,
                 int gcv_threads, mhs_tps **out) {
    MHS_REQUIRE(xy && y && out, "NULL argument");
    MHS_REQUIRE(N > 3 && N < (1LL << 30), "need more than 3 observations");
    MHS_REQUIRE(std::isnan(lambda) || lambda >= 0, "lambda must be >= 0 or NaN");
    MHS_REQUIRE(gcv_mode == MHS_GCV_FIELDS || gcv_mode == MHS_GCV_CONVERGED, "bad gcv_mode");
    TpsPrep prep;
    if (int rc = tps_prepare(xy, y, N, prep)) return rc;
    const int64_t n = prep.n;
    const int m = (int)(n - 3);

    const bool fixed = !std::isnan(lambda);
    Route route = pick_route(fixed, m);
    const bool confined = !fixed && ctx().reserved_cus > 0 && L.ms != nullptr;
    FitJob J{L, prep, n, ((int64_t)(3 + chol_padded(m)) + 15) & ~(int64_t)15, m, confined,
             confined ? L.ms : L.s, confined ? L.ms2 : L.s2, confined ? L.ms2 : (L.s2r ? L.s2r : L.s2)};
    J.gcv_mode = gcv_mode; J.gcv_threads = gcv_threads;
    J.timing = getenv("MHS_TIMING") != nullptr;
    J.t_last = std::chrono::steady_clock::now();
    hipStream_t s = J.s;

    // the arena, with the 32-column work space whenever size and environment ask for that route
    {
        ArenaCarver dry{nullptr};
        carve(dry, J.b, n, m, J.ld, fixed, route == Route::band32);
        if (dry.off > L.arena_cap) {   // grow-only; growing synchronises the device, a lane's first fits only
            if (L.arena) { (void)hipStreamSynchronize(L.s); (void)hipStreamSynchronize(L.s2); (void)hipFree(L.arena); L.arena = nullptr; L.arena_cap = 0; }
            const size_t cap = dry.off + dry.off / 8;
            MHS_HIP(hipMalloc((void **)&L.arena, cap));
            L.arena_cap = cap;
        }
        ArenaCarver real{L.arena};
        carve(real, J.b, n, m, J.ld, fixed, route == Route::band32);
    }

    // mhs_tps_reduction_cache: the reduction of this station set may already be there (another response layer); a fixed
    // lambda never asks, the 8-column route only while its reduction can be replayed
    std::shared_ptr<ReductionEntry> hit_sp;      // keeps the hit alive whatever another thread does to the map
    if (route == Route::tridiag || route == Route::band32 || (route == Route::band8 && band8_cacheable(m))) {
        J.key = rcache_key(prep);
        bool broke = false;
        hit_sp = rcache_find(J.key, prep, route, route == Route::band32 ? &broke : nullptr);
        if (broke) {      // the 32-column route broke down on these stations before: straight to the 8-column route
            route = Route::band8;
            if (band8_cacheable(m)) hit_sp = rcache_find(J.key, prep, route);
        }
    }
    const ReductionEntry *hit = hit_sp.get();

    // A = Q'KQ and its first three rows -- or, with a hit, nothing: reflectors, band and projected rows come from the cache
    J.Atop.resize(3 * (size_t)m);
    if (hit) J.Atop = hit->Atop;
    else {
        MHS_HIP(hipMemcpyAsync(J.b.duv, prep.uv.data(), sizeof(double) * 2 * n, hipMemcpyHostToDevice, s));
        MHS_HIP(hipMemcpyAsync(J.b.dsw, prep.sw.data(), sizeof(double) * n, hipMemcpyHostToDevice, s));
        if (int rc = build_A(J)) return rc;
    }
    J.lap("gram + projection");
    if (!hit)
        for (int k = 0; k < 3; ++k)
            MHS_HIP(hipMemcpyAsync(&J.Atop[(size_t)k * m], J.b.A + (int64_t)k * J.ld + 3, sizeof(double) * m, hipMemcpyDeviceToHost, s));

    FitSolution sol;
    sol.c2.resize((size_t)m);
    sol.lam = lambda;
    if (route == Route::fixed) {
        if (int rc = solve_fixed(J, sol)) return rc;
    } else if (route == Route::tridiag) {
        if (int rc = solve_tridiag(J, hit, sol)) return rc;
    } else if (route == Route::band32) {
        bool broke = false;
        if (int rc = solve_band32(J, hit, sol, &broke)) return rc;
        if (broke) {
            // the matrix is rebuilt and the 8-column route takes the fit: its reduction is kept for the other layers (if it
            // can be replayed), and they are told not to try the 32-column route again
            route = Route::band8;
            if (J.key.on) rcache_remember_breakdown(J.key, prep);
            if (int rc = build_A(J)) return rc;
            J.lap("32-column route handed the fit back: matrix rebuilt");
        }
    }
    if (route == Route::band8)
        if (int rc = solve_band8(J, hit, sol)) return rc;

    return make_spline(prep, J.Atop, sol, out);
}
}  // namespace mhs

extern "C" int mhs_tps_reduction_cache(int enable) {
    if (int rc = require_ready()) return rc;
    if (enable) {
        std::lock_guard<std::mutex> lk(g_rcache.mu);
        g_rcache.enabled = true;
        return MHS_OK;
    }
    reduction_cache_clear();      // entries still used by a running fit live until that fit lets go of them
    return MHS_OK;
}

extern "C" int mhs_tps_fit(const double *xy, const double *y, int64_t N, double lambda, int gcv_mode,
                           mhs_tps **out) {
    if (int rc = require_ready()) return rc;
    FitLane *L = nullptr;
    if (int rc = fit_lane(0, &L)) return rc;
    return tps_fit_lane(*L, xy, y, N, lambda, gcv_mode, 0, out);
}
