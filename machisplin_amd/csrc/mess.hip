// MESS, the multivariate environmental similarity surface of a grid against the stations' covariates (dismo::mess, Elith,
// Kearney & Phillips 2010; include/machisplin_hip.h states the rule, mess_rule.h holds it): for every cell and every variable
// the cell's value is placed in the stations' empirical distribution, the worst variable is the cell's MESS and its index the
// "most dissimilar variable" (MoD).
//
// One pass: every plane element of the window is read once and every output element written once, C sizeof(type) + 8 (+ 4)
// bytes per cell.  A block takes chunks of 1 024 consecutive cells of the window (row-major, so a chunk may run over a row end),
// four cells per lane 256 apart: every load and store of a wave is 64 consecutive elements.  The work is the search of V sorted
// tables per cell.  The tables stay in global memory (cfg3's 5 000 stations x 5 variables are 200 KB; they live in L2); a
// COARSE table -- every 64th value of every variable -- is staged in LDS once per block, and blocks are persistent (grid-stride
// over the chunks), so it is staged a few hundred times and not once per chunk.  A count is a binary search of the coarse
// values in LDS and six steps in the 512-byte segment it selects.  Past MESS_LDS_DOUBLES staged doubles the coarse table is
// read from global memory instead: the same code on another pointer, so both sides of the threshold give the same bits.  The
// running minimum and its variable stay in registers; no atomics: the same inputs give the same bits.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <mutex>
#include <vector>
#include "ensemble_int.h"
#include "mess_rule.h"

struct mhs_mess {
    int n = 0, V = 0, nc = 0;         // reference rows, variables, coarse values per variable (ceil(n / 64))
    double *tab = nullptr;            // device: sorted values [V x n], coarse [V x nc], min [V], max [V]
    int device = -1;
};

namespace mhs {

constexpr int MESS_NT = 256;                      // threads per block
constexpr int MESS_R = 4;                         // cells per lane
constexpr int MESS_CHUNK = MESS_NT * MESS_R;      // cells per chunk
constexpr int MESS_LDS_DOUBLES = 4096;            // V (nc + 2) doubles at most are staged (32 KiB); beyond, the coarse table stays global
constexpr int MESS_MAX_VARS = MESS_LDS_DOUBLES / 2;

struct MessTab {
    const double *sorted, *coarse;    // coarse is followed by min [V], max [V]
    int n, nc, V;
};

template <typename T, bool COARSE_LDS, bool MOD>
__global__ __launch_bounds__(MESS_NT) void mess_kernel(const MessTab t, const StackDev s, const PredGeom g, const int64_t n_chunks,
                                                       double *__restrict__ out, int32_t *__restrict__ mod, const int64_t ld_mod) {
    extern __shared__ double mess_sm[];
    {   // the coarse table with min / max behind it, or min / max alone
        const int count = COARSE_LDS ? t.V * (t.nc + 2) : 2 * t.V;
        const double *src = COARSE_LDS ? t.coarse : t.coarse + (size_t)t.V * t.nc;
        for (int e = threadIdx.x; e < count; e += MESS_NT) mess_sm[e] = src[e];
    }
    __syncthreads();
    const double *mn = COARSE_LDS ? mess_sm + t.V * t.nc : mess_sm, *mx = mn + t.V;
    const int top = mess_top(t.nc);
    const T *planes = (const T *)s.data;
    const unsigned nc = (unsigned)g.nc;
    for (int64_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        const int64_t first = ch * MESS_CHUNK;
        const int64_t row0 = first / g.nc;
        const unsigned col0 = (unsigned)(first - row0 * g.nc);
        int row[MESS_R], col[MESS_R], bv[MESS_R];
        bool in[MESS_R], na[MESS_R];
        double best[MESS_R];
#pragma unroll
        for (int k = 0; k < MESS_R; ++k) {
            const unsigned off = col0 + threadIdx.x + (unsigned)k * MESS_NT, q = off / nc;     // < 2^31 + 1 024
            const int64_t r = row0 + q;
            in[k] = r < g.nr;
            row[k] = in[k] ? (int)r : 0;
            col[k] = in[k] ? (int)(off - q * nc) : 0;
            na[k] = false; bv[k] = 0; best[k] = 0.0;
        }
        for (int v = 0; v < t.V; ++v) {
            double p[MESS_R];
            int lo[MESS_R], cnt[MESS_R];
#pragma unroll
            for (int k = 0; k < MESS_R; ++k) {
                const int64_t ar = g.r0 + row[k], ac = g.c0 + col[k];
                if (v < s.C) {
                    p[k] = in[k] ? (double)planes[(int64_t)v * s.plane_stride + ar * s.ld + ac] : 0.0;
                    if (s.has_nodata && p[k] == s.nodata) p[k] = NAN;
                } else if (v == s.C) p[k] = g.xmin + ((double)ac + 0.5) * g.xres;      // LONG, as ensemble_int.h:predictor()
                else p[k] = g.ymax - ((double)ar + 0.5) * g.yres;                      // LAT
                na[k] |= p[k] != p[k];
                lo[k] = 0;
            }
            const double *cv = COARSE_LDS ? mess_sm + v * t.nc : t.coarse + (size_t)v * t.nc;
            for (int st = top; st > 0; st >>= 1) {
#pragma unroll
                for (int k = 0; k < MESS_R; ++k) lo[k] = mess_step(cv, t.nc, p[k], lo[k], st);
            }
            const double *rv = t.sorted + (size_t)v * t.n;
            int seg[MESS_R], m[MESS_R];
#pragma unroll
            for (int k = 0; k < MESS_R; ++k) {      // the segment the coarse count selects: its first value is <= p.  lo == 0 (p below
                seg[k] = lo[k] > 0 ? (lo[k] - 1) * MESS_SEG : 0;       // every value, or NaN): segment 0 is searched and not used
                m[k] = min(t.n - seg[k], MESS_SEG);
                cnt[k] = 1;
            }
            for (int st = MESS_SEG / 2; st > 0; st >>= 1) {
#pragma unroll
                for (int k = 0; k < MESS_R; ++k) cnt[k] = mess_step(rv + seg[k], m[k], p[k], cnt[k], st);
            }
            const double vmn = mn[v], vmx = mx[v];
#pragma unroll
            for (int k = 0; k < MESS_R; ++k) {
                const int i = lo[k] > 0 ? seg[k] + cnt[k] : 0;
                const double sv = mess_value(p[k], i, t.n, vmn, vmx);
                if (v == 0 || sv < best[k]) { best[k] = sv; bv[k] = v; }
            }
        }
#pragma unroll
        for (int k = 0; k < MESS_R; ++k) {
            if (!in[k]) continue;
            out[(int64_t)row[k] * g.ld_out + col[k]] = na[k] ? NAN : best[k];
            if (MOD) mod[(int64_t)row[k] * ld_mod + col[k]] = na[k] ? -1 : bv[k];
        }
    }
}

template <typename T>
static void launch_mess_t(const MessTab &t, const StackDev &s, const PredGeom &g, int64_t n_chunks, unsigned blocks, bool lds,
                          double *out, int32_t *mod, int64_t ld_mod, hipStream_t st) {
    const size_t sm = sizeof(double) * (size_t)(lds ? t.V * (t.nc + 2) : 2 * t.V);
    if (lds && mod) hipLaunchKernelGGL((mess_kernel<T, true, true>), dim3(blocks), dim3(MESS_NT), sm, st, t, s, g, n_chunks, out, mod, ld_mod);
    else if (lds) hipLaunchKernelGGL((mess_kernel<T, true, false>), dim3(blocks), dim3(MESS_NT), sm, st, t, s, g, n_chunks, out, mod, ld_mod);
    else if (mod) hipLaunchKernelGGL((mess_kernel<T, false, true>), dim3(blocks), dim3(MESS_NT), sm, st, t, s, g, n_chunks, out, mod, ld_mod);
    else hipLaunchKernelGGL((mess_kernel<T, false, false>), dim3(blocks), dim3(MESS_NT), sm, st, t, s, g, n_chunks, out, mod, ld_mod);
}

// MESS (and MoD when mod != NULL) of the window g from the planes s; s.C planes, then LONG and LAT when the table has two more
static int launch_mess(const mhs_mess *m, const StackDev &s, const PredGeom &g, double *out, int32_t *mod, int64_t ld_mod,
                       hipStream_t st) {
    const int64_t cells = (int64_t)g.nr * g.nc;
    if (cells == 0) return MHS_OK;
    const int64_t n_chunks = (cells + MESS_CHUNK - 1) / MESS_CHUNK;
    const int n_cu = ctx().n_cu > 0 ? ctx().n_cu : 256;
    const unsigned blocks = (unsigned)std::min<int64_t>(n_chunks, (int64_t)n_cu * 4);
    const MessTab t{m->tab, m->tab + (size_t)m->V * m->n, m->n, m->nc, m->V};
    const bool lds = (int64_t)m->V * (m->nc + 2) <= MESS_LDS_DOUBLES;
    if (s.dtype == MHS_F64) launch_mess_t<double>(t, s, g, n_chunks, blocks, lds, out, mod, ld_mod, st);
    else if (s.dtype == MHS_F32) launch_mess_t<float>(t, s, g, n_chunks, blocks, lds, out, mod, ld_mod, st);
    else launch_mess_t<short>(t, s, g, n_chunks, blocks, lds, out, mod, ld_mod, st);
    MHS_HIP(hipGetLastError());
    return MHS_OK;
}

static int mess_args(const mhs_mess *m, const mhs_grid *g, const mhs_stack *c) {
    MHS_REQUIRE(m && g && c, "NULL argument");
    MHS_REQUIRE(c->n_layers >= 0 && (m->V == c->n_layers || m->V == c->n_layers + 2),
                "the reference table must have as many variables as the stack has layers, or two more (LONG, LAT)");
    MHS_REQUIRE(c->data || c->n_layers == 0, "covariate stack is NULL");
    MHS_REQUIRE(c->dtype == MHS_F64 || c->dtype == MHS_F32 || c->dtype == MHS_I16, "bad stack dtype");
    MHS_REQUIRE(c->ld >= g->ncol && c->plane_stride >= c->ld * g->nrow, "stack strides smaller than the grid");
    return MHS_OK;
}

}  // namespace mhs

using namespace mhs;

extern "C" {

int mhs_mess_create(const double *ref, int64_t n_ref, int n_vars, mhs_mess **out) {
    MHS_REQUIRE(ref && out, "NULL argument");
    *out = nullptr;
    MHS_REQUIRE(n_vars >= 1, "n_vars must be at least 1");
    MHS_REQUIRE(n_ref >= 2, "n_ref must be at least 2: a variable needs two distinct station values");
    MHS_REQUIRE(n_vars <= MESS_MAX_VARS, "too many variables (at most 2 048)");
    MHS_REQUIRE(n_ref * (int64_t)n_vars < (1LL << 31), "reference table too large (n_ref n_vars must stay below 2^31)");
    for (int v = 0; v < n_vars; ++v)
        for (int64_t i = 0; i < n_ref; ++i)
            if (!std::isfinite(ref[(size_t)v * n_ref + i])) {
                set_error("mhs_mess_create: row %lld of variable %d (both 0-based) is not finite: drop NA rows first, V73:154", (long long)i, v);
                return MHS_ERR_INVALID;
            }
    const int n = (int)n_ref, nc = (n + MESS_SEG - 1) / MESS_SEG;
    std::vector<double> h((size_t)n_vars * (n + nc + 2));
    double *coarse = h.data() + (size_t)n_vars * n, *mn = coarse + (size_t)n_vars * nc, *mx = mn + n_vars;
    for (int v = 0; v < n_vars; ++v) {
        double *r = h.data() + (size_t)v * n;
        std::copy(ref + (size_t)v * n, ref + (size_t)(v + 1) * n, r);
        std::sort(r, r + n);
        if (!(r[n - 1] > r[0])) {
            set_error("mhs_mess_create: variable %d (0-based) is constant over the reference rows: it has no range to place a cell in", v);
            return MHS_ERR_INVALID;
        }
        for (int k = 0; k < nc; ++k) coarse[(size_t)v * nc + k] = r[(size_t)k * MESS_SEG];
        mn[v] = r[0]; mx[v] = r[n - 1];
    }
    if (int rc = require_ready()) return rc;
    mhs_mess *m = new mhs_mess;
    m->n = n; m->V = n_vars; m->nc = nc; m->device = ctx().device;
    if (hipMalloc((void **)&m->tab, sizeof(double) * h.size()) != hipSuccess) {
        (void)hipGetLastError();
        delete m;
        set_error("mhs_mess_create: out of device memory (%zu bytes)", sizeof(double) * h.size());
        return MHS_ERR_ALLOC;
    }
    if (int rc = h2d_sync(m->tab, h.data(), sizeof(double) * h.size())) { (void)hipFree(m->tab); delete m; return rc; }
    *out = m;
    return MHS_OK;
}

int mhs_mess_free(mhs_mess *m) {
    if (!m) return MHS_OK;
    if (m->tab) { (void)hipDeviceSynchronize(); (void)hipFree(m->tab); }
    delete m;
    return MHS_OK;
}

int mhs_mess_grid_dev(const mhs_mess *m, const mhs_grid *g, const mhs_stack *covars, int64_t r0, int64_t r1, int64_t c0,
                      int64_t c1, double *out_dev, int64_t ld, int32_t *mod_dev, int64_t ld_mod, void *stream) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(out_dev, "NULL argument");
    if (int rc = mess_args(m, g, covars)) return rc;
    PredGeom pg;
    if (int rc = make_geom(g, r0, r1, c0, c1, ld, &pg)) return rc;
    MHS_REQUIRE(!mod_dev || ld_mod >= c1 - c0, "ld_mod smaller than the window width");
    const StackDev s{covars->data, covars->n_layers, covars->dtype, covars->plane_stride, covars->ld, covars->nodata,
                     !std::isnan(covars->nodata), 0};
    return launch_mess(m, s, pg, out_dev, mod_dev, ld_mod, pick_stream(stream));
}

// Host planes in, host planes out: row bands of the window go up, through the kernel and down again on one stream of the
// library's host-pointer pipeline (its persistent arena: no allocation per call).  A band is described with the parent
// grid's affine (rows_stack), so its cells get the whole-grid plane's bits.  Nothing is overlapped: the call is bound by the
// copies either way.  MHS_HOST_BANDS = n forces n equal bands, as it does for mhs_ensemble_predict.
int mhs_mess_grid(const mhs_mess *m, const mhs_grid *g, const mhs_stack *covars, int64_t r0, int64_t r1, int64_t c0, int64_t c1,
                  double *out_host, int32_t *mod_host) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(out_host, "NULL argument");
    if (int rc = mess_args(m, g, covars)) return rc;
    PredGeom whole;
    if (int rc = make_geom(g, r0, r1, c0, c1, c1 - c0, &whole)) return rc;
    const int64_t nr = r1 - r0, nc = c1 - c0;
    if (nr == 0 || nc == 0) return MHS_OK;
    const size_t esz = dtype_bytes(covars->dtype);
    const size_t row_bytes = (size_t)covars->n_layers * covars->ld * esz + (size_t)nc * 12 + 64;
    int64_t rows_per = std::max<int64_t>(1, std::min<int64_t>(nr, (int64_t)(((size_t)256 << 20) / row_bytes)));
    if (const char *e = getenv("MHS_HOST_BANDS")) {
        const int64_t nb = std::max<int64_t>(1, std::min<int64_t>(nr, atoll(e)));
        rows_per = (nr + nb - 1) / nb;
    }
    const size_t in_bytes = ((size_t)rows_per * covars->ld * esz * (size_t)covars->n_layers + 255) & ~(size_t)255;
    const size_t out_bytes = ((size_t)rows_per * nc * sizeof(double) + 255) & ~(size_t)255;
    const size_t mod_bytes = mod_host ? ((size_t)rows_per * nc * sizeof(int32_t) + 255) & ~(size_t)255 : 0;
    std::lock_guard<std::mutex> lk(pipe_mutex());
    if (int rc = host_pipe(in_bytes + out_bytes + mod_bytes)) return rc;
    Context &c = ctx();
    hipStream_t st = c.pipe_comp;
    char *in = c.pipe_arena;
    double *outb = (double *)(c.pipe_arena + in_bytes);
    int32_t *modb = mod_host ? (int32_t *)(c.pipe_arena + in_bytes + out_bytes) : nullptr;
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{st};   // no copy is left in flight, whatever the exit
    for (int64_t b0 = r0; b0 < r1; b0 += rows_per) {
        const int64_t b1 = std::min(r1, b0 + rows_per);
        const size_t plane_bytes = (size_t)(b1 - b0) * covars->ld * esz;
        for (int k = 0; k < covars->n_layers; ++k)
            MHS_HIP(hipMemcpyAsync(in + plane_bytes * k, (const char *)covars->data + ((size_t)k * covars->plane_stride + (size_t)b0 * covars->ld) * esz,
                                   plane_bytes, hipMemcpyHostToDevice, st));
        PredGeom pg;
        if (int rc = make_geom(g, b0, b1, c0, c1, nc, &pg)) return rc;
        const StackDev sd = rows_stack(in, b0, b1, covars->n_layers, covars->dtype, covars->ld, covars->nodata);
        if (int rc = launch_mess(m, sd, pg, outb, modb, nc, st)) return rc;
        MHS_HIP(hipMemcpyAsync(out_host + (size_t)(b0 - r0) * nc, outb, sizeof(double) * (size_t)((b1 - b0) * nc), hipMemcpyDeviceToHost, st));
        if (mod_host)
            MHS_HIP(hipMemcpyAsync(mod_host + (size_t)(b0 - r0) * nc, modb, sizeof(int32_t) * (size_t)((b1 - b0) * nc), hipMemcpyDeviceToHost, st));
        MHS_HIP(hipStreamSynchronize(st));       // the next band reuses the three buffers
    }
    return MHS_OK;
}

// the n x V table X as V "planes" of one row: every variable, LONG and LAT among them, comes from its column
int mhs_mess_points(const mhs_mess *m, const double *X, int64_t n, double *out_host, int32_t *mod_host) {
    if (int rc = require_ready()) return rc;
    MHS_REQUIRE(m && out_host && (X || n == 0) && n >= 0 && n < (1LL << 31), "bad arguments");
    if (n == 0) return MHS_OK;
    hipStream_t st = ctx().stream;
    DevBuf<double> dx, dout;
    DevBuf<int32_t> dmod;
    MHS_HIP(dx.alloc((size_t)n * m->V));
    MHS_HIP(dout.alloc((size_t)n));
    if (mod_host) MHS_HIP(dmod.alloc((size_t)n));
    MHS_HIP(hipMemcpyAsync(dx.p, X, sizeof(double) * (size_t)n * m->V, hipMemcpyHostToDevice, st));
    const StackDev s{dx.p, m->V, MHS_F64, n, n, NAN, 0, 1};
    const PredGeom pg{0, 0, 1, 1, 0, 0, 1, (int)n, n};
    if (int rc = launch_mess(m, s, pg, dout.p, mod_host ? dmod.p : nullptr, n, st)) return rc;
    MHS_HIP(hipMemcpyAsync(out_host, dout.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    if (mod_host) MHS_HIP(hipMemcpyAsync(mod_host, dmod.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
    MHS_HIP(hipStreamSynchronize(st));
    return MHS_OK;
}

}  // extern "C"
