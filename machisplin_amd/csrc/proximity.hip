// Exact Euclidean proximity of one plane (include/machisplin_hip.h, section "proximity", states the rule; proximity_rule.h
// holds it): for every cell the nearest feature cell, in integer arithmetic, and the products made from it.
//
// Three phases, three launches, no host decision between them:
//   A   prox_rows_kernel   one WAVE per row.  The wave goes over the row in chunks of PROX_CHUNK = 64 columns, lane l at column
//                          64 k + l, so every load and store is 64 consecutive elements.  Left to right an inclusive wave
//                          max-scan of (feature ? column : -1) with a carry from chunk to chunk gives the nearest feature at or
//                          left of each cell; right to left a suffix min-scan gives the one at or right of it; the nearer of the
//                          two (left on a tie) is near(r, c).  The features are counted by ballot on the way.
//   B1  prox_cols_kernel   one LANE per column, 64 adjacent columns per wave, walking DOWN the rows: at every row the wave reads
//                          64 consecutive near() values, and entry k of the 64 columns' stacks are 64 consecutive ints too --
//                          lanes down a column would touch addresses ncol apart.  The phase is a chain of nrow dependent
//                          steps per lane, so what counts is the latency of a step: a lane keeps the top of its stack in
//                          registers (a row that pops nothing reads nothing back) and the PROX_TOP = 16 entries below it in
//                          LDS (a pop reads LDS, not global memory, unless it goes deeper); near() is loaded PROX_PRELOAD rows
//                          ahead.  Rows without a feature are skipped, never entered with a stand-in value.
//   B2  prox_cells_kernel  one lane per column and band of PROX_BAND = 32 rows: a binary search finds the envelope segment of
//                          the band's first row, a monotone walk follows it down the band, and every requested product of a
//                          cell is written in the one pass.
// Every loop is bounded by the grid: the chunk loops by ncol, the pop loop and the walk by the stack height <= nrow (and by nrow
// itself), the search by 32 steps.
//
// Scratch, per cell: near 4 + stack rows 4 + stack first-rows 4 = 12 bytes, plus 4 bytes per column (the stack heights) and two
// counters, in ONE block of stream-ordered memory given back behind the last kernel.  LDS: 12 KiB per wave of B1.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <mutex>
#include "ensemble_int.h"
#include "proximity_rule.h"

namespace mhs {

constexpr int PX_NT = 256;                   // threads per workgroup of phases A and B2: 4 waves
constexpr int PX_WAVES = PX_NT / 64;

struct ProxGeom {
    int nrow, ncol;
    double nodata;
    int has_nodata;
};

struct ProxCounters {
    unsigned long long n_features;
    int max_d2;
    int pad;
};

// A
template <typename T>
__global__ __launch_bounds__(PX_NT) void prox_rows_kernel(const ProxGeom g, const T *__restrict__ z, const int64_t ldz, const int where,
                                                          const double threshold, int32_t *__restrict__ near, ProxCounters *counters) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool has_nd = g.has_nodata != 0;
    const int n_chunks = (g.ncol + PROX_CHUNK - 1) / PROX_CHUNK;
    unsigned long long n_feat = 0;
    for (int64_t row = (int64_t)blockIdx.x * PX_WAVES + wave; row < g.nrow; row += (int64_t)gridDim.x * PX_WAVES) {
        const T *zr = z + row * ldz;
        int32_t *nr = near + row * g.ncol;
        int carry = -1;
        for (int ch = 0; ch < n_chunks; ++ch) {
            const int c = ch * PROX_CHUNK + lane;
            const bool f = c < g.ncol && prox_is_feature((double)zr[c], has_nd, g.nodata, where, threshold);
            n_feat += (unsigned long long)__popcll(__ballot(f));
            int v = f ? c : -1;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int t = __shfl_up(v, d, 64);
                if (lane >= d) v = max(v, t);
            }
            v = max(v, carry);
            carry = __shfl(v, 63, 64);
            if (c < g.ncol) nr[c] = v;
        }
        carry = PROX_NONE;
        for (int ch = n_chunks - 1; ch >= 0; --ch) {
            const int c = ch * PROX_CHUNK + lane;
            const bool f = c < g.ncol && prox_is_feature((double)zr[c], has_nd, g.nodata, where, threshold);
            int v = f ? c : PROX_NONE;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int t = __shfl_down(v, d, 64);
                if (lane + d < 64) v = min(v, t);
            }
            v = min(v, carry);
            carry = __shfl(v, 0, 64);
            if (c < g.ncol) nr[c] = prox_nearer_in_row(c, nr[c], v == PROX_NONE ? -1 : v);
        }
    }
    if (lane == 0 && n_feat) atomicAdd(&counters->n_features, n_feat);
}

// the stack of column `col` in global scratch: entry k of all columns side by side
struct ProxDevStack {
    const int32_t *near;
    int32_t *srow, *sfrom;
    int col, ncol;
    __device__ int row(int k) const { return srow[(int64_t)k * ncol + col]; }
    __device__ int from(int k) const { return sfrom[(int64_t)k * ncol + col]; }
    __device__ int64_t h(int, int r) const {
        const int64_t d = (int64_t)col - near[(int64_t)r * ncol + col];
        return d * d;
    }
    __device__ void set(int k, int r, int f, int64_t) {
        srow[(int64_t)k * ncol + col] = r;
        sfrom[(int64_t)k * ncol + col] = f;
    }
};

// The same stack while B1 builds it: every push goes to global memory AND into slot k % PROX_TOP of the lane's window in LDS
// (row, first row, h; slot s of lane l at word s * 64 + l, so the lanes of a wave never share a bank), and an entry is read back
// from the window while it is there.  `base`: entries base .. height - 1 are in the window.  A push at k overwrites entry
// k - PROX_TOP (base rises to k - PROX_TOP + 1) and, after pops below base, restarts the window at k.  A pop sequence that goes
// below base reads global memory, as ProxDevStack does.
struct ProxBuildStack {
    ProxDevStack g;
    int *w_row, *w_from, *w_h;        // this lane's column of the three windows
    int base;
    __device__ int row(int k) const { return k >= base ? w_row[(k % PROX_TOP) * 64] : g.row(k); }
    __device__ int from(int k) const { return k >= base ? w_from[(k % PROX_TOP) * 64] : g.from(k); }
    __device__ int64_t h(int k, int r) const { return k >= base ? (int64_t)w_h[(k % PROX_TOP) * 64] : g.h(k, r); }
    __device__ void set(int k, int r, int f, int64_t hh) {
        g.set(k, r, f, hh);
        const int s = (k % PROX_TOP) * 64;
        w_row[s] = r; w_from[s] = f; w_h[s] = (int)hh;                 // h <= (ncol - 1)^2 <= INT32_MAX
        if (k < base) base = k;
        base = max(base, k - PROX_TOP + 1);
    }
};

// B1
__global__ __launch_bounds__(64) void prox_cols_kernel(const ProxGeom g, const int32_t *near, int32_t *srow, int32_t *sfrom,
                                                       int32_t *__restrict__ height) {
    __shared__ int window[3 * PROX_TOP * 64];
    const int col = blockIdx.x * 64 + threadIdx.x;
    if (col >= g.ncol) return;
    ProxBuildStack s{ProxDevStack{near, srow, sfrom, col, g.ncol}, window + threadIdx.x, window + PROX_TOP * 64 + threadIdx.x,
                     window + 2 * PROX_TOP * 64 + threadIdx.x, 0};
    ProxEnv e;
    for (int r0 = 0; r0 < g.nrow; r0 += PROX_PRELOAD) {
        int fc[PROX_PRELOAD];
#pragma unroll
        for (int j = 0; j < PROX_PRELOAD; ++j) fc[j] = r0 + j < g.nrow ? near[(int64_t)(r0 + j) * g.ncol + col] : -1;
#pragma unroll
        for (int j = 0; j < PROX_PRELOAD; ++j) {
            if (fc[j] < 0) continue;
            const int64_t d = (int64_t)col - fc[j];
            prox_env_add(s, e, r0 + j, d * d, g.nrow);
        }
    }
    height[col] = e.k;
}

struct ProxPlanes {
    int32_t *d2, *index;
    void *dist, *dir_x, *dir_y, *value;
};

// B2.  V: the type of the value layer's plane; O: the type of the float products
template <typename V, typename O>
__global__ __launch_bounds__(PX_NT) void prox_cells_kernel(const ProxGeom g, const int32_t *__restrict__ near, const int32_t *__restrict__ srow,
                                                           const int32_t *__restrict__ sfrom, const int32_t *__restrict__ height,
                                                           const V *__restrict__ vz, const int64_t ldv, const double unit, const ProxPlanes p,
                                                           const int64_t ld, ProxCounters *counters) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col = blockIdx.x * 64 + lane;
    const int r_begin = (blockIdx.y * PX_WAVES + wave) * PROX_BAND;
    const int r_end = min(r_begin + PROX_BAND, g.nrow);
    const bool has_nd = g.has_nodata != 0;
    O *dist = (O *)p.dist, *dir_x = (O *)p.dir_x, *dir_y = (O *)p.dir_y, *value = (O *)p.value;
    int far = 0;
    if (col < g.ncol && r_begin < g.nrow) {
        const ProxDevStack s{near, const_cast<int32_t *>(srow), const_cast<int32_t *>(sfrom), col, g.ncol};
        const int cnt = height[col];
        int k = 0, fr = -1, fc = -1, next_from = PROX_NONE;
        if (cnt > 0) {
            k = prox_segment(s, cnt, r_begin);
            fr = s.row(k);
            fc = near[(int64_t)fr * g.ncol + col];
            next_from = k + 1 < cnt ? s.from(k + 1) : PROX_NONE;
        }
        for (int r = r_begin; r < r_end; ++r) {
            if (next_from <= r) {
                for (int it = 0; it < cnt && next_from <= r; ++it) {
                    ++k;
                    next_from = k + 1 < cnt ? s.from(k + 1) : PROX_NONE;
                }
                fr = s.row(k);
                fc = near[(int64_t)fr * g.ncol + col];
            }
            const int64_t o = (int64_t)r * ld + col;
            const int d2 = fr < 0 ? -1 : (int)prox_d2(r, col, fr, fc);
            far = max(far, d2);
            if (p.d2) p.d2[o] = d2;
            if (p.index) p.index[o] = fr < 0 ? -1 : (int32_t)prox_index(fr, fc, g.ncol);
            if (dist || dir_x || dir_y) {
                const ProxFloat f = prox_float(r, col, fr, fc, unit);
                if (dist) dist[o] = (O)f.dist;
                if (dir_x) dir_x[o] = (O)f.dir_x;
                if (dir_y) dir_y[o] = (O)f.dir_y;
            }
            if (value) {
                double v = NAN;
                if (fr >= 0) {
                    v = (double)vz[(int64_t)fr * ldv + fc];
                    if (prox_na(v, has_nd, g.nodata)) v = NAN;
                }
                value[o] = (O)v;
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) far = max(far, __shfl_xor(far, d, 64));
    if (lane == 0 && far > 0) atomicMax(&counters->max_d2, far);
}

#define PX_REQUIRE(cond, ...)                                              \
    do {                                                                   \
        if (!(cond)) { set_error(__VA_ARGS__); return MHS_ERR_INVALID; }    \
    } while (0)

// Every check of a proximity call, before any device call; fn = the entry point's name for the message
static int prox_check(const char *fn, const mhs_grid *grid, const mhs_stack *stack, int layer, int where, double threshold, int value_layer,
                      double unit, const mhs_proximity_out *out, int out_dtype, int64_t ld, ProxGeom *g) {
    PX_REQUIRE(grid && stack && out, "%s: NULL argument (g, stack or out)", fn);
    PX_REQUIRE(grid->nrow > 0 && grid->ncol > 0 && grid->nrow < (1LL << 30) && grid->ncol < (1LL << 30),
               "%s: bad grid geometry (nrow, ncol must be in 1 .. 2^30)", fn);
    PX_REQUIRE((grid->nrow - 1) * (grid->nrow - 1) + (grid->ncol - 1) * (grid->ncol - 1) <= (int64_t)INT32_MAX,
               "%s: grid too large: (nrow - 1)^2 + (ncol - 1)^2 must not pass 2^31 - 1 (d2 is an int32)", fn);
    PX_REQUIRE(grid->nrow * grid->ncol <= (int64_t)INT32_MAX, "%s: grid too large: nrow * ncol must not pass 2^31 - 1 (index is an int32)", fn);
    PX_REQUIRE(stack->data, "%s: stack data is NULL", fn);
    PX_REQUIRE(stack->dtype == MHS_F64 || stack->dtype == MHS_F32 || stack->dtype == MHS_I16, "%s: bad stack dtype", fn);
    PX_REQUIRE(layer >= 0 && layer < stack->n_layers, "%s: layer %d is not one of the stack's %d layers", fn, layer, stack->n_layers);
    PX_REQUIRE(stack->ld >= grid->ncol && (stack->n_layers == 1 || stack->plane_stride >= stack->ld * (grid->nrow - 1) + grid->ncol),
               "%s: stack strides smaller than the grid", fn);
    PX_REQUIRE(where >= 0 && where < PROX_WHERES, "%s: unknown where %d (MHS_PROX_NA .. MHS_PROX_NE)", fn, where);
    PX_REQUIRE(where < PROX_LT || !std::isnan(threshold), "%s: threshold must not be NaN for a comparison", fn);
    PX_REQUIRE(std::isfinite(unit) && unit > 0.0, "%s: unit must be finite and positive", fn);
    PX_REQUIRE(out->d2 || out->index || out->dist || out->dir_x || out->dir_y || out->value,
               "%s: out names no product (d2, index, dist, dir_x, dir_y, value are all NULL)", fn);
    PX_REQUIRE(!out->value || (value_layer >= 0 && value_layer < stack->n_layers),
               "%s: value_layer %d is not one of the stack's %d layers", fn, value_layer, stack->n_layers);
    PX_REQUIRE(out_dtype == MHS_F64 || out_dtype == MHS_F32, "%s: out_dtype must be MHS_F64 or MHS_F32", fn);
    PX_REQUIRE(ld >= grid->ncol, "%s: ld smaller than the grid width", fn);
    *g = ProxGeom{(int)grid->nrow, (int)grid->ncol, stack->nodata, !std::isnan(stack->nodata)};
    return MHS_OK;
}

// the call's one block of stream-ordered memory, given back behind whatever was enqueued last
struct ProxScratch {
    char *p = nullptr;
    hipStream_t st = nullptr;
    ~ProxScratch() { if (p) (void)hipFreeAsync(p, st); }
};

static size_t px_align(size_t n) { return (n + 255) & ~(size_t)255; }

template <typename T>
static void launch_prox_rows(const ProxGeom &g, unsigned nb, hipStream_t st, const void *z, int64_t ldz, int where, double threshold, int32_t *near,
                             ProxCounters *counters) {
    hipLaunchKernelGGL((prox_rows_kernel<T>), dim3(nb), dim3(PX_NT), 0, st, g, (const T *)z, ldz, where, threshold, near, counters);
}
template <typename V, typename O>
static void launch_prox_cells(const ProxGeom &g, dim3 grid, hipStream_t st, const int32_t *near, const int32_t *srow, const int32_t *sfrom,
                              const int32_t *height, const void *vz, int64_t ldv, double unit, const ProxPlanes &p, int64_t ld,
                              ProxCounters *counters) {
    hipLaunchKernelGGL((prox_cells_kernel<V, O>), grid, dim3(PX_NT), 0, st, g, near, srow, sfrom, height, (const V *)vz, ldv, unit, p, ld, counters);
}
template <typename V>
static void launch_prox_cells_o(int out_dtype, const ProxGeom &g, dim3 grid, hipStream_t st, const int32_t *near, const int32_t *srow,
                                const int32_t *sfrom, const int32_t *height, const void *vz, int64_t ldv, double unit, const ProxPlanes &p,
                                int64_t ld, ProxCounters *counters) {
    if (out_dtype == MHS_F64) launch_prox_cells<V, double>(g, grid, st, near, srow, sfrom, height, vz, ldv, unit, p, ld, counters);
    else launch_prox_cells<V, float>(g, grid, st, near, srow, sfrom, height, vz, ldv, unit, p, ld, counters);
}

// Device planes.  `plane` = element (0, 0) of the feature layer, `vplane` of the value layer (read only when out.value is set);
// both of `dtype` with the row stride ldz.
static int prox_run(const char *fn, const ProxGeom &g, int dtype, const void *plane, const void *vplane, int64_t ldz, int where, double threshold,
                    double unit, const mhs_proximity_out &out, int out_dtype, int64_t ld, hipStream_t st, mhs_proximity_info *info) {
    const size_t n = (size_t)g.nrow * (size_t)g.ncol;
    const size_t o_near = 0, o_row = o_near + px_align(4 * n), o_from = o_row + px_align(4 * n), o_h = o_from + px_align(4 * n),
                 o_cnt = o_h + px_align(4 * (size_t)g.ncol), total = o_cnt + px_align(sizeof(ProxCounters));
    ProxScratch s;
    s.st = st;
    if (hipMallocAsync((void **)&s.p, total, st) != hipSuccess) {
        (void)hipGetLastError();
        s.p = nullptr;
        set_error("%s: no device memory for the scratch planes (%zu bytes: 12 per cell)", fn, total);
        return MHS_ERR_ALLOC;
    }
    int32_t *near = (int32_t *)(s.p + o_near), *srow = (int32_t *)(s.p + o_row), *sfrom = (int32_t *)(s.p + o_from), *height = (int32_t *)(s.p + o_h);
    ProxCounters *counters = (ProxCounters *)(s.p + o_cnt);
    MHS_HIP(hipMemsetAsync(counters, 0, sizeof(ProxCounters), st));
    const int n_cu = ctx().n_cu > 0 ? ctx().n_cu : 256;
    const unsigned nb_rows = (unsigned)std::min<int64_t>(((int64_t)g.nrow + PX_WAVES - 1) / PX_WAVES, (int64_t)n_cu * 32);
    if (dtype == MHS_F64) launch_prox_rows<double>(g, nb_rows, st, plane, ldz, where, threshold, near, counters);
    else if (dtype == MHS_F32) launch_prox_rows<float>(g, nb_rows, st, plane, ldz, where, threshold, near, counters);
    else launch_prox_rows<short>(g, nb_rows, st, plane, ldz, where, threshold, near, counters);
    MHS_HIP(hipGetLastError());
    const unsigned col_groups = (unsigned)((g.ncol + 63) / 64);
    hipLaunchKernelGGL(prox_cols_kernel, dim3(col_groups), dim3(64), 0, st, g, near, srow, sfrom, height);
    MHS_HIP(hipGetLastError());
    const dim3 grid(col_groups, (unsigned)((g.nrow + PX_WAVES * PROX_BAND - 1) / (PX_WAVES * PROX_BAND)));
    const ProxPlanes p{out.d2, out.index, out.dist, out.dir_x, out.dir_y, out.value};
    const void *vz = out.value ? vplane : nullptr;
    if (dtype == MHS_F64) launch_prox_cells_o<double>(out_dtype, g, grid, st, near, srow, sfrom, height, vz, ldz, unit, p, ld, counters);
    else if (dtype == MHS_F32) launch_prox_cells_o<float>(out_dtype, g, grid, st, near, srow, sfrom, height, vz, ldz, unit, p, ld, counters);
    else launch_prox_cells_o<short>(out_dtype, g, grid, st, near, srow, sfrom, height, vz, ldz, unit, p, ld, counters);
    MHS_HIP(hipGetLastError());
    if (info) {
        ProxCounters c;
        MHS_HIP(hipMemcpyAsync(&c, counters, sizeof(c), hipMemcpyDeviceToHost, st));
        MHS_HIP(hipStreamSynchronize(st));
        *info = mhs_proximity_info{(int64_t)c.n_features, c.n_features ? (int64_t)c.max_d2 : -1, (int64_t)total};
    }
    return MHS_OK;
}

}  // namespace mhs

using namespace mhs;

extern "C" {

int mhs_proximity_dev(const mhs_grid *g, const mhs_stack *stack, int layer, int where, double threshold, int value_layer, double unit,
                      const mhs_proximity_out *out, int out_dtype, int64_t ld, void *stream, mhs_proximity_info *info) {
    ProxGeom pg;
    if (int rc = prox_check(__func__, g, stack, layer, where, threshold, value_layer, unit, out, out_dtype, ld, &pg)) return rc;
    if (int rc = require_ready()) return rc;
    const size_t esz = dtype_bytes(stack->dtype);
    const char *base = (const char *)stack->data;
    const void *plane = base + (size_t)layer * stack->plane_stride * esz;
    const void *vplane = out->value ? base + (size_t)value_layer * stack->plane_stride * esz : nullptr;
    return prox_run(__func__, pg, stack->dtype, plane, vplane, stack->ld, where, threshold, unit, *out, out_dtype, ld, pick_stream(stream), info);
}

// Host planes: the WHOLE feature plane (and the value layer's) goes up and the requested planes come down.  No row bands: the
// nearest feature of a cell may lie anywhere in the raster.
int mhs_proximity(const mhs_grid *g, const mhs_stack *stack, int layer, int where, double threshold, int value_layer, double unit,
                  const mhs_proximity_out *out, int out_dtype, mhs_proximity_info *info) {
    ProxGeom pg;
    const char *fn = __func__;
    if (int rc = prox_check(fn, g, stack, layer, where, threshold, value_layer, unit, out, out_dtype, g ? g->ncol : 0, &pg)) return rc;
    if (int rc = require_ready()) return rc;
    const size_t esz = dtype_bytes(stack->dtype), n = (size_t)pg.nrow * (size_t)pg.ncol, osz = out_dtype == MHS_F64 ? 8 : 4;
    const size_t in_bytes = ((size_t)(pg.nrow - 1) * stack->ld + pg.ncol) * esz;
    const bool second = out->value && value_layer != layer;
    void *const host[6] = {out->d2, out->index, out->dist, out->dir_x, out->dir_y, out->value};
    const size_t bytes[6] = {4 * n, 4 * n, n * osz, n * osz, n * osz, n * osz};
    size_t off[6], o_v = px_align(in_bytes), total = o_v + (second ? px_align(in_bytes) : 0);
    for (int k = 0; k < 6; ++k) { off[k] = total; total += host[k] ? px_align(bytes[k]) : 0; }
    std::lock_guard<std::mutex> lk(pipe_mutex());
    if (int rc = host_pipe(0)) return rc;                      // the pipeline's streams; its arena is not used
    hipStream_t st = ctx().pipe_comp;
    ProxScratch s;
    s.st = st;
    if (hipMallocAsync((void **)&s.p, total, st) != hipSuccess) {
        (void)hipGetLastError();
        s.p = nullptr;
        set_error("%s: no device memory for the plane and its outputs (%zu bytes)", fn, total);
        return MHS_ERR_ALLOC;
    }
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{st};   // no copy is left in flight, whatever the exit
    const char *base = (const char *)stack->data;
    MHS_HIP(hipMemcpyAsync(s.p, base + (size_t)layer * stack->plane_stride * esz, in_bytes, hipMemcpyHostToDevice, st));
    if (second) MHS_HIP(hipMemcpyAsync(s.p + o_v, base + (size_t)value_layer * stack->plane_stride * esz, in_bytes, hipMemcpyHostToDevice, st));
    void *dev[6];
    for (int k = 0; k < 6; ++k) dev[k] = host[k] ? s.p + off[k] : nullptr;
    const mhs_proximity_out dout{(int32_t *)dev[0], (int32_t *)dev[1], dev[2], dev[3], dev[4], dev[5]};
    if (int rc = prox_run(fn, pg, stack->dtype, s.p, second ? s.p + o_v : s.p, stack->ld, where, threshold, unit, dout, out_dtype, pg.ncol, st, info))
        return rc;
    for (int k = 0; k < 6; ++k)
        if (host[k]) MHS_HIP(hipMemcpyAsync(host[k], s.p + off[k], bytes[k], hipMemcpyDeviceToHost, st));
    MHS_HIP(hipStreamSynchronize(st));
    return MHS_OK;
}

}  // extern "C"
