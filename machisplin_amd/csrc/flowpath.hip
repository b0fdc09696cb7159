// Flow paths along a D8 direction forest (include/machisplin_hip.h, section "flow paths", states the rule; flowpath_rule.h
// holds it): for every cell the first target cell on its own path downhill, by POINTER DOUBLING, and the products made from it.
//
// Four phases:
//   1  flow_seed_kernel     a workgroup per 32 x 64 tile, a wave per row of it at a time: validates the direction code, evaluates
//                           the predicate, writes the cell's record (pointer, step counts) and counts valid cells, targets,
//                           roots and malformed cells.
//   2  flow_local_kernel    a workgroup per tile holds the tile's records in LDS and doubles inside the tile until every cell of
//                           it points at a stop cell or at a cell outside the tile: at most FLOW_LOCAL_ROUNDS = 12 rounds, each
//                           "all read, barrier, all write, barrier".  Skipped with MHS_FLOWPATH_NO_LOCAL.
//   3  flow_round_kernel    one doubling round over the whole plane, a lane per cell: reads the records of one buffer (its own,
//                           and by a gather its pointer's) and writes the OTHER buffer, so no launch reads a record that the same
//                           launch writes.  The cells that moved are counted; the host reads the count after every round (one
//                           stream synchronisation per round) and stops at zero, or after FLOW_MAX_ROUNDS = 32 launches.  A cell
//                           whose pointer's pointer is the cell itself is counted as a cycle and stays.
//   4  flow_products_kernel a workgroup per tile: every requested plane in one pass, each element written once.
// Phase 2 also reads one buffer and writes the other.  In 1, 2 and 4 a wave loads and stores 64 consecutive elements of a row;
// in 3, 64 consecutive records.  1, 3 and 4 run a bounded number of workgroups (16 per compute unit) that loop over tiles or
// cells and add to the call's counters once per wave at their end: with a wave per tile adding to one address, the atomics, not
// the memory traffic, set the time of a round at 10^8 cells (measured: 20 - 30 ms a round).
//
// Records: with the step counts (steps or dist asked for) 16 bytes {pointer, E-W, N-S, diagonal}, moved by one 128-bit access;
// without them the pointer alone, 4 bytes.  Scratch: two record buffers = 32 or 8 bytes per cell, plus the counters, in ONE
// block of stream-ordered memory given back behind the last kernel.  LDS of phase 2: 32 KiB or 8 KiB.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <mutex>
#include "ensemble_int.h"
#include "flowpath_rule.h"

namespace mhs {

constexpr int FP_NT = 256;                            // threads per workgroup: 4 waves
constexpr int FP_ROWS = FLOW_TH / (FP_NT / 64);       // rows of a tile a wave goes over: 8

struct FlowGeom {
    int nrow, ncol;
    int tiles_c;            // tiles per tile row
    double nodata;
    int has_nodata;
    int where;
    double threshold;
};

struct FlowCounters {
    unsigned long long n_valid, n_targets, n_roots, n_bad, n_cycle, n_unreached;
    unsigned long long moved[FLOW_MAX_ROUNDS];
    int max_steps_p1;       // the largest step count of a reached cell + 1; 0: no cell was reached
    int pad;
};

// the records of a plane: CNT = with the step counts
template <bool CNT> struct FlowRecs;
template <> struct FlowRecs<false> {
    int32_t *p;
    __device__ void load(int64_t i, int32_t &ptr, FlowCounts &) const { ptr = p[i]; }
    __device__ void store(int64_t i, int32_t ptr, const FlowCounts &) const { p[i] = ptr; }
};
template <> struct FlowRecs<true> {
    int4 *p;
    __device__ void load(int64_t i, int32_t &ptr, FlowCounts &n) const {
        const int4 v = p[i];
        ptr = v.x;
        n = FlowCounts{(uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w};
    }
    __device__ void store(int64_t i, int32_t ptr, const FlowCounts &n) const { p[i] = make_int4(ptr, (int)n.ew, (int)n.ns, (int)n.dg); }
};

__device__ inline unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// 1
template <typename T, bool CNT>
__global__ __launch_bounds__(FP_NT) void flow_seed_kernel(const FlowGeom g, const unsigned n_tiles, const int8_t *__restrict__ dir, const int64_t ld_dir,
                                                          const T *__restrict__ z, const int64_t ldz, const FlowRecs<CNT> dst,
                                                          FlowCounters *counters) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool has_nd = g.has_nodata != 0;
    unsigned long long n_valid = 0, n_targets = 0, n_roots = 0, n_bad = 0;
    for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int tr0 = (int)(tile / (unsigned)g.tiles_c) * FLOW_TH, tc0 = (int)(tile % (unsigned)g.tiles_c) * FLOW_TW;
        const int c = tc0 + lane;
#pragma unroll
        for (int k = 0; k < FP_ROWS; ++k) {
            const int r = tr0 + wave * FP_ROWS + k;
            if (r >= g.nrow || c >= g.ncol) continue;
            const bool target = g.where != FLOW_OUTLET && prox_is_feature((double)z[(int64_t)r * ldz + c], has_nd, g.nodata, g.where, g.threshold);
            int32_t ptr;
            FlowCounts n;
            const int kind = flow_seed(dir, ld_dir, r, c, g.nrow, g.ncol, target, &ptr, &n);
            dst.store((int64_t)r * g.ncol + c, ptr, n);
            n_valid += kind != FLOW_CELL_NA;
            n_targets += kind != FLOW_CELL_NA && target;
            n_roots += kind == FLOW_CELL_ROOT;
            n_bad += kind == FLOW_CELL_BAD;
        }
    }
    n_valid = wave_sum(n_valid); n_targets = wave_sum(n_targets); n_roots = wave_sum(n_roots); n_bad = wave_sum(n_bad);
    if (lane == 0) {
        if (n_valid) atomicAdd(&counters->n_valid, n_valid);
        if (n_targets) atomicAdd(&counters->n_targets, n_targets);
        if (n_roots) atomicAdd(&counters->n_roots, n_roots);
        if (n_bad) atomicAdd(&counters->n_bad, n_bad);
    }
}

// the tile's records in LDS, as flow_local_step reads them
struct FlowTile {
    const int *lp;
    const uint32_t *ew, *ns, *dg;
    __device__ int ptr(int j) const { return lp[j]; }
    __device__ FlowCounts cnt(int j) const { return FlowCounts{ew[j], ns[j], dg[j]}; }
};

// 2
template <bool CNT>
__global__ __launch_bounds__(FP_NT) void flow_local_kernel(const FlowGeom g, const FlowRecs<CNT> src, const FlowRecs<CNT> dst) {
    constexpr int NC = CNT ? FLOW_TILE : 1;
    __shared__ int lp[FLOW_TILE];
    __shared__ uint32_t l_ew[NC], l_ns[NC], l_dg[NC];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tr0 = (int)(blockIdx.x / (unsigned)g.tiles_c) * FLOW_TH, tc0 = (int)(blockIdx.x % (unsigned)g.tiles_c) * FLOW_TW;
    const int c = tc0 + lane;
    int p[FP_ROWS];
    FlowCounts n[FP_ROWS];
#pragma unroll
    for (int k = 0; k < FP_ROWS; ++k) {
        const int lr = wave * FP_ROWS + k, i = lr * FLOW_TW + lane, r = tr0 + lr;
        p[k] = i;                                                   // a slot beyond the raster's edge: a stop cell nobody points at
        n[k] = FlowCounts{0u, 0u, 0u};
        if (r < g.nrow && c < g.ncol) {
            int32_t ptr;
            src.load((int64_t)r * g.ncol + c, ptr, n[k]);
            p[k] = flow_to_local(ptr, tr0, tc0, g.ncol);
        }
        lp[i] = p[k];
        if (CNT) { l_ew[i] = n[k].ew; l_ns[i] = n[k].ns; l_dg[i] = n[k].dg; }
    }
    __syncthreads();
    const FlowTile tile{lp, l_ew, l_ns, l_dg};
    for (int round = 0; round < FLOW_LOCAL_ROUNDS; ++round) {
        int moved = 0;
#pragma unroll
        for (int k = 0; k < FP_ROWS; ++k) moved |= flow_local_step(tile, (wave * FP_ROWS + k) * FLOW_TW + lane, p[k], n[k], CNT);
        if (!__syncthreads_or(moved)) break;                        // every read of the round is made before any of its writes
#pragma unroll
        for (int k = 0; k < FP_ROWS; ++k) {
            const int i = (wave * FP_ROWS + k) * FLOW_TW + lane;
            lp[i] = p[k];
            if (CNT) { l_ew[i] = n[k].ew; l_ns[i] = n[k].ns; l_dg[i] = n[k].dg; }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < FP_ROWS; ++k) {
        const int r = tr0 + wave * FP_ROWS + k;
        if (r < g.nrow && c < g.ncol) dst.store((int64_t)r * g.ncol + c, flow_from_local(p[k], tr0, tc0, g.ncol), n[k]);
    }
}

// 3.  A grid-stride loop: lane l of a wave takes cells 64 apart in time, 64 consecutive ones with its wave at a time.
// n_cells <= INT32_MAX, so a cell number fits an int whatever the grid's size
template <bool CNT>
__global__ __launch_bounds__(FP_NT) void flow_round_kernel(const int64_t n_cells, const FlowRecs<CNT> src, const FlowRecs<CNT> dst,
                                                           unsigned long long *moved_out, unsigned long long *cycle_out) {
    unsigned long long n_moved = 0, n_cycle = 0;
    for (int64_t i = (int64_t)blockIdx.x * FP_NT + threadIdx.x; i < n_cells; i += (int64_t)gridDim.x * FP_NT) {
        int32_t p, pp = 0;
        FlowCounts n, np{0u, 0u, 0u};
        src.load(i, p, n);
        if (p != (int32_t)i) {
            src.load(p, pp, np);
            const int what = flow_double((int32_t)i, p, n, pp, np);
            n_moved += what == FLOW_MOVED;
            n_cycle += what == FLOW_CYCLE;
        }
        dst.store(i, p, n);
    }
    n_moved = wave_sum(n_moved); n_cycle = wave_sum(n_cycle);
    if ((threadIdx.x & 63) == 0 && n_moved) atomicAdd(moved_out, n_moved);
    if ((threadIdx.x & 63) == 0 && n_cycle) atomicAdd(cycle_out, n_cycle);
}

struct FlowPlanes {
    int32_t *index, *steps;
    void *dist, *value, *drop;
};

// 4.  T: the type of the stack's planes; O: the type of the float products.  z = the predicate's layer, vz = the value layer.
template <typename T, typename O, bool CNT>
__global__ __launch_bounds__(FP_NT) void flow_products_kernel(const FlowGeom g, const int8_t *__restrict__ dir, const int64_t ld_dir,
                                                              const T *__restrict__ z, const T *__restrict__ vz, const int64_t ldz,
                                                              const FlowRecs<CNT> recs, const unsigned n_tiles, const int root_ok, const double dx, const double dy,
                                                              const double diag, const FlowPlanes pl, const int64_t ld, FlowCounters *counters) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool has_nd = g.has_nodata != 0;
    O *dist = (O *)pl.dist, *value = (O *)pl.value, *drop = (O *)pl.drop;
    unsigned long long n_unreached = 0;
    int far = 0;
    for (unsigned tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int tr0 = (int)(tile / (unsigned)g.tiles_c) * FLOW_TH, tc0 = (int)(tile % (unsigned)g.tiles_c) * FLOW_TW;
        const int c = tc0 + lane;
#pragma unroll
        for (int k = 0; k < FP_ROWS; ++k) {
            const int r = tr0 + wave * FP_ROWS + k;
            if (r >= g.nrow || c >= g.ncol) continue;
            const int64_t o = (int64_t)r * ld + c;
            int32_t s = -1, steps = -1;
            double d = NAN, v = NAN, h = NAN;
            if (dir[(int64_t)r * ld_dir + c] != FLOW_DIR_NA) {
                FlowCounts n{0u, 0u, 0u};
                recs.load((int64_t)r * g.ncol + c, s, n);
                const int sr = s / g.ncol, sc = s - sr * g.ncol;
                const int64_t zs = (int64_t)sr * ldz + sc;
                const bool reached = root_ok || prox_is_feature((double)z[zs], has_nd, g.nodata, g.where, g.threshold);
                if (reached) {
                    if (CNT) {
                        steps = flow_steps(n);
                        far = max(far, steps + 1);
                        if (dist) d = flow_dist(n, dx, dy, diag);
                    }
                    if (value || drop) {
                        const double vs = (double)vz[zs];
                        v = flow_value(vs, has_nd, g.nodata);
                        if (drop) h = flow_drop((double)vz[(int64_t)r * ldz + c], vs, has_nd, g.nodata);
                    }
                } else {
                    s = -1;
                    ++n_unreached;
                }
            }
            if (pl.index) pl.index[o] = s;
            if (pl.steps) pl.steps[o] = steps;
            if (dist) dist[o] = (O)d;
            if (value) value[o] = (O)v;
            if (drop) drop[o] = (O)h;
        }
    }
    n_unreached = wave_sum(n_unreached);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) far = max(far, __shfl_xor(far, d, 64));
    if (lane == 0) {
        if (n_unreached) atomicAdd(&counters->n_unreached, n_unreached);
        if (far > 0) atomicMax(&counters->max_steps_p1, far);
    }
}

#define FP_REQUIRE(cond, ...)                                              \
    do {                                                                   \
        if (!(cond)) { set_error(__VA_ARGS__); return MHS_ERR_INVALID; }    \
    } while (0)

// Every check of a flow-path call, before any device call; fn = the entry point's name for the message
static int flow_check(const char *fn, const mhs_grid *grid, const int8_t *flowdir, int64_t ld_dir, const mhs_stack *stack, int layer, int where,
                      double threshold, int value_layer, int flags, double dx, double dy, const mhs_flowpath_out *out, int out_dtype,
                      int64_t ld, FlowGeom *g) {
    FP_REQUIRE(grid && flowdir && stack && out, "%s: NULL argument (g, flowdir, stack or out)", fn);
    FP_REQUIRE(grid->nrow > 0 && grid->ncol > 0 && grid->nrow <= (int64_t)INT32_MAX && grid->ncol <= (int64_t)INT32_MAX,
               "%s: bad grid geometry (nrow, ncol must be in 1 .. 2^31 - 1)", fn);
    FP_REQUIRE(grid->nrow * grid->ncol <= (int64_t)INT32_MAX,
               "%s: grid too large: nrow * ncol must not pass 2^31 - 1 (index and steps are int32)", fn);
    FP_REQUIRE(ld_dir >= grid->ncol, "%s: ld_dir smaller than the grid width", fn);
    FP_REQUIRE(stack->data, "%s: stack data is NULL", fn);
    FP_REQUIRE(stack->dtype == MHS_F64 || stack->dtype == MHS_F32 || stack->dtype == MHS_I16, "%s: bad stack dtype", fn);
    FP_REQUIRE(layer >= 0 && layer < stack->n_layers, "%s: layer %d is not one of the stack's %d layers", fn, layer, stack->n_layers);
    FP_REQUIRE(stack->ld >= grid->ncol && (stack->n_layers == 1 || stack->plane_stride >= stack->ld * (grid->nrow - 1) + grid->ncol),
               "%s: stack strides smaller than the grid", fn);
    FP_REQUIRE(where >= 0 && where <= FLOW_OUTLET, "%s: unknown where %d (MHS_PROX_NA .. MHS_PROX_NE, MHS_FLOWPATH_OUTLET)", fn, where);
    FP_REQUIRE(where < PROX_LT || where == FLOW_OUTLET || !std::isnan(threshold), "%s: threshold must not be NaN for a comparison", fn);
    FP_REQUIRE((flags & ~(FLOW_ROOT_IS_TARGET | FLOW_NO_LOCAL)) == 0, "%s: unknown flags %d (MHS_FLOWPATH_ROOT_IS_TARGET, MHS_FLOWPATH_NO_LOCAL)", fn, flags);
    FP_REQUIRE(out->index || out->steps || out->dist || out->value || out->drop,
               "%s: out names no product (index, steps, dist, value, drop are all NULL)", fn);
    FP_REQUIRE(!out->dist || (std::isfinite(dx) && dx > 0.0 && std::isfinite(dy) && dy > 0.0),
               "%s: dx and dy must be finite and positive for dist", fn);
    FP_REQUIRE(!(out->value || out->drop) || (value_layer >= 0 && value_layer < stack->n_layers),
               "%s: value_layer %d is not one of the stack's %d layers", fn, value_layer, stack->n_layers);
    FP_REQUIRE(out_dtype == MHS_F64 || out_dtype == MHS_F32, "%s: out_dtype must be MHS_F64 or MHS_F32", fn);
    FP_REQUIRE(ld >= grid->ncol, "%s: ld smaller than the grid width", fn);
    *g = FlowGeom{(int)grid->nrow, (int)grid->ncol, (int)((grid->ncol + FLOW_TW - 1) / FLOW_TW), stack->nodata, !std::isnan(stack->nodata), where,
                  where >= PROX_LT && where != FLOW_OUTLET ? threshold : 0.0};
    return MHS_OK;
}

// the call's one block of stream-ordered memory, given back behind whatever was enqueued last
struct FlowScratch {
    char *p = nullptr;
    hipStream_t st = nullptr;
    ~FlowScratch() { if (p) (void)hipFreeAsync(p, st); }
};

static size_t fp_align(size_t n) { return (n + 255) & ~(size_t)255; }

// what a run is made of: the planes on the device
struct FlowRun {
    const char *fn;
    FlowGeom g;
    const int8_t *dir;
    int64_t ld_dir;
    int dtype;
    const void *z, *vz;       // element (0, 0) of the predicate's layer and of the value layer
    int64_t ldz;
    int flags;
    double dx, dy;
    mhs_flowpath_out out;
    int out_dtype;
    int64_t ld;
    hipStream_t st;
};

template <typename T, typename O, bool CNT>
static void launch_flow_products(const FlowRun &q, unsigned n_tiles, unsigned n_blocks, const FlowRecs<CNT> &recs, int root_ok, double diag, FlowCounters *counters) {
    const FlowPlanes pl{q.out.index, q.out.steps, q.out.dist, q.out.value, q.out.drop};
    hipLaunchKernelGGL((flow_products_kernel<T, O, CNT>), dim3(n_blocks), dim3(FP_NT), 0, q.st, q.g, q.dir, q.ld_dir, (const T *)q.z, (const T *)q.vz,
                       q.ldz, recs, n_tiles, root_ok, q.dx, q.dy, diag, pl, q.ld, counters);
}

template <typename T, bool CNT>
static int flow_run_t(const FlowRun &q, mhs_flowpath_info *info) {
    using Rec = FlowRecs<CNT>;
    const FlowGeom &g = q.g;
    const size_t n = (size_t)g.nrow * (size_t)g.ncol, rec_bytes = CNT ? 16 : 4;
    const size_t o_b = fp_align(rec_bytes * n), o_cnt = 2 * o_b, total = o_cnt + fp_align(sizeof(FlowCounters));
    FlowScratch s;
    s.st = q.st;
    if (hipMallocAsync((void **)&s.p, total, q.st) != hipSuccess) {
        (void)hipGetLastError();
        s.p = nullptr;
        set_error("%s: no device memory for the records (%zu bytes: %zu per cell)", q.fn, total, 2 * rec_bytes);
        return MHS_ERR_ALLOC;
    }
    Rec buf[2];
    buf[0].p = (decltype(buf[0].p))s.p;
    buf[1].p = (decltype(buf[1].p))(s.p + o_b);
    FlowCounters *counters = (FlowCounters *)(s.p + o_cnt);
    MHS_HIP(hipMemsetAsync(counters, 0, sizeof(FlowCounters), q.st));
    const unsigned n_tiles = (unsigned)((((int64_t)g.nrow + FLOW_TH - 1) / FLOW_TH) * g.tiles_c);
    // seed, rounds and products go over the plane with a bounded number of workgroups, each adding to the counters once per wave
    // at its end: a wave of every tile adding to the same address costs more than the kernels' memory traffic
    const unsigned cap = (unsigned)(ctx().n_cu > 0 ? ctx().n_cu : 256) * 16u, tile_blocks = std::min(n_tiles, cap);
    hipLaunchKernelGGL((flow_seed_kernel<T, CNT>), dim3(tile_blocks), dim3(FP_NT), 0, q.st, g, n_tiles, q.dir, q.ld_dir, (const T *)q.z, q.ldz, buf[0], counters);
    MHS_HIP(hipGetLastError());
    int cur = 0;
    if (!(q.flags & FLOW_NO_LOCAL)) {
        hipLaunchKernelGGL((flow_local_kernel<CNT>), dim3(n_tiles), dim3(FP_NT), 0, q.st, g, buf[0], buf[1]);
        MHS_HIP(hipGetLastError());
        cur = 1;
    }
    const unsigned n_blocks = (unsigned)std::min<size_t>((n + FP_NT - 1) / FP_NT, cap);
    FlowCounters c;
    int rounds = 0;
    bool done = false;
    for (int launch = 0; launch < FLOW_MAX_ROUNDS && !done; ++launch) {
        hipLaunchKernelGGL((flow_round_kernel<CNT>), dim3(n_blocks), dim3(FP_NT), 0, q.st, (int64_t)n, buf[cur], buf[cur ^ 1], &counters->moved[launch],
                           &counters->n_cycle);
        MHS_HIP(hipGetLastError());
        MHS_HIP(hipMemcpyAsync(&c, counters, sizeof(c), hipMemcpyDeviceToHost, q.st));
        MHS_HIP(hipStreamSynchronize(q.st));
        if (c.n_bad) {                             // the seed's count comes down with the first round's: a malformed cell points at itself, so
                                                   // the local phase and this round were safe to run on it
            set_error("%s: flowdir is malformed: %llu cells hold a code outside -2 .. 7 or point out of the raster or at an NA cell", q.fn, c.n_bad);
            return MHS_ERR_INVALID;
        }
        if (c.n_cycle) {
            set_error("%s: flowdir has a cycle: the path of %llu cells comes back to them", q.fn, c.n_cycle);
            return MHS_ERR_INVALID;
        }
        cur ^= 1;                                  // the round's output: equal to its input when nothing moved
        if (c.moved[launch] == 0) done = true;
        else ++rounds;
    }
    if (!done) {
        set_error("%s: flowdir has a cycle: cells still move after %d doubling rounds, which resolve every path of fewer than 2^31 steps", q.fn,
                  FLOW_MAX_ROUNDS);
        return MHS_ERR_INVALID;
    }
    const int root_ok = (q.flags & FLOW_ROOT_IS_TARGET) || g.where == FLOW_OUTLET;
    const double diag = q.out.dist ? flow_diag(q.dx, q.dy) : 0.0;
    if (q.out_dtype == MHS_F64) launch_flow_products<T, double, CNT>(q, n_tiles, tile_blocks, buf[cur], root_ok, diag, counters);
    else launch_flow_products<T, float, CNT>(q, n_tiles, tile_blocks, buf[cur], root_ok, diag, counters);
    MHS_HIP(hipGetLastError());
    if (info) {
        MHS_HIP(hipMemcpyAsync(&c, counters, sizeof(c), hipMemcpyDeviceToHost, q.st));
        MHS_HIP(hipStreamSynchronize(q.st));
        *info = mhs_flowpath_info{(int64_t)c.n_valid, (int64_t)c.n_targets, (int64_t)c.n_roots, (int64_t)c.n_unreached,
                                  CNT ? (int64_t)c.max_steps_p1 - 1 : -1, rounds, (int64_t)total};
    }
    return MHS_OK;
}

static int flow_run(const FlowRun &q, mhs_flowpath_info *info) {
    const bool cnt = q.out.steps || q.out.dist;
    if (q.dtype == MHS_F64) return cnt ? flow_run_t<double, true>(q, info) : flow_run_t<double, false>(q, info);
    if (q.dtype == MHS_F32) return cnt ? flow_run_t<float, true>(q, info) : flow_run_t<float, false>(q, info);
    return cnt ? flow_run_t<short, true>(q, info) : flow_run_t<short, false>(q, info);
}

}  // namespace mhs

using namespace mhs;

extern "C" {

int mhs_flowpath_dev(const mhs_grid *g, const int8_t *flowdir, int64_t ld_dir, const mhs_stack *stack, int layer, int where, double threshold,
                     int value_layer, int flags, double dx, double dy, const mhs_flowpath_out *out, int out_dtype, int64_t ld, void *stream,
                     mhs_flowpath_info *info) {
    FlowGeom fg;
    if (int rc = flow_check(__func__, g, flowdir, ld_dir, stack, layer, where, threshold, value_layer, flags, dx, dy, out, out_dtype, ld, &fg)) return rc;
    if (int rc = require_ready()) return rc;
    const size_t esz = dtype_bytes(stack->dtype);
    const char *base = (const char *)stack->data;
    const void *plane = base + (size_t)layer * stack->plane_stride * esz;
    const void *vplane = (out->value || out->drop) ? base + (size_t)value_layer * stack->plane_stride * esz : plane;
    const FlowRun q{__func__, fg, flowdir, ld_dir, stack->dtype, plane, vplane, stack->ld, flags, dx, dy, *out, out_dtype, ld, pick_stream(stream)};
    return flow_run(q, info);
}

// Host planes: the WHOLE direction plane and the layers the call reads go up and the requested planes come down.  No row bands:
// the path of a cell may run through any row of the raster.
int mhs_flowpath(const mhs_grid *g, const int8_t *flowdir, int64_t ld_dir, const mhs_stack *stack, int layer, int where, double threshold,
                 int value_layer, int flags, double dx, double dy, const mhs_flowpath_out *out, int out_dtype, mhs_flowpath_info *info) {
    FlowGeom fg;
    const char *fn = __func__;
    if (int rc = flow_check(fn, g, flowdir, ld_dir, stack, layer, where, threshold, value_layer, flags, dx, dy, out, out_dtype, g ? g->ncol : 0, &fg))
        return rc;
    if (int rc = require_ready()) return rc;
    const size_t esz = dtype_bytes(stack->dtype), n = (size_t)fg.nrow * (size_t)fg.ncol, osz = out_dtype == MHS_F64 ? 8 : 4;
    const size_t dir_bytes = (size_t)(fg.nrow - 1) * (size_t)ld_dir + fg.ncol;
    const size_t in_bytes = ((size_t)(fg.nrow - 1) * stack->ld + fg.ncol) * esz;
    const bool second = (out->value || out->drop) && value_layer != layer;
    void *const host[5] = {out->index, out->steps, out->dist, out->value, out->drop};
    const size_t bytes[5] = {4 * n, 4 * n, n * osz, n * osz, n * osz};
    size_t off[5];
    const size_t o_z = fp_align(dir_bytes), o_v = o_z + fp_align(in_bytes);
    size_t total = o_v + (second ? fp_align(in_bytes) : 0);
    for (int k = 0; k < 5; ++k) { off[k] = total; total += host[k] ? fp_align(bytes[k]) : 0; }
    std::lock_guard<std::mutex> lk(pipe_mutex());
    if (int rc = host_pipe(0)) return rc;                      // the pipeline's streams; its arena is not used
    hipStream_t st = ctx().pipe_comp;
    FlowScratch s;
    s.st = st;
    if (hipMallocAsync((void **)&s.p, total, st) != hipSuccess) {
        (void)hipGetLastError();
        s.p = nullptr;
        set_error("%s: no device memory for the planes and the outputs (%zu bytes)", fn, total);
        return MHS_ERR_ALLOC;
    }
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{st};   // no copy is left in flight, whatever the exit
    const char *base = (const char *)stack->data;
    MHS_HIP(hipMemcpyAsync(s.p, flowdir, dir_bytes, hipMemcpyHostToDevice, st));
    MHS_HIP(hipMemcpyAsync(s.p + o_z, base + (size_t)layer * stack->plane_stride * esz, in_bytes, hipMemcpyHostToDevice, st));
    if (second) MHS_HIP(hipMemcpyAsync(s.p + o_v, base + (size_t)value_layer * stack->plane_stride * esz, in_bytes, hipMemcpyHostToDevice, st));
    void *dev[5];
    for (int k = 0; k < 5; ++k) dev[k] = host[k] ? s.p + off[k] : nullptr;
    const mhs_flowpath_out dout{(int32_t *)dev[0], (int32_t *)dev[1], dev[2], dev[3], dev[4]};
    const FlowRun q{fn, fg, (const int8_t *)s.p, ld_dir, stack->dtype, s.p + o_z, second ? s.p + o_v : s.p + o_z, stack->ld, flags, dx, dy, dout,
                    out_dtype, fg.ncol, st};
    if (int rc = flow_run(q, info)) return rc;
    for (int k = 0; k < 5; ++k)
        if (host[k]) MHS_HIP(hipMemcpyAsync(host[k], s.p + off[k], bytes[k], hipMemcpyDeviceToHost, st));
    MHS_HIP(hipStreamSynchronize(st));
    return MHS_OK;
}

}  // extern "C"
