// Rasters onto a grid in another coordinate system (include/machisplin_hip.h, section "warp", states the rule; warp_rule.h holds
// it): the C layers of a source stack on grid S onto a window of a target grid T whose cells' source points come from a
// control lattice made on the host.  The device never sees a projection: it interpolates the lattice at each cell centre and
// applies the "resample" section's rule (resample_rule.h) at that point.  All layers go through ONE launch.  mhs_warp_dev takes
// device planes and a device lattice; mhs_warp (what the R shim calls) sends a whole host stack up and runs the same kernel.
//
// warp_kernel.  A workgroup of 256 threads takes tiles of RS_TH x RS_TW = 32 x 64 target cells, lane l of wave w the 8 cells of
// tile column l in tile rows 8 w .. 8 w + 7, as rs_interp_kernel does.  Per tile:
//   1. the lattice nodes the tile's cells read go into LDS once (WARP_NODES of them at most: every K >= 4; a finer lattice is as
//      dense as the cells themselves and is read from global memory, where a wave's reads are consecutive);
//   2. every lane makes the source points (sx, sy) of its 8 cells and KEEPS them in registers: the taps are no longer separable
//      into a row part and a column part, and 8 x 2 RsTaps would be about 220 VGPRs, so the taps are remade from the 16
//      coordinates per layer;
//   3. the source rectangle the tile's taps can touch is the block-wide min / max of the cells' own i0 / j0 (cells whose point
//      has no source cell are NA whatever is staged and do not count) -- a wave reduction, then an LDS combine of the four
//      waves -- expanded by the -1 / +2 taps and cut to the raster.  STAGED: it fits the staging array (RS_STAGE_BYTES) and is
//      loaded once per layer with coalesced loads in the plane's own type; DIRECT: that tile reads global memory.
// Both accessors check their indices against what is resident before they read, so a wrong rectangle would show as a wrong
// value (the bit-for-bit tests), never as a read out of bounds.  All LDS is in the dynamic region (its base stays 16-byte
// aligned): the staging array, the nodes, the reduction words.
#include <climits>
#include <cmath>
#include <mutex>
#include "resample_int.h"
#include "warp_rule.h"

namespace mhs {

constexpr int WARP_NODES = 256;                                    // nodes of a tile held in LDS: (31 / K + 3) (63 / K + 3) <= 180 for K >= 4
constexpr int WARP_LDS_BYTES = RS_STAGE_BYTES + 2 * WARP_NODES * (int)sizeof(double) + 4 * 4 * (int)sizeof(int);

struct WarpJob {
    RsSrc S;
    int r0, c0, nr, nc;      // the target window
    int method, step;
    const double *lx, *ly;   // the lattice, on the device
    int64_t n_node_cols;
    int tiles_x;
    int64_t n_tiles;
};

// the tile's nodes in LDS: rows [a0, a0 + na) x columns [b0, b0 + nb) of the lattice
struct WarpLatticeLds {
    const double *sx, *sy;
    int a0, b0, nb;
    __device__ double x(int a, int b) const { return sx[(a - a0) * nb + (b - b0)]; }
    __device__ double y(int a, int b) const { return sy[(a - a0) * nb + (b - b0)]; }
};

__device__ inline int wave_min(int v) {
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ inline int wave_max(int v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// px[j] for a j the compiler does not know: a chain of selects keeps the array in registers where an indexed access would
// send it to scratch, and lets the loops over a lane's cells stay rolled (their bodies -- a division per axis, the cubic taps
// through two accessors -- unrolled eight times spill)
__device__ inline double pick8(const double (&p)[RS_ROWS], int j) {
    double v = p[0];
#pragma unroll
    for (int q = 1; q < RS_ROWS; ++q) {
        v = j == q ? p[q] : v;
        asm("" : "+v"(v));                                         // keeps the chain a chain: the optimiser would make it a load from scratch
    }
    return v;
}
__device__ inline void put8(double (&p)[RS_ROWS], int j, double v) {
#pragma unroll
    for (int q = 0; q < RS_ROWS; ++q) {
        p[q] = j == q ? v : p[q];
        asm("" : "+v"(p[q]));
    }
}

template <typename T, typename O>
__global__ __launch_bounds__(RS_NT) void warp_kernel(const WarpJob job, O *__restrict__ out, const int64_t ld_out, const int64_t plane_stride) {
    extern __shared__ __align__(16) unsigned char warp_sm[];
    T *sm = (T *)warp_sm;
    double *node_x = (double *)(warp_sm + RS_STAGE_BYTES), *node_y = node_x + WARP_NODES;
    int *red = (int *)(node_y + WARP_NODES);                       // [4 waves][imin, imax, jmin, jmax]
    constexpr int sm_elems = RS_STAGE_BYTES / (int)sizeof(T);
    const RsSrc &S = job.S;
    const int K = job.step;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t tile = blockIdx.x; tile < job.n_tiles; tile += gridDim.x) {
        const int tr0 = (int)(tile / job.tiles_x) * RS_TH, tc0 = (int)(tile % job.tiles_x) * RS_TW;
        const int rows = min(RS_TH, job.nr - tr0), cols = min(RS_TW, job.nc - tc0);
        // 1. the nodes of this tile
        const int a0 = (job.r0 + tr0) / K, na = (job.r0 + tr0 + rows - 1) / K + 2 - a0;
        const int b0 = (job.c0 + tc0) / K, nb = (job.c0 + tc0 + cols - 1) / K + 2 - b0;
        const bool nodes_in_lds = na * nb <= WARP_NODES;
        if (nodes_in_lds) {
            for (int e = threadIdx.x; e < na * nb; e += RS_NT) {
                const int64_t at = (int64_t)(a0 + e / nb) * job.n_node_cols + b0 + e % nb;
                node_x[e] = job.lx[at];
                node_y[e] = job.ly[at];
            }
        }
        __syncthreads();
        // 2. the source points of this lane's cells, 3. the rectangle their taps touch
        const int col = tc0 + lane;
        double px[RS_ROWS], py[RS_ROWS];
        int imin = INT_MAX, imax = INT_MIN, jmin = INT_MAX, jmax = INT_MIN;
#pragma unroll
        for (int j = 0; j < RS_ROWS; ++j) px[j] = py[j] = (double)NAN;
#pragma unroll 1
        for (int j = 0; j < RS_ROWS; ++j) {
            const int lr = wave * RS_ROWS + j;
            if (col >= job.nc || lr >= rows) continue;
            double sx, sy;
            const bool ok = nodes_in_lds ? warp_source_point(WarpLatticeLds{node_x, node_y, a0, b0, nb}, K, job.r0 + tr0 + lr, job.c0 + col, sx, sy)
                                         : warp_source_point(WarpLatticeMem{job.lx, job.ly, job.n_node_cols}, K, job.r0 + tr0 + lr, job.c0 + col, sx, sy);
            if (!ok) continue;
            put8(px, j, sx); put8(py, j, sy);
            if (rs_col_from_x(S.g, sx) < 0 || rs_row_from_y(S.g, sy) < 0) continue;
            const int i0 = rs_axis_y(S.g, sy).i0, j0 = rs_axis_x(S.g, sx).i0;
            imin = min(imin, i0); imax = max(imax, i0);
            jmin = min(jmin, j0); jmax = max(jmax, j0);
        }
        imin = wave_min(imin); imax = wave_max(imax); jmin = wave_min(jmin); jmax = wave_max(jmax);
        if (lane == 0) { red[wave * 4 + 0] = imin; red[wave * 4 + 1] = imax; red[wave * 4 + 2] = jmin; red[wave * 4 + 3] = jmax; }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            imin = min(imin, red[w * 4 + 0]); imax = max(imax, red[w * 4 + 1]);
            jmin = min(jmin, red[w * 4 + 2]); jmax = max(jmax, red[w * 4 + 3]);
        }
        int ti0 = 0, tj0 = 0, lh = 0, lw = 0;
        if (imin <= imax) {                                        // some cell of the tile has a source cell
            ti0 = max(imin - 1, S.row_lo); tj0 = max(jmin - 1, 0);
            lh = max(0, min(imax + 2, S.row_hi - 1) - ti0 + 1); lw = max(0, min(jmax + 2, S.g.ncol - 1) - tj0 + 1);
        }
        const bool staged = (int64_t)lh * lw <= sm_elems;          // the same for every thread: made from the combined words
        for (int k = 0; k < S.C; ++k) {
            const T *plane = (const T *)S.data + (int64_t)k * S.plane_stride;
            if (staged) {
                for (int lr = wave; lr < lh; lr += 4)
                    for (int lc = lane; lc < lw; lc += 64) sm[lr * lw + lc] = plane[(int64_t)(ti0 + lr) * S.ld + tj0 + lc];
                __syncthreads();
            }
            if (col < job.nc) {
                const LdsAcc<T> la{sm, ti0, tj0, lh, lw, S.has_nodata != 0, S.nodata};
                const GlobalAcc<T> ga = global_acc<T>(S, k);
                O *dst = out + (int64_t)k * plane_stride + col;
#pragma unroll 1
                for (int j = 0; j < RS_ROWS; ++j) {
                    const int lr = wave * RS_ROWS + j;
                    if (lr >= rows) break;
                    const RsTaps ty = rs_taps_y(S.g, pick8(py, j)), tx = rs_taps_x(S.g, pick8(px, j));       // a NaN point has no cell: NA
                    double v;
                    const bool ok = staged ? rs_interp_at(la, job.method, ty, tx, v) : rs_interp_at(ga, job.method, ty, tx, v);
                    dst[(int64_t)(tr0 + lr) * ld_out] = (O)(ok ? v : (double)NAN);
                }
            }
            if (staged) __syncthreads();                           // the next layer overwrites the rectangle
        }
        __syncthreads();                                           // the next tile overwrites the nodes and the reduction words
    }
}

template <typename T, typename O>
static void launch_warp_to(const WarpJob &job, void *out, int64_t ld, int64_t ps, hipStream_t st) {
    hipLaunchKernelGGL((warp_kernel<T, O>), dim3(rs_blocks(job.n_tiles)), dim3(RS_NT), (size_t)WARP_LDS_BYTES, st, job, (O *)out, ld, ps);
}

static int launch_warp(WarpJob job, int dtype, int out_dtype, void *out, int64_t ld, int64_t ps, hipStream_t st) {
    if (job.nr == 0 || job.nc == 0) return MHS_OK;
    const bool f64 = out_dtype == MHS_F64;
    job.tiles_x = (job.nc + RS_TW - 1) / RS_TW;
    job.n_tiles = (int64_t)job.tiles_x * ((job.nr + RS_TH - 1) / RS_TH);
    if (dtype == MHS_F64) f64 ? launch_warp_to<double, double>(job, out, ld, ps, st) : launch_warp_to<double, float>(job, out, ld, ps, st);
    else if (dtype == MHS_F32) f64 ? launch_warp_to<float, double>(job, out, ld, ps, st) : launch_warp_to<float, float>(job, out, ld, ps, st);
    else f64 ? launch_warp_to<short, double>(job, out, ld, ps, st) : launch_warp_to<short, float>(job, out, ld, ps, st);
    MHS_HIP(hipGetLastError());
    return MHS_OK;
}

static int warp_check(const char *fn, const mhs_grid *sg, const mhs_stack *ss, const mhs_grid *tg, int64_t r0, int64_t r1, int64_t c0, int64_t c1,
                      const mhs_warp_lattice *lat, int method, const void *out, int64_t ld, int64_t plane_stride, int out_dtype, WarpJob *job) {
    RsGrid T;
    if (int rc = rs_check_src(fn, sg, ss, &job->S)) return rc;
    if (int rc = rs_check_grid(fn, "target", tg, &T)) return rc;
    RS_REQUIRE(lat, "%s: NULL argument (lattice)", fn);
    RS_REQUIRE(warp_step_ok(lat->step), "%s: the lattice's step %d is not a power of two in 1 .. %d", fn, (int)lat->step, WARP_MAX_STEP);
    RS_REQUIRE(lat->n_node_rows == warp_nodes(tg->nrow, lat->step) && lat->n_node_cols == warp_nodes(tg->ncol, lat->step),
               "%s: the lattice's node counts %lld x %lld differ from ceil(nrow / step) + 1 = %lld and ceil(ncol / step) + 1 = %lld of the target grid", fn,
               (long long)lat->n_node_rows, (long long)lat->n_node_cols, (long long)warp_nodes(tg->nrow, lat->step), (long long)warp_nodes(tg->ncol, lat->step));
    RS_REQUIRE(lat->sx && lat->sy, "%s: NULL argument (the lattice's sx or sy)", fn);
    RS_REQUIRE(0 <= r0 && r0 <= r1 && r1 <= tg->nrow && 0 <= c0 && c0 <= c1 && c1 <= tg->ncol, "%s: window outside the target grid", fn);
    RS_REQUIRE(method >= 0 && method < RS_METHODS, "%s: unknown method %d", fn, method);
    RS_REQUIRE(method <= RS_CUBIC, "%s: method %d is an aggregate method; a warp takes NEAR, BILINEAR or CUBIC (aggregate in the source system first)", fn, method);
    RS_REQUIRE(out_dtype == MHS_F64 || out_dtype == MHS_F32, "%s: out_dtype must be MHS_F64 or MHS_F32", fn);
    RS_REQUIRE(out, "%s: NULL argument (out)", fn);
    RS_REQUIRE(ld >= c1 - c0, "%s: out_ld smaller than the window width", fn);
    if (ss->n_layers > 1) RS_REQUIRE(plane_stride >= ld * (r1 - r0 - 1) + (c1 - c0), "%s: out_plane_stride smaller than an output plane", fn);
    job->r0 = (int)r0; job->c0 = (int)c0; job->nr = (int)(r1 - r0); job->nc = (int)(c1 - c0);
    job->method = method; job->step = lat->step;
    job->lx = lat->sx; job->ly = lat->sy; job->n_node_cols = lat->n_node_cols;
    job->tiles_x = 0; job->n_tiles = 0;
    return MHS_OK;
}

// Host planes, a host lattice, a host output: the whole stack (the rows a target row band reads are not a band) and the lattice go
// up in one piece on the library's host-pointer pipeline, the same kernel runs, the window comes down.
static int warp_host(WarpJob job, const mhs_stack *ss, const mhs_warp_lattice *lat, void *out_host, int out_dtype) {
    if (int rc = require_ready()) return rc;
    if (job.nr == 0 || job.nc == 0) return MHS_OK;
    const size_t esz = dtype_bytes(ss->dtype), oesz = out_dtype == MHS_F64 ? 8 : 4;
    const int C = job.S.C;
    const size_t in_plane = (size_t)job.S.g.nrow * ss->ld;                        // elements of one layer as it goes up
    const size_t in_bytes = (in_plane * esz * C + 255) & ~(size_t)255;
    const size_t n_nodes = (size_t)lat->n_node_rows * (size_t)lat->n_node_cols;
    const size_t lat_bytes = (sizeof(double) * n_nodes + 255) & ~(size_t)255;
    const size_t plane_out = (size_t)job.nr * job.nc;
    const size_t out_bytes = plane_out * oesz * C;
    std::lock_guard<std::mutex> lk(pipe_mutex());
    if (int rc = host_pipe(in_bytes + 2 * lat_bytes + out_bytes)) return rc;
    Context &c = ctx();
    hipStream_t st = c.pipe_comp;
    char *in = c.pipe_arena, *dlx = in + in_bytes, *dly = dlx + lat_bytes, *dout = dly + lat_bytes;
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{st};
    for (int k = 0; k < C; ++k)
        MHS_HIP(hipMemcpyAsync(in + (size_t)k * in_plane * esz, (const char *)ss->data + (size_t)k * ss->plane_stride * esz,
                               ((size_t)(job.S.g.nrow - 1) * ss->ld + job.S.g.ncol) * esz, hipMemcpyHostToDevice, st));
    MHS_HIP(hipMemcpyAsync(dlx, lat->sx, sizeof(double) * n_nodes, hipMemcpyHostToDevice, st));
    MHS_HIP(hipMemcpyAsync(dly, lat->sy, sizeof(double) * n_nodes, hipMemcpyHostToDevice, st));
    job.S.data = in;
    job.S.plane_stride = (int64_t)in_plane;
    job.lx = (const double *)dlx; job.ly = (const double *)dly;
    if (int rc = launch_warp(job, ss->dtype, out_dtype, dout, job.nc, (int64_t)plane_out, st)) return rc;
    MHS_HIP(hipMemcpyAsync(out_host, dout, out_bytes, hipMemcpyDeviceToHost, st));
    MHS_HIP(hipStreamSynchronize(st));
    return MHS_OK;
}

}  // namespace mhs

using namespace mhs;

extern "C" {

int mhs_warp_dev(const mhs_grid *src_grid, const mhs_stack *src_stack, const mhs_grid *dst_grid, int64_t r0, int64_t r1, int64_t c0, int64_t c1,
                 const mhs_warp_lattice *lat_dev, int method, void *out_dev, int64_t out_ld, int64_t out_plane_stride, int out_dtype, void *stream) {
    WarpJob job;
    if (int rc = warp_check(__func__, src_grid, src_stack, dst_grid, r0, r1, c0, c1, lat_dev, method, out_dev, out_ld, out_plane_stride, out_dtype, &job)) return rc;
    if (int rc = require_ready()) return rc;
    return launch_warp(job, src_stack->dtype, out_dtype, out_dev, out_ld, out_plane_stride, pick_stream(stream));
}

int mhs_warp(const mhs_grid *src_grid, const mhs_stack *src_stack, const mhs_grid *dst_grid, int64_t r0, int64_t r1, int64_t c0, int64_t c1,
             const mhs_warp_lattice *lat, int method, void *out_host, int out_dtype) {
    WarpJob job;
    if (int rc = warp_check(__func__, src_grid, src_stack, dst_grid, r0, r1, c0, c1, lat, method, out_host, c1 - c0, (r1 - r0) * (c1 - c0), out_dtype, &job)) return rc;
    return warp_host(job, src_stack, lat, out_host, out_dtype);
}

}  // extern "C"
