// Rasters onto one grid (include/machisplin_hip.h, section "resample", states the rules; resample_rule.h holds them): the C layers of
// a source stack on grid S onto a window of an axis-aligned target grid T in the same coordinate system -- nearest cell, bilinear,
// cubic; the aggregates mean, min, max, sum, count -- and the interpolating methods at points.  All layers of a stack go through
// ONE launch: the indices and weights of a target column and of a target row are made once and applied to every layer.
//
// rs_interp_kernel (NEAR / BILINEAR / CUBIC).  A workgroup of 256 threads takes tiles of RS_TH x RS_TW = 32 x 64 target cells,
// lane l of wave w the 8 cells of tile column l in tile rows 8 w .. 8 w + 7, as terrain3_kernel does.  The taps of the 32 tile
// rows are made by 32 threads into LDS, those of a column by its lane into registers.  Two regimes, chosen on the host from the
// two grids:
//   STAGED   the source cells the tile's taps can touch -- rows i0(first row) - 1 .. i0(last row) + 2, columns likewise, cut to
//            the raster -- are a rectangle of about (32 ry + 4) x (64 rx + 4) cells (rx, ry = target over source cell size).  When
//            that fits RS_STAGE_BYTES of LDS (the launch takes only what the two grids ask for: 10 KiB of float32 at a ratio of 1,
//            so eight workgroups share a CU) it is loaded once per layer with coalesced loads in the plane's own type, and the
//            taps are read from LDS: the upsampling and the near-1:1 shifted regime, where a source value is read by many cells.
//   DIRECT   a coarser target's taps are sparse in the source: they are read straight from global memory.
// A STAGED launch still measures every tile's rectangle and takes the direct path for a tile whose rectangle is larger than the
// LDS array, so the host's estimate decides speed, never safety.
//
// rs_aggregate_kernel (MEAN / MIN / MAX / SUM / COUNT).  A workgroup takes ONE target row and `twa` <= 64 consecutive target
// columns; their footprints partition a band of source rows [i_lo, i_hi) x columns [J0, J1).  The band goes through LDS in chunks
// of cr rows x cw <= AG_CW columns (AG_CHUNK elements), every element loaded once, coalesced.  Thread (il, t) adds the cells of
// footprint row il of the chunk that belong to target column t west to east, carrying its row's partial over the column chunks,
// so a footprint wider than a wave or than a chunk is only more iterations; then thread t folds the chunk's rows north to south
// into its cell.  That is the rule's order: a sum of row sums.  twa shrinks with the footprint's width and, if the grid would
// be short of workgroups, is halved while it is above 8.
//
// rs_points_kernel: a lane per point, the same rule functions, taps straight from global memory.
//
// Every accessor checks its indices against what is resident (the raster, a host band's rows, the staged rectangle) before it
// reads, so an error in a footprint would show as a wrong value, not as a read out of bounds.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <mutex>
#include <vector>
#include "resample_int.h"

namespace mhs {

static_assert(RS_NEAR == MHS_RS_NEAR && RS_BILINEAR == MHS_RS_BILINEAR && RS_CUBIC == MHS_RS_CUBIC && RS_MEAN == MHS_RS_MEAN && RS_MIN == MHS_RS_MIN &&
              RS_MAX == MHS_RS_MAX && RS_SUM == MHS_RS_SUM && RS_COUNT_CELLS == MHS_RS_COUNT, "resample_rule.h numbers the methods as the header does");

constexpr int AG_CHUNK = 6144;                  // elements of a staged chunk of the aggregate kernel (48 KiB of float64)
constexpr int AG_CW = 2048;                     // columns of a chunk at most
constexpr int AG_MAX_TW = 64;                   // target columns of a workgroup at most

struct RsJob {
    RsSrc S;
    RsGrid T;
    int r0, c0, nr, nc;      // the target window
    int method;
    int tiles_x;
    int64_t n_tiles;
};

template <typename T, typename O, bool STAGED>
__global__ __launch_bounds__(RS_NT) void rs_interp_kernel(const RsJob job, const int sm_elems, O *__restrict__ out, const int64_t ld_out,
                                                          const int64_t plane_stride) {
    extern __shared__ __align__(16) unsigned char rs_sm[];         // sm_elems elements of T: the host's bound on a tile's rectangle
    T *sm = (T *)rs_sm;
    __shared__ RsTaps row_taps[RS_TH];
    const RsSrc &S = job.S;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t tile = blockIdx.x; tile < job.n_tiles; tile += gridDim.x) {
        const int tr0 = (int)(tile / job.tiles_x) * RS_TH, tc0 = (int)(tile % job.tiles_x) * RS_TW;
        const int rows = min(RS_TH, job.nr - tr0), cols = min(RS_TW, job.nc - tc0);
        if ((int)threadIdx.x < rows) row_taps[threadIdx.x] = rs_taps_y(S.g, rs_cell_y(job.T, job.r0 + tr0 + (int)threadIdx.x));
        const int col = tc0 + lane;
        const RsTaps tx = rs_taps_x(S.g, rs_cell_x(job.T, job.c0 + min(col, job.nc - 1)));
        // the rectangle of source cells this tile's taps can touch (the coordinates grow with the row and with the column)
        int ti0 = 0, tj0 = 0, lh = 0, lw = 0;
        bool staged = false;
        if (STAGED) {
            const int ia = rs_axis_y(S.g, rs_cell_y(job.T, job.r0 + tr0)).i0 - 1, ib = rs_axis_y(S.g, rs_cell_y(job.T, job.r0 + tr0 + rows - 1)).i0 + 2;
            const int ja = rs_axis_x(S.g, rs_cell_x(job.T, job.c0 + tc0)).i0 - 1, jb = rs_axis_x(S.g, rs_cell_x(job.T, job.c0 + tc0 + cols - 1)).i0 + 2;
            ti0 = max(ia, S.row_lo); tj0 = max(ja, 0);
            lh = max(0, min(ib, S.row_hi - 1) - ti0 + 1); lw = max(0, min(jb, S.g.ncol - 1) - tj0 + 1);
            staged = (int64_t)lh * lw <= sm_elems;
        }
        __syncthreads();                                           // row_taps
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
                for (int j = 0; j < RS_ROWS; ++j) {
                    const int lr = wave * RS_ROWS + j;
                    if (lr >= rows) break;
                    double v;
                    const bool ok = staged ? rs_interp_at(la, job.method, row_taps[lr], tx, v) : rs_interp_at(ga, job.method, row_taps[lr], tx, v);
                    dst[(int64_t)(tr0 + lr) * ld_out] = (O)(ok ? v : (double)NAN);
                }
            }
            if (staged) __syncthreads();                           // the next layer overwrites the rectangle
        }
        __syncthreads();                                           // the next tile overwrites row_taps
    }
}

template <typename T, typename O>
__global__ __launch_bounds__(RS_NT) void rs_aggregate_kernel(const RsJob job, const int twa, O *__restrict__ out, const int64_t ld_out,
                                                             const int64_t plane_stride) {
    __shared__ T sm[AG_CHUNK];
    __shared__ RsPart part[RS_NT];
    __shared__ int jl[AG_MAX_TW], jh[AG_MAX_TW];
    const RsSrc &S = job.S;
    const int tid = threadIdx.x;
    const int cr_max = RS_NT / twa;
    const int t = tid % twa, il = tid / twa;
    const bool has_nd = S.has_nodata != 0;
    for (int64_t tile = blockIdx.x; tile < job.n_tiles; tile += gridDim.x) {
        const int row = (int)(tile / job.tiles_x), tc0 = (int)(tile % job.tiles_x) * twa;
        const int ntc = min(twa, job.nc - tc0);
        __syncthreads();                                           // the tile before has read jl, jh
        if (tid < ntc) {
            jl[tid] = rs_foot_col(S.g, job.T, job.c0 + tc0 + tid);
            jh[tid] = rs_foot_col(S.g, job.T, job.c0 + tc0 + tid + 1);
        }
        const int i_lo = max(rs_foot_row(S.g, job.T, job.r0 + row), S.row_lo), i_hi = min(rs_foot_row(S.g, job.T, job.r0 + row + 1), S.row_hi);
        __syncthreads();
        const int J0 = jl[0], J1 = jh[ntc - 1];
        const int cw = min(J1 - J0, AG_CW);
        const int cr = cw > 0 ? min(cr_max, AG_CHUNK / cw) : cr_max;         // at least AG_CHUNK / AG_CW = 3
        const bool worker = il < cr && t < ntc;
        const int my_lo = worker ? jl[t] : 0, my_hi = worker ? jh[t] : 0;
        for (int k = 0; k < S.C; ++k) {
            const T *plane = (const T *)S.data + (int64_t)k * S.plane_stride;
            RsPart cell = rs_part_empty();                         // of target column tid < ntc
            for (int ia = i_lo; ia < i_hi; ia += cr) {
                const int nrows = min(cr, i_hi - ia);
                RsPart rowp = rs_part_empty();                     // of footprint row ia + il, target column t
                for (int ja = J0; ja < J1; ja += cw) {
                    const int cwid = min(cw, J1 - ja);
                    __syncthreads();                               // the chunk before has been read
                    for (int e = tid; e < nrows * cwid; e += RS_NT) {
                        const int rr = e / cwid, cc = e - rr * cwid;
                        sm[e] = plane[(int64_t)(ia + rr) * S.ld + ja + cc];
                    }
                    __syncthreads();
                    if (worker && il < nrows) {
                        const int a = max(my_lo, ja), b = min(my_hi, ja + cwid);
                        for (int j = a; j < b; ++j) {
                            const double z = (double)sm[il * cwid + j - ja];
                            if (!rs_na(z, has_nd, S.nodata)) rs_part_add(rowp, z);
                        }
                    }
                }
                part[tid] = rowp;
                __syncthreads();
                if (tid < ntc)
                    for (int q = 0; q < nrows; ++q) rs_part_fold(cell, part[q * twa + tid]);
                __syncthreads();                                   // part is written again
            }
            if (tid < ntc) {
                double v;
                const bool ok = rs_part_value(cell, job.method, v);
                out[(int64_t)k * plane_stride + (int64_t)row * ld_out + tc0 + tid] = (O)(ok ? v : (double)NAN);
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(RS_NT) void rs_points_kernel(const RsSrc S, const double *__restrict__ xy, const int64_t n, const int method,
                                                          double *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * RS_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * RS_NT) {
        const RsTaps tx = rs_taps_x(S.g, xy[i]), ty = rs_taps_y(S.g, xy[n + i]);
        for (int k = 0; k < S.C; ++k) {
            double v;
            const bool ok = rs_interp_at(global_acc<T>(S, k), method, ty, tx, v);
            out[(int64_t)k * n + i] = ok ? v : (double)NAN;
        }
    }
}

// elements of the LDS array of a STAGED launch: the host's bound on a tile's rectangle (a tile's first and last row are at
// most 31 ry source rows apart, their taps reach 1 before and 2 behind, and a row of slack); 0 = it does not fit, DIRECT
static int rs_stage_elems(const RsJob &job, size_t esz) {
    const double ry = job.T.yres / job.S.g.yres, rx = job.T.xres / job.S.g.xres;
    const double lh = std::ceil((RS_TH - 1) * ry) + 5.0, lw = std::ceil((RS_TW - 1) * rx) + 5.0;
    return lh * lw * (double)esz <= (double)RS_STAGE_BYTES ? (int)(lh * lw) : 0;
}

template <typename T, typename O>
static void launch_interp_to(const RsJob &job, void *out, int64_t ld, int64_t ps, hipStream_t st) {
    const int elems = rs_stage_elems(job, sizeof(T));
    if (elems > 0)
        hipLaunchKernelGGL((rs_interp_kernel<T, O, true>), dim3(rs_blocks(job.n_tiles)), dim3(RS_NT), (size_t)elems * sizeof(T), st, job, elems, (O *)out, ld, ps);
    else
        hipLaunchKernelGGL((rs_interp_kernel<T, O, false>), dim3(rs_blocks(job.n_tiles)), dim3(RS_NT), 0, st, job, 0, (O *)out, ld, ps);
}
template <typename T, typename O>
static void launch_aggregate_to(const RsJob &job, int twa, void *out, int64_t ld, int64_t ps, hipStream_t st) {
    hipLaunchKernelGGL((rs_aggregate_kernel<T, O>), dim3(rs_blocks(job.n_tiles)), dim3(RS_NT), 0, st, job, twa, (O *)out, ld, ps);
}

// target columns of an aggregate workgroup: a band of about AG_CW source columns, fewer while the grid is short of workgroups
static int aggregate_tw(const RsJob &job) {
    const double fw = std::ceil(job.T.xres / job.S.g.xres) + 1.0;
    int twa = (int)std::max(1.0, std::min((double)AG_MAX_TW, std::floor((double)AG_CW / fw)));
    const int64_t want = 4 * (int64_t)(ctx().n_cu > 0 ? ctx().n_cu : 256);
    while (twa > 8 && (int64_t)job.nr * ((job.nc + twa - 1) / twa) < want) twa /= 2;
    return twa;
}

// the window (job.r0, c0, nr, nc filled in) of the stack `dtype` into out
static int launch_resample(RsJob job, int dtype, int out_dtype, void *out, int64_t ld, int64_t ps, hipStream_t st) {
    if (job.nr == 0 || job.nc == 0) return MHS_OK;
    const bool f64 = out_dtype == MHS_F64;
    if (job.method <= RS_CUBIC) {
        job.tiles_x = (job.nc + RS_TW - 1) / RS_TW;
        job.n_tiles = (int64_t)job.tiles_x * ((job.nr + RS_TH - 1) / RS_TH);
        if (dtype == MHS_F64) f64 ? launch_interp_to<double, double>(job, out, ld, ps, st) : launch_interp_to<double, float>(job, out, ld, ps, st);
        else if (dtype == MHS_F32) f64 ? launch_interp_to<float, double>(job, out, ld, ps, st) : launch_interp_to<float, float>(job, out, ld, ps, st);
        else f64 ? launch_interp_to<short, double>(job, out, ld, ps, st) : launch_interp_to<short, float>(job, out, ld, ps, st);
    } else {
        const int twa = aggregate_tw(job);
        job.tiles_x = (job.nc + twa - 1) / twa;
        job.n_tiles = (int64_t)job.tiles_x * job.nr;
        if (dtype == MHS_F64) f64 ? launch_aggregate_to<double, double>(job, twa, out, ld, ps, st) : launch_aggregate_to<double, float>(job, twa, out, ld, ps, st);
        else if (dtype == MHS_F32) f64 ? launch_aggregate_to<float, double>(job, twa, out, ld, ps, st) : launch_aggregate_to<float, float>(job, twa, out, ld, ps, st);
        else f64 ? launch_aggregate_to<short, double>(job, twa, out, ld, ps, st) : launch_aggregate_to<short, float>(job, twa, out, ld, ps, st);
    }
    MHS_HIP(hipGetLastError());
    return MHS_OK;
}

static int launch_points(const RsSrc &S, int dtype, const double *xy, int64_t n, int method, double *out, hipStream_t st) {
    if (n == 0) return MHS_OK;
    const dim3 grid(rs_blocks((n + RS_NT - 1) / RS_NT));
    if (dtype == MHS_F64) hipLaunchKernelGGL(rs_points_kernel<double>, grid, dim3(RS_NT), 0, st, S, xy, n, method, out);
    else if (dtype == MHS_F32) hipLaunchKernelGGL(rs_points_kernel<float>, grid, dim3(RS_NT), 0, st, S, xy, n, method, out);
    else hipLaunchKernelGGL(rs_points_kernel<short>, grid, dim3(RS_NT), 0, st, S, xy, n, method, out);
    MHS_HIP(hipGetLastError());
    return MHS_OK;
}

static int rs_check_resample(const char *fn, const mhs_grid *sg, const mhs_stack *ss, const mhs_grid *tg, int64_t r0, int64_t r1, int64_t c0, int64_t c1,
                             int method, const void *out, int64_t ld, int64_t plane_stride, int out_dtype, RsJob *job) {
    if (int rc = rs_check_src(fn, sg, ss, &job->S)) return rc;
    if (int rc = rs_check_grid(fn, "target", tg, &job->T)) return rc;
    RS_REQUIRE(0 <= r0 && r0 <= r1 && r1 <= tg->nrow && 0 <= c0 && c0 <= c1 && c1 <= tg->ncol, "%s: window outside the target grid", fn);
    RS_REQUIRE(method >= 0 && method < RS_METHODS, "%s: unknown method %d", fn, method);
    RS_REQUIRE(out_dtype == MHS_F64 || out_dtype == MHS_F32, "%s: out_dtype must be MHS_F64 or MHS_F32", fn);
    RS_REQUIRE(out, "%s: NULL argument (out)", fn);
    RS_REQUIRE(ld >= c1 - c0, "%s: out_ld smaller than the window width", fn);
    if (ss->n_layers > 1) RS_REQUIRE(plane_stride >= ld * (r1 - r0 - 1) + (c1 - c0), "%s: out_plane_stride smaller than an output plane", fn);
    job->r0 = (int)r0; job->c0 = (int)c0; job->nr = (int)(r1 - r0); job->nc = (int)(c1 - c0);
    job->method = method; job->tiles_x = 0; job->n_tiles = 0;
    return MHS_OK;
}

static int rs_check_points(const char *fn, const mhs_grid *sg, const mhs_stack *ss, const double *xy, int64_t n, int method, const double *out, RsSrc *S) {
    if (int rc = rs_check_src(fn, sg, ss, S)) return rc;
    RS_REQUIRE(n >= 0, "%s: n is negative", fn);
    RS_REQUIRE(method >= 0 && method < RS_METHODS, "%s: unknown method %d", fn, method);
    RS_REQUIRE(method <= RS_CUBIC, "%s: method %d is an aggregate method; points take NEAR, BILINEAR or CUBIC", fn, method);
    RS_REQUIRE((xy && out) || n == 0, "%s: NULL argument (xy or out)", fn);
    return MHS_OK;
}

// the source rows [lo, hi) that the target rows [b0, b1) read (empty: lo = hi)
static void rs_rows_needed(const RsJob &job, int64_t b0, int64_t b1, int *lo, int *hi) {
    const RsGrid &S = job.S.g;
    int a, b;
    if (job.method <= RS_CUBIC) {
        a = rs_axis_y(S, rs_cell_y(job.T, (int)b0)).i0 - 1;
        b = rs_axis_y(S, rs_cell_y(job.T, (int)b1 - 1)).i0 + 3;
    } else {
        a = rs_foot_row(S, job.T, (int)b0);
        b = rs_foot_row(S, job.T, (int)b1);
    }
    a = std::max(a, 0); b = std::min(b, S.nrow);
    *lo = a; *hi = std::max(a, b);
}

// Host planes in, host planes out: row bands of the target window, each with exactly the source rows it reads (of every
// layer), go up, through the same kernels and down again on one stream of the library's host-pointer pipeline, as
// mhs_terrain's do.  A band's buffer is described as the planes moved back to absolute row 0.  MHS_HOST_BANDS = n forces n
// equal bands.
static int resample_host(RsJob job, const mhs_stack *ss, void *out_host, int out_dtype) {
    if (int rc = require_ready()) return rc;
    const int64_t nr = job.nr, nc = job.nc, r0 = job.r0, r1 = r0 + nr;
    if (nr == 0 || nc == 0) return MHS_OK;
    const size_t esz = dtype_bytes(ss->dtype), oesz = out_dtype == MHS_F64 ? 8 : 4;
    const int C = job.S.C;
    const double src_rows_per_row = job.T.yres / job.S.g.yres;
    const double row_bytes = (double)C * ((double)nc * oesz + (src_rows_per_row + 1.0) * (double)ss->ld * esz);
    int64_t rows_per = std::max<int64_t>(1, std::min<int64_t>(nr, (int64_t)((double)((size_t)256 << 20) / row_bytes)));
    if (const char *e = getenv("MHS_HOST_BANDS")) {
        const int64_t nb = std::max<int64_t>(1, std::min<int64_t>(nr, atoll(e)));
        rows_per = (nr + nb - 1) / nb;
    }
    int64_t most_src = 0;
    for (int64_t b0 = r0; b0 < r1; b0 += rows_per) {
        int lo, hi;
        rs_rows_needed(job, b0, std::min(r1, b0 + rows_per), &lo, &hi);
        most_src = std::max<int64_t>(most_src, hi - lo);
    }
    const size_t in_plane = (size_t)std::max<int64_t>(most_src, 1) * ss->ld;       // elements of one layer of a band
    const size_t in_bytes = (in_plane * esz * C + 255) & ~(size_t)255;
    const size_t plane_out = (size_t)rows_per * nc;
    const size_t out_bytes = (plane_out * oesz * C + 255) & ~(size_t)255;
    std::lock_guard<std::mutex> lk(pipe_mutex());
    if (int rc = host_pipe(in_bytes + out_bytes)) return rc;
    Context &c = ctx();
    hipStream_t st = c.pipe_comp;
    char *in = c.pipe_arena, *outb = in + in_bytes;
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{st};
    for (int64_t b0 = r0; b0 < r1; b0 += rows_per) {
        const int64_t b1 = std::min(r1, b0 + rows_per);
        int lo, hi;
        rs_rows_needed(job, b0, b1, &lo, &hi);
        if (hi > lo)
            for (int k = 0; k < C; ++k)
                MHS_HIP(hipMemcpyAsync(in + (size_t)k * in_plane * esz, (const char *)ss->data + ((size_t)k * ss->plane_stride + (size_t)lo * ss->ld) * esz,
                                       ((size_t)(hi - lo - 1) * ss->ld + job.S.g.ncol) * esz, hipMemcpyHostToDevice, st));
        RsJob bj = job;
        bj.S.data = in - (size_t)lo * ss->ld * esz;
        bj.S.plane_stride = (int64_t)in_plane;
        bj.S.row_lo = lo; bj.S.row_hi = hi;
        bj.r0 = (int)b0; bj.nr = (int)(b1 - b0);
        if (int rc = launch_resample(bj, ss->dtype, out_dtype, outb, nc, (int64_t)plane_out, st)) return rc;
        for (int k = 0; k < C; ++k)
            MHS_HIP(hipMemcpyAsync((char *)out_host + ((size_t)k * nr * nc + (size_t)(b0 - r0) * nc) * oesz, outb + (size_t)k * plane_out * oesz,
                                   (size_t)(b1 - b0) * nc * oesz, hipMemcpyDeviceToHost, st));
        MHS_HIP(hipStreamSynchronize(st));       // the next band reuses the buffers
    }
    return MHS_OK;
}

// Host planes and host points: the source rows between the northernmost and the southernmost tap of a point that has a cell go
// up in one piece with the points, the values come down.
static int points_host(RsSrc S, const mhs_stack *ss, const double *xy, int64_t n, int method, double *out) {
    if (int rc = require_ready()) return rc;
    if (n == 0) return MHS_OK;
    int lo = S.g.nrow, hi = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (rs_col_from_x(S.g, xy[i]) < 0 || rs_row_from_y(S.g, xy[n + i]) < 0) continue;
        const int i0 = rs_axis_y(S.g, xy[n + i]).i0;
        lo = std::min(lo, std::max(i0 - 1, 0));
        hi = std::max(hi, std::min(i0 + 3, S.g.nrow));
    }
    if (hi <= lo) {                              // no point has a cell
        for (int64_t i = 0; i < n * S.C; ++i) out[i] = NAN;
        return MHS_OK;
    }
    const size_t esz = dtype_bytes(ss->dtype);
    const size_t in_plane = (size_t)(hi - lo) * ss->ld;
    const size_t in_bytes = (in_plane * esz * S.C + 255) & ~(size_t)255;
    const size_t xy_bytes = (sizeof(double) * 2 * (size_t)n + 255) & ~(size_t)255;
    const size_t out_bytes = sizeof(double) * (size_t)n * S.C;
    std::lock_guard<std::mutex> lk(pipe_mutex());
    if (int rc = host_pipe(in_bytes + xy_bytes + out_bytes)) return rc;
    Context &c = ctx();
    hipStream_t st = c.pipe_comp;
    char *in = c.pipe_arena, *dxy = in + in_bytes, *dout = dxy + xy_bytes;
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{st};
    for (int k = 0; k < S.C; ++k)
        MHS_HIP(hipMemcpyAsync(in + (size_t)k * in_plane * esz, (const char *)ss->data + ((size_t)k * ss->plane_stride + (size_t)lo * ss->ld) * esz,
                               ((size_t)(hi - lo - 1) * ss->ld + S.g.ncol) * esz, hipMemcpyHostToDevice, st));
    MHS_HIP(hipMemcpyAsync(dxy, xy, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, st));
    S.data = in - (size_t)lo * ss->ld * esz;
    S.plane_stride = (int64_t)in_plane;
    S.row_lo = lo; S.row_hi = hi;
    if (int rc = launch_points(S, ss->dtype, (const double *)dxy, n, method, (double *)dout, st)) return rc;
    MHS_HIP(hipMemcpyAsync(out, dout, out_bytes, hipMemcpyDeviceToHost, st));
    MHS_HIP(hipStreamSynchronize(st));
    return MHS_OK;
}

}  // namespace mhs

using namespace mhs;

extern "C" {

int mhs_resample_dev(const mhs_grid *src_grid, const mhs_stack *src_stack, const mhs_grid *dst_grid, int64_t r0, int64_t r1, int64_t c0, int64_t c1,
                     int method, void *out_dev, int64_t out_ld, int64_t out_plane_stride, int out_dtype, void *stream) {
    RsJob job;
    if (int rc = rs_check_resample(__func__, src_grid, src_stack, dst_grid, r0, r1, c0, c1, method, out_dev, out_ld, out_plane_stride, out_dtype, &job)) return rc;
    if (int rc = require_ready()) return rc;
    return launch_resample(job, src_stack->dtype, out_dtype, out_dev, out_ld, out_plane_stride, pick_stream(stream));
}

int mhs_resample(const mhs_grid *src_grid, const mhs_stack *src_stack, const mhs_grid *dst_grid, int64_t r0, int64_t r1, int64_t c0, int64_t c1,
                 int method, void *out_host, int out_dtype) {
    RsJob job;
    if (int rc = rs_check_resample(__func__, src_grid, src_stack, dst_grid, r0, r1, c0, c1, method, out_host, c1 - c0, (r1 - r0) * (c1 - c0), out_dtype, &job)) return rc;
    return resample_host(job, src_stack, out_host, out_dtype);
}

int mhs_extract_points_dev(const mhs_grid *src_grid, const mhs_stack *src_stack, const double *xy_dev, int64_t n, int method, double *out_dev,
                           void *stream) {
    RsSrc S;
    if (int rc = rs_check_points(__func__, src_grid, src_stack, xy_dev, n, method, out_dev, &S)) return rc;
    if (int rc = require_ready()) return rc;
    return launch_points(S, src_stack->dtype, xy_dev, n, method, out_dev, pick_stream(stream));
}

int mhs_extract_points(const mhs_grid *src_grid, const mhs_stack *src_stack, const double *xy, int64_t n, int method, double *out) {
    RsSrc S;
    if (int rc = rs_check_points(__func__, src_grid, src_stack, xy, n, method, out, &S)) return rc;
    return points_host(S, src_stack, xy, n, method, out);
}

}  // extern "C"
