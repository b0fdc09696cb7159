// Topographic covariates from one elevation plane (include/machisplin_hip.h, section "terrain", states the rules;
// terrain_rule.h holds them): the 3 x 3 terrain variables, relief in a circular window, geomorphons -- and the solar products of
// section "solar" (solar_rule.h): the horizon along sixteen rays, sky view, direct insolation, sun hours.
//
// All four kernels work the same way.  A workgroup of 256 threads takes output tiles of TER_TH x TER_TW = 32 x 64 cells of
// the window and stages each tile with a halo of H cells on every side (H = 1, the relief radius, the geomorphon search
// length) in LDS IN THE PLANE'S OWN TYPE: (32 + 2 H) x (64 + 2 H) elements, wave w taking LDS rows w, w + 4, ... and its 64
// lanes 64 consecutive elements of the row at a time, so every global load of a wave is 64 consecutive elements whatever
// the window's origin.  Only cells of the raster within H of the window are loaded (a host band holds no others); what is
// outside the raster is never looked at, the rules get the distance to the raster's border instead.  Then lane l of wave w
// makes the 8 cells of tile column l in tile rows 8 w .. 8 w + 7 from LDS, converting to double as it reads, and writes each
// output element once: the 64 lanes of a wave write 64 consecutive elements.  No atomics; a cell's value depends on the
// plane alone, so a window gives the whole-grid call's bits.
//
// The 3 x 3 kernel slides its nine values down the column (three LDS reads per cell) and makes every requested plane in that
// one pass: sizeof(T) + sizeof(O) n_out bytes per cell (O = float64 or float32, the float64 result rounded once).  The
// relief, geomorphon and solar kernels take their LDS as dynamic memory of the size H asks for; MHS_TERRAIN_MAX_RADIUS = 45 is the
// largest H whose float64 tile, 122 x 154 x 8 = 150 304 bytes, stays within the 150 KiB a workgroup of this library may
// take of the CU's 160 KiB.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <mutex>
#include <vector>
#include "ensemble_int.h"
#include "solar_rule.h"
#include "terrain_rule.h"

namespace mhs {

static_assert(sizeof(SunEntry) == sizeof(mhs_sun_entry) && sizeof(SunEntry) == 64, "SunEntry is mhs_sun_entry");

constexpr int TER_NT = 256;                // threads per workgroup: 4 waves
constexpr int TER_TH = 32, TER_TW = 64;    // output tile
constexpr int TER_ROWS = TER_TH / 4;       // consecutive tile rows per lane

constexpr size_t terrain_tile_bytes(int H, size_t esz) { return (size_t)(TER_TH + 2 * H) * (TER_TW + 2 * H) * esz; }
static_assert(terrain_tile_bytes(MHS_TERRAIN_MAX_RADIUS, 8) <= LDS_LIMIT, "MHS_TERRAIN_MAX_RADIUS: the float64 tile must fit");
static_assert(terrain_tile_bytes(MHS_TERRAIN_MAX_RADIUS + 1, 8) > LDS_LIMIT, "MHS_TERRAIN_MAX_RADIUS is the largest that fits");
static_assert(MHS_TERRAIN_MAX_RADIUS >= 32, "the issue's floor");

struct TerrainGeom {
    const void *plane;       // element (0, 0) of the raster's plane (a row band's buffer: moved back to absolute row 0)
    int64_t ld;
    int nrow, ncol;          // the raster
    int r0, c0, nr, nc;      // the output window
    int tiles_x;
    int64_t n_tiles;
    double nodata;
    int has_nodata;
    const double *dx_row;    // device, by ABSOLUTE row, or NULL: dx everywhere
    double dx, dy, zf;
};

// the tile's cells in LDS: what the rules read through (terrain_rule.h)
template <typename T>
struct TileAcc {
    const T *centre;
    int lw;
    int up, down, left, right;
    bool has_nodata;
    double nodata;
    __device__ bool get(int dr, int dc, double &z) const {
        z = (double)centre[dr * lw + dc];
        return !terrain_na(z, has_nodata, nodata);
    }
};

// LDS rows [0, 32 + 2 H) x columns [0, 64 + 2 H) <- raster rows from r0 + tr0 - H, columns from c0 + tc0 - H
template <typename T>
__device__ inline void stage_tile(const TerrainGeom &g, T *sm, int tr0, int tc0, int H) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int LH = TER_TH + 2 * H, LW = TER_TW + 2 * H;
    const int ar0 = g.r0 + tr0 - H, ac0 = g.c0 + tc0 - H;
    const int rlo = max(0, g.r0 - H), rhi = min(g.nrow, g.r0 + g.nr + H);        // the raster within H of the window
    const int clo = max(0, g.c0 - H), chi = min(g.ncol, g.c0 + g.nc + H);
    const T *plane = (const T *)g.plane;
    for (int lr = wave; lr < LH; lr += 4) {
        const int ar = ar0 + lr;
        const bool rin = ar >= rlo && ar < rhi;
        for (int lc = lane; lc < LW; lc += 64) {
            const int ac = ac0 + lc;
            T v = (T)0;
            if (rin && ac >= clo && ac < chi) v = plane[(int64_t)ar * g.ld + ac];
            sm[lr * LW + lc] = v;
        }
    }
}

template <typename T, typename O>
__global__ __launch_bounds__(TER_NT) void terrain3_kernel(const TerrainGeom g, const unsigned mask, O *__restrict__ out,
                                                          const int64_t ld_out, const int64_t plane_stride) {
    constexpr int LW = TER_TW + 2;
    __shared__ T sm[(TER_TH + 2) * LW];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool has_nd = g.has_nodata != 0;
    for (int64_t tile = blockIdx.x; tile < g.n_tiles; tile += gridDim.x) {
        const int tr0 = (int)(tile / g.tiles_x) * TER_TH, tc0 = (int)(tile % g.tiles_x) * TER_TW;
        stage_tile<T>(g, sm, tr0, tc0, 1);
        __syncthreads();
        const int col = tc0 + lane, ac = g.c0 + col;
        if (col < g.nc) {
            const bool cin = ac >= 1 && ac < g.ncol - 1;
            const int lr0 = wave * TER_ROWS;                   // LDS row lr0 + j holds the row NORTH of output row lr0 + j
            double z[9];
            bool na_n, na_c, na_s;                             // any NA in the north / centre / south row of the 3 x 3
            auto load_row = [&](int lr, double *dst) -> bool {
                const int ar = g.r0 + tr0 + lr - 1;
                bool na = !(ar >= 0 && ar < g.nrow) || !cin;
                for (int k = 0; k < 3; ++k) {
                    dst[k] = (double)sm[lr * LW + lane + k];
                    na |= terrain_na(dst[k], has_nd, g.nodata);
                }
                return na;
            };
            na_c = load_row(lr0, z + 3);
            na_s = load_row(lr0 + 1, z + 6);
#pragma unroll
            for (int j = 0; j < TER_ROWS; ++j) {
                const int row = tr0 + lr0 + j;
                for (int k = 0; k < 6; ++k) z[k] = z[k + 3];
                na_n = na_c; na_c = na_s;
                na_s = load_row(lr0 + j + 2, z + 6);
                if (row >= g.nr) break;
                const bool na = na_n | na_c | na_s;
                const int ar = g.r0 + row;
                const double dx = g.dx_row ? g.dx_row[ar] : g.dx;
                double o[TV_COUNT];
                terrain_3x3(z, dx, g.dy, g.zf, mask, o);
                O *dst = out + (int64_t)row * ld_out + col;
#pragma unroll
                for (int k = 0; k < TV_COUNT; ++k)
                    if (mask & (1u << k)) { *dst = (O)(na ? (double)NAN : o[k]); dst += plane_stride; }
            }
        }
        __syncthreads();                                       // the next tile overwrites the LDS
    }
}

// the cell of tile row lr, tile column lane, which is cell (ar, ac) of the raster
template <typename T>
__device__ inline TileAcc<T> tile_acc(const TerrainGeom &g, const T *sm, int H, int lr, int lane, int ar, int ac) {
    const int LW = TER_TW + 2 * H;
    return TileAcc<T>{sm + (lr + H) * LW + lane + H, LW, ar, g.nrow - 1 - ar, ac, g.ncol - 1 - ac, g.has_nodata != 0, g.nodata};
}

template <typename T, typename O>
__global__ __launch_bounds__(TER_NT) void relief_kernel(const TerrainGeom g, const int R, const unsigned mask,
                                                        O *__restrict__ out, const int64_t ld_out, const int64_t plane_stride) {
    extern __shared__ __align__(16) unsigned char terrain_sm[];
    T *sm = (T *)terrain_sm;
    __shared__ int16_t w_sm[MHS_TERRAIN_MAX_RADIUS + 1];      // the half widths, read with the row offset as index
    if ((int)threadIdx.x <= R) w_sm[threadIdx.x] = (int16_t)relief_half_width(R, (int)threadIdx.x);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t tile = blockIdx.x; tile < g.n_tiles; tile += gridDim.x) {
        const int tr0 = (int)(tile / g.tiles_x) * TER_TH, tc0 = (int)(tile % g.tiles_x) * TER_TW;
        stage_tile<T>(g, sm, tr0, tc0, R);
        __syncthreads();
        const int col = tc0 + lane, ac = g.c0 + col;
        if (col < g.nc) {
            for (int j = 0; j < TER_ROWS; ++j) {
                const int lr = wave * TER_ROWS + j, row = tr0 + lr;
                if (row >= g.nr) break;
                const TileAcc<T> acc = tile_acc<T>(g, sm, R, lr, lane, g.r0 + row, ac);
                double e, o[RS_COUNT];
                const bool na = !acc.get(0, 0, e);
                if (!na) relief_cell(acc, R, w_sm, e, g.zf, o);
                O *dst = out + (int64_t)row * ld_out + col;
#pragma unroll
                for (int k = 0; k < RS_COUNT; ++k)
                    if (mask & (1u << k)) { *dst = (O)(na ? (double)NAN : o[k]); dst += plane_stride; }
            }
        }
        __syncthreads();
    }
}

template <typename T>
__global__ __launch_bounds__(TER_NT) void geomorphon_kernel(const TerrainGeom g, const int L, const double t, int16_t *__restrict__ out,
                                                            const int64_t ld_out) {
    extern __shared__ __align__(16) unsigned char terrain_sm[];
    T *sm = (T *)terrain_sm;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t tile = blockIdx.x; tile < g.n_tiles; tile += gridDim.x) {
        const int tr0 = (int)(tile / g.tiles_x) * TER_TH, tc0 = (int)(tile % g.tiles_x) * TER_TW;
        stage_tile<T>(g, sm, tr0, tc0, L);
        __syncthreads();
        const int col = tc0 + lane, ac = g.c0 + col;
        if (col < g.nc) {
            for (int j = 0; j < TER_ROWS; ++j) {
                const int lr = wave * TER_ROWS + j, row = tr0 + lr;
                if (row >= g.nr) break;
                const int ar = g.r0 + row;
                const TileAcc<T> acc = tile_acc<T>(g, sm, L, lr, lane, ar, ac);
                double e;
                int16_t form = GEOMORPHON_NA;
                if (acc.get(0, 0, e)) form = geomorphon_cell(acc, L, t, e, g.dx_row ? g.dx_row[ar] : g.dx, g.dy, g.zf);
                out[(int64_t)row * ld_out + col] = form;
            }
        }
        __syncthreads();
    }
}

// the sun tables of a solar call on the device (mhs_sun_tables, uploaded once per call)
struct SolarTabs {
    const int32_t *tab_row;     // by ABSOLUTE row, or NULL: table 0
    const int64_t *start;       // n_tab * 16 + 1
    const SunEntry *entries;
    const double *omega;        // n_tab * 16
};

// The solar products (solar_rule.h), with the geometry of geomorphon_kernel.  A wave works on ONE raster row at a time, so
// the row's table index, its offsets, its entries and its sector weights are wave-uniform: the index goes through
// readfirstlane and the 64-byte entries come through the scalar cache (the tables are __restrict__ kernel arguments of their
// own: only then does the compiler know that the stores to out leave them alone and make the loads scalar).  Only what the
// mask asks for is made: no table walk for svf or horizon alone, no slope without direct.
template <typename T, typename O>
__global__ __launch_bounds__(TER_NT) void solar_kernel(const TerrainGeom g, const int L, const unsigned mask,
                                                       const int32_t *__restrict__ tab_row, const int64_t *__restrict__ tab_start,
                                                       const SunEntry *__restrict__ entries, const double *__restrict__ omega_all,
                                                       O *__restrict__ out, const int64_t ld_out, const int64_t plane_stride) {
    extern __shared__ __align__(16) unsigned char terrain_sm[];
    T *sm = (T *)terrain_sm;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool want_svf = mask & (1u << SP_SVF), want_direct = mask & (1u << SP_DIRECT), want_hours = mask & (1u << SP_SUN_HOURS);
    for (int64_t tile = blockIdx.x; tile < g.n_tiles; tile += gridDim.x) {
        const int tr0 = (int)(tile / g.tiles_x) * TER_TH, tc0 = (int)(tile % g.tiles_x) * TER_TW;
        stage_tile<T>(g, sm, tr0, tc0, L);
        __syncthreads();
        const int col = tc0 + lane, ac = g.c0 + col;
        if (col < g.nc) {
            for (int j = 0; j < TER_ROWS; ++j) {
                const int lr = wave * TER_ROWS + j, row = tr0 + lr;
                if (row >= g.nr) break;
                const int ar = __builtin_amdgcn_readfirstlane(g.r0 + row);
                const TileAcc<T> acc = tile_acc<T>(g, sm, L, lr, lane, ar, ac);
                const double dx = g.dx_row ? g.dx_row[ar] : g.dx;
                double e, H[SOLAR_DIRS], svf = 0.0, beam = 0.0, hrs = 0.0;
                const bool na = !acc.get(0, 0, e);
                bool na_slope = true;
                if (!na) {
                    solar_horizon(acc, L, e, dx, g.dy, g.zf, H);
                    const int b = (want_svf || want_direct || want_hours) && tab_row ? __builtin_amdgcn_readfirstlane(tab_row[ar]) : 0;
                    if (want_svf) svf = solar_svf(H, omega_all + (size_t)b * SOLAR_DIRS);
                    if (want_direct || want_hours) {
                        const int64_t *start = tab_start + (size_t)b * SOLAR_DIRS;
                        double dzdx = 0.0, dzdy = 0.0, nrm = 1.0;
                        if (want_direct) na_slope = !solar_slope(acc, dx, g.dy, g.zf, dzdx, dzdy, nrm);
                        if (!want_direct) solar_walk<false, true>(H, start, entries, dzdx, dzdy, beam, hrs);
                        else if (!want_hours) solar_walk<true, false>(H, start, entries, dzdx, dzdy, beam, hrs);
                        else solar_walk<true, true>(H, start, entries, dzdx, dzdy, beam, hrs);
                        beam = beam / nrm;
                    }
                }
                const double nan = (double)NAN;
                O *dst = out + (int64_t)row * ld_out + col;
                if (want_svf) { *dst = (O)(na ? nan : svf); dst += plane_stride; }
                if (want_direct) { *dst = (O)(na || na_slope ? nan : beam); dst += plane_stride; }
                if (want_hours) { *dst = (O)(na ? nan : hrs); dst += plane_stride; }
                if (mask & (1u << SP_HORIZON)) {
#pragma unroll
                    for (int k = 0; k < SOLAR_DIRS; ++k) { *dst = (O)(na ? nan : H[k]); dst += plane_stride; }
                }
            }
        }
        __syncthreads();
    }
}

static unsigned terrain_blocks(int64_t n_tiles) {
    const int n_cu = ctx().n_cu > 0 ? ctx().n_cu : 256;
    return (unsigned)std::min<int64_t>(n_tiles, (int64_t)n_cu * 32);
}

// a kernel whose dynamic LDS passes 64 KiB has to be told so
template <typename K>
static int allow_lds(K kernel, size_t bytes) {
    if (bytes > (size_t)64 * 1024) MHS_HIP(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return MHS_OK;
}

template <typename T, typename O>
static int launch_terrain_to(const TerrainGeom &g, unsigned mask, void *out, int64_t ld, int64_t ps, hipStream_t st) {
    hipLaunchKernelGGL((terrain3_kernel<T, O>), dim3(terrain_blocks(g.n_tiles)), dim3(TER_NT), 0, st, g, mask, (O *)out, ld, ps);
    return MHS_OK;
}
template <typename T, typename O>
static int launch_relief_to(const TerrainGeom &g, int R, unsigned mask, void *out, int64_t ld, int64_t ps, hipStream_t st) {
    const size_t sm = terrain_tile_bytes(R, sizeof(T));
    if (int rc = allow_lds(relief_kernel<T, O>, sm)) return rc;
    hipLaunchKernelGGL((relief_kernel<T, O>), dim3(terrain_blocks(g.n_tiles)), dim3(TER_NT), sm, st, g, R, mask, (O *)out, ld, ps);
    return MHS_OK;
}
template <typename T>
static int launch_geomorphon_t(const TerrainGeom &g, int L, double t, int16_t *out, int64_t ld, hipStream_t st) {
    const size_t sm = terrain_tile_bytes(L, sizeof(T));
    if (int rc = allow_lds(geomorphon_kernel<T>, sm)) return rc;
    hipLaunchKernelGGL((geomorphon_kernel<T>), dim3(terrain_blocks(g.n_tiles)), dim3(TER_NT), sm, st, g, L, t, out, ld);
    return MHS_OK;
}

template <typename T, typename O>
static int launch_solar_to(const TerrainGeom &g, int L, unsigned mask, const SolarTabs &tabs, void *out, int64_t ld, int64_t ps, hipStream_t st) {
    const size_t sm = terrain_tile_bytes(L, sizeof(T));
    if (int rc = allow_lds(solar_kernel<T, O>, sm)) return rc;
    hipLaunchKernelGGL((solar_kernel<T, O>), dim3(terrain_blocks(g.n_tiles)), dim3(TER_NT), sm, st, g, L, mask, tabs.tab_row, tabs.start, tabs.entries, tabs.omega,
                       (O *)out, ld, ps);
    return MHS_OK;
}

// what a call makes: the 3 x 3 variables, the relief statistics, the geomorphons or the solar products
struct TerrainJob {
    int kind;               // 0 terrain, 1 relief, 2 geomorphon, 3 solar
    unsigned mask;
    int H;                  // halo: 1, the radius, the search length
    double t;               // geomorphon: flat_deg (pi / 180)
    int out_dtype;          // MHS_F64 / MHS_F32 (geomorphon: int16)
    int n_out;
    size_t out_esz;
    const mhs_sun_tables *tables;   // solar: the caller's tables on the HOST, or NULL (horizon alone)
    SolarTabs tabs;                 // solar: the same on the device, set by solar_upload
};

// the window (g.r0, g.c0, g.nr, g.nc filled in) of the plane `dtype` into out
static int launch_job(const TerrainJob &job, TerrainGeom g, int dtype, void *out, int64_t ld, int64_t ps, hipStream_t st) {
    if (g.nr == 0 || g.nc == 0) return MHS_OK;
    g.tiles_x = (g.nc + TER_TW - 1) / TER_TW;
    g.n_tiles = (int64_t)g.tiles_x * ((g.nr + TER_TH - 1) / TER_TH);
    int rc = MHS_OK;
    const bool f64 = job.out_dtype == MHS_F64;
    if (job.kind == 0) {
        if (dtype == MHS_F64) rc = f64 ? launch_terrain_to<double, double>(g, job.mask, out, ld, ps, st) : launch_terrain_to<double, float>(g, job.mask, out, ld, ps, st);
        else if (dtype == MHS_F32) rc = f64 ? launch_terrain_to<float, double>(g, job.mask, out, ld, ps, st) : launch_terrain_to<float, float>(g, job.mask, out, ld, ps, st);
        else rc = f64 ? launch_terrain_to<short, double>(g, job.mask, out, ld, ps, st) : launch_terrain_to<short, float>(g, job.mask, out, ld, ps, st);
    } else if (job.kind == 1) {
        if (dtype == MHS_F64) rc = f64 ? launch_relief_to<double, double>(g, job.H, job.mask, out, ld, ps, st) : launch_relief_to<double, float>(g, job.H, job.mask, out, ld, ps, st);
        else if (dtype == MHS_F32) rc = f64 ? launch_relief_to<float, double>(g, job.H, job.mask, out, ld, ps, st) : launch_relief_to<float, float>(g, job.H, job.mask, out, ld, ps, st);
        else rc = f64 ? launch_relief_to<short, double>(g, job.H, job.mask, out, ld, ps, st) : launch_relief_to<short, float>(g, job.H, job.mask, out, ld, ps, st);
    } else if (job.kind == 3) {
        if (dtype == MHS_F64) rc = f64 ? launch_solar_to<double, double>(g, job.H, job.mask, job.tabs, out, ld, ps, st) : launch_solar_to<double, float>(g, job.H, job.mask, job.tabs, out, ld, ps, st);
        else if (dtype == MHS_F32) rc = f64 ? launch_solar_to<float, double>(g, job.H, job.mask, job.tabs, out, ld, ps, st) : launch_solar_to<float, float>(g, job.H, job.mask, job.tabs, out, ld, ps, st);
        else rc = f64 ? launch_solar_to<short, double>(g, job.H, job.mask, job.tabs, out, ld, ps, st) : launch_solar_to<short, float>(g, job.H, job.mask, job.tabs, out, ld, ps, st);
    } else {
        if (dtype == MHS_F64) rc = launch_geomorphon_t<double>(g, job.H, job.t, (int16_t *)out, ld, st);
        else if (dtype == MHS_F32) rc = launch_geomorphon_t<float>(g, job.H, job.t, (int16_t *)out, ld, st);
        else rc = launch_geomorphon_t<short>(g, job.H, job.t, (int16_t *)out, ld, st);
    }
    if (rc) return rc;
    MHS_HIP(hipGetLastError());
    return MHS_OK;
}

static int popcount(unsigned m) { int n = 0; for (; m; m &= m - 1) ++n; return n; }

#define TER_REQUIRE(cond, ...)                                             \
    do {                                                                   \
        if (!(cond)) { set_error(__VA_ARGS__); return MHS_ERR_INVALID; }    \
    } while (0)

// Every check of a terrain call, before any device call; fn = the entry point's name for the message.  Fills job and geom
// (but for the plane pointer and dx_row).
static int terrain_check(const char *fn, int kind, const mhs_grid *grid, const mhs_stack *dem, int layer, const mhs_terrain_units *u,
                         int H, double flat_deg, int64_t r0, int64_t r1, int64_t c0, int64_t c1, unsigned mask, const void *out,
                         int out_dtype, int64_t ld, int64_t plane_stride, TerrainJob *job, TerrainGeom *g) {
    TER_REQUIRE(grid && dem && u, "%s: NULL argument (grid, dem or units)", fn);
    TER_REQUIRE(grid->nrow > 0 && grid->ncol > 0 && grid->nrow < (1LL << 30) && grid->ncol < (1LL << 30), "%s: bad grid geometry (nrow, ncol must be in 1 .. 2^30)", fn);
    TER_REQUIRE(0 <= r0 && r0 <= r1 && r1 <= grid->nrow && 0 <= c0 && c0 <= c1 && c1 <= grid->ncol, "%s: window outside the grid", fn);
    TER_REQUIRE(dem->data, "%s: dem data is NULL", fn);
    TER_REQUIRE(dem->dtype == MHS_F64 || dem->dtype == MHS_F32 || dem->dtype == MHS_I16, "%s: bad dem dtype", fn);
    TER_REQUIRE(layer >= 0 && layer < dem->n_layers, "%s: layer %d is not one of the stack's %d layers", fn, layer, dem->n_layers);
    TER_REQUIRE(dem->ld >= grid->ncol && (dem->n_layers == 1 || dem->plane_stride >= dem->ld * (grid->nrow - 1) + grid->ncol),
                "%s: dem strides smaller than the grid", fn);          // a single plane has no stride to speak of
    const char *what = kind == 1 ? "radius" : "search";
    if (kind != 0)
        TER_REQUIRE(H >= 1 && H <= MHS_TERRAIN_MAX_RADIUS, "%s: %s must be in 1 .. %d (MHS_TERRAIN_MAX_RADIUS), got %d", fn, what, MHS_TERRAIN_MAX_RADIUS, H);
    if (kind == 2) TER_REQUIRE(std::isfinite(flat_deg) && flat_deg >= 0.0, "%s: flat_deg must be finite and not negative", fn);
    TER_REQUIRE(std::isfinite(u->z_factor) && u->z_factor > 0.0, "%s: z_factor must be finite and positive", fn);
    if (kind != 1) {            // relief has no horizontal distance in it
        TER_REQUIRE(std::isfinite(u->dy) && u->dy > 0.0, "%s: dy must be finite and positive", fn);
        if (u->dx_row) {
            for (int64_t r = 0; r < grid->nrow; ++r)
                TER_REQUIRE(std::isfinite(u->dx_row[r]) && u->dx_row[r] > 0.0, "%s: dx_row[%lld] must be finite and positive", fn, (long long)r);
        } else TER_REQUIRE(std::isfinite(u->dx) && u->dx > 0.0, "%s: dx must be finite and positive (or give dx_row)", fn);
    }
    const unsigned all = kind == 0 ? (1u << TV_COUNT) - 1 : kind == 1 ? (1u << RS_COUNT) - 1 : (1u << SP_COUNT) - 1;
    if (kind != 2) {
        TER_REQUIRE(mask != 0 && (mask & ~all) == 0, "%s: %s mask 0x%x selects nothing or unknown bits", fn, kind == 0 ? "vars" : kind == 1 ? "stats" : "products", mask);
        TER_REQUIRE(out_dtype == MHS_F64 || out_dtype == MHS_F32, "%s: out_dtype must be MHS_F64 or MHS_F32", fn);
    }
    TER_REQUIRE(out, "%s: out is NULL", fn);
    TER_REQUIRE(ld >= c1 - c0, "%s: ld smaller than the window width", fn);
    job->kind = kind; job->mask = mask; job->H = kind == 0 ? 1 : H; job->t = flat_deg * TERRAIN_RAD;
    job->out_dtype = out_dtype; job->n_out = kind == 2 ? 1 : kind == 3 ? popcount(mask & 7u) + (mask >> SP_HORIZON & 1u) * SOLAR_DIRS : popcount(mask);
    job->tables = nullptr; job->tabs = SolarTabs{nullptr, nullptr, nullptr, nullptr};
    job->out_esz = kind == 2 ? 2 : out_dtype == MHS_F64 ? 8 : 4;
    if (job->n_out > 1) TER_REQUIRE(plane_stride >= ld * (r1 - r0 - 1) + (c1 - c0), "%s: plane_stride smaller than an output plane", fn);
    *g = TerrainGeom{nullptr, dem->ld, (int)grid->nrow, (int)grid->ncol, (int)r0, (int)c0, (int)(r1 - r0), (int)(c1 - c0), 0, 0,
                     dem->nodata, !std::isnan(dem->nodata), nullptr, u->dx, u->dy, u->z_factor};
    return MHS_OK;
}

// Every check of the sun tables of a solar call (section "solar", (c)), before any device call.
static int solar_check(const char *fn, const mhs_grid *grid, const mhs_sun_tables *t, unsigned mask) {
    if (!t) {
        TER_REQUIRE((mask & ~(1u << SP_HORIZON)) == 0, "%s: tables is NULL (only the horizon product needs none)", fn);
        return MHS_OK;
    }
    TER_REQUIRE(t->n_tab >= 1, "%s: tables->n_tab must be at least 1, got %d", fn, (int)t->n_tab);
    TER_REQUIRE(t->start && t->omega, "%s: tables->start or tables->omega is NULL", fn);
    const int64_t ns = (int64_t)t->n_tab * SOLAR_DIRS;
    TER_REQUIRE(t->start[0] == 0, "%s: tables->start[0] must be 0", fn);
    for (int64_t k = 0; k < ns; ++k) {
        TER_REQUIRE(t->start[k + 1] >= t->start[k], "%s: tables->start[%lld] decreases", fn, (long long)(k + 1));
        TER_REQUIRE(t->start[k + 1] <= MHS_SOLAR_MAX_ENTRIES, "%s: tables->start[%lld]: more than %d entries (MHS_SOLAR_MAX_ENTRIES)", fn,
                    (long long)(k + 1), MHS_SOLAR_MAX_ENTRIES);
        TER_REQUIRE(std::isfinite(t->omega[k]) && t->omega[k] >= 0.0, "%s: tables->omega[%lld] must be finite and not negative", fn, (long long)k);
    }
    const int64_t n = t->start[ns];
    TER_REQUIRE(n == 0 || t->entries, "%s: tables->entries is NULL", fn);
    for (int64_t i = 0; i < n; ++i) {
        const mhs_sun_entry &s = t->entries[i];
        TER_REQUIRE(s.t >= 0.0 && s.t <= 1.0, "%s: tables->entries[%lld].t must be in [0, 1]", fn, (long long)i);
        TER_REQUIRE(std::isfinite(s.tan_h) && s.tan_h > 0.0, "%s: tables->entries[%lld].tan_h must be finite and positive", fn, (long long)i);
        TER_REQUIRE(std::isfinite(s.ux) && std::isfinite(s.uy) && std::isfinite(s.uz), "%s: tables->entries[%lld].ux, uy, uz must be finite", fn, (long long)i);
        TER_REQUIRE(std::isfinite(s.w) && s.w >= 0.0, "%s: tables->entries[%lld].w must be finite and not negative", fn, (long long)i);
        TER_REQUIRE(std::isfinite(s.d) && s.d >= 0.0, "%s: tables->entries[%lld].d must be finite and not negative", fn, (long long)i);
    }
    if (t->tab_row)
        for (int64_t r = 0; r < grid->nrow; ++r)
            TER_REQUIRE(t->tab_row[r] >= 0 && t->tab_row[r] < t->n_tab, "%s: tables->tab_row[%lld] = %d is not in 0 .. n_tab - 1", fn, (long long)r, (int)t->tab_row[r]);
    return MHS_OK;
}

// What a call keeps on the device beside the planes: dx_row and, for a solar call, the sun tables, each piece rounded up to
// 256 bytes.  up_bytes = the size of the block; upload enqueues the copies into it and sets g.dx_row and job.tabs.
static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
static size_t up_bytes(const TerrainJob &job, const TerrainGeom &g, const mhs_terrain_units *u) {
    size_t n = job.kind != 1 && u->dx_row ? up256(sizeof(double) * (size_t)g.nrow) : 0;
    if (const mhs_sun_tables *t = job.tables) {
        const size_t ns = (size_t)t->n_tab * SOLAR_DIRS;
        n += up256(sizeof(int64_t) * (ns + 1)) + up256(sizeof(double) * ns) + up256(sizeof(mhs_sun_entry) * (size_t)t->start[ns]);
        if (t->tab_row) n += up256(sizeof(int32_t) * (size_t)g.nrow);
    }
    return n;
}
static int upload(TerrainJob &job, TerrainGeom &g, const mhs_terrain_units *u, char *base, hipStream_t st) {
    auto put = [&](const void *src, size_t bytes) -> const void * {
        char *dst = base;
        base += up256(bytes);
        return bytes == 0 || hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) == hipSuccess ? dst : nullptr;
    };
    bool ok = true;
    if (job.kind != 1 && u->dx_row) ok &= (g.dx_row = (const double *)put(u->dx_row, sizeof(double) * (size_t)g.nrow)) != nullptr;
    if (const mhs_sun_tables *t = job.tables) {
        const size_t ns = (size_t)t->n_tab * SOLAR_DIRS;
        ok &= (job.tabs.start = (const int64_t *)put(t->start, sizeof(int64_t) * (ns + 1))) != nullptr;
        ok &= (job.tabs.omega = (const double *)put(t->omega, sizeof(double) * ns)) != nullptr;
        ok &= (job.tabs.entries = (const SunEntry *)put(t->entries, sizeof(mhs_sun_entry) * (size_t)t->start[ns])) != nullptr;
        if (t->tab_row) ok &= (job.tabs.tab_row = (const int32_t *)put(t->tab_row, sizeof(int32_t) * (size_t)g.nrow)) != nullptr;
    }
    if (!ok) { MHS_HIP(hipGetLastError()); return MHS_ERR_HIP; }
    return MHS_OK;
}

// device planes: only enqueues.  dx_row and the sun tables go up once, into stream-ordered memory that is given back behind
// the kernel.
static int terrain_dev(TerrainJob job, TerrainGeom g, const mhs_stack *dem, int layer, const mhs_terrain_units *u, void *out,
                       int64_t ld, int64_t ps, void *stream) {
    if (int rc = require_ready()) return rc;
    hipStream_t st = pick_stream(stream);
    g.plane = (const char *)dem->data + (size_t)layer * dem->plane_stride * dtype_bytes(dem->dtype);
    if (g.nr == 0 || g.nc == 0) return MHS_OK;
    char *up = nullptr;
    if (const size_t bytes = up_bytes(job, g, u)) {
        MHS_HIP(hipMallocAsync((void **)&up, bytes, st));
        if (int rc = upload(job, g, u, up, st)) {
            (void)hipFreeAsync(up, st);
            return rc;
        }
    }
    const int rc = launch_job(job, g, dem->dtype, out, ld, ps, st);
    if (up) (void)hipFreeAsync(up, st);
    return rc;
}

// Host planes in, host planes out: row bands of the window, each with the H halo rows the raster has above and below it, go
// up, through the same kernels and down again on one stream of the library's host-pointer pipeline, as mhs_mess_grid's do.
// A band's buffer is described as the raster's plane moved back to absolute row 0, so its cells get the one-piece call's
// bits.  MHS_HOST_BANDS = n forces n equal bands.
static int terrain_host(TerrainJob job, TerrainGeom g, const mhs_stack *dem, int layer, const mhs_terrain_units *u, void *out_host) {
    if (int rc = require_ready()) return rc;
    const int64_t nr = g.nr, nc = g.nc, r0 = g.r0, r1 = r0 + nr;
    if (nr == 0 || nc == 0) return MHS_OK;
    const size_t esz = dtype_bytes(dem->dtype);
    const size_t row_bytes = (size_t)dem->ld * esz + (size_t)nc * job.out_esz * job.n_out;
    int64_t rows_per = std::max<int64_t>(1, std::min<int64_t>(nr, (int64_t)(((size_t)256 << 20) / row_bytes)));
    if (const char *e = getenv("MHS_HOST_BANDS")) {
        const int64_t nb = std::max<int64_t>(1, std::min<int64_t>(nr, atoll(e)));
        rows_per = (nr + nb - 1) / nb;
    }
    const size_t head_bytes = up_bytes(job, g, u);                                     // dx_row and the sun tables
    const size_t in_bytes = ((size_t)(rows_per + 2 * job.H) * dem->ld * esz + 255) & ~(size_t)255;
    const size_t plane_out = (size_t)rows_per * nc;                                  // elements of one output plane of a band
    const size_t out_bytes = (plane_out * job.out_esz * job.n_out + 255) & ~(size_t)255;
    std::lock_guard<std::mutex> lk(pipe_mutex());
    if (int rc = host_pipe(head_bytes + in_bytes + out_bytes)) return rc;
    Context &c = ctx();
    hipStream_t st = c.pipe_comp;
    char *in = c.pipe_arena + head_bytes, *outb = in + in_bytes;
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{st};   // no copy is left in flight, whatever the exit
    if (int rc = upload(job, g, u, c.pipe_arena, st)) return rc;
    const char *src = (const char *)dem->data + (size_t)layer * dem->plane_stride * esz;
    for (int64_t b0 = r0; b0 < r1; b0 += rows_per) {
        const int64_t b1 = std::min(r1, b0 + rows_per);
        const int64_t i0 = std::max<int64_t>(0, b0 - job.H), i1 = std::min<int64_t>(g.nrow, b1 + job.H);       // rows that go up
        MHS_HIP(hipMemcpyAsync(in, src + (size_t)i0 * dem->ld * esz, ((size_t)(i1 - i0 - 1) * dem->ld + g.ncol) * esz, hipMemcpyHostToDevice, st));
        TerrainGeom bg = g;
        bg.plane = in - (size_t)i0 * dem->ld * esz;
        bg.r0 = (int)b0; bg.nr = (int)(b1 - b0);
        if (int rc = launch_job(job, bg, dem->dtype, outb, nc, (int64_t)plane_out, st)) return rc;
        for (int p = 0; p < job.n_out; ++p)
            MHS_HIP(hipMemcpyAsync((char *)out_host + ((size_t)p * nr * nc + (size_t)(b0 - r0) * nc) * job.out_esz, outb + (size_t)p * plane_out * job.out_esz,
                                   (size_t)(b1 - b0) * nc * job.out_esz, hipMemcpyDeviceToHost, st));
        MHS_HIP(hipStreamSynchronize(st));       // the next band reuses the buffers
    }
    return MHS_OK;
}

}  // namespace mhs

using namespace mhs;

extern "C" {

int mhs_terrain_max_radius(void) { return MHS_TERRAIN_MAX_RADIUS; }

int mhs_terrain_dev(const mhs_grid *g, const mhs_stack *dem, int layer, const mhs_terrain_units *units, int64_t r0, int64_t r1,
                    int64_t c0, int64_t c1, unsigned vars, void *out_dev, int out_dtype, int64_t ld, int64_t plane_stride, void *stream) {
    TerrainJob job; TerrainGeom tg;
    if (int rc = terrain_check(__func__, 0, g, dem, layer, units, 1, 0.0, r0, r1, c0, c1, vars, out_dev, out_dtype, ld, plane_stride, &job, &tg)) return rc;
    return terrain_dev(job, tg, dem, layer, units, out_dev, ld, plane_stride, stream);
}

int mhs_relief_dev(const mhs_grid *g, const mhs_stack *dem, int layer, const mhs_terrain_units *units, int radius, int64_t r0,
                   int64_t r1, int64_t c0, int64_t c1, unsigned stats, void *out_dev, int out_dtype, int64_t ld, int64_t plane_stride,
                   void *stream) {
    TerrainJob job; TerrainGeom tg;
    if (int rc = terrain_check(__func__, 1, g, dem, layer, units, radius, 0.0, r0, r1, c0, c1, stats, out_dev, out_dtype, ld, plane_stride, &job, &tg)) return rc;
    return terrain_dev(job, tg, dem, layer, units, out_dev, ld, plane_stride, stream);
}

int mhs_geomorphon_dev(const mhs_grid *g, const mhs_stack *dem, int layer, const mhs_terrain_units *units, int search, double flat_deg,
                       int64_t r0, int64_t r1, int64_t c0, int64_t c1, int16_t *out_dev, int64_t ld, void *stream) {
    TerrainJob job; TerrainGeom tg;
    if (int rc = terrain_check(__func__, 2, g, dem, layer, units, search, flat_deg, r0, r1, c0, c1, 0, out_dev, MHS_I16, ld, 0, &job, &tg)) return rc;
    return terrain_dev(job, tg, dem, layer, units, out_dev, ld, 0, stream);
}

int mhs_solar_dev(const mhs_grid *g, const mhs_stack *dem, int layer, const mhs_terrain_units *units, int search,
                  const mhs_sun_tables *tables, int64_t r0, int64_t r1, int64_t c0, int64_t c1, unsigned products, void *out_dev,
                  int out_dtype, int64_t ld, int64_t plane_stride, void *stream) {
    TerrainJob job; TerrainGeom tg;
    if (int rc = terrain_check(__func__, 3, g, dem, layer, units, search, 0.0, r0, r1, c0, c1, products, out_dev, out_dtype, ld, plane_stride, &job, &tg)) return rc;
    if (int rc = solar_check(__func__, g, tables, products)) return rc;
    job.tables = tables;
    return terrain_dev(job, tg, dem, layer, units, out_dev, ld, plane_stride, stream);
}

int mhs_solar(const mhs_grid *g, const mhs_stack *dem, int layer, const mhs_terrain_units *units, int search,
              const mhs_sun_tables *tables, int64_t r0, int64_t r1, int64_t c0, int64_t c1, unsigned products, void *out_host, int out_dtype) {
    TerrainJob job; TerrainGeom tg;
    if (int rc = terrain_check(__func__, 3, g, dem, layer, units, search, 0.0, r0, r1, c0, c1, products, out_host, out_dtype, c1 - c0, (r1 - r0) * (c1 - c0), &job, &tg)) return rc;
    if (int rc = solar_check(__func__, g, tables, products)) return rc;
    job.tables = tables;
    return terrain_host(job, tg, dem, layer, units, out_host);
}

int mhs_terrain(const mhs_grid *g, const mhs_stack *dem, int layer, const mhs_terrain_units *units, int64_t r0, int64_t r1, int64_t c0,
                int64_t c1, unsigned vars, void *out_host, int out_dtype) {
    TerrainJob job; TerrainGeom tg;
    if (int rc = terrain_check(__func__, 0, g, dem, layer, units, 1, 0.0, r0, r1, c0, c1, vars, out_host, out_dtype, c1 - c0, (r1 - r0) * (c1 - c0), &job, &tg)) return rc;
    return terrain_host(job, tg, dem, layer, units, out_host);
}

int mhs_relief(const mhs_grid *g, const mhs_stack *dem, int layer, const mhs_terrain_units *units, int radius, int64_t r0, int64_t r1,
               int64_t c0, int64_t c1, unsigned stats, void *out_host, int out_dtype) {
    TerrainJob job; TerrainGeom tg;
    if (int rc = terrain_check(__func__, 1, g, dem, layer, units, radius, 0.0, r0, r1, c0, c1, stats, out_host, out_dtype, c1 - c0, (r1 - r0) * (c1 - c0), &job, &tg)) return rc;
    return terrain_host(job, tg, dem, layer, units, out_host);
}

int mhs_geomorphon(const mhs_grid *g, const mhs_stack *dem, int layer, const mhs_terrain_units *units, int search, double flat_deg,
                   int64_t r0, int64_t r1, int64_t c0, int64_t c1, int16_t *out_host) {
    TerrainJob job; TerrainGeom tg;
    if (int rc = terrain_check(__func__, 2, g, dem, layer, units, search, flat_deg, r0, r1, c0, c1, 0, out_host, MHS_I16, c1 - c0, 0, &job, &tg)) return rc;
    return terrain_host(job, tg, dem, layer, units, out_host);
}

}  // extern "C"
