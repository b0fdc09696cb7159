// Hydrology of one elevation plane (include/machisplin_hip.h, section "hydrology", states the rules; hydro_rule.h holds
// them): the flat-filled surface W, the flat distance D, the D8 direction, the flow accumulation A and the topographic
// wetness index.
//
// Geometry as in terrain.hip: a workgroup of 256 threads takes tiles of HY_TH x HY_TW = 32 x 64 cells and stages each with a
// halo of one cell in LDS, wave w taking LDS rows w, w + 4, ... and its 64 lanes 64 consecutive elements of a row, so every
// global load and store of a wave is 64 consecutive elements; lane l of wave w then owns the 8 cells of tile column l in tile
// rows 8 w .. 8 w + 7.
//
// W, D and A are fixed points over the whole plane.  Each has a SOLVE kernel: a workgroup stages its tile and the halo, sweeps
// the rule over its own cells in LDS, in place, until a sweep changes nothing (a block-wide OR over the barrier), and writes
// the tile back.  A sweep that changes nothing leaves every cell equal to its rule applied to values that did not move during
// the sweep: the tile's fixed point for this halo.  A tile has 2 048 cells and a fixed point is reached in at most that many
// sweeps (every sweep before the last settles at least one more cell for good), so the bound HY_MAX_SWEEPS = 2 049 is never
// what ends the loop, and nothing can spin.
//
// The updates are MONOTONE (W and D only fall from +inf / HYDRO_D_INF, A only rises from 1), so the plane's fixed point does
// not depend on the order of the sweeps, on the order of the tiles, or on whether a halo value a workgroup reads is the one
// from before or after its neighbour's write-back in the same launch: an old value is merely a weaker bound that the next
// pass tightens.  A value is one aligned 4- or 8-byte store and is never torn.  Hence every result is an exact function of
// the input, whatever the schedule.
//
// The HOST drives each phase: passes (ordinary launches) until one reports no change.  A workgroup whose perimeter cells
// changed marks the up-to-8 neighbouring tiles in the NEXT pass's dirty array with plain byte stores and bumps a change
// counter with one atomicAdd; a tile that is not dirty in the current pass is skipped at once.  The two dirty arrays
// ping-pong across launches.  That is all the communication there is, and only the next launch reads it: no grid barrier, no
// cooperative launch, no spin wait.  The host reads the counter back through the stream after every pass.
//
// Scratch, per cell: W 8 + D 4 + direction 1 + A 8 + flags 1 = 22 bytes, plus 2 bytes per tile and dx_row, in ONE block of
// stream-ordered memory given back behind the last kernel.
//
// The MULTIPLE FLOW DIRECTION route (section "hydrology, multiple flow direction" of the header) shares the init, fill, seed
// and flat phases (HydroWork::surface) and replaces the direction and the D8 accumulation: a SHARES kernel makes every
// valid cell's eight shares once (the only place pow is called) and stores each into the RECEIVER's slot of the
// incoming-share plane F -- eight doubles per cell, plane k holding f(neighbour k -> cell) -- and the MFD solve kernel, built
// like hydro_acc_kernel, loads a cell's eight incoming shares into registers once per tile solve and sweeps
// A(c) = 1 + sum_k F_k(c) A(k).  The shares are static and >= 0 and rounding is monotone, so A only rises from 1 and the
// argument above holds unchanged; the flow graph is acyclic because (W, D) falls strictly along every positive share, so
// the fixed point is unique and a cell is final one sweep after its donors are.
// Scratch of that route, per cell: W 8 + D 4 + A 8 + flags 1 + F 64 = 85 bytes (no direction plane).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <mutex>
#include "ensemble_int.h"
#include "hydro_rule.h"

namespace mhs {

constexpr int HY_NT = 256;                  // threads per workgroup: 4 waves
constexpr int HY_TH = 32, HY_TW = 64;       // tile
constexpr int HY_ROWS = HY_TH / 4;          // consecutive tile rows per lane
constexpr int HY_LH = HY_TH + 2, HY_LW = HY_TW + 2;
constexpr int HY_MAX_SWEEPS = HY_TH * HY_TW + 1;
constexpr int64_t HY_MAX_CELLS = 1LL << 56;      // every byte count of a call (at most 85 per cell of scratch; the host entry's planes, at most 33) fits a size_t
enum { HF_VALID = 1, HF_OUTLET = 2, HF_RAISED = 4 };                    // the flags plane
enum { HS_NORTH = 1, HS_SOUTH = 2, HS_WEST = 4, HS_EAST = 8 };          // sides of a tile whose cells changed
enum { HC_CHANGE = 0, HC_VALID, HC_RAISED, HC_SINKS, HC_SOLVES, HC_COUNT };   // the counters

struct HydroGeom {
    int nrow, ncol;
    int tiles_x, tiles_y;
    int64_t n_tiles;
    double nodata;
    int has_nodata;
    const double *dx_row;    // device, by row, or NULL: dx everywhere
    double dx, dy, zf;
};

// what a solve pass reads and writes beside its planes
struct HydroPass {
    unsigned char *cur;              // dirty in this pass (a solved tile clears its own entry)
    unsigned char *nxt;              // dirty in the next pass
    unsigned long long *counters;    // HC_COUNT of them
};

// LDS rows [0, 34) x columns [0, 66) <- plane rows from tr0 - 1, columns from tc0 - 1; `outside` where the raster has no cell
template <typename V>
__device__ inline void hydro_stage(const HydroGeom &g, V *sm, const V *plane, int tr0, int tc0, V outside) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int lr = wave; lr < HY_LH; lr += 4) {
        const int ar = tr0 - 1 + lr;
        const bool rin = ar >= 0 && ar < g.nrow;
        for (int lc = lane; lc < HY_LW; lc += 64) {
            const int ac = tc0 - 1 + lc;
            V v = outside;
            if (rin && ac >= 0 && ac < g.ncol) v = plane[(int64_t)ar * g.ncol + ac];
            sm[lr * HY_LW + lc] = v;
        }
    }
}

// the eight neighbours of the LDS cell `c` (hydro_rule.h's order)
template <typename V>
__device__ inline void hydro_gather(const V *c, V out[8]) {
    out[0] = c[1];          out[1] = c[HY_LW + 1];  out[2] = c[HY_LW];   out[3] = c[HY_LW - 1];
    out[4] = c[-1];         out[5] = c[-HY_LW - 1]; out[6] = c[-HY_LW];  out[7] = c[-HY_LW + 1];
}

// the tile is dirty in this pass?  Its entry is cleared for the pass after the next.  Every thread of the block calls.
__device__ inline bool hydro_take_tile(const HydroPass &p, int64_t tile, int *s_flag) {
    if (threadIdx.x == 0) { *s_flag = p.cur[tile]; p.cur[tile] = 0; }
    __syncthreads();
    const bool dirty = *s_flag != 0;
    __syncthreads();                                   // before thread 0 writes the flag of the next tile
    return dirty;
}

// the tiles this block solved in the launch, for mhs_hydro_info: one add per block
__device__ inline void hydro_count_solves(const HydroPass &p, unsigned n_solved) {
    if (threadIdx.x == 0 && n_solved) atomicAdd(&p.counters[HC_SOLVES], (unsigned long long)n_solved);
}

// `sides` of the tile changed: mark the neighbouring tiles that see them and count the tile as changed.  One thread calls.
__device__ inline void hydro_mark(const HydroGeom &g, const HydroPass &p, int64_t tile, unsigned sides) {
    if (!sides) return;
    const int ty = (int)(tile / g.tiles_x), tx = (int)(tile % g.tiles_x);
    bool any = false;
    for (int k = 0; k < 8; ++k) {
        const int dr = hydro_dr(k), dc = hydro_dc(k);
        const int ny = ty + dr, nx = tx + dc;
        if (ny < 0 || ny >= g.tiles_y || nx < 0 || nx >= g.tiles_x) continue;
        const bool rows = dr == 0 || (sides & (dr < 0 ? HS_NORTH : HS_SOUTH));
        const bool cols = dc == 0 || (sides & (dc < 0 ? HS_WEST : HS_EAST));
        if (rows && cols) { p.nxt[(int64_t)ny * g.tiles_x + nx] = 1; any = true; }
    }
    if (any) atomicAdd(&p.counters[HC_CHANGE], 1ull);
}

// the sides on which the cell of tile row lr, tile column lane, raster row `row` lies
__device__ inline unsigned hydro_sides(const HydroGeom &g, int lr, int lane, int row, int col) {
    return (lr == 0 ? HS_NORTH : 0u) | ((lr == HY_TH - 1 || row == g.nrow - 1) ? HS_SOUTH : 0u) | (lane == 0 ? HS_WEST : 0u) |
           ((lane == HY_TW - 1 || col == g.ncol - 1) ? HS_EAST : 0u);
}

// W = z at outlets, +inf at the other valid cells, NaN at NA cells; the flags plane
template <typename T>
__global__ __launch_bounds__(HY_NT) void hydro_init_kernel(const HydroGeom g, const T *__restrict__ z, const int64_t ldz,
                                                           double *__restrict__ W, unsigned char *__restrict__ flags) {
    __shared__ double sm[HY_LH * HY_LW];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool has_nd = g.has_nodata != 0;
    for (int64_t tile = blockIdx.x; tile < g.n_tiles; tile += gridDim.x) {
        const int tr0 = (int)(tile / g.tiles_x) * HY_TH, tc0 = (int)(tile % g.tiles_x) * HY_TW;
        for (int lr = wave; lr < HY_LH; lr += 4) {                  // the plane's own type and ld: converted as it is staged
            const int ar = tr0 - 1 + lr;
            const bool rin = ar >= 0 && ar < g.nrow;
            for (int lc = lane; lc < HY_LW; lc += 64) {
                const int ac = tc0 - 1 + lc;
                double v = NAN;
                if (rin && ac >= 0 && ac < g.ncol) {
                    v = (double)z[(int64_t)ar * ldz + ac];
                    if (terrain_na(v, has_nd, g.nodata)) v = NAN;
                }
                sm[lr * HY_LW + lc] = v;
            }
        }
        __syncthreads();
        const int col = tc0 + lane;
        if (col < g.ncol) {
            for (int j = 0; j < HY_ROWS; ++j) {
                const int lr = wave * HY_ROWS + j, row = tr0 + lr;
                if (row >= g.nrow) break;
                const double *c = sm + (lr + 1) * HY_LW + lane + 1;
                const double e = *c;
                double zn[8];
                hydro_gather(c, zn);
                const bool valid = e == e, outlet = valid && hydro_outlet(zn);
                const int64_t idx = (int64_t)row * g.ncol + col;
                W[idx] = !valid ? (double)NAN : outlet ? e : (double)INFINITY;
                flags[idx] = (unsigned char)((valid ? HF_VALID : 0) | (outlet ? HF_OUTLET : 0));
            }
        }
        __syncthreads();
    }
}

// SOLVE 1: W(c) = max(z(c), min W(k)) at the valid cells that are no outlets, from above
template <typename T>
__global__ __launch_bounds__(HY_NT) void hydro_fill_kernel(const HydroGeom g, const T *__restrict__ z, const int64_t ldz, double *W,
                                                           unsigned char *flags, const HydroPass p) {
    __shared__ double sm[HY_LH * HY_LW];
    __shared__ int s_flag;
    __shared__ unsigned s_sides;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned n_solved = 0;
    for (int64_t tile = blockIdx.x; tile < g.n_tiles; tile += gridDim.x) {
        if (!hydro_take_tile(p, tile, &s_flag)) continue;
        ++n_solved;
        const int tr0 = (int)(tile / g.tiles_x) * HY_TH, tc0 = (int)(tile % g.tiles_x) * HY_TW;
        hydro_stage<double>(g, sm, W, tr0, tc0, (double)NAN);
        if (threadIdx.x == 0) s_sides = 0;
        __syncthreads();
        const int col = tc0 + lane, lr0 = wave * HY_ROWS;
        double *c0 = sm + (lr0 + 1) * HY_LW + lane + 1;
        double zc[HY_ROWS], w[HY_ROWS], w0[HY_ROWS];
        unsigned char fl[HY_ROWS];
        unsigned act = 0;                                           // bit j: cell j is stepped
#pragma unroll
        for (int j = 0; j < HY_ROWS; ++j) {
            const int row = tr0 + lr0 + j;
            zc[j] = 0.0; fl[j] = 0;
            w[j] = w0[j] = c0[j * HY_LW];
            if (col < g.ncol && row < g.nrow) {
                fl[j] = flags[(int64_t)row * g.ncol + col];
                if (fl[j] & HF_VALID) zc[j] = (double)z[(int64_t)row * ldz + col];
                if ((fl[j] & (HF_VALID | HF_OUTLET)) == HF_VALID) act |= 1u << j;
            }
        }
        for (int sweep = 0; sweep < HY_MAX_SWEEPS; ++sweep) {
            int changed = 0;
#pragma unroll
            for (int j = 0; j < HY_ROWS; ++j) {
                if (!(act & (1u << j))) continue;
                double wn[8];
                hydro_gather(c0 + j * HY_LW, wn);
                const double nw = hydro_fill_step(zc[j], wn);
                if (nw < w[j]) { w[j] = nw; c0[j * HY_LW] = nw; changed = 1; }
            }
            if (!__syncthreads_or(changed)) break;
        }
        unsigned sides = 0;
#pragma unroll
        for (int j = 0; j < HY_ROWS; ++j) {
            const int row = tr0 + lr0 + j;
            if (!(col < g.ncol && row < g.nrow) || !(fl[j] & HF_VALID)) continue;
            const int64_t idx = (int64_t)row * g.ncol + col;
            if (w[j] != w0[j]) { W[idx] = w[j]; sides |= hydro_sides(g, lr0 + j, lane, row, col); }
            const unsigned char nf = (unsigned char)((fl[j] & (HF_VALID | HF_OUTLET)) | (w[j] > zc[j] ? HF_RAISED : 0));
            if (nf != fl[j]) flags[idx] = nf;
        }
        if (sides) atomicOr(&s_sides, sides);
        __syncthreads();
        if (threadIdx.x == 0) hydro_mark(g, p, tile, s_sides);
        __syncthreads();
    }
    hydro_count_solves(p, n_solved);
}

// the seeds of D: 0 at outlets and at cells with a strictly lower neighbour, HYDRO_D_INF at the other valid cells
__global__ __launch_bounds__(HY_NT) void hydro_seed_kernel(const HydroGeom g, const double *__restrict__ W,
                                                           const unsigned char *__restrict__ flags, int32_t *__restrict__ D) {
    __shared__ double sm[HY_LH * HY_LW];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t tile = blockIdx.x; tile < g.n_tiles; tile += gridDim.x) {
        const int tr0 = (int)(tile / g.tiles_x) * HY_TH, tc0 = (int)(tile % g.tiles_x) * HY_TW;
        hydro_stage<double>(g, sm, W, tr0, tc0, (double)NAN);
        __syncthreads();
        const int col = tc0 + lane;
        if (col < g.ncol) {
            for (int j = 0; j < HY_ROWS; ++j) {
                const int lr = wave * HY_ROWS + j, row = tr0 + lr;
                if (row >= g.nrow) break;
                const double *c = sm + (lr + 1) * HY_LW + lane + 1;
                double wn[8];
                hydro_gather(c, wn);
                const int64_t idx = (int64_t)row * g.ncol + col;
                const unsigned char f = flags[idx];
                D[idx] = (!(f & HF_VALID) || (f & HF_OUTLET) || hydro_has_lower(*c, wn)) ? 0 : HYDRO_D_INF;
            }
        }
        __syncthreads();
    }
}

// SOLVE 2: D(c) = 1 + min D(k) over the neighbours of equal W, at the valid cells that are no seeds, from above
__global__ __launch_bounds__(HY_NT) void hydro_flat_kernel(const HydroGeom g, const double *__restrict__ W, int32_t *D, const HydroPass p) {
    __shared__ double sw[HY_LH * HY_LW];
    __shared__ int32_t sd[HY_LH * HY_LW];
    __shared__ int s_flag;
    __shared__ unsigned s_sides;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned n_solved = 0;
    for (int64_t tile = blockIdx.x; tile < g.n_tiles; tile += gridDim.x) {
        if (!hydro_take_tile(p, tile, &s_flag)) continue;
        ++n_solved;
        const int tr0 = (int)(tile / g.tiles_x) * HY_TH, tc0 = (int)(tile % g.tiles_x) * HY_TW;
        hydro_stage<double>(g, sw, W, tr0, tc0, (double)NAN);
        hydro_stage<int32_t>(g, sd, D, tr0, tc0, HYDRO_D_INF);
        if (threadIdx.x == 0) s_sides = 0;
        __syncthreads();
        const int col = tc0 + lane, lr0 = wave * HY_ROWS;
        const double *w0p = sw + (lr0 + 1) * HY_LW + lane + 1;
        int32_t *d0p = sd + (lr0 + 1) * HY_LW + lane + 1;
        int32_t d[HY_ROWS], d0[HY_ROWS];
        unsigned act = 0;
#pragma unroll
        for (int j = 0; j < HY_ROWS; ++j) {
            const int row = tr0 + lr0 + j;
            d[j] = d0[j] = d0p[j * HY_LW];
            const double wc = w0p[j * HY_LW];
            if (col < g.ncol && row < g.nrow && wc == wc && d[j] != 0) act |= 1u << j;      // a seed stays 0
        }
        for (int sweep = 0; sweep < HY_MAX_SWEEPS; ++sweep) {
            int changed = 0;
#pragma unroll
            for (int j = 0; j < HY_ROWS; ++j) {
                if (!(act & (1u << j))) continue;
                double wn[8];
                int32_t dn[8];
                hydro_gather(w0p + j * HY_LW, wn);
                hydro_gather<int32_t>(d0p + j * HY_LW, dn);
                const int32_t nd = hydro_flat_step(w0p[j * HY_LW], wn, dn);
                if (nd < d[j]) { d[j] = nd; d0p[j * HY_LW] = nd; changed = 1; }
            }
            if (!__syncthreads_or(changed)) break;
        }
        unsigned sides = 0;
#pragma unroll
        for (int j = 0; j < HY_ROWS; ++j) {
            const int row = tr0 + lr0 + j;
            if (!(act & (1u << j)) || d[j] == d0[j]) continue;
            D[(int64_t)row * g.ncol + col] = d[j];
            sides |= hydro_sides(g, lr0 + j, lane, row, col);
        }
        if (sides) atomicOr(&s_sides, sides);
        __syncthreads();
        if (threadIdx.x == 0) hydro_mark(g, p, tile, s_sides);
        __syncthreads();
    }
    hydro_count_solves(p, n_solved);
}

// the direction of every cell, A = 1 at the valid cells (NaN at NA cells), and the counts of mhs_hydro_info
__global__ __launch_bounds__(HY_NT) void hydro_dir_kernel(const HydroGeom g, const double *__restrict__ W, const int32_t *__restrict__ D,
                                                          const unsigned char *__restrict__ flags, signed char *__restrict__ dir,
                                                          double *__restrict__ A, unsigned long long *counters) {
    __shared__ double sw[HY_LH * HY_LW];
    __shared__ int32_t sd[HY_LH * HY_LW];
    __shared__ unsigned s_count[3];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x < 3) s_count[threadIdx.x] = 0;
    __syncthreads();
    unsigned n_valid = 0, n_raised = 0, n_sinks = 0;              // a thread sees at most 8 cells of each of its tiles
    for (int64_t tile = blockIdx.x; tile < g.n_tiles; tile += gridDim.x) {
        const int tr0 = (int)(tile / g.tiles_x) * HY_TH, tc0 = (int)(tile % g.tiles_x) * HY_TW;
        hydro_stage<double>(g, sw, W, tr0, tc0, (double)NAN);
        hydro_stage<int32_t>(g, sd, D, tr0, tc0, HYDRO_D_INF);
        __syncthreads();
        const int col = tc0 + lane;
        if (col < g.ncol) {
            for (int j = 0; j < HY_ROWS; ++j) {
                const int lr = wave * HY_ROWS + j, row = tr0 + lr;
                if (row >= g.nrow) break;
                const int off = (lr + 1) * HY_LW + lane + 1;
                const int64_t idx = (int64_t)row * g.ncol + col;
                const double wc = sw[off];
                int8_t k = HYDRO_DIR_NA;
                if (wc == wc) {
                    double wn[8];
                    int32_t dn[8];
                    hydro_gather(sw + off, wn);
                    hydro_gather<int32_t>(sd + off, dn);
                    k = hydro_direction(wc, sd[off], wn, dn, g.dx_row ? g.dx_row[row] : g.dx, g.dy);
                    ++n_valid;
                    n_raised += (flags[idx] & HF_RAISED) != 0;
                    n_sinks += k == HYDRO_DIR_OUT;
                }
                dir[idx] = k;
                A[idx] = wc == wc ? 1.0 : (double)NAN;
            }
        }
        __syncthreads();
    }
    if (n_valid) atomicAdd(&s_count[0], n_valid);                 // a block's tiles hold fewer than 2^32 cells: 2^21 tiles each
    if (n_raised) atomicAdd(&s_count[1], n_raised);
    if (n_sinks) atomicAdd(&s_count[2], n_sinks);
    __syncthreads();
    if (threadIdx.x < 3 && s_count[threadIdx.x]) atomicAdd(&counters[HC_VALID + threadIdx.x], (unsigned long long)s_count[threadIdx.x]);
}

// SOLVE 3: A(c) = 1 + the A of the neighbours that point at c, from below
__global__ __launch_bounds__(HY_NT) void hydro_acc_kernel(const HydroGeom g, const signed char *__restrict__ dir, double *A, const HydroPass p) {
    __shared__ double sa[HY_LH * HY_LW];
    __shared__ signed char sdir[HY_LH * HY_LW];
    __shared__ int s_flag;
    __shared__ unsigned s_sides;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned n_solved = 0;
    for (int64_t tile = blockIdx.x; tile < g.n_tiles; tile += gridDim.x) {
        if (!hydro_take_tile(p, tile, &s_flag)) continue;
        ++n_solved;
        const int tr0 = (int)(tile / g.tiles_x) * HY_TH, tc0 = (int)(tile % g.tiles_x) * HY_TW;
        hydro_stage<double>(g, sa, A, tr0, tc0, (double)NAN);
        hydro_stage<signed char>(g, sdir, dir, tr0, tc0, (signed char)HYDRO_DIR_NA);
        if (threadIdx.x == 0) s_sides = 0;
        __syncthreads();
        const int col = tc0 + lane, lr0 = wave * HY_ROWS;
        double *a0p = sa + (lr0 + 1) * HY_LW + lane + 1;
        const signed char *k0p = sdir + (lr0 + 1) * HY_LW + lane + 1;
        double a[HY_ROWS], a0[HY_ROWS];
        unsigned donors[HY_ROWS];                                   // bit k: neighbour k points at the cell
        unsigned act = 0;
#pragma unroll
        for (int j = 0; j < HY_ROWS; ++j) {
            const int row = tr0 + lr0 + j;
            a[j] = a0[j] = a0p[j * HY_LW];
            int8_t kn[8];
            hydro_gather<int8_t>(k0p + j * HY_LW, kn);
            donors[j] = hydro_donors(kn);
            if (col < g.ncol && row < g.nrow && k0p[j * HY_LW] != HYDRO_DIR_NA && donors[j]) act |= 1u << j;
        }
        for (int sweep = 0; sweep < HY_MAX_SWEEPS; ++sweep) {
            int changed = 0;
#pragma unroll
            for (int j = 0; j < HY_ROWS; ++j) {
                if (!(act & (1u << j))) continue;
                double an[8];
                hydro_gather(a0p + j * HY_LW, an);
                const double na = hydro_acc_step(donors[j], an);
                if (na > a[j]) { a[j] = na; a0p[j * HY_LW] = na; changed = 1; }
            }
            if (!__syncthreads_or(changed)) break;
        }
        unsigned sides = 0;
#pragma unroll
        for (int j = 0; j < HY_ROWS; ++j) {
            const int row = tr0 + lr0 + j;
            if (!(act & (1u << j)) || a[j] == a0[j]) continue;
            A[(int64_t)row * g.ncol + col] = a[j];
            sides |= hydro_sides(g, lr0 + j, lane, row, col);
        }
        if (sides) atomicOr(&s_sides, sides);
        __syncthreads();
        if (threadIdx.x == 0) hydro_mark(g, p, tile, s_sides);
        __syncthreads();
    }
    hydro_count_solves(p, n_solved);
}

// MFD: the shares of every valid cell, each stored into its receiver's slot of F (zeroed before: plane k of F holds the share
// neighbour k sends to the cell, so the donor writes plane (k + 4) & 7 of its neighbour k -- a slot has one writer); A = 1 at
// the valid cells (NaN at NA cells), and the counts of mhs_hydro_info.  A positive share goes to a neighbour with a W that is
// no NaN: a cell of the raster.
__global__ __launch_bounds__(HY_NT) void hydro_shares_kernel(const HydroGeom g, const double *__restrict__ W, const int32_t *__restrict__ D,
                                                             const unsigned char *__restrict__ flags, const double exponent,
                                                             double *__restrict__ F, double *__restrict__ A, unsigned long long *counters) {
    __shared__ double sw[HY_LH * HY_LW];
    __shared__ int32_t sd[HY_LH * HY_LW];
    __shared__ unsigned s_count[3];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t n = (int64_t)g.nrow * g.ncol;
    if (threadIdx.x < 3) s_count[threadIdx.x] = 0;
    __syncthreads();
    unsigned n_valid = 0, n_raised = 0, n_sinks = 0;
    for (int64_t tile = blockIdx.x; tile < g.n_tiles; tile += gridDim.x) {
        const int tr0 = (int)(tile / g.tiles_x) * HY_TH, tc0 = (int)(tile % g.tiles_x) * HY_TW;
        hydro_stage<double>(g, sw, W, tr0, tc0, (double)NAN);
        hydro_stage<int32_t>(g, sd, D, tr0, tc0, HYDRO_D_INF);
        __syncthreads();
        const int col = tc0 + lane;
        if (col < g.ncol) {
            for (int j = 0; j < HY_ROWS; ++j) {
                const int lr = wave * HY_ROWS + j, row = tr0 + lr;
                if (row >= g.nrow) break;
                const int off = (lr + 1) * HY_LW + lane + 1;
                const int64_t idx = (int64_t)row * g.ncol + col;
                const double wc = sw[off];
                if (wc == wc) {
                    double wn[8], f[8];
                    int32_t dn[8];
                    hydro_gather(sw + off, wn);
                    hydro_gather<int32_t>(sd + off, dn);
                    const bool any = hydro_mfd_shares(wc, sd[off], wn, dn, g.dx_row ? g.dx_row[row] : g.dx, g.dy, exponent, f);
                    ++n_valid;
                    n_raised += (flags[idx] & HF_RAISED) != 0;
                    n_sinks += !any;
                    if (any) {
                        for (int k = 0; k < 8; ++k) {
                            const int rr = row + hydro_dr(k), cc = col + hydro_dc(k);
                            if (f[k] > 0.0 && rr >= 0 && rr < g.nrow && cc >= 0 && cc < g.ncol)
                                F[(int64_t)((k + 4) & 7) * n + (int64_t)rr * g.ncol + cc] = f[k];
                        }
                    }
                }
                A[idx] = wc == wc ? 1.0 : (double)NAN;
            }
        }
        __syncthreads();
    }
    if (n_valid) atomicAdd(&s_count[0], n_valid);
    if (n_raised) atomicAdd(&s_count[1], n_raised);
    if (n_sinks) atomicAdd(&s_count[2], n_sinks);
    __syncthreads();
    if (threadIdx.x < 3 && s_count[threadIdx.x]) atomicAdd(&counters[HC_VALID + threadIdx.x], (unsigned long long)s_count[threadIdx.x]);
}

// SOLVE 4 (MFD): A(c) = 1 + sum over k of F_k(c) A(k), from below.  A lane holds the eight incoming shares of each of its
// eight cells in registers (64 doubles), loaded once per tile solve; the sweeps read only A, from LDS.
__global__ __launch_bounds__(HY_NT) void hydro_mfd_kernel(const HydroGeom g, const double *__restrict__ F, double *A, const HydroPass p) {
    __shared__ double sa[HY_LH * HY_LW];
    __shared__ int s_flag;
    __shared__ unsigned s_sides;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t n = (int64_t)g.nrow * g.ncol;
    unsigned n_solved = 0;
    for (int64_t tile = blockIdx.x; tile < g.n_tiles; tile += gridDim.x) {
        if (!hydro_take_tile(p, tile, &s_flag)) continue;
        ++n_solved;
        const int tr0 = (int)(tile / g.tiles_x) * HY_TH, tc0 = (int)(tile % g.tiles_x) * HY_TW;
        hydro_stage<double>(g, sa, A, tr0, tc0, (double)NAN);
        if (threadIdx.x == 0) s_sides = 0;
        const int col = tc0 + lane, lr0 = wave * HY_ROWS;
        double fin[HY_ROWS][8];
        unsigned act = 0;
#pragma unroll
        for (int j = 0; j < HY_ROWS; ++j) {
            const int row = tr0 + lr0 + j;
            const bool in = col < g.ncol && row < g.nrow;
            const int64_t idx = in ? (int64_t)row * g.ncol + col : 0;
            bool any = false;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                fin[j][k] = in ? F[(int64_t)k * n + idx] : 0.0;
                any |= fin[j][k] > 0.0;
            }
            if (any) act |= 1u << j;                                // a cell with a donor is valid: only valid cells receive
        }
        __syncthreads();
        double *a0p = sa + (lr0 + 1) * HY_LW + lane + 1;
        double a[HY_ROWS], a0[HY_ROWS];
#pragma unroll
        for (int j = 0; j < HY_ROWS; ++j) a[j] = a0[j] = a0p[j * HY_LW];
        for (int sweep = 0; sweep < HY_MAX_SWEEPS; ++sweep) {
            int changed = 0;
#pragma unroll
            for (int j = 0; j < HY_ROWS; ++j) {
                if (!(act & (1u << j))) continue;
                double an[8];
                hydro_gather(a0p + j * HY_LW, an);
                const double na = hydro_mfd_step(fin[j], an);
                if (na > a[j]) { a[j] = na; a0p[j * HY_LW] = na; changed = 1; }
            }
            if (!__syncthreads_or(changed)) break;
        }
        unsigned sides = 0;
#pragma unroll
        for (int j = 0; j < HY_ROWS; ++j) {
            const int row = tr0 + lr0 + j;
            if (!(act & (1u << j)) || a[j] == a0[j]) continue;
            A[(int64_t)row * g.ncol + col] = a[j];
            sides |= hydro_sides(g, lr0 + j, lane, row, col);
        }
        if (sides) atomicOr(&s_sides, sides);
        __syncthreads();
        if (threadIdx.x == 0) hydro_mark(g, p, tile, s_sides);
        __syncthreads();
    }
    hydro_count_solves(p, n_solved);
}

// the requested planes: filled, flowdir, flowacc, twi.  The nine W values slide down the column as in terrain3_kernel.
template <typename O>
__global__ __launch_bounds__(HY_NT) void hydro_emit_kernel(const HydroGeom g, const double *__restrict__ W, const signed char *__restrict__ dir,
                                                           const double *__restrict__ A, const double min_slope_tan, O *__restrict__ filled,
                                                           signed char *__restrict__ flowdir, O *__restrict__ flowacc, O *__restrict__ twi,
                                                           const int64_t ld) {
    __shared__ double sm[HY_LH * HY_LW];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t tile = blockIdx.x; tile < g.n_tiles; tile += gridDim.x) {
        const int tr0 = (int)(tile / g.tiles_x) * HY_TH, tc0 = (int)(tile % g.tiles_x) * HY_TW;
        hydro_stage<double>(g, sm, W, tr0, tc0, (double)NAN);
        __syncthreads();
        const int col = tc0 + lane;
        if (col < g.ncol) {
            const int lr0 = wave * HY_ROWS;                        // LDS row lr0 + j holds the row NORTH of tile row lr0 + j
            double w9[9];
            bool na_n, na_c, na_s;
            auto load_row = [&](int lr, double *dst) -> bool {
                bool na = false;
                for (int k = 0; k < 3; ++k) {
                    dst[k] = sm[lr * HY_LW + lane + k];
                    na |= dst[k] != dst[k];
                }
                return na;
            };
            na_c = load_row(lr0, w9 + 3);
            na_s = load_row(lr0 + 1, w9 + 6);
#pragma unroll
            for (int j = 0; j < HY_ROWS; ++j) {
                const int row = tr0 + lr0 + j;
                for (int k = 0; k < 6; ++k) w9[k] = w9[k + 3];
                na_n = na_c; na_c = na_s;
                na_s = load_row(lr0 + j + 2, w9 + 6);
                if (row >= g.nrow) break;
                const int64_t idx = (int64_t)row * g.ncol + col, odx = (int64_t)row * ld + col;
                const double acc = A[idx];
                if (filled) filled[odx] = (O)w9[4];
                if (flowdir) flowdir[odx] = dir[idx];
                if (flowacc) flowacc[odx] = (O)acc;
                if (twi) {
                    const bool na = na_n | na_c | na_s;
                    const double dx = g.dx_row ? g.dx_row[row] : g.dx;
                    twi[odx] = (O)(na ? (double)NAN : hydro_twi(w9, acc, dx, g.dy, g.zf, min_slope_tan));
                }
            }
        }
        __syncthreads();
    }
}

static unsigned hydro_blocks(int64_t n_tiles) {
    const int n_cu = ctx().n_cu > 0 ? ctx().n_cu : 256;
    return (unsigned)std::min<int64_t>(n_tiles, (int64_t)n_cu * 32);
}

#define HY_REQUIRE(cond, ...)                                              \
    do {                                                                   \
        if (!(cond)) { set_error(__VA_ARGS__); return MHS_ERR_INVALID; }    \
    } while (0)

// Every check of a hydrology call, before any device call; fn = the entry point's name for the message.  out = the call's
// output struct, n_out of whose planes are named (`fields` lists them for the message); per_cell = the route's scratch bytes
static int hydro_check(const char *fn, int per_cell, const mhs_grid *grid, const mhs_stack *dem, int layer, const mhs_terrain_units *u,
                       double min_slope_tan, int max_passes, const void *out, int n_out, const char *fields, int out_dtype, int64_t ld,
                       HydroGeom *g) {
    HY_REQUIRE(grid && dem && u, "%s: NULL argument (grid, dem or units)", fn);
    HY_REQUIRE(grid->nrow > 0 && grid->ncol > 0 && grid->nrow < (1LL << 30) && grid->ncol < (1LL << 30), "%s: bad grid geometry (nrow, ncol must be in 1 .. 2^30)", fn);
    HY_REQUIRE(grid->nrow * grid->ncol <= HY_MAX_CELLS, "%s: too many cells (nrow * ncol must not pass 2^56: the scratch planes take %d bytes per cell)", fn, per_cell);
    HY_REQUIRE(dem->data, "%s: dem data is NULL", fn);
    HY_REQUIRE(dem->dtype == MHS_F64 || dem->dtype == MHS_F32 || dem->dtype == MHS_I16, "%s: bad dem dtype", fn);
    HY_REQUIRE(layer >= 0 && layer < dem->n_layers, "%s: layer %d is not one of the stack's %d layers", fn, layer, dem->n_layers);
    HY_REQUIRE(dem->ld >= grid->ncol && (dem->n_layers == 1 || dem->plane_stride >= dem->ld * (grid->nrow - 1) + grid->ncol),
               "%s: dem strides smaller than the grid", fn);
    HY_REQUIRE(std::isfinite(u->z_factor) && u->z_factor > 0.0, "%s: z_factor must be finite and positive", fn);
    HY_REQUIRE(std::isfinite(u->dy) && u->dy > 0.0, "%s: dy must be finite and positive", fn);
    if (u->dx_row) {
        for (int64_t r = 0; r < grid->nrow; ++r)
            HY_REQUIRE(std::isfinite(u->dx_row[r]) && u->dx_row[r] > 0.0, "%s: dx_row[%lld] must be finite and positive", fn, (long long)r);
    } else HY_REQUIRE(std::isfinite(u->dx) && u->dx > 0.0, "%s: dx must be finite and positive (or give dx_row)", fn);
    HY_REQUIRE(std::isfinite(min_slope_tan) && min_slope_tan > 0.0, "%s: min_slope_tan must be finite and positive", fn);
    HY_REQUIRE(max_passes >= 0, "%s: max_passes must not be negative (0 = the default cap)", fn);
    HY_REQUIRE(out, "%s: out is NULL", fn);
    HY_REQUIRE(n_out > 0, "%s: out names no plane (%s are all NULL)", fn, fields);
    HY_REQUIRE(out_dtype == MHS_F64 || out_dtype == MHS_F32, "%s: out_dtype must be MHS_F64 or MHS_F32", fn);
    HY_REQUIRE(ld >= grid->ncol, "%s: ld smaller than the grid width", fn);
    const int tiles_x = (int)((grid->ncol + HY_TW - 1) / HY_TW), tiles_y = (int)((grid->nrow + HY_TH - 1) / HY_TH);
    *g = HydroGeom{(int)grid->nrow, (int)grid->ncol, tiles_x, tiles_y, (int64_t)tiles_x * tiles_y, dem->nodata, !std::isnan(dem->nodata),
                   nullptr, u->dx, u->dy, u->z_factor};
    return MHS_OK;
}

// the call's one block of stream-ordered memory, given back behind whatever was enqueued last
struct HydroScratch {
    char *p = nullptr;
    hipStream_t st = nullptr;
    ~HydroScratch() { if (p) (void)hipFreeAsync(p, st); }
};

static size_t hy_align(size_t n) { return (n + 255) & ~(size_t)255; }

template <typename T>
static void launch_hydro_init(const HydroGeom &g, unsigned nb, hipStream_t st, const void *z, int64_t ldz, double *W, unsigned char *flags) {
    hipLaunchKernelGGL((hydro_init_kernel<T>), dim3(nb), dim3(HY_NT), 0, st, g, (const T *)z, ldz, W, flags);
}
template <typename T>
static void launch_hydro_fill(const HydroGeom &g, unsigned nb, hipStream_t st, const void *z, int64_t ldz, double *W, unsigned char *flags,
                              const HydroPass &p) {
    hipLaunchKernelGGL((hydro_fill_kernel<T>), dim3(nb), dim3(HY_NT), 0, st, g, (const T *)z, ldz, W, flags, p);
}
template <typename O>
static void launch_hydro_emit(const HydroGeom &g, unsigned nb, hipStream_t st, const double *W, const signed char *dir, const double *A,
                              double min_slope_tan, const mhs_hydro_out &out, int64_t ld) {
    hipLaunchKernelGGL((hydro_emit_kernel<O>), dim3(nb), dim3(HY_NT), 0, st, g, W, dir, A, min_slope_tan, (O *)out.filled,
                       (signed char *)out.flowdir, (O *)out.flowacc, (O *)out.twi, ld);
}

// One call on device planes: its block of scratch, the pass loop of a phase and the records of mhs_hydro_info -- what the D8
// and the MFD route share.  The host loop of every phase synchronises `st` once per pass.
struct HydroWork {
    const char *fn;
    HydroGeom g;
    hipStream_t st;
    HydroScratch s;
    double *W = nullptr, *A = nullptr, *F = nullptr;       // F: the MFD route's eight incoming-share planes
    int32_t *D = nullptr;
    signed char *dir = nullptr;                            // the D8 route's directions
    unsigned char *flags = nullptr, *dirty = nullptr;
    unsigned long long *counters = nullptr;
    size_t n = 0, nt = 0;
    unsigned nb = 0;
    int cap = 0;
    int passes[3] = {0, 0, 0};
    double ms[3] = {0.0, 0.0, 0.0}, t0 = 0.0;
    long long solves[3] = {0, 0, 0};
    unsigned long long solved = 0;           // the count of tile solves runs on through the three phases ...
    unsigned long long seen = 0;             // ... and so does the change counter

    // the scratch planes of the route (mfd: F instead of the directions), dx_row on the device, the counters at 0
    int begin(const char *fn_, const HydroGeom &g_, bool mfd, const double *dx_row_host, int max_passes, hipStream_t st_) {
        fn = fn_; g = g_; st = st_;
        n = (size_t)g.nrow * (size_t)g.ncol; nt = (size_t)g.n_tiles;
        const size_t o_w = 0, o_a = o_w + hy_align(8 * n), o_d = o_a + hy_align(8 * n), o_dir = o_d + hy_align(4 * n),
                     o_fl = o_dir + hy_align(mfd ? 64 * n : n), o_dirty = o_fl + hy_align(n), o_cnt = o_dirty + hy_align(2 * nt),
                     o_dx = o_cnt + hy_align(8 * HC_COUNT), total = o_dx + hy_align(dx_row_host ? 8 * (size_t)g.nrow : 0);
        s.st = st;
        if (hipMallocAsync((void **)&s.p, total, st) != hipSuccess) {
            (void)hipGetLastError();
            s.p = nullptr;
            set_error("%s: no device memory for the scratch planes (%zu bytes: %d per cell)", fn, total, mfd ? 85 : 22);
            return MHS_ERR_ALLOC;
        }
        W = (double *)(s.p + o_w); A = (double *)(s.p + o_a);
        D = (int32_t *)(s.p + o_d);
        if (mfd) F = (double *)(s.p + o_dir);
        else dir = (signed char *)(s.p + o_dir);
        flags = (unsigned char *)(s.p + o_fl); dirty = (unsigned char *)(s.p + o_dirty);
        counters = (unsigned long long *)(s.p + o_cnt);
        if (dx_row_host) {
            MHS_HIP(hipMemcpyAsync(s.p + o_dx, dx_row_host, 8 * (size_t)g.nrow, hipMemcpyHostToDevice, st));
            g.dx_row = (const double *)(s.p + o_dx);
        }
        MHS_HIP(hipMemsetAsync(counters, 0, 8 * HC_COUNT, st));
        nb = hydro_blocks(g.n_tiles);
        cap = max_passes > 0 ? max_passes : 16 * (g.tiles_y + g.tiles_x) + 64;
        t0 = now_ms();
        return MHS_OK;
    }

    // passes of one phase until one reports no change: every tile is dirty in the first
    template <typename Launch>
    int solve(int phase, const char *name, Launch &&launch) {
        MHS_HIP(hipMemsetAsync(dirty, 1, nt, st));
        MHS_HIP(hipMemsetAsync(dirty + nt, 0, nt, st));
        unsigned long long c[HC_COUNT];
        for (int pass = 0; pass < cap; ++pass) {
            launch(HydroPass{dirty + (size_t)(pass & 1) * nt, dirty + (size_t)((pass + 1) & 1) * nt, counters});
            MHS_HIP(hipGetLastError());
            MHS_HIP(hipMemcpyAsync(c, counters, 8 * HC_COUNT, hipMemcpyDeviceToHost, st));
            MHS_HIP(hipStreamSynchronize(st));
            passes[phase] = pass + 1;
            solves[phase] = (long long)(c[HC_SOLVES] - solved);
            if (c[HC_CHANGE] == seen) {
                solved = c[HC_SOLVES];
                const double t1 = now_ms();
                ms[phase] = t1 - t0; t0 = t1;
                return MHS_OK;
            }
            seen = c[HC_CHANGE];
        }
        set_error("%s: the %s phase still changed after %d passes (max_passes; 0 = the default, 16 * (tile rows + tile columns) + 64)", fn, name, cap);
        return MHS_ERR_NUMERIC;
    }

    // W and D of the plane whose element (0, 0) is `plane`: init, the fill, the seeds, the flat distance
    int surface(int dtype, const void *plane, int64_t ldz) {
        if (dtype == MHS_F64) launch_hydro_init<double>(g, nb, st, plane, ldz, W, flags);
        else if (dtype == MHS_F32) launch_hydro_init<float>(g, nb, st, plane, ldz, W, flags);
        else launch_hydro_init<short>(g, nb, st, plane, ldz, W, flags);
        MHS_HIP(hipGetLastError());
        int rc = solve(0, "fill", [&](const HydroPass &p) {
            if (dtype == MHS_F64) launch_hydro_fill<double>(g, nb, st, plane, ldz, W, flags, p);
            else if (dtype == MHS_F32) launch_hydro_fill<float>(g, nb, st, plane, ldz, W, flags, p);
            else launch_hydro_fill<short>(g, nb, st, plane, ldz, W, flags, p);
        });
        if (rc) return rc;
        hipLaunchKernelGGL(hydro_seed_kernel, dim3(nb), dim3(HY_NT), 0, st, g, W, flags, D);
        MHS_HIP(hipGetLastError());
        return solve(1, "flat distance", [&](const HydroPass &p) { hipLaunchKernelGGL(hydro_flat_kernel, dim3(nb), dim3(HY_NT), 0, st, g, W, D, p); });
    }

    // the requested planes (dir and out.flowdir may both be NULL) and the call's records
    int emit(double min_slope_tan, const mhs_hydro_out &out, int out_dtype, int64_t ld, mhs_hydro_info *info) {
        if (out_dtype == MHS_F64) launch_hydro_emit<double>(g, nb, st, W, dir, A, min_slope_tan, out, ld);
        else launch_hydro_emit<float>(g, nb, st, W, dir, A, min_slope_tan, out, ld);
        MHS_HIP(hipGetLastError());
        if (info) {
            unsigned long long c[HC_COUNT];
            MHS_HIP(hipMemcpyAsync(c, counters, 8 * HC_COUNT, hipMemcpyDeviceToHost, st));
            MHS_HIP(hipStreamSynchronize(st));
            *info = mhs_hydro_info{passes[0], passes[1], passes[2], (int64_t)c[HC_VALID], (int64_t)c[HC_RAISED], (int64_t)c[HC_SINKS], g.n_tiles,
                                   solves[0], solves[1], solves[2], ms[0], ms[1], ms[2]};
        }
        return MHS_OK;
    }
};

// Device planes, D8.  `plane` = element (0, 0) of the DEM's layer.
static int hydro_run(const char *fn, const HydroGeom &g, int dtype, const void *plane, int64_t ldz, const double *dx_row_host, double min_slope_tan,
                     int max_passes, const mhs_hydro_out &out, int out_dtype, int64_t ld, hipStream_t st, mhs_hydro_info *info) {
    HydroWork w;
    if (int rc = w.begin(fn, g, false, dx_row_host, max_passes, st)) return rc;
    if (int rc = w.surface(dtype, plane, ldz)) return rc;
    hipLaunchKernelGGL(hydro_dir_kernel, dim3(w.nb), dim3(HY_NT), 0, st, w.g, w.W, w.D, w.flags, w.dir, w.A, w.counters);
    MHS_HIP(hipGetLastError());
    if (int rc = w.solve(2, "accumulation", [&](const HydroPass &p) { hipLaunchKernelGGL(hydro_acc_kernel, dim3(w.nb), dim3(HY_NT), 0, st, w.g, w.dir, w.A, p); }))
        return rc;
    return w.emit(min_slope_tan, out, out_dtype, ld, info);
}

// Device planes, MFD: the shares once, then the accumulation over them
static int hydro_mfd_run(const char *fn, const HydroGeom &g, int dtype, const void *plane, int64_t ldz, const double *dx_row_host, double min_slope_tan,
                         int max_passes, double exponent, const mhs_hydro_mfd_out &out, int out_dtype, int64_t ld, hipStream_t st,
                         mhs_hydro_info *info) {
    HydroWork w;
    if (int rc = w.begin(fn, g, true, dx_row_host, max_passes, st)) return rc;
    if (int rc = w.surface(dtype, plane, ldz)) return rc;
    MHS_HIP(hipMemsetAsync(w.F, 0, 64 * w.n, st));                  // no share where no donor writes one
    hipLaunchKernelGGL(hydro_shares_kernel, dim3(w.nb), dim3(HY_NT), 0, st, w.g, w.W, w.D, w.flags, exponent, w.F, w.A, w.counters);
    MHS_HIP(hipGetLastError());
    if (int rc = w.solve(2, "accumulation", [&](const HydroPass &p) { hipLaunchKernelGGL(hydro_mfd_kernel, dim3(w.nb), dim3(HY_NT), 0, st, w.g, w.F, w.A, p); }))
        return rc;
    return w.emit(min_slope_tan, mhs_hydro_out{out.filled, nullptr, out.flowacc, out.twi}, out_dtype, ld, info);
}

// the host entries: the plane goes up, `run` fills the device planes dev[k] (NULL where host[k] is), the planes come down
template <typename Run>
static int hydro_host(const char *fn, const HydroGeom &hg, const mhs_stack *dem, int layer, int n_planes, void *const *host, const size_t *bytes,
                      Run &&run) {
    const size_t esz = dtype_bytes(dem->dtype);
    const size_t in_bytes = ((size_t)(hg.nrow - 1) * dem->ld + hg.ncol) * esz;
    size_t off[4], total = hy_align(in_bytes);
    for (int k = 0; k < n_planes; ++k) { off[k] = total; total += host[k] ? hy_align(bytes[k]) : 0; }
    std::lock_guard<std::mutex> lk(pipe_mutex());
    if (int rc = host_pipe(0)) return rc;                      // the pipeline's streams; its arena is not used
    hipStream_t st = ctx().pipe_comp;
    HydroScratch s;
    s.st = st;
    if (hipMallocAsync((void **)&s.p, total, st) != hipSuccess) {
        (void)hipGetLastError();
        s.p = nullptr;
        set_error("%s: no device memory for the plane and its outputs (%zu bytes)", fn, total);
        return MHS_ERR_ALLOC;
    }
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{st};   // no copy is left in flight, whatever the exit
    const char *src = (const char *)dem->data + (size_t)layer * dem->plane_stride * esz;
    MHS_HIP(hipMemcpyAsync(s.p, src, in_bytes, hipMemcpyHostToDevice, st));
    void *dev[4];
    for (int k = 0; k < n_planes; ++k) dev[k] = host[k] ? s.p + off[k] : nullptr;
    if (int rc = run((const void *)s.p, dev, st)) return rc;
    for (int k = 0; k < n_planes; ++k)
        if (host[k]) MHS_HIP(hipMemcpyAsync(host[k], s.p + off[k], bytes[k], hipMemcpyDeviceToHost, st));
    MHS_HIP(hipStreamSynchronize(st));
    return MHS_OK;
}

static int hydro_mfd_check(const char *fn, const mhs_grid *g, const mhs_stack *dem, int layer, const mhs_terrain_units *units, double min_slope_tan,
                           int max_passes, double exponent, const mhs_hydro_mfd_out *out, int out_dtype, int64_t ld, HydroGeom *hg) {
    if (int rc = hydro_check(fn, 85, g, dem, layer, units, min_slope_tan, max_passes, out, out ? (out->filled != nullptr) + (out->flowacc != nullptr) + (out->twi != nullptr) : 0,
                             "filled, flowacc, twi", out_dtype, ld, hg))
        return rc;
    HY_REQUIRE(std::isfinite(exponent) && exponent > 0.0 && exponent <= HYDRO_MFD_MAX_EXPONENT, "%s: exponent must be finite, above 0 and at most 64", fn);
    return MHS_OK;
}

}  // namespace mhs

using namespace mhs;

extern "C" {

int mhs_hydro_dev(const mhs_grid *g, const mhs_stack *dem, int layer, const mhs_terrain_units *units, double min_slope_tan, int max_passes,
                  const mhs_hydro_out *out, int out_dtype, int64_t ld, void *stream, mhs_hydro_info *info) {
    HydroGeom hg;
    if (int rc = hydro_check(__func__, 22, g, dem, layer, units, min_slope_tan, max_passes, out,
                             out ? (out->filled != nullptr) + (out->flowdir != nullptr) + (out->flowacc != nullptr) + (out->twi != nullptr) : 0,
                             "filled, flowdir, flowacc, twi", out_dtype, ld, &hg))
        return rc;
    if (int rc = require_ready()) return rc;
    const void *plane = (const char *)dem->data + (size_t)layer * dem->plane_stride * dtype_bytes(dem->dtype);
    return hydro_run(__func__, hg, dem->dtype, plane, dem->ld, units->dx_row, min_slope_tan, max_passes, *out, out_dtype, ld, pick_stream(stream), info);
}

// Host planes: the WHOLE plane goes up and the requested planes come down.  No row bands: a cell's fill, direction and
// accumulation depend on cells anywhere in the raster.
int mhs_hydro(const mhs_grid *g, const mhs_stack *dem, int layer, const mhs_terrain_units *units, double min_slope_tan, int max_passes,
              const mhs_hydro_out *out, int out_dtype, mhs_hydro_info *info) {
    HydroGeom hg;
    if (int rc = hydro_check(__func__, 22, g, dem, layer, units, min_slope_tan, max_passes, out,
                             out ? (out->filled != nullptr) + (out->flowdir != nullptr) + (out->flowacc != nullptr) + (out->twi != nullptr) : 0,
                             "filled, flowdir, flowacc, twi", out_dtype, g ? g->ncol : 0, &hg))
        return rc;
    if (int rc = require_ready()) return rc;
    const size_t n = (size_t)hg.nrow * (size_t)hg.ncol, osz = out_dtype == MHS_F64 ? 8 : 4;
    void *const host[4] = {out->filled, out->flowdir, out->flowacc, out->twi};
    const size_t bytes[4] = {n * osz, n, n * osz, n * osz};
    const char *fn = __func__;
    return hydro_host(fn, hg, dem, layer, 4, host, bytes, [&](const void *plane, void *const *dev, hipStream_t st) {
        return hydro_run(fn, hg, dem->dtype, plane, dem->ld, units->dx_row, min_slope_tan, max_passes,
                         mhs_hydro_out{dev[0], (int8_t *)dev[1], dev[2], dev[3]}, out_dtype, hg.ncol, st, info);
    });
}

int mhs_hydro_mfd_dev(const mhs_grid *g, const mhs_stack *dem, int layer, const mhs_terrain_units *units, double min_slope_tan, int max_passes,
                      double exponent, const mhs_hydro_mfd_out *out, int out_dtype, int64_t ld, void *stream, mhs_hydro_info *info) {
    HydroGeom hg;
    if (int rc = hydro_mfd_check(__func__, g, dem, layer, units, min_slope_tan, max_passes, exponent, out, out_dtype, ld, &hg)) return rc;
    if (int rc = require_ready()) return rc;
    const void *plane = (const char *)dem->data + (size_t)layer * dem->plane_stride * dtype_bytes(dem->dtype);
    return hydro_mfd_run(__func__, hg, dem->dtype, plane, dem->ld, units->dx_row, min_slope_tan, max_passes, exponent, *out, out_dtype, ld,
                         pick_stream(stream), info);
}

int mhs_hydro_mfd(const mhs_grid *g, const mhs_stack *dem, int layer, const mhs_terrain_units *units, double min_slope_tan, int max_passes,
                  double exponent, const mhs_hydro_mfd_out *out, int out_dtype, mhs_hydro_info *info) {
    HydroGeom hg;
    if (int rc = hydro_mfd_check(__func__, g, dem, layer, units, min_slope_tan, max_passes, exponent, out, out_dtype, g ? g->ncol : 0, &hg)) return rc;
    if (int rc = require_ready()) return rc;
    const size_t n = (size_t)hg.nrow * (size_t)hg.ncol, osz = out_dtype == MHS_F64 ? 8 : 4;
    void *const host[3] = {out->filled, out->flowacc, out->twi};
    const size_t bytes[3] = {n * osz, n * osz, n * osz};
    const char *fn = __func__;
    return hydro_host(fn, hg, dem, layer, 3, host, bytes, [&](const void *plane, void *const *dev, hipStream_t st) {
        return hydro_mfd_run(fn, hg, dem->dtype, plane, dem->ld, units->dx_row, min_slope_tan, max_passes, exponent,
                             mhs_hydro_mfd_out{dev[0], dev[1], dev[2]}, out_dtype, hg.ncol, st, info);
    });
}

}  // extern "C"
