// Zonal statistics of one layer per zone of an int32 zone plane (include/machisplin_hip.h, section "zonal", states the rule;
// zonal_rule.h holds it).  Every accumulator is an exact integer -- cells, n, S1, the two words of S2, qmin, qmax -- so the
// order in which lanes, waves and workgroups add is free, and every atomic here is an integer atomic.
//
// Every phase is its own launch on the stream, and a kernel boundary is the only ordering between phases: no cross-block flag
// protocol, no spin wait, and every loop has a bound that is evident from the code.  The host decides between launches only
// where it reads back a value of the info (behind phase 1: the quantum and n_zones size the scratch).
//   1   zonal_range_kernel       max|v| over the layer's valid finite cells, max(zone) + 1, the +-Inf cells with a zone: a
//                                grid-stride pass, one set of atomics per workgroup.  Skipped when quantum and n_zones are
//                                given and no info is asked for.
//   2   zonal_accumulate_kernel  the hot path.  A workgroup of four waves takes a STRIP of ZONAL_STRIP_TILES tiles of
//                                32 x 64 cells, one below the other, a wave per row at a time.  A lane is a run head when
//                                its zone differs from its left neighbour's; a segmented wave scan (shuffles) makes the run's
//                                totals, and only the run's last lane leaves the wave: to an open-addressed table of
//                                ZONAL_LDS_SLOTS slots in LDS keyed by zone -- one compare-and-swap claims a key, at most
//                                ZONAL_PROBES probes, 64-bit integer adds and 32-bit min / max LDS atomics -- or, when it finds
//                                no slot, straight to the global table with the same integer atomics (speckled zone
//                                planes).  After a barrier every occupied slot is flushed, one global atomic per accumulator.
//                                The table lives across the strip: a zone that covers the plane receives one flush per
//                                strip on its address, not one per tile.
//   3   zonal_finalise_kernel    a lane per zone slot: the integers become the float64 statistics (zonal_rule.h), into the
//                                dense table and into the scratch arrays that phases 4 and 5 gather from.
//   4   zonal_present_kernel     per block of ZONAL_SCAN_BLOCK zone slots the number of zones with cells > 0,
//       zonal_scan_kernel        the exclusive prefix sum of the blocks' numbers (one workgroup),
//       zonal_rows_kernel        and the compaction: row = the number of present zones before this one.
//   5   zonal_planes_kernel      a lane per cell: its zone's statistics, or its own value against them, in one pass.
// A device flag (a zone >= n_zones, a value that does not fit the quantum) is raised by phase 2 when phase 1 was skipped;
// phases 3 to 5 write nothing when it is set.
//
// Scratch: ONE block of stream-ordered memory for the tables, given back behind the last kernel -- per zone slot 4 + 4 + 8 +
// 8 + 8 + 4 + 4 = 40 bytes of integer accumulators (each only when a requested statistic needs it), 8 per float64 statistic
// that a plane or a present table reads, 4 bytes per ZONAL_SCAN_BLOCK slots, 256-byte alignments -- and the counter block of
// 256 bytes, which has to exist before n_zones is known.  LDS: 11.25 KiB per workgroup of phase 2.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include "ensemble_int.h"
#include "proximity_rule.h"
#include "zonal_int.h"
#include "zonal_rule.h"

namespace mhs {

constexpr int ZN_NT = 256;                   // threads per workgroup of every phase: 4 waves
constexpr int ZN_WAVES = ZN_NT / 64;
constexpr int ZN_PER_THREAD = ZONAL_SCAN_BLOCK / ZN_NT;
static_assert(ZONAL_TILE_COLS == 64, "a wave holds one tile row in its lanes");
static_assert(ZONAL_TILE_ROWS % ZN_WAVES == 0 && ZONAL_SCAN_BLOCK % ZN_NT == 0, "whole rows per wave, whole chunks per block");
static_assert((ZONAL_LDS_SLOTS & (ZONAL_LDS_SLOTS - 1)) == 0 && ZONAL_LDS_SLOTS % ZN_NT == 0, "a power of two, whole slots per thread");
static_assert(MHS_ZONAL_N_STATS == ZONAL_N_STATS, "the header and the rule agree");

// the global table, one array per accumulator; NULL where no requested statistic needs it
struct ZonalTables {
    uint32_t *cells, *n;
    unsigned long long *S1, *L, *H;          // S1 is an int64 added in two's complement
    int *qmin, *qmax;
};
// the finalised float64 statistics that phases 4 and 5 read (bits 1 .. 6); NULL where not needed
struct ZonalFin {
    double *s[7];
};
struct ZonalDense {
    int32_t *zone;
    int64_t *count, *cells;
    double *s[7];                            // bits 1 .. 6 by their number; [0] unused
    int64_t capacity;
};
struct ZonalPlaneOut {
    void *p[ZONAL_N_STATS];
    int64_t ld[ZONAL_N_STATS];
};

__device__ inline unsigned zn_wave_sum(unsigned v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// 1
template <typename T>
__global__ __launch_bounds__(ZN_NT) void zonal_range_kernel(const ZonalGeom g, const T *__restrict__ z, const int64_t ldz,
                                                            const int32_t *__restrict__ zones, const int64_t ldq, ZonalCounters *counters) {
    __shared__ double part_max[ZN_WAVES];
    __shared__ unsigned part_end[ZN_WAVES], part_inf[ZN_WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t n = (int64_t)g.nrow * g.ncol;
    const bool has_nd = g.has_nodata != 0;
    double m = 0.0;
    unsigned end = 0, inf = 0;
    for (int64_t i = (int64_t)blockIdx.x * ZN_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * ZN_NT) {
        const int64_t r = i / g.ncol, c = i - r * g.ncol;
        const int zn = zones[r * ldq + c];
        const double v = (double)z[r * ldz + c];
        if (zn >= 0) end = max(end, (unsigned)zn + 1u);
        if (prox_na(v, has_nd, g.nodata)) continue;
        if (zn_finite(v)) m = fmax(m, fabs(v));
        else if (zn >= 0) ++inf;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        m = fmax(m, __shfl_xor(m, d, 64));
        end = max(end, (unsigned)__shfl_xor((int)end, d, 64));
    }
    inf = zn_wave_sum(inf);
    if (lane == 0) { part_max[wave] = m; part_end[wave] = end; part_inf[wave] = inf; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long f = 0;
        for (int w = 0; w < ZN_WAVES; ++w) { m = fmax(m, part_max[w]); end = max(end, part_end[w]); f += part_inf[w]; }
        if (m > 0.0) atomicMax(&counters->max_abs_bits, (unsigned long long)__double_as_longlong(m));
        if (end) atomicMax(&counters->zones_end, end);
        if (f) atomicAdd(&counters->n_nonfinite, f);
    }
}

// qmin and qmax start at the ends of int32; everything else starts at zero (a memset)
__global__ __launch_bounds__(ZN_NT) void zonal_init_kernel(const unsigned nz, int *__restrict__ qmin, int *__restrict__ qmax) {
    const unsigned i = blockIdx.x * ZN_NT + threadIdx.x;
    if (i >= nz) return;
    if (qmin) qmin[i] = INT32_MAX;
    if (qmax) qmax[i] = INT32_MIN;
}

// one run's (or one LDS slot's) totals
struct ZonalRun {
    unsigned cells, n;
    long long S1;
    unsigned long long L, H;
    int qmin, qmax;
};

// totals to the global table: no-return integer atomics, only the accumulators of `need`, nothing for a zero
__device__ inline void zonal_send(const ZonalTables &t, const unsigned need, const int zn, const ZonalRun &a) {
    if ((need & ZONAL_A_CELLS) && a.cells) atomicAdd(&t.cells[zn], a.cells);
    if (!a.n) return;
    if (need & ZONAL_A_N) atomicAdd(&t.n[zn], a.n);
    if ((need & ZONAL_A_S1) && a.S1) atomicAdd(&t.S1[zn], (unsigned long long)a.S1);
    if (need & ZONAL_A_S2) {
        if (a.L) atomicAdd(&t.L[zn], a.L);
        if (a.H) atomicAdd(&t.H[zn], a.H);
    }
    if (need & ZONAL_A_MIN) atomicMin(&t.qmin[zn], a.qmin);
    if (need & ZONAL_A_MAX) atomicMax(&t.qmax[zn], a.qmax);
}

// 2.  blockIdx.x = strip * tiles_c + tile column; the strip's rows are r_begin .. r_end - 1, `strip_rows` of them at most.
template <typename T>
__global__ __launch_bounds__(ZN_NT) void zonal_accumulate_kernel(const ZonalGeom g, const T *__restrict__ z, const int64_t ldz,
                                                                 const int32_t *__restrict__ zones, const int64_t ldq, const unsigned n_zones,
                                                                 const double quantum, const unsigned need, const int strip_rows,
                                                                 const ZonalTables t, ZonalCounters *counters) {
    __shared__ int key[ZONAL_LDS_SLOTS];
    __shared__ unsigned s_cells[ZONAL_LDS_SLOTS], s_n[ZONAL_LDS_SLOTS];
    __shared__ unsigned long long s_S1[ZONAL_LDS_SLOTS], s_L[ZONAL_LDS_SLOTS], s_H[ZONAL_LDS_SLOTS];
    __shared__ int s_min[ZONAL_LDS_SLOTS], s_max[ZONAL_LDS_SLOTS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int s = threadIdx.x; s < ZONAL_LDS_SLOTS; s += ZN_NT) {
        key[s] = -1;
        s_cells[s] = 0; s_n[s] = 0;
        s_S1[s] = 0; s_L[s] = 0; s_H[s] = 0;
        s_min[s] = INT32_MAX; s_max[s] = INT32_MIN;
    }
    __syncthreads();
    const int c = (int)(blockIdx.x % (unsigned)g.tiles_c) * ZONAL_TILE_COLS + lane;
    const int r_begin = (int)(blockIdx.x / (unsigned)g.tiles_c) * strip_rows;
    const int r_end = (int)min((int64_t)g.nrow, (int64_t)r_begin + strip_rows);
    const bool has_nd = g.has_nodata != 0;
    unsigned in_zone = 0, contrib = 0, inexact = 0, bad = 0;
    for (int r = r_begin + wave; r < r_end; r += ZN_WAVES) {
        int zn = c < g.ncol ? zones[(int64_t)r * ldq + c] : -1;
        if (zn >= 0 && (unsigned)zn >= n_zones) { bad |= ZN_BAD_ZONE; zn = -1; }
        if (__ballot(zn >= 0) == 0) continue;                              // wave-uniform: no cell of this row has a zone
        ZonalRun a{0u, 0u, 0ll, 0ull, 0ull, INT32_MAX, INT32_MIN};
        if (zn >= 0) {
            a.cells = 1;
            ++in_zone;
            const double v = (double)z[(int64_t)r * ldz + c];
            if (!prox_na(v, has_nd, g.nodata) && zn_finite(v)) {
                if (!zonal_fits(v, quantum)) bad |= ZN_BAD_QUANTUM;
                else {
                    const int32_t q = zonal_q(v, quantum);
                    if ((double)q * quantum != v) ++inexact;
                    ++contrib;
                    a.n = 1;
                    a.S1 = q;
                    a.L = zonal_sq_lo(q);
                    a.H = zonal_sq_hi(q);
                    a.qmin = a.qmax = q;
                }
            }
        }
        // the runs of equal zone: `start` = the lane of this lane's run head
        const int left = __shfl_up(zn, 1, 64);
        const uint64_t heads = __ballot(lane == 0 || zn != left);
        const int start = 63 - __builtin_clzll(heads & ((2ull << lane) - 1ull));
        // segmented inclusive scan: after the step of distance d a lane holds the total of the min(2 d, lane - start + 1) lanes up to it
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const bool take = lane - d >= start;
            if (need & ZONAL_A_CELLS) { const unsigned x = __shfl_up(a.cells, d, 64); if (take) a.cells += x; }
            { const unsigned x = __shfl_up(a.n, d, 64); if (take) a.n += x; }
            if (need & ZONAL_A_S1) { const long long x = __shfl_up(a.S1, d, 64); if (take) a.S1 += x; }
            if (need & ZONAL_A_S2) {
                const unsigned long long x = __shfl_up(a.L, d, 64), y = __shfl_up(a.H, d, 64);
                if (take) { a.L += x; a.H += y; }
            }
            if (need & ZONAL_A_MIN) { const int x = __shfl_up(a.qmin, d, 64); if (take) a.qmin = min(a.qmin, x); }
            if (need & ZONAL_A_MAX) { const int x = __shfl_up(a.qmax, d, 64); if (take) a.qmax = max(a.qmax, x); }
        }
        const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
        if (tail && zn >= 0) {                                             // only the run's last lane leaves the wave
            unsigned s = (((unsigned)zn * 0x9E3779B1u) >> 24) & (unsigned)(ZONAL_LDS_SLOTS - 1);
            int slot = -1;
            for (int p = 0; p < ZONAL_PROBES; ++p) {
                const int k = atomicCAS(&key[s], -1, zn);
                if (k == -1 || k == zn) { slot = (int)s; break; }
                s = (s + 1u) & (unsigned)(ZONAL_LDS_SLOTS - 1);
            }
            if (slot < 0) zonal_send(t, need, zn, a);
            else {
                if (need & ZONAL_A_CELLS) atomicAdd(&s_cells[slot], a.cells);
                if (a.n) {
                    atomicAdd(&s_n[slot], a.n);
                    if (need & ZONAL_A_S1) atomicAdd(&s_S1[slot], (unsigned long long)a.S1);
                    if (need & ZONAL_A_S2) { atomicAdd(&s_L[slot], a.L); atomicAdd(&s_H[slot], a.H); }
                    if (need & ZONAL_A_MIN) atomicMin(&s_min[slot], a.qmin);
                    if (need & ZONAL_A_MAX) atomicMax(&s_max[slot], a.qmax);
                }
            }
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < ZONAL_LDS_SLOTS; s += ZN_NT) {
        const int zn = key[s];
        if (zn < 0) continue;
        zonal_send(t, need, zn, ZonalRun{s_cells[s], s_n[s], (long long)s_S1[s], s_L[s], s_H[s], s_min[s], s_max[s]});
    }
    in_zone = zn_wave_sum(in_zone);
    contrib = zn_wave_sum(contrib);
    inexact = zn_wave_sum(inexact);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) bad |= (unsigned)__shfl_xor((int)bad, d, 64);
    if (lane == 0) {
        if (in_zone) atomicAdd(&counters->n_in_zone, (unsigned long long)in_zone);
        if (contrib) atomicAdd(&counters->n_contrib, (unsigned long long)contrib);
        if (inexact) atomicAdd(&counters->n_inexact, (unsigned long long)inexact);
        if (bad) atomicOr(&counters->bad, bad);
    }
}

__device__ inline ZonalAcc zonal_load(const ZonalTables &t, const unsigned i) {
    ZonalAcc a;
    a.cells = t.cells ? t.cells[i] : 0u;
    a.n = t.n ? t.n[i] : 0u;
    a.S1 = t.S1 ? (int64_t)t.S1[i] : 0;
    a.L = t.L ? t.L[i] : 0ull;
    a.H = t.H ? t.H[i] : 0ull;
    a.qmin = t.qmin ? t.qmin[i] : 0;
    a.qmax = t.qmax ? t.qmax[i] : 0;
    return a;
}

// 3.  Statistic k goes to the scratch array f.s[k] and to the dense table's d.s[k]; either may be NULL.
__global__ __launch_bounds__(ZN_NT) void zonal_finalise_kernel(const unsigned nz, const double quantum, const ZonalTables t, const ZonalFin f,
                                                               const ZonalDense d, const ZonalCounters *__restrict__ counters) {
    if (counters->bad) return;
    const unsigned i = blockIdx.x * ZN_NT + threadIdx.x;
    if (i >= nz) return;
    const ZonalAcc a = zonal_load(t, i);
    if (d.count) d.count[i] = (int64_t)a.n;
    if (d.cells) d.cells[i] = (int64_t)a.cells;
    double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (f.s[1] || d.s[1]) v[1] = zonal_sum(a, quantum);
    if (f.s[2] || d.s[2]) v[2] = zonal_mean(a, quantum);
    if (f.s[3] || d.s[3]) v[3] = zonal_sd(a, quantum);
    if (f.s[4] || d.s[4] || f.s[6] || d.s[6]) v[4] = zonal_min(a, quantum);
    if (f.s[5] || d.s[5] || f.s[6] || d.s[6]) v[5] = zonal_max(a, quantum);
    if (f.s[6] || d.s[6]) v[6] = a.n ? v[5] - v[4] : zonal_nan();
#pragma unroll
    for (int k = 1; k < 7; ++k) {
        if (f.s[k]) f.s[k][i] = v[k];
        if (d.s[k]) d.s[k][i] = v[k];
    }
}

// 4, the blocks' numbers of present zones; a workgroup takes blocks blockIdx.x, blockIdx.x + gridDim.x, ...
__global__ __launch_bounds__(ZN_NT) void zonal_present_kernel(const unsigned nz, const unsigned n_blocks, const uint32_t *__restrict__ cells,
                                                              int32_t *__restrict__ block_count, ZonalCounters *counters) {
    __shared__ unsigned part[ZN_WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned long long all = 0;
    for (unsigned b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        unsigned k = 0;
#pragma unroll
        for (int j = 0; j < ZN_PER_THREAD; ++j) {
            const uint64_t i = (uint64_t)b * ZONAL_SCAN_BLOCK + j * ZN_NT + threadIdx.x;
            if (i < nz && cells[i]) ++k;
        }
        k = zn_wave_sum(k);
        if (lane == 0) part[wave] = k;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned s = 0;
            for (int w = 0; w < ZN_WAVES; ++w) s += part[w];
            if (block_count) block_count[b] = (int32_t)s;
            all += s;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && all) atomicAdd(&counters->n_present, all);
}

// 4, one workgroup: block_count becomes its own exclusive prefix sum, chunk by chunk with a carry
__global__ __launch_bounds__(ZN_NT) void zonal_scan_kernel(const unsigned n_blocks, int32_t *block_count) {
    __shared__ int wave_total[ZN_WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int carry = 0;
    for (unsigned base = 0; base < n_blocks; base += ZN_NT) {
        const unsigned i = base + threadIdx.x;
        const int v = i < n_blocks ? block_count[i] : 0;
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int x = __shfl_up(incl, d, 64);
            if (lane >= d) incl += x;
        }
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < ZN_WAVES; ++w) {
            if (w < wave) before += wave_total[w];
            total += wave_total[w];
        }
        if (i < n_blocks) block_count[i] = carry + before + incl - v;
        carry += total;
        __syncthreads();
    }
}

// 4, the rows: zone slots base + q * 64 + lane, q = 0 .. 31, are in zone order
__global__ __launch_bounds__(ZN_NT) void zonal_rows_kernel(const unsigned nz, const ZonalTables t, const ZonalFin f, const int32_t *__restrict__ block_before,
                                                           const ZonalDense d, const ZonalCounters *__restrict__ counters) {
    __shared__ int count[ZN_PER_THREAD * ZN_WAVES];
    if (counters->bad) return;                                             // uniform over the grid
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t base = (uint64_t)blockIdx.x * ZONAL_SCAN_BLOCK;
    uint64_t present[ZN_PER_THREAD];
#pragma unroll
    for (int j = 0; j < ZN_PER_THREAD; ++j) {
        const uint64_t i = base + j * ZN_NT + threadIdx.x;
        present[j] = __ballot(i < nz && t.cells[i] != 0u);
        if (lane == 0) count[j * ZN_WAVES + wave] = __popcll(present[j]);
    }
    __syncthreads();
    const int first = block_before[blockIdx.x];
#pragma unroll
    for (int j = 0; j < ZN_PER_THREAD; ++j) {
        if (!((present[j] >> lane) & 1)) continue;
        int64_t row = first;
        for (int q = 0; q < j * ZN_WAVES + wave; ++q) row += count[q];
        row += __popcll(present[j] & ((1ull << lane) - 1));
        if (row >= d.capacity) continue;                                   // the call then fails, naming capacity
        const unsigned i = (unsigned)(base + j * ZN_NT + threadIdx.x);
        d.zone[row] = (int32_t)i;
        if (d.count) d.count[row] = (int64_t)t.n[i];
        if (d.cells) d.cells[row] = (int64_t)t.cells[i];
#pragma unroll
        for (int k = 1; k < 7; ++k)
            if (d.s[k]) d.s[k][row] = f.s[k][i];
    }
}

// 5
template <typename T, typename O>
__global__ __launch_bounds__(ZN_NT) void zonal_planes_kernel(const ZonalGeom g, const T *__restrict__ z, const int64_t ldz,
                                                             const int32_t *__restrict__ zones, const int64_t ldq, const unsigned nz,
                                                             const double quantum, const ZonalTables t, const ZonalFin f, const ZonalPlaneOut o,
                                                             const ZonalCounters *__restrict__ counters) {
    if (counters->bad) return;
    const int64_t i = (int64_t)blockIdx.x * ZN_NT + threadIdx.x;
    if (i >= (int64_t)g.nrow * g.ncol) return;
    const int64_t r = i / g.ncol, c = i - r * g.ncol;
    const int zn = zones[r * ldq + c];
    const bool in = zn >= 0 && (unsigned)zn < nz;
    const double na = zonal_nan();
    if (o.p[0]) ((int32_t *)o.p[0])[r * o.ld[0] + c] = in ? (int32_t)t.n[zn] : 0;
    if (o.p[11]) ((int32_t *)o.p[11])[r * o.ld[11] + c] = in ? (int32_t)t.cells[zn] : 0;
#pragma unroll
    for (int k = 1; k < 7; ++k)
        if (o.p[k]) ((O *)o.p[k])[r * o.ld[k] + c] = (O)(in ? f.s[k][zn] : na);
    if (!(o.p[7] || o.p[8] || o.p[9] || o.p[10])) return;
    bool contributes = false;
    int32_t q = 0;
    if (in) {
        const double v = (double)z[r * ldz + c];
        if (!prox_na(v, g.has_nodata != 0, g.nodata) && zn_finite(v) && zonal_fits(v, quantum)) {
            contributes = true;
            q = zonal_q(v, quantum);
        }
    }
    const double mm = contributes && (o.p[7] || o.p[10]) ? zonal_minus_mean(q, quantum, f.s[2][zn]) : na;
    if (o.p[7]) ((O *)o.p[7])[r * o.ld[7] + c] = (O)mm;
    if (o.p[8]) ((O *)o.p[8])[r * o.ld[8] + c] = (O)(contributes ? zonal_above_min(q, quantum, f.s[4][zn]) : na);
    if (o.p[9]) ((O *)o.p[9])[r * o.ld[9] + c] = (O)(contributes ? zonal_below_max(q, quantum, f.s[5][zn]) : na);
    if (o.p[10]) ((O *)o.p[10])[r * o.ld[10] + c] = (O)(contributes ? zonal_dev(mm, f.s[3][zn]) : na);
}

static unsigned zn_table_stats(const mhs_zonal_table *t) {
    if (!t) return 0u;
    return (t->count ? ZONAL_COUNT : 0u) | (t->sum ? ZONAL_SUM : 0u) | (t->mean ? ZONAL_MEAN : 0u) | (t->sd ? ZONAL_SD : 0u) |
           (t->min ? ZONAL_MIN : 0u) | (t->max ? ZONAL_MAX : 0u) | (t->range ? ZONAL_RANGE : 0u) | (t->cells ? ZONAL_CELLS : 0u);
}
static unsigned zn_plane_stats(const mhs_zonal_planes *p) {
    unsigned m = 0;
    if (p)
        for (int k = 0; k < ZONAL_N_STATS; ++k)
            if (p->plane[k]) m |= 1u << k;
    return m;
}

// Every check of a zonal call, before any device call; fn = the entry point's name for the message
static int zonal_check(const char *fn, const mhs_grid *grid, const mhs_stack *stack, int layer, const int32_t *zones, int64_t ld_zones, int64_t n_zones,
                       double quantum, int flags, const mhs_zonal_table *table, const mhs_zonal_planes *planes, bool dev, const mhs_zonal_info *info,
                       ZonalGeom *g) {
    ZN_REQUIRE(grid && stack && zones, "%s: NULL argument (g, stack or zones)", fn);
    ZN_REQUIRE(grid->nrow > 0 && grid->ncol > 0 && grid->nrow <= (int64_t)INT32_MAX && grid->ncol <= (int64_t)INT32_MAX,
               "%s: bad grid geometry (nrow, ncol must be in 1 .. 2^31 - 1)", fn);
    ZN_REQUIRE(grid->nrow * grid->ncol <= (int64_t)INT32_MAX, "%s: grid too large: nrow * ncol must not pass 2^31 - 1", fn);
    ZN_REQUIRE(stack->data, "%s: stack data is NULL", fn);
    ZN_REQUIRE(stack->dtype == MHS_F64 || stack->dtype == MHS_F32 || stack->dtype == MHS_I16, "%s: bad stack dtype", fn);
    ZN_REQUIRE(layer >= 0 && layer < stack->n_layers, "%s: layer %d is not one of the stack's %d layers", fn, layer, stack->n_layers);
    ZN_REQUIRE(stack->ld >= grid->ncol && (stack->n_layers == 1 || stack->plane_stride >= stack->ld * (grid->nrow - 1) + grid->ncol),
               "%s: stack strides smaller than the grid", fn);
    ZN_REQUIRE(ld_zones >= grid->ncol, "%s: ld_zones smaller than the grid width", fn);
    ZN_REQUIRE(n_zones >= 0 && n_zones <= (int64_t)INT32_MAX, "%s: n_zones must be 0 (measure it) or in 1 .. 2^31 - 1 (a zone is an int32)", fn);
    ZN_REQUIRE(quantum == 0.0 || zonal_quantum_ok(quantum), "%s: quantum must be 0 (measure it) or a power of two in 2^-1022 .. 2^1023", fn);
    ZN_REQUIRE((flags & ~MHS_ZONAL_NO_STRIP) == 0, "%s: unknown bit in flags", fn);
    const unsigned ts = zn_table_stats(table), ps = zn_plane_stats(planes);
    ZN_REQUIRE(ts || ps || info, "%s: no output: the table names no statistic, planes no plane, and info is NULL", fn);
    ZN_REQUIRE(!table || ts || !table->zone, "%s: the table names no statistic (only zone is set)", fn);
    if (ts) {
        ZN_REQUIRE(table->capacity >= 0, "%s: the table's capacity must not be negative", fn);
        ZN_REQUIRE(!table->zone || info, "%s: a present table (zone is set) needs info: K comes back in info->n_present", fn);
        ZN_REQUIRE(table->zone || n_zones <= table->capacity, "%s: n_zones %lld passes the dense table's capacity %lld", fn, (long long)n_zones,
                   (long long)table->capacity);
    }
    if (ps) {
        ZN_REQUIRE(planes->dtype == MHS_F64 || planes->dtype == MHS_F32, "%s: the planes' dtype must be MHS_F64 or MHS_F32", fn);
        if (dev)
            for (int k = 0; k < ZONAL_N_STATS; ++k)
                ZN_REQUIRE(!planes->plane[k] || planes->ld[k] >= grid->ncol, "%s: ld of plane %d smaller than the grid width", fn, k);
    }
    *g = ZonalGeom{(int)grid->nrow, (int)grid->ncol, stack->nodata, !std::isnan(stack->nodata),
                   (int)((grid->ncol + ZONAL_TILE_COLS - 1) / ZONAL_TILE_COLS)};
    return MHS_OK;
}

// Phase 1 and what the host decides from it (zonal_int.h)
int zonal_measure(const char *fn, const ZonalGeom &g, int dtype, const void *plane, int64_t ldz, const int32_t *zones, int64_t ldq, hipStream_t st,
                  ZonalCounters *counters, ZonalCounters *c, int64_t *n_zones, double *quantum) {
    const size_t n = (size_t)g.nrow * (size_t)g.ncol;
    const int n_cu = ctx().n_cu > 0 ? ctx().n_cu : 256;
    const unsigned nb = std::min<unsigned>((unsigned)((n + ZN_NT - 1) / ZN_NT), (unsigned)n_cu * 8u);
    if (dtype == MHS_F64) hipLaunchKernelGGL(zonal_range_kernel<double>, dim3(nb), dim3(ZN_NT), 0, st, g, (const double *)plane, ldz, zones, ldq, counters);
    else if (dtype == MHS_F32) hipLaunchKernelGGL(zonal_range_kernel<float>, dim3(nb), dim3(ZN_NT), 0, st, g, (const float *)plane, ldz, zones, ldq, counters);
    else hipLaunchKernelGGL(zonal_range_kernel<short>, dim3(nb), dim3(ZN_NT), 0, st, g, (const short *)plane, ldz, zones, ldq, counters);
    MHS_HIP(hipGetLastError());
    MHS_HIP(hipMemcpyAsync(c, counters, sizeof(*c), hipMemcpyDeviceToHost, st));
    MHS_HIP(hipStreamSynchronize(st));
    double max_abs;
    std::memcpy(&max_abs, &c->max_abs_bits, 8);
    if (*n_zones == 0) *n_zones = (int64_t)c->zones_end;
    ZN_REQUIRE((int64_t)c->zones_end <= *n_zones, "%s: the zone plane holds zone %lld, which is not below n_zones %lld", fn, (long long)c->zones_end - 1,
               (long long)*n_zones);
    if (*quantum == 0.0) *quantum = zonal_default_quantum(max_abs);
    ZN_REQUIRE(zonal_fits(max_abs, *quantum), "%s: quantum %g is too small: the layer's largest magnitude %g passes 2^30 * quantum", fn, *quantum, max_abs);
    return MHS_OK;
}

template <typename T>
static void launch_zonal_planes(int out_dtype, unsigned nb, hipStream_t st, const ZonalGeom &g, const void *z, int64_t ldz, const int32_t *zones,
                                int64_t ldq, unsigned nz, double quantum, const ZonalTables &t, const ZonalFin &f, const ZonalPlaneOut &o,
                                const ZonalCounters *counters) {
    if (out_dtype == MHS_F64)
        hipLaunchKernelGGL((zonal_planes_kernel<T, double>), dim3(nb), dim3(ZN_NT), 0, st, g, (const T *)z, ldz, zones, ldq, nz, quantum, t, f, o, counters);
    else
        hipLaunchKernelGGL((zonal_planes_kernel<T, float>), dim3(nb), dim3(ZN_NT), 0, st, g, (const T *)z, ldz, zones, ldq, nz, quantum, t, f, o, counters);
}

// Device planes.  `plane` = element (0, 0) of the layer, of `dtype`, with the row stride ldz; the table's arrays and the planes
// are device memory.
static int zonal_run(const char *fn, const ZonalGeom &g, int dtype, const void *plane, int64_t ldz, const int32_t *zones, int64_t ldq, int64_t n_zones,
                     double quantum, int flags, const mhs_zonal_table *table, const mhs_zonal_planes *planes, hipStream_t st, mhs_zonal_info *info) {
    const size_t n = (size_t)g.nrow * (size_t)g.ncol;
    const unsigned ts = zn_table_stats(table), ps = zn_plane_stats(planes);
    const bool present = ts && table->zone;
    const int n_cu = ctx().n_cu > 0 ? ctx().n_cu : 256;
    const unsigned nb_cells = (unsigned)((n + ZN_NT - 1) / ZN_NT);
    ZonalScratch cs;
    if (int rc = cs.get(fn, 256, st, "the counter block")) return rc;
    ZonalCounters *counters = (ZonalCounters *)cs.p;
    MHS_HIP(hipMemsetAsync(counters, 0, 256, st));
    ZonalCounters c;
    std::memset(&c, 0, sizeof(c));
    // 1
    const bool measure = n_zones == 0 || (quantum == 0.0 && dtype != MHS_I16) || info;
    if (quantum == 0.0 && dtype == MHS_I16) quantum = 1.0;
    if (measure) {
        if (int rc = zonal_measure(fn, g, dtype, plane, ldz, zones, ldq, st, counters, &c, &n_zones, &quantum)) return rc;
        ZN_REQUIRE(!ts || present || n_zones <= table->capacity, "%s: n_zones %lld passes the dense table's capacity %lld", fn, (long long)n_zones,
                   (long long)table->capacity);
    }
    const unsigned nz = (unsigned)n_zones;
    // what is needed
    unsigned fin_bits = (present ? ts : 0u) | (ps & 0x7eu);                                   // float64 statistics gathered later
    if (ps & (ZONAL_MINUS_MEAN | ZONAL_DEV)) fin_bits |= ZONAL_MEAN;
    if (ps & ZONAL_DEV) fin_bits |= ZONAL_SD;
    if (ps & ZONAL_ABOVE_MIN) fin_bits |= ZONAL_MIN;
    if (ps & ZONAL_BELOW_MAX) fin_bits |= ZONAL_MAX;
    fin_bits &= 0x7eu;
    const bool count_present = present || info;
    const unsigned need = zonal_needs(ts | ps) | (count_present ? (unsigned)ZONAL_A_CELLS : 0u) | (unsigned)ZONAL_A_N;
    // the block of tables
    const size_t slots = std::max<size_t>(nz, 1), n_blocks = (slots + ZONAL_SCAN_BLOCK - 1) / ZONAL_SCAN_BLOCK;
    size_t total = 0;
    auto take = [&](bool wanted, size_t bytes) { const size_t o = total; if (wanted) total += zn_align(bytes); return wanted ? o : (size_t)-1; };
    const size_t o_cells = take(need & ZONAL_A_CELLS, 4 * slots), o_n = take(true, 4 * slots), o_S1 = take(need & ZONAL_A_S1, 8 * slots),
                 o_L = take(need & ZONAL_A_S2, 8 * slots), o_H = take(need & ZONAL_A_S2, 8 * slots), o_min = take(need & ZONAL_A_MIN, 4 * slots),
                 o_max = take(need & ZONAL_A_MAX, 4 * slots), int_bytes = total;
    size_t o_fin[7];
    for (int k = 1; k < 7; ++k) o_fin[k] = take(fin_bits >> k & 1u, 8 * slots);
    const size_t o_blocks = take(present, 4 * n_blocks);
    ZonalScratch s;
    if (int rc = s.get(fn, total, st, "the zone tables (at most 40 bytes per zone slot and 8 per float64 statistic)")) return rc;
    auto at = [&](size_t o) { return o == (size_t)-1 ? nullptr : s.p + o; };
    const ZonalTables t{(uint32_t *)at(o_cells), (uint32_t *)at(o_n), (unsigned long long *)at(o_S1), (unsigned long long *)at(o_L),
                        (unsigned long long *)at(o_H), (int *)at(o_min), (int *)at(o_max)};
    ZonalFin f{};
    for (int k = 1; k < 7; ++k) f.s[k] = (double *)at(o_fin[k]);
    int32_t *blocks = (int32_t *)at(o_blocks);
    MHS_HIP(hipMemsetAsync(s.p, 0, int_bytes, st));
    const unsigned nb_slots = (unsigned)((slots + ZN_NT - 1) / ZN_NT);
    if (nz > 0) {
        if (t.qmin || t.qmax) {
            hipLaunchKernelGGL(zonal_init_kernel, dim3(nb_slots), dim3(ZN_NT), 0, st, nz, t.qmin, t.qmax);
            MHS_HIP(hipGetLastError());
        }
        // 2
        const int strip_rows = ZONAL_TILE_ROWS * ((flags & MHS_ZONAL_NO_STRIP) ? 1 : ZONAL_STRIP_TILES);
        const unsigned nb = (unsigned)g.tiles_c * (unsigned)((g.nrow + strip_rows - 1) / strip_rows);
        if (dtype == MHS_F64)
            hipLaunchKernelGGL(zonal_accumulate_kernel<double>, dim3(nb), dim3(ZN_NT), 0, st, g, (const double *)plane, ldz, zones, ldq, nz, quantum, need,
                               strip_rows, t, counters);
        else if (dtype == MHS_F32)
            hipLaunchKernelGGL(zonal_accumulate_kernel<float>, dim3(nb), dim3(ZN_NT), 0, st, g, (const float *)plane, ldz, zones, ldq, nz, quantum, need,
                               strip_rows, t, counters);
        else
            hipLaunchKernelGGL(zonal_accumulate_kernel<short>, dim3(nb), dim3(ZN_NT), 0, st, g, (const short *)plane, ldz, zones, ldq, nz, quantum, need,
                               strip_rows, t, counters);
        MHS_HIP(hipGetLastError());
        // 3
        ZonalDense d{};
        if (ts && !present) {
            d.count = table->count; d.cells = table->cells;
            d.s[1] = table->sum; d.s[2] = table->mean; d.s[3] = table->sd; d.s[4] = table->min; d.s[5] = table->max; d.s[6] = table->range;
        }
        if (fin_bits || (ts && !present)) {
            hipLaunchKernelGGL(zonal_finalise_kernel, dim3(nb_slots), dim3(ZN_NT), 0, st, nz, quantum, t, f, d, (const ZonalCounters *)counters);
            MHS_HIP(hipGetLastError());
        }
        // 4
        if (count_present) {
            hipLaunchKernelGGL(zonal_present_kernel, dim3((unsigned)std::min<size_t>(n_blocks, (size_t)n_cu * 8)), dim3(ZN_NT), 0, st, nz, (unsigned)n_blocks,
                               (const uint32_t *)t.cells, blocks, counters);
            MHS_HIP(hipGetLastError());
        }
        if (present) {
            hipLaunchKernelGGL(zonal_scan_kernel, dim3(1), dim3(ZN_NT), 0, st, (unsigned)n_blocks, blocks);
            MHS_HIP(hipGetLastError());
            ZonalDense p{};
            p.zone = table->zone; p.count = table->count; p.cells = table->cells; p.capacity = table->capacity;
            p.s[1] = table->sum; p.s[2] = table->mean; p.s[3] = table->sd; p.s[4] = table->min; p.s[5] = table->max; p.s[6] = table->range;
            hipLaunchKernelGGL(zonal_rows_kernel, dim3((unsigned)n_blocks), dim3(ZN_NT), 0, st, nz, t, f, (const int32_t *)blocks, p,
                               (const ZonalCounters *)counters);
            MHS_HIP(hipGetLastError());
        }
    }
    // 5
    if (ps) {
        ZonalPlaneOut o;
        for (int k = 0; k < ZONAL_N_STATS; ++k) { o.p[k] = planes->plane[k]; o.ld[k] = planes->plane[k] ? planes->ld[k] : 0; }
        if (dtype == MHS_F64) launch_zonal_planes<double>(planes->dtype, nb_cells, st, g, plane, ldz, zones, ldq, nz, quantum, t, f, o, counters);
        else if (dtype == MHS_F32) launch_zonal_planes<float>(planes->dtype, nb_cells, st, g, plane, ldz, zones, ldq, nz, quantum, t, f, o, counters);
        else launch_zonal_planes<short>(planes->dtype, nb_cells, st, g, plane, ldz, zones, ldq, nz, quantum, t, f, o, counters);
        MHS_HIP(hipGetLastError());
    }
    if (info || !measure) {
        const unsigned long long n_nonfinite = c.n_nonfinite;
        MHS_HIP(hipMemcpyAsync(&c, counters, sizeof(c), hipMemcpyDeviceToHost, st));
        MHS_HIP(hipStreamSynchronize(st));
        ZN_REQUIRE(!(c.bad & ZN_BAD_ZONE), "%s: the zone plane holds a zone that is not below n_zones %lld", fn, (long long)n_zones);
        ZN_REQUIRE(!(c.bad & ZN_BAD_QUANTUM), "%s: quantum %g is too small: a value's magnitude passes 2^30 * quantum", fn, quantum);
        ZN_REQUIRE(!present || (int64_t)c.n_present <= table->capacity, "%s: %lld zones are present, which passes the table's capacity %lld", fn,
                   (long long)c.n_present, (long long)table->capacity);
        if (info)
            *info = mhs_zonal_info{n_zones, (int64_t)c.n_present, (int64_t)c.n_in_zone, (int64_t)c.n_contrib, (int64_t)n_nonfinite, (int64_t)c.n_inexact,
                                   quantum, (int64_t)(total + 256)};
    }
    return MHS_OK;
}

}  // namespace mhs

using namespace mhs;

extern "C" {

int mhs_zonal_dev(const mhs_grid *g, const mhs_stack *stack, int layer, const int32_t *zones, int64_t ld_zones, int64_t n_zones, double quantum, int flags,
                  const mhs_zonal_table *table, const mhs_zonal_planes *planes, void *stream, mhs_zonal_info *info) {
    ZonalGeom zg;
    if (int rc = zonal_check(__func__, g, stack, layer, zones, ld_zones, n_zones, quantum, flags, table, planes, true, info, &zg)) return rc;
    if (int rc = require_ready()) return rc;
    const void *plane = (const char *)stack->data + (size_t)layer * stack->plane_stride * dtype_bytes(stack->dtype);
    return zonal_run(__func__, zg, stack->dtype, plane, stack->ld, zones, ld_zones, n_zones, quantum, flags, table, planes, pick_stream(stream), info);
}

// Host planes: the layer and the zone plane go up whole, the table's rows and the planes come down.
int mhs_zonal(const mhs_grid *g, const mhs_stack *stack, int layer, const int32_t *zones, int64_t n_zones, double quantum, int flags,
              const mhs_zonal_table *table, const mhs_zonal_planes *planes, mhs_zonal_info *info) {
    ZonalGeom zg;
    const char *fn = __func__;
    if (int rc = zonal_check(fn, g, stack, layer, zones, g ? g->ncol : 0, n_zones, quantum, flags, table, planes, false, info, &zg)) return rc;
    if (int rc = require_ready()) return rc;
    const size_t esz = dtype_bytes(stack->dtype), n = (size_t)zg.nrow * (size_t)zg.ncol;
    const size_t in_bytes = ((size_t)(zg.nrow - 1) * stack->ld + zg.ncol) * esz;
    const unsigned ts = zn_table_stats(table), ps = zn_plane_stats(planes);
    const size_t cap = ts ? (size_t)table->capacity : 0;
    // the table's arrays in the order zone, count, sum .. range, cells; then the planes
    void *const thost[9] = {ts ? (void *)table->zone : nullptr, ts ? (void *)table->count : nullptr, ts ? (void *)table->sum : nullptr,
                            ts ? (void *)table->mean : nullptr, ts ? (void *)table->sd : nullptr,    ts ? (void *)table->min : nullptr,
                            ts ? (void *)table->max : nullptr,  ts ? (void *)table->range : nullptr, ts ? (void *)table->cells : nullptr};
    size_t toff[9], poff[ZONAL_N_STATS], pbytes[ZONAL_N_STATS];
    size_t total = zn_align(in_bytes);
    const size_t o_zones = total;
    total += zn_align(4 * n);
    for (int k = 0; k < 9; ++k) { toff[k] = total; total += thost[k] ? zn_align((k == 0 ? 4 : 8) * std::max<size_t>(cap, 1)) : 0; }
    for (int k = 0; k < ZONAL_N_STATS; ++k) {
        pbytes[k] = (k == 0 || k == 11 || (ps && planes->dtype == MHS_F32) ? 4 : 8) * n;
        poff[k] = total;
        total += (ps >> k & 1u) ? zn_align(pbytes[k]) : 0;
    }
    std::lock_guard<std::mutex> lk(pipe_mutex());
    if (int rc = host_pipe(0)) return rc;                      // the pipeline's streams; its arena is not used
    hipStream_t st = ctx().pipe_comp;
    ZonalScratch s;
    if (int rc = s.get(fn, total, st, "the layer, the zone plane and the outputs")) return rc;
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{st};   // no copy is left in flight, whatever the exit
    MHS_HIP(hipMemcpyAsync(s.p, (const char *)stack->data + (size_t)layer * stack->plane_stride * esz, in_bytes, hipMemcpyHostToDevice, st));
    MHS_HIP(hipMemcpyAsync(s.p + o_zones, zones, 4 * n, hipMemcpyHostToDevice, st));
    auto tdev = [&](int k) { return thost[k] ? (void *)(s.p + toff[k]) : nullptr; };
    mhs_zonal_table dt{(int64_t)cap, (int32_t *)tdev(0), (int64_t *)tdev(1), (double *)tdev(2), (double *)tdev(3), (double *)tdev(4),
                       (double *)tdev(5), (double *)tdev(6), (double *)tdev(7), (int64_t *)tdev(8)};
    mhs_zonal_planes dp;
    std::memset(&dp, 0, sizeof(dp));
    if (ps) {
        dp.dtype = planes->dtype;
        for (int k = 0; k < ZONAL_N_STATS; ++k)
            if (ps >> k & 1u) { dp.plane[k] = s.p + poff[k]; dp.ld[k] = zg.ncol; }
    }
    mhs_zonal_info mine;
    if (int rc = zonal_run(fn, zg, stack->dtype, s.p, stack->ld, (const int32_t *)(s.p + o_zones), zg.ncol, n_zones, quantum, flags, ts ? &dt : nullptr,
                           ps ? &dp : nullptr, st, &mine))
        return rc;
    const size_t rows = ts ? (size_t)(table->zone ? mine.n_present : mine.n_zones) : 0;
    for (int k = 0; k < 9; ++k)
        if (thost[k] && rows) MHS_HIP(hipMemcpyAsync(thost[k], s.p + toff[k], (k == 0 ? 4 : 8) * rows, hipMemcpyDeviceToHost, st));
    for (int k = 0; k < ZONAL_N_STATS; ++k)
        if (ps >> k & 1u) MHS_HIP(hipMemcpyAsync(planes->plane[k], s.p + poff[k], pbytes[k], hipMemcpyDeviceToHost, st));
    MHS_HIP(hipStreamSynchronize(st));
    if (info) *info = mine;
    return MHS_OK;
}

}  // extern "C"
