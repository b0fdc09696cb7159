// Categorical layers: class counts, fractions and mode per zone, per target cell of another geometry and per window
// (include/machisplin_hip.h, section "classes", states the rule; classes_rule.h holds it).  Every accumulator is an exact
// integer count, so the order in which lanes, waves and workgroups add is free, and every atomic here is an integer atomic.
//
// Every phase is its own launch on the stream, and a kernel boundary is the only ordering between phases: no cross-block flag
// protocol, no spin wait, and every loop is bounded by the plane, by K or by a constant.
//   class_present_kernel        the census: n_valid, n_na, n_other, and -- when the class list is measured -- the codes present,
//                               as a 65 536-bit map: 2 048 words in LDS per workgroup, ORed to global by atomicOr of the
//                               non-zero words only.  The host reads 8 KiB back.
//   class_zone_range_kernel     max(zone) + 1, when n_zones is measured or an info is asked for.
//   class_zone_kernel           crosstab.  A workgroup of four waves takes a strip of CLS_STRIP_TILES tiles of 32 x 64 cells, a
//                               wave per row at a time.  A cell's KEY is zone * (K + 3) + slot (slot: k, K for `other`, K + 1
//                               for an NA cell of the zone).  A lane is a run head when its key differs from its left
//                               neighbour's; one ballot gives the heads, the run's length is the distance to the next head (a
//                               bit operation on the ballot, no scan), and only the head adds the length: to an open-addressed
//                               table of CLS_LDS_SLOTS slots in LDS keyed by the key -- one compare-and-swap claims a slot, at
//                               most CLS_PROBES probes -- or, when it finds no slot, straight to the global n_zones x (K + 3)
//                               uint32 table with a no-return atomicAdd.  Occupied slots are flushed once per strip.
//   class_zone_finish_kernel    a lane per zone: the rule's finishing function, into the dense table and the per-zone scratch.
//   class_zone_planes_kernel    a lane per cell: its zone's values.
//   class_aggregate_kernel      aggregate.  A workgroup owns a tile of target cells whose (K + 2)-word counters live entirely in
//                               LDS (at most CLS_AGG_WORDS words); its waves read the tile's source footprint row by row,
//                               consecutive lanes on consecutive cells, with the same run logic on the key (target column,
//                               slot); after a barrier a lane per target cell finishes and writes.  No global atomic, no
//                               device scratch.
//   class_indicator_kernel      focal: class k's 0 / 1 / NoData int16 plane; the library's own focal sum at offset 0 gives the
//   class_window_update_kernel  window count of that class, and the update keeps the running best count and code, the variety,
//   class_window_finish_kernel  and writes the requested frac plane; the finish writes mode, mode_frac, variety and n.
// A zone >= n_zones met without the measuring pass raises a device flag; such a cell touches no table, and the finish and
// planes kernels write nothing when it is set.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include "ensemble_int.h"
#include "resample_int.h"
#include "classes_rule.h"

namespace mhs {

constexpr int CL_NT = 256;                   // threads per workgroup of every phase: 4 waves
constexpr int CL_WAVES = CL_NT / 64;
constexpr int CL_MAP_WORDS = (CLS_MAX_CODE + 1) / 32;
static_assert(CLS_TILE_COLS == 64, "a wave holds one tile row in its lanes");
static_assert((CLS_LDS_SLOTS & (CLS_LDS_SLOTS - 1)) == 0 && CLS_LDS_SLOTS % CL_NT == 0, "a power of two, whole slots per thread");
static_assert(MHS_CLASS_MAX == CLS_MAX_K, "the header and the rule agree");

// how a kernel finds k: the list travels as a kernel argument and is put into LDS by the workgroup
struct ClsIndex {
    int K;                                   // 0: no list (the census of a measuring call)
    int use_table, min_code, span;
    uint16_t codes[CLS_MAX_K];
};
struct ClsFracSel {
    int n;
    uint8_t k[CLS_MAX_K];                    // the class index of each requested frac output
};
struct ClsLds {
    uint16_t codes[CLS_MAX_K];
    int16_t tab[CLS_TABLE_SPAN];
};

struct ClsCounters {
    unsigned long long n_valid, n_na, n_other;
    unsigned zones_end;                      // max(zone) + 1
    unsigned bad;                            // a zone >= n_zones
};
static_assert(sizeof(ClsCounters) <= 256, "the counter block");

struct ClsPlane {                            // the layer
    const void *z;
    int64_t ld;
    int nrow, ncol;
    double nodata;
    int has_nodata;
};

// the outputs on the cells (of the grid, or of the target geometry)
struct ClsOut {
    int32_t *mode, *variety, *n;
    void *mode_frac, *simpson, *frac;
    int64_t ld, frac_stride;
    int f64;
};
struct ClsTableOut {
    int32_t *counts, *n, *other, *cells, *mode, *variety;
    double *mode_frac, *simpson, *frac;
};
// what class_zone_planes_kernel gathers from
struct ClsZoneFin {
    int32_t *mode, *variety, *n;
    double *mode_frac, *simpson;
};

__device__ inline void cls_store(void *p, int f64, int64_t i, double v) {
    if (f64) ((double *)p)[i] = v;
    else ((float *)p)[i] = (float)v;
}

__device__ inline unsigned long long cl_wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// the list into LDS; the caller's barrier follows
__device__ inline void class_lds_fill(const ClsIndex &ix, ClsLds &s) {
    for (int k = threadIdx.x; k < ix.K; k += blockDim.x) s.codes[k] = ix.codes[k];
    if (ix.use_table) {
        for (int d = threadIdx.x; d < ix.span; d += blockDim.x) s.tab[d] = -1;
        __syncthreads();
        for (int k = threadIdx.x; k < ix.K; k += blockDim.x) s.tab[(int)ix.codes[k] - ix.min_code] = (int16_t)k;
    }
}
// code to k, by the direct table or by bisection: both give the same k (tests/classes_check.cpp)
__device__ inline int class_index(const ClsIndex &ix, const ClsLds &s, int code) {
    if (code < 0) return -1;
    return ix.use_table ? cls_index_table(s.tab, ix.min_code, ix.span, code) : cls_index_bisect(s.codes, ix.K, code);
}

// the census
template <typename T>
__global__ __launch_bounds__(CL_NT) void class_present_kernel(const ClsPlane p, const ClsIndex ix, uint32_t *present, ClsCounters *counters) {
    __shared__ uint32_t map[CL_MAP_WORDS];
    __shared__ ClsLds lds;
    const bool measure = ix.K == 0;
    if (measure)
        for (int w = threadIdx.x; w < CL_MAP_WORDS; w += CL_NT) map[w] = 0u;
    else class_lds_fill(ix, lds);
    __syncthreads();
    const T *z = (const T *)p.z;
    const unsigned chunks = ((unsigned)p.ncol + CL_NT - 1) / CL_NT;       // an item is CL_NT columns of a row: one division an item, none a cell
    const uint64_t items = (uint64_t)p.nrow * chunks;
    unsigned long long valid = 0, na = 0, other = 0;
    for (uint64_t t = blockIdx.x; t < items; t += gridDim.x) {
        const unsigned r = (unsigned)(t / chunks), c = (unsigned)(t - (uint64_t)r * chunks) * CL_NT + threadIdx.x;
        if (c >= (unsigned)p.ncol) continue;
        const double v = (double)z[(int64_t)r * p.ld + c];
        if (cls_na(v, p.has_nodata != 0, p.nodata)) { ++na; continue; }
        ++valid;
        const int code = cls_code(v);
        if (measure) {
            if (code < 0) ++other;
            else atomicOr(&map[code >> 5], 1u << (code & 31));
        } else if (class_index(ix, lds, code) < 0) ++other;
    }
    __syncthreads();
    if (measure)
        for (int w = threadIdx.x; w < CL_MAP_WORDS; w += CL_NT)
            if (map[w]) atomicOr(&present[w], map[w]);
    valid = cl_wave_sum(valid);
    na = cl_wave_sum(na);
    other = cl_wave_sum(other);
    if ((threadIdx.x & 63) == 0) {
        if (valid) atomicAdd(&counters->n_valid, valid);
        if (na) atomicAdd(&counters->n_na, na);
        if (other) atomicAdd(&counters->n_other, other);
    }
}

__global__ __launch_bounds__(CL_NT) void class_zone_range_kernel(const int nrow, const int ncol, const int32_t *__restrict__ zones, const int64_t ldq,
                                                                 ClsCounters *counters) {
    const unsigned chunks = ((unsigned)ncol + CL_NT - 1) / CL_NT;
    const uint64_t items = (uint64_t)nrow * chunks;
    unsigned end = 0;
    for (uint64_t t = blockIdx.x; t < items; t += gridDim.x) {
        const unsigned r = (unsigned)(t / chunks), c = (unsigned)(t - (uint64_t)r * chunks) * CL_NT + threadIdx.x;
        if (c >= (unsigned)ncol) continue;
        const int zn = zones[(int64_t)r * ldq + c];
        if (zn >= 0) end = max(end, (unsigned)zn + 1u);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) end = max(end, (unsigned)__shfl_xor((int)end, d, 64));
    if ((threadIdx.x & 63) == 0 && end) atomicMax(&counters->zones_end, end);
}

// the length of the run that starts at `lane`, from the ballot of the run heads
__device__ inline unsigned class_run_length(uint64_t heads, int lane) {
    const uint64_t after = lane == 63 ? 0ull : heads >> (lane + 1);
    return after ? (unsigned)__builtin_ctzll(after) + 1u : (unsigned)(64 - lane);
}

// crosstab.  blockIdx.x = strip * tiles_c + tile column; the table's row of zone z is table[z * (K + 3) ..]: count[K], other,
// the zone's NA cells, and a word that the finish kernel fills with n.
template <typename T>
__global__ __launch_bounds__(CL_NT) void class_zone_kernel(const ClsPlane p, const int32_t *__restrict__ zones, const int64_t ldq, const unsigned n_zones,
                                                           const ClsIndex ix, const int tiles_c, const int strip_rows, uint32_t *table,
                                                           ClsCounters *counters) {
    __shared__ int key[CLS_LDS_SLOTS];
    __shared__ unsigned val[CLS_LDS_SLOTS];
    __shared__ ClsLds lds;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int s = threadIdx.x; s < CLS_LDS_SLOTS; s += CL_NT) { key[s] = -1; val[s] = 0u; }
    class_lds_fill(ix, lds);
    __syncthreads();
    const T *z = (const T *)p.z;
    const int W = ix.K + 3;
    const int c = (int)(blockIdx.x % (unsigned)tiles_c) * CLS_TILE_COLS + lane;
    const int r_begin = (int)(blockIdx.x / (unsigned)tiles_c) * strip_rows;
    const int r_end = (int)min((int64_t)p.nrow, (int64_t)r_begin + strip_rows);
    unsigned bad = 0;
    for (int r = r_begin + wave; r < r_end; r += CL_WAVES) {
        int zn = c < p.ncol ? zones[(int64_t)r * ldq + c] : -1;
        if (zn >= 0 && (unsigned)zn >= n_zones) { bad = 1u; zn = -1; }
        if (__ballot(zn >= 0) == 0) continue;                              // wave-uniform: no cell of this row has a zone
        int kk = -1;
        if (zn >= 0) {
            const double v = (double)z[(int64_t)r * p.ld + c];
            const int slot = cls_na(v, p.has_nodata != 0, p.nodata) ? ix.K + 1 : cls_slot(class_index(ix, lds, cls_code(v)), ix.K);
            kk = zn * W + slot;                                            // n_zones * (K + 3) <= 2^31 - 1 (checked by the host)
        }
        const int left = __shfl_up(kk, 1, 64);
        const uint64_t heads = __ballot(lane == 0 || kk != left);
        if (kk < 0 || !((heads >> lane) & 1ull)) continue;                 // only a run's head leaves the wave
        const unsigned len = class_run_length(heads, lane);
        unsigned s = (((unsigned)kk * 0x9E3779B1u) >> 20) & (unsigned)(CLS_LDS_SLOTS - 1);
        int slot = -1;
        for (int q = 0; q < CLS_PROBES; ++q) {
            const int k = atomicCAS(&key[s], -1, kk);
            if (k == -1 || k == kk) { slot = (int)s; break; }
            s = (s + 1u) & (unsigned)(CLS_LDS_SLOTS - 1);
        }
        if (slot < 0) atomicAdd(&table[kk], len);
        else atomicAdd(&val[slot], len);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < CLS_LDS_SLOTS; s += CL_NT) {
        const int kk = key[s];
        if (kk >= 0 && val[s]) atomicAdd(&table[kk], val[s]);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) bad |= (unsigned)__shfl_xor((int)bad, d, 64);
    if (lane == 0 && bad) atomicOr(&counters->bad, bad);
}

__global__ __launch_bounds__(CL_NT) void class_zone_finish_kernel(const unsigned nz, const ClsIndex ix, const ClsFracSel sel, uint32_t *table,
                                                                  const ClsTableOut t, const ClsZoneFin f, const ClsCounters *__restrict__ counters) {
    if (counters->bad) return;
    const unsigned i = blockIdx.x * CL_NT + threadIdx.x;
    if (i >= nz) return;
    const int K = ix.K, W = K + 3;
    uint32_t *row = table + (size_t)i * W;
    const ClsFin fin = cls_finish(row, K, row[K], ix.codes);
    row[K + 2] = fin.n;
    if (t.counts)
        for (int k = 0; k < K; ++k) t.counts[(size_t)i * K + k] = (int32_t)row[k];
    if (t.n) t.n[i] = (int32_t)fin.n;
    if (t.other) t.other[i] = (int32_t)row[K];
    if (t.cells) t.cells[i] = (int32_t)(fin.n + row[K + 1]);
    if (t.mode) t.mode[i] = fin.mode;
    if (t.variety) t.variety[i] = fin.variety;
    if (t.mode_frac) t.mode_frac[i] = fin.mode_frac;
    if (t.simpson) t.simpson[i] = fin.simpson;
    if (t.frac)
        for (int j = 0; j < sel.n; ++j) t.frac[(size_t)i * sel.n + j] = cls_frac(row[sel.k[j]], fin.n);
    if (f.mode) f.mode[i] = fin.mode;
    if (f.variety) f.variety[i] = fin.variety;
    if (f.n) f.n[i] = (int32_t)fin.n;
    if (f.mode_frac) f.mode_frac[i] = fin.mode_frac;
    if (f.simpson) f.simpson[i] = fin.simpson;
}

__global__ __launch_bounds__(CL_NT) void class_zone_planes_kernel(const int nrow, const int ncol, const int32_t *__restrict__ zones, const int64_t ldq,
                                                                  const unsigned nz, const int K, const ClsFracSel sel, const uint32_t *__restrict__ table,
                                                                  const ClsZoneFin f, const ClsOut o, const ClsCounters *__restrict__ counters) {
    if (counters->bad) return;
    const int64_t i = (int64_t)blockIdx.x * CL_NT + threadIdx.x;
    if (i >= (int64_t)nrow * ncol) return;
    const int64_t r = (unsigned)i / (unsigned)ncol, c = i - r * ncol, at = r * o.ld + c;      // i < 2^31: a 32-bit division
    const int zn = zones[r * ldq + c];
    const bool in = zn >= 0 && (unsigned)zn < nz;
    const double na = cls_nan();
    if (o.mode) o.mode[at] = in ? f.mode[zn] : -1;
    if (o.variety) o.variety[at] = in ? f.variety[zn] : -1;
    if (o.n) o.n[at] = in ? f.n[zn] : -1;
    if (o.mode_frac) cls_store(o.mode_frac, o.f64, at, in ? f.mode_frac[zn] : na);
    if (o.simpson) cls_store(o.simpson, o.f64, at, in ? f.simpson[zn] : na);
    if (o.frac) {
        const uint32_t *row = table + (size_t)(in ? zn : 0) * (K + 3);
        for (int j = 0; j < sel.n; ++j) cls_store(o.frac, o.f64, (int64_t)j * o.frac_stride + at, in ? cls_frac(row[sel.k[j]], row[K + 2]) : na);
    }
}

// aggregate.  A tile is tr x tc target cells (tr, tc <= CLS_AGG_SIDE, tr * tc * (K + 2) <= CLS_AGG_WORDS); blockIdx.x = tile row
// * tiles_c + tile column.  Dynamic LDS: the tile's counters, cell after cell: count[K], other, a spare word.
template <typename T>
__global__ __launch_bounds__(CL_NT) void class_aggregate_kernel(const ClsPlane p, const RsGrid S, const RsGrid Tg, const ClsIndex ix, const ClsFracSel sel,
                                                                const int tr, const int tc, const int tiles_c, const ClsOut o) {
    extern __shared__ uint32_t cnt[];
    __shared__ ClsLds lds;
    __shared__ int col_edge[CLS_AGG_SIDE + 1], row_edge[CLS_AGG_SIDE + 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int K = ix.K, W = K + 2;
    const int R0 = (int)(blockIdx.x / (unsigned)tiles_c) * tr, C0 = (int)(blockIdx.x % (unsigned)tiles_c) * tc;
    const int nr = min(tr, Tg.nrow - R0), ncl = min(tc, Tg.ncol - C0);     // the tile's target rows and columns: both >= 1
    for (int i = threadIdx.x; i < nr * ncl * W; i += CL_NT) cnt[i] = 0u;
    for (int i = threadIdx.x; i <= ncl; i += CL_NT) col_edge[i] = rs_foot_col(S, Tg, C0 + i);
    for (int i = threadIdx.x; i <= nr; i += CL_NT) row_edge[i] = rs_foot_row(S, Tg, R0 + i);
    class_lds_fill(ix, lds);
    __syncthreads();
    const T *z = (const T *)p.z;
    const int j_lo = col_edge[0], j_hi = col_edge[ncl], i_lo = row_edge[0], i_hi = row_edge[nr];     // inside [0, ncol] x [0, nrow]
    for (int i = i_lo + wave; i < i_hi; i += CL_WAVES) {
        // the target row of source row i: the first tr_ with row_edge[tr_ + 1] > i (7 halvings of at most 64)
        int lo = 0, hi = nr - 1;
        for (int s = 0; s < 7; ++s) {
            if (lo >= hi) break;
            const int mid = (lo + hi) >> 1;
            if (row_edge[mid + 1] > i) hi = mid;
            else lo = mid + 1;
        }
        const int base = lo * ncl * W;
        const T *zrow = z + (int64_t)i * p.ld;
        int a = 0;                                                         // the lane's target column: j grows by 64 a chunk, so it only moves east
        T next = j_lo + lane < j_hi ? zrow[j_lo + lane] : T(0);            // the load of a chunk is issued one chunk ahead of its use
        for (int j0 = j_lo; j0 < j_hi; j0 += 64) {
            const int j = j0 + lane;
            const T cur = next;
            if (j + 64 < j_hi) next = zrow[j + 64];
            int kk = -1;
            if (j < j_hi) {
                while (a < ncl - 1 && col_edge[a + 1] <= j) ++a;           // the first column with col_edge[. + 1] > j: at most ncl - 1 steps a row
                const double v = (double)cur;
                if (!cls_na(v, p.has_nodata != 0, p.nodata)) kk = a * W + cls_slot(class_index(ix, lds, cls_code(v)), K);
            }
            const int left = __shfl_up(kk, 1, 64);
            const uint64_t heads = __ballot(lane == 0 || kk != left);
            if (kk >= 0 && ((heads >> lane) & 1ull)) atomicAdd(&cnt[base + kk], class_run_length(heads, lane));
        }
    }
    __syncthreads();
    for (int cell = threadIdx.x; cell < nr * ncl; cell += CL_NT) {
        const uint32_t *row = cnt + cell * W;
        const ClsFin fin = cls_finish(row, K, row[K], lds.codes);
        const int r = cell / ncl, c = cell - r * ncl;
        const int64_t at = (int64_t)(R0 + r) * o.ld + (C0 + c);
        if (o.mode) o.mode[at] = fin.mode;
        if (o.variety) o.variety[at] = fin.variety;
        if (o.n) o.n[at] = (int32_t)fin.n;
        if (o.mode_frac) cls_store(o.mode_frac, o.f64, at, fin.mode_frac);
        if (o.simpson) cls_store(o.simpson, o.f64, at, fin.simpson);
        if (o.frac)
            for (int j = 0; j < sel.n; ++j) cls_store(o.frac, o.f64, (int64_t)j * o.frac_stride + at, cls_frac(row[sel.k[j]], fin.n));
    }
}

// focal: class `code`'s indicator, 1 / 0 / -1 (NoData) as int16, dense
template <typename T>
__global__ __launch_bounds__(CL_NT) void class_indicator_kernel(const ClsPlane p, const int code, int16_t *__restrict__ ind) {
    const int64_t i = (int64_t)blockIdx.x * CL_NT + threadIdx.x;
    if (i >= (int64_t)p.nrow * p.ncol) return;
    const int64_t r = (unsigned)i / (unsigned)p.ncol, c = i - r * p.ncol;                     // i < 2^31: a 32-bit division
    const double v = (double)((const T *)p.z)[r * p.ld + c];
    ind[i] = cls_na(v, p.has_nodata != 0, p.nodata) ? (int16_t)-1 : (int16_t)(cls_code(v) == code ? 1 : 0);
}

// focal: the window count of class k (a double that holds an integer below 2^53; NaN where the centre is NA) against the
// running best.  `win_n` is focal's count of the window's valid cells; first = 1 starts the state.
__global__ __launch_bounds__(CL_NT) void class_window_update_kernel(const int64_t n_cells, const int ncol, const int first, const int code,
                                                                    const double *__restrict__ sum, const double *__restrict__ win_n,
                                                                    uint32_t *__restrict__ best_count, int32_t *__restrict__ best_code,
                                                                    int32_t *__restrict__ variety, void *frac_plane, const int64_t ld, const int f64) {
    const int64_t i = (int64_t)blockIdx.x * CL_NT + threadIdx.x;
    if (i >= n_cells) return;
    const double s = sum[i];
    const bool centre = s == s;
    const uint32_t c = centre ? (uint32_t)s : 0u;
    uint32_t bc = first ? 0u : best_count[i];
    int32_t bk = first ? -1 : best_code[i], var = first ? 0 : variety[i];
    if (c) ++var;
    if (cls_takes(c, bc)) { bc = c; bk = code; }
    best_count[i] = bc; best_code[i] = bk; variety[i] = var;
    if (frac_plane) {
        const int64_t r = (unsigned)i / (unsigned)ncol, cc = i - r * ncol;
        const double wn = win_n[i];
        cls_store(frac_plane, f64, r * ld + cc, centre ? cls_frac(c, (uint32_t)wn) : cls_nan());
    }
}

__global__ __launch_bounds__(CL_NT) void class_window_finish_kernel(const int64_t n_cells, const int ncol, const double *__restrict__ win_n,
                                                                    const uint32_t *__restrict__ best_count, const int32_t *__restrict__ best_code,
                                                                    const int32_t *__restrict__ variety, const ClsOut o) {
    const int64_t i = (int64_t)blockIdx.x * CL_NT + threadIdx.x;
    if (i >= n_cells) return;
    const int64_t r = (unsigned)i / (unsigned)ncol, c = i - r * ncol, at = r * o.ld + c;      // i < 2^31: a 32-bit division
    const double wn = win_n[i];
    const bool centre = wn == wn;                                          // focal gives NaN where the centre is NA
    const uint32_t n = centre ? (uint32_t)wn : 0u;
    if (o.mode) o.mode[at] = centre ? best_code[i] : -1;
    if (o.variety) o.variety[at] = centre ? variety[i] : -1;
    if (o.n) o.n[at] = centre ? (int32_t)n : -1;
    if (o.mode_frac) cls_store(o.mode_frac, o.f64, at, centre && best_code[i] >= 0 ? cls_frac(best_count[i], n) : cls_nan());
}

#define CL_REQUIRE(cond, ...)                                              \
    do {                                                                   \
        if (!(cond)) { set_error(__VA_ARGS__); return MHS_ERR_INVALID; }    \
    } while (0)

// the class list and frac_of of a call, checked before any device call.  n_classes = 0: the list is measured (K stays 0)
static int class_check_list(const char *fn, const int32_t *classes, int n_classes, const int32_t *frac_of, int n_frac, bool want_frac, ClsIndex *ix) {
    std::memset(ix, 0, sizeof(*ix));
    CL_REQUIRE(n_classes >= 0 && n_classes <= CLS_MAX_K, "%s: classes holds %d codes: K must be in 1 .. %d (or 0 with classes NULL: measure them)", fn, n_classes,
               CLS_MAX_K);
    CL_REQUIRE((n_classes == 0) == (classes == nullptr), "%s: classes and n_classes disagree (NULL and 0 measure the codes; K = 0 is no list)", fn);
    CL_REQUIRE(n_frac >= 0 && n_frac <= CLS_MAX_K, "%s: n_frac_of must be in 0 .. %d", fn, CLS_MAX_K);
    CL_REQUIRE((n_frac == 0) == (frac_of == nullptr), "%s: frac_of and n_frac_of disagree", fn);
    CL_REQUIRE(!want_frac || n_classes > 0 || n_frac > 0, "%s: frac with measured classes needs frac_of: the number of outputs must be known", fn);
    for (int k = 0; k < n_classes; ++k)
        CL_REQUIRE(classes[k] >= 0 && classes[k] <= CLS_MAX_CODE, "%s: classes[%d] = %d: a code must be in 0 .. %d", fn, k, classes[k], CLS_MAX_CODE);
    for (int j = 0; j < n_frac; ++j)
        CL_REQUIRE(frac_of[j] >= 0 && frac_of[j] <= CLS_MAX_CODE, "%s: frac_of[%d] = %d: a code must be in 0 .. %d", fn, j, frac_of[j], CLS_MAX_CODE);
    for (int k = 0; k < n_classes; ++k) ix->codes[k] = (uint16_t)classes[k];
    std::sort(ix->codes, ix->codes + n_classes);
    for (int k = 1; k < n_classes; ++k)
        CL_REQUIRE(ix->codes[k] != ix->codes[k - 1], "%s: classes names code %d twice: the codes must be distinct", fn, (int)ix->codes[k]);
    ix->K = n_classes;
    for (int j = 0; j < n_frac && n_classes > 0; ++j)              // a measured list is held against frac_of behind the census (class_select)
        CL_REQUIRE(cls_index_bisect(ix->codes, n_classes, frac_of[j]) >= 0, "%s: frac_of[%d] = %d is not one of the %d classes", fn, j, frac_of[j], n_classes);
    return MHS_OK;
}
static void class_set_form(ClsIndex *ix) {
    ix->use_table = cls_use_table(ix->codes, ix->K) ? 1 : 0;
    ix->min_code = ix->codes[0];
    ix->span = ix->use_table ? (int)ix->codes[ix->K - 1] - (int)ix->codes[0] + 1 : 0;
}
// frac_of against the list in force (given or measured)
static int class_select(const char *fn, const ClsIndex &ix, const int32_t *frac_of, int n_frac, ClsFracSel *sel) {
    std::memset(sel, 0, sizeof(*sel));
    if (n_frac == 0) {
        sel->n = ix.K;
        for (int k = 0; k < ix.K; ++k) sel->k[k] = (uint8_t)k;
        return MHS_OK;
    }
    sel->n = n_frac;
    for (int j = 0; j < n_frac; ++j) {
        const int k = cls_index_bisect(ix.codes, ix.K, frac_of[j]);
        CL_REQUIRE(k >= 0, "%s: frac_of[%d] = %d is not one of the %d classes", fn, j, frac_of[j], ix.K);
        sel->k[j] = (uint8_t)k;
    }
    return MHS_OK;
}

static int class_check_layer(const char *fn, const mhs_grid *grid, const mhs_stack *stack, int layer, ClsPlane *p) {
    CL_REQUIRE(grid && stack, "%s: NULL argument (g or stack)", fn);
    CL_REQUIRE(grid->nrow > 0 && grid->ncol > 0 && grid->nrow <= (int64_t)INT32_MAX && grid->ncol <= (int64_t)INT32_MAX,
               "%s: bad grid geometry (nrow, ncol must be in 1 .. 2^31 - 1)", fn);
    CL_REQUIRE(grid->nrow * grid->ncol <= (int64_t)INT32_MAX, "%s: grid too large: nrow * ncol must not pass 2^31 - 1", fn);
    CL_REQUIRE(stack->data, "%s: stack data is NULL", fn);
    CL_REQUIRE(stack->dtype == MHS_F64 || stack->dtype == MHS_F32 || stack->dtype == MHS_I16, "%s: bad stack dtype", fn);
    CL_REQUIRE(layer >= 0 && layer < stack->n_layers, "%s: layer %d is not one of the stack's %d layers", fn, layer, stack->n_layers);
    CL_REQUIRE(stack->ld >= grid->ncol && (stack->n_layers == 1 || stack->plane_stride >= stack->ld * (grid->nrow - 1) + grid->ncol),
               "%s: stack strides smaller than the grid", fn);
    *p = ClsPlane{nullptr, stack->ld, (int)grid->nrow, (int)grid->ncol, stack->nodata, !std::isnan(stack->nodata)};
    return MHS_OK;
}

static bool class_planes_any(const mhs_class_planes *pl) {
    return pl && (pl->mode || pl->variety || pl->n || pl->mode_frac || pl->simpson || pl->frac);
}
static bool class_table_any(const mhs_class_table *t) {
    return t && (t->counts || t->n || t->other || t->cells || t->mode || t->variety || t->mode_frac || t->simpson || t->frac);
}
// the planes of a call against the width of what they cover
static int class_check_planes(const char *fn, const mhs_class_planes *pl, int64_t nrow, int64_t ncol, int n_frac_out, bool dev, bool simpson_ok) {
    if (!class_planes_any(pl)) return MHS_OK;
    CL_REQUIRE(pl->dtype == MHS_F64 || pl->dtype == MHS_F32, "%s: the planes' dtype must be MHS_F64 or MHS_F32", fn);
    CL_REQUIRE(simpson_ok || !pl->simpson, "%s: simpson is not a product of a window", fn);
    if (dev) {
        CL_REQUIRE(pl->ld >= ncol, "%s: the planes' ld is smaller than their width %lld", fn, (long long)ncol);
        CL_REQUIRE(!pl->frac || n_frac_out <= 1 || pl->frac_stride >= pl->ld * (nrow - 1) + ncol, "%s: frac_stride smaller than a plane", fn);
    }
    return MHS_OK;
}
static ClsOut class_out(const mhs_class_planes *pl) {
    if (!pl) return ClsOut{};
    return ClsOut{pl->mode, pl->variety, pl->n, pl->mode_frac, pl->simpson, pl->frac, pl->ld, pl->frac_stride, pl->dtype == MHS_F64};
}

// a block of stream-ordered memory, given back behind whatever was enqueued last
struct ClsScratch {
    char *p = nullptr;
    hipStream_t st = nullptr;
    ~ClsScratch() { if (p) (void)hipFreeAsync(p, st); }
    int get(const char *fn, size_t bytes, hipStream_t s, const char *what) {
        st = s;
        if (hipMallocAsync((void **)&p, std::max<size_t>(bytes, 256), s) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            set_error("%s: no device memory for %s (%zu bytes)", fn, what, bytes);
            return MHS_ERR_ALLOC;
        }
        return MHS_OK;
    }
};
static size_t cl_align(size_t n) { return (n + 255) & ~(size_t)255; }
static unsigned cl_blocks(size_t n) { return (unsigned)((n + CL_NT - 1) / CL_NT); }

#define CL_BY_DTYPE(dtype, KERNEL, grid, lds, st, ...)                                                          \
    do {                                                                                                        \
        if ((dtype) == MHS_F64) hipLaunchKernelGGL(KERNEL<double>, dim3(grid), dim3(CL_NT), lds, st, __VA_ARGS__); \
        else if ((dtype) == MHS_F32) hipLaunchKernelGGL(KERNEL<float>, dim3(grid), dim3(CL_NT), lds, st, __VA_ARGS__); \
        else hipLaunchKernelGGL(KERNEL<short>, dim3(grid), dim3(CL_NT), lds, st, __VA_ARGS__);                     \
        MHS_HIP(hipGetLastError());                                                                             \
    } while (0)

// The census of a layer and, where K is 0, its class list: counters + the presence map in `block` (256 + 8 KiB).  Synchronises.
static int class_census(const char *fn, const ClsPlane &p, int dtype, ClsIndex *ix, char *block, hipStream_t st, ClsCounters *c) {
    ClsCounters *counters = (ClsCounters *)block;
    uint32_t *present = (uint32_t *)(block + 256);
    const bool measure = ix->K == 0;
    const int n_cu = ctx().n_cu > 0 ? ctx().n_cu : 256;
    const unsigned nb = std::min<unsigned>(cl_blocks((size_t)p.nrow * p.ncol), (unsigned)n_cu * 8u);
    CL_BY_DTYPE(dtype, class_present_kernel, nb, 0, st, p, *ix, present, counters);
    MHS_HIP(hipMemcpyAsync(c, counters, sizeof(*c), hipMemcpyDeviceToHost, st));
    static thread_local uint32_t map[CL_MAP_WORDS];
    if (measure) MHS_HIP(hipMemcpyAsync(map, present, sizeof(map), hipMemcpyDeviceToHost, st));
    MHS_HIP(hipStreamSynchronize(st));
    if (measure) {
        int found = 0;
        for (int w = 0; w < CL_MAP_WORDS; ++w) found += __builtin_popcount(map[w]);
        CL_REQUIRE(found <= CLS_MAX_K, "%s: the layer holds %d distinct codes: more than %d classes are out of scope (give classes)", fn, found, CLS_MAX_K);
        CL_REQUIRE(found >= 1, "%s: the layer holds no code in 0 .. %d: there is no class to measure (give classes)", fn, CLS_MAX_CODE);
        int k = 0;
        for (int code = 0; code <= CLS_MAX_CODE; ++code)
            if (map[code >> 5] >> (code & 31) & 1u) ix->codes[k++] = (uint16_t)code;
        ix->K = found;
    }
    return MHS_OK;
}
static void class_info(mhs_class_info *info, const ClsIndex &ix, int64_t n_zones, const ClsCounters &c, size_t scratch) {
    if (!info) return;
    std::memset(info, 0, sizeof(*info));
    info->K = ix.K;
    for (int k = 0; k < ix.K; ++k) info->codes[k] = ix.codes[k];
    info->n_zones = n_zones;
    info->n_valid = (int64_t)c.n_valid; info->n_na = (int64_t)c.n_na; info->n_other = (int64_t)c.n_other;
    info->scratch_bytes = (int64_t)scratch;
}

constexpr size_t CL_HEAD = 256 + CL_MAP_WORDS * 4;       // the counter block and the presence map

// ---- crosstab
static int crosstab_check(const char *fn, const mhs_grid *grid, const mhs_stack *stack, int layer, const int32_t *zones, int64_t ld_zones, int64_t n_zones,
                          const int32_t *classes, int n_classes, const int32_t *frac_of, int n_frac, const mhs_class_table *table,
                          const mhs_class_planes *planes, bool dev, const mhs_class_info *info, ClsPlane *p, ClsIndex *ix) {
    if (int rc = class_check_layer(fn, grid, stack, layer, p)) return rc;
    CL_REQUIRE(zones, "%s: NULL argument (zones)", fn);
    CL_REQUIRE(ld_zones >= grid->ncol, "%s: ld_zones smaller than the grid width", fn);
    CL_REQUIRE(n_zones >= 0 && n_zones <= (int64_t)INT32_MAX, "%s: n_zones must be 0 (measure it) or in 1 .. 2^31 - 1 (a zone is an int32)", fn);
    const bool ta = class_table_any(table), pa = class_planes_any(planes);
    const bool want_frac = (ta && table->frac) || (pa && planes->frac);
    if (int rc = class_check_list(fn, classes, n_classes, frac_of, n_frac, want_frac, ix)) return rc;
    CL_REQUIRE(ta || pa || info, "%s: no output: the table names no statistic, planes no plane, and info is NULL", fn);
    CL_REQUIRE(n_classes > 0 || !(ta && table->counts), "%s: counts with measured classes: the table's width K must be known (measure with info first)", fn);
    CL_REQUIRE(n_zones * (int64_t)(n_classes + 3) <= (int64_t)INT32_MAX, "%s: n_zones * (K + 3) = %lld passes 2^31 - 1", fn,
               (long long)(n_zones * (int64_t)(n_classes + 3)));
    if (ta) {
        CL_REQUIRE(table->capacity >= 0, "%s: the table's capacity must not be negative", fn);
        CL_REQUIRE(n_zones <= table->capacity, "%s: n_zones %lld passes the table's capacity %lld", fn, (long long)n_zones, (long long)table->capacity);
    }
    return class_check_planes(fn, planes, grid->nrow, grid->ncol, n_frac ? n_frac : n_classes, dev, true);
}

static int crosstab_run(const char *fn, ClsPlane p, int dtype, const int32_t *zones, int64_t ldq, int64_t n_zones, ClsIndex ix, const int32_t *frac_of,
                        int n_frac, const mhs_class_table *table, const mhs_class_planes *planes, hipStream_t st, mhs_class_info *info) {
    const size_t n = (size_t)p.nrow * (size_t)p.ncol;
    const bool ta = class_table_any(table), pa = class_planes_any(planes);
    const int n_cu = ctx().n_cu > 0 ? ctx().n_cu : 256;
    ClsScratch head;
    if (int rc = head.get(fn, CL_HEAD, st, "the counter block and the presence map")) return rc;
    MHS_HIP(hipMemsetAsync(head.p, 0, CL_HEAD, st));
    ClsCounters *counters = (ClsCounters *)head.p;
    ClsCounters c;
    std::memset(&c, 0, sizeof(c));
    const bool measured = ix.K == 0 || n_zones == 0 || info;
    if (n_zones == 0 || info) {
        hipLaunchKernelGGL(class_zone_range_kernel, dim3(std::min<unsigned>(cl_blocks(n), (unsigned)n_cu * 8u)), dim3(CL_NT), 0, st, p.nrow, p.ncol, zones, ldq,
                           counters);
        MHS_HIP(hipGetLastError());
    }
    if (ix.K == 0 || info) {
        if (int rc = class_census(fn, p, dtype, &ix, head.p, st, &c)) return rc;
    } else if (n_zones == 0) {
        MHS_HIP(hipMemcpyAsync(&c, counters, sizeof(c), hipMemcpyDeviceToHost, st));
        MHS_HIP(hipStreamSynchronize(st));
    }
    if (measured) {
        if (n_zones == 0) n_zones = (int64_t)c.zones_end;
        CL_REQUIRE(!(info || c.zones_end) || (int64_t)c.zones_end <= n_zones, "%s: the zone plane holds zone %lld, which is not below n_zones %lld", fn,
                   (long long)c.zones_end - 1, (long long)n_zones);
        CL_REQUIRE(n_zones * (int64_t)(ix.K + 3) <= (int64_t)INT32_MAX, "%s: n_zones * (K + 3) = %lld passes 2^31 - 1", fn,
                   (long long)(n_zones * (int64_t)(ix.K + 3)));
        CL_REQUIRE(!ta || n_zones <= table->capacity, "%s: n_zones %lld passes the table's capacity %lld", fn, (long long)n_zones, (long long)table->capacity);
    }
    class_set_form(&ix);
    ClsFracSel sel;
    if (int rc = class_select(fn, ix, frac_of, n_frac, &sel)) return rc;
    size_t total = 0;
    if (ta || pa) {
        const unsigned nz = (unsigned)n_zones;
        const int W = ix.K + 3;
        const size_t slots = std::max<size_t>(nz, 1);
        const size_t o_table = 0, b_table = cl_align(slots * W * 4);
        size_t o_fin[5];
        total = b_table;
        for (int k = 0; k < 5; ++k) { o_fin[k] = total; if (pa) total += cl_align(slots * (k < 3 ? 4 : 8)); }
        ClsScratch s;
        if (int rc = s.get(fn, total, st, "the zone table (4 (K + 3) bytes per zone, 28 more with planes)")) return rc;
        uint32_t *tab = (uint32_t *)(s.p + o_table);
        MHS_HIP(hipMemsetAsync(tab, 0, b_table, st));
        ClsZoneFin f{};
        if (pa) f = ClsZoneFin{(int32_t *)(s.p + o_fin[0]), (int32_t *)(s.p + o_fin[1]), (int32_t *)(s.p + o_fin[2]), (double *)(s.p + o_fin[3]),
                               (double *)(s.p + o_fin[4])};
        if (nz > 0) {
            const int strip_rows = CLS_TILE_ROWS * CLS_STRIP_TILES;
            const int tiles_c = (p.ncol + CLS_TILE_COLS - 1) / CLS_TILE_COLS;
            const unsigned nb = (unsigned)tiles_c * (unsigned)((p.nrow + strip_rows - 1) / strip_rows);
            CL_BY_DTYPE(dtype, class_zone_kernel, nb, 0, st, p, zones, ldq, nz, ix, tiles_c, strip_rows, tab, counters);
            ClsTableOut t{};
            if (ta) t = ClsTableOut{table->counts, table->n, table->other, table->cells, table->mode, table->variety, table->mode_frac, table->simpson, table->frac};
            hipLaunchKernelGGL(class_zone_finish_kernel, dim3(cl_blocks(nz)), dim3(CL_NT), 0, st, nz, ix, sel, tab, t, f, (const ClsCounters *)counters);
            MHS_HIP(hipGetLastError());
        }
        if (pa) {
            hipLaunchKernelGGL(class_zone_planes_kernel, dim3(cl_blocks(n)), dim3(CL_NT), 0, st, p.nrow, p.ncol, zones, ldq, nz, ix.K, sel,
                               (const uint32_t *)tab, f, class_out(planes), (const ClsCounters *)counters);
            MHS_HIP(hipGetLastError());
        }
        if (!info) {                                                       // the device flag: the zone plane was not measured
            MHS_HIP(hipMemcpyAsync(&c, counters, sizeof(c), hipMemcpyDeviceToHost, st));
            MHS_HIP(hipStreamSynchronize(st));
            CL_REQUIRE(!c.bad, "%s: the zone plane holds a zone that is not below n_zones %lld", fn, (long long)n_zones);
        }
    }
    class_info(info, ix, n_zones, c, total + CL_HEAD);
    return MHS_OK;
}

// ---- aggregate
static int aggregate_check(const char *fn, const mhs_grid *sg, const mhs_stack *ss, int layer, const mhs_grid *tg, const int32_t *classes, int n_classes,
                           const int32_t *frac_of, int n_frac, const mhs_class_planes *planes, bool dev, const mhs_class_info *info, RsSrc *S, RsGrid *T,
                           ClsIndex *ix) {
    if (int rc = rs_check_src(fn, sg, ss, S)) return rc;
    if (int rc = rs_check_grid(fn, "target", tg, T)) return rc;
    CL_REQUIRE(layer >= 0 && layer < ss->n_layers, "%s: layer %d is not one of the stack's %d layers", fn, layer, ss->n_layers);
    CL_REQUIRE(sg->nrow * sg->ncol <= (int64_t)INT32_MAX, "%s: source grid too large: nrow * ncol must not pass 2^31 - 1", fn);
    CL_REQUIRE(tg->nrow * tg->ncol <= (int64_t)INT32_MAX, "%s: target grid too large: nrow * ncol must not pass 2^31 - 1", fn);
    const bool pa = class_planes_any(planes);
    if (int rc = class_check_list(fn, classes, n_classes, frac_of, n_frac, pa && planes->frac, ix)) return rc;
    CL_REQUIRE(pa || info, "%s: no output: planes names no plane and info is NULL", fn);
    return class_check_planes(fn, planes, tg->nrow, tg->ncol, n_frac ? n_frac : n_classes, dev, true);
}

// The tile of class_aggregate_kernel for K classes on an nrow x ncol target.  The LDS budget allows floor(CLS_AGG_WORDS / (K + 2))
// cells, at most CLS_AGG_SIDE a side; but a workgroup reads its whole footprint with four waves, so a target of few tiles leaves
// most of the device idle (measured: 203 tiles of 14 x 64 cells took 2.07 ms over 10^8 source cells).  The tile is therefore
// halved, rows first, then columns down to CLS_AGG_MIN_COLS, while there are fewer than CLS_AGG_MIN_TILES tiles.
static int64_t aggregate_tiles(int nrow, int ncol, int tr, int tc) { return (int64_t)((nrow + tr - 1) / tr) * ((ncol + tc - 1) / tc); }
static void aggregate_tile(int K, int nrow, int ncol, int *tr, int *tc) {
    const int cap = CLS_AGG_WORDS / (K + 2);
    *tc = std::min(std::min(ncol, cap), CLS_AGG_SIDE);
    *tr = std::max(1, std::min(std::min(nrow, cap / *tc), CLS_AGG_SIDE));
    while (*tr > 1 && aggregate_tiles(nrow, ncol, *tr, *tc) < CLS_AGG_MIN_TILES) *tr = (*tr + 1) / 2;
    while (*tc > CLS_AGG_MIN_COLS && aggregate_tiles(nrow, ncol, *tr, *tc) < CLS_AGG_MIN_TILES) *tc = (*tc + 1) / 2;
}

// class_aggregate_kernel<T> may take CLS_AGG_WORDS words of dynamic LDS beside its static arrays (more than the default limit of
// 64 KiB together): said to the runtime once per process and instantiation, not on every call
template <typename T>
static int aggregate_lds_limit() {
    static std::once_flag once;
    static hipError_t err = hipSuccess;
    std::call_once(once, [] { err = hipFuncSetAttribute((const void *)class_aggregate_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, CLS_AGG_WORDS * 4); });
    MHS_HIP(err);
    return MHS_OK;
}

static int aggregate_run(const char *fn, const RsSrc &S, const RsGrid &T, int dtype, const void *plane, ClsIndex ix, const int32_t *frac_of, int n_frac,
                         const mhs_class_planes *planes, hipStream_t st, mhs_class_info *info) {
    ClsPlane p{plane, S.ld, S.g.nrow, S.g.ncol, S.nodata, S.has_nodata};
    ClsCounters c;
    std::memset(&c, 0, sizeof(c));
    size_t scratch = 0;
    if (ix.K == 0 || info) {
        ClsScratch head;
        if (int rc = head.get(fn, CL_HEAD, st, "the counter block and the presence map")) return rc;
        MHS_HIP(hipMemsetAsync(head.p, 0, CL_HEAD, st));
        if (int rc = class_census(fn, p, dtype, &ix, head.p, st, &c)) return rc;
        scratch = CL_HEAD;
    }
    class_set_form(&ix);
    ClsFracSel sel;
    if (int rc = class_select(fn, ix, frac_of, n_frac, &sel)) return rc;
    if (class_planes_any(planes)) {
        int tr, tc;
        aggregate_tile(ix.K, T.nrow, T.ncol, &tr, &tc);
        const int tiles_c = (T.ncol + tc - 1) / tc, tiles_r = (T.nrow + tr - 1) / tr;
        const size_t lds = (size_t)tr * tc * (ix.K + 2) * 4;
        const ClsOut o = class_out(planes);
        const unsigned nb = (unsigned)tiles_c * (unsigned)tiles_r;
        if (int rc = dtype == MHS_F64 ? aggregate_lds_limit<double>() : dtype == MHS_F32 ? aggregate_lds_limit<float>() : aggregate_lds_limit<short>()) return rc;
        CL_BY_DTYPE(dtype, class_aggregate_kernel, nb, lds, st, p, S.g, T, ix, sel, tr, tc, tiles_c, o);
    }
    class_info(info, ix, 0, c, scratch);
    return MHS_OK;
}

// ---- focal
static int focal_run_classes(const char *fn, const mhs_grid *grid, ClsPlane p, int dtype, int radius, int shape, ClsIndex ix, const int32_t *frac_of,
                             int n_frac, const mhs_class_planes *planes, void *stream, mhs_class_info *info) {
    hipStream_t st = pick_stream(stream);
    const size_t n = (size_t)p.nrow * (size_t)p.ncol;
    ClsCounters c;
    std::memset(&c, 0, sizeof(c));
    const bool pa = class_planes_any(planes);                             // an info-only call takes the counter block and the presence map alone
    const size_t o_ind = cl_align(CL_HEAD), o_sum = o_ind + cl_align(n * 2), o_bc = o_sum + cl_align(n * 16), o_bk = o_bc + cl_align(n * 4),
                 o_var = o_bk + cl_align(n * 4), total = pa ? o_var + cl_align(n * 4) : CL_HEAD;
    ClsScratch s;
    if (int rc = s.get(fn, total, st, "the indicator, two window sums and the running mode (30 bytes per cell)")) return rc;
    MHS_HIP(hipMemsetAsync(s.p, 0, CL_HEAD, st));
    if (ix.K == 0 || info)
        if (int rc = class_census(fn, p, dtype, &ix, s.p, st, &c)) return rc;
    class_set_form(&ix);
    ClsFracSel sel;
    if (int rc = class_select(fn, ix, frac_of, n_frac, &sel)) return rc;
    if (pa) {
        int16_t *ind = (int16_t *)(s.p + o_ind);
        double *win_n = (double *)(s.p + o_sum), *sum = win_n + n;         // focal's planes: count, then sum
        uint32_t *best_count = (uint32_t *)(s.p + o_bc);
        int32_t *best_code = (int32_t *)(s.p + o_bk), *variety = (int32_t *)(s.p + o_var);
        const ClsOut o = class_out(planes);
        const mhs_stack is{ind, 1, MHS_I16, (int64_t)n, p.ncol, -1.0};
        const unsigned nb = cl_blocks(n);
        for (int k = 0; k < ix.K; ++k) {
            CL_BY_DTYPE(dtype, class_indicator_kernel, nb, 0, st, p, (int)ix.codes[k], ind);
            // the window count of class k: focal's sum of 0 / 1 values at offset 0 (k = 0 also takes its count: the window's n)
            const unsigned stats = k == 0 ? 3u : 2u;
            if (int rc = mhs_focal_dev(grid, &is, 0, &radius, 1, shape, stats, 0, 0.0, 0, p.nrow, 0, p.ncol, k == 0 ? (void *)win_n : (void *)sum, MHS_F64,
                                       p.ncol, (int64_t)n, stream)) {
                // the composed step failed (its own scratch, say): reported under this entry's name, with the step's message behind it
                char inner[512];
                std::snprintf(inner, sizeof(inner), "%s", mhs_last_error());
                set_error("%s: the window sum of class %d (code %d) failed: %s", fn, k, (int)ix.codes[k], inner);
                return rc;
            }
            void *fp = nullptr;                                            // the frac plane of class k, if asked for (a code is named once)
            if (o.frac)
                for (int j = 0; j < sel.n; ++j)
                    if (sel.k[j] == k)
                        fp = o.f64 ? (void *)((double *)o.frac + (int64_t)j * o.frac_stride) : (void *)((float *)o.frac + (int64_t)j * o.frac_stride);
            hipLaunchKernelGGL(class_window_update_kernel, dim3(nb), dim3(CL_NT), 0, st, (int64_t)n, p.ncol, k == 0 ? 1 : 0, (int)ix.codes[k], (const double *)sum,
                               (const double *)win_n, best_count, best_code, variety, fp, o.ld, o.f64);
            MHS_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(class_window_finish_kernel, dim3(nb), dim3(CL_NT), 0, st, (int64_t)n, p.ncol, (const double *)win_n, (const uint32_t *)best_count,
                           (const int32_t *)best_code, (const int32_t *)variety, o);
        MHS_HIP(hipGetLastError());
    }
    class_info(info, ix, 0, c, total);
    return MHS_OK;
}

// host staging of the two host-pointer entries: the outputs of a call on the device, and their way down
struct ClsStage {
    struct Item { void *host; size_t off, bytes; };
    Item items[16];
    int n_items = 0;
    size_t total = 0;
    size_t add(void *host, size_t bytes) {
        const size_t o = total;
        if (host) { items[n_items++] = Item{host, o, bytes}; total += cl_align(bytes); }
        return o;
    }
};

}  // namespace mhs

using namespace mhs;

extern "C" {

int mhs_class_crosstab_dev(const mhs_grid *g, const mhs_stack *stack, int layer, const int32_t *zones, int64_t ld_zones, int64_t n_zones,
                           const int32_t *classes, int n_classes, const int32_t *frac_of, int n_frac_of, const mhs_class_table *table,
                           const mhs_class_planes *planes, void *stream, mhs_class_info *info) {
    ClsPlane p;
    ClsIndex ix;
    if (int rc = crosstab_check(__func__, g, stack, layer, zones, ld_zones, n_zones, classes, n_classes, frac_of, n_frac_of, table, planes, true, info, &p, &ix))
        return rc;
    if (int rc = require_ready()) return rc;
    p.z = (const char *)stack->data + (size_t)layer * stack->plane_stride * dtype_bytes(stack->dtype);
    return crosstab_run(__func__, p, stack->dtype, zones, ld_zones, n_zones, ix, frac_of, n_frac_of, table, planes, pick_stream(stream), info);
}

// Host planes: the layer and the zone plane go up whole, the table's rows and the planes come down.
int mhs_class_crosstab(const mhs_grid *g, const mhs_stack *stack, int layer, const int32_t *zones, int64_t n_zones, const int32_t *classes, int n_classes,
                       const int32_t *frac_of, int n_frac_of, const mhs_class_table *table, const mhs_class_planes *planes, mhs_class_info *info) {
    const char *fn = __func__;
    ClsPlane p;
    ClsIndex ix;
    if (int rc = crosstab_check(fn, g, stack, layer, zones, g ? g->ncol : 0, n_zones, classes, n_classes, frac_of, n_frac_of, table, planes, false, info, &p, &ix))
        return rc;
    const bool ta = class_table_any(table), pa = class_planes_any(planes);
    CL_REQUIRE(!ta || n_zones > 0, "%s: a table on the host needs n_zones: its rows must be known (measure with info first)", fn);
    CL_REQUIRE(!((ta && table->frac) || (pa && planes->frac)) || n_classes > 0 || n_frac_of > 0, "%s: frac needs classes or frac_of", fn);
    if (int rc = require_ready()) return rc;
    const size_t esz = dtype_bytes(stack->dtype), n = (size_t)p.nrow * (size_t)p.ncol;
    const size_t in_bytes = ((size_t)(p.nrow - 1) * stack->ld + p.ncol) * esz;
    const size_t rows = ta ? (size_t)n_zones : 0, nf = n_frac_of ? (size_t)n_frac_of : (size_t)n_classes, fsz = pa && planes->dtype == MHS_F32 ? 4 : 8;
    ClsStage sg;
    sg.total = cl_align(in_bytes);
    const size_t o_zones = sg.total;
    sg.total += cl_align(4 * n);
    mhs_class_table dt;
    mhs_class_planes dp;
    std::memset(&dt, 0, sizeof(dt));
    std::memset(&dp, 0, sizeof(dp));
    size_t off[15];
    if (ta) {
        off[0] = sg.add(table->counts, 4 * rows * n_classes); off[1] = sg.add(table->n, 4 * rows); off[2] = sg.add(table->other, 4 * rows);
        off[3] = sg.add(table->cells, 4 * rows); off[4] = sg.add(table->mode, 4 * rows); off[5] = sg.add(table->variety, 4 * rows);
        off[6] = sg.add(table->mode_frac, 8 * rows); off[7] = sg.add(table->simpson, 8 * rows); off[8] = sg.add(table->frac, 8 * rows * nf);
    }
    if (pa) {
        off[9] = sg.add(planes->mode, 4 * n); off[10] = sg.add(planes->variety, 4 * n); off[11] = sg.add(planes->n, 4 * n);
        off[12] = sg.add(planes->mode_frac, fsz * n); off[13] = sg.add(planes->simpson, fsz * n); off[14] = sg.add(planes->frac, fsz * n * nf);
    }
    std::lock_guard<std::mutex> lk(pipe_mutex());
    if (int rc = host_pipe(0)) return rc;                      // the pipeline's streams; its arena is not used
    hipStream_t st = ctx().pipe_comp;
    ClsScratch s;
    if (int rc = s.get(fn, sg.total, st, "the layer, the zone plane and the outputs")) return rc;
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{st};   // no copy is left in flight, whatever the exit
    MHS_HIP(hipMemcpyAsync(s.p, (const char *)stack->data + (size_t)layer * stack->plane_stride * esz, in_bytes, hipMemcpyHostToDevice, st));
    MHS_HIP(hipMemcpyAsync(s.p + o_zones, zones, 4 * n, hipMemcpyHostToDevice, st));
    auto at = [&](const void *host, size_t o) { return host ? (void *)(s.p + o) : nullptr; };
    if (ta)
        dt = mhs_class_table{(int64_t)rows, (int32_t *)at(table->counts, off[0]), (int32_t *)at(table->n, off[1]), (int32_t *)at(table->other, off[2]),
                             (int32_t *)at(table->cells, off[3]), (int32_t *)at(table->mode, off[4]), (int32_t *)at(table->variety, off[5]),
                             (double *)at(table->mode_frac, off[6]), (double *)at(table->simpson, off[7]), (double *)at(table->frac, off[8])};
    if (pa)
        dp = mhs_class_planes{(int32_t *)at(planes->mode, off[9]), (int32_t *)at(planes->variety, off[10]), (int32_t *)at(planes->n, off[11]),
                              at(planes->mode_frac, off[12]), at(planes->simpson, off[13]), at(planes->frac, off[14]), (int64_t)p.ncol, (int64_t)n,
                              planes->dtype};
    p.z = s.p;
    mhs_class_info mine;
    if (int rc = crosstab_run(fn, p, stack->dtype, (const int32_t *)(s.p + o_zones), p.ncol, n_zones, ix, frac_of, n_frac_of, ta ? &dt : nullptr,
                              pa ? &dp : nullptr, st, &mine))
        return rc;
    for (int i = 0; i < sg.n_items; ++i)
        if (sg.items[i].bytes) MHS_HIP(hipMemcpyAsync(sg.items[i].host, s.p + sg.items[i].off, sg.items[i].bytes, hipMemcpyDeviceToHost, st));
    MHS_HIP(hipStreamSynchronize(st));
    if (info) *info = mine;
    return MHS_OK;
}

int mhs_class_aggregate_dev(const mhs_grid *src_grid, const mhs_stack *src_stack, int layer, const mhs_grid *dst_grid, const int32_t *classes, int n_classes,
                            const int32_t *frac_of, int n_frac_of, const mhs_class_planes *planes, void *stream, mhs_class_info *info) {
    RsSrc S;
    RsGrid T;
    ClsIndex ix;
    if (int rc = aggregate_check(__func__, src_grid, src_stack, layer, dst_grid, classes, n_classes, frac_of, n_frac_of, planes, true, info, &S, &T, &ix)) return rc;
    if (int rc = require_ready()) return rc;
    const void *plane = (const char *)src_stack->data + (size_t)layer * src_stack->plane_stride * dtype_bytes(src_stack->dtype);
    return aggregate_run(__func__, S, T, src_stack->dtype, plane, ix, frac_of, n_frac_of, planes, pick_stream(stream), info);
}

// Host planes: the layer goes up whole, the target planes come down.
int mhs_class_aggregate(const mhs_grid *src_grid, const mhs_stack *src_stack, int layer, const mhs_grid *dst_grid, const int32_t *classes, int n_classes,
                        const int32_t *frac_of, int n_frac_of, const mhs_class_planes *planes, mhs_class_info *info) {
    const char *fn = __func__;
    RsSrc S;
    RsGrid T;
    ClsIndex ix;
    if (int rc = aggregate_check(fn, src_grid, src_stack, layer, dst_grid, classes, n_classes, frac_of, n_frac_of, planes, false, info, &S, &T, &ix)) return rc;
    if (int rc = require_ready()) return rc;
    const bool pa = class_planes_any(planes);
    const size_t esz = dtype_bytes(src_stack->dtype), n = (size_t)T.nrow * (size_t)T.ncol;
    const size_t in_bytes = ((size_t)(S.g.nrow - 1) * src_stack->ld + S.g.ncol) * esz;
    const size_t nf = n_frac_of ? (size_t)n_frac_of : (size_t)n_classes, fsz = pa && planes->dtype == MHS_F32 ? 4 : 8;
    ClsStage sg;
    sg.total = cl_align(in_bytes);
    size_t off[6] = {0, 0, 0, 0, 0, 0};
    if (pa) {
        off[0] = sg.add(planes->mode, 4 * n); off[1] = sg.add(planes->variety, 4 * n); off[2] = sg.add(planes->n, 4 * n);
        off[3] = sg.add(planes->mode_frac, fsz * n); off[4] = sg.add(planes->simpson, fsz * n); off[5] = sg.add(planes->frac, fsz * n * nf);
    }
    std::lock_guard<std::mutex> lk(pipe_mutex());
    if (int rc = host_pipe(0)) return rc;
    hipStream_t st = ctx().pipe_comp;
    ClsScratch s;
    if (int rc = s.get(fn, sg.total, st, "the layer and the outputs")) return rc;
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{st};
    MHS_HIP(hipMemcpyAsync(s.p, (const char *)src_stack->data + (size_t)layer * src_stack->plane_stride * esz, in_bytes, hipMemcpyHostToDevice, st));
    auto at = [&](const void *host, size_t o) { return host ? (void *)(s.p + o) : nullptr; };
    mhs_class_planes dp;
    std::memset(&dp, 0, sizeof(dp));
    if (pa)
        dp = mhs_class_planes{(int32_t *)at(planes->mode, off[0]), (int32_t *)at(planes->variety, off[1]), (int32_t *)at(planes->n, off[2]),
                              at(planes->mode_frac, off[3]), at(planes->simpson, off[4]), at(planes->frac, off[5]), (int64_t)T.ncol, (int64_t)n, planes->dtype};
    mhs_class_info mine;
    if (int rc = aggregate_run(fn, S, T, src_stack->dtype, s.p, ix, frac_of, n_frac_of, pa ? &dp : nullptr, st, &mine)) return rc;
    for (int i = 0; i < sg.n_items; ++i)
        if (sg.items[i].bytes) MHS_HIP(hipMemcpyAsync(sg.items[i].host, s.p + sg.items[i].off, sg.items[i].bytes, hipMemcpyDeviceToHost, st));
    MHS_HIP(hipStreamSynchronize(st));
    if (info) *info = mine;
    return MHS_OK;
}

int mhs_class_focal_dev(const mhs_grid *g, const mhs_stack *stack, int layer, int radius, int shape, const int32_t *classes, int n_classes,
                        const int32_t *frac_of, int n_frac_of, const mhs_class_planes *planes, void *stream, mhs_class_info *info) {
    const char *fn = __func__;
    ClsPlane p;
    ClsIndex ix;
    if (int rc = class_check_layer(fn, g, stack, layer, &p)) return rc;
    CL_REQUIRE(radius >= 1 && (int64_t)radius <= std::max(g->nrow, g->ncol), "%s: radius %d is not in 1 .. max(nrow, ncol) = %lld", fn, radius,
               (long long)std::max(g->nrow, g->ncol));
    CL_REQUIRE(shape == MHS_FOCAL_SQUARE || shape == MHS_FOCAL_CIRCLE, "%s: unknown shape %d", fn, shape);
    const bool pa = class_planes_any(planes);
    if (int rc = class_check_list(fn, classes, n_classes, frac_of, n_frac_of, pa && planes->frac, &ix)) return rc;
    for (int j = 0; j < n_frac_of; ++j)
        for (int i = 0; i < j; ++i) CL_REQUIRE(frac_of[i] != frac_of[j], "%s: frac_of names code %d twice", fn, frac_of[j]);
    CL_REQUIRE(pa || info, "%s: no output: planes names no plane and info is NULL", fn);
    if (int rc = class_check_planes(fn, planes, g->nrow, g->ncol, n_frac_of ? n_frac_of : n_classes, true, false)) return rc;
    if (int rc = require_ready()) return rc;
    p.z = (const char *)stack->data + (size_t)layer * stack->plane_stride * dtype_bytes(stack->dtype);
    return focal_run_classes(fn, g, p, stack->dtype, radius, shape, ix, frac_of, n_frac_of, planes, stream, info);
}

}  // extern "C"
