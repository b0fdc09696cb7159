// Zonal quantiles of one layer (include/machisplin_hip.h, section "zonal quantiles", states the rule; quantile_rule.h holds it):
// R's type 7 quantile per zone, per coarse cell of a target grid, or of the whole layer, and a cell's rank inside its zone.  A
// quantile needs the values in order, so the cells' (zone, q) keys are SORTED by the deterministic radix sort of sort_keys.hip;
// everything behind the sort is a look-up in the sorted keys.
//
// Every phase is its own launch on the stream, a kernel boundary the only ordering between phases.
//   0   quantile_zones_kernel   only without a zone plane: the zone of every cell as an int32 plane, written INTO THE SECOND KEY
//                               BUFFER (free until the sort begins), so that phase 1 is zonal's own and costs no scratch
//   1   zonal_measure           zonal.hip's range and zone check, reused: max|v|, max(zone) + 1, the +-Inf cells.  Always run:
//                               a zone >= n_zones or a quantum that does not fit is refused here, before anything is written
//   2   quantile_keys_kernel    a lane per cell: key = (zone << 32) | (q + 2^30); a cell that does not contribute gets the
//                               SENTINEL (n_zones << 32), which sorts last.  The info's counts are summed here
//   3   sort_keys_run           bits 0 .. 32 + bits(n_zones); the host reads back the number m of contributing cells
//   4   quantile_heads_kernel   place i < m is a segment head when its zone differs from place i - 1's: heads per block of
//       quantile_scan_kernel    QT_BLOCK places, their exclusive prefix sum (one workgroup),
//       quantile_rows_kernel    and per head its row: zone, count (a bisection for the zone's end) and quantiles -- the PRESENT
//                               table, with no array of n_zones slots
//   4'  quantile_starts_kernel  a lane per zone slot, only for a dense table or planes: the zone's first place, by bisection
//       quantile_dense_kernel   the DENSE table from the starts
//   5   (quantiles are read straight from the sorted keys by 4, 4' and 6: s[lo], s[hi] of quantile_type7)
//   6   quantile_planes_kernel  a lane per cell: its zone's quantiles, and `below` by a lower-bound bisection for its own key
//                               inside its zone's segment
//
// Scratch, stream-ordered: the counter block (256 bytes); one block of two key buffers (8 bytes per cell each), the sort's
// per-tile digit counts (SORT_TILE_BYTES per SORT_TILE_KEYS cells) and histograms, 4 bytes per QT_BLOCK cells for a present
// table, 4 bytes per source row and column with a target; and 4 bytes per zone slot (+ 1) ONLY for a dense table or planes.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>
#include "proximity_rule.h"
#include "quantile_rule.h"
#include "resample_rule.h"
#include "zonal_int.h"

namespace mhs {

constexpr int QT_NT = 256;
constexpr int QT_WAVES = QT_NT / 64;
constexpr int QT_ROUNDS = 8;
constexpr int QT_BLOCK = QT_NT * QT_ROUNDS;          // places per block of the heads' prefix sum
static_assert(MHS_QUANTILE_MAX_PROBS == QUANTILE_MAX_PROBS, "the header and the rule agree");

// where a cell's zone comes from: a plane, the footprints of a target grid (two index tables), or zone 0 everywhere
struct QZones {
    const int32_t *zones;
    int64_t ld;
    const int32_t *col_zone, *row_zone;      // target column of a source column, target row of a source row; -1: none
    int tcols;
};
__device__ inline int qt_zone(const QZones &z, int64_t r, int64_t c) {
    if (z.zones) return z.zones[r * z.ld + c];
    if (!z.col_zone) return 0;
    const int tr = z.row_zone[r], tc = z.col_zone[c];
    return tr < 0 || tc < 0 ? -1 : tr * z.tcols + tc;
}

struct QProbs {
    double p[QUANTILE_MAX_PROBS];
    int n;
};
struct QPlaneOut {
    void *q[QUANTILE_MAX_PROBS];
    int64_t ld_q[QUANTILE_MAX_PROBS];
    int32_t *below;
    void *frac;
    int64_t ld_below, ld_frac;
};
struct QTable {
    int32_t *zone;
    int64_t *count;
    double *q;
    int64_t capacity;
};

struct QKeys {
    const uint64_t *k;
    MHS_ZONAL_HD uint64_t operator()(int64_t i) const { return k[i]; }
};
struct QSegment {                                      // the q of place i of a zone's segment
    const uint64_t *k;
    MHS_ZONAL_HD int32_t operator()(int64_t i) const { return quantile_key_q(k[i]); }
};

__device__ inline unsigned qt_wave_sum(unsigned v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// 0
__global__ __launch_bounds__(QT_NT) void quantile_zones_kernel(const int nrow, const int ncol, const QZones z, int32_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * QT_NT + threadIdx.x;
    if (i >= (int64_t)nrow * ncol) return;
    const int64_t r = i / ncol, c = i - r * ncol;
    out[i] = qt_zone(z, r, c);
}

// 2
template <typename T>
__global__ __launch_bounds__(QT_NT) void quantile_keys_kernel(const ZonalGeom g, const T *__restrict__ v_, const int64_t ldz, const QZones z, const unsigned nz,
                                                              const double quantum, uint64_t *__restrict__ keys, ZonalCounters *counters) {
    const int64_t i = (int64_t)blockIdx.x * QT_NT + threadIdx.x;
    unsigned in_zone = 0, contrib = 0, inexact = 0;
    if (i < (int64_t)g.nrow * g.ncol) {
        const int64_t r = i / g.ncol, c = i - r * g.ncol;
        const int zn = qt_zone(z, r, c);
        uint64_t key = quantile_sentinel(nz);
        if (zn >= 0 && (unsigned)zn < nz) {
            in_zone = 1;
            const double v = (double)v_[r * ldz + c];
            if (!prox_na(v, g.has_nodata != 0, g.nodata) && zn_finite(v) && zonal_fits(v, quantum)) {
                const int32_t q = zonal_q(v, quantum);
                if ((double)q * quantum != v) inexact = 1;
                contrib = 1;
                key = quantile_key((uint32_t)zn, q);
            }
        }
        keys[i] = key;
    }
    in_zone = qt_wave_sum(in_zone);
    contrib = qt_wave_sum(contrib);
    inexact = qt_wave_sum(inexact);
    if ((threadIdx.x & 63) == 0) {
        if (in_zone) atomicAdd(&counters->n_in_zone, (unsigned long long)in_zone);
        if (contrib) atomicAdd(&counters->n_contrib, (unsigned long long)contrib);
        if (inexact) atomicAdd(&counters->n_inexact, (unsigned long long)inexact);
    }
}

__device__ inline bool qt_is_head(const uint64_t *__restrict__ keys, const int64_t i, const int64_t m) {
    return i < m && (i == 0 || quantile_key_zone(keys[i]) != quantile_key_zone(keys[i - 1]));
}

// 4, the blocks' numbers of heads
__global__ __launch_bounds__(QT_NT) void quantile_heads_kernel(const uint64_t *__restrict__ keys, const int64_t m, int32_t *__restrict__ block_count,
                                                               ZonalCounters *counters) {
    __shared__ unsigned part[QT_WAVES];
    const int64_t base = (int64_t)blockIdx.x * QT_BLOCK;
    unsigned k = 0;
#pragma unroll
    for (int j = 0; j < QT_ROUNDS; ++j) k += qt_is_head(keys, base + j * QT_NT + threadIdx.x, m) ? 1u : 0u;
    k = qt_wave_sum(k);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = k;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned s = 0;
        for (int w = 0; w < QT_WAVES; ++w) s += part[w];
        if (block_count) block_count[blockIdx.x] = (int32_t)s;
        if (s) atomicAdd(&counters->n_present, (unsigned long long)s);
    }
}

// 4, one workgroup: block_count becomes its own exclusive prefix sum, chunk by chunk with a carry
__global__ __launch_bounds__(QT_NT) void quantile_scan_kernel(const unsigned n_blocks, int32_t *block_count) {
    __shared__ int wave_total[QT_WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int carry = 0;
    for (unsigned base = 0; base < n_blocks; base += QT_NT) {
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
        for (int w = 0; w < QT_WAVES; ++w) {
            if (w < wave) before += wave_total[w];
            total += wave_total[w];
        }
        if (i < n_blocks) block_count[i] = carry + before + incl - v;
        carry += total;
        __syncthreads();
    }
}

__device__ inline void qt_quantiles(const uint64_t *__restrict__ keys, const int64_t start, const int64_t cnt, const QProbs &pr, const double quantum,
                                    double *__restrict__ out) {
    const QSegment seg{keys + start};
    for (int j = 0; j < pr.n; ++j) out[j] = cnt > 0 ? quantile_type7(seg, cnt, pr.p[j], quantum) : zonal_nan();
}

// 4, the rows of the present table: wave w of a block holds places w * 512 + j * 64 + lane in round j, in place order
__global__ __launch_bounds__(QT_NT) void quantile_rows_kernel(const uint64_t *__restrict__ keys, const int64_t m, const int32_t *__restrict__ block_before,
                                                              const QProbs pr, const double quantum, const QTable t) {
    __shared__ int count[QT_WAVES * QT_ROUNDS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * QT_BLOCK + wave * (QT_BLOCK / QT_WAVES);
    uint64_t heads[QT_ROUNDS];
#pragma unroll
    for (int j = 0; j < QT_ROUNDS; ++j) {
        heads[j] = __ballot(qt_is_head(keys, base + j * 64 + lane, m));
        if (lane == 0) count[wave * QT_ROUNDS + j] = __popcll(heads[j]);
    }
    __syncthreads();
    const int first = block_before[blockIdx.x];
#pragma unroll
    for (int j = 0; j < QT_ROUNDS; ++j) {
        if (!((heads[j] >> lane) & 1)) continue;
        int64_t row = first;
        for (int q = 0; q < wave * QT_ROUNDS + j; ++q) row += count[q];
        row += __popcll(heads[j] & ((1ull << lane) - 1));
        if (row >= t.capacity) continue;                                   // the call then fails, naming capacity
        const int64_t i = base + j * 64 + lane;
        const uint32_t zn = quantile_key_zone(keys[i]);
        const int64_t end = quantile_lower_bound(QKeys{keys}, i, m, (uint64_t)(zn + 1u) << 32);
        t.zone[row] = (int32_t)zn;
        if (t.count) t.count[row] = end - i;
        if (t.q) qt_quantiles(keys, i, end - i, pr, quantum, t.q + row * pr.n);
    }
}

// 4', start[z] = the first place of zone z among the m contributing places, z = 0 .. nz (start[nz] = m)
__global__ __launch_bounds__(QT_NT) void quantile_starts_kernel(const uint64_t *__restrict__ keys, const int64_t m, const unsigned nz, int32_t *__restrict__ start) {
    const uint64_t z = (uint64_t)blockIdx.x * QT_NT + threadIdx.x;
    if (z > nz) return;
    start[z] = (int32_t)quantile_lower_bound(QKeys{keys}, 0, m, z << 32);
}

__global__ __launch_bounds__(QT_NT) void quantile_dense_kernel(const uint64_t *__restrict__ keys, const unsigned nz, const int32_t *__restrict__ start,
                                                               const QProbs pr, const double quantum, const QTable t) {
    const uint64_t z = (uint64_t)blockIdx.x * QT_NT + threadIdx.x;
    if (z >= nz) return;
    const int64_t a = start[z], cnt = start[z + 1] - a;
    if (t.count) t.count[z] = cnt;
    if (t.q) qt_quantiles(keys, a, cnt, pr, quantum, t.q + z * pr.n);
}

// 6
template <typename T, typename O>
__global__ __launch_bounds__(QT_NT) void quantile_planes_kernel(const ZonalGeom g, const T *__restrict__ v_, const int64_t ldz, const QZones z, const unsigned nz,
                                                                const double quantum, const uint64_t *__restrict__ keys, const int32_t *__restrict__ start,
                                                                const QProbs pr, const QPlaneOut o) {
    const int64_t i = (int64_t)blockIdx.x * QT_NT + threadIdx.x;
    if (i >= (int64_t)g.nrow * g.ncol) return;
    const int64_t r = i / g.ncol, c = i - r * g.ncol;
    const int zn = qt_zone(z, r, c);
    const bool in = zn >= 0 && (unsigned)zn < nz;
    const double na = zonal_nan();
    int64_t a = 0, cnt = 0;
    if (in) { a = start[zn]; cnt = start[zn + 1] - a; }
    const QSegment seg{keys + a};
    for (int j = 0; j < pr.n; ++j)
        if (o.q[j]) ((O *)o.q[j])[r * o.ld_q[j] + c] = (O)(cnt > 0 ? quantile_type7(seg, cnt, pr.p[j], quantum) : na);
    if (!o.below && !o.frac) return;
    int32_t below = -1;
    if (in) {
        const double v = (double)v_[r * ldz + c];
        if (!prox_na(v, g.has_nodata != 0, g.nodata) && zn_finite(v) && zonal_fits(v, quantum))
            below = (int32_t)(quantile_lower_bound(QKeys{keys}, a, a + cnt, quantile_key((uint32_t)zn, zonal_q(v, quantum))) - a);
    }
    if (o.below) o.below[r * o.ld_below + c] = below;
    if (o.frac) ((O *)o.frac)[r * o.ld_frac + c] = (O)(below >= 0 ? quantile_frac_below(below, cnt) : na);
}

static bool qt_table_wanted(const mhs_quantile_table *t) { return t && (t->q || t->count); }
static bool qt_planes_wanted(const mhs_quantile_planes *p) {
    if (!p) return false;
    for (int j = 0; j < QUANTILE_MAX_PROBS; ++j)
        if (p->q[j]) return true;
    return p->below || p->frac_below;
}

struct QCall {
    ZonalGeom g;
    RsGrid S, T;             // the source grid and, with a target, the target
    int mode;                // 0: a zone plane, 1: a target's footprints, 2: the whole layer
};

// Every check of a quantile call, before any device call; fn = the entry point's name for the message
static int quantile_check(const char *fn, const mhs_grid *grid, const mhs_stack *stack, int layer, const int32_t *zones, int64_t ld_zones, int64_t n_zones,
                          double quantum, int flags, const double *probs, int n_probs, const mhs_grid *target, const mhs_quantile_table *table,
                          const mhs_quantile_planes *planes, bool dev, const mhs_quantile_info *info, QCall *call) {
    ZN_REQUIRE(grid && stack, "%s: NULL argument (g or stack)", fn);
    ZN_REQUIRE(grid->nrow > 0 && grid->ncol > 0 && grid->nrow <= (int64_t)INT32_MAX && grid->ncol <= (int64_t)INT32_MAX,
               "%s: bad grid geometry (nrow, ncol must be in 1 .. 2^31 - 1)", fn);
    ZN_REQUIRE(grid->nrow * grid->ncol <= (int64_t)INT32_MAX, "%s: grid too large: nrow * ncol must not pass 2^31 - 1", fn);
    ZN_REQUIRE(stack->data, "%s: stack data is NULL", fn);
    ZN_REQUIRE(stack->dtype == MHS_F64 || stack->dtype == MHS_F32 || stack->dtype == MHS_I16, "%s: bad stack dtype", fn);
    ZN_REQUIRE(layer >= 0 && layer < stack->n_layers, "%s: layer %d is not one of the stack's %d layers", fn, layer, stack->n_layers);
    ZN_REQUIRE(stack->ld >= grid->ncol && (stack->n_layers == 1 || stack->plane_stride >= stack->ld * (grid->nrow - 1) + grid->ncol),
               "%s: stack strides smaller than the grid", fn);
    ZN_REQUIRE(!(zones && target), "%s: zones and target are both given: a cell's zone is one or the other", fn);
    ZN_REQUIRE(!zones || ld_zones >= grid->ncol, "%s: ld_zones smaller than the grid width", fn);
    ZN_REQUIRE(n_zones >= 0 && n_zones <= (int64_t)INT32_MAX, "%s: n_zones must be 0 (measure it) or in 1 .. 2^31 - 1 (a zone is an int32)", fn);
    ZN_REQUIRE(zones || n_zones == 0, "%s: n_zones must be 0 without a zone plane (it follows from the target, or is 1)", fn);
    if (target) {
        ZN_REQUIRE(target->nrow > 0 && target->ncol > 0 && target->nrow <= (int64_t)INT32_MAX && target->ncol <= (int64_t)INT32_MAX &&
                       target->nrow * target->ncol <= (int64_t)INT32_MAX,
                   "%s: bad target geometry (nrow, ncol and nrow * ncol must be in 1 .. 2^31 - 1)", fn);
        ZN_REQUIRE(target->xres > 0.0 && target->yres > 0.0 && grid->xres > 0.0 && grid->yres > 0.0 && std::isfinite(target->xmin) &&
                       std::isfinite(target->ymax) && std::isfinite(grid->xmin) && std::isfinite(grid->ymax),
                   "%s: bad target or grid geometry (the resolutions must be positive, the origins finite)", fn);
    }
    ZN_REQUIRE(quantum == 0.0 || zonal_quantum_ok(quantum), "%s: quantum must be 0 (measure it) or a power of two in 2^-1022 .. 2^1023", fn);
    ZN_REQUIRE(flags == 0, "%s: unknown bit in flags", fn);
    ZN_REQUIRE(probs && n_probs >= 1 && n_probs <= QUANTILE_MAX_PROBS, "%s: probs must hold n_probs = 1 .. %d probabilities", fn, QUANTILE_MAX_PROBS);
    for (int j = 0; j < n_probs; ++j)
        ZN_REQUIRE(quantile_prob_ok(probs[j]), "%s: probs[%d] = %g is not in [0, 1] (NaN is refused)", fn, j, probs[j]);
    const bool tw = qt_table_wanted(table), pw = qt_planes_wanted(planes);
    ZN_REQUIRE(tw || pw || info, "%s: no output: the table names neither q nor count, planes no plane, and info is NULL", fn);
    ZN_REQUIRE(!table || tw || !table->zone, "%s: the table names neither q nor count (only zone is set)", fn);
    if (tw) {
        ZN_REQUIRE(table->capacity >= 0, "%s: the table's capacity must not be negative", fn);
        ZN_REQUIRE(!table->zone || info, "%s: a present table (zone is set) needs info: K comes back in info->n_present", fn);
        const int64_t known = zones ? n_zones : target ? target->nrow * target->ncol : 1;
        ZN_REQUIRE(table->zone || known <= table->capacity, "%s: n_zones %lld passes the dense table's capacity %lld", fn, (long long)known,
                   (long long)table->capacity);
    }
    if (pw) {
        ZN_REQUIRE(planes->dtype == MHS_F64 || planes->dtype == MHS_F32, "%s: the planes' dtype must be MHS_F64 or MHS_F32", fn);
        for (int j = n_probs; j < QUANTILE_MAX_PROBS; ++j) ZN_REQUIRE(!planes->q[j], "%s: plane q[%d] has no probability (n_probs is %d)", fn, j, n_probs);
        if (dev) {
            for (int j = 0; j < n_probs; ++j)
                ZN_REQUIRE(!planes->q[j] || planes->ld_q[j] >= grid->ncol, "%s: ld of plane q[%d] smaller than the grid width", fn, j);
            ZN_REQUIRE(!planes->below || planes->ld_below >= grid->ncol, "%s: ld of plane below smaller than the grid width", fn);
            ZN_REQUIRE(!planes->frac_below || planes->ld_frac_below >= grid->ncol, "%s: ld of plane frac_below smaller than the grid width", fn);
        }
    }
    call->g = ZonalGeom{(int)grid->nrow, (int)grid->ncol, stack->nodata, !std::isnan(stack->nodata),
                        (int)((grid->ncol + ZONAL_TILE_COLS - 1) / ZONAL_TILE_COLS)};
    call->S = RsGrid{grid->xmin, grid->ymax, grid->xres, grid->yres, (int)grid->nrow, (int)grid->ncol};
    call->T = target ? RsGrid{target->xmin, target->ymax, target->xres, target->yres, (int)target->nrow, (int)target->ncol} : call->S;
    call->mode = zones ? 0 : target ? 1 : 2;
    return MHS_OK;
}

template <typename T>
static void launch_quantile_planes(int out_dtype, unsigned nb, hipStream_t st, const ZonalGeom &g, const void *v, int64_t ldz, const QZones &z, unsigned nz,
                                   double quantum, const uint64_t *keys, const int32_t *start, const QProbs &pr, const QPlaneOut &o) {
    if (out_dtype == MHS_F64)
        hipLaunchKernelGGL((quantile_planes_kernel<T, double>), dim3(nb), dim3(QT_NT), 0, st, g, (const T *)v, ldz, z, nz, quantum, keys, start, pr, o);
    else
        hipLaunchKernelGGL((quantile_planes_kernel<T, float>), dim3(nb), dim3(QT_NT), 0, st, g, (const T *)v, ldz, z, nz, quantum, keys, start, pr, o);
}

// Device planes.  `plane` = element (0, 0) of the layer, of `dtype`, with the row stride ldz.
static int quantile_run(const char *fn, const QCall &call, int dtype, const void *plane, int64_t ldz, const int32_t *zones, int64_t ldq, int64_t n_zones,
                        double quantum, const double *probs, int n_probs, const mhs_quantile_table *table, const mhs_quantile_planes *planes,
                        hipStream_t st, mhs_quantile_info *info) {
    const ZonalGeom &g = call.g;
    const size_t n = (size_t)g.nrow * (size_t)g.ncol;
    const bool tw = qt_table_wanted(table), pw = qt_planes_wanted(planes);
    const bool present = tw && table->zone, dense = tw && !present;
    const unsigned nb_cells = (unsigned)((n + QT_NT - 1) / QT_NT);
    QProbs pr;
    std::memset(&pr, 0, sizeof(pr));
    pr.n = n_probs;
    for (int j = 0; j < n_probs; ++j) pr.p[j] = probs[j];
    ZonalScratch cs;
    if (int rc = cs.get(fn, 256, st, "the counter block")) return rc;
    ZonalCounters *counters = (ZonalCounters *)cs.p;
    MHS_HIP(hipMemsetAsync(counters, 0, 256, st));
    // the block of keys
    const size_t n_hblocks_max = (n + QT_BLOCK - 1) / QT_BLOCK;
    const size_t o_a = 0, o_b = sort_align(8 * n), o_counts = 2 * sort_align(8 * n);
    size_t total = o_counts + sort_counts_bytes((int64_t)n);
    const size_t o_blocks = total;
    if (present) total += zn_align(4 * n_hblocks_max);
    const size_t o_tabs = total;
    if (call.mode == 1) total += zn_align(4 * ((size_t)g.nrow + (size_t)g.ncol));
    ZonalScratch s;
    if (int rc = s.get(fn, total, st, "the two key buffers (16 bytes per cell) and the tiles' digit counts")) return rc;
    uint64_t *key_a = (uint64_t *)(s.p + o_a), *key_b = (uint64_t *)(s.p + o_b);
    // the zone of a cell
    QZones z{zones, ldq, nullptr, nullptr, 0};
    std::vector<int32_t> tabs;                                             // outlives its copy: phase 1 synchronises the stream
    if (call.mode == 1) {
        tabs.assign((size_t)g.nrow + (size_t)g.ncol, -1);
        for (int r = 0; r < call.T.nrow; ++r)
            for (int i = rs_foot_row(call.S, call.T, r), e = rs_foot_row(call.S, call.T, r + 1); i < e; ++i) tabs[(size_t)i] = r;
        for (int c = 0; c < call.T.ncol; ++c)
            for (int j = rs_foot_col(call.S, call.T, c), e = rs_foot_col(call.S, call.T, c + 1); j < e; ++j) tabs[(size_t)g.nrow + (size_t)j] = c;
        int32_t *dev = (int32_t *)(s.p + o_tabs);
        MHS_HIP(hipMemcpyAsync(dev, tabs.data(), 4 * tabs.size(), hipMemcpyHostToDevice, st));
        z.row_zone = dev;
        z.col_zone = dev + g.nrow;
        z.tcols = call.T.ncol;
        n_zones = (int64_t)call.T.nrow * call.T.ncol;
    } else if (call.mode == 2) {
        n_zones = 1;
    }
    // 0, 1
    const int32_t *zone_plane = zones;
    int64_t ld_plane = ldq;
    if (call.mode != 0) {
        hipLaunchKernelGGL(quantile_zones_kernel, dim3(nb_cells), dim3(QT_NT), 0, st, g.nrow, g.ncol, z, (int32_t *)key_b);
        MHS_HIP(hipGetLastError());
        zone_plane = (const int32_t *)key_b;
        ld_plane = g.ncol;
    }
    if (quantum == 0.0 && dtype == MHS_I16) quantum = 1.0;
    ZonalCounters c;
    std::memset(&c, 0, sizeof(c));
    if (int rc = zonal_measure(fn, g, dtype, plane, ldz, zone_plane, ld_plane, st, counters, &c, &n_zones, &quantum)) return rc;
    ZN_REQUIRE(!dense || n_zones <= table->capacity, "%s: n_zones %lld passes the dense table's capacity %lld", fn, (long long)n_zones,
               (long long)table->capacity);
    const unsigned nz = (unsigned)n_zones;
    const unsigned long long n_nonfinite = c.n_nonfinite;
    // 2
    if (dtype == MHS_F64)
        hipLaunchKernelGGL(quantile_keys_kernel<double>, dim3(nb_cells), dim3(QT_NT), 0, st, g, (const double *)plane, ldz, z, nz, quantum, key_a, counters);
    else if (dtype == MHS_F32)
        hipLaunchKernelGGL(quantile_keys_kernel<float>, dim3(nb_cells), dim3(QT_NT), 0, st, g, (const float *)plane, ldz, z, nz, quantum, key_a, counters);
    else
        hipLaunchKernelGGL(quantile_keys_kernel<short>, dim3(nb_cells), dim3(QT_NT), 0, st, g, (const short *)plane, ldz, z, nz, quantum, key_a, counters);
    MHS_HIP(hipGetLastError());
    MHS_HIP(hipMemcpyAsync(&c, counters, sizeof(c), hipMemcpyDeviceToHost, st));
    // 3 (synchronises the stream: c is read behind it)
    int passes = 0;
    uint64_t *sorted = nullptr;
    if (int rc = sort_keys_run(fn, key_a, key_b, s.p + o_counts, (int64_t)n, 0, 32 + quantile_bits(nz), st, &passes, &sorted)) return rc;
    const int64_t m = (int64_t)c.n_contrib;
    const uint64_t *keys = sorted;
    // 4
    const unsigned n_hblocks = (unsigned)((m + QT_BLOCK - 1) / QT_BLOCK);
    int32_t *blocks = present ? (int32_t *)(s.p + o_blocks) : nullptr;
    if (n_hblocks && (present || info)) {
        hipLaunchKernelGGL(quantile_heads_kernel, dim3(n_hblocks), dim3(QT_NT), 0, st, keys, m, blocks, counters);
        MHS_HIP(hipGetLastError());
    }
    if (n_hblocks && present) {
        hipLaunchKernelGGL(quantile_scan_kernel, dim3(1), dim3(QT_NT), 0, st, n_hblocks, blocks);
        MHS_HIP(hipGetLastError());
        hipLaunchKernelGGL(quantile_rows_kernel, dim3(n_hblocks), dim3(QT_NT), 0, st, keys, m, (const int32_t *)blocks, pr, quantum,
                           QTable{table->zone, table->count, table->q, table->capacity});
        MHS_HIP(hipGetLastError());
    }
    // 4'
    ZonalScratch zs;
    size_t start_bytes = 0;
    if (dense || pw) {
        start_bytes = zn_align(4 * ((size_t)nz + 1));
        if (int rc = zs.get(fn, start_bytes, st, "the zones' first places (4 bytes per zone slot)")) return rc;
        int32_t *start = (int32_t *)zs.p;
        hipLaunchKernelGGL(quantile_starts_kernel, dim3((unsigned)(((size_t)nz + 1 + QT_NT - 1) / QT_NT)), dim3(QT_NT), 0, st, keys, m, nz, start);
        MHS_HIP(hipGetLastError());
        if (dense && nz > 0) {
            hipLaunchKernelGGL(quantile_dense_kernel, dim3((nz + QT_NT - 1) / QT_NT), dim3(QT_NT), 0, st, keys, nz, (const int32_t *)start, pr, quantum,
                               QTable{nullptr, table->count, table->q, table->capacity});
            MHS_HIP(hipGetLastError());
        }
        // 6
        if (pw) {
            QPlaneOut o;
            std::memset(&o, 0, sizeof(o));
            for (int j = 0; j < n_probs; ++j) { o.q[j] = planes->q[j]; o.ld_q[j] = planes->ld_q[j]; }
            o.below = planes->below; o.ld_below = planes->ld_below;
            o.frac = planes->frac_below; o.ld_frac = planes->ld_frac_below;
            if (dtype == MHS_F64) launch_quantile_planes<double>(planes->dtype, nb_cells, st, g, plane, ldz, z, nz, quantum, keys, start, pr, o);
            else if (dtype == MHS_F32) launch_quantile_planes<float>(planes->dtype, nb_cells, st, g, plane, ldz, z, nz, quantum, keys, start, pr, o);
            else launch_quantile_planes<short>(planes->dtype, nb_cells, st, g, plane, ldz, z, nz, quantum, keys, start, pr, o);
            MHS_HIP(hipGetLastError());
        }
    }
    if (info) {
        ZonalCounters e;
        MHS_HIP(hipMemcpyAsync(&e, counters, sizeof(e), hipMemcpyDeviceToHost, st));
        MHS_HIP(hipStreamSynchronize(st));
        ZN_REQUIRE(!present || (int64_t)e.n_present <= table->capacity, "%s: %lld zones are present, which passes the table's capacity %lld", fn,
                   (long long)e.n_present, (long long)table->capacity);
        *info = mhs_quantile_info{n_zones, (int64_t)e.n_present, (int64_t)e.n_in_zone, (int64_t)e.n_contrib, (int64_t)n_nonfinite, (int64_t)e.n_inexact,
                                  quantum, (int64_t)(total + start_bytes + 256), (int64_t)passes};
    }
    return MHS_OK;
}

}  // namespace mhs

using namespace mhs;

extern "C" {

int mhs_zonal_quantile_dev(const mhs_grid *g, const mhs_stack *stack, int layer, const int32_t *zones, int64_t ld_zones, int64_t n_zones, double quantum,
                           int flags, const double *probs, int n_probs, const mhs_grid *target, const mhs_quantile_table *table,
                           const mhs_quantile_planes *planes, void *stream, mhs_quantile_info *info) {
    QCall call;
    if (int rc = quantile_check(__func__, g, stack, layer, zones, ld_zones, n_zones, quantum, flags, probs, n_probs, target, table, planes, true, info, &call))
        return rc;
    if (int rc = require_ready()) return rc;
    const void *plane = (const char *)stack->data + (size_t)layer * stack->plane_stride * dtype_bytes(stack->dtype);
    return quantile_run(__func__, call, stack->dtype, plane, stack->ld, zones, ld_zones, n_zones, quantum, probs, n_probs, table, planes, pick_stream(stream),
                        info);
}

// Host planes: the layer and the zone plane go up whole, the table's rows and the planes come down.
int mhs_zonal_quantile(const mhs_grid *g, const mhs_stack *stack, int layer, const int32_t *zones, int64_t n_zones, double quantum, int flags,
                       const double *probs, int n_probs, const mhs_grid *target, const mhs_quantile_table *table, const mhs_quantile_planes *planes,
                       mhs_quantile_info *info) {
    QCall call;
    const char *fn = __func__;
    if (int rc = quantile_check(fn, g, stack, layer, zones, g ? g->ncol : 0, n_zones, quantum, flags, probs, n_probs, target, table, planes, false, info, &call))
        return rc;
    if (int rc = require_ready()) return rc;
    const ZonalGeom &zg = call.g;
    const size_t esz = dtype_bytes(stack->dtype), n = (size_t)zg.nrow * (size_t)zg.ncol;
    const size_t in_bytes = ((size_t)(zg.nrow - 1) * stack->ld + zg.ncol) * esz;
    const bool tw = qt_table_wanted(table), pw = qt_planes_wanted(planes);
    const size_t cap = tw ? (size_t)table->capacity : 0, fsz = pw && planes->dtype == MHS_F32 ? 4 : 8;
    // the layer, the zone plane, the table's zone / count / q, the planes q[0 .. 15] / below / frac_below
    void *host[3 + QUANTILE_MAX_PROBS + 2];
    size_t bytes[3 + QUANTILE_MAX_PROBS + 2], off[3 + QUANTILE_MAX_PROBS + 2];
    host[0] = tw ? (void *)table->zone : nullptr;  bytes[0] = 4 * std::max<size_t>(cap, 1);
    host[1] = tw ? (void *)table->count : nullptr; bytes[1] = 8 * std::max<size_t>(cap, 1);
    host[2] = tw ? (void *)table->q : nullptr;     bytes[2] = 8 * std::max<size_t>(cap, 1) * (size_t)n_probs;
    for (int j = 0; j < QUANTILE_MAX_PROBS; ++j) { host[3 + j] = pw ? planes->q[j] : nullptr; bytes[3 + j] = fsz * n; }
    host[3 + QUANTILE_MAX_PROBS] = pw ? (void *)planes->below : nullptr;      bytes[3 + QUANTILE_MAX_PROBS] = 4 * n;
    host[4 + QUANTILE_MAX_PROBS] = pw ? planes->frac_below : nullptr;         bytes[4 + QUANTILE_MAX_PROBS] = fsz * n;
    size_t total = zn_align(in_bytes);
    const size_t o_zones = total;
    if (zones) total += zn_align(4 * n);
    for (int k = 0; k < 3 + QUANTILE_MAX_PROBS + 2; ++k) { off[k] = total; if (host[k]) total += zn_align(bytes[k]); }
    std::lock_guard<std::mutex> lk(pipe_mutex());
    if (int rc = host_pipe(0)) return rc;                      // the pipeline's streams; its arena is not used
    hipStream_t st = ctx().pipe_comp;
    ZonalScratch s;
    if (int rc = s.get(fn, total, st, "the layer, the zone plane and the outputs")) return rc;
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{st};   // no copy is left in flight, whatever the exit
    MHS_HIP(hipMemcpyAsync(s.p, (const char *)stack->data + (size_t)layer * stack->plane_stride * esz, in_bytes, hipMemcpyHostToDevice, st));
    if (zones) MHS_HIP(hipMemcpyAsync(s.p + o_zones, zones, 4 * n, hipMemcpyHostToDevice, st));
    auto dev = [&](int k) { return host[k] ? (void *)(s.p + off[k]) : nullptr; };
    mhs_quantile_table dt{(int64_t)cap, (int32_t *)dev(0), (int64_t *)dev(1), (double *)dev(2)};
    mhs_quantile_planes dp;
    std::memset(&dp, 0, sizeof(dp));
    if (pw) {
        dp.dtype = planes->dtype;
        for (int j = 0; j < QUANTILE_MAX_PROBS; ++j) { dp.q[j] = dev(3 + j); dp.ld_q[j] = zg.ncol; }
        dp.below = (int32_t *)dev(3 + QUANTILE_MAX_PROBS); dp.ld_below = zg.ncol;
        dp.frac_below = dev(4 + QUANTILE_MAX_PROBS); dp.ld_frac_below = zg.ncol;
    }
    mhs_quantile_info mine;
    if (int rc = quantile_run(fn, call, stack->dtype, s.p, stack->ld, zones ? (const int32_t *)(s.p + o_zones) : nullptr, zg.ncol, n_zones, quantum, probs,
                              n_probs, tw ? &dt : nullptr, pw ? &dp : nullptr, st, &mine))
        return rc;
    const size_t rows = tw ? (size_t)(table->zone ? mine.n_present : mine.n_zones) : 0;
    const size_t row_bytes[3] = {4, 8, 8 * (size_t)n_probs};
    for (int k = 0; k < 3; ++k)
        if (host[k] && rows) MHS_HIP(hipMemcpyAsync(host[k], s.p + off[k], row_bytes[k] * rows, hipMemcpyDeviceToHost, st));
    for (int k = 3; k < 3 + QUANTILE_MAX_PROBS + 2; ++k)
        if (host[k]) MHS_HIP(hipMemcpyAsync(host[k], s.p + off[k], bytes[k], hipMemcpyDeviceToHost, st));
    MHS_HIP(hipStreamSynchronize(st));
    if (info) *info = mine;
    return MHS_OK;
}

}  // extern "C"
