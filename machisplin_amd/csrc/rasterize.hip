// Points, lines and polygons burned onto the grid (include/machisplin_hip.h, section "rasterize", states the rule;
// rasterize_rule.h holds it).  Every product is an integer or a gather: the only atomics are integer XOR / OR on a feature's bit
// plane and integer max / add on the key and count planes, all of which commute, so the order in which lanes, waves and
// workgroups run is free and a repeated call gives the same bytes.
//
// Every phase is its own launch on the stream, and a kernel boundary is the only ordering between phases: no cross-block flag
// protocol, no spin wait, and every loop has a bound that is evident from the code (the input's sizes, 31 bisection steps, the
// 32 bits of a word).  The geometry arrives as host arrays; the host checks it, finds every feature's box, makes the keys and
// plans the batches in passes of O(vertices), and copies it up on the call's stream.
//   0   rz_init_kernel        key plane = -1, count plane = 0.
//   1   rz_count_kernel       a lane per vertex v: the number of items of the edge v -> v + 1 (the grid rows a polygon edge
//                             crosses, or the rows of a line segment inside the grid), and each block's total;
//       rz_scan_kernel        the exclusive prefix sum of the blocks' totals (one workgroup);
//       rz_prefix_kernel      the exclusive prefix sum P over the vertices;
//       rz_gather_kernel      P at the batches' first vertices, which the host reads (the one synchronisation before the end).
//                             With touches a polygon runs this twice: its crossings and its rings' line items.
//   2   rz_cross_kernel       a lane per (edge, row) item: the edge by bisection in P -- an edge 10 000 rows tall does not
//                             serialise a lane --, X(y_r), c*, and atomicXor of bit c* - c0 in the TOGGLE layer of the feature's
//                             bit plane.  A crossing left of the box toggles nothing in it; one right of it toggles the sentinel.
//       rz_span_kernel        a lane per (segment, row) item: the span's columns, ORed word by word into the BURN layer.
//   3   rz_fill_kernel        a wave per (feature, box row): the suffix XOR of the toggle bits -- in a word by shifts, across the
//                             RZ_CHUNK_WORDS words of a chunk by a ballot, across chunks by a carried parity --, OR the burn
//                             layer, then two words at a time over the lanes: atomicMax of the key, atomicAdd of 1 to count.
//       rz_points_kernel      a lane per point, straight to the two planes.
//   4   rz_products_kernel    a grid-stride pass over the cells: key -> index through the key table, values[index], and the number of
//                             burned cells, added once per workgroup.
// A line's cells go through a bit plane too, not straight to the planes as a polygon's fill does not either: `count` is the number
// of FEATURES on a cell, and consecutive segments of one polyline share their end cell.  The burn layer makes a feature count once.
//
// Scratch: ONE block of stream-ordered memory, given back behind the last kernel: the geometry (16 + 4 bytes per vertex), the
// item counts and prefix sums (4 + 8 per vertex, 8 more with touches), 8 bytes per RZ_SCAN_BLOCK vertices, 32 + 8 bytes per
// feature (box, key, plane offset; cumulated box rows), the key table and the values (4 + 8 per feature), the key plane (4 per
// cell), the largest batch's bit planes and a counter block, with 256-byte alignments.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <numeric>
#include <vector>
#include "ensemble_int.h"
#include "rasterize_rule.h"

namespace mhs {

constexpr int RZ_NT = 256;                   // threads per workgroup of every phase: 4 waves
constexpr int RZ_WAVES = RZ_NT / 64;
constexpr int RZ_PER_THREAD = RZ_SCAN_BLOCK / RZ_NT;
constexpr uint64_t RZ_LAUNCH_ITEMS = 1ull << 30;         // items per launch of a phase-2 or phase-3 kernel
static_assert(RZ_SCAN_BLOCK % RZ_NT == 0 && RZ_CHUNK_WORDS == 64, "whole chunks per block; a wave holds a chunk's words in its lanes");

struct RzFeat {
    int r0, c0, h, w;        // the box, clipped to the grid; h = w = 0: the feature lies outside
    int flags;               // RZ_TOGGLE | RZ_BURN: the layers of its bit plane
    int key;
    long long word_off;      // of its bit plane inside its batch's block, in 32-bit words
};
struct RzCounters {
    unsigned long long n_burned, n_outside;
};
struct RzPlanes {
    int32_t *key, *count;
    int64_t ld_count;
};

__device__ inline unsigned rz_wave_sum(unsigned v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// 0
__global__ __launch_bounds__(RZ_NT) void rz_init_kernel(const RzGrid g, const RzPlanes p) {
    const int64_t i = (int64_t)blockIdx.x * RZ_NT + threadIdx.x;
    if (i >= (int64_t)g.nrow * g.ncol) return;
    p.key[i] = -1;
    if (p.count) { const int64_t r = i / g.ncol; p.count[r * p.ld_count + (i - r * g.ncol)] = 0; }
}

// the edge that starts at vertex v, if one does
__device__ inline bool rz_edge(const double *__restrict__ xy, const int32_t *__restrict__ vfeat, const int64_t n_vertices, const int64_t v, RzSeg *s) {
    if (v + 1 >= n_vertices || vfeat[v] < 0) return false;
    *s = rz_seg(xy[2 * v], xy[2 * v + 1], xy[2 * v + 2], xy[2 * v + 3]);
    return true;
}
__device__ inline unsigned rz_items(const RzGrid &g, const RzSeg &s, const int lines, int *first) {
    return (unsigned)(lines ? rz_line_rows(g, s, first) : rz_cross_rows(g, s, first));
}

// 1.  Thread t of block b takes the RZ_PER_THREAD consecutive vertices from b * RZ_SCAN_BLOCK + t * RZ_PER_THREAD.
__global__ __launch_bounds__(RZ_NT) void rz_count_kernel(const RzGrid g, const double *__restrict__ xy, const int32_t *__restrict__ vfeat,
                                                         const int64_t n_vertices, const int lines, uint32_t *__restrict__ cnt,
                                                         unsigned long long *__restrict__ block_total) {
    __shared__ unsigned long long part[RZ_WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * RZ_SCAN_BLOCK + (int64_t)threadIdx.x * RZ_PER_THREAD;
    unsigned long long sum = 0;                              // an edge may cross every row: the totals need 64 bits
#pragma unroll
    for (int j = 0; j < RZ_PER_THREAD; ++j) {
        const int64_t v = base + j;
        if (v >= n_vertices) break;
        RzSeg s;
        int first;
        const unsigned c = rz_edge(xy, vfeat, n_vertices, v, &s) ? rz_items(g, s, lines, &first) : 0u;
        cnt[v] = c;
        sum += c;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if (lane == 0) part[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < RZ_WAVES; ++w) s += part[w];
        block_total[blockIdx.x] = s;
    }
}

// 1, one workgroup: block_total becomes its own exclusive prefix sum, chunk by chunk with a carry; [n_blocks] receives the total
__global__ __launch_bounds__(RZ_NT) void rz_scan_kernel(const int64_t n_blocks, unsigned long long *block_total) {
    __shared__ unsigned long long wave_total[RZ_WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned long long carry = 0;
    for (int64_t base = 0; base < n_blocks; base += RZ_NT) {
        const int64_t i = base + threadIdx.x;
        const unsigned long long v = i < n_blocks ? block_total[i] : 0ull;
        unsigned long long incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        unsigned long long before = 0, total = 0;
        for (int w = 0; w < RZ_WAVES; ++w) {
            if (w < wave) before += wave_total[w];
            total += wave_total[w];
        }
        if (i < n_blocks) block_total[i] = carry + before + incl - v;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) block_total[n_blocks] = carry;
}

// 1, the prefix sums over the vertices: P[v] = the items before edge v; P[n_vertices] = all of them
__global__ __launch_bounds__(RZ_NT) void rz_prefix_kernel(const int64_t n_vertices, const int64_t n_blocks, const uint32_t *__restrict__ cnt,
                                                          const unsigned long long *__restrict__ block_before, unsigned long long *__restrict__ P) {
    __shared__ unsigned long long wave_total[RZ_WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * RZ_SCAN_BLOCK + (int64_t)threadIdx.x * RZ_PER_THREAD;
    unsigned c[RZ_PER_THREAD];
    unsigned long long mine = 0;
#pragma unroll
    for (int j = 0; j < RZ_PER_THREAD; ++j) {
        c[j] = base + j < n_vertices ? cnt[base + j] : 0u;
        mine += c[j];
    }
    unsigned long long incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    unsigned long long run = block_before[blockIdx.x] + incl - mine;
    for (int w = 0; w < wave; ++w) run += wave_total[w];
#pragma unroll
    for (int j = 0; j < RZ_PER_THREAD; ++j) {
        if (base + j < n_vertices) P[base + j] = run;
        run += c[j];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) P[n_vertices] = block_before[n_blocks];
}

// 1, what the host reads: P at the n vertices of `at`
__global__ __launch_bounds__(RZ_NT) void rz_gather_kernel(const int64_t n, const int64_t *__restrict__ at, const unsigned long long *__restrict__ P,
                                                          unsigned long long *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * RZ_NT + threadIdx.x;
    if (i < n) out[i] = P[at[i]];
}

// the edge of item `item`: the v in v0 .. v1 - 1 with P[v] <= item < P[v + 1]; at most 31 steps
__device__ inline int64_t rz_find(const unsigned long long *__restrict__ P, int64_t v0, int64_t v1, const unsigned long long item) {
    while (v1 - v0 > 1) {
        const int64_t mid = v0 + (v1 - v0) / 2;
        if (P[mid] <= item) v0 = mid; else v1 = mid;
    }
    return v0;
}

// 2.  Items begin .. end - 1 of the batch whose vertices are v0 .. v1 - 1; `bits` is the batch's block of bit planes.
__global__ __launch_bounds__(RZ_NT) void rz_cross_kernel(const RzGrid g, const double *__restrict__ xy, const int32_t *__restrict__ vfeat,
                                                         const int64_t n_vertices, const unsigned long long *__restrict__ P, const int64_t v0,
                                                         const int64_t v1, const unsigned long long begin, const unsigned long long end,
                                                         const RzFeat *__restrict__ feats, uint32_t *__restrict__ bits) {
    const unsigned long long item = begin + (unsigned long long)blockIdx.x * RZ_NT + threadIdx.x;
    if (item >= end) return;
    const int64_t v = rz_find(P, v0, v1, item);
    RzSeg s;
    if (!rz_edge(xy, vfeat, n_vertices, v, &s)) return;
    const RzFeat f = feats[vfeat[v]];
    if (f.h == 0 || !(f.flags & RZ_TOGGLE)) return;
    int first;
    const unsigned n = rz_items(g, s, 0, &first);
    const unsigned long long k = item - P[v];
    if (k >= n) return;
    const int r = first + (int)k, rr = r - f.r0;
    if (rr < 0 || rr >= f.h) return;
    int j = rz_cstar(g, rz_X(s, rz_yr(g, r))) - f.c0;
    if (j <= 0) return;                                      // toggles no cell of the box
    if (j > f.w) j = f.w;                                    // the sentinel: every cell of the box's row
    atomicXor(&bits[f.word_off + (long long)rr * rz_row_words(f.w) + (j >> 5)], 1u << (j & 31));
}

__global__ __launch_bounds__(RZ_NT) void rz_span_kernel(const RzGrid g, const double *__restrict__ xy, const int32_t *__restrict__ vfeat,
                                                        const int64_t n_vertices, const unsigned long long *__restrict__ P, const int64_t v0,
                                                        const int64_t v1, const unsigned long long begin, const unsigned long long end,
                                                        const RzFeat *__restrict__ feats, uint32_t *__restrict__ bits) {
    const unsigned long long item = begin + (unsigned long long)blockIdx.x * RZ_NT + threadIdx.x;
    if (item >= end) return;
    const int64_t v = rz_find(P, v0, v1, item);
    RzSeg s;
    if (!rz_edge(xy, vfeat, n_vertices, v, &s)) return;
    const RzFeat f = feats[vfeat[v]];
    if (f.h == 0 || !(f.flags & RZ_BURN)) return;
    int first;
    const unsigned n = rz_items(g, s, 1, &first);
    const unsigned long long k = item - P[v];
    if (k >= n) return;
    const int r = first + (int)k, rr = r - f.r0;
    if (rr < 0 || rr >= f.h) return;
    int c_lo, c_hi;
    if (!rz_line_span(g, s, r, &c_lo, &c_hi)) return;
    int j_lo = c_lo - f.c0, j_hi = c_hi - f.c0;
    if (j_lo < 0) j_lo = 0;
    if (j_hi > f.w - 1) j_hi = f.w - 1;
    if (j_lo > j_hi) return;
    const long long wpr = rz_row_words(f.w);
    uint32_t *row = bits + f.word_off + ((f.flags & RZ_TOGGLE) ? (long long)f.h * wpr : 0ll) + (long long)rr * wpr;
    for (int wi = j_lo >> 5; wi <= (j_hi >> 5); ++wi) {       // at most wpr words
        const int a = wi == (j_lo >> 5) ? (j_lo & 31) : 0, b = wi == (j_hi >> 5) ? (j_hi & 31) : 31;
        const uint32_t m = (b == 31 ? 0xffffffffu : (1u << (b + 1)) - 1u) & ~((1u << a) - 1u);
        atomicOr(&row[wi], m);
    }
}

// 3.  Wave `item` of the launch takes box row (first_row + item) of the batch's features f0 .. f1 - 1, counted through their
// cumulated heights R.
__global__ __launch_bounds__(RZ_NT) void rz_fill_kernel(const RzGrid g, const RzFeat *__restrict__ feats, const long long *__restrict__ R, const int64_t f0,
                                                        const int64_t f1, const long long first_row, const long long end_row,
                                                        const uint32_t *__restrict__ bits, const RzPlanes p) {
    const int lane = threadIdx.x & 63;
    const long long row_id = first_row + (long long)blockIdx.x * RZ_WAVES + (threadIdx.x >> 6);
    if (row_id >= end_row) return;                            // wave-uniform
    int64_t lo = f0, hi = f1;                                 // the feature with R[f] <= row_id < R[f + 1]
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (R[mid] <= row_id) lo = mid; else hi = mid;
    }
    const RzFeat f = feats[lo];
    const int rr = (int)(row_id - R[lo]);
    if (rr < 0 || rr >= f.h) return;
    const int r = f.r0 + rr;
    const long long wpr = rz_row_words(f.w);
    const uint32_t *T = (f.flags & RZ_TOGGLE) ? bits + f.word_off + (long long)rr * wpr : nullptr;
    const uint32_t *B = (f.flags & RZ_BURN) ? bits + f.word_off + ((f.flags & RZ_TOGGLE) ? (long long)f.h * wpr : 0ll) + (long long)rr * wpr : nullptr;
    const int n_chunks = (int)((wpr + RZ_CHUNK_WORDS - 1) / RZ_CHUNK_WORDS);
    unsigned carry = 0;                                       // the parity of every toggle bit right of this chunk
    for (int ch = n_chunks - 1; ch >= 0; --ch) {
        const long long wi = (long long)ch * RZ_CHUNK_WORDS + lane;
        const uint32_t t = T && wi < wpr ? T[wi] : 0u, b = B && wi < wpr ? B[wi] : 0u;
        uint32_t s = t;                                       // bit j of s: the XOR of bits j .. 31 of t
        s ^= s >> 1; s ^= s >> 2; s ^= s >> 4; s ^= s >> 8; s ^= s >> 16;
        const uint32_t e = s ^ t;                             // ... of bits j + 1 .. 31: the toggles right of column j in this word
        const uint64_t odd = __ballot(s & 1u);                // the words with an odd number of toggles
        const unsigned right = lane == 63 ? 0u : (unsigned)__popcll(odd >> (lane + 1)) & 1u;
        uint32_t cover = ((right ^ carry) ? ~e : e) | b;
        const long long col0 = wi * 32;                       // the box column of bit 0; columns w and above are no cells
        if (col0 >= f.w) cover = 0u;
        else if (f.w - col0 < 32) cover &= (1u << (int)(f.w - col0)) - 1u;
        carry ^= (unsigned)__popcll(odd) & 1u;
        const uint64_t any = __ballot(cover != 0u);
        for (int k = 0; k < RZ_CHUNK_WORDS / 2; ++k) {        // words 2k and 2k + 1 over the 64 lanes: consecutive cells
            if (!((any >> (2 * k)) & 3ull)) continue;         // wave-uniform
            const uint32_t cw = (uint32_t)__shfl((int)cover, 2 * k + (lane >> 5), 64);
            if (!((cw >> (lane & 31)) & 1u)) continue;
            const int64_t c = (int64_t)f.c0 + ((int64_t)ch * RZ_CHUNK_WORDS + 2 * k) * 32 + lane;
            atomicMax(&p.key[(int64_t)r * g.ncol + c], f.key);
            if (p.count) atomicAdd(&p.count[(int64_t)r * p.ld_count + c], 1);
        }
    }
}

// 3, points
__global__ __launch_bounds__(RZ_NT) void rz_points_kernel(const RzGrid g, const double *__restrict__ xy, const int32_t *__restrict__ vfeat,
                                                          const int64_t n_vertices, const RzFeat *__restrict__ feats, const RzPlanes p,
                                                          RzCounters *counters) {
    const int64_t v = (int64_t)blockIdx.x * RZ_NT + threadIdx.x;
    unsigned outside = 0;
    if (v < n_vertices && vfeat[v] >= 0) {
        int r, c;
        if (rz_point_cell(g, xy[2 * v], xy[2 * v + 1], &r, &c)) {
            atomicMax(&p.key[(int64_t)r * g.ncol + c], feats[vfeat[v]].key);
            if (p.count) atomicAdd(&p.count[(int64_t)r * p.ld_count + c], 1);
        } else outside = 1;
    }
    outside = rz_wave_sum(outside);
    if ((threadIdx.x & 63) == 0 && outside) atomicAdd(&counters->n_outside, (unsigned long long)outside);
}

// 4.  A grid-stride pass: a workgroup adds its burned cells to the counter ONCE (an atomic per wave on the one address took 19 ms
// of a 10^8-cell call when every cell was burned; the planes themselves take a fraction of a millisecond).
template <typename O>
__global__ __launch_bounds__(RZ_NT) void rz_products_kernel(const RzGrid g, const int32_t *__restrict__ key, const int32_t *__restrict__ key_feature,
                                                            const double *__restrict__ values, int32_t *__restrict__ index, const int64_t ld_index,
                                                            O *__restrict__ value, const int64_t ld_value, RzCounters *counters) {
    __shared__ unsigned part[RZ_WAVES];
    const int64_t n = (int64_t)g.nrow * g.ncol;
    unsigned burned = 0;                                      // at most 2^31 / RZ_NT cells per thread
    for (int64_t i = (int64_t)blockIdx.x * RZ_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * RZ_NT) {
        const int64_t r = i / g.ncol, c = i - r * g.ncol;
        const int k = key[i];
        const int f = k >= 0 ? key_feature[k] : -1;
        burned += k >= 0;
        if (index) index[r * ld_index + c] = f;
        if (value) value[r * ld_value + c] = (O)(f >= 0 ? values[f] : __builtin_nan(""));
    }
    burned = rz_wave_sum(burned);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = burned;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long all = 0;
        for (int w = 0; w < RZ_WAVES; ++w) all += part[w];
        if (all) atomicAdd(&counters->n_burned, all);
    }
}

#define RZ_REQUIRE(cond, ...)                                              \
    do {                                                                   \
        if (!(cond)) { set_error(__VA_ARGS__); return MHS_ERR_INVALID; }    \
    } while (0)

static bool rz_finite(double v) { return std::fabs(v) <= 1.7976931348623157e308; }

// Every check of a rasterize call, before any device call; fn = the entry point's name for the message
static int rasterize_check(const char *fn, const mhs_grid *grid, const mhs_features *ft, int rule, const mhs_rasterize_out *out, int64_t budget, bool dev,
                           RzGrid *g) {
    RZ_REQUIRE(grid && ft && out, "%s: NULL argument (g, features or out)", fn);
    RZ_REQUIRE(grid->nrow > 0 && grid->ncol > 0 && grid->nrow <= (int64_t)INT32_MAX && grid->ncol <= (int64_t)INT32_MAX,
               "%s: bad grid geometry (nrow, ncol must be in 1 .. 2^31 - 1)", fn);
    RZ_REQUIRE(grid->nrow * grid->ncol <= (int64_t)INT32_MAX, "%s: grid too large: nrow * ncol must not pass 2^31 - 1", fn);
    RZ_REQUIRE(rz_finite(grid->xmin) && rz_finite(grid->ymax) && grid->xres > 0.0 && grid->yres > 0.0 && rz_finite(grid->xres) && rz_finite(grid->yres),
               "%s: bad grid geometry (xmin, ymax must be finite, xres, yres positive and finite)", fn);
    RZ_REQUIRE(ft->kind == RZ_POINT || ft->kind == RZ_LINE || ft->kind == RZ_POLYGON, "%s: unknown kind %d of features", fn, ft->kind);
    RZ_REQUIRE(rule >= RZ_LAST && rule <= RZ_MIN, "%s: unknown rule %d", fn, rule);
    RZ_REQUIRE(out->index || out->count || out->value, "%s: no product requested (index, count and value are all NULL)", fn);
    RZ_REQUIRE(!out->value || out->value_dtype == MHS_F64 || out->value_dtype == MHS_F32, "%s: value_dtype must be MHS_F64 or MHS_F32", fn);
    if (dev) {
        RZ_REQUIRE(!out->index || out->ld_index >= grid->ncol, "%s: ld_index smaller than the grid width", fn);
        RZ_REQUIRE(!out->count || out->ld_count >= grid->ncol, "%s: ld_count smaller than the grid width", fn);
        RZ_REQUIRE(!out->value || out->ld_value >= grid->ncol, "%s: ld_value smaller than the grid width", fn);
    }
    RZ_REQUIRE(budget >= 0, "%s: scratch_budget must not be negative (0: the default)", fn);
    const int64_t nv = ft->n_vertices, np = ft->n_parts, nf = ft->n_features;
    RZ_REQUIRE(nv >= 0 && np >= 0 && nf >= 0 && nv <= (int64_t)INT32_MAX && np <= (int64_t)INT32_MAX && nf <= (int64_t)INT32_MAX,
               "%s: n_vertices, n_parts and n_features must be in 0 .. 2^31 - 1", fn);
    RZ_REQUIRE(ft->part_offsets && ft->feature_offsets && (ft->coords || nv == 0), "%s: NULL array (coords, part_offsets or feature_offsets)", fn);
    RZ_REQUIRE(ft->values || !out->value, "%s: values is missing: the value product needs it", fn);
    RZ_REQUIRE(ft->values || (rule != RZ_MAX && rule != RZ_MIN), "%s: values is missing: the rules min and max need it", fn);
    RZ_REQUIRE(ft->feature_offsets[0] == 0 && ft->feature_offsets[nf] == np, "%s: feature_offsets must start at 0 and end at n_parts = %lld", fn, (long long)np);
    for (int64_t i = 0; i < nf; ++i)
        RZ_REQUIRE(ft->feature_offsets[i + 1] >= ft->feature_offsets[i] && ft->feature_offsets[i + 1] <= np,
                   "%s: feature_offsets must not decrease (at feature %lld)", fn, (long long)i);
    RZ_REQUIRE(ft->part_offsets[0] == 0 && ft->part_offsets[np] == nv, "%s: part_offsets must start at 0 and end at n_vertices = %lld", fn, (long long)nv);
    for (int64_t i = 0; i < np; ++i)
        RZ_REQUIRE(ft->part_offsets[i + 1] >= ft->part_offsets[i] && ft->part_offsets[i + 1] <= nv, "%s: part_offsets must not decrease (at part %lld)", fn,
                   (long long)i);
    for (int64_t i = 0; i < 2 * nv; ++i)
        RZ_REQUIRE(rz_finite(ft->coords[i]), "%s: coords holds a non-finite coordinate (vertex %lld)", fn, (long long)(i / 2));
    for (int64_t i = 0; i < np; ++i) {
        const int64_t a = ft->part_offsets[i], n = ft->part_offsets[i + 1] - a;
        if (ft->kind == RZ_LINE) RZ_REQUIRE(n >= 2, "%s: line part %lld has fewer than 2 vertices", fn, (long long)i);
        if (ft->kind == RZ_POLYGON) {
            RZ_REQUIRE(n >= 4, "%s: ring %lld has fewer than 4 vertices", fn, (long long)i);
            RZ_REQUIRE(ft->coords[2 * a] == ft->coords[2 * (a + n - 1)] && ft->coords[2 * a + 1] == ft->coords[2 * (a + n - 1) + 1],
                       "%s: ring %lld is not closed (its last vertex is not its first)", fn, (long long)i);
        }
    }
    if (ft->values && (rule == RZ_MAX || rule == RZ_MIN))
        for (int64_t i = 0; i < nf; ++i) RZ_REQUIRE(rz_finite(ft->values[i]), "%s: values must be finite with the rules min and max (feature %lld)", fn, (long long)i);
    *g = RzGrid{grid->xmin, grid->ymax, grid->xres, grid->yres, (int)grid->nrow, (int)grid->ncol};
    return MHS_OK;
}

// a block of stream-ordered memory, given back behind whatever was enqueued last
struct RzScratch {
    char *p = nullptr;
    hipStream_t st = nullptr;
    ~RzScratch() { if (p) (void)hipFreeAsync(p, st); }
    int get(const char *fn, size_t bytes, hipStream_t s, const char *what) {
        st = s;
        if (hipMallocAsync((void **)&p, bytes, s) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            set_error("%s: no device memory for %s (%zu bytes)", fn, what, bytes);
            return MHS_ERR_ALLOC;
        }
        return MHS_OK;
    }
};
struct RzDrain {                             // no copy from a host array of the call is left in flight, whatever the exit
    hipStream_t s;
    ~RzDrain() { (void)hipStreamSynchronize(s); }
};

static size_t rz_align(size_t n) { return (n + 255) & ~(size_t)255; }

struct RzBatch {
    int64_t f0, f1, v0, v1;
    long long words;
};

// The prefix sums of one kind of item over all vertices, and their values at the batches' first vertices in `at_host`
static int rz_prefix(const RzGrid &g, const double *xy, const int32_t *vfeat, int64_t nv, int lines, uint32_t *cnt, unsigned long long *blocks,
                     unsigned long long *P, const int64_t *at_dev, int64_t n_at, unsigned long long *at_out, hipStream_t st) {
    const int64_t n_blocks = (nv + RZ_SCAN_BLOCK - 1) / RZ_SCAN_BLOCK;
    hipLaunchKernelGGL(rz_count_kernel, dim3((unsigned)n_blocks), dim3(RZ_NT), 0, st, g, xy, vfeat, nv, lines, cnt, blocks);
    MHS_HIP(hipGetLastError());
    hipLaunchKernelGGL(rz_scan_kernel, dim3(1), dim3(RZ_NT), 0, st, n_blocks, blocks);
    MHS_HIP(hipGetLastError());
    hipLaunchKernelGGL(rz_prefix_kernel, dim3((unsigned)n_blocks), dim3(RZ_NT), 0, st, nv, n_blocks, (const uint32_t *)cnt, (const unsigned long long *)blocks, P);
    MHS_HIP(hipGetLastError());
    hipLaunchKernelGGL(rz_gather_kernel, dim3((unsigned)((n_at + RZ_NT - 1) / RZ_NT)), dim3(RZ_NT), 0, st, n_at, at_dev, (const unsigned long long *)P, at_out);
    MHS_HIP(hipGetLastError());
    return MHS_OK;
}

// Device planes; the geometry on the host.  Every argument has been checked.
static int rasterize_run(const char *fn, const RzGrid &g, const mhs_features *ft, int rule, int touches, const mhs_rasterize_out *out, int64_t budget,
                         hipStream_t st, mhs_rasterize_info *info) {
    const int64_t nv = ft->n_vertices, np = ft->n_parts, nf = ft->n_features;
    const size_t n = (size_t)g.nrow * (size_t)g.ncol;
    const int kind = ft->kind;
    const bool cross = kind == RZ_POLYGON, lines = kind == RZ_LINE || (kind == RZ_POLYGON && touches);
    if (budget == 0) budget = RZ_DEFAULT_BUDGET;
    // the host's passes over the geometry: the feature of every edge, the boxes, the keys, the batches
    std::vector<int32_t> vfeat((size_t)std::max<int64_t>(nv, 1), -1), key_feature((size_t)std::max<int64_t>(nf, 1), 0);
    std::vector<RzFeat> feats((size_t)std::max<int64_t>(nf, 1));
    std::vector<long long> R((size_t)nf + 1, 0);
    std::vector<int32_t> keys((size_t)std::max<int64_t>(nf, 1), 0);
    if (rule == RZ_MAX || rule == RZ_MIN) {
        std::vector<int32_t> order((size_t)nf);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return ft->values[a] < ft->values[b]; });
        for (int64_t k = 0; k < nf; ++k) keys[order[k]] = (int32_t)(rule == RZ_MAX ? k : nf - 1 - k);
    } else
        for (int64_t i = 0; i < nf; ++i) keys[i] = (int32_t)(rule == RZ_LAST ? i : nf - 1 - i);
    for (int64_t i = 0; i < nf; ++i) key_feature[keys[i]] = (int32_t)i;
    std::vector<RzBatch> batches;
    std::vector<unsigned long long> atc, atl;                 // the prefix sums at the batches' first vertices, read back
    long long max_words = 0;
    for (int64_t i = 0; i < nf; ++i) {
        const int64_t p0 = ft->feature_offsets[i], p1 = ft->feature_offsets[i + 1], v0 = ft->part_offsets[p0], v1 = ft->part_offsets[p1];
        RzFeat &f = feats[i];
        f = RzFeat{0, 0, 0, 0, 0, keys[i], 0};
        for (int64_t p = p0; p < p1; ++p) {
            const int64_t a = ft->part_offsets[p], b = ft->part_offsets[p + 1];
            for (int64_t v = a; v < b; ++v) vfeat[v] = kind == RZ_POINT || v + 1 < b ? (int32_t)i : -1;
        }
        long long words = 0;
        if (kind != RZ_POINT && v1 > v0) {
            double x0 = ft->coords[2 * v0], x1 = x0, y0 = ft->coords[2 * v0 + 1], y1 = y0;
            for (int64_t v = v0 + 1; v < v1; ++v) {
                const double x = ft->coords[2 * v], y = ft->coords[2 * v + 1];
                x0 = std::min(x0, x); x1 = std::max(x1, x); y0 = std::min(y0, y); y1 = std::max(y1, y);
            }
            RzBox b;
            if (rz_box(g, x0, x1, y0, y1, &b)) {
                f.r0 = b.r0; f.c0 = b.c0; f.h = b.h; f.w = b.w;
                f.flags = (cross ? RZ_TOGGLE : 0) | (lines ? RZ_BURN : 0);
                words = (long long)b.h * rz_row_words(b.w) * ((cross ? 1 : 0) + (lines ? 1 : 0));
            }
        }
        R[i + 1] = R[i] + f.h;
        // consecutive features share a batch while their bit planes fit the budget; one that is larger gets a batch of its own
        if (batches.empty() || (batches.back().words > 0 && (batches.back().words + words) * 4 > budget)) batches.push_back(RzBatch{i, i, v0, v0, 0});
        RzBatch &b = batches.back();
        f.word_off = b.words;
        b.words += words;
        b.f1 = i + 1;
        b.v1 = v1;
        max_words = std::max(max_words, b.words);
    }
    if (batches.empty()) batches.push_back(RzBatch{0, 0, 0, 0, 0});
    const int64_t n_batches = (int64_t)batches.size(), n_at = n_batches + 1;
    std::vector<int64_t> at((size_t)n_at);
    for (int64_t b = 0; b < n_batches; ++b) at[b] = batches[b].v0;
    at[n_batches] = nv;
    // the block of scratch
    const int64_t n_blocks = std::max<int64_t>(1, (nv + RZ_SCAN_BLOCK - 1) / RZ_SCAN_BLOCK);
    const bool scans = kind != RZ_POINT && nv > 0;
    size_t total = 0;
    auto take = [&](bool wanted, size_t bytes) { const size_t o = total; if (wanted) total += rz_align(std::max<size_t>(bytes, 1)); return wanted ? o : (size_t)-1; };
    const size_t o_counters = take(true, 256), o_xy = take(true, 16 * (size_t)nv), o_vfeat = take(true, 4 * (size_t)nv), o_cnt = take(scans, 4 * (size_t)nv),
                 o_blocks = take(scans, 8 * (size_t)(n_blocks + 1)), o_Pc = take(scans && cross, 8 * (size_t)(nv + 1)),
                 o_Pl = take(scans && lines, 8 * (size_t)(nv + 1)), o_at = take(scans, 8 * (size_t)n_at), o_atc = take(scans, 8 * (size_t)n_at),
                 o_atl = take(scans, 8 * (size_t)n_at), o_feats = take(true, sizeof(RzFeat) * (size_t)nf), o_R = take(true, 8 * (size_t)(nf + 1)),
                 o_kf = take(true, 4 * (size_t)nf), o_values = take(out->value != nullptr, 8 * (size_t)nf), o_key = take(true, 4 * n),
                 o_bits = take(max_words > 0, 4 * (size_t)max_words);
    RzScratch s;
    if (int rc = s.get(fn, total, st, "the geometry, the prefix sums, the key plane and the bit planes")) return rc;
    RzDrain drain{st};
    auto at_off = [&](size_t o) { return o == (size_t)-1 ? nullptr : s.p + o; };
    RzCounters *counters = (RzCounters *)at_off(o_counters);
    double *xy = (double *)at_off(o_xy);
    int32_t *d_vfeat = (int32_t *)at_off(o_vfeat);
    RzFeat *d_feats = (RzFeat *)at_off(o_feats);
    long long *d_R = (long long *)at_off(o_R);
    int32_t *d_kf = (int32_t *)at_off(o_kf);
    double *d_values = (double *)at_off(o_values);
    uint32_t *bits = (uint32_t *)at_off(o_bits);
    unsigned long long *Pc = (unsigned long long *)at_off(o_Pc), *Pl = (unsigned long long *)at_off(o_Pl);
    const RzPlanes planes{(int32_t *)at_off(o_key), out->count, out->count ? out->ld_count : 0};
    MHS_HIP(hipMemsetAsync(counters, 0, 256, st));
    if (nv > 0) {
        MHS_HIP(hipMemcpyAsync(xy, ft->coords, 16 * (size_t)nv, hipMemcpyHostToDevice, st));
        MHS_HIP(hipMemcpyAsync(d_vfeat, vfeat.data(), 4 * (size_t)nv, hipMemcpyHostToDevice, st));
    }
    if (nf > 0) {
        MHS_HIP(hipMemcpyAsync(d_feats, feats.data(), sizeof(RzFeat) * (size_t)nf, hipMemcpyHostToDevice, st));
        MHS_HIP(hipMemcpyAsync(d_kf, key_feature.data(), 4 * (size_t)nf, hipMemcpyHostToDevice, st));
        if (d_values) MHS_HIP(hipMemcpyAsync(d_values, ft->values, 8 * (size_t)nf, hipMemcpyHostToDevice, st));
    }
    MHS_HIP(hipMemcpyAsync(d_R, R.data(), 8 * (size_t)(nf + 1), hipMemcpyHostToDevice, st));
    const unsigned nb_cells = (unsigned)((n + RZ_NT - 1) / RZ_NT);
    // 0
    hipLaunchKernelGGL(rz_init_kernel, dim3(nb_cells), dim3(RZ_NT), 0, st, g, planes);
    MHS_HIP(hipGetLastError());
    int64_t n_items = 0;
    if (kind == RZ_POINT) {
        n_items = nv;
        if (nv > 0) {
            hipLaunchKernelGGL(rz_points_kernel, dim3((unsigned)((nv + RZ_NT - 1) / RZ_NT)), dim3(RZ_NT), 0, st, g, (const double *)xy, (const int32_t *)d_vfeat,
                               nv, (const RzFeat *)d_feats, planes, counters);
            MHS_HIP(hipGetLastError());
        }
    } else if (scans) {
        // 1
        atc.assign((size_t)n_at, 0ull);
        atl.assign((size_t)n_at, 0ull);
        MHS_HIP(hipMemcpyAsync(at_off(o_at), at.data(), 8 * (size_t)n_at, hipMemcpyHostToDevice, st));
        if (cross) {
            if (int rc = rz_prefix(g, xy, d_vfeat, nv, 0, (uint32_t *)at_off(o_cnt), (unsigned long long *)at_off(o_blocks), Pc, (const int64_t *)at_off(o_at), n_at,
                                   (unsigned long long *)at_off(o_atc), st))
                return rc;
            MHS_HIP(hipMemcpyAsync(atc.data(), at_off(o_atc), 8 * (size_t)n_at, hipMemcpyDeviceToHost, st));
        }
        if (lines) {
            if (int rc = rz_prefix(g, xy, d_vfeat, nv, 1, (uint32_t *)at_off(o_cnt), (unsigned long long *)at_off(o_blocks), Pl, (const int64_t *)at_off(o_at), n_at,
                                   (unsigned long long *)at_off(o_atl), st))
                return rc;
            MHS_HIP(hipMemcpyAsync(atl.data(), at_off(o_atl), 8 * (size_t)n_at, hipMemcpyDeviceToHost, st));
        }
        MHS_HIP(hipStreamSynchronize(st));
        n_items = (int64_t)(atc[n_batches] + atl[n_batches]);
        for (int64_t b = 0; b < n_batches; ++b) {
            const RzBatch &bt = batches[b];
            if (bt.words == 0) continue;                         // every feature of the batch lies outside the grid
            MHS_HIP(hipMemsetAsync(bits, 0, 4 * (size_t)bt.words, st));
            // 2
            for (unsigned long long i = atc[b]; i < atc[b + 1]; i += RZ_LAUNCH_ITEMS) {
                const unsigned long long e = std::min(atc[b + 1], i + RZ_LAUNCH_ITEMS);
                hipLaunchKernelGGL(rz_cross_kernel, dim3((unsigned)((e - i + RZ_NT - 1) / RZ_NT)), dim3(RZ_NT), 0, st, g, (const double *)xy, (const int32_t *)d_vfeat,
                                   nv, (const unsigned long long *)Pc, bt.v0, bt.v1, i, e, (const RzFeat *)d_feats, bits);
                MHS_HIP(hipGetLastError());
            }
            for (unsigned long long i = atl[b]; i < atl[b + 1]; i += RZ_LAUNCH_ITEMS) {
                const unsigned long long e = std::min(atl[b + 1], i + RZ_LAUNCH_ITEMS);
                hipLaunchKernelGGL(rz_span_kernel, dim3((unsigned)((e - i + RZ_NT - 1) / RZ_NT)), dim3(RZ_NT), 0, st, g, (const double *)xy, (const int32_t *)d_vfeat,
                                   nv, (const unsigned long long *)Pl, bt.v0, bt.v1, i, e, (const RzFeat *)d_feats, bits);
                MHS_HIP(hipGetLastError());
            }
            // 3
            for (long long i = R[bt.f0]; i < R[bt.f1]; i += (long long)RZ_LAUNCH_ITEMS) {
                const long long e = std::min(R[bt.f1], i + (long long)RZ_LAUNCH_ITEMS);
                hipLaunchKernelGGL(rz_fill_kernel, dim3((unsigned)((e - i + RZ_WAVES - 1) / RZ_WAVES)), dim3(RZ_NT), 0, st, g, (const RzFeat *)d_feats,
                                   (const long long *)d_R, bt.f0, bt.f1, i, e, (const uint32_t *)bits, planes);
                MHS_HIP(hipGetLastError());
            }
        }
    }
    // 4
    const unsigned nb_products = std::min<unsigned>(nb_cells, (unsigned)(ctx().n_cu > 0 ? ctx().n_cu : 256) * 32u);
    if (out->value && out->value_dtype == MHS_F32)
        hipLaunchKernelGGL(rz_products_kernel<float>, dim3(nb_products), dim3(RZ_NT), 0, st, g, (const int32_t *)planes.key, (const int32_t *)d_kf,
                           (const double *)d_values, out->index, out->ld_index, (float *)out->value, out->ld_value, counters);
    else
        hipLaunchKernelGGL(rz_products_kernel<double>, dim3(nb_products), dim3(RZ_NT), 0, st, g, (const int32_t *)planes.key, (const int32_t *)d_kf,
                           (const double *)d_values, out->index, out->ld_index, (double *)out->value, out->ld_value, counters);
    MHS_HIP(hipGetLastError());
    RzCounters c;
    MHS_HIP(hipMemcpyAsync(&c, counters, sizeof(c), hipMemcpyDeviceToHost, st));
    MHS_HIP(hipStreamSynchronize(st));
    if (info)
        *info = mhs_rasterize_info{nf, np, nv, kind == RZ_POINT ? 0 : nv - np, n_items, n_batches, (int64_t)c.n_burned, (int64_t)c.n_outside, (int64_t)total};
    return MHS_OK;
}

}  // namespace mhs

using namespace mhs;

extern "C" {

int mhs_rasterize_dev(const mhs_grid *g, const mhs_features *features, int rule, int touches, const mhs_rasterize_out *out, int64_t scratch_budget,
                      void *stream, mhs_rasterize_info *info) {
    RzGrid rg;
    if (int rc = rasterize_check(__func__, g, features, rule, out, scratch_budget, true, &rg)) return rc;
    if (int rc = require_ready()) return rc;
    return rasterize_run(__func__, rg, features, rule, touches, out, scratch_budget, pick_stream(stream), info);
}

// Host planes: the products are made in device memory of the call and come down.
int mhs_rasterize(const mhs_grid *g, const mhs_features *features, int rule, int touches, const mhs_rasterize_out *out, int64_t scratch_budget,
                  mhs_rasterize_info *info) {
    RzGrid rg;
    const char *fn = __func__;
    if (int rc = rasterize_check(fn, g, features, rule, out, scratch_budget, false, &rg)) return rc;
    if (int rc = require_ready()) return rc;
    const size_t n = (size_t)rg.nrow * (size_t)rg.ncol, vsz = out->value && out->value_dtype == MHS_F32 ? 4 : 8;
    const size_t o_index = 0, o_count = o_index + (out->index ? rz_align(4 * n) : 0), o_value = o_count + (out->count ? rz_align(4 * n) : 0),
                 total = o_value + (out->value ? rz_align(vsz * n) : 0);
    std::lock_guard<std::mutex> lk(pipe_mutex());
    if (int rc = host_pipe(0)) return rc;                      // the pipeline's streams; its arena is not used
    hipStream_t st = ctx().pipe_comp;
    RzScratch s;
    if (int rc = s.get(fn, total, st, "the products")) return rc;
    RzDrain drain{st};
    const mhs_rasterize_out d{out->index ? (int32_t *)(s.p + o_index) : nullptr, out->count ? (int32_t *)(s.p + o_count) : nullptr,
                              out->value ? (void *)(s.p + o_value) : nullptr, rg.ncol, rg.ncol, rg.ncol, out->value_dtype};
    mhs_rasterize_info mine;
    if (int rc = rasterize_run(fn, rg, features, rule, touches, &d, scratch_budget, st, &mine)) return rc;
    if (out->index) MHS_HIP(hipMemcpyAsync(out->index, d.index, 4 * n, hipMemcpyDeviceToHost, st));
    if (out->count) MHS_HIP(hipMemcpyAsync(out->count, d.count, 4 * n, hipMemcpyDeviceToHost, st));
    if (out->value) MHS_HIP(hipMemcpyAsync(out->value, d.value, vsz * n, hipMemcpyDeviceToHost, st));
    MHS_HIP(hipStreamSynchronize(st));
    mine.scratch_bytes += (int64_t)total;
    if (info) *info = mine;
    return MHS_OK;
}

}  // extern "C"
