// Connected patches of one plane's feature cells (include/machisplin_hip.h, section "patches", states the rule; patches_rule.h
// holds it): label = the smallest cell number of the cell's patch, and the products made from it -- id, size, edge, keep.
//
// Block-based union-find over the int32 label plane, one word per cell: -1, or the cell number of the cell's parent.
//
// THE DESCENT INVARIANT (patches_rule.h states it in full).  Every word of the label plane, at every moment of every phase,
// holds either -1 or a cell number less than or equal to its own index.  Pointers only descend, so no find loop can cycle,
// whatever the interleaving; no loop here has an iteration cap.  It holds by construction: links are made only by atomicMin,
// and only from the larger root to the smaller (patch_union); every other store writes a cell's own root.
//
// Every phase is its own launch on the stream, and a kernel boundary is the only ordering between phases: no cross-block flag
// protocol, no host decision between launches.
//   1   patch_tile_kernel     a workgroup per tile of PATCH_TILE_ROWS x PATCH_TILE_COLS cells, a wave per row at a time.  The
//                             row's feature flags are one ballot, kept in LDS; every feature cell starts at the head of its row
//                             run, so only run heads enter the union; the rows are joined through patch_up_links by the
//                             lock-free union on the tile's words in LDS.  Every feature cell then writes the GLOBAL cell number
//                             of its tile-local root, which is the smallest cell number of its tile-local patch.  When a count
//                             is wanted, the tile's share of phase 4 happens here, where the tile-local roots are known: run
//                             heads add their run's length and edge flag to their root's word in LDS, and the tile writes the
//                             count table -- that word at a tile-local root, 0 at every other cell.
//   2   patch_border_kernel   a lane per cell on a tile's south or east edge: union with the feature neighbours across the edge
//                             (patches_rule.h says which links are made).  find reads with relaxed agent-scope atomic loads; the
//                             links are vector atomicMin on the label plane.
//   3   patch_flatten_kernel  every feature cell: label = find(cell).
//   4   patch_counts_kernel   every tile-local root that is not its patch's root adds its word to the root's: one integer
//                             atomicAdd (and an atomicOr for the edge bit) per (tile, patch).  Integer atomics: the sums do not
//                             depend on the order.
//   5   patch_roots_kernel    per block of PATCH_SCAN_BLOCK cells the number of roots (label == cell) -- and the info's counts, from
//                             the roots' words (the feature cells are the sum of the sizes: no phase counts them apart),
//       patch_scan_kernel     the exclusive prefix sum of the blocks' numbers (one workgroup),
//       patch_ids_kernel      and the rank of every root inside its block: id = 1 + the number of roots before it.
//   6   patch_products_kernel size, edge, id, keep through label from the two tables, -1 / 0 on a non-feature cell.
// A phase runs only when a requested product (or the info) needs it; a plane of one tile skips 2 and 3.
//
// Scratch, per cell: the label plane 4 (none when `label` is requested with ld = ncol: it is then written in place), the count
// table 4 (size in 31 bits, the edge flag in the top bit), the id table 4: at most 12 bytes, plus 4 bytes per
// PATCH_SCAN_BLOCK cells (the blocks' root counts), the counters and 256-byte alignments, in ONE block of stream-ordered memory
// given back behind the last kernel.  LDS: 16.25 KiB per workgroup of phase 1.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <mutex>
#include "ensemble_int.h"
#include "patches_rule.h"

namespace mhs {

constexpr int PT_NT = 256;                   // threads per workgroup of every phase: 4 waves
constexpr int PT_WAVES = PT_NT / 64;
constexpr int PT_ROWS_PER_WAVE = PATCH_TILE_ROWS / PT_WAVES;
constexpr int PT_TILE = PATCH_TILE_ROWS * PATCH_TILE_COLS;
constexpr int PT_PER_THREAD = PATCH_SCAN_BLOCK / PT_NT;
static_assert(PATCH_TILE_COLS == 64, "a wave holds one tile row in its lanes");
static_assert(PATCH_TILE_ROWS % PT_WAVES == 0 && PATCH_SCAN_BLOCK % PT_NT == 0, "whole rows per wave, whole chunks per block");

struct PatchGeom {
    int nrow, ncol;
    double nodata;
    int has_nodata;
    int tiles_c;             // tiles side by side
};

struct PatchFilter {
    int min_size, max_size, edge_rule;
};

struct PatchCounters {
    unsigned long long n_features, n_patches, n_kept_patches, n_kept_cells;
    int max_size;
    int pad;
};

// the words of a tile in LDS
struct PatchLdsWords {
    int *w;
    __device__ int load(int i) const { return __hip_atomic_load(w + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ int fetch_min(int i, int v) { return atomicMin(w + i, v); }
};
// the label plane
struct PatchPlaneWords {
    int32_t *w;
    __device__ int load(int i) const { return __hip_atomic_load(w + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ int fetch_min(int i, int v) { return atomicMin(w + i, v); }
};

// 1
template <typename T, bool COUNTS>
__global__ __launch_bounds__(PT_NT) void patch_tile_kernel(const PatchGeom g, const T *__restrict__ z, const int64_t ldz, const int where,
                                                           const double threshold, const int connectivity, int32_t *__restrict__ label,
                                                           uint32_t *__restrict__ table) {
    __shared__ uint64_t rows[PATCH_TILE_ROWS];
    __shared__ int words[PT_TILE];
    __shared__ uint32_t agg[COUNTS ? PT_TILE : 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r0 = (int)(blockIdx.x / (unsigned)g.tiles_c) * PATCH_TILE_ROWS, c0 = (int)(blockIdx.x % (unsigned)g.tiles_c) * PATCH_TILE_COLS;
    const int c = c0 + lane;
    const bool has_nd = g.has_nodata != 0;
    PatchLdsWords a{words};
    uint64_t mine[PT_ROWS_PER_WAVE];
#pragma unroll
    for (int j = 0; j < PT_ROWS_PER_WAVE; ++j) {
        const int lr = wave * PT_ROWS_PER_WAVE + j, r = r0 + lr;
        const bool f = r < g.nrow && c < g.ncol && prox_is_feature((double)z[(int64_t)r * ldz + c], has_nd, g.nodata, where, threshold);
        const uint64_t m = __ballot(f);
        mine[j] = m;
        if (lane == 0) rows[lr] = m;
        words[lr * 64 + lane] = f ? lr * 64 + patch_run_start(m, lane) : -1;
        if (COUNTS) agg[lr * 64 + lane] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PT_ROWS_PER_WAVE; ++j) {
        const int lr = wave * PT_ROWS_PER_WAVE + j;
        if (lr == 0 || !((mine[j] >> lane) & 1)) continue;
        const int links = patch_up_links(mine[j], rows[lr - 1], lane, connectivity);
        const int me = lr * 64 + lane, above = me - 64;
        if (links & 1) patch_union(a, me, above);
        if (links & 2) patch_union(a, me, above - 1);
        if (links & 4) patch_union(a, me, above + 1);
    }
    __syncthreads();
    int root[PT_ROWS_PER_WAVE];
#pragma unroll
    for (int j = 0; j < PT_ROWS_PER_WAVE; ++j) {
        const int lr = wave * PT_ROWS_PER_WAVE + j, r = r0 + lr;
        const bool f = (mine[j] >> lane) & 1;
        root[j] = f ? patch_find(a, lr * 64 + lane) : -1;
        if (r < g.nrow && c < g.ncol)
            label[(int64_t)r * g.ncol + c] = f ? (int32_t)((int64_t)(r0 + (root[j] >> 6)) * g.ncol + c0 + (root[j] & 63)) : -1;
        if (COUNTS && f && patch_run_start(mine[j], lane) == lane) {
            const int len = patch_run_length(mine[j], lane);
            atomicAdd(&agg[root[j]], (uint32_t)len);
            if (r == 0 || r == g.nrow - 1 || c == 0 || c + len == g.ncol) atomicOr(&agg[root[j]], PATCH_EDGE_BIT);
        }
    }
    if (COUNTS) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PT_ROWS_PER_WAVE; ++j) {
            const int lr = wave * PT_ROWS_PER_WAVE + j, r = r0 + lr;
            if (r < g.nrow && c < g.ncol) table[(int64_t)r * g.ncol + c] = root[j] == lr * 64 + lane ? agg[lr * 64 + lane] : 0u;
        }
    }
}

// 2.  Lanes 0 .. n_south - 1: the cells of the rows that end a tile row and have a row below, row by row; the others: the cells
// of the columns that end a tile column and have a column to the right, column by column.
__global__ __launch_bounds__(PT_NT) void patch_border_kernel(const PatchGeom g, const int connectivity, const int64_t n_south, const int64_t n_east,
                                                             int32_t *label) {
    const int64_t t = (int64_t)blockIdx.x * PT_NT + threadIdx.x;
    if (t >= n_south + n_east) return;
    PatchPlaneWords a{label};
    const int ncol = g.ncol;
    auto feat = [&](int r, int c) { return a.load((int)((int64_t)r * ncol + c)) >= 0; };
    if (t < n_south) {
        const int r = (int)(t / ncol) * PATCH_TILE_ROWS + PATCH_TILE_ROWS - 1, c = (int)(t % ncol);
        if (!feat(r, c)) return;
        const int me = (int)((int64_t)r * ncol + c), below = me + ncol;
        const bool s = feat(r + 1, c), w = c > 0 && feat(r, c - 1), e = c + 1 < ncol && feat(r, c + 1);
        const bool sw = c > 0 && feat(r + 1, c - 1), se = c + 1 < ncol && feat(r + 1, c + 1);
        if (s && patch_south_link(w, sw, c)) patch_union(a, me, below);
        if (connectivity == 8) {
            if (sw && patch_diagonal_link(w, s)) patch_union(a, me, below - 1);
            if (se && patch_diagonal_link(e, s)) patch_union(a, me, below + 1);
        }
    } else {
        const int64_t u = t - n_south;
        const int c = (int)(u / g.nrow) * PATCH_TILE_COLS + PATCH_TILE_COLS - 1, r = (int)(u % g.nrow);
        if (!feat(r, c)) return;
        const int me = (int)((int64_t)r * ncol + c);
        const bool e = feat(r, c + 1);
        if (e) patch_union(a, me, me + 1);
        if (connectivity == 8) {
            if (r > 0 && feat(r - 1, c + 1) && patch_diagonal_link(feat(r - 1, c), e)) patch_union(a, me, me - ncol + 1);
            if (r + 1 < g.nrow && feat(r + 1, c + 1) && patch_diagonal_link(feat(r + 1, c), e)) patch_union(a, me, me + ncol + 1);
        }
    }
}

// 3
__global__ __launch_bounds__(PT_NT) void patch_flatten_kernel(const int64_t n, int32_t *label) {
    const int64_t i = (int64_t)blockIdx.x * PT_NT + threadIdx.x;
    if (i >= n) return;
    const int v = label[i];
    if (v < 0) return;
    PatchPlaneWords a{label};
    const int root = patch_find(a, v);
    if (root != v) __hip_atomic_store(label + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// 4.  A nonzero word of the table marks a tile-local root; a patch's root is one too, and keeps its own word.
// A patch that winds through many tiles gets a word from every one of them, all for the one root: the words of a block of
// PATCH_SCAN_BLOCK cells that go to the block's SMALLEST root (a spanning patch starts near the top of the plane) are summed in
// LDS first and leave as one atomic of the block.  Which root is chosen changes the number of atomics, never a sum.
__global__ __launch_bounds__(PT_NT) void patch_counts_kernel(const int64_t n, const int32_t *__restrict__ label, uint32_t *table) {
    __shared__ int hot_root;
    __shared__ uint32_t hot_size, hot_edge;
    if (threadIdx.x == 0) { hot_root = 0x7fffffff; hot_size = 0; hot_edge = 0; }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * PATCH_SCAN_BLOCK;
    uint32_t word[PT_PER_THREAD];
    int root[PT_PER_THREAD];
#pragma unroll
    for (int j = 0; j < PT_PER_THREAD; ++j) {
        const int64_t i = base + j * PT_NT + threadIdx.x;
        word[j] = i < n ? table[i] : 0u;
        root[j] = word[j] ? label[i] : -1;
        if (root[j] == (int)i) word[j] = 0;                        // the patch's root keeps its own word
        if (word[j]) atomicMin(&hot_root, root[j]);
    }
    __syncthreads();
    const int hot = hot_root;
#pragma unroll
    for (int j = 0; j < PT_PER_THREAD; ++j) {
        if (!word[j]) continue;
        if (root[j] == hot) {
            atomicAdd(&hot_size, word[j] & PATCH_SIZE_MASK);
            if (word[j] & PATCH_EDGE_BIT) atomicOr(&hot_edge, PATCH_EDGE_BIT);
        } else {
            atomicAdd(&table[root[j]], word[j] & PATCH_SIZE_MASK);
            if (word[j] & PATCH_EDGE_BIT) atomicOr(&table[root[j]], PATCH_EDGE_BIT);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && hot_size) {
        atomicAdd(&table[hot], hot_size);
        if (hot_edge) atomicOr(&table[hot], PATCH_EDGE_BIT);
    }
}

__device__ inline int pt_wave_sum(int v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// 5, the blocks' root counts and the counts of the info (table may be NULL: then only the roots are counted).  A workgroup takes
// blocks blockIdx.x, blockIdx.x + gridDim.x, ... and adds its counts to the counters once, at its end: four atomics per workgroup
// of a grid that the launch keeps to a few per CU, not per block of cells.
__global__ __launch_bounds__(PT_NT) void patch_roots_kernel(const int64_t n, const int64_t n_blocks, const int32_t *__restrict__ label,
                                                            const uint32_t *__restrict__ table, const PatchFilter flt, int32_t *__restrict__ block_roots,
                                                            PatchCounters *counters) {
    __shared__ int part[2][PT_WAVES];
    __shared__ int part_max[PT_WAVES];
    __shared__ unsigned long long part_cells[PT_WAVES], part_feats[PT_WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int kept = 0, biggest = 0;
    unsigned long long cells = 0, feats = 0, all_roots = 0;        // the kept patches' cells, all patches' cells, and (thread 0) the roots
    for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const int64_t base = b * PATCH_SCAN_BLOCK;
        int roots = 0;
#pragma unroll
        for (int j = 0; j < PT_PER_THREAD; ++j) {
            const int64_t i = base + j * PT_NT + threadIdx.x;
            if (i >= n || label[i] != (int)i) continue;
            ++roots;
            if (!table) continue;
            const uint32_t t = table[i];
            const int size = patch_size_of(t);
            biggest = max(biggest, size);
            feats += (unsigned long long)size;                     // every feature cell is in one patch: the sizes add up to n_features
            if (patch_keep(size, patch_edge_of(t), flt.min_size, flt.max_size, flt.edge_rule)) { ++kept; cells += (unsigned long long)size; }
        }
        roots = pt_wave_sum(roots);
        if (lane == 0) part[0][wave] = roots;
        __syncthreads();
        if (threadIdx.x == 0) {
            int r = 0;
            for (int w = 0; w < PT_WAVES; ++w) r += part[0][w];
            block_roots[b] = r;
            all_roots += (unsigned long long)r;
        }
        __syncthreads();
    }
    kept = pt_wave_sum(kept);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        cells += __shfl_xor(cells, d, 64);
        feats += __shfl_xor(feats, d, 64);
        biggest = max(biggest, __shfl_xor(biggest, d, 64));
    }
    if (lane == 0) {
        part[1][wave] = kept;
        part_max[wave] = biggest;
        part_cells[wave] = cells;
        part_feats[wave] = feats;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int k = 0, m = 0;
        unsigned long long c = 0, f = 0;
        for (int w = 0; w < PT_WAVES; ++w) { k += part[1][w]; m = max(m, part_max[w]); c += part_cells[w]; f += part_feats[w]; }
        if (c) atomicAdd(&counters->n_kept_cells, c);
        if (f) atomicAdd(&counters->n_features, f);
        if (all_roots) atomicAdd(&counters->n_patches, all_roots);
        if (k) atomicAdd(&counters->n_kept_patches, (unsigned long long)k);
        if (m) atomicMax(&counters->max_size, m);
    }
}

// 5, one workgroup: block_roots becomes its own exclusive prefix sum, chunk by chunk with a carry
__global__ __launch_bounds__(PT_NT) void patch_scan_kernel(const int64_t n_blocks, int32_t *block_roots) {
    __shared__ int wave_total[PT_WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int carry = 0;
    for (int64_t base = 0; base < n_blocks; base += PT_NT) {
        const int64_t i = base + threadIdx.x;
        const int v = i < n_blocks ? block_roots[i] : 0;
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < PT_WAVES; ++w) {
            if (w < wave) before += wave_total[w];
            total += wave_total[w];
        }
        if (i < n_blocks) block_roots[i] = carry + before + incl - v;
        carry += total;
        __syncthreads();
    }
}

// 5, the ids: cells base + q * 64 + lane, q = 0 .. 31, are in cell order
__global__ __launch_bounds__(PT_NT) void patch_ids_kernel(const int64_t n, const int32_t *__restrict__ label, const int32_t *__restrict__ block_before,
                                                          int32_t *__restrict__ ids) {
    __shared__ int count[PT_PER_THREAD * PT_WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * PATCH_SCAN_BLOCK;
    uint64_t is_root[PT_PER_THREAD];
#pragma unroll
    for (int j = 0; j < PT_PER_THREAD; ++j) {
        const int64_t i = base + j * PT_NT + threadIdx.x;
        is_root[j] = __ballot(i < n && label[i] == (int)i);
        if (lane == 0) count[j * PT_WAVES + wave] = __popcll(is_root[j]);
    }
    __syncthreads();
    const int first = block_before[blockIdx.x];
#pragma unroll
    for (int j = 0; j < PT_PER_THREAD; ++j) {
        if (!((is_root[j] >> lane) & 1)) continue;
        int before = first;
        for (int q = 0; q < j * PT_WAVES + wave; ++q) before += count[q];
        before += __popcll(is_root[j] & ((1ull << lane) - 1));
        ids[base + j * PT_NT + threadIdx.x] = before + 1;
    }
}

struct PatchPlanes {
    int32_t *label, *id, *size;
    uint8_t *edge, *keep;
};

// 6.  p.label is set only when the label plane is to be copied out of the scratch (ld != ncol)
__global__ __launch_bounds__(PT_NT) void patch_products_kernel(const PatchGeom g, const int32_t *__restrict__ label, const uint32_t *__restrict__ table,
                                                               const int32_t *__restrict__ ids, const PatchFilter flt, const PatchPlanes p,
                                                               const int64_t ld) {
    const int64_t i = (int64_t)blockIdx.x * PT_NT + threadIdx.x;
    if (i >= (int64_t)g.nrow * g.ncol) return;
    const int64_t o = i / g.ncol * ld + i % g.ncol;
    const int root = label[i];
    if (p.label) p.label[o] = root;
    const uint32_t t = (root >= 0 && table) ? table[root] : 0u;
    const int size = patch_size_of(t);
    if (p.size) p.size[o] = size;
    if (p.edge) p.edge[o] = (uint8_t)(root >= 0 ? patch_edge_of(t) : 0);
    if (p.keep) p.keep[o] = (uint8_t)(root >= 0 && patch_keep(size, patch_edge_of(t), flt.min_size, flt.max_size, flt.edge_rule));
    if (p.id) p.id[o] = root >= 0 ? ids[root] : 0;
}

#define PT_REQUIRE(cond, ...)                                              \
    do {                                                                   \
        if (!(cond)) { set_error(__VA_ARGS__); return MHS_ERR_INVALID; }    \
    } while (0)

// Every check of a patches call, before any device call; fn = the entry point's name for the message
static int patch_check(const char *fn, const mhs_grid *grid, const mhs_stack *stack, int layer, int where, double threshold, int connectivity,
                       int64_t min_size, int64_t max_size, int edge_rule, const mhs_patches_out *out, int64_t ld, PatchGeom *g, PatchFilter *flt) {
    PT_REQUIRE(grid && stack && out, "%s: NULL argument (g, stack or out)", fn);
    PT_REQUIRE(grid->nrow > 0 && grid->ncol > 0 && grid->nrow <= (int64_t)INT32_MAX && grid->ncol <= (int64_t)INT32_MAX,
               "%s: bad grid geometry (nrow, ncol must be in 1 .. 2^31 - 1)", fn);
    PT_REQUIRE(grid->nrow * grid->ncol <= (int64_t)INT32_MAX, "%s: grid too large: nrow * ncol must not pass 2^31 - 1 (label is an int32)", fn);
    PT_REQUIRE(stack->data, "%s: stack data is NULL", fn);
    PT_REQUIRE(stack->dtype == MHS_F64 || stack->dtype == MHS_F32 || stack->dtype == MHS_I16, "%s: bad stack dtype", fn);
    PT_REQUIRE(layer >= 0 && layer < stack->n_layers, "%s: layer %d is not one of the stack's %d layers", fn, layer, stack->n_layers);
    PT_REQUIRE(stack->ld >= grid->ncol && (stack->n_layers == 1 || stack->plane_stride >= stack->ld * (grid->nrow - 1) + grid->ncol),
               "%s: stack strides smaller than the grid", fn);
    PT_REQUIRE(where >= 0 && where < PROX_WHERES, "%s: unknown where %d (MHS_PROX_NA .. MHS_PROX_NE)", fn, where);
    PT_REQUIRE(where < PROX_LT || !std::isnan(threshold), "%s: threshold must not be NaN for a comparison", fn);
    PT_REQUIRE(connectivity == 4 || connectivity == 8, "%s: connectivity must be 4 or 8, not %d", fn, connectivity);
    PT_REQUIRE(min_size >= 1, "%s: min_size must be at least 1", fn);
    PT_REQUIRE(max_size >= min_size, "%s: max_size must not be below min_size", fn);
    PT_REQUIRE(edge_rule >= 0 && edge_rule < PATCH_EDGE_RULES, "%s: unknown edge_rule %d (MHS_PATCH_EDGE_ANY .. MHS_PATCH_EDGE_INTERIOR)", fn, edge_rule);
    PT_REQUIRE(out->label || out->id || out->size || out->edge || out->keep, "%s: out names no product (label, id, size, edge, keep are all NULL)", fn);
    PT_REQUIRE(ld >= grid->ncol, "%s: ld smaller than the grid width", fn);
    *g = PatchGeom{(int)grid->nrow, (int)grid->ncol, stack->nodata, !std::isnan(stack->nodata),
                   (int)((grid->ncol + PATCH_TILE_COLS - 1) / PATCH_TILE_COLS)};
    *flt = PatchFilter{(int)std::min<int64_t>(min_size, (int64_t)INT32_MAX), (int)std::min<int64_t>(max_size, (int64_t)INT32_MAX), edge_rule};
    return MHS_OK;
}

// the call's one block of stream-ordered memory, given back behind whatever was enqueued last
struct PatchScratch {
    char *p = nullptr;
    hipStream_t st = nullptr;
    ~PatchScratch() { if (p) (void)hipFreeAsync(p, st); }
};

static size_t pt_align(size_t n) { return (n + 255) & ~(size_t)255; }

template <typename T>
static void launch_patch_tile(bool counts, const PatchGeom &g, unsigned n_tiles, hipStream_t st, const void *z, int64_t ldz, int where, double threshold,
                              int connectivity, int32_t *label, uint32_t *table) {
    if (counts)
        hipLaunchKernelGGL((patch_tile_kernel<T, true>), dim3(n_tiles), dim3(PT_NT), 0, st, g, (const T *)z, ldz, where, threshold, connectivity, label,
                           table);
    else
        hipLaunchKernelGGL((patch_tile_kernel<T, false>), dim3(n_tiles), dim3(PT_NT), 0, st, g, (const T *)z, ldz, where, threshold, connectivity, label,
                           table);
}

// Device planes.  `plane` = element (0, 0) of the feature layer, of `dtype`, with the row stride ldz.
static int patch_run(const char *fn, const PatchGeom &g, const PatchFilter &flt, int dtype, const void *plane, int64_t ldz, int where, double threshold,
                     int connectivity, const mhs_patches_out &out, int64_t ld, hipStream_t st, mhs_patches_info *info) {
    const size_t n = (size_t)g.nrow * (size_t)g.ncol;
    const bool in_place = out.label && ld == g.ncol;
    const bool need_table = out.size || out.edge || out.keep || info, need_ids = out.id != nullptr, need_roots = need_ids || info;
    const size_t n_blocks = (n + PATCH_SCAN_BLOCK - 1) / PATCH_SCAN_BLOCK;
    const size_t o_label = 0, o_table = o_label + (in_place ? 0 : pt_align(4 * n)), o_ids = o_table + (need_table ? pt_align(4 * n) : 0),
                 o_blocks = o_ids + (need_ids ? pt_align(4 * n) : 0), o_cnt = o_blocks + (need_roots ? pt_align(4 * n_blocks) : 0),
                 total = o_cnt + pt_align(sizeof(PatchCounters));
    PatchScratch s;
    s.st = st;
    if (hipMallocAsync((void **)&s.p, total, st) != hipSuccess) {
        (void)hipGetLastError();
        s.p = nullptr;
        set_error("%s: no device memory for the scratch planes (%zu bytes: at most 12 per cell)", fn, total);
        return MHS_ERR_ALLOC;
    }
    int32_t *label = in_place ? out.label : (int32_t *)(s.p + o_label);
    uint32_t *table = need_table ? (uint32_t *)(s.p + o_table) : nullptr;
    int32_t *ids = need_ids ? (int32_t *)(s.p + o_ids) : nullptr, *blocks = need_roots ? (int32_t *)(s.p + o_blocks) : nullptr;
    PatchCounters *counters = (PatchCounters *)(s.p + o_cnt);
    MHS_HIP(hipMemsetAsync(counters, 0, sizeof(PatchCounters), st));
    const int64_t tiles_r = ((int64_t)g.nrow + PATCH_TILE_ROWS - 1) / PATCH_TILE_ROWS, n_tiles = tiles_r * g.tiles_c;
    const unsigned nb_cells = (unsigned)((n + PT_NT - 1) / PT_NT);
    if (dtype == MHS_F64) launch_patch_tile<double>(need_table, g, (unsigned)n_tiles, st, plane, ldz, where, threshold, connectivity, label, table);
    else if (dtype == MHS_F32) launch_patch_tile<float>(need_table, g, (unsigned)n_tiles, st, plane, ldz, where, threshold, connectivity, label, table);
    else launch_patch_tile<short>(need_table, g, (unsigned)n_tiles, st, plane, ldz, where, threshold, connectivity, label, table);
    MHS_HIP(hipGetLastError());
    if (n_tiles > 1) {
        const int64_t n_south = (int64_t)((g.nrow - 1) / PATCH_TILE_ROWS) * g.ncol, n_east = (int64_t)((g.ncol - 1) / PATCH_TILE_COLS) * g.nrow;
        hipLaunchKernelGGL(patch_border_kernel, dim3((unsigned)((n_south + n_east + PT_NT - 1) / PT_NT)), dim3(PT_NT), 0, st, g, connectivity, n_south,
                           n_east, label);
        MHS_HIP(hipGetLastError());
        hipLaunchKernelGGL(patch_flatten_kernel, dim3(nb_cells), dim3(PT_NT), 0, st, (int64_t)n, label);
        MHS_HIP(hipGetLastError());
        if (need_table) {
            hipLaunchKernelGGL(patch_counts_kernel, dim3((unsigned)n_blocks), dim3(PT_NT), 0, st, (int64_t)n, label, table);
            MHS_HIP(hipGetLastError());
        }
    }
    if (need_roots) {
        const int n_cu = ctx().n_cu > 0 ? ctx().n_cu : 256;
        hipLaunchKernelGGL(patch_roots_kernel, dim3((unsigned)std::min<size_t>(n_blocks, (size_t)n_cu * 8)), dim3(PT_NT), 0, st, (int64_t)n,
                           (int64_t)n_blocks, label, table, flt, blocks, counters);
        MHS_HIP(hipGetLastError());
    }
    if (need_ids) {
        hipLaunchKernelGGL(patch_scan_kernel, dim3(1), dim3(PT_NT), 0, st, (int64_t)n_blocks, blocks);
        MHS_HIP(hipGetLastError());
        hipLaunchKernelGGL(patch_ids_kernel, dim3((unsigned)n_blocks), dim3(PT_NT), 0, st, (int64_t)n, label, blocks, ids);
        MHS_HIP(hipGetLastError());
    }
    const PatchPlanes p{in_place ? nullptr : out.label, out.id, out.size, out.edge, out.keep};
    if (p.label || p.id || p.size || p.edge || p.keep) {
        hipLaunchKernelGGL(patch_products_kernel, dim3(nb_cells), dim3(PT_NT), 0, st, g, label, table, ids, flt, p, ld);
        MHS_HIP(hipGetLastError());
    }
    if (info) {
        PatchCounters c;
        MHS_HIP(hipMemcpyAsync(&c, counters, sizeof(c), hipMemcpyDeviceToHost, st));
        MHS_HIP(hipStreamSynchronize(st));
        *info = mhs_patches_info{(int64_t)c.n_features, (int64_t)c.n_patches, (int64_t)c.n_kept_patches, (int64_t)c.n_kept_cells, (int64_t)c.max_size,
                                 (int64_t)total};
    }
    return MHS_OK;
}

}  // namespace mhs

using namespace mhs;

extern "C" {

int mhs_patches_dev(const mhs_grid *g, const mhs_stack *stack, int layer, int where, double threshold, int connectivity, int64_t min_size,
                    int64_t max_size, int edge_rule, const mhs_patches_out *out, int64_t ld, void *stream, mhs_patches_info *info) {
    PatchGeom pg;
    PatchFilter flt;
    if (int rc = patch_check(__func__, g, stack, layer, where, threshold, connectivity, min_size, max_size, edge_rule, out, ld, &pg, &flt)) return rc;
    if (int rc = require_ready()) return rc;
    const void *plane = (const char *)stack->data + (size_t)layer * stack->plane_stride * dtype_bytes(stack->dtype);
    return patch_run(__func__, pg, flt, stack->dtype, plane, stack->ld, where, threshold, connectivity, *out, ld, pick_stream(stream), info);
}

// Host planes: the WHOLE feature plane goes up and the requested planes come down.  No row bands: a patch may wind through any
// row of the raster.
int mhs_patches(const mhs_grid *g, const mhs_stack *stack, int layer, int where, double threshold, int connectivity, int64_t min_size, int64_t max_size,
                int edge_rule, const mhs_patches_out *out, mhs_patches_info *info) {
    PatchGeom pg;
    PatchFilter flt;
    const char *fn = __func__;
    if (int rc = patch_check(fn, g, stack, layer, where, threshold, connectivity, min_size, max_size, edge_rule, out, g ? g->ncol : 0, &pg, &flt)) return rc;
    if (int rc = require_ready()) return rc;
    const size_t esz = dtype_bytes(stack->dtype), n = (size_t)pg.nrow * (size_t)pg.ncol;
    const size_t in_bytes = ((size_t)(pg.nrow - 1) * stack->ld + pg.ncol) * esz;
    void *const host[5] = {out->label, out->id, out->size, out->edge, out->keep};
    const size_t bytes[5] = {4 * n, 4 * n, 4 * n, n, n};
    size_t off[5], total = pt_align(in_bytes);
    for (int k = 0; k < 5; ++k) { off[k] = total; total += host[k] ? pt_align(bytes[k]) : 0; }
    std::lock_guard<std::mutex> lk(pipe_mutex());
    if (int rc = host_pipe(0)) return rc;                      // the pipeline's streams; its arena is not used
    hipStream_t st = ctx().pipe_comp;
    PatchScratch s;
    s.st = st;
    if (hipMallocAsync((void **)&s.p, total, st) != hipSuccess) {
        (void)hipGetLastError();
        s.p = nullptr;
        set_error("%s: no device memory for the plane and its outputs (%zu bytes)", fn, total);
        return MHS_ERR_ALLOC;
    }
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{st};   // no copy is left in flight, whatever the exit
    MHS_HIP(hipMemcpyAsync(s.p, (const char *)stack->data + (size_t)layer * stack->plane_stride * esz, in_bytes, hipMemcpyHostToDevice, st));
    void *dev[5];
    for (int k = 0; k < 5; ++k) dev[k] = host[k] ? s.p + off[k] : nullptr;
    const mhs_patches_out dout{(int32_t *)dev[0], (int32_t *)dev[1], (int32_t *)dev[2], (uint8_t *)dev[3], (uint8_t *)dev[4]};
    if (int rc = patch_run(fn, pg, flt, stack->dtype, s.p, stack->ld, where, threshold, connectivity, dout, pg.ncol, st, info)) return rc;
    for (int k = 0; k < 5; ++k)
        if (host[k]) MHS_HIP(hipMemcpyAsync(host[k], s.p + off[k], bytes[k], hipMemcpyDeviceToHost, st));
    MHS_HIP(hipStreamSynchronize(st));
    return MHS_OK;
}

}  // extern "C"
