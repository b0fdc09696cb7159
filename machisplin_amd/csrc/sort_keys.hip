// A deterministic LSD radix sort of 64-bit keys, 8 bits a pass (include/machisplin_hip.h, section "sort"; sort_keys.h holds the
// constants).  A key's place in every pass is COMPUTED FROM RANKS and never handed out by an atomic: the order of equal digits
// is the order of the input, whatever the order in which waves and workgroups run, so every pass is stable and a repeated call
// gives the same bytes.  The only atomics here are integer ADDS INTO HISTOGRAMS, whose totals do not depend on their order.
//
// Every phase is its own launch on the stream; a kernel boundary is the only ordering between them.
//   0   sort_digits_kernel   ONE pass over the keys takes the histograms of ALL digits of the window (LDS histograms, one global
//                            add per occupied bin and workgroup).  The host reads them (the one synchronisation) and leaves out
//                            every digit whose histogram has a single occupied bin: such a pass would be the identity.
//   per remaining digit:
//   1   sort_count_kernel    a workgroup per TILE of SORT_TILE_KEYS keys: the tile's count of each bin, to counts[bin][tile].
//   2   sort_scan_kernel     a workgroup per bin: the row counts[bin][.] becomes its exclusive prefix sum over the tiles plus
//                            the number of keys in smaller bins (from the digit's upfront histogram) -- the global place of the
//                            tile's first key of that bin.
//   3   sort_scatter_kernel  a workgroup per tile.  Wave w holds keys w * 512 + k * 64 + lane of the tile in round k: lanes, then
//                            rounds, then waves are in input order.  Per round a lane finds its digit's PEERS in the wave by
//                            eight ballots (one per digit bit); its rank in the wave is the wave's running count of the digit,
//                            kept in LDS and advanced by the peers' lowest lane, plus the peers below it.  After a barrier
//                            thread d sums bin d over the waves; a block scan over the bins gives each bin's first slot in the
//                            tile.  Every key goes to its slot of an LDS stage IN DIGIT ORDER, and after another barrier thread
//                            j takes slot j, j + 256, ...: a bin's run leaves as contiguous stores to place[bin] + its offset in
//                            the run.
// The passes ping-pong between `keys` and the second buffer; after an odd number the result is copied back.
//
// Bounds: every index into keys / alt is below n (a lane whose index is not takes no part in a ballot's peers and stores
// nothing); a slot of the stage is below the tile's number of keys <= SORT_TILE_KEYS; counts is indexed by bin * n_tiles + tile.
// LDS: 16 KiB of stage + 4 KiB of per-wave counts + 3 KiB per workgroup of phase 3; 8 KiB in phase 0.
#include <algorithm>
#include <cstring>
#include "zonal_int.h"

namespace mhs {

constexpr int SK_WAVES = SORT_THREADS / 64;
constexpr int SK_WAVE_KEYS = SORT_TILE_KEYS / SK_WAVES;
static_assert(SORT_THREADS == SORT_RADIX, "thread d of a workgroup owns bin d");

__device__ inline unsigned sk_digit(uint64_t key, int shift, unsigned mask) { return (unsigned)(key >> shift) & mask; }

// 0.  hist[p * 256 + b]: the keys whose digit p is b.  The last digit of the window may be narrower than 8 bits (mask_last).
__global__ __launch_bounds__(SORT_THREADS) void sort_digits_kernel(const uint64_t *__restrict__ keys, const int64_t n, const int bit_lo, const int n_digits,
                                                                   const unsigned mask_last, unsigned *__restrict__ hist) {
    __shared__ unsigned h[SORT_MAX_PASSES * SORT_RADIX];
    for (int i = threadIdx.x; i < SORT_MAX_PASSES * SORT_RADIX; i += SORT_THREADS) h[i] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * SORT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SORT_THREADS) {
        const uint64_t k = keys[i];
        for (int p = 0; p < n_digits; ++p)
            atomicAdd(&h[p * SORT_RADIX + sk_digit(k, bit_lo + p * SORT_RADIX_BITS, p == n_digits - 1 ? mask_last : (unsigned)(SORT_RADIX - 1))], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_digits * SORT_RADIX; i += SORT_THREADS)
        if (h[i]) atomicAdd(&hist[i], h[i]);
}

// 1
__global__ __launch_bounds__(SORT_THREADS) void sort_count_kernel(const uint64_t *__restrict__ keys, const int64_t n, const int shift, const unsigned mask,
                                                                  const unsigned n_tiles, unsigned *__restrict__ counts) {
    __shared__ unsigned h[SORT_RADIX];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * SORT_TILE_KEYS;
#pragma unroll
    for (int k = 0; k < SORT_KEYS_PER_LANE; ++k) {
        const int64_t i = base + k * SORT_THREADS + threadIdx.x;
        if (i < n) atomicAdd(&h[sk_digit(keys[i], shift, mask)], 1u);
    }
    __syncthreads();
    counts[(size_t)threadIdx.x * n_tiles + blockIdx.x] = h[threadIdx.x];
}

// inclusive scan over the 256 threads of a workgroup; part: SK_WAVES ints of LDS.  Returns the inclusive value, *total the sum.
__device__ inline unsigned sk_block_scan(unsigned v, unsigned *part, unsigned *total) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned x = __shfl_up(incl, d, 64);
        if (lane >= d) incl += x;
    }
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SK_WAVES; ++w) {
        if (w < wave) before += part[w];
        all += part[w];
    }
    __syncthreads();
    *total = all;
    return before + incl;
}

// 2.  blockIdx.x = the bin.  hist: the 256 bins of this digit's upfront histogram.
__global__ __launch_bounds__(SORT_THREADS) void sort_scan_kernel(const unsigned n_tiles, const unsigned *__restrict__ hist, unsigned *counts) {
    __shared__ unsigned part[SK_WAVES];
    const unsigned bin = blockIdx.x;
    unsigned total;
    const unsigned below = sk_block_scan(threadIdx.x < bin ? hist[threadIdx.x] : 0u, part, &total);
    (void)below;
    unsigned carry = total;                                                // the keys in smaller bins
    unsigned *row = counts + (size_t)bin * n_tiles;
    for (unsigned first = 0; first < n_tiles; first += SORT_THREADS) {
        const unsigned t = first + threadIdx.x;
        const unsigned v = t < n_tiles ? row[t] : 0u;
        unsigned sum;
        const unsigned incl = sk_block_scan(v, part, &sum);
        if (t < n_tiles) row[t] = carry + incl - v;
        carry += sum;
    }
}

// 3
__global__ __launch_bounds__(SORT_THREADS) void sort_scatter_kernel(const uint64_t *__restrict__ in, uint64_t *__restrict__ out, const int64_t n,
                                                                    const int shift, const unsigned mask, const unsigned n_tiles,
                                                                    const unsigned *__restrict__ place) {
    __shared__ uint64_t stage[SORT_TILE_KEYS];
    __shared__ unsigned wave_cnt[SK_WAVES][SORT_RADIX];                    // running count, then the count of the waves before
    __shared__ unsigned first_slot[SORT_RADIX], goes_to[SORT_RADIX], part[SK_WAVES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t base = (int64_t)blockIdx.x * SORT_TILE_KEYS;
    const int tile_n = (int)min((int64_t)SORT_TILE_KEYS, n - base);
#pragma unroll
    for (int w = 0; w < SK_WAVES; ++w) wave_cnt[w][threadIdx.x] = 0;
    __syncthreads();
    uint64_t key[SORT_KEYS_PER_LANE];
    unsigned rank[SORT_KEYS_PER_LANE];                                     // among the wave's keys of the same digit
    const uint64_t lanes_below = (1ull << lane) - 1ull;
#pragma unroll
    for (int k = 0; k < SORT_KEYS_PER_LANE; ++k) {
        const int j = wave * SK_WAVE_KEYS + k * 64 + lane;
        const bool valid = j < tile_n;
        key[k] = valid ? in[base + j] : 0ull;
        const unsigned d = sk_digit(key[k], shift, mask);
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < SORT_RADIX_BITS; ++b) {
            const uint64_t m = __ballot((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? m : ~m;
        }
        const unsigned before = valid ? wave_cnt[wave][d] : 0u;
        rank[k] = before + (unsigned)__popcll(peers & lanes_below);
        __builtin_amdgcn_wave_barrier();                                   // every lane has read the count before a lane advances it
        if (valid && (peers & lanes_below) == 0ull) wave_cnt[wave][d] = before + (unsigned)__popcll(peers);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    {   // thread d: bin d over the waves, then over the bins
        const unsigned d = threadIdx.x;
        unsigned sum = 0;
#pragma unroll
        for (int w = 0; w < SK_WAVES; ++w) {
            const unsigned c = wave_cnt[w][d];
            wave_cnt[w][d] = sum;
            sum += c;
        }
        unsigned total;
        const unsigned incl = sk_block_scan(sum, part, &total);
        first_slot[d] = incl - sum;
        goes_to[d] = place[(size_t)d * n_tiles + blockIdx.x];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SORT_KEYS_PER_LANE; ++k) {
        const int j = wave * SK_WAVE_KEYS + k * 64 + lane;
        if (j >= tile_n) continue;
        const unsigned d = sk_digit(key[k], shift, mask);
        stage[first_slot[d] + wave_cnt[wave][d] + rank[k]] = key[k];
    }
    __syncthreads();
    for (int j = threadIdx.x; j < tile_n; j += SORT_THREADS) {
        const uint64_t v = stage[j];
        const unsigned d = sk_digit(v, shift, mask);
        out[(int64_t)goes_to[d] + (int64_t)((unsigned)j - first_slot[d])] = v;
    }
}

int sort_keys_run(const char *fn, uint64_t *keys, uint64_t *alt, void *counts_block, int64_t n, int bit_lo, int bit_hi, hipStream_t st, int *passes_run,
                  uint64_t **where) {
    (void)fn;
    const int n_digits = sort_digits(bit_lo, bit_hi);
    const unsigned n_tiles = (unsigned)sort_tiles(n);
    unsigned *counts = (unsigned *)counts_block;
    unsigned *hist = (unsigned *)((char *)counts_block + sort_align((size_t)n_tiles * SORT_TILE_BYTES));
    int passes = 0;
    uint64_t *src = keys, *dst = alt;
    if (n_digits > 0) {
        const int last_bits = bit_hi - bit_lo - (n_digits - 1) * SORT_RADIX_BITS;
        const unsigned mask_last = (1u << last_bits) - 1u;
        const int n_cu = ctx().n_cu > 0 ? ctx().n_cu : 256;
        MHS_HIP(hipMemsetAsync(hist, 0, SORT_HIST_BYTES, st));
        const unsigned nb = (unsigned)std::min<int64_t>((n + SORT_THREADS - 1) / SORT_THREADS, (int64_t)n_cu * 8);
        hipLaunchKernelGGL(sort_digits_kernel, dim3(nb), dim3(SORT_THREADS), 0, st, (const uint64_t *)keys, n, bit_lo, n_digits, mask_last, hist);
        MHS_HIP(hipGetLastError());
        static_assert(SORT_HIST_BYTES == sizeof(unsigned) * SORT_MAX_PASSES * SORT_RADIX, "the histograms' block");
        unsigned host[SORT_MAX_PASSES * SORT_RADIX];
        MHS_HIP(hipMemcpyAsync(host, hist, SORT_HIST_BYTES, hipMemcpyDeviceToHost, st));
        MHS_HIP(hipStreamSynchronize(st));
        for (int p = 0; p < n_digits; ++p) {
            int occupied = 0;
            for (int b = 0; b < SORT_RADIX; ++b) occupied += host[p * SORT_RADIX + b] != 0u;
            if (occupied <= 1) continue;                                   // every key has the same digit: the pass is the identity
            const int shift = bit_lo + p * SORT_RADIX_BITS;
            const unsigned mask = p == n_digits - 1 ? mask_last : (unsigned)(SORT_RADIX - 1);
            hipLaunchKernelGGL(sort_count_kernel, dim3(n_tiles), dim3(SORT_THREADS), 0, st, (const uint64_t *)src, n, shift, mask, n_tiles, counts);
            MHS_HIP(hipGetLastError());
            hipLaunchKernelGGL(sort_scan_kernel, dim3(SORT_RADIX), dim3(SORT_THREADS), 0, st, n_tiles, (const unsigned *)(hist + p * SORT_RADIX), counts);
            MHS_HIP(hipGetLastError());
            hipLaunchKernelGGL(sort_scatter_kernel, dim3(n_tiles), dim3(SORT_THREADS), 0, st, (const uint64_t *)src, dst, n, shift, mask, n_tiles,
                               (const unsigned *)counts);
            MHS_HIP(hipGetLastError());
            std::swap(src, dst);
            ++passes;
        }
    }
    if (passes_run) *passes_run = passes;
    if (where) *where = src;
    else if (src != keys) MHS_HIP(hipMemcpyAsync(keys, src, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
    return MHS_OK;
}

}  // namespace mhs

using namespace mhs;

extern "C" {

int mhs_sort_keys_dev(uint64_t *keys, int64_t n, int bit_lo, int bit_hi, void *stream, mhs_sort_info *info) {
    const char *fn = __func__;
    ZN_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX, "%s: n must be in 0 .. 2^31 - 1", fn);
    ZN_REQUIRE(bit_lo >= 0 && bit_lo <= bit_hi && bit_hi <= 64, "%s: the window needs 0 <= bit_lo <= bit_hi <= 64", fn);
    ZN_REQUIRE(keys || n == 0, "%s: keys is NULL", fn);
    if (int rc = require_ready()) return rc;
    if (info) *info = mhs_sort_info{0, 0};
    if (n == 0) return MHS_OK;
    hipStream_t st = pick_stream(stream);
    const size_t bytes = sort_scratch_bytes(n);
    ZonalScratch s;
    if (int rc = s.get(fn, bytes, st, "the second key buffer and the tiles' digit counts")) return rc;
    int passes = 0;
    if (int rc = sort_keys_run(fn, keys, (uint64_t *)s.p, s.p + sort_align((size_t)n * 8), n, bit_lo, bit_hi, st, &passes, nullptr)) return rc;
    if (info) *info = mhs_sort_info{passes, (int64_t)bytes};
    return MHS_OK;
}

}  // extern "C"
