// The device sort of 64-bit keys (include/machisplin_hip.h, section "sort"): the constants that sort_keys.hip is built from and
// tests/test_sort_keys_gpu.py reads from this text, the host helpers that size its scratch, and the internal entry that
// quantile.hip calls with scratch of its own.  Free of any HIP header.
#pragma once

#include <cstddef>
#include <cstdint>

namespace mhs {

constexpr int SORT_RADIX_BITS = 8;                       // bits of a digit: 256 bins
constexpr int SORT_RADIX = 1 << SORT_RADIX_BITS;
constexpr int SORT_THREADS = 256;                        // a workgroup: 4 waves of 64
constexpr int SORT_KEYS_PER_LANE = 8;                    // rounds of a wave over its part of the tile
constexpr int SORT_TILE_KEYS = 2048;                     // keys of a tile = SORT_THREADS * SORT_KEYS_PER_LANE: 16 KiB staged in LDS
constexpr int SORT_MAX_PASSES = 64 / SORT_RADIX_BITS;    // 8
constexpr int SORT_TILE_BYTES = 1024;                   // scratch per tile: one uint32 per bin
static_assert(SORT_TILE_BYTES == SORT_RADIX * 4, "one uint32 per bin");
constexpr int SORT_HIST_BYTES = SORT_MAX_PASSES * SORT_RADIX * 4;   // the upfront histograms of all digits: 8 KiB
static_assert(SORT_TILE_KEYS == SORT_THREADS * SORT_KEYS_PER_LANE, "a tile is what a workgroup holds in registers");

inline int64_t sort_tiles(int64_t n) { return (n + SORT_TILE_KEYS - 1) / SORT_TILE_KEYS; }
inline size_t sort_align(size_t b) { return (b + 255) & ~(size_t)255; }
// what a sort of n keys needs beside its second key buffer: the per-tile digit counts of ONE pass and the upfront histograms
inline size_t sort_counts_bytes(int64_t n) { return sort_align((size_t)sort_tiles(n) * SORT_TILE_BYTES) + SORT_HIST_BYTES; }
// the whole scratch of mhs_sort_keys_dev
inline size_t sort_scratch_bytes(int64_t n) { return n > 0 ? sort_align((size_t)n * 8) + sort_counts_bytes(n) : 0; }

// number of 8-bit digits of the window [bit_lo, bit_hi)
inline int sort_digits(int bit_lo, int bit_hi) { return (bit_hi - bit_lo + SORT_RADIX_BITS - 1) / SORT_RADIX_BITS; }

}  // namespace mhs
