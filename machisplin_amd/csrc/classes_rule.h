// The rule of categorical layers (include/machisplin_hip.h, section "classes"): the class of a cell, and what follows from the
// EXACT INTEGER class counts of a unit -- a zone, a target cell of another geometry, a window.  Free of any HIP header: the
// kernels of classes.hip, its host checks and a plain C++ check program (tests/classes_check.cpp) share it.
//
// A value v (converted exactly to double) that is not NA has the CODE (int)v when it is an integer in 0 .. 65 535, else none.
// The class list holds K distinct codes, 1 <= K <= 256, ascending; a valid cell has class index k when its code is codes[k],
// and is OTHER when it has no code or its code is not listed.  Per unit: count[k], other, and n = sum count + other.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define CLS_HD __host__ __device__
#else
#define CLS_HD
#endif

namespace mhs {

constexpr int CLS_MAX_K = 256;              // classes of a list at most
constexpr int CLS_MAX_CODE = 65535;         // a code is in 0 .. 65 535
constexpr int CLS_TABLE_SPAN = 1024;        // max code - min code below this: a direct table; else bisection
constexpr int CLS_BISECT_STEPS = 9;         // halvings of an interval of 256: 256, 128, .. 1, 0

// The sizes at which classes.hip changes path; tests/test_classes_gpu.py reads them from this text.
constexpr int CLS_TILE_ROWS = 32;           // class_zone_kernel: rows of a tile
constexpr int CLS_TILE_COLS = 64;           //   and its columns: a wave holds a tile row in its lanes
constexpr int CLS_STRIP_TILES = 8;          //   tiles, one below the other, that a workgroup takes before it flushes its LDS table
constexpr int CLS_LDS_SLOTS = 1024;         //   slots of the workgroup's open-addressed table, a power of two
constexpr int CLS_PROBES = 4;               //   slots a run tries before its length goes straight to the global table
constexpr int CLS_AGG_WORDS = 16384;        // class_aggregate_kernel: 64 KiB of uint32 counters per workgroup
constexpr int CLS_AGG_SIDE = 64;            //   target rows, and target columns, of a tile at most
constexpr int CLS_AGG_MIN_TILES = 2048;     //   fewer tiles than this: the tile is halved, rows first, so that the device is filled
constexpr int CLS_AGG_MIN_COLS = 4;         //   ... then its columns, down to this

// a plane value converted exactly to double is NA when it is NaN or equals the stack's nodata
CLS_HD inline bool cls_na(double v, bool has_nodata, double nodata) { return v != v || (has_nodata && v == nodata); }

// the code of a valid value, -1 where it has none (non-integral, negative, above 65 535, +-Inf)
CLS_HD inline int cls_code(double v) {
    if (!(v >= 0.0 && v <= (double)CLS_MAX_CODE)) return -1;
    const int c = (int)v;
    return (double)c == v ? c : -1;
}

// CLASS INDEX, form 1: bisection in the ascending list -- the first index whose code is not below `code`, then one compare
CLS_HD inline int cls_index_bisect(const uint16_t *codes, int K, int code) {
    int lo = 0, hi = K;
    for (int s = 0; s < CLS_BISECT_STEPS; ++s) {
        if (lo >= hi) break;
        const int mid = (lo + hi) >> 1;
        if ((int)codes[mid] < code) lo = mid + 1;
        else hi = mid;
    }
    return lo < K && (int)codes[lo] == code ? lo : -1;
}

// CLASS INDEX, form 2: a direct table over min code .. max code (span = max - min + 1 <= CLS_TABLE_SPAN), -1 where not listed
CLS_HD inline bool cls_use_table(const uint16_t *codes, int K) { return (int)codes[K - 1] - (int)codes[0] < CLS_TABLE_SPAN; }
CLS_HD inline int cls_index_table(const int16_t *tab, int min_code, int span, int code) {
    const int d = code - min_code;
    return (unsigned)d < (unsigned)span ? (int)tab[d] : -1;
}
inline void cls_fill_table(const uint16_t *codes, int K, int16_t *tab) {
    const int span = (int)codes[K - 1] - (int)codes[0] + 1;
    for (int d = 0; d < span; ++d) tab[d] = -1;
    for (int k = 0; k < K; ++k) tab[(int)codes[k] - (int)codes[0]] = (int16_t)k;
}

// the slot of a value once its class index is known: -1 NA is decided before; k, or K for `other`
CLS_HD inline int cls_slot(int k, int K) { return k >= 0 ? k : K; }

// DERIVED VALUES: each a fixed handful of IEEE operations on the integers
CLS_HD inline double cls_nan() { return std::nan(""); }
CLS_HD inline double cls_frac(uint32_t count, uint32_t n) { return n ? (double)count / (double)n : cls_nan(); }
// the running mode over ascending k: a strict > keeps the SMALLER code on a tie (terra's modal takes the first occurrence)
CLS_HD inline bool cls_takes(uint32_t count, uint32_t best_count) { return count > best_count; }

struct ClsFin {
    uint32_t n;              // sum count + other
    int32_t mode;            // the code with the largest count, the smaller code on a tie; -1 where no listed class occurs
    int32_t variety;         // the number of k with count[k] > 0
    double mode_frac;        // count[mode] / n; NA where mode is -1
    double simpson;          // (n n - sum count^2 - other^2) / (n n); NA where n = 0
};
// the finishing function of every unit: count[0 .. K), each and their sum with `other` at most 2^31 - 1
CLS_HD inline ClsFin cls_finish(const uint32_t *count, int K, uint32_t other, const uint16_t *codes) {
    ClsFin f;
    uint64_t n = other, sq = (uint64_t)other * (uint64_t)other;
    uint32_t best = 0;
    int best_k = -1;
    f.variety = 0;
    for (int k = 0; k < K; ++k) {
        const uint32_t c = count[k];
        n += c;
        sq += (uint64_t)c * (uint64_t)c;
        if (c) ++f.variety;
        if (cls_takes(c, best)) { best = c; best_k = k; }
    }
    f.n = (uint32_t)n;
    f.mode = best_k < 0 ? -1 : (int32_t)codes[best_k];
    f.mode_frac = best_k < 0 ? cls_nan() : cls_frac(best, f.n);
    f.simpson = n ? (double)(n * n - sq) / ((double)n * (double)n) : cls_nan();
    return f;
}

}  // namespace mhs
