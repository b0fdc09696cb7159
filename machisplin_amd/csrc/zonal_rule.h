// The zonal rule (include/machisplin_hip.h, section "zonal"): the statistics of one layer inside each zone of an int32 zone
// plane, from EXACT INTEGER accumulators, so that no result depends on the order in which the cells were added.  Free of any
// HIP header: the kernels of zonal.hip and a plain C++ check program (tests/zonal_check.cpp) share it.
//
// A value v (converted exactly to double) is quantised to q = rint(v / quantum), round half to even, quantum a power of two,
// |q| <= 2^30.  Per zone: cells, n, S1 = sum q (int64: at most 2^31 * 2^30), S2 = sum q^2 held as TWO uint64 words --
// L = the sum of the low 32 bits of every q^2 (at most 2^31 * 2^32), H = the sum of the bits above them (q^2 <= 2^60, so at
// most 2^31 * 2^28) --, S2 = H * 2^32 + L as a 128-bit integer, and qmin, qmax.  Neither word can overflow, and the words are
// COMBINED, never carried: L may well pass 2^32.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MHS_ZONAL_HD __host__ __device__
#else
#define MHS_ZONAL_HD
#endif

namespace mhs {

// the statistics, as bits of `stats` (the numbering of the "focal" section, and cells)
enum {
    ZONAL_COUNT = 1 << 0, ZONAL_SUM = 1 << 1, ZONAL_MEAN = 1 << 2, ZONAL_SD = 1 << 3, ZONAL_MIN = 1 << 4, ZONAL_MAX = 1 << 5,
    ZONAL_RANGE = 1 << 6, ZONAL_MINUS_MEAN = 1 << 7, ZONAL_ABOVE_MIN = 1 << 8, ZONAL_BELOW_MAX = 1 << 9, ZONAL_DEV = 1 << 10,
    ZONAL_CELLS = 1 << 11, ZONAL_N_STATS = 12
};
constexpr unsigned ZONAL_TABLE_STATS = 0x87fu;       // bits 0 .. 6 and 11: what a table can hold; 7 .. 10 exist only as planes
constexpr unsigned ZONAL_ALL_STATS = 0xfffu;
// the integer accumulators, as bits of the kernels' mask
enum { ZONAL_A_CELLS = 1, ZONAL_A_N = 2, ZONAL_A_S1 = 4, ZONAL_A_S2 = 8, ZONAL_A_MIN = 16, ZONAL_A_MAX = 32 };

// The sizes at which zonal.hip changes path; tests/test_zonal_gpu.py reads them from this text.
constexpr int ZONAL_TILE_ROWS = 32;
constexpr int ZONAL_TILE_COLS = 64;
constexpr int ZONAL_STRIP_TILES = 8;        // tiles, one below the other, that a workgroup takes before it flushes its LDS table
constexpr int ZONAL_LDS_SLOTS = 256;        // slots of the workgroup's open-addressed table, a power of two
constexpr int ZONAL_PROBES = 4;             // slots a run tries before its totals go straight to the global table
constexpr int ZONAL_SCAN_BLOCK = 2048;      // zone slots per block of the blocked prefix sum over the present zones

constexpr int32_t ZONAL_Q_MAX = 1 << 30;    // |q| <= 2^30

// which accumulators the statistics of `stats` need; n goes with every statistic of the values (it tells an empty zone)
MHS_ZONAL_HD inline unsigned zonal_needs(unsigned stats) {
    unsigned a = 0;
    if (stats & ZONAL_CELLS) a |= ZONAL_A_CELLS;
    if (stats & (ZONAL_ALL_STATS & ~(unsigned)ZONAL_CELLS)) a |= ZONAL_A_N;
    if (stats & (ZONAL_SUM | ZONAL_MEAN | ZONAL_SD | ZONAL_MINUS_MEAN | ZONAL_DEV)) a |= ZONAL_A_S1;
    if (stats & (ZONAL_SD | ZONAL_DEV)) a |= ZONAL_A_S2;
    if (stats & (ZONAL_MIN | ZONAL_RANGE | ZONAL_ABOVE_MIN)) a |= ZONAL_A_MIN;
    if (stats & (ZONAL_MAX | ZONAL_RANGE | ZONAL_BELOW_MAX)) a |= ZONAL_A_MAX;
    return a;
}

// a power of two that q * quantum can be formed with exactly: finite, normal, positive, one bit of mantissa
MHS_ZONAL_HD inline bool zonal_quantum_ok(double quantum) {
    if (!(quantum >= 2.2250738585072014e-308) || !(quantum <= 8.98846567431158e307)) return false;      // 2^-1022 .. 2^1023
    int e;
    return std::frexp(quantum, &e) == 0.5;
}

// the default quantum: the smallest power of two (not below 2^-1022) with max_abs <= 2^30 * quantum; 1 for an all-zero layer
MHS_ZONAL_HD inline double zonal_default_quantum(double max_abs) {
    if (!(max_abs > 0.0)) return 1.0;
    int e;
    const double f = std::frexp(max_abs, &e);          // max_abs = f * 2^e, 0.5 <= f < 1
    int k = (f == 0.5 ? e - 1 : e) - 30;               // max_abs <= 2^(k + 30)
    if (k < -1022) k = -1022;
    return std::ldexp(1.0, k);
}

// the layer's value fits the quantum?  (then |q| <= 2^30)
MHS_ZONAL_HD inline bool zonal_fits(double v, double quantum) { return std::fabs(v) <= 1073741824.0 * quantum; }

// q of a finite value that fits
MHS_ZONAL_HD inline int32_t zonal_q(double v, double quantum) { return (int32_t)std::rint(v / quantum); }

// the two words that one q adds to S2
MHS_ZONAL_HD inline uint64_t zonal_sq(int32_t q) { return (uint64_t)((int64_t)q * (int64_t)q); }
MHS_ZONAL_HD inline uint64_t zonal_sq_lo(int32_t q) { return zonal_sq(q) & 0xffffffffull; }
MHS_ZONAL_HD inline uint64_t zonal_sq_hi(int32_t q) { return zonal_sq(q) >> 32; }

typedef unsigned __int128 zonal_u128;

// S2 from its words
MHS_ZONAL_HD inline zonal_u128 zonal_s2(uint64_t H, uint64_t L) { return ((zonal_u128)H << 32) + (zonal_u128)L; }

// n * S2 - S1 * S1: exact, non-negative (Cauchy-Schwarz) and at most 123 bits wide
MHS_ZONAL_HD inline zonal_u128 zonal_var_num(uint64_t n, int64_t S1, uint64_t H, uint64_t L) {
    const uint64_t a = S1 < 0 ? (uint64_t)0 - (uint64_t)S1 : (uint64_t)S1;
    return (zonal_u128)n * zonal_s2(H, L) - (zonal_u128)a * (zonal_u128)a;
}

// D(x) = (double)(uint64)(x >> 64) * 2^64 + (double)(uint64)x: two conversions, one exact product, one addition
MHS_ZONAL_HD inline double zonal_D(zonal_u128 x) {
    return (double)(uint64_t)(x >> 64) * 18446744073709551616.0 + (double)(uint64_t)x;
}

MHS_ZONAL_HD inline double zonal_nan() { return __builtin_nan(""); }

// one zone's accumulators, and its statistics in the table's order of operations
struct ZonalAcc {
    uint32_t cells, n;
    int64_t S1;
    uint64_t L, H;
    int32_t qmin, qmax;
};

MHS_ZONAL_HD inline double zonal_sum(const ZonalAcc &a, double quantum) { return a.n ? (double)a.S1 * quantum : zonal_nan(); }
MHS_ZONAL_HD inline double zonal_mean(const ZonalAcc &a, double quantum) {
    return a.n ? ((double)a.S1 / (double)a.n) * quantum : zonal_nan();
}
MHS_ZONAL_HD inline double zonal_sd(const ZonalAcc &a, double quantum) {
    if (a.n < 2) return zonal_nan();
    return std::sqrt(zonal_D(zonal_var_num(a.n, a.S1, a.H, a.L)) / ((double)a.n * (double)(a.n - 1))) * quantum;
}
MHS_ZONAL_HD inline double zonal_min(const ZonalAcc &a, double quantum) { return a.n ? (double)a.qmin * quantum : zonal_nan(); }
MHS_ZONAL_HD inline double zonal_max(const ZonalAcc &a, double quantum) { return a.n ? (double)a.qmax * quantum : zonal_nan(); }

// bits 7 .. 10 at a contributing cell of value q, from the zone's finalised mean, sd, min, max
MHS_ZONAL_HD inline double zonal_minus_mean(int32_t q, double quantum, double mean) { return (double)q * quantum - mean; }
MHS_ZONAL_HD inline double zonal_above_min(int32_t q, double quantum, double mn) { return (double)q * quantum - mn; }
MHS_ZONAL_HD inline double zonal_below_max(int32_t q, double quantum, double mx) { return mx - (double)q * quantum; }
MHS_ZONAL_HD inline double zonal_dev(double minus_mean, double sd) { return (sd != sd || sd == 0.0) ? zonal_nan() : minus_mean / sd; }

}  // namespace mhs
