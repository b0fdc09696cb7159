// The focal rules (include/machisplin_hip.h, section "focal"): window statistics of one plane at any radius from blocked prefix
// sums.  Free of any HIP header: the kernels of focal.hip and a plain C++ check program (tests/focal_check.cpp) share it.  The
// header states the rules; the operations stand here in that order, each rounded once (the library is built with
// -ffp-contract=off), and only + - * / sqrt are used, so a numpy restatement (tests/focal_ref.py) gives the same bits.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MHS_FOCAL_HD __host__ __device__
#else
#define MHS_FOCAL_HD
#endif

namespace mhs {

// bit k of the `stats` mask of mhs_focal*; the output planes follow in this order
enum { FS_COUNT = 0, FS_SUM, FS_MEAN, FS_SD, FS_MIN, FS_MAX, FS_RANGE, FS_MINUS_MEAN, FS_ABOVE_MIN, FS_BELOW_MAX, FS_DEV, FS_NSTATS };
constexpr unsigned FS_SUM_FAMILY = 1u << FS_COUNT | 1u << FS_SUM | 1u << FS_MEAN | 1u << FS_SD | 1u << FS_MINUS_MEAN | 1u << FS_DEV;
constexpr unsigned FS_MINMAX_FAMILY = 1u << FS_MIN | 1u << FS_MAX | 1u << FS_RANGE | 1u << FS_ABOVE_MIN | 1u << FS_BELOW_MAX;
constexpr unsigned FS_NEEDS_CENTRE = 1u << FS_MINUS_MEAN | 1u << FS_ABOVE_MIN | 1u << FS_BELOW_MAX | 1u << FS_DEV;
enum { FOCAL_SQUARE = 0, FOCAL_CIRCLE = 1 };          // MHS_FOCAL_SQUARE, MHS_FOCAL_CIRCLE
constexpr int FOCAL_B = 64;                           // MHS_FOCAL_BLOCK

// a plane value converted exactly to double is NA when it is NaN or equals the stack's nodata ("terrain"'s rule)
MHS_FOCAL_HD inline bool focal_na(double v, bool has_nodata, double nodata) { return v != v || (has_nodata && v == nodata); }

// half width of the circular window of radius R in the row |dr| <= R away: the largest dc with dr^2 + dc^2 <= R^2
MHS_FOCAL_HD inline int focal_half_width(int R, int dr) {
    const int64_t rem = (int64_t)R * R - (int64_t)dr * dr;
    int64_t d = (int64_t)sqrt((double)rem);
    while (d * d > rem) --d;
    while ((d + 1) * (d + 1) <= rem) ++d;
    return (int)d;
}

// THE BLOCKED PREFIX of x[0 .. n): P[i] = offset of i's aligned block of FOCAL_B elements + the sequential sum from the block's
// first element to i; the offsets are the sequential running sum of the block totals, from 0.0.  (The kernels make the same
// values block-parallel; this is the rule as one loop, for the check program.)
template <typename S>
MHS_FOCAL_HD inline void focal_blocked_prefix(const S *x, int64_t n, int64_t stride, S *P) {
    S run = (S)0;
    for (int64_t b0 = 0; b0 < n; b0 += FOCAL_B) {
        S s = (S)0;
        for (int64_t i = b0; i < n && i < b0 + FOCAL_B; ++i) {
            s = i == b0 ? x[i * stride] : s + x[i * stride];
            P[i * stride] = run + s;
        }
        run = run + s;
    }
}

// the sum of x[lo .. hi] from its blocked prefix, lo and hi already cut to the array: P[hi] - P[lo - 1], P[-1] = 0
template <typename S>
MHS_FOCAL_HD inline S focal_window_sum(const S *P, int64_t stride, int64_t lo, int64_t hi) {
    return P[hi * stride] - (lo > 0 ? P[(lo - 1) * stride] : (S)0);
}

// THE STATISTICS of one window: n valid cells, S1 = sum of (z - offset), S2 = sum of (z - offset)^2 over them, mn and mx their
// smallest and largest value (exact whatever the order they are found in; looked at only where `mask` has one of the min / max
// family); e is the centre (has_e: it is not NA).  NA = NaN.
MHS_FOCAL_HD inline void focal_stats(unsigned mask, int64_t n, double S1, double S2, double offset, bool has_e, double e, double mn, double mx,
                                     double out[FS_NSTATS]) {
    const double nan = (double)NAN, dn = (double)n;
    out[FS_COUNT] = dn;
    out[FS_SUM] = n > 0 ? S1 + dn * offset : nan;
    const double mean = n > 0 ? offset + S1 / dn : nan;
    out[FS_MEAN] = mean;
    double sd = nan;
    if ((mask & (1u << FS_SD | 1u << FS_DEV)) && n >= 2) {
        const double v = (S2 - S1 * S1 / dn) / (double)(n - 1);
        sd = sqrt(v > 0.0 ? v : 0.0);
    }
    out[FS_SD] = sd;
    const bool mm = (mask & FS_MINMAX_FAMILY) && n > 0;
    out[FS_MIN] = mm ? mn : nan;
    out[FS_MAX] = mm ? mx : nan;
    out[FS_RANGE] = mm ? mx - mn : nan;
    const double d = has_e && n > 0 ? e - mean : nan;
    out[FS_MINUS_MEAN] = d;
    out[FS_ABOVE_MIN] = mm && has_e ? e - mn : nan;
    out[FS_BELOW_MAX] = mm && has_e ? mx - e : nan;
    out[FS_DEV] = sd > 0.0 ? d / sd : nan;                      // an NA sd compares false
}

// THE RUNNING MINIMUM of a square window, one axis after the other, from aligned blocks of FOCAL_B elements: pm[i] = the minimum
// from the block's first element to i, sm[i] = from i to the block's last, and a table T[j][k] = the minimum of the blocks
// k .. k + 2^j - 1 (each level the minimum of two entries of the level below).  The minimum of x[lo .. hi], lo and hi cut to the
// array of n elements, reads at most two entries of each -- or, where lo .. hi lies strictly inside one block, its fewer than
// FOCAL_B elements themselves.  A minimum is exact in any order, so this is a way to find it, not a rule about its value.
// The accessor A: pm(i), sm(i), raw(i), table(j, k).  The maximum is minus the minimum of -x.
template <class A>
MHS_FOCAL_HD inline double focal_range_min(const A &acc, int64_t n, int64_t lo, int64_t hi) {
    const int64_t kl = lo / FOCAL_B, kh = hi / FOCAL_B;
    if (kl == kh) {
        if (lo % FOCAL_B == 0) return acc.pm(hi);
        if (hi % FOCAL_B == FOCAL_B - 1 || hi == n - 1) return acc.sm(lo);
        double m = acc.raw(lo);
        for (int64_t i = lo + 1; i <= hi; ++i) { const double v = acc.raw(i); m = v < m ? v : m; }
        return m;
    }
    double m = acc.sm(lo);
    const double p = acc.pm(hi);
    m = p < m ? p : m;
    if (kh - kl >= 2) {
        const int64_t a = kl + 1, len = kh - kl - 1;
        int j = 0;
        while (((int64_t)2 << j) <= len) ++j;                    // the largest j with 2^j <= len
        const double t0 = acc.table(j, a), t1 = acc.table(j, a + len - ((int64_t)1 << j));
        m = t0 < m ? t0 : m;
        m = t1 < m ? t1 : m;
    }
    return m;
}

// levels of the table over nb blocks: j = 0 .. floor(log2(nb))
MHS_FOCAL_HD inline int focal_levels(int64_t nb) {
    int l = 1;
    while (((int64_t)1 << l) <= nb) ++l;
    return l;
}

}  // namespace mhs
