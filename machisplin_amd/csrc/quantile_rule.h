// The quantile rule (include/machisplin_hip.h, section "zonal quantiles"): R's type 7 quantile (numpy's "linear") of the
// quantised values q of a zone's contributing cells, in a fixed sequence of operations, each rounded once.  Free of any HIP
// header: the kernels of quantile.hip and a plain C++ check program (tests/quantile_check.cpp) share it.  The input layer, NA and
// +-Inf, zone membership and the quantisation q = rint(v / quantum) are zonal_rule.h's, through its functions.
//
// The library is built with -ffp-contract=off, as every rule header relies on; the pragma below says the same where the
// compiler knows it, so g * d and the sum that follows are never fused.
#pragma once

#include <cmath>
#include <cstdint>
#include "zonal_rule.h"

namespace mhs {

constexpr int QUANTILE_MAX_PROBS = 16;

// The sort key of a contributing cell: the zone above the biased quantum, so that keys order by zone, then by q.
// q + 2^30 lies in 0 .. 2^31.  A cell that does not contribute gets the key of zone `n_zones` with the low word 0: it sorts
// behind every contributing cell, and the window of the sort is 32 + quantile_bits(n_zones) bits wide.
MHS_ZONAL_HD inline uint64_t quantile_key(uint32_t zone, int32_t q) { return ((uint64_t)zone << 32) | (uint64_t)((uint32_t)q + (uint32_t)ZONAL_Q_MAX); }
MHS_ZONAL_HD inline uint64_t quantile_sentinel(uint32_t n_zones) { return (uint64_t)n_zones << 32; }
MHS_ZONAL_HD inline int32_t quantile_key_q(uint64_t key) { return (int32_t)((uint32_t)(key & 0xffffffffull) - (uint32_t)ZONAL_Q_MAX); }
MHS_ZONAL_HD inline uint32_t quantile_key_zone(uint64_t key) { return (uint32_t)(key >> 32); }
// the number of bits that hold x: 0 for 0, 1 for 1, 2 for 2 and 3, ...
MHS_ZONAL_HD inline int quantile_bits(uint32_t x) {
    int b = 0;
    while (x) { ++b; x >>= 1; }
    return b;
}

// a probability that the rule takes: in [0, 1], not NaN
MHS_ZONAL_HD inline bool quantile_prob_ok(double p) { return p >= 0.0 && p <= 1.0; }

// Type 7 of the ascending s[0 .. n), n >= 1, s[i] = the q of sorted place i (a functor):
//   h = (double)(n - 1) * p;  lo = (int64)floor(h);  g = h - (double)lo;  hi = min(lo + 1, n - 1)
//   Q = ((double)s[lo] + g * (double)((int64)s[hi] - (int64)s[lo])) * quantum
// (double)(n - 1), (double)s[lo] and the difference d (below 2^32) are exact; h, g * d, the sum and the scaling round once each
// (the scaling by a power of two is exact unless the result is subnormal).
// BOUNDS.  0 <= g < 1 and d >= 0, so 0 <= fl(g * d) <= d, and s[lo] + fl(g d) lies in [s[lo], s[hi]]: min <= Q <= max always,
// and p = 0, p = 1 give s[0] * quantum and s[n - 1] * quantum, zonal's min and max.  With n even and p = 0.5, h = (n - 1) / 2 is
// exact, g = 0.5 and g * d is exact (d an integer below 2^32), so the median is (s[lo] + d / 2) * quantum rounded once -- the
// exact mean of the two middle values, as numpy.median forms it when q * quantum = v.
// Against the exact type 7 value X = s[LO] + G (s[LO + 1] - s[LO]) with H = (n - 1) p exact, LO = floor(H), G = H - LO: let
// D = s[n - 1] - s[0] (every neighbour difference is at most D) and M = max(|s[0]|, |s[n - 1]|).  h = H (1 + e0), |e0| <= u =
// 2^-53, and g = h - lo is exact, so with lo = LO, |g - G| <= u H < u n and g d is off by at most u n D; where rounding carries
// h over an integer that H stays below, Q = s[lo] while X = s[lo] - (lo - H) d', again within u n D.  g d rounds with at most
// u D, the sum with at most u M.  Hence |Q - X quantum| <= u (n D + D + M) quantum: quantile_bound below.
// numpy.quantile(method = "linear") forms h and g the same way and carries roundings of the same size on the values
// themselves (b - (b - a)(1 - g) where g >= 0.5), so it lies within the same bound of X, and the tests allow twice the bound
// between the two.
template <class S>
MHS_ZONAL_HD inline double quantile_type7(const S &s, int64_t n, double p, double quantum) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double h = (double)(n - 1) * p;
    const int64_t lo = (int64_t)std::floor(h);
    const double g = h - (double)lo;
    const int64_t hi = lo + 1 < n - 1 ? lo + 1 : n - 1;
    const int32_t a = s(lo), b = s(hi);
    const double gd = g * (double)((int64_t)b - (int64_t)a);
    return ((double)a + gd) * quantum;
}

// the bound on |Q - exact| derived above, for a zone of n values between qlo and qhi (as quanta)
MHS_ZONAL_HD inline double quantile_bound(int64_t n, int32_t qlo, int32_t qhi, double quantum) {
    const double u = 1.1102230246251565e-16;
    const double d = (double)((int64_t)qhi - (int64_t)qlo);
    const double m = std::fabs((double)qlo) > std::fabs((double)qhi) ? std::fabs((double)qlo) : std::fabs((double)qhi);
    return u * ((double)n * d + d + m) * quantum;
}

// frac_below of a contributing cell with `below` smaller values among its zone's n
MHS_ZONAL_HD inline double quantile_frac_below(int32_t below, int64_t n) { return (double)below / (double)n; }

// the first place in the ascending keys[lo .. hi) whose key is not below `key` (hi if none)
template <class K>
MHS_ZONAL_HD inline int64_t quantile_lower_bound(const K &keys, int64_t lo, int64_t hi, uint64_t key) {
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (keys(mid) < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

}  // namespace mhs
