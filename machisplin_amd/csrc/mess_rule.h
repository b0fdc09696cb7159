// The MESS rule (multivariate environmental similarity surface, Elith, Kearney & Phillips 2010; dismo::mess), free of any HIP
// header: the grid kernel, the points call (mess.hip) and a plain C++ check program (tests/test_mess_host.py) share it.
// include/machisplin_hip.h states the rule; the operations stand here in that order, each rounded once (the library is built
// with -ffp-contract=off), so a numpy restatement gives the same bits.
#pragma once

#if defined(__HIPCC__)
#define MHS_MESS_HD __host__ __device__
#else
#define MHS_MESS_HD
#endif

namespace mhs {

constexpr int MESS_SEG = 64;   // the device's coarse table holds every 64th sorted value: a segment is 512 bytes

// THE per-value rule: the similarity of a cell value p to one variable of the reference table, given
// i = #{j : r_j <= p} among its n sorted values r_1 <= ... <= r_n, mn = r_1, mx = r_n > mn.
MHS_MESS_HD inline double mess_value(double p, int i, int n, double mn, double mx) {
    const bool below = i == 0, above = i == n;                  // below every station / at or above the largest
    // ONE division serves the three cases, chosen by selects (no divergent branch on the device); every operation of the rule
    // is still done once, in the rule's order
    const double num = below ? 100.0 * (p - mn) : above ? 100.0 * (mx - p) : 100.0 * (double)i;
    const double den = (below || above) ? mx - mn : (double)n;
    const double f = num / den;                                 // outside the range this is s itself: negative, or <= 0
    if (below || above) return f;                               // (dismo's quirk: p == mx has i == n and gets 0)
    return f <= 50.0 ? 2.0 * f : 200.0 - 2.0 * f;
}

// One step of the count's binary search over r[0 .. m), m >= 1: lo = the count found so far, st the step.  The value is
// loaded whether or not the step can be taken (from a clamped, always valid index): no branch, so the loads of several
// searches run side by side.
MHS_MESS_HD inline int mess_step(const double *r, int m, double p, int lo, int st) {
    const int mid = lo + st, j = mid < m ? mid : m;
    const bool take = (mid <= m) & (r[j - 1] <= p);
    return take ? mid : lo;
}
// the first step for m values: the largest power of two <= m (1 for m <= 1)
MHS_MESS_HD inline int mess_top(int m) {
    int top = 1;
    while (2 * top <= m) top <<= 1;
    return top;
}
// #{j in [0, m) : r[j] <= p} for ascending r, m >= 1 (R's findInterval, numpy's searchsorted(side = "right")); 0 for a NaN p
MHS_MESS_HD inline int mess_count(const double *r, int m, double p) {
    int lo = 0;
    for (int st = mess_top(m); st > 0; st >>= 1) lo = mess_step(r, m, p, lo, st);
    return lo;
}
// The same count in two levels, as the kernel takes them: `coarse` holds r[0], r[64], r[128], ... (nc = ceil(n / 64) values);
// g = #{coarse <= p} selects the segment r[64 (g - 1) .. ), whose first value is known to be <= p: six steps from a count of 1.
MHS_MESS_HD inline int mess_count2(const double *r, int n, const double *coarse, int nc, double p) {
    const int g = mess_count(coarse, nc, p);
    if (g == 0) return 0;
    const int base = (g - 1) * MESS_SEG;
    const int m = n - base < MESS_SEG ? n - base : MESS_SEG;            // values in the segment
    int cnt = 1;                                                        // its first one is <= p
    for (int st = MESS_SEG / 2; st > 0; st >>= 1) cnt = mess_step(r + base, m, p, cnt, st);
    return base + cnt;
}

}  // namespace mhs
