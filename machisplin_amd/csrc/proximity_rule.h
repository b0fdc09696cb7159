// The proximity rules (include/machisplin_hip.h, section "proximity"): which cells are features, the nearest feature of a cell
// in exact integers -- d2 = the smallest (r - fr)^2 + (c - fc)^2, index = the smallest fr * ncol + fc that attains it -- and the
// products made from (fr, fc).  Free of any HIP header: the kernels of proximity.hip and a plain C++ check program
// (tests/proximity_check.cpp) share it.  The search is all int32 / int64; the products use only + - * /, sqrt and comparisons,
// each rounded once (the library is built with -ffp-contract=off), so a numpy restatement gives the same bits.
//
// The search has three phases:
//   A   rows     near(r, c) = the column of the nearest feature in row r, the LEFT one on a tie, -1 if the row has none
//   B1  columns  for every column the lower envelope over the rows r' that have a feature of  (r - r')^2 + h(r'),
//                h(r') = (c - near(r', c))^2: a stack of (row, the first row it wins from), built top to bottom (Meijster)
//   B2  cells    the envelope segment of the cell's row gives fr, near(fr, c) gives fc, and every product follows
// The envelope is read and written through an ACCESSOR `S`, so a rule never sees where the stack lives (global scratch with one
// lane per column, a host vector):
//   int S::row(k), int S::from(k)     entry k of the column's stack
//   int64_t S::h(k, row)              the squared in-row offset of entry k, whose row is `row`, in this column
//   void S::set(k, row, from, h)      a push: entry k, above which nothing is kept; h need not be stored (h(k, row) can make
//                                     it again from near()), but an accessor may keep it to spare the look-up
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MHS_PROX_HD __host__ __device__
#else
#define MHS_PROX_HD
#endif

namespace mhs {

// the predicates of mhs_proximity* (the MHS_PROX_* of the header, in its order)
enum { PROX_NA = 0, PROX_VALID, PROX_LT, PROX_LE, PROX_GT, PROX_GE, PROX_EQ, PROX_NE, PROX_WHERES };
// the products, as bits of the kernels' mask
enum { PROX_D2 = 1, PROX_INDEX = 2, PROX_DIST = 4, PROX_DIR_X = 8, PROX_DIR_Y = 16, PROX_VALUE = 32 };

// The sizes at which proximity.hip changes path; tests/test_proximity_gpu.py reads them from this text.
constexpr int PROX_CHUNK = 64;       // phase A: columns a wave scans at once; the carry crosses from chunk to chunk
constexpr int PROX_PRELOAD = 8;      // phase B1: rows of near() a lane loads ahead of the envelope build
constexpr int PROX_BAND = 32;        // phase B2: rows a lane walks down from one binary search
constexpr int PROX_TOP = 16;         // phase B1: entries at the top of a lane's stack that are also kept in LDS

constexpr int PROX_NONE = 0x7fffffff;                  // "no feature to the right" in the suffix scan of phase A

// a plane value converted exactly to double is NA when it is NaN or equals the stack's nodata
MHS_PROX_HD inline bool prox_na(double v, bool has_nodata, double nodata) { return v != v || (has_nodata && v == nodata); }

// the cell is a feature?  An NA cell never satisfies a comparison.
MHS_PROX_HD inline bool prox_is_feature(double v, bool has_nodata, double nodata, int where, double threshold) {
    const bool na = prox_na(v, has_nodata, nodata);
    switch (where) {
    case PROX_NA: return na;
    case PROX_VALID: return !na;
    case PROX_LT: return !na && v < threshold;
    case PROX_LE: return !na && v <= threshold;
    case PROX_GT: return !na && v > threshold;
    case PROX_GE: return !na && v >= threshold;
    case PROX_EQ: return !na && v == threshold;
    case PROX_NE: return !na && v != threshold;
    default: return false;
    }
}

// A: the nearer of the nearest feature column at or left of c (`left`, -1: none) and at or right of it (`right`, -1: none);
// the left one on a tie
MHS_PROX_HD inline int prox_nearer_in_row(int c, int left, int right) {
    if (left < 0) return right;
    if (right < 0) return left;
    return c - left <= right - c ? left : right;
}

// floor(a / b) for b > 0: C's division truncates towards zero, which is one too many for a negative a that b does not divide
MHS_PROX_HD inline int64_t prox_floor_div(int64_t a, int64_t b) {
    const int64_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// B1: the first row at which the later row u (squared in-row offset hu) is STRICTLY nearer than the earlier row i < u (hi):
// (r - u)^2 + hu < (r - i)^2 + hi  <=>  r > (u^2 - i^2 + hu - hi) / (2 (u - i)).  Below it the earlier row keeps the cell, ties
// included -- which is what gives the smaller row on a tie.  May be negative or past the grid.
struct ProxSep { int64_t n, d; };          // the separator's numerator and its denominator > 0
MHS_PROX_HD inline ProxSep prox_sep(int64_t i, int64_t hi, int64_t u, int64_t hu) { return ProxSep{u * u - i * i + hu - hi, 2 * (u - i)}; }
MHS_PROX_HD inline int64_t prox_takeover(int64_t i, int64_t hi, int64_t u, int64_t hu) {
    const ProxSep p = prox_sep(i, hi, u, hu);
    return prox_floor_div(p.n, p.d) + 1;
}

// the envelope of one column while it is built: its height and a copy of its top entry
struct ProxEnv {
    int k = 0;
    int top_row = 0, top_from = 0;
    int64_t top_h = 0;
};

// B1: row u, which has a feature at squared in-row offset hu, enters the column's envelope; u is greater than every row
// entered before.  Entries that u beats from their own first row on are popped; u is pushed unless it wins nowhere in the grid.
// The pop loop runs at most k <= nrow times (it is bounded by nrow besides), and k grows by at most one per call, so entry k of
// a set() is below the number of calls: a stack of nrow entries per column suffices.
// The takeover row w = floor(n / d) + 1 is compared WITHOUT dividing: for an integer f,  w > f  <=>  floor(n / d) >= f  <=>
// n >= f d  (d > 0), all in int64 (|n| < 2^33, f d < 2^33).  Only a row that is pushed pays the one true floor division.
template <typename S>
MHS_PROX_HD inline void prox_env_add(S &s, ProxEnv &e, int u, int64_t hu, int nrow) {
    for (int it = 0; it <= nrow && e.k > 0; ++it) {
        const ProxSep p = prox_sep(e.top_row, e.top_h, u, hu);
        if (p.n >= (int64_t)e.top_from * p.d) break;                  // w > top_from: the top keeps its first rows
        --e.k;
        if (e.k > 0) {
            e.top_row = s.row(e.k - 1);
            e.top_from = s.from(e.k - 1);
            e.top_h = s.h(e.k - 1, e.top_row);
        }
    }
    int64_t w = 0;
    if (e.k > 0) {
        const ProxSep p = prox_sep(e.top_row, e.top_h, u, hu);
        if (p.n >= (int64_t)(nrow - 1) * p.d) return;                 // w >= nrow: u wins nowhere in the grid
        w = prox_floor_div(p.n, p.d) + 1;
    }
    s.set(e.k, u, (int)w, hu);
    e.top_row = u; e.top_from = (int)w; e.top_h = hu;
    ++e.k;
}

// B2: the entry of a stack of cnt > 0 entries whose segment holds row r: the greatest k with from(k) <= r (from(0) is 0 and the
// entries' from rise strictly).  A binary search of at most 32 steps.
template <typename S>
MHS_PROX_HD inline int prox_segment(const S &s, int cnt, int r) {
    int lo = 0, hi = cnt - 1;
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (s.from(mid) <= r) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the exact part of a cell's answer
MHS_PROX_HD inline int64_t prox_d2(int r, int c, int fr, int fc) {
    const int64_t dr = (int64_t)r - fr, dc = (int64_t)c - fc;
    return dr * dr + dc * dc;
}
MHS_PROX_HD inline int64_t prox_index(int fr, int fc, int ncol) { return (int64_t)fr * ncol + fc; }

// the float products of cell (r, c) whose nearest feature is (fr, fc); fr < 0: there is no feature anywhere
struct ProxFloat { double dist, dir_x, dir_y; };
MHS_PROX_HD inline ProxFloat prox_float(int r, int c, int fr, int fc, double unit) {
    if (fr < 0) return ProxFloat{(double)NAN, (double)NAN, (double)NAN};
    const int64_t d2 = prox_d2(r, c, fr, fc);
    if (d2 == 0) return ProxFloat{0.0 * unit, 0.0, 0.0};
    const double s = sqrt((double)d2);
    return ProxFloat{s * unit, (double)(fc - c) / s, (double)(r - fr) / s};
}

}  // namespace mhs
