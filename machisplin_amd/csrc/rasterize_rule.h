// The rasterize rule (include/machisplin_hip.h, section "rasterize"): which cells of a grid a point, a line or a polygon covers.
// Free of any HIP header: the kernels and the host planner of rasterize.hip and a plain C++ check program
// (tests/rasterize_check.cpp) share it.  The library is built with -ffp-contract=off, so every line is a fixed sequence of
// float64 operations, each rounded once; no transcendental is used.
//
// Two COUNTS carry the centre rule, and both are exact whatever the rounding of the guess they start from:
//   rz_cstar(g, X)  = #{c in 0 .. ncol - 1 : x_c(c) < X}       the cells of a row that a crossing at X toggles are c < c*
//   rz_rabove(g, y) = #{r in 0 .. nrow - 1 : y_r(r) >= y}       an edge (ya < yb) crosses the rows rz_rabove(yb) .. rz_rabove(ya) - 1
// x_c is non-decreasing in c and y_r non-increasing in r (a sum and a product of non-negative terms, each rounded monotonically),
// so each predicate is monotone; the guess from floor() is confirmed by two comparisons against the rule's own x_c / y_r and, where
// they do not confirm it (huge or tiny cells, coordinates far away), a bisection of at most 31 steps finds the count.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MHS_RZ_HD __host__ __device__
#else
#define MHS_RZ_HD
#endif

namespace mhs {

enum { RZ_POINT = 0, RZ_LINE = 1, RZ_POLYGON = 2 };
enum { RZ_LAST = 0, RZ_FIRST = 1, RZ_MAX = 2, RZ_MIN = 3 };
// the layers of a feature's bit plane, as bits of its flags
enum { RZ_TOGGLE = 1, RZ_BURN = 2 };

// The sizes at which rasterize.hip changes path; tests/test_rasterize_gpu.py reads them from this text.
constexpr int RZ_SCAN_BLOCK = 2048;         // vertices per block of the blocked prefix sum over the edges' items
constexpr int RZ_CHUNK_WORDS = 64;          // 32-bit words of a bit-plane row that a wave scans at a time: 2 048 columns
constexpr int64_t RZ_DEFAULT_BUDGET = 256ll << 20;      // bytes of bit planes per batch

struct RzGrid {
    double xmin, ymax, xres, yres;
    int nrow, ncol;
};

MHS_RZ_HD inline double rz_xc(const RzGrid &g, int c) { return g.xmin + ((double)c + 0.5) * g.xres; }
MHS_RZ_HD inline double rz_yr(const RzGrid &g, int r) { return g.ymax - ((double)r + 0.5) * g.yres; }
MHS_RZ_HD inline double rz_yedge(const RzGrid &g, int r) { return g.ymax - (double)r * g.yres; }

// a double as an int inside lo .. hi (the double is never NaN: the coordinates are finite and the cell sizes positive)
MHS_RZ_HD inline int rz_clampi(double v, int lo, int hi) { return v < (double)lo ? lo : v > (double)hi ? hi : (int)v; }

// col(x), row(y) of the line and point rules, clipped to -1 .. ncol (nrow): -1 and ncol (nrow) stand for "outside"
MHS_RZ_HD inline int rz_col(const RzGrid &g, double x) { return rz_clampi(std::floor((x - g.xmin) / g.xres), -1, g.ncol); }
MHS_RZ_HD inline int rz_row(const RzGrid &g, double y) { return rz_clampi(std::floor((g.ymax - y) / g.yres), -1, g.nrow); }

MHS_RZ_HD inline int rz_cstar(const RzGrid &g, double X) {
    const int k = rz_clampi(std::floor((X - g.xmin) / g.xres + 0.5), 0, g.ncol);
    int lo = 0, hi = g.ncol;                                  // the count lies in lo .. hi
    if (k > 0) { if (rz_xc(g, k - 1) < X) lo = k; else hi = k - 1; }
    if (lo == k) { if (k < g.ncol && rz_xc(g, k) < X) lo = k + 1; else hi = k; }
    while (lo < hi) {                                         // only where the guess was not confirmed
        const int mid = lo + (hi - lo) / 2;
        if (rz_xc(g, mid) < X) lo = mid + 1; else hi = mid;
    }
    return lo;
}

MHS_RZ_HD inline int rz_rabove(const RzGrid &g, double y) {
    const int k = rz_clampi(std::floor((g.ymax - y) / g.yres + 0.5), 0, g.nrow);
    int lo = 0, hi = g.nrow;
    if (k > 0) { if (rz_yr(g, k - 1) >= y) lo = k; else hi = k - 1; }
    if (lo == k) { if (k < g.nrow && rz_yr(g, k) >= y) lo = k + 1; else hi = k; }
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (rz_yr(g, mid) >= y) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// A segment in canonical orientation: (xa, ya) is the endpoint with the smaller y.  Two rings that share an edge in opposite
// directions therefore compute identical bits on it.
struct RzSeg {
    double xa, ya, xb, yb, t;
};
MHS_RZ_HD inline RzSeg rz_seg(double x0, double y0, double x1, double y1) {
    RzSeg s;
    if (y1 < y0) { s.xa = x1; s.ya = y1; s.xb = x0; s.yb = y0; }
    else { s.xa = x0; s.ya = y0; s.xb = x1; s.yb = y1; }
    s.t = s.yb > s.ya ? (s.xb - s.xa) / (s.yb - s.ya) : 0.0;
    return s;
}
// X(y) for ya <= y <= yb on a segment that is not horizontal.  X(ya) = xa and X(yb) = xb exactly, and X never leaves the
// segment's own x range, so a feature's cover lies inside the bounding box of its vertices whatever the rounding of t.
MHS_RZ_HD inline double rz_X(const RzSeg &s, double y) {
    if (y >= s.yb) return s.xb;
    const double v = s.xa + (y - s.ya) * s.t;
    const double lo = s.xa < s.xb ? s.xa : s.xb, hi = s.xa < s.xb ? s.xb : s.xa;
    return v < lo ? lo : v > hi ? hi : v;
}

// POLYGONS: the rows an edge crosses are first .. first + n - 1; a horizontal edge crosses none.
MHS_RZ_HD inline int rz_cross_rows(const RzGrid &g, const RzSeg &s, int *first) {
    if (!(s.yb > s.ya)) { *first = 0; return 0; }
    *first = rz_rabove(g, s.yb);
    return rz_rabove(g, s.ya) - *first;
}

// LINES: the rows whose items a segment has, clipped to the grid: first .. first + n - 1
MHS_RZ_HD inline int rz_line_rows(const RzGrid &g, const RzSeg &s, int *first) {
    const int top = rz_row(g, s.yb), bottom = rz_row(g, s.ya);
    const int a = top < 0 ? 0 : top, b = bottom > g.nrow - 1 ? g.nrow - 1 : bottom;
    *first = a;
    return b >= a ? b - a + 1 : 0;
}
// ... and the columns c_lo .. c_hi it burns in row r of them, clipped to the grid; false: none
MHS_RZ_HD inline bool rz_line_span(const RzGrid &g, const RzSeg &s, int r, int *c_lo, int *c_hi) {
    double x0, x1;
    if (!(s.yb > s.ya)) { x0 = s.xa; x1 = s.xb; }
    else {
        const double e1 = rz_yedge(g, r + 1), e0 = rz_yedge(g, r);
        const double ylo = s.ya > e1 ? s.ya : e1, yhi = s.yb < e0 ? s.yb : e0;
        if (ylo > yhi) return false;
        x0 = rz_X(s, ylo);
        x1 = rz_X(s, yhi);
    }
    if (x1 < x0) { const double x = x0; x0 = x1; x1 = x; }
    const int a = rz_col(g, x0), b = rz_col(g, x1);
    *c_lo = a < 0 ? 0 : a;
    *c_hi = b > g.ncol - 1 ? g.ncol - 1 : b;
    return *c_lo <= *c_hi;
}

// POINTS: terra's colFromX / rowFromY -- the east edge belongs to the last column, the south edge to the last row; false: outside
MHS_RZ_HD inline bool rz_point_cell(const RzGrid &g, double x, double y, int *r, int *c) {
    const double xmax = g.xmin + (double)g.ncol * g.xres, ymin = g.ymax - (double)g.nrow * g.yres;
    if (x < g.xmin || x > xmax || y < ymin || y > g.ymax) return false;
    *c = x == xmax ? g.ncol - 1 : rz_col(g, x);
    *r = y == ymin ? g.nrow - 1 : rz_row(g, y);
    return *c >= 0 && *c < g.ncol && *r >= 0 && *r < g.nrow;
}

// The box of a feature whose vertices span x0 .. x1, y0 .. y1: every cell that the centre rule or the line rule can give it,
// clipped to the grid.  Empty (false) for a feature that lies outside.
struct RzBox {
    int r0, c0, h, w;
};
MHS_RZ_HD inline bool rz_box(const RzGrid &g, double x0, double x1, double y0, double y1, RzBox *b) {
    int ca = rz_cstar(g, x0), cb = rz_cstar(g, x1) - 1, ra = rz_rabove(g, y1), rb = rz_rabove(g, y0) - 1;
    const int la = rz_col(g, x0), lb = rz_col(g, x1), ta = rz_row(g, y1), tb = rz_row(g, y0);
    if (la < ca) ca = la;
    if (lb > cb) cb = lb;
    if (ta < ra) ra = ta;
    if (tb > rb) rb = tb;
    if (ca < 0) ca = 0;
    if (ra < 0) ra = 0;
    if (cb > g.ncol - 1) cb = g.ncol - 1;
    if (rb > g.nrow - 1) rb = g.nrow - 1;
    b->r0 = ra; b->c0 = ca; b->h = rb - ra + 1; b->w = cb - ca + 1;
    if (b->h <= 0 || b->w <= 0) { b->h = 0; b->w = 0; return false; }
    return true;
}
// 32-bit words of one row of a box's bit plane: one bit per column and the sentinel
MHS_RZ_HD inline int64_t rz_row_words(int w) { return ((int64_t)w + 1 + 31) / 32; }

}  // namespace mhs
