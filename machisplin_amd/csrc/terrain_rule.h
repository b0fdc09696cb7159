// The terrain rules (include/machisplin_hip.h, section "terrain"): 3 x 3 terrain variables (Horn 1981), relief in a circular
// window, geomorphons (Jasiewicz & Stepinski 2013).  Free of any HIP header: the three kernels of terrain.hip and a plain C++
// check program (tests/terrain_check.cpp) share it.  The header states the rules; the operations stand here in that order,
// each rounded once (the library is built with -ffp-contract=off), so a numpy restatement gives the same bits -- except
// through atan and atan2, which no two math libraries need round alike.
//
// A rule reads the neighbourhood of its cell through an ACCESSOR `A`:
//   int  A::up, down, left, right     cells of the raster north / south / west / east of the centre (0 on the border)
//   bool A::get(dr, dc, double &z)    the cell dr rows south and dc columns east of the centre, which the caller keeps inside
//                                     the raster; false where that cell is NA
// so a rule never sees how the plane is stored (an LDS tile in the plane's own type, or a host array).  w[0 .. R] are the
// half widths of the relief window's rows (relief_half_width).
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MHS_TERRAIN_HD __host__ __device__
#else
#define MHS_TERRAIN_HD
#endif

namespace mhs {

// bit k of the `vars` mask of mhs_terrain* selects variable k; the output planes follow in this order
enum { TV_DZDX = 0, TV_DZDY, TV_SLOPE_TAN, TV_SLOPE_DEG, TV_EASTNESS, TV_NORTHNESS, TV_ASPECT_DEG, TV_TPI, TV_TRI, TV_ROUGHNESS, TV_COUNT };
// bit k of the `stats` mask of mhs_relief*
enum { RS_ABOVE_MIN = 0, RS_BELOW_MAX, RS_MINUS_MEAN, RS_COUNT };

constexpr double TERRAIN_DEG = 180.0 / 3.14159265358979323846;       // 180 / pi, the double numpy's 180 / np.pi is
constexpr double TERRAIN_RAD = 3.14159265358979323846 / 180.0;       // pi / 180
constexpr int16_t GEOMORPHON_NA = -32768;

// a plane value converted exactly to double is NA when it is NaN or equals the stack's nodata
MHS_TERRAIN_HD inline bool terrain_na(double v, bool has_nodata, double nodata) { return v != v || (has_nodata && v == nodata); }

// 1. THE 3 x 3 rule.  z = a b c / d e f / g h i, north row first, none NA.  Only the variables of `mask` are made (the
// others' entries of out are left alone); dx is the width of the centre's row.
MHS_TERRAIN_HD inline void terrain_3x3(const double z[9], double dx, double dy, double zf, unsigned mask, double out[TV_COUNT]) {
    const double a = z[0], b = z[1], c = z[2], d = z[3], e = z[4], f = z[5], g = z[6], h = z[7], i = z[8];
    const double dzdx = (((c + 2.0 * f) + i) - ((a + 2.0 * d) + g)) * zf / (8.0 * dx);
    const double dzdy = (((g + 2.0 * h) + i) - ((a + 2.0 * b) + c)) * zf / (8.0 * dy);
    const double st = sqrt(dzdx * dzdx + dzdy * dzdy);
    out[TV_DZDX] = dzdx;
    out[TV_DZDY] = dzdy;
    out[TV_SLOPE_TAN] = st;
    if (mask & (1u << TV_SLOPE_DEG)) out[TV_SLOPE_DEG] = atan(st) * TERRAIN_DEG;
    const bool flat = st == 0.0;
    if (mask & (1u << TV_EASTNESS)) out[TV_EASTNESS] = flat ? 0.0 : -dzdx / st;         // a division is asked for, or not made
    if (mask & (1u << TV_NORTHNESS)) out[TV_NORTHNESS] = flat ? 0.0 : dzdy / st;
    if (mask & (1u << TV_ASPECT_DEG)) {
        const double deg = atan2(-dzdx, dzdy) * TERRAIN_DEG;
        out[TV_ASPECT_DEG] = flat ? -1.0 : deg < 0.0 ? deg + 360.0 : deg;
    }
    const double sum = ((((((a + b) + c) + d) + f) + g) + h) + i;
    out[TV_TPI] = (e - sum / 8.0) * zf;
    const double dev = ((((((fabs(a - e) + fabs(b - e)) + fabs(c - e)) + fabs(d - e)) + fabs(f - e)) + fabs(g - e)) + fabs(h - e)) + fabs(i - e);
    out[TV_TRI] = dev / 8.0 * zf;
    double mn = a, mx = a;
    for (int k = 1; k < 9; ++k) { mn = z[k] < mn ? z[k] : mn; mx = z[k] > mx ? z[k] : mx; }
    out[TV_ROUGHNESS] = (mx - mn) * zf;
}

// half width of the circular window of radius R in the row |dr| <= R away: the largest dc with dr^2 + dc^2 <= R^2
MHS_TERRAIN_HD inline int relief_half_width(int R, int dr) {
    int dc = 0;
    while ((dc + 1) * (dc + 1) + dr * dr <= R * R) ++dc;
    return dc;
}

// 2. THE relief rule for a centre e that is not NA: the offsets of the circular window row-major, NA cells and cells outside
// the raster skipped, the sum added in that order.  out = above_min, below_max, minus_mean.
template <class A>
MHS_TERRAIN_HD inline void relief_cell(const A &acc, int R, const int16_t *w, double e, double zf, double out[RS_COUNT]) {
    double mn = e, mx = e, sum = 0.0;               // the centre is one of the offsets, so min <= e <= max either way
    int count = 0;
    const int r_lo = -(R < acc.up ? R : acc.up), r_hi = R < acc.down ? R : acc.down;
    for (int dr = r_lo; dr <= r_hi; ++dr) {
        const int hw = w[dr < 0 ? -dr : dr];
        const int c_lo = -(hw < acc.left ? hw : acc.left), c_hi = hw < acc.right ? hw : acc.right;
        for (int dc = c_lo; dc <= c_hi; ++dc) {
            double z;
            if (!acc.get(dr, dc, z)) continue;
            mn = z < mn ? z : mn;
            mx = z > mx ? z : mx;
            sum = sum + z;
            ++count;
        }
    }
    out[RS_ABOVE_MIN] = (e - mn) * zf;
    out[RS_BELOW_MAX] = (mx - e) * zf;
    out[RS_MINUS_MEAN] = (e - sum / (double)count) * zf;
}

// the paper's table: the form of (n_minus, n_plus), n_minus + n_plus <= 8
// 1 flat FL, 2 peak PK, 3 ridge RI, 4 shoulder SH, 5 spur SP, 6 slope SL, 7 hollow HO, 8 footslope FS, 9 valley VL, 10 pit PT
MHS_TERRAIN_HD inline int16_t geomorphon_form(int n_minus, int n_plus) {
    const unsigned char form[81] = {
        1, 1, 1, 8, 8, 9, 9, 9, 10,
        1, 1, 8, 8, 8, 9, 9, 9, 0,
        1, 4, 6, 6, 7, 7, 9, 0, 0,
        4, 4, 6, 6, 6, 7, 0, 0, 0,
        4, 4, 5, 6, 6, 0, 0, 0, 0,
        3, 3, 5, 5, 0, 0, 0, 0, 0,
        3, 3, 3, 0, 0, 0, 0, 0, 0,
        3, 3, 0, 0, 0, 0, 0, 0, 0,
        2, 0, 0, 0, 0, 0, 0, 0, 0};
    return (int16_t)form[n_minus * 9 + n_plus];
}

// 3. THE geomorphon rule for a centre e that is not NA.  L = search length in cells, t = flat_deg (pi / 180); dx is the
// width of the CENTRE's row.  Directions N, NE, E, SE, S, SW, W, NW.
template <class A>
MHS_TERRAIN_HD inline int16_t geomorphon_cell(const A &acc, int L, double t, double e, double dx, double dy, double zf) {
    const int ddr[8] = {-1, -1, 0, 1, 1, 1, 0, -1}, ddc[8] = {0, 1, 1, 1, 0, -1, -1, -1};
    const double diag = sqrt(dy * dy + dx * dx);
    int n_minus = 0, n_plus = 0;
    bool na = false;
    for (int dir = 0; dir < 8; ++dir) {
        const int dr = ddr[dir], dc = ddc[dir];
        int kmax = L;
        if (dr < 0) kmax = kmax < acc.up ? kmax : acc.up;
        if (dr > 0) kmax = kmax < acc.down ? kmax : acc.down;
        if (dc < 0) kmax = kmax < acc.left ? kmax : acc.left;
        if (dc > 0) kmax = kmax < acc.right ? kmax : acc.right;
        const double step = dc == 0 ? dy : dr == 0 ? dx : diag;
        double a = 0.0, b = 0.0;
        int k = 1;
        for (; k <= kmax; ++k) {
            double z;
            if (!acc.get(k * dr, k * dc, z)) break;             // a ray stops at the first NA
            const double s = ((z - e) * zf) / ((double)k * step);
            a = (k == 1 || s > a) ? s : a;
            b = (k == 1 || s < b) ? s : b;
        }
        if (k == 1) { na = true; continue; }                    // no valid step on this ray
        const double delta = atan(a) + atan(b);                 // nadir minus zenith angle
        n_plus += delta > t;
        n_minus += delta < -t;
    }
    return na ? GEOMORPHON_NA : geomorphon_form(n_minus, n_plus);
}

}  // namespace mhs
