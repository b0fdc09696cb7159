// The resampling rules (include/machisplin_hip.h, section "resample"): the value of a target cell, or of a point, from a source
// raster in the same coordinate system -- nearest cell, bilinear, cubic (Catmull-Rom) -- and the footprints of the aggregates
// mean / min / max / sum / count.  Free of any HIP header: the kernels of resample.hip and a plain C++ check program
// (tests/resample_check.cpp) share it.  The operations stand here in the header's order, each rounded once (the library is
// built with -ffp-contract=off), and there is no transcendental, so a numpy restatement gives the same bits.
//
// A rule reads the source through an ACCESSOR `A`:
//   bool A::get(i, j, double &z)     the value of source cell (row i, column j), converted exactly to double; false where the
//                                    cell is outside the raster or NA
// so a rule never sees how the plane is stored (an LDS tile in the plane's own type, global memory, a host array).
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MHS_RESAMPLE_HD __host__ __device__
#else
#define MHS_RESAMPLE_HD
#endif

namespace mhs {

// the methods of mhs_resample* and mhs_extract_points* (the MHS_RS_* of the header, in its order)
enum { RS_NEAR = 0, RS_BILINEAR, RS_CUBIC, RS_MEAN, RS_MIN, RS_MAX, RS_SUM, RS_COUNT_CELLS, RS_METHODS };

struct RsGrid {          // mhs_grid with int dimensions
    double xmin, ymax, xres, yres;
    int nrow, ncol;
};

// a plane value converted exactly to double is NA when it is NaN or equals the stack's nodata
MHS_RESAMPLE_HD inline bool rs_na(double v, bool has_nodata, double nodata) { return v != v || (has_nodata && v == nodata); }

// centre of target cell (r, c)
MHS_RESAMPLE_HD inline double rs_cell_x(const RsGrid &T, int c) { return T.xmin + ((double)c + 0.5) * T.xres; }
MHS_RESAMPLE_HD inline double rs_cell_y(const RsGrid &T, int r) { return T.ymax - ((double)r + 0.5) * T.yres; }

// terra's colFromX / rowFromY as mhs_cells_from_xy has them: the east and south edges belong to the last column and row, -1
// outside (and for NaN).  A quotient that rounds up to the dimension just inside the far edge stays in the last column / row.
MHS_RESAMPLE_HD inline int rs_col_from_x(const RsGrid &S, double x) {
    const double xmax = S.xmin + (double)S.ncol * S.xres;
    if (x == xmax) return S.ncol - 1;
    if (!(x >= S.xmin && x <= xmax)) return -1;
    const double q = floor((x - S.xmin) / S.xres);
    return q < (double)(S.ncol - 1) ? (int)q : S.ncol - 1;
}
MHS_RESAMPLE_HD inline int rs_row_from_y(const RsGrid &S, double y) {
    const double ymin = S.ymax - (double)S.nrow * S.yres;
    if (y == ymin) return S.nrow - 1;
    if (!(y >= ymin && y <= S.ymax)) return -1;
    const double q = floor((S.ymax - y) / S.yres);
    return q < (double)(S.nrow - 1) ? (int)q : S.nrow - 1;
}

// The interpolation coordinate along one axis: f = d / res - 0.5 (d = x - xmin, or ymax - y), i0 = floor(f), t = f - i0.
// Where the point has a cell, f lies in [-0.5, n - 0.5]; beyond [-4, n + 4] (the output is NA there) f is held at that bound so
// that i0 is an int whatever the point.
struct RsAxis { int i0; double t; };
MHS_RESAMPLE_HD inline RsAxis rs_axis(double d, double res, int n) {
    double f = d / res - 0.5;
    if (!(f >= -4.0)) f = -4.0;
    if (f > (double)n + 4.0) f = (double)n + 4.0;
    const double fl = floor(f);
    return RsAxis{(int)fl, f - fl};
}
MHS_RESAMPLE_HD inline RsAxis rs_axis_x(const RsGrid &S, double x) { return rs_axis(x - S.xmin, S.xres, S.ncol); }
MHS_RESAMPLE_HD inline RsAxis rs_axis_y(const RsGrid &S, double y) { return rs_axis(S.ymax - y, S.yres, S.nrow); }

// the Catmull-Rom weights (a = -0.5) of the taps i0 - 1 .. i0 + 2 for the fraction t, in Horner form
MHS_RESAMPLE_HD inline void rs_cubic_weights(double t, double w[4]) {
    w[0] = ((-0.5 * t + 1.0) * t - 0.5) * t;
    w[1] = ((1.5 * t - 2.5) * t) * t + 1.0;
    w[2] = ((-1.5 * t + 2.0) * t + 0.5) * t;
    w[3] = ((0.5 * t - 0.5) * t) * t;
}

// What one axis contributes to an interpolated value: the nearest cell (-1: no cell), i0, and the weights of the bilinear taps
// i0, i0 + 1 and of the cubic taps i0 - 1 .. i0 + 2.  Made once per target column and once per target row, used by every layer.
struct RsTaps {
    int near, i0;
    double wl[2], wc[4];
};
MHS_RESAMPLE_HD inline RsTaps rs_taps(int near, const RsAxis &a) {
    RsTaps t;
    t.near = near; t.i0 = a.i0;
    t.wl[0] = 1.0 - a.t; t.wl[1] = a.t;
    rs_cubic_weights(a.t, t.wc);
    return t;
}
MHS_RESAMPLE_HD inline RsTaps rs_taps_x(const RsGrid &S, double x) { return rs_taps(rs_col_from_x(S, x), rs_axis_x(S, x)); }
MHS_RESAMPLE_HD inline RsTaps rs_taps_y(const RsGrid &S, double y) { return rs_taps(rs_row_from_y(S, y), rs_axis_y(S, y)); }

// BILINEAR: taps (i0, j0), (i0, j0 + 1), (i0 + 1, j0), (i0 + 1, j0 + 1); a tap outside the raster, NA or of weight 0 is skipped
// and the weights of the others renormalise.  false: no tap left.
template <class A>
MHS_RESAMPLE_HD inline bool rs_bilinear(const A &acc, const RsTaps &ty, const RsTaps &tx, double &out) {
    double num = 0.0, den = 0.0;
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) {
            const double w = ty.wl[i] * tx.wl[j];
            double z;
            if (w == 0.0 || !acc.get(ty.i0 + i, tx.i0 + j, z)) continue;
            num = num + w * z;
            den = den + w;
        }
    if (!(den > 0.0)) return false;
    out = num / den;
    return true;
}

// CUBIC: the 4 x 4 taps, rows then columns.  false: a tap whose two weights are both not 0 is outside the raster or NA (the
// caller takes the BILINEAR value).  A tap with a weight of 0 enters as z = 0 when it has no value.
template <class A>
MHS_RESAMPLE_HD inline bool rs_cubic(const A &acc, const RsTaps &ty, const RsTaps &tx, double &out) {
    double rowv[4];
    for (int i = 0; i < 4; ++i) {
        double z[4];
        for (int j = 0; j < 4; ++j) {
            if (acc.get(ty.i0 - 1 + i, tx.i0 - 1 + j, z[j])) continue;
            if (tx.wc[j] != 0.0 && ty.wc[i] != 0.0) return false;
            z[j] = 0.0;
        }
        rowv[i] = ((tx.wc[0] * z[0] + tx.wc[1] * z[1]) + tx.wc[2] * z[2]) + tx.wc[3] * z[3];
    }
    out = ((ty.wc[0] * rowv[0] + ty.wc[1] * rowv[1]) + ty.wc[2] * rowv[2]) + ty.wc[3] * rowv[3];
    return true;
}

// the value of the point whose axes are ty, tx by an interpolating method; false = NA
template <class A>
MHS_RESAMPLE_HD inline bool rs_interp_at(const A &acc, int method, const RsTaps &ty, const RsTaps &tx, double &out) {
    if (tx.near < 0 || ty.near < 0) return false;
    if (method == RS_NEAR) return acc.get(ty.near, tx.near, out);
    if (method == RS_CUBIC && rs_cubic(acc, ty, tx, out)) return true;
    return rs_bilinear(acc, ty, tx, out);
}
template <class A>
MHS_RESAMPLE_HD inline bool rs_interp(const A &acc, const RsGrid &S, int method, double x, double y, double &out) {
    return rs_interp_at(acc, method, rs_taps_y(S, y), rs_taps_x(S, x), out);
}

// Aggregates: the first source index whose centre is not before the edge at distance d from the source's origin,
// ceil(d / res - 0.5) held in [0, n].  The footprint of target column c is [rs_edge(x0 - S.xmin), rs_edge(x1 - S.xmin)) with
// x0 = T.xmin + c T.xres and x1 = T.xmin + (c + 1) T.xres: x1 of c is x0 of c + 1, so the footprints partition the columns.
MHS_RESAMPLE_HD inline int rs_edge(double d, double res, int n) {
    const double q = ceil(d / res - 0.5);
    if (!(q > 0.0)) return 0;
    return q < (double)n ? (int)q : n;
}
MHS_RESAMPLE_HD inline int rs_foot_col(const RsGrid &S, const RsGrid &T, int c) { return rs_edge((T.xmin + (double)c * T.xres) - S.xmin, S.xres, S.ncol); }
MHS_RESAMPLE_HD inline int rs_foot_row(const RsGrid &S, const RsGrid &T, int r) { return rs_edge(S.ymax - (T.ymax - (double)r * T.yres), S.yres, S.nrow); }

// one row of a footprint, west to east from 0: its sum, count, and the first smallest and first largest value
struct RsPart {
    double sum, mn, mx;
    int count;
};
MHS_RESAMPLE_HD inline RsPart rs_part_empty() { return RsPart{0.0, 0.0, 0.0, 0}; }
MHS_RESAMPLE_HD inline void rs_part_add(RsPart &p, double z) {
    p.sum = p.sum + z;
    p.mn = (p.count == 0 || z < p.mn) ? z : p.mn;
    p.mx = (p.count == 0 || z > p.mx) ? z : p.mx;
    ++p.count;
}
// the rows of a footprint, north to south from 0: a sum of row sums
MHS_RESAMPLE_HD inline void rs_part_fold(RsPart &cell, const RsPart &row) {
    cell.sum = cell.sum + row.sum;
    if (row.count == 0) return;
    cell.mn = (cell.count == 0 || row.mn < cell.mn) ? row.mn : cell.mn;
    cell.mx = (cell.count == 0 || row.mx > cell.mx) ? row.mx : cell.mx;
    cell.count += row.count;
}
// the aggregate of a folded footprint; false = NA (MEAN, MIN, MAX of no valid cell)
MHS_RESAMPLE_HD inline bool rs_part_value(const RsPart &cell, int method, double &out) {
    if (method == RS_SUM) { out = cell.sum; return true; }
    if (method == RS_COUNT_CELLS) { out = (double)cell.count; return true; }
    if (cell.count == 0) return false;
    out = method == RS_MEAN ? cell.sum / (double)cell.count : method == RS_MIN ? cell.mn : cell.mx;
    return true;
}

// the whole aggregate of target cell (r, c) through an accessor: what the kernel's lanes do between them
template <class A>
MHS_RESAMPLE_HD inline bool rs_aggregate(const A &acc, const RsGrid &S, const RsGrid &T, int method, int r, int c, double &out) {
    const int j_lo = rs_foot_col(S, T, c), j_hi = rs_foot_col(S, T, c + 1);
    const int i_lo = rs_foot_row(S, T, r), i_hi = rs_foot_row(S, T, r + 1);
    RsPart cell = rs_part_empty();
    for (int i = i_lo; i < i_hi; ++i) {
        RsPart row = rs_part_empty();
        for (int j = j_lo; j < j_hi; ++j) {
            double z;
            if (acc.get(i, j, z)) rs_part_add(row, z);
        }
        rs_part_fold(cell, row);
    }
    return rs_part_value(cell, method, out);
}

}  // namespace mhs
