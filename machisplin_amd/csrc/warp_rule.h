// The warp rule (include/machisplin_hip.h, section "warp"): the source point of a target cell from a control lattice of the
// target grid, and the cell's value there by the "resample" section's interpolating methods.  Free of any HIP header: the
// kernel of warp.hip and a plain C++ check program (tests/warp_check.cpp) share it.  The operations stand here in the header's
// order, each rounded once (the library is built with -ffp-contract=off), and there is no transcendental, so a numpy restatement
// gives the same bits.
#pragma once

#include "resample_rule.h"

namespace mhs {

constexpr int WARP_MAX_STEP = 1024;

// nodes along an axis of n target cells at step K: ceil(n / K) + 1
MHS_RESAMPLE_HD inline int64_t warp_nodes(int64_t n, int step) { return (n + step - 1) / step + 1; }
MHS_RESAMPLE_HD inline bool warp_step_ok(int64_t step) { return step >= 1 && step <= WARP_MAX_STEP && (step & (step - 1)) == 0; }

// where a target row or column lies in its lattice cell: the node before it and the fraction (idx - a K + 0.5) / K, exact
struct WarpFrac { int node; double t; };
MHS_RESAMPLE_HD inline WarpFrac warp_frac(int idx, int step) {
    const int a = idx / step;
    return WarpFrac{a, ((double)(idx - a * step) + 0.5) / (double)step};
}

// (1 - tv) ((1 - tu) p00 + tu p01) + tv ((1 - tu) p10 + tu p11)
MHS_RESAMPLE_HD inline double warp_bilerp(double p00, double p01, double p10, double p11, double tu, double tv) {
    const double u0 = 1.0 - tu, v0 = 1.0 - tv;
    const double top = u0 * p00 + tu * p01;
    const double bot = u0 * p10 + tu * p11;
    return v0 * top + tv * bot;
}

MHS_RESAMPLE_HD inline bool warp_finite(double v) { return v - v == 0.0; }      // neither NaN nor an infinity

// The source point of target cell (r, c).  `L` gives node values: L.x(a, b), L.y(a, b) for 0 <= a <= r / K + 1, 0 <= b <= c / K + 1.
// false: one of the eight node values is not finite (the cell is NA).
template <class L>
MHS_RESAMPLE_HD inline bool warp_source_point(const L &lat, int step, int r, int c, double &sx, double &sy) {
    const WarpFrac fv = warp_frac(r, step), fu = warp_frac(c, step);
    const double x00 = lat.x(fv.node, fu.node), x01 = lat.x(fv.node, fu.node + 1), x10 = lat.x(fv.node + 1, fu.node), x11 = lat.x(fv.node + 1, fu.node + 1);
    const double y00 = lat.y(fv.node, fu.node), y01 = lat.y(fv.node, fu.node + 1), y10 = lat.y(fv.node + 1, fu.node), y11 = lat.y(fv.node + 1, fu.node + 1);
    if (!(warp_finite(x00) && warp_finite(x01) && warp_finite(x10) && warp_finite(x11) && warp_finite(y00) && warp_finite(y01) && warp_finite(y10) &&
          warp_finite(y11)))
        return false;
    sx = warp_bilerp(x00, x01, x10, x11, fu.t, fv.t);
    sy = warp_bilerp(y00, y01, y10, y11, fu.t, fv.t);
    return true;
}

// a dense row-major lattice in memory
struct WarpLatticeMem {
    const double *sx, *sy;
    int64_t n_node_cols;
    MHS_RESAMPLE_HD double x(int a, int b) const { return sx[(int64_t)a * n_node_cols + b]; }
    MHS_RESAMPLE_HD double y(int a, int b) const { return sy[(int64_t)a * n_node_cols + b]; }
};

// the value of target cell (r, c) through an accessor of the source: false = NA
template <class A, class L>
MHS_RESAMPLE_HD inline bool warp_cell(const A &acc, const RsGrid &S, const L &lat, int step, int method, int r, int c, double &out) {
    double sx, sy;
    if (!warp_source_point(lat, step, r, c, sx, sy)) return false;
    return rs_interp(acc, S, method, sx, sy, out);
}

}  // namespace mhs
