// The hydrology rules (include/machisplin_hip.h, section "hydrology"): flat fill, flat distance, D8 direction, flow
// accumulation and the topographic wetness index of one elevation plane.  Free of any HIP header: the kernels of hydro.hip and
// a plain C++ check program (tests/hydro_check.cpp) share it.  The header states the rules; the operations stand here in that
// order, each rounded once (the library is built with -ffp-contract=off), so a numpy restatement gives the same bits -- except
// through log, which no two math libraries need round alike.  Rules 6 and 7 (section "hydrology, multiple flow direction":
// the shares and the accumulation over them; tests/hydro_mfd_check.cpp) follow the five; there pow joins log unless the
// exponent is 1.
//
// A rule sees the eight neighbours of its cell as arrays indexed by k = 0 .. 7 = E, SE, S, SW, W, NW, N, NE:
//   wn[k]   the neighbour's filled value W, NaN where that cell is outside the raster or NA ("not a neighbour")
//   dn[k]   its flat distance D (looked at only where wn[k] is not NaN)
// so a rule never sees how the planes are stored (an LDS tile or a host array).  The three fixed points (W, D, A) are
// MONOTONE: W and D start from above (+inf, HYDRO_D_INF) and a step can only lower them, A starts from 1 and a step can only
// raise it.  Whatever the order in which cells are stepped, and whether a step reads a neighbour's old or new value, the
// iteration ends in the same, the greatest (W, D) or the least (A), fixed point.
#pragma once

#include <cmath>
#include <cstdint>

#include "terrain_rule.h"

namespace mhs {

constexpr int8_t HYDRO_DIR_OUT = -1;                  // an outlet with nothing lower: the water leaves the raster
constexpr int8_t HYDRO_DIR_NA = -2;                   // an NA cell
constexpr int32_t HYDRO_D_INF = 2147483647;           // "no distance yet"

// neighbour k lies hydro_dr(k) rows south and hydro_dc(k) columns east of the centre; neighbour (k + 4) & 7 is the opposite one
MHS_TERRAIN_HD inline int hydro_dr(int k) { return (k >= 1 && k <= 3) ? 1 : (k >= 5) ? -1 : 0; }
MHS_TERRAIN_HD inline int hydro_dc(int k) { return (k <= 1 || k == 7) ? 1 : (k >= 3 && k <= 5) ? -1 : 0; }

// the distances d_k to the eight neighbours: dx is the width of the CENTRE's row
MHS_TERRAIN_HD inline void hydro_distances(double dx, double dy, double d[8]) {
    const double g = sqrt(dx * dx + dy * dy);
    d[0] = dx; d[1] = g; d[2] = dy; d[3] = g; d[4] = dx; d[5] = g; d[6] = dy; d[7] = g;
}

// an OUTLET: a valid cell one of whose eight is not a neighbour -- on the raster's outer ring, or beside an NA cell
MHS_TERRAIN_HD inline bool hydro_outlet(const double wn[8]) {
    bool out = false;
    for (int k = 0; k < 8; ++k) out |= wn[k] != wn[k];
    return out;
}

// 1. one step of the FILL at a valid cell that is no outlet (all eight are neighbours): max(z, min W(k)).  W = z at outlets.
MHS_TERRAIN_HD inline double hydro_fill_step(double z, const double wn[8]) {
    double m = wn[0];
    for (int k = 1; k < 8; ++k) m = wn[k] < m ? wn[k] : m;
    return z > m ? z : m;
}

// 2. FLAT DISTANCE.  The seeds D = 0: outlets and cells with a strictly lower neighbour ...
MHS_TERRAIN_HD inline bool hydro_has_lower(double w, const double wn[8]) {
    bool lower = false;
    for (int k = 0; k < 8; ++k) lower |= wn[k] < w;             // false for a NaN
    return lower;
}
// ... and one step elsewhere: 1 + min D(k) over the neighbours with W(k) == W, HYDRO_D_INF while none of them has a distance
MHS_TERRAIN_HD inline int32_t hydro_flat_step(double w, const double wn[8], const int32_t dn[8]) {
    int32_t m = HYDRO_D_INF;
    for (int k = 0; k < 8; ++k)
        if (wn[k] == w && dn[k] < m) m = dn[k];
    return m == HYDRO_D_INF ? HYDRO_D_INF : m + 1;
}

// 3. DIRECTION of a valid cell: the k of the largest s_k = (W - W(k)) / d_k > 0, the lowest k on ties; none and D > 0: the
// lowest k with W(k) == W and D(k) == D - 1; none and D == 0: HYDRO_DIR_OUT.
MHS_TERRAIN_HD inline int8_t hydro_direction(double w, int32_t dist, const double wn[8], const int32_t dn[8], double dx, double dy) {
    double d[8];
    hydro_distances(dx, dy, d);
    int best = -1;
    double s_best = 0.0;
    for (int k = 0; k < 8; ++k) {
        if (wn[k] != wn[k]) continue;
        const double s = (w - wn[k]) / d[k];
        if (s > s_best) { s_best = s; best = k; }
    }
    if (best >= 0) return (int8_t)best;
    if (dist > 0)
        for (int k = 0; k < 8; ++k)
            if (wn[k] == w && dn[k] == dist - 1) return (int8_t)k;
    return HYDRO_DIR_OUT;
}

// 4. ACCUMULATION.  The DONORS of a cell, looked at once: bit k is set where neighbour k's direction points at the centre.
// dirn[k] = the direction of neighbour k (HYDRO_DIR_NA where it is none) ...
MHS_TERRAIN_HD inline unsigned hydro_donors(const int8_t dirn[8]) {
    unsigned donors = 0;
    for (int k = 0; k < 8; ++k) donors |= (dirn[k] == ((k + 4) & 7) ? 1u : 0u) << k;
    return donors;
}
// ... and one step: 1 + the A of the donors; an integer count held in a double, exact below 2^53
MHS_TERRAIN_HD inline double hydro_acc_step(unsigned donors, const double an[8]) {
    double a = 1.0;
    for (int k = 0; k < 8; ++k)
        if (donors & (1u << k)) a = a + an[k];
    return a;
}

// 5. TWI from the nine FILLED values (a b c / d e f / g h i, north row first, none NA) and the cell's accumulation
MHS_TERRAIN_HD inline double hydro_twi(const double w9[9], double acc, double dx, double dy, double zf, double min_slope_tan) {
    double o[TV_COUNT];
    terrain_3x3(w9, dx, dy, zf, 1u << TV_SLOPE_TAN, o);
    const double t = o[TV_SLOPE_TAN];
    const double len = sqrt(dx * dy);
    const double a = acc * len;
    return log(a / (t > min_slope_tan ? t : min_slope_tan));
}

// The rules of section "hydrology, multiple flow direction".  Rules 1 and 2 (W, D) are the ones above.
constexpr double HYDRO_MFD_MAX_EXPONENT = 64.0;

// 6. SHARES of a valid cell, the DONOR: f[k] = the part of its water that goes to neighbour k, dx = the width of the donor's
// row.  Steep (some s_k > 0): p_k = s_k / s_max, raised to x unless x == 1, over their sum in k order; else D > 0: 1 / m to each
// of the m neighbours of equal W one step nearer the flat's exit; else none (false): the water leaves.  pow is called only
// for 0 < p_k < 1: pow(0, x) = 0 and pow(1, x) = 1 exactly, so the steepest neighbour has p = 1 and the sum is >= 1.
MHS_TERRAIN_HD inline bool hydro_mfd_shares(double w, int32_t dist, const double wn[8], const int32_t dn[8], double dx, double dy, double x,
                                            double f[8]) {
    double d[8], s[8];
    hydro_distances(dx, dy, d);
    double s_max = 0.0;
    for (int k = 0; k < 8; ++k) {
        s[k] = (w - wn[k]) / d[k];                              // NaN where there is no neighbour
        if (s[k] > s_max) s_max = s[k];
    }
    if (s_max > 0.0) {
        double sum = 0.0;
        for (int k = 0; k < 8; ++k) {
            double p = s[k] > 0.0 ? s[k] / s_max : 0.0;
            if (x != 1.0 && p > 0.0 && p < 1.0) p = pow(p, x);
            f[k] = p;
            sum = sum + p;
        }
        for (int k = 0; k < 8; ++k) f[k] = f[k] / sum;
        return true;
    }
    int m = 0;
    for (int k = 0; k < 8; ++k) {
        f[k] = 0.0;
        m += (dist > 0 && wn[k] == w && dn[k] == dist - 1) ? 1 : 0;
    }
    if (m == 0) return false;
    const double each = 1.0 / (double)m;
    for (int k = 0; k < 8; ++k)
        if (wn[k] == w && dn[k] == dist - 1) f[k] = each;
    return true;
}

// 7. one step of the MFD ACCUMULATION: fin[k] = f(k -> c), the share neighbour k sends to the cell (0 where it sends none or
// is no neighbour); product first, then the add, in k order
MHS_TERRAIN_HD inline double hydro_mfd_step(const double fin[8], const double an[8]) {
    double a = 1.0;
    for (int k = 0; k < 8; ++k)
        if (fin[k] > 0.0) a = a + fin[k] * an[k];
    return a;
}

}  // namespace mhs
