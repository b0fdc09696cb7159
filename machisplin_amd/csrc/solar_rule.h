// The solar rules (include/machisplin_hip.h, section "solar"): the local horizon along sixteen rays, the sky-view factor,
// potential direct insolation and sun hours from host-made sun tables.  Free of any HIP header, as terrain_rule.h is: the
// kernel of terrain.hip and a plain C++ check program (tests/solar_check.cpp) share it.  The neighbourhood is read through
// the accessor of terrain_rule.h.  Only + - * /, sqrt and comparisons occur, each in the header's order and rounded once
// (the library is built with -ffp-contract=off): every plane is an exact function of the input and a numpy restatement gives
// the same bits.
#pragma once

#include "terrain_rule.h"

namespace mhs {

// bit k of the `products` mask of mhs_solar*; the output planes follow in this order (horizon: sixteen planes)
enum { SP_SVF = 0, SP_DIRECT, SP_SUN_HOURS, SP_HORIZON, SP_COUNT };
constexpr int SOLAR_DIRS = 16;

// mhs_sun_entry: one position of the sun in a table (64 bytes)
struct SunEntry {
    double t;               // position of the azimuth between direction j and j + 1, in [0, 1]
    double tan_h;           // tangent of the elevation, > 0
    double ux, uy, uz;      // east, north and up components
    double w, d;            // energy and time weight
    double pad;
};

// the step vector of direction j: rows south, columns east.  N NNE NE ENE E ESE SE SSE S SSW SW WSW W WNW NW NNW
MHS_TERRAIN_HD constexpr int solar_dr(int j) {
    return j == 0 ? -1 : j == 1 ? -2 : j == 2 ? -1 : j == 3 ? -1 : j == 4 ? 0 : j == 5 ? 1 : j == 6 ? 1 : j == 7 ? 2
         : j == 8 ? 1 : j == 9 ? 2 : j == 10 ? 1 : j == 11 ? 1 : j == 12 ? 0 : j == 13 ? -1 : j == 14 ? -1 : -2;
}
MHS_TERRAIN_HD constexpr int solar_dc(int j) {
    return j == 0 ? 0 : j == 1 ? 1 : j == 2 ? 1 : j == 3 ? 2 : j == 4 ? 1 : j == 5 ? 2 : j == 6 ? 1 : j == 7 ? 1
         : j == 8 ? 0 : j == 9 ? -1 : j == 10 ? -1 : j == 11 ? -2 : j == 12 ? -1 : j == 13 ? -2 : j == 14 ? -1 : -1;
}

// (a) the horizon tangent of a centre e that is not NA along the ray (dr, dc): the largest s_m > 0, else 0.  An NA cell on
// the ray is skipped, the ray goes on; it ends at the search length L (Chebyshev) or at the raster's border.
template <class A>
MHS_TERRAIN_HD inline double solar_ray(const A &acc, int dr, int dc, int L, double e, double dx, double dy, double zf) {
    const int ar = dr < 0 ? -dr : dr, ac = dc < 0 ? -dc : dc;
    int mmax = L / (ar > ac ? ar : ac);
    if (dr < 0) mmax = mmax < acc.up / ar ? mmax : acc.up / ar;
    if (dr > 0) mmax = mmax < acc.down / ar ? mmax : acc.down / ar;
    if (dc < 0) mmax = mmax < acc.left / ac ? mmax : acc.left / ac;
    if (dc > 0) mmax = mmax < acc.right / ac ? mmax : acc.right / ac;
    const double ry = (double)ar * dy, rx = (double)ac * dx;
    const double len = sqrt(ry * ry + rx * rx);
    double h = 0.0;
    for (int m = 1; m <= mmax; ++m) {
        double z;
        if (!acc.get(m * dr, m * dc, z)) continue;
        const double s = ((z - e) * zf) / ((double)m * len);
        h = s > h ? s : h;
    }
    return h;
}

// the sixteen horizon tangents; dx is the width of the CENTRE's row.  Every index into H is a constant once unrolled.
template <class A>
MHS_TERRAIN_HD inline void solar_horizon(const A &acc, int L, double e, double dx, double dy, double zf, double H[SOLAR_DIRS]) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < SOLAR_DIRS; ++j) H[j] = solar_ray(acc, solar_dr(j), solar_dc(j), L, e, dx, dy, zf);
}

// (b) the Horn slope of the cell: false where any of the nine cells is NA or outside the raster
template <class A>
MHS_TERRAIN_HD inline bool solar_slope(const A &acc, double dx, double dy, double zf, double &dzdx, double &dzdy, double &nrm) {
    if (acc.up < 1 || acc.down < 1 || acc.left < 1 || acc.right < 1) return false;
    double z[9], o[TV_COUNT];
    bool ok = true;
    for (int k = 0; k < 9; ++k) ok &= acc.get(k / 3 - 1, k % 3 - 1, z[k]);
    if (!ok) return false;
    terrain_3x3(z, dx, dy, zf, 0u, o);
    dzdx = o[TV_DZDX];
    dzdy = o[TV_DZDY];
    nrm = sqrt((1.0 + dzdx * dzdx) + dzdy * dzdy);
    return true;
}

// (d) 0: the sky-view factor, omega = the sixteen sector weights of the row's table
MHS_TERRAIN_HD inline double solar_svf(const double H[SOLAR_DIRS], const double *omega) {
    double v = 0.0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < SOLAR_DIRS; ++j) v = v + omega[j] / (1.0 + H[j] * H[j]);
    return v;
}

// (d) 1 and 2: the walk over the row's table, start = its seventeen offsets into entries.  acc is the beam sum before the
// division by nrm, hrs the sun hours; only what DIRECT / HOURS ask for is made.  The loop over the sectors is unrolled
// around the loop over a sector's entries, so H[j] and H[j1] are fixed names.
template <bool DIRECT, bool HOURS, typename I>
MHS_TERRAIN_HD inline void solar_walk(const double H[SOLAR_DIRS], const I *start, const SunEntry *entries, double dzdx, double dzdy,
                                      double &acc, double &hrs) {
    acc = 0.0;
    hrs = 0.0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < SOLAR_DIRS; ++j) {
        const double h0 = H[j], dh = H[(j + 1) & 15] - h0;
        const I i1 = start[j + 1];
        for (I i = start[j]; i < i1; ++i) {
            const SunEntry s = entries[i];
            const double hs = h0 + s.t * dh;
            if (s.tan_h > hs) {
                if (HOURS) hrs = hrs + s.d;
                if (DIRECT) {
                    const double c = (s.uz - dzdx * s.ux) + dzdy * s.uy;
                    if (c > 0.0) acc = acc + s.w * c;
                }
            }
        }
    }
}

}  // namespace mhs
