// Plain C++ check of machisplin_amd/csrc/terrain_rule.h (no HIP): the three rules on the hand-computed table of
// tests/test_terrain_host.py, read through a host accessor over a row-major array.  Built with -fsanitize=address,undefined by
// the test and run stand-alone.  Prints "name value" lines (%.17g), then "OK".
#include <cmath>
#include <cstdio>
#include <vector>
#include "terrain_rule.h"

struct Plane {
    std::vector<double> z;
    int nr, nc;
    Plane(int r, int c) : z((size_t)r * c, 0.0), nr(r), nc(c) {}
    double &at(int r, int c) { return z[(size_t)r * nc + c]; }
};

struct HostAcc {            // the accessor of terrain_rule.h over a Plane, centred on (r, c)
    const Plane *p;
    int r, c;
    int up, down, left, right;
    HostAcc(const Plane &pl, int r_, int c_) : p(&pl), r(r_), c(c_), up(r_), down(pl.nr - 1 - r_), left(c_), right(pl.nc - 1 - c_) {}
    bool get(int dr, int dc, double &z) const {
        z = p->z.at((size_t)(r + dr) * p->nc + (c + dc));        // .at(): a rule that leaves the raster throws
        return !mhs::terrain_na(z, false, 0.0);
    }
};

static int form_at_centre(const Plane &p) {
    HostAcc acc(p, p.nr / 2, p.nc / 2);
    double e;
    if (!acc.get(0, 0, e)) return mhs::GEOMORPHON_NA;
    return mhs::geomorphon_cell(acc, 5, 1.0 * mhs::TERRAIN_RAD, e, 1.0, 1.0, 1.0);
}

int main() {
    const char *names[mhs::TV_COUNT] = {"dzdx", "dzdy", "slope_tan", "slope_deg", "eastness", "northness", "aspect_deg", "tpi", "tri", "roughness"};
    double o[mhs::TV_COUNT];
    const unsigned all = (1u << mhs::TV_COUNT) - 1;
    const double hand[9] = {1, 2, 3, 4, 5, 6, 7, 8, 10};
    mhs::terrain_3x3(hand, 2.0, 4.0, 1.0, all, o);
    for (int k = 0; k < mhs::TV_COUNT; ++k) std::printf("hand_%s %.17g\n", names[k], o[k]);
    double east[9], south[9], flat[9];
    for (int k = 0; k < 9; ++k) { east[k] = 3.0 * (k % 3); south[k] = 3.0 * (k / 3); flat[k] = 7.0; }
    mhs::terrain_3x3(east, 1.0, 1.0, 1.0, all, o);
    std::printf("east_aspect_deg %.17g\neast_eastness %.17g\neast_northness %.17g\n", o[mhs::TV_ASPECT_DEG], o[mhs::TV_EASTNESS], o[mhs::TV_NORTHNESS]);
    mhs::terrain_3x3(south, 1.0, 1.0, 1.0, all, o);
    std::printf("south_aspect_deg %.17g\n", o[mhs::TV_ASPECT_DEG]);
    mhs::terrain_3x3(flat, 1.0, 1.0, 1.0, all, o);
    std::printf("flat_aspect_deg %.17g\nflat_eastness %.17g\nflat_northness %.17g\n", o[mhs::TV_ASPECT_DEG], o[mhs::TV_EASTNESS], o[mhs::TV_NORTHNESS]);

    // relief, R = 1, on z = 5 r + c with an NA at (2, 3): the centre (next to the NA) and the corner (outside cells skipped)
    Plane p(5, 5);
    for (int r = 0; r < 5; ++r) for (int c = 0; c < 5; ++c) p.at(r, c) = 5.0 * r + c;
    p.at(2, 3) = NAN;
    int16_t w[3];
    for (int dr = 0; dr <= 2; ++dr) w[dr] = (int16_t)mhs::relief_half_width(2, dr);
    if (w[0] != 2 || w[1] != 1 || w[2] != 0) { std::printf("half widths of R = 2 wrong\n"); return 1; }
    w[0] = (int16_t)mhs::relief_half_width(1, 0); w[1] = (int16_t)mhs::relief_half_width(1, 1);
    double rs[mhs::RS_COUNT];
    mhs::relief_cell(HostAcc(p, 2, 2), 1, w, p.at(2, 2), 1.0, rs);
    std::printf("relief_centre_above_min %.17g\nrelief_centre_below_max %.17g\nrelief_centre_minus_mean %.17g\n", rs[0], rs[1], rs[2]);
    mhs::relief_cell(HostAcc(p, 0, 0), 1, w, p.at(0, 0), 1.0, rs);
    std::printf("relief_corner_above_min %.17g\nrelief_corner_below_max %.17g\nrelief_corner_minus_mean %.17g\n", rs[0], rs[1], rs[2]);

    // geomorphons at the centre of six 21 x 21 shapes, L = 5, flat_deg = 1
    Plane cone(21, 21), pit(21, 21), incl(21, 21), level(21, 21), roof(21, 21), vee(21, 21);
    for (int r = 0; r < 21; ++r)
        for (int c = 0; c < 21; ++c) {
            const double d = std::sqrt((double)((r - 10) * (r - 10) + (c - 10) * (c - 10)));
            cone.at(r, c) = -d; pit.at(r, c) = d; incl.at(r, c) = c; level.at(r, c) = 3.0;
            roof.at(r, c) = -std::fabs((double)(c - 10)); vee.at(r, c) = std::fabs((double)(c - 10));
        }
    std::printf("form_cone %d\nform_pit %d\nform_inclined %d\nform_constant %d\nform_roof %d\nform_vee %d\n", form_at_centre(cone),
                form_at_centre(pit), form_at_centre(incl), form_at_centre(level), form_at_centre(roof), form_at_centre(vee));
    // the border has a ray with no valid step, an NA centre is NA
    double e;
    HostAcc border(level, 0, 10);
    border.get(0, 0, e);
    std::printf("form_border %d\n", (int)mhs::geomorphon_cell(border, 5, 0.0, e, 1.0, 1.0, 1.0));
    // every (minus, plus) of the table is one of the ten forms
    for (int m = 0; m <= 8; ++m)
        for (int q = 0; m + q <= 8; ++q)
            if (mhs::geomorphon_form(m, q) < 1 || mhs::geomorphon_form(m, q) > 10) { std::printf("no form for %d %d\n", m, q); return 1; }
    std::printf("OK\n");
    return 0;
}
