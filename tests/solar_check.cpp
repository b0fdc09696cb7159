// Plain C++ check of machisplin_amd/csrc/solar_rule.h (no HIP): the solar rules on the plane and the sun tables that
// tests/test_solar_host.py builds from the same formulas, read through a host accessor over a row-major array.  Built with
// -fsanitize=address,undefined by the test and run stand-alone.  For search lengths up to 45 on a plane that the rays leave on
// every side it prints "name value" lines (%.17g) for cells on every border, at the corners and inside, then "OK"; the test
// compares them with the numpy restatement.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "solar_rule.h"

constexpr int NR = 50, NC = 60;

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
        const int rr = r + dr, cc = c + dc;
        if (rr < 0 || rr >= p->nr || cc < 0 || cc >= p->nc) { std::printf("a rule left the raster at (%d, %d)\n", rr, cc); std::abort(); }
        z = p->z.at((size_t)rr * p->nc + cc);
        return !mhs::terrain_na(z, false, 0.0);
    }
};

int main() {
    Plane p(NR, NC);
    for (int r = 0; r < NR; ++r)
        for (int c = 0; c < NC; ++c) {
            p.at(r, c) = (double)((r * 37 + c * 91 + r * c * 7) % 101) + 0.25 * r;
            if ((r * 5 + c * 3 + 1) % 17 == 0) p.at(r, c) = NAN;
        }
    // two tables: sector j has j % 3 entries (so some have none), every value a small rational
    std::vector<mhs::SunEntry> entries;
    std::vector<int64_t> start(1, 0);
    std::vector<double> omega;
    for (int b = 0; b < 2; ++b)
        for (int j = 0; j < 16; ++j) {
            for (int k = 0; k < j % 3; ++k)
                entries.push_back(mhs::SunEntry{k / 4.0 + b / 8.0, 0.05 + 0.3 * j + b, (j - 8) / 16.0, (k - 1) / 4.0, 0.5, 1.0 + j, 0.5 + b, 0.0});
            start.push_back((int64_t)entries.size());
            omega.push_back((1.0 + (j + b) % 4) / 40.0);
        }
    const double dy = 28.5, zf = 0.3048;
    const int cells[9][2] = {{0, 0}, {0, NC - 1}, {NR - 1, 0}, {NR - 1, NC - 1}, {0, 31}, {NR - 1, 7}, {23, 0}, {24, NC - 1}, {25, 30}};
    const int searches[4] = {1, 7, 44, 45};
    for (int L : searches)
        for (const auto &rc : cells) {
            const int r = rc[0], c = rc[1], b = r >= 20;
            const double dx = 30.0 * (1.0 - 0.3 * r / (NR - 1));
            HostAcc acc(p, r, c);
            double e;
            if (!acc.get(0, 0, e)) { std::printf("cell %d %d is NA: choose another\n", r, c); return 1; }
            double H[mhs::SOLAR_DIRS], dzdx = 0.0, dzdy = 0.0, nrm = 1.0, beam, hrs, beam2, hrs2;
            mhs::solar_horizon(acc, L, e, dx, dy, zf, H);
            for (int j = 0; j < mhs::SOLAR_DIRS; ++j) std::printf("L%d_r%d_c%d_h%d %.17g\n", L, r, c, j, H[j]);
            std::printf("L%d_r%d_c%d_svf %.17g\n", L, r, c, mhs::solar_svf(H, omega.data() + 16 * b));
            const bool slope = mhs::solar_slope(acc, dx, dy, zf, dzdx, dzdy, nrm);
            mhs::solar_walk<true, true>(H, start.data() + 16 * b, entries.data(), dzdx, dzdy, beam, hrs);
            std::printf("L%d_r%d_c%d_direct %.17g\n", L, r, c, slope ? beam / nrm : (double)NAN);
            std::printf("L%d_r%d_c%d_sun_hours %.17g\n", L, r, c, hrs);
            // what is not asked for is not made, and what is made does not depend on it
            mhs::solar_walk<false, true>(H, start.data() + 16 * b, entries.data(), dzdx, dzdy, beam2, hrs2);
            if (hrs2 != hrs || beam2 != 0.0) { std::printf("the hours-only walk differs\n"); return 1; }
            mhs::solar_walk<true, false>(H, start.data() + 16 * b, entries.data(), dzdx, dzdy, beam2, hrs2);
            if (beam2 != beam || hrs2 != 0.0) { std::printf("the direct-only walk differs\n"); return 1; }
        }
    std::printf("OK\n");
    return 0;
}
