// Stand-alone check of csrc/rasterize_rule.h, compiled by tests/test_rasterize_host.py with the host sanitizers and run on its
// own: the two counts of the centre rule (floor, two confirming comparisons, a bisection where they fail) against brute-force
// counts over the cells, at coordinates on, just below and just above cell centres and edges, with huge and tiny cells, cell
// centres that collide in float64, and coordinates far outside the grid; the rows an edge crosses against the rule's own
// sentence; and that no crossing or line span of a feature leaves the box the host plans its bit plane by.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rasterize_rule.h"

using namespace mhs;

static long n_checked = 0;
static int fail(const char *what, const RzGrid &g, double v, long got, long want) {
    std::printf("FAIL %s: grid (%.17g %.17g %.17g %.17g %d %d) at %.17g: %ld, brute force %ld\n", what, g.xmin, g.ymax, g.xres, g.yres, g.nrow, g.ncol, v,
                got, want);
    return 1;
}

static int check_counts(const RzGrid &g, double x, double y) {
    long cs = 0, ra = 0;
    for (int c = 0; c < g.ncol; ++c) cs += rz_xc(g, c) < x;
    for (int r = 0; r < g.nrow; ++r) ra += rz_yr(g, r) >= y;
    if (rz_cstar(g, x) != cs) return fail("cstar", g, x, rz_cstar(g, x), cs);
    if (rz_rabove(g, y) != ra) return fail("rabove", g, y, rz_rabove(g, y), ra);
    n_checked += 2;
    return 0;
}

// the probes around one coordinate
static std::vector<double> around(double v) {
    const double inf = INFINITY;
    return {v, std::nextafter(v, -inf), std::nextafter(v, inf), std::nextafter(std::nextafter(v, -inf), -inf), std::nextafter(std::nextafter(v, inf), inf)};
}

static unsigned long long lcg = 12345;
static double uniform() {
    lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(lcg >> 11) / 9007199254740992.0;
}

static int check_grid(const RzGrid &g) {
    // centres, edges and their neighbours in float64
    for (int c = -2; c <= g.ncol + 2; ++c)
        for (double base : {g.xmin + ((double)c + 0.5) * g.xres, g.xmin + (double)c * g.xres})
            for (double x : around(base))
                for (int r = -2; r <= g.nrow + 2; r += (g.nrow > 40 ? 7 : 1))
                    for (double y : around(r & 1 ? g.ymax - ((double)r + 0.5) * g.yres : g.ymax - (double)r * g.yres))
                        if (check_counts(g, x, y)) return 1;
    // far outside
    for (double far : {1e300, -1e300, 1.7e308, -1.7e308, 0.0, 1e-300})
        if (check_counts(g, far, far)) return 1;
    // edges: the rows crossed are those with (y0 <= y_r) != (y1 <= y_r); every crossing and every span stays in the box
    const double w = (double)g.ncol * g.xres, h = (double)g.nrow * g.yres;
    for (int k = 0; k < 400; ++k) {
        double x0 = g.xmin + (uniform() * 1.6 - 0.3) * w, x1 = g.xmin + (uniform() * 1.6 - 0.3) * w;
        double y0 = g.ymax - (uniform() * 1.6 - 0.3) * h, y1 = g.ymax - (uniform() * 1.6 - 0.3) * h;
        if (k % 7 == 0) y1 = y0;                                               // horizontal
        if (k % 11 == 0) x1 = x0;                                              // vertical
        if (k % 13 == 0) y0 = rz_yr(g, (int)(uniform() * g.nrow));             // an endpoint on a row of centres
        const RzSeg s = rz_seg(x0, y0, x1, y1);
        int first;
        const int n = rz_cross_rows(g, s, &first);
        long brute = 0;
        for (int r = 0; r < g.nrow; ++r) {
            const bool crosses = (y0 <= rz_yr(g, r)) != (y1 <= rz_yr(g, r));
            brute += crosses;
            if (crosses != (r >= first && r < first + n)) return fail("cross_rows", g, y0, first, r);
        }
        if (brute != n) return fail("cross_rows count", g, y0, n, brute);
        RzBox b;
        const bool in = rz_box(g, std::fmin(x0, x1), std::fmax(x0, x1), std::fmin(y0, y1), std::fmax(y0, y1), &b);
        for (int r = first; r < first + n; ++r) {
            const double X = rz_X(s, rz_yr(g, r));
            if (X < std::fmin(x0, x1) || X > std::fmax(x0, x1)) return fail("X leaves the segment", g, X, r, 0);
            // the cells this crossing toggles that can end up covered lie between the box's columns
            if (in && (r < b.r0 || r >= b.r0 + b.h)) return fail("crossing row outside the box", g, X, r, b.r0);
            if (!in && n > 0 && rz_cstar(g, std::fmin(x0, x1)) < rz_cstar(g, std::fmax(x0, x1))) return fail("empty box with a cover", g, X, r, 0);
        }
        int lfirst;
        const int ln = rz_line_rows(g, s, &lfirst);
        for (int r = lfirst; r < lfirst + ln; ++r) {
            int c_lo, c_hi;
            if (r < 0 || r >= g.nrow) return fail("line row outside the grid", g, y0, r, 0);
            if (!rz_line_span(g, s, r, &c_lo, &c_hi)) continue;
            if (c_lo < 0 || c_hi >= g.ncol) return fail("span outside the grid", g, x0, c_lo, c_hi);
            if (!in || r < b.r0 || r >= b.r0 + b.h || c_lo < b.c0 || c_hi >= b.c0 + b.w) return fail("span outside the box", g, x0, c_lo, c_hi);
        }
        n_checked += 1;
    }
    return 0;
}

int main() {
    const RzGrid grids[] = {
        {100.0, 900.0, 1.5, 2.0, 67, 133},                   // the tests' grid
        {0.0, 1.0, 1.0, 1.0, 1, 1},
        {-78.0, -5.0, 1.0 / 1200, 1.0 / 1200, 96, 128},      // lon/lat, 30 arc seconds
        {500000.0, 5000000.0, 30.0, 30.0, 45, 77},           // UTM
        {0.0, 0.0, 1e150, 1e150, 20, 30},                    // huge cells
        {0.0, 0.0, 1e-150, 1e-150, 20, 30},                  // tiny cells
        {-1e300, 1e300, 1e298, 1e298, 50, 60},               // at the edge of the range
        {5e6, 5e6, 1e-9, 1e-9, 40, 50},                      // centres that collide: the cell is a fraction of an ulp of xmin
        {1e16, 1e16, 1.0, 1.0, 30, 30},                      // an ulp of two cells
        {0.1, 0.7, 0.1, 0.1, 33, 65},                        // cell sizes that are not dyadic
    };
    for (const RzGrid &g : grids)
        if (check_grid(g)) return 1;
    // the point rule: the east edge belongs to the last column, the south edge to the last row, beyond them is outside
    const RzGrid g = grids[0];
    int r, c;
    const double xmax = g.xmin + g.ncol * g.xres, ymin = g.ymax - g.nrow * g.yres;
    if (!rz_point_cell(g, xmax, ymin, &r, &c) || r != g.nrow - 1 || c != g.ncol - 1) return fail("point on the south-east corner", g, xmax, r, c);
    if (!rz_point_cell(g, g.xmin, g.ymax, &r, &c) || r != 0 || c != 0) return fail("point on the north-west corner", g, g.xmin, r, c);
    if (rz_point_cell(g, std::nextafter(xmax, INFINITY), ymin, &r, &c) || rz_point_cell(g, g.xmin, std::nextafter(g.ymax, INFINITY), &r, &c) ||
        rz_point_cell(g, std::nextafter(g.xmin, -INFINITY), ymin, &r, &c) || rz_point_cell(g, xmax, std::nextafter(ymin, -INFINITY), &r, &c))
        return fail("point outside", g, xmax, 0, 0);
    std::printf("checked %ld\nOK\n", n_checked);
    return 0;
}
