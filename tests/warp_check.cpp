// The warp rule of csrc/warp_rule.h in a plain C++ program: the header the kernel is built from is compiled here with gcc (no
// HIP), under AddressSanitizer and UBSan, and prints the table of hand-worked cases that tests/test_project_host.py holds against
// the numpy restatement (tests/warp_ref.py).  One "name value" per line, then OK.  The lattices are vectors of exactly the
// section's node counts, so a node index past the lattice is an AddressSanitizer report.
#include <cmath>
#include <cstdio>
#include <vector>

#include "warp_rule.h"

using namespace mhs;

struct HostAcc {
    const std::vector<double> &z;
    int nrow, ncol;
    bool get(int i, int j, double &v) const {
        if (i < 0 || i >= nrow || j < 0 || j >= ncol) return false;
        v = z[(size_t)i * ncol + j];
        return !rs_na(v, false, 0.0);
    }
};

// nodes sx = x_origin + b x_step, sy = y_origin - a y_step for a target of nrow x ncol cells at step K
struct Lat {
    std::vector<double> sx, sy;
    int K;
    int64_t nr, nc;
    Lat(int nrow, int ncol, int K_, double xo, double xs, double yo, double ys) : K(K_), nr(warp_nodes(nrow, K_)), nc(warp_nodes(ncol, K_)) {
        for (int64_t a = 0; a < nr; ++a)
            for (int64_t b = 0; b < nc; ++b) { sx.push_back(xo + (double)b * xs); sy.push_back(yo - (double)a * ys); }
    }
    WarpLatticeMem mem() const { return WarpLatticeMem{sx.data(), sy.data(), nc}; }
};

static void line(const char *name, double v) { std::printf("%s %.17g\n", name, v); }

static double cell(const HostAcc &a, const RsGrid &S, const Lat &l, int method, int r, int c) {
    double v;
    return warp_cell(a, S, l.mem(), l.K, method, r, c, v) ? v : NAN;
}

int main() {
    // the source: 3 x 3, unit cells, north-west corner (0, 3)
    const RsGrid S3{0.0, 3.0, 1.0, 1.0, 3, 3};
    std::vector<double> z3{1, 2, 3, 4, 5, 6, 7, 8, 10};
    const HostAcc a3{z3, 3, 3};
    double sx, sy;
    // K = 1: a 2 x 2 target, 3 x 3 nodes sx = 1.25, 2.25, 3.25 and sy = 1.75, 0.75, -0.25
    const Lat l1(2, 2, 1, 1.25, 1.0, 1.75, 1.0);
    line("k1_nodes", (double)(l1.nr * 10 + l1.nc));
    line("k1_ok_00", warp_source_point(l1.mem(), 1, 0, 0, sx, sy) ? 1.0 : 0.0);
    line("k1_sx_00", sx); line("k1_sy_00", sy);
    line("k1_bilinear_00", cell(a3, S3, l1, RS_BILINEAR, 0, 0));
    line("k1_cubic_00", cell(a3, S3, l1, RS_CUBIC, 0, 0));
    line("k1_near_00", cell(a3, S3, l1, RS_NEAR, 0, 0));
    line("k1_near_11", cell(a3, S3, l1, RS_NEAR, 1, 1));
    line("k1_bilinear_11", cell(a3, S3, l1, RS_BILINEAR, 1, 1));
    // K = 4: a 6 x 5 target, 3 x 3 nodes sx = 0.5, 2.5, 4.5 and sy = 3, 1, -1; rows 4 .. 5 and column 4 are the last, partial lattice cell
    const Lat l4(6, 5, 4, 0.5, 2.0, 3.0, 2.0);
    line("k4_nodes", (double)(l4.nr * 10 + l4.nc));
    line("k4_tu_c1", warp_frac(1, 4).t); line("k4_tv_r5", warp_frac(5, 4).t); line("k4_node_r5", warp_frac(5, 4).node);
    warp_source_point(l4.mem(), 4, 2, 1, sx, sy);
    line("k4_sx_21", sx); line("k4_sy_21", sy);
    line("k4_bilinear_21", cell(a3, S3, l4, RS_BILINEAR, 2, 1));
    warp_source_point(l4.mem(), 4, 5, 4, sx, sy);
    line("k4_last_sx", sx); line("k4_last_sy", sy);
    line("k4_last_near", cell(a3, S3, l4, RS_NEAR, 5, 4));
    line("k4_last_bilinear", cell(a3, S3, l4, RS_BILINEAR, 5, 4));
    // a node that is not finite makes NA of the cells of the lattice cells that read it, and of no other
    Lat lnan = l4;
    lnan.sx[2 * 3 + 2] = NAN;                        // node (2, 2): only the lattice cell a = 1, b = 1 reads it
    line("nan_node_is_na", std::isnan(cell(a3, S3, lnan, RS_BILINEAR, 5, 4)) && std::isnan(cell(a3, S3, lnan, RS_NEAR, 4, 4)) ? 1.0 : 0.0);
    line("nan_node_elsewhere", cell(a3, S3, lnan, RS_BILINEAR, 2, 1));
    Lat linf = l4;
    linf.sy[0] = INFINITY;                           // node (0, 0)
    line("inf_node_is_na", std::isnan(cell(a3, S3, linf, RS_BILINEAR, 2, 1)) ? 1.0 : 0.0);
    line("inf_node_elsewhere", cell(a3, S3, linf, RS_NEAR, 5, 4));
    // node counts and steps
    line("nodes_8_by_4", (double)warp_nodes(8, 4)); line("nodes_9_by_4", (double)warp_nodes(9, 4)); line("nodes_1_by_1024", (double)warp_nodes(1, 1024));
    line("steps", warp_step_ok(1) && warp_step_ok(64) && warp_step_ok(1024) && !warp_step_ok(0) && !warp_step_ok(3) && !warp_step_ok(2048) && !warp_step_ok(-4) ? 1.0 : 0.0);
    // every cell of both targets is read without leaving the lattice (the sanitizer's part)
    double sum = 0.0;
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 5; ++c) { const double v = cell(a3, S3, l4, RS_CUBIC, r, c); sum += std::isnan(v) ? 0.0 : 1.0; }
    line("k4_cells_with_a_value", sum);
    std::printf("OK\n");
    return 0;
}
