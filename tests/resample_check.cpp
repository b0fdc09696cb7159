// The resampling rules of csrc/resample_rule.h in a plain C++ program: the header the kernels are built from is compiled here
// with gcc (no HIP), under AddressSanitizer and UBSan, and prints the table of hand-computed cases that
// tests/test_resample_host.py holds against the numpy restatement (tests/resample_ref.py).  One "name value" per line, then OK.
#include <cmath>
#include <cstdio>
#include <vector>

#include "resample_rule.h"

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

static void line(const char *name, double v) { std::printf("%s %.17g\n", name, v); }

static double at(const HostAcc &a, const RsGrid &S, int method, double x, double y) {
    double v;
    return rs_interp(a, S, method, x, y, v) ? v : NAN;
}

int main() {
    // 3 x 3, unit cells, north-west corner (0, 3)
    const RsGrid S3{0.0, 3.0, 1.0, 1.0, 3, 3};
    std::vector<double> z3{1, 2, 3, 4, 5, 6, 7, 8, 10};
    const HostAcc a3{z3, 3, 3};
    line("bilinear_quarter", at(a3, S3, RS_BILINEAR, 1.75, 1.25));
    line("cubic_fallback", at(a3, S3, RS_CUBIC, 1.75, 1.25));
    line("near_quarter", at(a3, S3, RS_NEAR, 1.75, 1.25));
    line("near_east_edge", at(a3, S3, RS_NEAR, 3.0, 1.5));
    line("near_south_edge", at(a3, S3, RS_NEAR, 0.5, 0.0));
    line("outside_is_na", std::isnan(at(a3, S3, RS_BILINEAR, 3.0000001, 1.5)) && std::isnan(at(a3, S3, RS_NEAR, 1.0, -0.1)) ? 1.0 : 0.0);
    std::vector<double> z3na = z3;
    z3na[5] = NAN;                                   // cell (1, 2)
    const HostAcc a3na{z3na, 3, 3};
    line("bilinear_na_tap", at(a3na, S3, RS_BILINEAR, 1.75, 1.25));
    line("bilinear_na_weight0", at(a3na, S3, RS_BILINEAR, 1.5, 1.5));
    // 4 x 4, every row 0 1 4 9
    const RsGrid S4{0.0, 4.0, 1.0, 1.0, 4, 4};
    std::vector<double> z4;
    for (int i = 0; i < 4; ++i) for (double v : {0.0, 1.0, 4.0, 9.0}) z4.push_back(v);
    const HostAcc a4{z4, 4, 4};
    double w[4];
    rs_cubic_weights(0.5, w);
    line("cubic_w0", w[0]); line("cubic_w1", w[1]); line("cubic_w2", w[2]); line("cubic_w3", w[3]);
    line("cubic_half", at(a4, S4, RS_CUBIC, 2.0, 2.0));
    line("bilinear_half", at(a4, S4, RS_BILINEAR, 2.0, 2.0));
    // footprints of 10 source columns under 3 target columns of the same extent
    const RsGrid S10{0.0, 1.0, 1.0, 1.0, 1, 10}, T3{0.0, 1.0, 10.0 / 3.0, 1.0, 1, 3};
    line("foot_0", rs_foot_col(S10, T3, 0)); line("foot_1", rs_foot_col(S10, T3, 1));
    line("foot_2", rs_foot_col(S10, T3, 2)); line("foot_3", rs_foot_col(S10, T3, 3));
    // the 3 x 3 plane with its NA under one target cell
    const RsGrid T1{0.0, 3.0, 3.0, 3.0, 1, 1};
    const char *names[] = {"agg_mean", "agg_min", "agg_max", "agg_sum", "agg_count"};
    for (int m = RS_MEAN; m <= RS_COUNT_CELLS; ++m) {
        double v;
        line(names[m - RS_MEAN], rs_aggregate(a3na, S3, T1, m, 0, 0, v) ? v : NAN);
    }
    // a target finer than the source: the footprint of a cell that holds no source centre is empty
    const RsGrid Tf{0.0, 3.0, 0.25, 0.25, 12, 12};
    double v;
    line("agg_empty_mean_is_na", rs_aggregate(a3, S3, Tf, RS_MEAN, 0, 0, v) ? 0.0 : 1.0);
    line("agg_empty_count", rs_aggregate(a3, S3, Tf, RS_COUNT_CELLS, 0, 0, v) ? v : NAN);
    line("agg_fine_hit", rs_aggregate(a3, S3, Tf, RS_MEAN, 6, 6, v) ? v : NAN);      // holds the centre (1.5, 1.5) of cell (1, 1)
    // the same grid: every method but SUM and COUNT returns the source
    int same = 1;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const double want = z3[(size_t)r * 3 + c];
            for (int m = RS_NEAR; m <= RS_CUBIC; ++m) same &= at(a3, S3, m, rs_cell_x(S3, c), rs_cell_y(S3, r)) == want;
            for (int m = RS_MEAN; m <= RS_MAX; ++m) same &= rs_aggregate(a3, S3, S3, m, r, c, v) && v == want;
            same &= rs_aggregate(a3, S3, S3, RS_COUNT_CELLS, r, c, v) && v == 1.0;
        }
    line("identity", same);
    std::printf("OK\n");
    return 0;
}
