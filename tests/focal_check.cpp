// The focal rule of csrc/focal_rule.h in a plain C++ program: the header the kernels are built from is compiled here with gcc (no
// HIP), under AddressSanitizer and UBSan.  It makes a 70 x 150 plane from a 64-bit congruential generator (full mantissas, NA
// cells, an all-NA row), runs the rule as plain loops -- blocked prefixes along the rows, row-window sums, blocked prefixes down the
// columns or the circle's row-by-row sum, the statistics -- and prints every plane as the bit patterns of its doubles, which
// tests/test_focal_host.py holds against the numpy restatement (tests/focal_ref.py) made on the same plane.  The arrays are vectors
// of exactly the plane's size, so an index past a row, a column or the half-width table is an AddressSanitizer report.
//   line:  <shape> <R> <fill_na> <statistic> <nrow * ncol hexadecimal words>      then OK
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "focal_rule.h"

using namespace mhs;

static const int NR = 70, NC = 150;
static const double OFFSET = 1500.0;

// the running minimum of focal_rule.h over host vectors: channel values x (+inf at NA cells), one axis
struct VecAcc {
    const std::vector<double> &x, &pm_, &sm_;
    const std::vector<std::vector<double>> &tab;
    size_t at, stride;
    double pm(int64_t i) const { return pm_.at(at + (size_t)i * stride); }
    double sm(int64_t i) const { return sm_.at(at + (size_t)i * stride); }
    double raw(int64_t i) const { return x.at(at + (size_t)i * stride); }
    double table(int j, int64_t k) const { return tab.at((size_t)j).at((size_t)k); }
};

// the minimum of x[i - R .. i + R] cut to the n elements at `at`, `stride` apart, for every i, into out
static void axis_min(const std::vector<double> &x, size_t at, size_t stride, int n, int R, std::vector<double> &out) {
    std::vector<double> pm(x.size(), 0.0), sm(x.size(), 0.0);
    const int nb = (n + FOCAL_B - 1) / FOCAL_B;
    std::vector<std::vector<double>> tab((size_t)focal_levels(nb), std::vector<double>((size_t)nb, INFINITY));
    for (int k = 0; k < nb; ++k) {
        const int lo = k * FOCAL_B, hi = lo + FOCAL_B < n ? lo + FOCAL_B : n;
        double m = INFINITY;
        for (int i = lo; i < hi; ++i) { const double v = x[at + (size_t)i * stride]; m = v < m ? v : m; pm[at + (size_t)i * stride] = m; }
        tab[0][(size_t)k] = m;
        m = INFINITY;
        for (int i = hi - 1; i >= lo; --i) { const double v = x[at + (size_t)i * stride]; m = v < m ? v : m; sm[at + (size_t)i * stride] = m; }
    }
    for (size_t j = 1; j < tab.size(); ++j)
        for (int k = 0; k < nb; ++k) {
            const int half = 1 << (j - 1);
            double a = tab[j - 1][(size_t)k];
            if (k + half < nb && tab[j - 1][(size_t)(k + half)] < a) a = tab[j - 1][(size_t)(k + half)];
            tab[j][(size_t)k] = a;
        }
    const VecAcc acc{x, pm, sm, tab, at, stride};
    for (int i = 0; i < n; ++i)
        out[at + (size_t)i * stride] = focal_range_min(acc, n, i - R > 0 ? i - R : 0, i + R < n - 1 ? i + R : n - 1);
}

static void min_max(const std::vector<double> &z, const std::vector<int64_t> &f, int R, std::vector<double> &mn, std::vector<double> &mx) {
    for (int ch = 0; ch < 2; ++ch) {
        std::vector<double> x(z.size()), rm(z.size()), cm(z.size());
        for (size_t i = 0; i < z.size(); ++i) x[i] = f[i] ? (ch ? -z[i] : z[i]) : INFINITY;
        for (int r = 0; r < NR; ++r) axis_min(x, (size_t)r * NC, 1, NC, R, rm);
        for (int c = 0; c < NC; ++c) axis_min(rm, (size_t)c, NC, NR, R, cm);
        for (size_t i = 0; i < z.size(); ++i) (ch ? mx : mn)[i] = ch ? -cm[i] : cm[i];
    }
}

int main() {
    std::vector<double> z((size_t)NR * NC);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (size_t i = 0; i < z.size(); ++i) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        z[i] = 1200.0 + (double)(x >> 11) * (600.0 / 9007199254740992.0);
        if (i % 17 == 3 || i / NC == 5) z[i] = NAN;
    }
    z[40 * NC + 7] = -9999.0;                                    // the nodata value
    std::vector<double> a(z.size()), b(z.size()), P1(z.size()), P2(z.size());
    std::vector<int64_t> f(z.size()), Pn(z.size());
    for (size_t i = 0; i < z.size(); ++i) {
        const bool na = focal_na(z[i], true, -9999.0);
        const double zc = z[i] - OFFSET;
        a[i] = na ? 0.0 : zc; b[i] = na ? 0.0 : zc * zc; f[i] = na ? 0 : 1;
    }
    for (int r = 0; r < NR; ++r) {
        focal_blocked_prefix(a.data() + (size_t)r * NC, NC, 1, P1.data() + (size_t)r * NC);
        focal_blocked_prefix(b.data() + (size_t)r * NC, NC, 1, P2.data() + (size_t)r * NC);
        focal_blocked_prefix(f.data() + (size_t)r * NC, NC, 1, Pn.data() + (size_t)r * NC);
    }
    auto row_lo = [](int c, int w) { return c - w > 0 ? c - w : 0; };
    auto row_hi = [](int c, int w) { return c + w < NC - 1 ? c + w : NC - 1; };
    const int cases[5][2] = {{FOCAL_SQUARE, 1}, {FOCAL_SQUARE, 64}, {FOCAL_SQUARE, 65}, {FOCAL_CIRCLE, 3}, {FOCAL_CIRCLE, 66}};
    const char *names[FS_NSTATS] = {"count", "sum", "mean", "sd", "min", "max", "range", "minus_mean", "above_min", "below_max", "dev"};
    for (const auto &cs : cases) {
        const int shape = cs[0], R = cs[1];
        std::vector<double> S1(z.size()), S2(z.size());
        std::vector<int64_t> Sn(z.size());
        std::vector<double> mn(z.size(), 0.0), mx(z.size(), 0.0);
        if (shape == FOCAL_SQUARE) {
            min_max(z, f, R, mn, mx);
            std::vector<double> W1(z.size()), W2(z.size()), Q1(z.size()), Q2(z.size());
            std::vector<int64_t> Wn(z.size()), Qn(z.size());
            for (int r = 0; r < NR; ++r)
                for (int c = 0; c < NC; ++c) {
                    const size_t i = (size_t)r * NC + c;
                    W1[i] = focal_window_sum(P1.data() + (size_t)r * NC, 1, row_lo(c, R), row_hi(c, R));
                    W2[i] = focal_window_sum(P2.data() + (size_t)r * NC, 1, row_lo(c, R), row_hi(c, R));
                    Wn[i] = focal_window_sum(Pn.data() + (size_t)r * NC, 1, row_lo(c, R), row_hi(c, R));
                }
            for (int c = 0; c < NC; ++c) {
                focal_blocked_prefix(W1.data() + c, NR, NC, Q1.data() + c);
                focal_blocked_prefix(W2.data() + c, NR, NC, Q2.data() + c);
                focal_blocked_prefix(Wn.data() + c, NR, NC, Qn.data() + c);
            }
            for (int r = 0; r < NR; ++r)
                for (int c = 0; c < NC; ++c) {
                    const int lo = r - R > 0 ? r - R : 0, hi = r + R < NR - 1 ? r + R : NR - 1;
                    const size_t i = (size_t)r * NC + c;
                    S1[i] = focal_window_sum(Q1.data() + c, NC, lo, hi);
                    S2[i] = focal_window_sum(Q2.data() + c, NC, lo, hi);
                    Sn[i] = focal_window_sum(Qn.data() + c, NC, lo, hi);
                }
        } else {
            std::vector<int> hw((size_t)(R < NR - 1 ? R : NR - 1) + 1);
            for (size_t d = 0; d < hw.size(); ++d) hw[d] = focal_half_width(R, (int)d);
            for (int r = 0; r < NR; ++r)
                for (int c = 0; c < NC; ++c) {
                    double s1 = 0.0, s2 = 0.0;
                    int64_t n = 0;
                    for (int dr = -R; dr <= R; ++dr) {
                        const int rr = r + dr;
                        if (rr < 0 || rr >= NR) continue;
                        const int w = hw[(size_t)(dr < 0 ? -dr : dr)];
                        s1 = s1 + focal_window_sum(P1.data() + (size_t)rr * NC, 1, row_lo(c, w), row_hi(c, w));
                        s2 = s2 + focal_window_sum(P2.data() + (size_t)rr * NC, 1, row_lo(c, w), row_hi(c, w));
                        n += focal_window_sum(Pn.data() + (size_t)rr * NC, 1, row_lo(c, w), row_hi(c, w));
                    }
                    const size_t i = (size_t)r * NC + c;
                    S1[i] = s1; S2[i] = s2; Sn[i] = n;
                }
        }
        for (int fill = 0; fill < 2; ++fill)
            for (int k = 0; k < FS_NSTATS; ++k) {
                if (!(FS_SUM_FAMILY >> k & 1u) && shape != FOCAL_SQUARE) continue;
                std::printf("%s %d %d %s", shape == FOCAL_SQUARE ? "square" : "circle", R, fill, names[k]);
                for (size_t i = 0; i < z.size(); ++i) {
                    const bool has_e = f[i] != 0;
                    double o[FS_NSTATS];
                    for (double &v : o) v = NAN;
                    if (has_e || fill) focal_stats(shape == FOCAL_SQUARE ? (1u << FS_NSTATS) - 1 : FS_SUM_FAMILY, Sn[i], S1[i], S2[i], OFFSET, has_e, z[i], mn[i], mx[i], o);
                    const double v = !has_e && (FS_NEEDS_CENTRE >> k & 1u) ? NAN : o[k];
                    uint64_t bits;
                    std::memcpy(&bits, &v, sizeof bits);
                    std::printf(" %" PRIx64, bits);
                }
                std::printf("\n");
            }
    }
    std::printf("OK\n");
    return 0;
}
