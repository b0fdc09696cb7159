// The proximity rule of csrc/proximity_rule.h in a plain C++ program: the header the kernels are built from is compiled here
// with gcc (no HIP), under AddressSanitizer and UBSan, and drives the HOST side of the rule -- the predicate, the floor-division
// separator with negative numerators, the envelope build and query, the product formulas -- over small grids made by a
// 64-bit congruential generator that tests/test_proximity_host.py restates.  It prints
//   floor_div a b q          for a table of numerators and divisors
//   takeover i hi u hu w     for a table of row pairs
//   compare count            how often w > f and n >= f d agree at the seven f around each of those w (all 70 times)
//   case k nrow ncol where checksum     one line per grid: the sum over the six planes' cells of bits * (2 i + 1) mod 2^64
// and then OK; the test holds every line against the numpy restatement (tests/proximity_ref.py).
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "proximity_rule.h"

using namespace mhs;

static uint64_t lcg_state;
static uint32_t lcg() {
    lcg_state = lcg_state * 6364136223846793005ULL + 1442695040888963407ULL;
    return (uint32_t)(lcg_state >> 33);
}

struct HostStack {
    const std::vector<int> &near;
    std::vector<int> &srow, &sfrom;
    int col, ncol;
    int row(int k) const { return srow.at((size_t)k * ncol + col); }
    int from(int k) const { return sfrom.at((size_t)k * ncol + col); }
    int64_t h(int, int r) const {
        const int64_t d = (int64_t)col - near.at((size_t)r * ncol + col);
        return d * d;
    }
    void set(int k, int r, int f, int64_t) {
        srow.at((size_t)k * ncol + col) = r;
        sfrom.at((size_t)k * ncol + col) = f;
    }
};

static uint64_t bits(double v) {
    if (v != v) return 0x7ff8000000000000ULL;            // one NaN
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}

int main() {
    const int64_t num[] = {-7, -6, -1, 0, 1, 6, 7, -2147483647LL * 2, 4294967295LL, -4294967295LL};
    const int64_t den[] = {2, 3, 4, 92000};
    for (int64_t a : num)
        for (int64_t b : den) std::printf("floor_div %" PRId64 " %" PRId64 " %" PRId64 "\n", a, b, prox_floor_div(a, b));
    const int64_t pairs[][4] = {{0, 0, 1, 0}, {0, 0, 2, 0}, {0, 9, 1, 0}, {0, 0, 1, 9}, {3, 4, 7, 4}, {3, 100, 4, 0}, {3, 0, 4, 100},
                                {0, 2115908001LL, 45999, 0}, {0, 0, 45999, 2115908001LL}, {10, 25, 12, 16}};
    for (const auto &p : pairs)
        std::printf("takeover %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", p[0], p[1], p[2], p[3], prox_takeover(p[0], p[1], p[2], p[3]));
    // the comparison prox_env_add makes instead of dividing:  w > f  <=>  n >= f d
    int64_t agree = 0;
    for (const auto &p : pairs) {
        const ProxSep s = prox_sep(p[0], p[1], p[2], p[3]);
        const int64_t w = prox_takeover(p[0], p[1], p[2], p[3]);
        for (int64_t f = w - 3; f <= w + 3; ++f) agree += (w > f) == (s.n >= f * s.d);
    }
    std::printf("compare %" PRId64 "\n", agree);

    const int shapes[][2] = {{1, 1}, {1, 9}, {9, 1}, {3, 17}, {17, 5}, {24, 24}, {13, 20}, {20, 13}};
    const double unit = 2.5, threshold = 2.0;
    int k = 0;
    for (const auto &sh : shapes) {
        for (int where = 0; where < PROX_WHERES; ++where, ++k) {
            const int nrow = sh[0], ncol = sh[1];
            lcg_state = 1000 + (uint64_t)k;
            std::vector<double> z((size_t)nrow * ncol);
            for (double &v : z) {
                const uint32_t q = lcg() % 23;                   // mostly 3: few features for LT / GT / NA, many for the others
                v = q == 0 ? NAN : q == 1 ? -9.0 : q < 4 ? (double)(q - 1) : 3.0;   // -9 is the nodata value
            }
            // A
            std::vector<int> near((size_t)nrow * ncol);
            for (int r = 0; r < nrow; ++r) {
                std::vector<int> left(ncol);
                int last = -1;
                for (int c = 0; c < ncol; ++c) {
                    if (prox_is_feature(z[(size_t)r * ncol + c], true, -9.0, where, threshold)) last = c;
                    left[c] = last;
                }
                last = -1;
                for (int c = ncol - 1; c >= 0; --c) {
                    if (prox_is_feature(z[(size_t)r * ncol + c], true, -9.0, where, threshold)) last = c;
                    near[(size_t)r * ncol + c] = prox_nearer_in_row(c, left[c], last);
                }
            }
            // B1
            std::vector<int> srow((size_t)nrow * ncol, -1), sfrom((size_t)nrow * ncol, -1), height(ncol);
            for (int c = 0; c < ncol; ++c) {
                HostStack s{near, srow, sfrom, c, ncol};
                ProxEnv e;
                for (int r = 0; r < nrow; ++r) {
                    const int fc = near[(size_t)r * ncol + c];
                    if (fc < 0) continue;
                    const int64_t d = (int64_t)c - fc;
                    prox_env_add(s, e, r, d * d, nrow);
                }
                height[c] = e.k;
            }
            // B2
            uint64_t sum = 0, i = 0;
            for (int r = 0; r < nrow; ++r)
                for (int c = 0; c < ncol; ++c) {
                    const HostStack s{near, srow, sfrom, c, ncol};
                    int fr = -1, fc = -1;
                    if (height[c] > 0) {
                        fr = s.row(prox_segment(s, height[c], r));
                        fc = near[(size_t)fr * ncol + c];
                    }
                    const int64_t d2 = fr < 0 ? -1 : prox_d2(r, c, fr, fc), index = fr < 0 ? -1 : prox_index(fr, fc, ncol);
                    const ProxFloat f = prox_float(r, c, fr, fc, unit);
                    double v = NAN;
                    if (fr >= 0) {
                        v = z[(size_t)fr * ncol + fc];
                        if (prox_na(v, true, -9.0)) v = NAN;
                    }
                    const uint64_t x[6] = {(uint64_t)d2, (uint64_t)index, bits(f.dist), bits(f.dir_x), bits(f.dir_y), bits(v)};
                    for (uint64_t b : x) { sum += b * (2 * i + 1); ++i; }
                }
            std::printf("case %d %d %d %d %" PRIu64 "\n", k, nrow, ncol, where, sum);
        }
    }
    std::printf("OK\n");
    return 0;
}
