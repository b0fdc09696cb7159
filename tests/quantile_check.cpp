// The quantile rule of csrc/quantile_rule.h in a plain C++ program: the header the kernels are built from is compiled here with
// gcc (no HIP), under AddressSanitizer and UBSan.  It checks the key's packing and order, the bit count that sizes the sort's
// window, the lower-bound bisection, hand-worked quantiles and the rule's stated consequences (p = 0 and 1 are the ends,
// min <= Q <= max, an even n's median is the exact mean of the middle pair); then it runs the rule over planes made by the
// 64-bit congruential generator that tests/test_quantile_host.py restates, through sorted KEYS as the kernels do, and prints
//   case k nrow ncol n_zones quantum_exponent
//   zone z n bits(Q(p)) for p in 0 0.05 1/3 0.5 0.9 1, then the sum of `below` over the zone's cells
// and then OK; the test holds every line against the numpy restatement (tests/quantile_ref.py).
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "quantile_rule.h"

using namespace mhs;

static uint64_t lcg_state;
static uint32_t lcg() {
    lcg_state = lcg_state * 6364136223846793005ULL + 1442695040888963407ULL;
    return (uint32_t)(lcg_state >> 33);
}

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static uint64_t bits(double v) {
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}

struct Vec {
    const std::vector<int32_t> *s;
    int32_t operator()(int64_t i) const { return s->at((size_t)i); }
};
struct Keys {
    const std::vector<uint64_t> *k;
    uint64_t operator()(int64_t i) const { return k->at((size_t)i); }
};
struct Segment {
    const std::vector<uint64_t> *k;
    int64_t start;
    int32_t operator()(int64_t i) const { return quantile_key_q(k->at((size_t)(start + i))); }
};

static double Q(const std::vector<int32_t> &s, double p, double quantum) { return quantile_type7(Vec{&s}, (int64_t)s.size(), p, quantum); }

int main() {
    // the key: packing, unpacking and order
    const int32_t qs[] = {-ZONAL_Q_MAX, -ZONAL_Q_MAX + 1, -1, 0, 1, 65536, ZONAL_Q_MAX - 1, ZONAL_Q_MAX};
    const uint32_t zs[] = {0u, 1u, 255u, 256u, 16777219u, 2147483645u, 2147483646u};
    uint64_t last = 0;
    bool first = true;
    for (uint32_t z : zs)
        for (int32_t q : qs) {
            const uint64_t k = quantile_key(z, q);
            CHECK(quantile_key_q(k) == q && quantile_key_zone(k) == z);
            CHECK(first || k > last);
            CHECK(k < quantile_sentinel(z + 1) && k >= quantile_sentinel(z) && k >> (32 + quantile_bits(z + 1)) == 0);
            last = k;
            first = false;
        }
    CHECK(quantile_bits(0) == 0 && quantile_bits(1) == 1 && quantile_bits(2) == 2 && quantile_bits(3) == 2 && quantile_bits(255) == 8 &&
          quantile_bits(256) == 9 && quantile_bits(2147483647u) == 31);
    CHECK(quantile_prob_ok(0.0) && quantile_prob_ok(1.0) && quantile_prob_ok(0.5) && !quantile_prob_ok(-1e-300) && !quantile_prob_ok(1.0000000000000002) &&
          !quantile_prob_ok(NAN) && !quantile_prob_ok(INFINITY));
    // hand-worked: n = 1, 2, an even n with a .5 median, p at the ends, repeated values
    CHECK(Q({7}, 0.0, 0.5) == 3.5 && Q({7}, 0.5, 0.5) == 3.5 && Q({7}, 1.0, 0.5) == 3.5);
    CHECK(Q({1, 2}, 0.5, 1.0) == 1.5 && Q({1, 2}, 0.0, 1.0) == 1.0 && Q({1, 2}, 1.0, 1.0) == 2.0 && Q({1, 2}, 0.25, 1.0) == 1.25);
    CHECK(Q({1, 2, 4, 9}, 0.5, 1.0) == 3.0 && Q({1, 2, 5, 9}, 0.5, 1.0) == 3.5 && Q({1, 2, 5, 9}, 0.5, 0.25) == 0.875);
    CHECK(Q({1, 2, 3}, 0.5, 1.0) == 2.0 && Q({3, 3, 3, 3}, 0.3, 2.0) == 6.0 && Q({-4, 0, 4, 8, 12}, 0.75, 1.0) == 8.0);
    CHECK(Q({-ZONAL_Q_MAX, ZONAL_Q_MAX}, 0.5, 1.0) == 0.0 && Q({-ZONAL_Q_MAX, ZONAL_Q_MAX}, 1.0, 1.0) == 1073741824.0);
    CHECK(Q({ZONAL_Q_MAX - 1, ZONAL_Q_MAX}, 0.5, 1.0) == 1073741823.5);
    // the bisection
    {
        const std::vector<uint64_t> k = {quantile_key(0, -5), quantile_key(0, -5), quantile_key(0, 3), quantile_key(2, -9), quantile_key(2, 0)};
        const Keys K{&k};
        CHECK(quantile_lower_bound(K, 0, 5, quantile_sentinel(0)) == 0 && quantile_lower_bound(K, 0, 5, quantile_sentinel(1)) == 3);
        CHECK(quantile_lower_bound(K, 0, 5, quantile_sentinel(2)) == 3 && quantile_lower_bound(K, 0, 5, quantile_sentinel(3)) == 5);
        CHECK(quantile_lower_bound(K, 0, 3, quantile_key(0, -5)) == 0 && quantile_lower_bound(K, 0, 3, quantile_key(0, 3)) == 2);
        CHECK(quantile_lower_bound(K, 0, 3, quantile_key(0, 4)) == 3 && quantile_lower_bound(K, 2, 2, 0) == 2);
    }
    CHECK(quantile_frac_below(0, 3) == 0.0 && quantile_frac_below(1, 4) == 0.25 && quantile_frac_below(2, 3) == 2.0 / 3.0);

    // planes by the generator: value = a multiple of 1/4 in -250 .. 250 (or +-(2^30 - 1) quanta, case 3), zone in -1 .. nz - 1
    const int shapes[][3] = {{1, 1, 1}, {5, 7, 3}, {33, 65, 40}, {67, 133, 1}, {67, 133, 9000}};
    const double probs[6] = {0.0, 0.05, 1.0 / 3.0, 0.5, 0.9, 1.0};
    for (int k = 0; k < 5; ++k) {
        const int nrow = shapes[k][0], ncol = shapes[k][1], nz = shapes[k][2];
        const size_t n = (size_t)nrow * ncol;
        lcg_state = 9000 + (uint64_t)k;
        const double quantum = 0.25;
        std::vector<uint64_t> keys, mine(n);
        for (size_t i = 0; i < n; ++i) {
            const uint32_t a = lcg(), b = lcg();
            const double v = k == 3 ? (a % 2 ? 1.0 : -1.0) * (double)(ZONAL_Q_MAX - 1) * 0.25 : ((double)(a % 2001) - 1000.0) * 0.25;
            const int zone = (int)(b % (uint32_t)(nz + 1)) - 1;
            mine[i] = zone >= 0 ? quantile_key((uint32_t)zone, zonal_q(v, quantum)) : quantile_sentinel((uint32_t)nz);
            if (zone >= 0) keys.push_back(mine[i]);
        }
        std::sort(keys.begin(), keys.end());
        const int64_t m = (int64_t)keys.size();
        const Keys K{&keys};
        std::vector<int64_t> below_sum((size_t)nz, 0);
        for (size_t i = 0; i < n; ++i) {
            const uint32_t z = quantile_key_zone(mine[i]);
            if (z == (uint32_t)nz) continue;
            const int64_t a = quantile_lower_bound(K, 0, m, quantile_sentinel(z)), e = quantile_lower_bound(K, 0, m, quantile_sentinel(z + 1));
            below_sum.at(z) += quantile_lower_bound(K, a, e, mine[i]) - a;
        }
        std::printf("case %d %d %d %d %d\n", k, nrow, ncol, nz, -2);
        for (int z = 0; z < nz; ++z) {
            const int64_t a = quantile_lower_bound(K, 0, m, quantile_sentinel((uint32_t)z)), e = quantile_lower_bound(K, 0, m, quantile_sentinel((uint32_t)z + 1));
            const int64_t cnt = e - a;
            std::printf("zone %d %" PRId64, z, cnt);
            const Segment seg{&keys, a};
            double mn = 0, mx = 0;
            for (int j = 0; j < 6; ++j) {
                const double q = cnt ? quantile_type7(seg, cnt, probs[j], quantum) : zonal_nan();
                if (cnt) {
                    if (j == 0) { mn = q; CHECK(q == (double)seg(0) * quantum); }
                    if (j == 5) { mx = q; CHECK(q == (double)seg(cnt - 1) * quantum); }
                    CHECK(q >= (double)seg(0) * quantum && q <= (double)seg(cnt - 1) * quantum);
                }
                std::printf(" %016" PRIx64, bits(q));
            }
            if (cnt) {
                CHECK(mn <= mx);
                // the median: the exact mean of the middle pair (the q are below 2^31, so the sum is exact)
                const double mid = cnt % 2 ? (double)seg(cnt / 2) * quantum : ((double)seg(cnt / 2 - 1) + (double)seg(cnt / 2)) * 0.5 * quantum;
                CHECK(quantile_type7(seg, cnt, 0.5, quantum) == mid);
            }
            std::printf(" %" PRId64 "\n", below_sum[(size_t)z]);
        }
    }
    if (failures) return 1;
    std::printf("OK\n");
    return 0;
}
