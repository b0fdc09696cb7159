// The zonal rule of csrc/zonal_rule.h in a plain C++ program: the header the kernels are built from is compiled here with gcc
// (no HIP), under AddressSanitizer and UBSan.  It checks the two-word S2 and the 128-bit step against __int128 on extreme
// inputs, the quantum rules and the rounding of q, and that the accumulators do not depend on the order of addition; then it
// runs the rule over planes made by a 64-bit congruential generator that tests/test_zonal_host.py restates, and prints
//   case k nrow ncol n_zones quantum_exponent
//   zone z cells n bits(sum) bits(mean) bits(sd) bits(min) bits(max)      one line per zone, the doubles as hex words
// and then OK; the test holds every line against the numpy and Python-int restatement (tests/zonal_ref.py).
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zonal_rule.h"

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

static void add(ZonalAcc &a, int32_t q) {
    ++a.n;
    a.S1 += q;
    a.L += zonal_sq_lo(q);
    a.H += zonal_sq_hi(q);
    if (q < a.qmin) a.qmin = q;
    if (q > a.qmax) a.qmax = q;
}

int main() {
    typedef __int128 i128;
    // the two words against one 128-bit sum: n cells of the same extreme q, n up to 2^31 - 1 (the words are sums, so n * word)
    const int32_t extremes[] = {ZONAL_Q_MAX, -ZONAL_Q_MAX, ZONAL_Q_MAX - 1, 1 - ZONAL_Q_MAX, 65536, 65535, -65537, 1, 0, -1, 46341, 0x3fff0001};
    const uint64_t counts[] = {1, 2, 3, 8911, 65536, 2147483647ull};
    for (int32_t q : extremes)
        for (uint64_t n : counts) {
            const uint64_t L = n * zonal_sq_lo(q), H = n * zonal_sq_hi(q);
            CHECK(zonal_sq_lo(q) < (1ull << 32) && zonal_sq_hi(q) <= (1ull << 28));
            const zonal_u128 want = (zonal_u128)n * (zonal_u128)((i128)q * q);
            CHECK(zonal_s2(H, L) == want);
            // all cells equal: the variance numerator is exactly zero, whatever its 120 bits were made of
            CHECK(zonal_var_num(n, (int64_t)n * q, H, L) == 0);
            if (n >= 2) {
                ZonalAcc a{(uint32_t)n, (uint32_t)n, (int64_t)n * q, L, H, q, q};
                CHECK(zonal_sd(a, 0.25) == 0.0);
                CHECK(zonal_mean(a, 0.25) == (double)q * 0.25 && zonal_min(a, 0.25) == zonal_max(a, 0.25));
            }
        }
    // half the cells at +Q, half at -Q + 1: the widest numerator; against signed 128-bit arithmetic
    for (uint64_t half : {1ull, 4455ull, 1073741823ull}) {
        const int32_t p = ZONAL_Q_MAX, m = 1 - ZONAL_Q_MAX;
        const uint64_t n = 2 * half;
        const uint64_t L = half * zonal_sq_lo(p) + half * zonal_sq_lo(m), H = half * zonal_sq_hi(p) + half * zonal_sq_hi(m);
        const int64_t S1 = (int64_t)half * p + (int64_t)half * m;
        const i128 S2 = (i128)half * ((i128)p * p) + (i128)half * ((i128)m * m);
        const i128 want = (i128)n * S2 - (i128)S1 * S1;
        CHECK(want > 0 && zonal_var_num(n, S1, H, L) == (zonal_u128)want);
        CHECK(zonal_var_num(n, -S1, H, L) == (zonal_u128)want);
    }
    // D: exact below 2^53, and the two halves are combined
    CHECK(zonal_D(0) == 0.0 && zonal_D(12345) == 12345.0 && zonal_D((zonal_u128)1 << 64) == 18446744073709551616.0);
    CHECK(zonal_D(((zonal_u128)3 << 100) + 5) == std::ldexp(3.0, 100) && zonal_D(((zonal_u128)1 << 122) + ((zonal_u128)1 << 80)) == std::ldexp(1.0, 122) + std::ldexp(1.0, 80));
    // hand-worked: 1, 2, 3 at quantum 1/4 has mean 1/2 and sd 1/4; one cell has no sd; none has nothing
    {
        ZonalAcc a{0, 0, 0, 0, 0, INT32_MAX, INT32_MIN};
        CHECK(std::isnan(zonal_mean(a, 1.0)) && std::isnan(zonal_sd(a, 1.0)) && std::isnan(zonal_min(a, 1.0)) && std::isnan(zonal_sum(a, 1.0)));
        add(a, 2);
        CHECK(zonal_mean(a, 0.25) == 0.5 && std::isnan(zonal_sd(a, 0.25)) && zonal_min(a, 0.25) == 0.5 && zonal_max(a, 0.25) == 0.5);
        add(a, 1);
        add(a, 3);
        CHECK(zonal_sum(a, 0.25) == 1.5 && zonal_mean(a, 0.25) == 0.5 && zonal_sd(a, 0.25) == 0.25 && zonal_min(a, 0.25) == 0.25 && zonal_max(a, 0.25) == 0.75);
        CHECK(zonal_minus_mean(3, 0.25, 0.5) == 0.25 && zonal_dev(0.25, 0.25) == 1.0 && std::isnan(zonal_dev(0.25, 0.0)) && std::isnan(zonal_dev(0.25, NAN)));
        CHECK(zonal_above_min(3, 0.25, 0.25) == 0.5 && zonal_below_max(1, 0.25, 0.75) == 0.5);
    }
    // the quantum
    CHECK(zonal_default_quantum(0.0) == 1.0 && zonal_default_quantum(1.0) == std::ldexp(1.0, -30) && zonal_default_quantum(1073741824.0) == 1.0);
    CHECK(zonal_default_quantum(1073741825.0) == 2.0 && zonal_default_quantum(0.75) == std::ldexp(1.0, -30) && zonal_default_quantum(1e-320) == std::ldexp(1.0, -1022));
    CHECK(zonal_default_quantum(8848.86) == std::ldexp(1.0, -16) && zonal_default_quantum(1.7976931348623157e308) == std::ldexp(1.0, 994));
    for (double m : {1.0, 3.0, 8848.86, 1e-200, 1e300, 1073741824.0, 1073741825.0}) {
        const double q = zonal_default_quantum(m);
        CHECK(zonal_quantum_ok(q) && zonal_fits(m, q) && !zonal_fits(m, q / 2) && std::abs(zonal_q(m, q)) <= ZONAL_Q_MAX && std::abs(zonal_q(-m, q)) <= ZONAL_Q_MAX);
    }
    CHECK(zonal_quantum_ok(1.0) && zonal_quantum_ok(0.5) && zonal_quantum_ok(std::ldexp(1.0, -1022)) && zonal_quantum_ok(std::ldexp(1.0, 1023)));
    CHECK(!zonal_quantum_ok(3.0) && !zonal_quantum_ok(0.0) && !zonal_quantum_ok(-1.0) && !zonal_quantum_ok(INFINITY) && !zonal_quantum_ok(NAN) &&
          !zonal_quantum_ok(std::ldexp(1.0, -1023)) && !zonal_quantum_ok(0.75));
    // q rounds half to even
    CHECK(zonal_q(0.5, 1.0) == 0 && zonal_q(1.5, 1.0) == 2 && zonal_q(2.5, 1.0) == 2 && zonal_q(-0.5, 1.0) == 0 && zonal_q(-1.5, 1.0) == -2 && zonal_q(0.75, 0.5) == 2);
    // which accumulators a statistic needs
    CHECK(zonal_needs(ZONAL_CELLS) == ZONAL_A_CELLS && zonal_needs(ZONAL_COUNT) == ZONAL_A_N && zonal_needs(ZONAL_MEAN) == (ZONAL_A_N | ZONAL_A_S1));
    CHECK(zonal_needs(ZONAL_DEV) == (ZONAL_A_N | ZONAL_A_S1 | ZONAL_A_S2) && zonal_needs(ZONAL_RANGE) == (ZONAL_A_N | ZONAL_A_MIN | ZONAL_A_MAX));
    CHECK(zonal_needs(ZONAL_ALL_STATS) == 63u);

    // planes by the generator: value = a multiple of 1/4 in -250 .. 250 (or of 2^30 - 1 quanta, case 3), zone in -1 .. nz - 1
    const int shapes[][3] = {{1, 1, 1}, {5, 7, 3}, {33, 65, 40}, {67, 133, 1}, {67, 133, 9000}};
    for (int k = 0; k < 5; ++k) {
        const int nrow = shapes[k][0], ncol = shapes[k][1], nz = shapes[k][2];
        const size_t n = (size_t)nrow * ncol;
        lcg_state = 9000 + (uint64_t)k;
        std::vector<double> v(n);
        std::vector<int> zone(n);
        for (size_t i = 0; i < n; ++i) {
            const uint32_t a = lcg(), b = lcg();
            v[i] = k == 3 ? (a % 2 ? 1.0 : -1.0) * (double)(ZONAL_Q_MAX - 1) * 0.25 : ((double)(a % 2001) - 1000.0) * 0.25;
            zone[i] = (int)(b % (uint32_t)(nz + 1)) - 1;
        }
        const double quantum = 0.25;
        // forwards, backwards, and in two halves that are then combined: the same accumulators
        std::vector<ZonalAcc> fw((size_t)nz, ZonalAcc{0, 0, 0, 0, 0, INT32_MAX, INT32_MIN}), bw = fw, h0 = fw, h1 = fw;
        for (size_t i = 0; i < n; ++i) {
            if (zone[i] >= 0) { ++fw.at((size_t)zone[i]).cells; add(fw.at((size_t)zone[i]), zonal_q(v[i], quantum)); }
            const size_t j = n - 1 - i;
            if (zone[j] >= 0) { ++bw.at((size_t)zone[j]).cells; add(bw.at((size_t)zone[j]), zonal_q(v[j], quantum)); }
            std::vector<ZonalAcc> &h = i < n / 2 ? h0 : h1;
            if (zone[i] >= 0) { ++h.at((size_t)zone[i]).cells; add(h.at((size_t)zone[i]), zonal_q(v[i], quantum)); }
        }
        std::printf("case %d %d %d %d %d\n", k, nrow, ncol, nz, -2);
        for (int z = 0; z < nz; ++z) {
            const ZonalAcc &a = fw[(size_t)z], &b = bw[(size_t)z];
            ZonalAcc c = h0[(size_t)z];
            const ZonalAcc &d = h1[(size_t)z];
            c.cells += d.cells; c.n += d.n; c.S1 += d.S1; c.L += d.L; c.H += d.H;
            c.qmin = d.qmin < c.qmin ? d.qmin : c.qmin; c.qmax = d.qmax > c.qmax ? d.qmax : c.qmax;
            CHECK(std::memcmp(&a, &b, sizeof(a)) == 0 && std::memcmp(&a, &c, sizeof(a)) == 0);
            if (k == 3) CHECK(a.L >> 32 != 0 && a.H != 0);                     // the low word has passed 2^32: combined, not carried
            std::printf("zone %d %u %u %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", z, a.cells, a.n,
                        bits(zonal_sum(a, quantum)), bits(zonal_mean(a, quantum)), bits(zonal_sd(a, quantum)), bits(zonal_min(a, quantum)),
                        bits(zonal_max(a, quantum)));
        }
    }
    if (failures) return 1;
    std::printf("OK\n");
    return 0;
}
