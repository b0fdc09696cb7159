// classes_rule.h in a plain C++ program (no HIP header), built with -fsanitize=address,undefined by tests/test_classes_host.py:
//   * both class-index forms against a linear search, for every code 0 .. 65 535 (and -1, 65 536), over lists of K = 1, 2, 255,
//     256 with the codes 0 and 65 535 among them, dense lists that take the direct table and spread lists that take bisection;
//   * cls_code on the values at its edges;
//   * the finishing function on all-equal counts, n = 0, n = 2^31 - 1 in one class (simpson's numerator at its largest), a tie
//     at every position, against 128-bit integer arithmetic;
//   * and it prints LCG cases "unit ..." that the test compares with the numpy restatement.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "classes_rule.h"

using namespace mhs;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static uint64_t bits(double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; }

static int linear(const std::vector<uint16_t> &codes, int code) {
    for (size_t k = 0; k < codes.size(); ++k)
        if ((int)codes[k] == code) return (int)k;
    return -1;
}

static void check_index(const std::vector<uint16_t> &codes) {
    const int K = (int)codes.size();
    for (int k = 1; k < K; ++k) CHECK(codes[k - 1] < codes[k]);
    const bool table = cls_use_table(codes.data(), K);
    std::vector<int16_t> tab(CLS_TABLE_SPAN, (int16_t)-7);
    const int span = (int)codes[K - 1] - (int)codes[0] + 1;
    if (table) {
        CHECK(span <= CLS_TABLE_SPAN);
        cls_fill_table(codes.data(), K, tab.data());
    }
    for (int code = -1; code <= CLS_MAX_CODE + 1; ++code) {
        const int want = linear(codes, code);
        CHECK(cls_index_bisect(codes.data(), K, code) == want);
        if (table) CHECK(cls_index_table(tab.data(), codes[0], span, code) == want);
    }
    std::printf("index K %d span %d %s\n", K, span, table ? "table+bisect" : "bisect");
}

static std::vector<uint16_t> spread(int K, int first, int step, bool with_last) {
    std::vector<uint16_t> c;
    for (int k = 0; k < K; ++k) c.push_back((uint16_t)(first + k * step));
    if (with_last) c.back() = (uint16_t)CLS_MAX_CODE;
    return c;
}

// the rule against 128-bit integers and one division each
static void check_finish(const std::vector<uint32_t> &count, uint32_t other, const std::vector<uint16_t> &codes) {
    const int K = (int)count.size();
    const ClsFin f = cls_finish(count.data(), K, other, codes.data());
    unsigned __int128 n = other, sq = (unsigned __int128)other * other;
    uint32_t best = 0;
    int mode = -1, variety = 0;
    for (int k = 0; k < K; ++k) {
        n += count[k];
        sq += (unsigned __int128)count[k] * count[k];
        if (count[k]) ++variety;
        if (count[k] > best) { best = count[k]; mode = codes[k]; }
    }
    CHECK(n <= 2147483647u);
    CHECK(f.n == (uint32_t)n && f.mode == mode && f.variety == variety);
    if (mode < 0) CHECK(f.mode_frac != f.mode_frac);
    else CHECK(bits(f.mode_frac) == bits((double)best / (double)(uint64_t)n));
    if (n == 0) CHECK(f.simpson != f.simpson);
    else {
        const unsigned __int128 num = n * n - sq;
        CHECK(num <= ((unsigned __int128)1 << 62));
        CHECK(bits(f.simpson) == bits((double)(uint64_t)num / ((double)(uint64_t)n * (double)(uint64_t)n)));
        CHECK(f.simpson >= 0.0 && f.simpson < 1.0);
    }
    for (int k = 0; k < K; ++k) {
        const double fr = cls_frac(count[k], f.n);
        if (n == 0) CHECK(fr != fr);
        else CHECK(bits(fr) == bits((double)count[k] / (double)(uint64_t)n));
    }
}

int main() {
    // the class index
    check_index({0});
    check_index({65535});
    check_index({0, 65535});
    check_index({7, 8});
    check_index(spread(255, 0, 1, false));
    check_index(spread(255, 0, 257, true));
    check_index(spread(256, 0, 1, false));               // span 256: the table
    check_index(spread(256, 0, 4, false));               // span 1021: the table, at its widest but three
    check_index({0, 1023});                              // span 1024: the table's last size
    check_index({0, 1024});                              // one more: bisection
    check_index(spread(256, 0, 256, true));              // 0 .. 65 535: bisection at K = 256
    check_index(spread(256, 65280, 1, false));           // the top 256 codes
    check_index(spread(3, 11, 1000, false));
    // the code of a value
    CHECK(cls_code(0.0) == 0 && cls_code(-0.0) == 0 && cls_code(65535.0) == 65535 && cls_code(65536.0) == -1 && cls_code(-1.0) == -1);
    CHECK(cls_code(0.5) == -1 && cls_code(65534.999) == -1 && cls_code(1e300) == -1 && cls_code(-1e300) == -1);
    CHECK(cls_code(INFINITY) == -1 && cls_code(-INFINITY) == -1 && cls_code(std::nan("")) == -1 && cls_code(41.0) == 41);
    CHECK(cls_na(std::nan(""), false, 0.0) && cls_na(-32768.0, true, -32768.0) && !cls_na(-32768.0, false, -32768.0) && !cls_na(0.0, true, -1.0));
    // the finishing function
    const std::vector<uint16_t> c4 = {3, 9, 200, 65535};
    check_finish({0, 0, 0, 0}, 0, c4);                                     // n = 0
    check_finish({0, 0, 0, 0}, 17, c4);                                    // only `other`: mode -1, n > 0
    check_finish({5, 5, 5, 5}, 0, c4);                                     // all equal: the smallest code
    check_finish({5, 5, 5, 5}, 5, c4);
    check_finish({2147483647u, 0, 0, 0}, 0, c4);                           // n = 2^31 - 1 in one class: simpson 0
    check_finish({0, 0, 0, 2147483647u}, 0, c4);
    check_finish({0, 0, 0, 0}, 2147483647u, c4);
    check_finish({1073741824u, 1073741823u, 0, 0}, 0, c4);                 // the numerator near 2^61
    check_finish({536870912u, 536870912u, 536870912u, 536870911u}, 0, c4);
    {
        const ClsFin f = cls_finish(std::vector<uint32_t>{5, 5, 5, 5}.data(), 4, 0, c4.data());
        CHECK(f.mode == 3 && f.variety == 4 && f.mode_frac == 0.25 && f.simpson == 0.75);
    }
    for (int a = 0; a < 6; ++a)                                            // a tie at every pair of positions of K = 6
        for (int b = a + 1; b < 6; ++b) {
            std::vector<uint32_t> cnt = {1, 2, 3, 1, 2, 3};
            const std::vector<uint16_t> c6 = {10, 20, 30, 40, 50, 60};
            cnt[a] = cnt[b] = 9;
            check_finish(cnt, 4, c6);
            CHECK(cls_finish(cnt.data(), 6, 4, c6.data()).mode == c6[a]);
        }
    {   // K = 256, one cell each
        const std::vector<uint16_t> c = spread(256, 0, 256, true);
        std::vector<uint32_t> cnt(256, 1u);
        check_finish(cnt, 0, c);
        CHECK(cls_finish(cnt.data(), 256, 0, c.data()).mode == 0);
        cnt[255] = 2;
        CHECK(cls_finish(cnt.data(), 256, 0, c.data()).mode == 65535);
    }
    // LCG cases for the numpy restatement: "case id K" then "unit other count.. -> n mode variety mode_frac simpson" in hex bits
    uint64_t state = 20240607;
    auto next = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(state >> 33); };
    for (int id = 0; id < 4; ++id) {
        const int K = id == 0 ? 1 : id == 1 ? 3 : id == 2 ? 16 : 256;
        const std::vector<uint16_t> c = spread(K, 5, K == 256 ? 200 : 7, false);
        std::printf("case %d %d\n", id, K);
        for (int u = 0; u < 50; ++u) {
            std::vector<uint32_t> cnt(K);
            const uint32_t range = u % 5 == 0 ? 3u : u % 5 == 1 ? 1u : 100000u;      // many ties, all zero, large
            for (int k = 0; k < K; ++k) cnt[k] = next() % range;
            const uint32_t other = next() % range;
            check_finish(cnt, other, c);
            const ClsFin f = cls_finish(cnt.data(), K, other, c.data());
            std::printf("unit %u", other);
            for (int k = 0; k < K; ++k) std::printf(" %u", cnt[k]);
            std::printf(" -> %u %d %d %016" PRIx64 " %016" PRIx64 "\n", f.n, f.mode, f.variety, bits(f.mode_frac), bits(f.simpson));
        }
    }
    std::printf("OK\n");
    return 0;
}
