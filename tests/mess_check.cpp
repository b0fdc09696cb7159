// Plain C++ check of machisplin_amd/csrc/mess_rule.h (no HIP): the rule on the hand-computed table of
// tests/test_mess_host.py, and the two-level count the kernel takes against the one-level binary search.  Built with
// -fsanitize=address,undefined by the test and run stand-alone.  Prints "p s i" lines (s as %.17g), then "OK".
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>
#include "mess_rule.h"

int main() {
    const double ref[4] = {1.0, 2.0, 3.0, 4.0};
    const double ps[] = {2.5, 1.0, 3.0, 4.0, 0.0, 5.0};
    for (double p : ps) {
        const int i = mhs::mess_count(ref, 4, p);
        std::printf("%.17g %.17g %d\n", p, mhs::mess_value(p, i, 4, ref[0], ref[3]), i);
    }
    // two levels == one level, over table sizes around the 64-value segments, duplicated values included
    const int sizes[] = {2, 3, 63, 64, 65, 127, 128, 129, 200, 732};
    for (int n : sizes) {
        std::vector<double> r((size_t)n);
        for (int j = 0; j < n; ++j) r[(size_t)j] = (double)((j * 7919) % 97) * 0.5;      // many ties
        std::sort(r.begin(), r.end());
        const int nc = (n + mhs::MESS_SEG - 1) / mhs::MESS_SEG;
        std::vector<double> coarse((size_t)nc);
        for (int k = 0; k < nc; ++k) coarse[(size_t)k] = r[(size_t)k * mhs::MESS_SEG];
        for (double p = -1.0; p <= 50.0; p += 0.25) {
            const int want = (int)(std::upper_bound(r.begin(), r.end(), p) - r.begin());
            const int one = mhs::mess_count(r.data(), n, p), two = mhs::mess_count2(r.data(), n, coarse.data(), nc, p);
            if (one != want || two != want) { std::printf("count mismatch: n %d p %g: %d %d, want %d\n", n, p, one, two, want); return 1; }
        }
        if (mhs::mess_count2(r.data(), n, coarse.data(), nc, NAN) != 0) { std::printf("NaN must count 0\n"); return 1; }
    }
    std::printf("OK\n");
    return 0;
}
