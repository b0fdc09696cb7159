// Stand-alone check of machisplin_amd/csrc/fit_stage.h, the HIP-free plan of the fits' staging block (built and run by
// test_fit_stage_host.py with a plain C++17 compiler).
#undef NDEBUG
#include <cassert>
#include <cstdint>
#include <cstdio>
#include "fit_stage.h"

using namespace mhs;

int main() {
    FitPlan blk;
    const FitPiece<int> a = blk.take<int>(1), b = blk.take<int>(37), c = blk.take<int>(101);
    const FitPiece<double> d = blk.take<double>(63);
    const FitPiece<char> e = blk.take<char>(5);
    const size_t off[5] = {a.off, b.off, c.off, d.off, e.off};
    const size_t len[5] = {a.bytes(), b.bytes(), c.bytes(), d.bytes(), e.bytes()};
    assert(len[0] == 4 && len[1] == 148 && len[2] == 404 && len[3] == 504 && len[4] == 5);
    size_t sum = 0;
    for (int i = 0; i < 5; ++i) {
        assert(off[i] % 16 == 0);                                   // every piece on a 16-byte boundary
        assert(off[i] == sum);                                      // behind its predecessor's aligned size: no overlap, no gap
        if (i) assert(off[i - 1] + len[i - 1] <= off[i]);
        sum += (len[i] + 15) / 16 * 16;
    }
    assert(blk.mark() == sum && sum == 16 + 160 + 416 + 512 + 16);

    // a zero-length piece is legal and takes no bytes
    const FitPiece<double> z = blk.take<double>(0);
    assert(z.off == sum && z.bytes() == 0 && blk.mark() == sum);

    // the mirror of the whole block: a piece's address is its offset into the mirror
    blk.mirror(0, blk.mark());
    const char *base = blk.buf.data();
    assert(blk.buf.size() == sum);
    assert((const char *)blk.host(a) == base + a.off && (const char *)blk.host(c) == base + c.off);
    assert((const char *)blk.host(d) == base + d.off && (const char *)blk.host(e) == base + e.off);
    assert((const char *)blk.host(z) == base + sum);
    assert((uintptr_t)blk.host(d) % alignof(double) == 0);
    for (size_t i = 0; i < d.count; ++i) blk.host(d)[i] = (double)i;
    for (size_t i = 0; i < c.count; ++i) blk.host(c)[i] = (int)i;
    for (size_t i = 0; i < d.count; ++i) assert(blk.host(d)[i] == (double)i);       // c's last element did not reach d

    // a mirror that starts at a mark other than 0 (a block that brings home a range behind its inputs): the first and
    // the last piece of [b, e] lie `off - from` bytes into it, and moving the mirror within its storage reallocates nothing
    const size_t from = b.off;
    blk.mirror(from, blk.mark());
    assert(blk.buf.data() == base && blk.from == from && blk.to == sum);
    assert((const char *)blk.host(b) == base + (b.off - from) && (const char *)blk.host(b) == base);
    assert((const char *)blk.host(e) == base + (e.off - from));
    blk.host(e)[4] = 'x';
    blk.host(b)[36] = 7;

    // room: the storage is sized once for the longest range
    FitPlan two;
    const FitPiece<int> up = two.take<int>(3);
    const size_t m1 = two.mark();
    const FitPiece<double> down = two.take<double>(100);
    two.mirror(0, m1, two.mark() - m1);
    const char *base2 = two.buf.data();
    assert(two.buf.size() == 800 && (const char *)two.host(up) == base2);
    two.mirror(m1, two.mark());
    assert(two.buf.data() == base2 && (const char *)two.host(down) == base2);
    two.host(down)[99] = 1.0;

    std::printf("fit_stage OK: %zu bytes in 5 pieces\n", sum);
    return 0;
}
