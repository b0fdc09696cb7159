// The plan of a batched fit's staging block, free of any HIP header: one block of bytes handed out as typed pieces, every
// piece on a 16-byte boundary (the kernels rely on that), and the host's mirror of ONE contiguous byte range of it.  A
// fit lays out "what goes up", "what comes home" and "work" in turn and notes mark() between them; fit_common.h's
// FitBlock adds the device memory and the copies.
#pragma once
#include <algorithm>
#include <cassert>
#include <cstddef>
#include <vector>

namespace mhs {

constexpr size_t fit_align(size_t b) { return (b + 15) & ~(size_t)15; }

template <typename T>
struct FitPiece { size_t off = 0, count = 0; size_t bytes() const { return sizeof(T) * count; } };     // count elements of T at byte `off`

struct FitPlan {
    size_t at = 0;                      // bytes planned so far
    size_t from = 0, to = 0;            // the mirror holds the block's bytes [from, to)
    std::vector<char> buf;
    template <typename T>
    FitPiece<T> take(size_t count) { const FitPiece<T> q{at, count}; at += fit_align(q.bytes()); return q; }
    size_t mark() const { return at; }
    // The mirror covers [a, b), both marks, zero-filled where it grows; it keeps what it held.  A fit that moves its mirror
    // while a copy may still read the old range passes `room`, the longest range it will ask for, the first time: storage
    // that is large enough is never reallocated.
    void mirror(size_t a, size_t b, size_t room = 0) {
        assert(a % 16 == 0 && a <= b && b <= at);
        from = a; to = b;
        if (buf.size() < std::max(b - a, room)) buf.resize(std::max(b - a, room));
    }
    template <typename T>
    T *host(FitPiece<T> q) {
        assert(from <= q.off && q.off + q.bytes() <= to && "the piece lies outside the mirrored range");
        return reinterpret_cast<T *>(buf.data() + (q.off - from));
    }
};

}  // namespace mhs
