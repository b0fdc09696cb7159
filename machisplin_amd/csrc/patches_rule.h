// The patches rules (include/machisplin_hip.h, section "patches"): which feature cells belong together, and the products made
// from that -- label = the smallest cell number row * ncol + col of the cell's patch, id = the dense numbering 1 .. K in
// increasing order of label, size, edge, keep.  Free of any HIP header: the kernels of patches.hip and a plain C++ check
// program (tests/patches_check.cpp) share it.  Everything is an integer, so a numpy restatement gives the same bits.
//
// The labelling is a block-based union-find over a plane of WORDS, one int32 per cell: a word holds -1 (no
// feature) or the cell number of another cell of the same patch, its PARENT; a cell whose word is its own number is a ROOT.
//
// THE DESCENT INVARIANT.  Every word, at every moment of every phase, holds either -1 or a cell number LESS THAN OR EQUAL to
// its own index.  Pointers then only descend: a walk from parent to parent strictly decreases until it stands on a root, so no
// find loop can cycle, whatever the interleaving of the lanes that link meanwhile -- the loops below have no iteration cap
// and need none.  The invariant holds by construction: a word is first written with a number <= its index (its run's head,
// its tile's root), and afterwards it changes only through fetch_min with a number smaller than its index (patch_union links
// the LARGER root to the smaller, never the other way) or by a store of its own root (the flatten).  A word never rises, and it
// never becomes -1.
//
// The words are read and written through an ACCESSOR `A`, so a rule never sees where they live (a tile's words in LDS, the
// label plane in global memory, a host vector):
//   int A::load(int i)               word i; on the device a relaxed atomic load
//   int A::fetch_min(int i, int v)   word i = min(word i, v), atomically; returns what the word held before
#pragma once

#include <cstdint>

#include "proximity_rule.h"            // prox_is_feature: the predicates are proximity's, not restated here

namespace mhs {

// The tile of phase 1; tests/test_patches_gpu.py reads the two from this text.  A wave holds one row of a tile in its 64 lanes.
constexpr int PATCH_TILE_ROWS = 32;
constexpr int PATCH_TILE_COLS = 64;
constexpr int PATCH_SCAN_BLOCK = 2048;         // phase 5: cells per block of the blocked prefix sum over the roots

// edge_rule of the filter (the MHS_PATCH_EDGE_* of the header, in its order)
enum { PATCH_EDGE_ANY = 0, PATCH_EDGE_TOUCHING, PATCH_EDGE_INTERIOR, PATCH_EDGE_RULES };
// the products, as bits of the kernels' mask
enum { PATCH_LABEL = 1, PATCH_ID = 2, PATCH_SIZE = 4, PATCH_EDGE = 8, PATCH_KEEP = 16 };

// One word of the count table, indexed by root cell number: the patch's size in the low 31 bits (a plane has at most
// 2^31 - 1 cells), bit 31 set when the patch has a cell in the first or last row or column.
constexpr uint32_t PATCH_EDGE_BIT = 0x80000000u;
constexpr uint32_t PATCH_SIZE_MASK = 0x7fffffffu;
MHS_PROX_HD inline int patch_size_of(uint32_t word) { return (int)(word & PATCH_SIZE_MASK); }
MHS_PROX_HD inline int patch_edge_of(uint32_t word) { return (int)(word >> 31); }

// the filter: the patch of `size` cells that touches the raster's edge (edge = 1) or not passes?
MHS_PROX_HD inline bool patch_keep(int64_t size, int edge, int64_t min_size, int64_t max_size, int edge_rule) {
    if (size < min_size || size > max_size) return false;
    return edge_rule == PATCH_EDGE_ANY || (edge_rule == PATCH_EDGE_TOUCHING ? edge != 0 : edge == 0);
}

// the root of x's patch as the words stand: parents strictly decrease (the invariant), so the walk ends
template <typename A>
MHS_PROX_HD inline int patch_find(A &a, int x) {
    for (int p = a.load(x); p != x; p = a.load(x)) x = p;
    return x;
}

// Join the patches of x and y, lock-free: find both roots; fetch_min the LARGER root's word with the smaller; if the word
// still held the root itself the link is made.  If not, another lane had linked that root meanwhile: the word then held a
// parent `old`, and whichever of old and the smaller root the word now holds, the other one is still to be joined -- retry
// from the value returned.  Every retry follows a word that some lane lowered, and words never rise: the loop ends.
template <typename A>
MHS_PROX_HD inline void patch_union(A &a, int x, int y) {
    for (;;) {
        x = patch_find(a, x);
        y = patch_find(a, y);
        if (x == y) return;
        if (x < y) { const int t = x; x = y; y = t; }           // x: the larger root
        const int old = a.fetch_min(x, y);
        if (old == x) return;
        x = old;
    }
}

// Phase 1, rows: the feature flags of one tile row are a 64-bit ballot.  The first column of the run of set bits that holds
// bit `c` (which is set): one past the highest clear bit below c.
MHS_PROX_HD inline int patch_run_start(uint64_t row, int c) {
    const uint64_t gaps = ~row & ((1ull << c) - 1);
    return gaps ? 64 - __builtin_clzll(gaps) : 0;
}
// ... and the number of set bits from bit c (set) up to the run's end
MHS_PROX_HD inline int patch_run_length(uint64_t row, int c) {
    const uint64_t clear = ~(row >> c);                            // bit k: column c + k is clear (the bits shifted in at the top are)
    return clear ? __builtin_ctzll(clear) : 64;                    // no clear bit: c = 0 and the whole row is one run
}
MHS_PROX_HD inline bool patch_bit(uint64_t row, int c) { return c >= 0 && c < 64 && ((row >> c) & 1); }

// Phase 1, run heads only: which cells of the row above must the feature cell at column c link with, so that every pair of
// neighbouring runs of the two rows is linked at least once and (nearly) no pair twice?  `row` holds the cell, `up` is the row
// above.  Returns bits: 1 = the cell above, 2 = above left, 4 = above right.
//   above        at the first column of every stretch in which the two rows are both set
//   above left   (8) only from a run's first cell, and only when the cell above is clear: otherwise above-left and above are
//                one run of the upper row, and a cell further right in this run has the link already
//   above right  (8) only from a run's last cell, and only when the cell above is clear
MHS_PROX_HD inline int patch_up_links(uint64_t row, uint64_t up, int c, int connectivity) {
    int links = 0;
    const bool above = patch_bit(up, c);
    if (above && !(patch_bit(row, c - 1) && patch_bit(up, c - 1))) links |= 1;
    if (connectivity == 8 && !above) {
        if (patch_bit(up, c - 1) && !patch_bit(row, c - 1)) links |= 2;
        if (patch_bit(up, c + 1) && !patch_bit(row, c + 1)) links |= 4;
    }
    return links;
}

// Phase 2, which links across a tile border are made.  A link may be left out only when links that ARE made imply it, and
// the order below is well-founded: east links are always made; a south link may lean on the south link one column to the
// left and on the two cells' links within their own tiles; a diagonal link may lean on east, south and in-tile links.
//   south   (r, c) -- (r + 1, c): left out when (r, c - 1) and (r + 1, c - 1) are both features AND column c - 1 is in the
//           same tile column -- those two are then joined to (r, c) and (r + 1, c) inside their tiles by phase 1
//   diagonal  P -- Q: left out when either of the other two cells of their 2 x 2 block is a feature: P and Q then meet
//           through it by two links along rows and columns
MHS_PROX_HD inline bool patch_south_link(bool left, bool left_below, int c) {
    return !(left && left_below && c % PATCH_TILE_COLS != 0);
}
MHS_PROX_HD inline bool patch_diagonal_link(bool other_a, bool other_b) { return !other_a && !other_b; }

}  // namespace mhs
