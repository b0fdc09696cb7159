// The flow-path rules (include/machisplin_hip.h, section "flow paths"): the pointer a D8 direction code makes of a cell, which
// cells stop a path, one step of pointer doubling -- over the whole plane and inside a tile -- and the products made from the
// cell a path ends at.  Free of any HIP header: the kernels of flowpath.hip and a plain C++ check program
// (tests/flowpath_check.cpp) share it.  Pointers and step counts are integers; the float products use only + - *, sqrt and
// comparisons, each rounded once (the library is built with -ffp-contract=off), so a numpy restatement gives the same bits.
//
// A cell's RECORD is its pointer (a cell number) and the counts of E-W, N-S and diagonal steps from the cell to the cell it
// points at.  A STOP cell points at itself: roots (direction -1), targets, NA cells, and the cells of a malformed plane that
// point nowhere.  Doubling replaces (pointer, counts) of a cell whose pointer is no stop cell by (pointer of pointer, counts +
// counts of pointer); it is a Jacobi step: every read is of the records as they stood before the round.  The counts are
// uint32, so that a plane with a cycle, on which they grow without bound, wraps instead of overflowing.
#pragma once

#include <cmath>
#include <cstdint>

#include "proximity_rule.h"

namespace mhs {

constexpr int FLOW_OUTLET = PROX_WHERES;               // MHS_FLOWPATH_OUTLET: no targets, the path runs to its root
enum { FLOW_ROOT_IS_TARGET = 1, FLOW_NO_LOCAL = 2 };   // the MHS_FLOWPATH_* flags of the header
enum { FLOW_DIR_OUT = -1, FLOW_DIR_NA = -2 };          // the direction codes of "hydrology" below 0

// The sizes at which flowpath.hip changes path; tests/test_flowpath_gpu.py reads them from this text.
constexpr int FLOW_TH = 32;                            // the tile of the local phase: rows ...
constexpr int FLOW_TW = 64;                            // ... and columns, the tile of terrain.hip and hydro.hip
constexpr int FLOW_TILE = FLOW_TH * FLOW_TW;
constexpr int FLOW_LOCAL_ROUNDS = 12;                  // ceil(log2(FLOW_TILE)) + 1: a path inside a tile has < 2048 steps
constexpr int FLOW_MAX_ROUNDS = 32;                    // a path has < 2^31 steps: 31 rounds move, the 32nd finds nothing to move

struct FlowCounts { uint32_t ew, ns, dg; };

// what the seed makes of a cell
enum { FLOW_CELL_NA = 0, FLOW_CELL_ROOT, FLOW_CELL_FLOWS, FLOW_CELL_BAD };

// rows south and columns east of direction k = 0 .. 7 = E, SE, S, SW, W, NW, N, NE
MHS_PROX_HD inline int flow_dr(int k) { return (k >= 1 && k <= 3) ? 1 : (k >= 5 ? -1 : 0); }
MHS_PROX_HD inline int flow_dc(int k) { return (k == 0 || k == 1 || k == 7) ? 1 : ((k >= 3 && k <= 5) ? -1 : 0); }

// Seed of cell (r, c) of an nrow x ncol plane `dir` with the row stride ld_dir: its kind, and its record in *ptr, *n.
// `target`: the cell satisfies the predicate (looked at only for a cell that is not NA).  Every cell but a FLOWS cell that is
// no target points at itself with counts 0.  BAD: a code outside -2 .. 7, or a pointer out of the raster or at an NA cell; the
// cell then points at itself, so that whatever the bytes of the plane are every pointer is a cell of the plane.
MHS_PROX_HD inline int flow_seed(const int8_t *dir, int64_t ld_dir, int r, int c, int nrow, int ncol, bool target, int32_t *ptr, FlowCounts *n) {
    const int32_t self = (int32_t)((int64_t)r * ncol + c);
    *ptr = self;
    *n = FlowCounts{0u, 0u, 0u};
    const int k = dir[(int64_t)r * ld_dir + c];
    if (k == FLOW_DIR_NA) return FLOW_CELL_NA;
    if (k == FLOW_DIR_OUT) return FLOW_CELL_ROOT;
    if (k < 0 || k > 7) return FLOW_CELL_BAD;
    const int rr = r + flow_dr(k), cc = c + flow_dc(k);
    if (rr < 0 || rr >= nrow || cc < 0 || cc >= ncol) return FLOW_CELL_BAD;
    if (dir[(int64_t)rr * ld_dir + cc] == FLOW_DIR_NA) return FLOW_CELL_BAD;
    if (!target) {
        *ptr = (int32_t)((int64_t)rr * ncol + cc);
        if (k & 1) n->dg = 1u;
        else if (k == 0 || k == 4) n->ew = 1u;
        else n->ns = 1u;
    }
    return FLOW_CELL_FLOWS;
}

MHS_PROX_HD inline void flow_add(FlowCounts &a, const FlowCounts &b) { a.ew += b.ew; a.ns += b.ns; a.dg += b.dg; }

// One doubling step of cell `self` with the record (p, n): pp, np = the record of cell p as it stood BEFORE the round.  A stop
// cell (p == self) and a cell that points at one (pp == p) stay.  FLOW_CYCLE: the pointer's pointer is the cell itself, which no
// forest has -- a cycle whose length is a power of two would otherwise fold into self-pointers and pass for stop cells (a cycle
// of any other length never settles and meets the round bound); the record stays as it is.
enum { FLOW_STAYS = 0, FLOW_MOVED, FLOW_CYCLE };
MHS_PROX_HD inline int flow_double(int32_t self, int32_t &p, FlowCounts &n, int32_t pp, const FlowCounts &np) {
    if (p == self || pp == p) return FLOW_STAYS;
    if (pp == self) return FLOW_CYCLE;
    flow_add(n, np);
    p = pp;
    return FLOW_MOVED;
}

// The local phase works on the tile whose first cell is (tr0, tc0), with LOCAL pointers: j >= 0 is slot j = (row in the tile)
// * FLOW_TW + (column in the tile) of the same tile, j < 0 is the cell ~j outside it.
MHS_PROX_HD inline int flow_to_local(int32_t p, int tr0, int tc0, int ncol) {
    const int pr = p / ncol, pc = p - pr * ncol;
    const int lr = pr - tr0, lc = pc - tc0;
    return (lr >= 0 && lr < FLOW_TH && lc >= 0 && lc < FLOW_TW) ? lr * FLOW_TW + lc : ~p;
}
MHS_PROX_HD inline int32_t flow_from_local(int j, int tr0, int tc0, int ncol) {
    return j < 0 ? (int32_t)~j : (int32_t)((int64_t)(tr0 + j / FLOW_TW) * ncol + tc0 + j % FLOW_TW);
}
// One doubling step of slot i with the local record (p, n) inside the tile `t` (int T::ptr(j), FlowCounts T::cnt(j): the slots
// as they stood before the round).  A slot that points outside the tile, at itself, or at a slot that points at itself stays:
// when no slot of a tile moves, every cell of the tile points at a stop cell of the tile or at a cell outside the tile.  A slot
// whose pointer points back at it (a cycle) stays too, and keeps a pointer that is no stop cell: the global rounds report it.
template <typename T>
MHS_PROX_HD inline bool flow_local_step(const T &t, int i, int &p, FlowCounts &n, bool counts) {
    if (p < 0 || p == i) return false;
    const int q = t.ptr(p);
    if (q == p || q == i) return false;
    if (counts) flow_add(n, t.cnt(p));
    p = q;
    return true;
}

// the products of a valid cell whose path ends at cell s after the steps n
MHS_PROX_HD inline double flow_diag(double dx, double dy) { return sqrt(dx * dx + dy * dy); }
MHS_PROX_HD inline int32_t flow_steps(const FlowCounts &n) { return (int32_t)(n.ew + n.ns + n.dg); }
MHS_PROX_HD inline double flow_dist(const FlowCounts &n, double dx, double dy, double g) {
    return ((double)n.ew * dx + (double)n.ns * dy) + (double)n.dg * g;
}
// layer values converted exactly to double: vs at the end of the path, vc at the cell itself
MHS_PROX_HD inline double flow_value(double vs, bool has_nodata, double nodata) { return prox_na(vs, has_nodata, nodata) ? (double)NAN : vs; }
MHS_PROX_HD inline double flow_drop(double vc, double vs, bool has_nodata, double nodata) {
    return (prox_na(vc, has_nodata, nodata) || prox_na(vs, has_nodata, nodata)) ? (double)NAN : vc - vs;
}

}  // namespace mhs
