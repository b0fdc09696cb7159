// The flow-path rule of csrc/flowpath_rule.h in a plain C++ program: the header the kernels are built from is compiled here with
// gcc (no HIP), under AddressSanitizer and UBSan, and drives the rule on HOST arrays the way csrc/flowpath.hip drives it on the
// device -- seed, the local phase tile by tile (Jacobi rounds on a copy of the tile), the global rounds between two buffers,
// the products -- with every access bounds-checked (.at()).  Each case runs twice, with and without the local phase; the two
// must give the same planes.
//
// Input, a text file named by the only argument (tests/test_flowpath_host.py writes it):
//   n_cases, then per case:  nrow ncol where root_is_target has_nodata  threshold nodata dx dy (doubles as hex bits)
//                            nrow * ncol direction codes, nrow * ncol layer values, nrow * ncol value-layer values (hex bits)
// Output per case:  "case k malformed" | "case k cycle" | "case k ok n_valid n_targets n_roots n_unreached max_steps rounds
// rounds_with_local" and then five lines: index, steps (integers), dist, value, drop (hex bits, one NaN).  Then OK.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "flowpath_rule.h"

using namespace mhs;

struct Rec { int32_t ptr; FlowCounts n; };

static uint64_t bits(double v) {
    if (v != v) return 0x7ff8000000000000ULL;            // one NaN
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}
static double from_bits(uint64_t b) {
    double v;
    std::memcpy(&v, &b, 8);
    return v;
}

struct HostTile {
    const std::vector<int> &lp;
    const std::vector<FlowCounts> &ln;
    int ptr(int j) const { return lp.at((size_t)j); }
    FlowCounts cnt(int j) const { return ln.at((size_t)j); }
};

struct Case {
    int nrow, ncol, where, root_ok, has_nodata;
    double threshold, nodata, dx, dy;
    std::vector<int8_t> dir;
    std::vector<double> z, v;
};

struct Result {
    int status = 0;                                       // 0 ok, 1 malformed, 2 cycle
    long long n_valid = 0, n_targets = 0, n_roots = 0, n_unreached = 0, max_steps = -1;
    int rounds = 0;
    std::vector<int32_t> index, steps;
    std::vector<double> dist, value, drop;
};

static Result run(const Case &q, bool local) {
    Result res;
    const int nrow = q.nrow, ncol = q.ncol;
    const size_t n = (size_t)nrow * ncol;
    std::vector<Rec> buf[2] = {std::vector<Rec>(n), std::vector<Rec>(n)};
    long long n_bad = 0;
    for (int r = 0; r < nrow; ++r)
        for (int c = 0; c < ncol; ++c) {
            const size_t i = (size_t)r * ncol + c;
            const bool target = q.where != FLOW_OUTLET && prox_is_feature(q.z.at(i), q.has_nodata != 0, q.nodata, q.where, q.threshold);
            Rec &rec = buf[0].at(i);
            const int kind = flow_seed(q.dir.data(), ncol, r, c, nrow, ncol, target, &rec.ptr, &rec.n);
            res.n_valid += kind != FLOW_CELL_NA;
            res.n_targets += kind != FLOW_CELL_NA && target;
            res.n_roots += kind == FLOW_CELL_ROOT;
            n_bad += kind == FLOW_CELL_BAD;
            if (rec.ptr < 0 || (size_t)rec.ptr >= n) std::abort();
        }
    if (n_bad) { res.status = 1; return res; }
    int cur = 0;
    if (local) {
        for (int tr0 = 0; tr0 < nrow; tr0 += FLOW_TH)
            for (int tc0 = 0; tc0 < ncol; tc0 += FLOW_TW) {
                std::vector<int> lp(FLOW_TILE);
                std::vector<FlowCounts> ln(FLOW_TILE, FlowCounts{0u, 0u, 0u});
                for (int i = 0; i < FLOW_TILE; ++i) {
                    const int r = tr0 + i / FLOW_TW, c = tc0 + i % FLOW_TW;
                    lp[(size_t)i] = i;
                    if (r < nrow && c < ncol) {
                        const Rec &rec = buf[0].at((size_t)r * ncol + c);
                        lp[(size_t)i] = flow_to_local(rec.ptr, tr0, tc0, ncol);
                        ln[(size_t)i] = rec.n;
                    }
                }
                int round = 0;
                for (; round < FLOW_LOCAL_ROUNDS; ++round) {
                    std::vector<int> np(lp);
                    std::vector<FlowCounts> nn(ln);
                    const HostTile tile{lp, ln};
                    bool moved = false;
                    for (int i = 0; i < FLOW_TILE; ++i) moved |= flow_local_step(tile, i, np[(size_t)i], nn[(size_t)i], true);
                    if (!moved) break;
                    lp.swap(np);
                    ln.swap(nn);
                }
                if (round == FLOW_LOCAL_ROUNDS) res.status = 2;        // only a cycle inside the tile keeps moving; the global rounds say so too
                for (int i = 0; i < FLOW_TILE; ++i) {
                    const int r = tr0 + i / FLOW_TW, c = tc0 + i % FLOW_TW;
                    if (r < nrow && c < ncol) buf[1].at((size_t)r * ncol + c) = Rec{flow_from_local(lp[(size_t)i], tr0, tc0, ncol), ln[(size_t)i]};
                }
            }
        cur = 1;
    }
    bool done = false;
    for (int launch = 0; launch < FLOW_MAX_ROUNDS && !done; ++launch) {
        const std::vector<Rec> &src = buf[cur];
        std::vector<Rec> &dst = buf[cur ^ 1];
        long long moved = 0, cycle = 0;
        for (size_t i = 0; i < n; ++i) {
            Rec rec = src.at(i);
            if (rec.ptr != (int32_t)i) {
                const Rec &pr = src.at((size_t)rec.ptr);
                const int what = flow_double((int32_t)i, rec.ptr, rec.n, pr.ptr, pr.n);
                moved += what == FLOW_MOVED;
                cycle += what == FLOW_CYCLE;
            }
            dst.at(i) = rec;
        }
        if (cycle) { res.status = 2; return res; }
        cur ^= 1;
        if (moved == 0) done = true;
        else ++res.rounds;
    }
    if (!done) { res.status = 2; return res; }
    if (res.status) std::abort();                          // a tile that never settled on a plane the global rounds resolved
    const double g = flow_diag(q.dx, q.dy);
    res.index.assign(n, -1); res.steps.assign(n, -1);
    res.dist.assign(n, NAN); res.value.assign(n, NAN); res.drop.assign(n, NAN);
    for (size_t i = 0; i < n; ++i) {
        if (q.dir.at(i) == FLOW_DIR_NA) continue;
        const Rec &rec = buf[cur].at(i);
        const size_t s = (size_t)rec.ptr;
        const bool reached = q.root_ok || prox_is_feature(q.z.at(s), q.has_nodata != 0, q.nodata, q.where, q.threshold);
        if (!reached) { ++res.n_unreached; continue; }
        res.index[i] = rec.ptr;
        res.steps[i] = flow_steps(rec.n);
        if (res.steps[i] > res.max_steps) res.max_steps = res.steps[i];
        res.dist[i] = flow_dist(rec.n, q.dx, q.dy, g);
        res.value[i] = flow_value(q.v.at(s), q.has_nodata != 0, q.nodata);
        res.drop[i] = flow_drop(q.v.at(i), q.v.at(s), q.has_nodata != 0, q.nodata);
    }
    return res;
}

static bool same(const std::vector<double> &a, const std::vector<double> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (bits(a[i]) != bits(b[i])) return false;
    return true;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int n_cases = 0;
    if (std::fscanf(f, "%d", &n_cases) != 1) return 2;
    for (int k = 0; k < n_cases; ++k) {
        Case q;
        uint64_t b[4];
        if (std::fscanf(f, "%d %d %d %d %d %" SCNx64 " %" SCNx64 " %" SCNx64 " %" SCNx64, &q.nrow, &q.ncol, &q.where, &q.root_ok, &q.has_nodata, &b[0],
                        &b[1], &b[2], &b[3]) != 9)
            return 2;
        q.threshold = from_bits(b[0]); q.nodata = from_bits(b[1]); q.dx = from_bits(b[2]); q.dy = from_bits(b[3]);
        q.root_ok = q.root_ok || q.where == FLOW_OUTLET;
        const size_t n = (size_t)q.nrow * q.ncol;
        q.dir.resize(n); q.z.resize(n); q.v.resize(n);
        for (size_t i = 0; i < n; ++i) {
            int d;
            if (std::fscanf(f, "%d", &d) != 1 || d < -128 || d > 127) return 2;
            q.dir[i] = (int8_t)d;
        }
        for (std::vector<double> *p : {&q.z, &q.v})
            for (size_t i = 0; i < n; ++i) {
                uint64_t x;
                if (std::fscanf(f, "%" SCNx64, &x) != 1) return 2;
                (*p)[i] = from_bits(x);
            }
        const Result a = run(q, false), l = run(q, true);
        if (a.status != l.status) { std::printf("case %d: the routes disagree on the status\n", k); return 1; }
        if (a.status) { std::printf("case %d %s\n", k, a.status == 1 ? "malformed" : "cycle"); continue; }
        if (a.index != l.index || a.steps != l.steps || !same(a.dist, l.dist) || !same(a.value, l.value) || !same(a.drop, l.drop) ||
            a.n_unreached != l.n_unreached || a.max_steps != l.max_steps || l.rounds > a.rounds) {
            std::printf("case %d: the routes disagree\n", k);
            return 1;
        }
        std::printf("case %d ok %lld %lld %lld %lld %lld %d %d\n", k, a.n_valid, a.n_targets, a.n_roots, a.n_unreached, a.max_steps, a.rounds, l.rounds);
        for (int32_t x : a.index) std::printf("%d ", x);
        std::printf("\n");
        for (int32_t x : a.steps) std::printf("%d ", x);
        std::printf("\n");
        for (const std::vector<double> *p : {&a.dist, &a.value, &a.drop}) {
            for (double x : *p) std::printf("%" PRIx64 " ", bits(x));
            std::printf("\n");
        }
    }
    std::fclose(f);
    std::printf("OK\n");
    return 0;
}
