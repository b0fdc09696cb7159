// Plain C++ check of the multiple-flow-direction rules of machisplin_amd/csrc/hydro_rule.h (no HIP): rules 1 and 2 (W, D),
// the shares of rule 6 and the accumulation of rule 7 on a plane read from standard input, every fixed point reached by
// sweeping the rule functions over the whole plane, in place, until a sweep changes nothing -- what a workgroup of hydro.hip
// does with a tile.  Built with -fsanitize=address,undefined by the test and run stand-alone.
//
// Input:  nr nc dx dy exponent, then nr * nc heights in row-major order ("nan" = NA).
// Output: "n_valid N", "n_sinks N", "sweeps N", then one line per cell with A as a C99 hexadecimal double (%a: exact), then "OK".
#include <cmath>
#include <cstdio>
#include <vector>
#include "hydro_rule.h"

struct Plane {
    int nr, nc;
    size_t at(int r, int c) const { return (size_t)r * nc + c; }
    // the eight neighbours of (r, c) from plane p: `none` where the raster has no cell
    template <typename V>
    void gather(const std::vector<V> &p, int r, int c, V none, V out[8]) const {
        for (int k = 0; k < 8; ++k) {
            const int rr = r + mhs::hydro_dr(k), cc = c + mhs::hydro_dc(k);
            out[k] = (rr >= 0 && rr < nr && cc >= 0 && cc < nc) ? p.at(at(rr, cc)) : none;      // .at(): a rule that leaves the raster throws
        }
    }
};

int main() {
    int nr = 0, nc = 0;
    double dx = 0.0, dy = 0.0, x = 0.0;
    if (std::scanf("%d %d %lf %lf %lf", &nr, &nc, &dx, &dy, &x) != 5 || nr < 1 || nc < 1 || nr > 4096 || nc > 4096) { std::printf("bad header\n"); return 1; }
    const Plane pl{nr, nc};
    const size_t n = (size_t)nr * nc;
    std::vector<double> z(n), W(n), A(n), fin(8 * n, 0.0);
    std::vector<int32_t> D(n);
    std::vector<char> outlet(n, 0);
    for (size_t i = 0; i < n; ++i)
        if (std::scanf("%lf", &z[i]) != 1) { std::printf("bad plane\n"); return 1; }
    double wn[8];
    int32_t dn[8];
    for (int r = 0; r < nr; ++r)
        for (int c = 0; c < nc; ++c) {
            const size_t i = pl.at(r, c);
            pl.gather(z, r, c, (double)NAN, wn);
            const bool valid = z[i] == z[i];
            outlet[i] = valid && mhs::hydro_outlet(wn);
            W[i] = !valid ? NAN : outlet[i] ? z[i] : INFINITY;
        }
    for (bool changed = true; changed;) {                       // 1. the fill, from above
        changed = false;
        for (int r = 0; r < nr; ++r)
            for (int c = 0; c < nc; ++c) {
                const size_t i = pl.at(r, c);
                if (z[i] != z[i] || outlet[i]) continue;
                pl.gather(W, r, c, (double)NAN, wn);
                const double w = mhs::hydro_fill_step(z[i], wn);
                if (w < W[i]) { W[i] = w; changed = true; }
            }
    }
    for (int r = 0; r < nr; ++r)
        for (int c = 0; c < nc; ++c) {
            const size_t i = pl.at(r, c);
            pl.gather(W, r, c, (double)NAN, wn);
            D[i] = (z[i] != z[i] || outlet[i] || mhs::hydro_has_lower(W[i], wn)) ? 0 : mhs::HYDRO_D_INF;
        }
    for (bool changed = true; changed;) {                       // 2. the flat distance, from above
        changed = false;
        for (int r = 0; r < nr; ++r)
            for (int c = 0; c < nc; ++c) {
                const size_t i = pl.at(r, c);
                if (z[i] != z[i] || D[i] == 0) continue;
                pl.gather(W, r, c, (double)NAN, wn);
                pl.gather(D, r, c, (int32_t)mhs::HYDRO_D_INF, dn);
                const int32_t d = mhs::hydro_flat_step(W[i], wn, dn);
                if (d < D[i]) { D[i] = d; changed = true; }
            }
    }
    long n_valid = 0, n_sinks = 0;
    for (int r = 0; r < nr; ++r)                                // 6. the shares, each stored at its receiver: plane k of fin
        for (int c = 0; c < nc; ++c) {                          //    holds what neighbour k sends to the cell
            const size_t i = pl.at(r, c);
            A[i] = z[i] == z[i] ? 1.0 : NAN;
            if (z[i] != z[i]) continue;
            double f[8];
            pl.gather(W, r, c, (double)NAN, wn);
            pl.gather(D, r, c, (int32_t)mhs::HYDRO_D_INF, dn);
            const bool any = mhs::hydro_mfd_shares(W[i], D[i], wn, dn, dx, dy, x, f);
            ++n_valid;
            n_sinks += !any;
            for (int k = 0; any && k < 8; ++k)
                if (f[k] > 0.0) fin.at((size_t)((k + 4) & 7) * n + pl.at(r + mhs::hydro_dr(k), c + mhs::hydro_dc(k))) = f[k];
        }
    long sweeps = 0;
    for (bool changed = true; changed; ++sweeps) {              // 7. the accumulation, from below
        changed = false;
        for (int r = 0; r < nr; ++r)
            for (int c = 0; c < nc; ++c) {
                const size_t i = pl.at(r, c);
                if (z[i] != z[i]) continue;
                double an[8], fk[8];
                pl.gather(A, r, c, (double)NAN, an);
                for (int k = 0; k < 8; ++k) fk[k] = fin[(size_t)k * n + i];
                const double a = mhs::hydro_mfd_step(fk, an);
                if (a < A[i]) { std::printf("a sweep lowered cell %d %d\n", r, c); return 1; }
                if (a > A[i]) { A[i] = a; changed = true; }
            }
    }
    std::printf("n_valid %ld\nn_sinks %ld\nsweeps %ld\n", n_valid, n_sinks, sweeps);
    for (size_t i = 0; i < n; ++i) std::printf("%a\n", A[i]);
    std::printf("OK\n");
    return 0;
}
