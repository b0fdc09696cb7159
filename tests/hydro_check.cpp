// Plain C++ check of machisplin_amd/csrc/hydro_rule.h (no HIP): the rules on the hand-worked table of
// tests/test_hydro_host.py.  The three fixed points are reached by sweeping the rule functions over the whole plane, in place,
// until a sweep changes nothing -- what a workgroup of hydro.hip does with a tile.  Built with -fsanitize=address,undefined by
// the test and run stand-alone.  Prints "name value" lines (%.17g), then "OK".
#include <cmath>
#include <cstdio>
#include <vector>
#include "hydro_rule.h"

struct Solved {
    int nr, nc;
    std::vector<double> z, W, A;
    std::vector<int32_t> D;
    std::vector<int8_t> dir;
    long n_valid = 0, n_raised = 0, n_sinks = 0;
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

static Solved solve(int nr, int nc, const std::vector<double> &z, double dx, double dy) {
    Solved s{nr, nc, z, std::vector<double>(z.size()), std::vector<double>(z.size()), std::vector<int32_t>(z.size()),
             std::vector<int8_t>(z.size())};
    std::vector<char> outlet(z.size(), 0);
    double wn[8];
    int32_t dn[8];
    for (int r = 0; r < nr; ++r)
        for (int c = 0; c < nc; ++c) {
            const size_t i = s.at(r, c);
            s.gather(z, r, c, (double)NAN, wn);
            const bool valid = z[i] == z[i];
            outlet[i] = valid && mhs::hydro_outlet(wn);
            s.W[i] = !valid ? NAN : outlet[i] ? z[i] : INFINITY;
        }
    for (bool changed = true; changed;) {                       // 1. the fill, from above
        changed = false;
        for (int r = 0; r < nr; ++r)
            for (int c = 0; c < nc; ++c) {
                const size_t i = s.at(r, c);
                if (z[i] != z[i] || outlet[i]) continue;
                s.gather(s.W, r, c, (double)NAN, wn);
                const double w = mhs::hydro_fill_step(z[i], wn);
                if (w < s.W[i]) { s.W[i] = w; changed = true; }
            }
    }
    for (int r = 0; r < nr; ++r)
        for (int c = 0; c < nc; ++c) {
            const size_t i = s.at(r, c);
            s.gather(s.W, r, c, (double)NAN, wn);
            s.D[i] = (z[i] != z[i] || outlet[i] || mhs::hydro_has_lower(s.W[i], wn)) ? 0 : mhs::HYDRO_D_INF;
        }
    for (bool changed = true; changed;) {                       // 2. the flat distance, from above
        changed = false;
        for (int r = 0; r < nr; ++r)
            for (int c = 0; c < nc; ++c) {
                const size_t i = s.at(r, c);
                if (z[i] != z[i] || s.D[i] == 0) continue;
                s.gather(s.W, r, c, (double)NAN, wn);
                s.gather(s.D, r, c, (int32_t)mhs::HYDRO_D_INF, dn);
                const int32_t d = mhs::hydro_flat_step(s.W[i], wn, dn);
                if (d < s.D[i]) { s.D[i] = d; changed = true; }
            }
    }
    for (int r = 0; r < nr; ++r)                                // 3. the directions
        for (int c = 0; c < nc; ++c) {
            const size_t i = s.at(r, c);
            s.A[i] = z[i] == z[i] ? 1.0 : NAN;
            if (z[i] != z[i]) { s.dir[i] = mhs::HYDRO_DIR_NA; continue; }
            s.gather(s.W, r, c, (double)NAN, wn);
            s.gather(s.D, r, c, (int32_t)mhs::HYDRO_D_INF, dn);
            s.dir[i] = mhs::hydro_direction(s.W[i], s.D[i], wn, dn, dx, dy);
            s.n_valid += 1; s.n_raised += s.W[i] > z[i]; s.n_sinks += s.dir[i] == mhs::HYDRO_DIR_OUT;
        }
    for (bool changed = true; changed;) {                       // 4. the accumulation, from below
        changed = false;
        for (int r = 0; r < nr; ++r)
            for (int c = 0; c < nc; ++c) {
                const size_t i = s.at(r, c);
                if (z[i] != z[i]) continue;
                int8_t kn[8];
                double an[8];
                s.gather(s.dir, r, c, (int8_t)mhs::HYDRO_DIR_NA, kn);
                s.gather(s.A, r, c, (double)NAN, an);
                const double a = mhs::hydro_acc_step(mhs::hydro_donors(kn), an);
                if (a > s.A[i]) { s.A[i] = a; changed = true; }
            }
    }
    return s;
}

static double sink_sum(const Solved &s) {
    double sum = 0.0;
    for (size_t i = 0; i < s.z.size(); ++i)
        if (s.dir[i] == mhs::HYDRO_DIR_OUT) sum += s.A[i];
    return sum;
}

static std::vector<double> ring_plane(int nr, int nc, double ring, double inside) {
    std::vector<double> z((size_t)nr * nc, inside);
    for (int r = 0; r < nr; ++r)
        for (int c = 0; c < nc; ++c)
            if (r == 0 || c == 0 || r == nr - 1 || c == nc - 1) z[(size_t)r * nc + c] = ring;
    return z;
}

int main() {
    for (int k = 0; k < 8; ++k)                                 // the opposite neighbour undoes the step
        if (mhs::hydro_dr(k) + mhs::hydro_dr((k + 4) & 7) != 0 || mhs::hydro_dc(k) + mhs::hydro_dc((k + 4) & 7) != 0) { std::printf("neighbour table wrong\n"); return 1; }

    {   // a single pit: ring 5, inside 4, centre 1
        std::vector<double> z = ring_plane(5, 5, 5.0, 4.0);
        z[12] = 1.0;
        const Solved s = solve(5, 5, z, 1.0, 1.0);
        std::printf("pit_w_centre %.17g\npit_d_centre %d\npit_dir_centre %d\npit_dir_11 %d\npit_a_24 %.17g\npit_raised %ld\npit_sinks %ld\npit_sink_sum %.17g\n",
                    s.W[12], s.D[12], s.dir[12], s.dir[s.at(1, 1)], s.A[s.at(2, 4)], s.n_raised, s.n_sinks, sink_sum(s));
    }
    {   // a tilted plane z = column, 4 x 6: no fill, all directions west, A a ramp
        std::vector<double> z(24);
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 6; ++c) z[(size_t)r * 6 + c] = c;
        const Solved s = solve(4, 6, z, 1.0, 1.0);
        bool west = true, ramp = true;
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 6; ++c) {
                west &= s.dir[s.at(r, c)] == (c == 0 ? -1 : 4);
                ramp &= s.A[s.at(r, c)] == 6.0 - c;
            }
        std::printf("tilt_all_west %d\ntilt_ramp %d\ntilt_raised %ld\ntilt_sinks %ld\n", (int)west, (int)ramp, s.n_raised, s.n_sinks);
    }
    {   // a constant plane 5 x 7: D is the ring distance to the border
        const Solved s = solve(5, 7, std::vector<double>(35, 17.0), 1.0, 1.0);
        bool rings = true;
        for (int r = 0; r < 5; ++r)
            for (int c = 0; c < 7; ++c) {
                int d = r < c ? r : c;
                d = 4 - r < d ? 4 - r : d;
                d = 6 - c < d ? 6 - c : d;
                rings &= s.D[s.at(r, c)] == d;
            }
        std::printf("const_ring_distance %d\nconst_sinks %ld\nconst_sink_sum %.17g\n", (int)rings, s.n_sinks, sink_sum(s));
    }
    {   // two nested pits, 7 x 7: ring 9 with a gap of 3 at (3, 6); inside 6; the middle 3 x 3 is 4 with a centre of 2
        std::vector<double> z = ring_plane(7, 7, 9.0, 6.0);
        for (int r = 2; r <= 4; ++r) for (int c = 2; c <= 4; ++c) z[(size_t)r * 7 + c] = 4.0;
        z[3 * 7 + 3] = 2.0;
        z[3 * 7 + 6] = 3.0;
        const Solved s = solve(7, 7, z, 1.0, 1.0);
        std::printf("nest_w_centre %.17g\nnest_d_centre %d\nnest_d_11 %d\nnest_dir_centre %d\nnest_dir_25 %d\nnest_a_gap %.17g\nnest_raised %ld\nnest_sinks %ld\n",
                    s.W[s.at(3, 3)], s.D[s.at(3, 3)], s.D[s.at(1, 1)], s.dir[s.at(3, 3)], s.dir[s.at(2, 5)], s.A[s.at(3, 6)], s.n_raised, s.n_sinks);
    }
    {   // an NA hole that drains its surroundings, 5 x 5: ring 5, inside 3, the centre NA
        std::vector<double> z = ring_plane(5, 5, 5.0, 3.0);
        z[12] = NAN;
        const Solved s = solve(5, 5, z, 1.0, 1.0);
        std::printf("hole_dir_centre %d\nhole_dir_11 %d\nhole_dir_00 %d\nhole_a_11 %.17g\nhole_a_12 %.17g\nhole_sinks %ld\nhole_valid %ld\nhole_sink_sum %.17g\n",
                    s.dir[12], s.dir[s.at(1, 1)], s.dir[0], s.A[s.at(1, 1)], s.A[s.at(1, 2)], s.n_sinks, s.n_valid, sink_sum(s));
    }
    {   // ties go to the lowest k: a 3 x 3 with the centre above its neighbours
        std::vector<double> z(9, 4.0);
        z[4] = 5.0;
        std::printf("tie_dir_square %d\n", solve(3, 3, z, 1.0, 1.0).dir[4]);         // E, S, W, N tie at 1: E
        std::printf("tie_dir_wide %d\n", solve(3, 3, z, 2.0, 1.0).dir[4]);           // S and N tie at 1, E and W 0.5: S
        z[1] = z[3] = z[5] = z[7] = 5.0;
        std::printf("tie_dir_diag %d\n", solve(3, 3, z, 1.0, 1.0).dir[4]);           // the four diagonals tie: SE
    }
    {   // TWI of the hand 3 x 3 of the terrain table (dx = 2, dy = 4): slope_tan = sqrt(0.5625^2 + 0.78125^2), A = 7
        const double w9[9] = {1, 2, 3, 4, 5, 6, 7, 8, 10};
        std::printf("twi_hand %.17g\ntwi_floor %.17g\n", mhs::hydro_twi(w9, 7.0, 2.0, 4.0, 1.0, 0.001), mhs::hydro_twi(w9, 7.0, 2.0, 4.0, 1.0, 2.0));
    }
    std::printf("OK\n");
    return 0;
}
