// The patches rule of csrc/patches_rule.h in a plain C++ program: the header the kernels are built from is compiled here with
// gcc (no HIP), under AddressSanitizer and UBSan, and drives the HOST side of the rule -- the run heads from a row's bits, the
// links between two rows, the sequential union-find, the tile and border decomposition run tile by tile, the flatten, the
// counts through the packed table word, the filter -- over grids made by a 64-bit congruential generator that
// tests/test_patches_host.py restates.  It prints
//   run bits c start length          for a table of rows and columns
//   case k nrow ncol where threshold connectivity min_size max_size edge_rule checksum n_features n_patches n_kept_patches
//        n_kept_cells max_size       one line per grid: the sum over the five planes' cells of value * (2 i + 1) mod 2^64
// and then OK; the test holds every line against the numpy restatement (tests/patches_ref.py).
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <vector>

#include "patches_rule.h"

using namespace mhs;

static uint64_t lcg_state;
static uint32_t lcg() {
    lcg_state = lcg_state * 6364136223846793005ULL + 1442695040888963407ULL;
    return (uint32_t)(lcg_state >> 33);
}

// the words of a tile, or of the plane, in a host vector: every access is bounds-checked
struct HostWords {
    std::vector<int> &w;
    int load(int i) const { return w.at((size_t)i); }
    int fetch_min(int i, int v) {
        const int old = w.at((size_t)i);
        if (v < old) w.at((size_t)i) = v;
        return old;
    }
};

int main() {
    const uint64_t rows[] = {0x1ULL, 0x8000000000000000ULL, 0xffffffffffffffffULL, 0x00f0ff0ff00f0f01ULL, 0x7ffffffffffffffeULL, 0xaaaaaaaaaaaaaaaaULL};
    for (uint64_t m : rows)
        for (int c = 0; c < 64; ++c)
            if (patch_bit(m, c)) std::printf("run %" PRIu64 " %d %d %d\n", m, c, patch_run_start(m, c), patch_run_length(m, c));

    const int R = PATCH_TILE_ROWS, Cc = PATCH_TILE_COLS;
    const int shapes[][2] = {{1, 1}, {1, Cc + 1}, {R + 1, 1}, {R - 1, Cc - 1}, {R, Cc}, {R + 1, Cc + 1}, {2 * R + 3, 2 * Cc + 5}, {13, 20}};
    const double thresholds[] = {0.0, 10.0, 41.0, 59.0, 100.0};
    int k = 0;
    for (const auto &sh : shapes)
        for (double threshold : thresholds)
            for (int connectivity = 4; connectivity <= 8; connectivity += 4, ++k) {
                const int nrow = sh[0], ncol = sh[1], where = (k % 5 == 4) ? PROX_NA : PROX_LT;
                const int64_t min_size = 1 + k % 3, max_size = (k % 4 == 0) ? (int64_t)nrow * ncol : 40;
                const int edge_rule = k % PATCH_EDGE_RULES;
                const size_t n = (size_t)nrow * ncol;
                lcg_state = 7000 + (uint64_t)k;
                std::vector<double> z(n);
                for (double &v : z) {
                    const uint32_t q = lcg() % 100;
                    v = (where == PROX_NA && (double)q < threshold) ? (q % 2 ? NAN : -9.0) : (double)q;       // -9 is the nodata value
                }
                // 1: tile by tile
                std::vector<int> label(n, -2);
                std::vector<uint32_t> table(n, 0xdeadbeefu);
                int64_t n_features = 0;
                const int tiles_r = (nrow + R - 1) / R, tiles_c = (ncol + Cc - 1) / Cc;
                for (int tr = 0; tr < tiles_r; ++tr)
                    for (int tc = 0; tc < tiles_c; ++tc) {
                        const int r0 = tr * R, c0 = tc * Cc;
                        std::vector<uint64_t> bits((size_t)R, 0);
                        std::vector<int> words((size_t)R * Cc, -1);
                        std::vector<uint32_t> agg((size_t)R * Cc, 0);
                        HostWords a{words};
                        for (int lr = 0; lr < R; ++lr)
                            for (int l = 0; l < Cc; ++l) {
                                const int r = r0 + lr, c = c0 + l;
                                if (r < nrow && c < ncol && prox_is_feature(z[(size_t)r * ncol + c], true, -9.0, where, threshold))
                                    bits[(size_t)lr] |= 1ull << l;
                            }
                        for (int lr = 0; lr < R; ++lr)
                            for (int l = 0; l < Cc; ++l)
                                if (patch_bit(bits[(size_t)lr], l)) { words[(size_t)lr * Cc + l] = lr * Cc + patch_run_start(bits[(size_t)lr], l); ++n_features; }
                        for (int lr = 1; lr < R; ++lr)
                            for (int l = 0; l < Cc; ++l) {
                                if (!patch_bit(bits[(size_t)lr], l)) continue;
                                const int links = patch_up_links(bits[(size_t)lr], bits[(size_t)lr - 1], l, connectivity);
                                const int me = lr * Cc + l, above = me - Cc;
                                if (links & 1) patch_union(a, me, above);
                                if (links & 2) patch_union(a, me, above - 1);
                                if (links & 4) patch_union(a, me, above + 1);
                            }
                        for (int lr = 0; lr < R; ++lr)
                            for (int l = 0; l < Cc; ++l) {
                                const int r = r0 + lr, c = c0 + l;
                                if (r >= nrow || c >= ncol) continue;
                                const uint64_t m = bits[(size_t)lr];
                                if (!patch_bit(m, l)) { label[(size_t)r * ncol + c] = -1; continue; }
                                const int root = patch_find(a, lr * Cc + l);
                                label[(size_t)r * ncol + c] = (r0 + root / Cc) * ncol + c0 + root % Cc;
                                if (patch_run_start(m, l) == l) {
                                    const int len = patch_run_length(m, l);
                                    agg[(size_t)root] += (uint32_t)len;
                                    if (r == 0 || r == nrow - 1 || c == 0 || c + len == ncol) agg[(size_t)root] |= PATCH_EDGE_BIT;
                                }
                            }
                        for (int lr = 0; lr < R; ++lr)
                            for (int l = 0; l < Cc; ++l) {
                                const int r = r0 + lr, c = c0 + l;
                                if (r < nrow && c < ncol) table[(size_t)r * ncol + c] = words[(size_t)lr * Cc + l] == lr * Cc + l ? agg[(size_t)lr * Cc + l] : 0u;
                            }
                    }
                // the invariant after phase 1, and behind every later phase
                auto descends = [&]() {
                    for (size_t i = 0; i < n; ++i)
                        if (label[i] < -1 || label[i] > (int)i) return false;
                    return true;
                };
                if (!descends()) { std::printf("case %d: a word above its index after the tiles\n", k); return 1; }
                // 2: the borders
                HostWords a{label};
                auto feat = [&](int r, int c) { return label.at((size_t)r * ncol + c) >= 0; };
                const int64_t n_south = (int64_t)((nrow - 1) / R) * ncol, n_east = (int64_t)((ncol - 1) / Cc) * nrow;
                for (int64_t t = 0; t < n_south + n_east; ++t) {
                    if (t < n_south) {
                        const int r = (int)(t / ncol) * R + R - 1, c = (int)(t % ncol);
                        if (!feat(r, c)) continue;
                        const int me = r * ncol + c, below = me + ncol;
                        const bool s = feat(r + 1, c), w = c > 0 && feat(r, c - 1), e = c + 1 < ncol && feat(r, c + 1);
                        const bool sw = c > 0 && feat(r + 1, c - 1), se = c + 1 < ncol && feat(r + 1, c + 1);
                        if (s && patch_south_link(w, sw, c)) patch_union(a, me, below);
                        if (connectivity == 8) {
                            if (sw && patch_diagonal_link(w, s)) patch_union(a, me, below - 1);
                            if (se && patch_diagonal_link(e, s)) patch_union(a, me, below + 1);
                        }
                    } else {
                        const int64_t u = t - n_south;
                        const int c = (int)(u / nrow) * Cc + Cc - 1, r = (int)(u % nrow);
                        if (!feat(r, c)) continue;
                        const int me = r * ncol + c;
                        const bool e = feat(r, c + 1);
                        if (e) patch_union(a, me, me + 1);
                        if (connectivity == 8) {
                            if (r > 0 && feat(r - 1, c + 1) && patch_diagonal_link(feat(r - 1, c), e)) patch_union(a, me, me - ncol + 1);
                            if (r + 1 < nrow && feat(r + 1, c + 1) && patch_diagonal_link(feat(r + 1, c), e)) patch_union(a, me, me + ncol + 1);
                        }
                    }
                }
                if (!descends()) { std::printf("case %d: a word above its index after the borders\n", k); return 1; }
                // 3: flatten
                for (size_t i = 0; i < n; ++i)
                    if (label[i] >= 0) label[i] = patch_find(a, label[i]);
                if (!descends()) { std::printf("case %d: a word above its index after the flatten\n", k); return 1; }
                // 4: counts
                for (size_t i = 0; i < n; ++i) {
                    const uint32_t t = table[i];
                    if (t == 0 || label[i] == (int)i) continue;
                    table.at((size_t)label[i]) += t & PATCH_SIZE_MASK;
                    table.at((size_t)label[i]) |= t & PATCH_EDGE_BIT;
                }
                // 5: ids, in the order of the roots
                std::vector<int> ids(n, 0);
                int64_t n_patches = 0, n_kept = 0, n_kept_cells = 0, biggest = 0;
                for (size_t i = 0; i < n; ++i) {
                    if (label[i] != (int)i) continue;
                    ids[i] = (int)++n_patches;
                    const int size = patch_size_of(table[i]);
                    if (size > biggest) biggest = size;
                    if (patch_keep(size, patch_edge_of(table[i]), min_size, max_size, edge_rule)) { ++n_kept; n_kept_cells += size; }
                }
                // 6: products
                uint64_t sum = 0, i5 = 0;
                for (size_t i = 0; i < n; ++i) {
                    const int root = label[i];
                    const uint32_t t = root >= 0 ? table.at((size_t)root) : 0u;
                    const int64_t x[5] = {root, root >= 0 ? ids.at((size_t)root) : 0, patch_size_of(t), root >= 0 ? patch_edge_of(t) : 0,
                                          root >= 0 && patch_keep(patch_size_of(t), patch_edge_of(t), min_size, max_size, edge_rule)};
                    for (int64_t b : x) { sum += (uint64_t)b * (2 * i5 + 1); ++i5; }
                }
                std::printf("case %d %d %d %d %g %d %" PRId64 " %" PRId64 " %d %" PRIu64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", k, nrow,
                            ncol, where, threshold, connectivity, min_size, max_size, edge_rule, sum, n_features, n_patches, n_kept, n_kept_cells, biggest);
            }
    std::printf("OK\n");
    return 0;
}
