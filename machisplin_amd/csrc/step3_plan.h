// The three rules of the reference-tiled Step 3 (V73:636-747), stated once for its drivers (tps_surface.hip, tps_se.hip, multi.hip):
// the cut of the grid into fit and keep windows, a tile's stations, the place of its keep-window plane in a packed buffer (tiles.hip)
#pragma once
#include "common.h"

namespace mhs {

constexpr double STEP3_FIT_OVERLAP = 0.2;      // V73:673: the fit box reaches 20 % of a tile's size into its neighbours
constexpr double STEP3_KEEP_OVERLAP = 0.025;   // V73:680: the kept box 2.5 %
constexpr int64_t STEP3_MIN_STATIONS = 10;     // V73:710-721: a tile with fewer stations gets no spline

struct Step3Plan {
    int64_t nRx = 1, nCx = 1, nt = 1;
    std::vector<int64_t> fit, keep;            // per tile (r0, r1, c0, c1) in grid rows / columns; empty in the global plan
    // cells of tile h's keep-window plane in a packed buffer: rounded up to 32 doubles, so that every plane starts on a 256-byte line
    size_t cells(int64_t h) const {
        const int64_t *k = &keep[(size_t)h * 4];
        return ((size_t)((k[1] - k[0]) * (k[3] - k[2])) + 31) & ~(size_t)31;
    }
    // every tile's plane one behind the other: its offset in doubles, and the buffer's size as entry nt
    std::vector<size_t> pack() const {
        std::vector<size_t> off((size_t)nt + 1, 0);
        for (int64_t h = 0; h < nt; ++h) off[(size_t)h + 1] = off[(size_t)h] + cells(h);
        return off;
    }
    // terra::rast(rb): the fit raster of tile h, whose cell centres the spline is evaluated on (V73:726) ...
    mhs_grid fit_grid(const mhs_grid *g, int64_t h) const;
    // ... and the keep window in that raster's rows and columns
    void keep_in_fit(int64_t h, int64_t *r0, int64_t *r1, int64_t *c0, int64_t *c1) const {
        const int64_t *f = &fit[(size_t)h * 4], *k = &keep[(size_t)h * 4];
        *r0 = k[0] - f[0]; *r1 = k[1] - f[0]; *c0 = k[2] - f[2]; *c1 = k[3] - f[2];
    }
};

// tile_edge > 0: the ceil(nrow / tile_edge) x ceil(ncol / tile_edge) tiles and their windows; tile_edge <= 0: the global fit's
// 1 x 1 plan, no windows (V73:748-753).  P is a fresh plan.
int step3_plan(const mhs_grid *g, int64_t tile_edge, Step3Plan &P);

// The stations of tile h (terra::extract(rb[[1]], Full.cords) + complete.cases, V73:701-706): those whose cell (rows / cols,
// mhs_cells_from_xy) lies in the fit window, covariate 1 (cov1, may be NULL) and the residual not NA -- in input order,
// txy = x block then y block, sr = their residuals.  Fewer than STEP3_MIN_STATIONS: the caller fits no spline.
void step3_stations(const Step3Plan &P, int64_t h, const int64_t *rows, const int64_t *cols, const double *xy, const double *resid,
                    const double *cov1, int64_t n, std::vector<double> &txy, std::vector<double> &sr);

}  // namespace mhs
