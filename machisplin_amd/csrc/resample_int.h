// What the kernels that read a source stack through resample_rule.h share (resample.hip, warp.hip): the description of the
// source, the accessors that check their indices before they read, the tile shape of the interpolating kernels and the checks
// of a source grid and stack that every entry point makes before its first device call.
#pragma once

#include <algorithm>
#include <cmath>
#include "ensemble_int.h"
#include "resample_rule.h"

namespace mhs {

constexpr int RS_NT = 256;
constexpr int RS_TH = 32, RS_TW = 64;
constexpr int RS_ROWS = RS_TH / 4;
constexpr int RS_STAGE_BYTES = 48 * 1024;       // the staged rectangle

struct RsSrc {
    const void *data;        // element (0, 0) of layer 0 (a row band's buffer: moved back to absolute row 0)
    int64_t ld, plane_stride;
    int C;
    int row_lo, row_hi;      // the rows that are resident: [0, nrow), or a host band's
    double nodata;
    int has_nodata;
    RsGrid g;
};

template <typename T>
struct GlobalAcc {
    const T *plane;
    int64_t ld;
    int row_lo, row_hi, ncol;
    bool has_nodata;
    double nodata;
    __device__ bool get(int i, int j, double &z) const {
        if (i < row_lo || i >= row_hi || j < 0 || j >= ncol) return false;
        z = (double)plane[(int64_t)i * ld + j];
        return !rs_na(z, has_nodata, nodata);
    }
};

template <typename T>
struct LdsAcc {
    const T *sm;
    int ti0, tj0, lh, lw;    // the staged rectangle: source rows [ti0, ti0 + lh) x columns [tj0, tj0 + lw), all inside the raster
    bool has_nodata;
    double nodata;
    __device__ bool get(int i, int j, double &z) const {
        const int li = i - ti0, lj = j - tj0;
        if ((unsigned)li >= (unsigned)lh || (unsigned)lj >= (unsigned)lw) return false;
        z = (double)sm[li * lw + lj];
        return !rs_na(z, has_nodata, nodata);
    }
};

template <typename T>
__device__ inline GlobalAcc<T> global_acc(const RsSrc &S, int k) {
    return GlobalAcc<T>{(const T *)S.data + (int64_t)k * S.plane_stride, S.ld, S.row_lo, S.row_hi, S.g.ncol, S.has_nodata != 0, S.nodata};
}

inline unsigned rs_blocks(int64_t n_tiles) {
    const int n_cu = ctx().n_cu > 0 ? ctx().n_cu : 256;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(n_tiles, (int64_t)n_cu * 32));
}

#define RS_REQUIRE(cond, ...)                                              \
    do {                                                                   \
        if (!(cond)) { set_error(__VA_ARGS__); return MHS_ERR_INVALID; }    \
    } while (0)

inline int rs_check_grid(const char *fn, const char *which, const mhs_grid *g, RsGrid *o) {
    RS_REQUIRE(g, "%s: NULL argument (%s grid)", fn, which);
    RS_REQUIRE(g->nrow > 0 && g->ncol > 0 && g->nrow < (1LL << 30) && g->ncol < (1LL << 30), "%s: bad %s grid dimension (nrow, ncol must be in 1 .. 2^30)", fn, which);
    RS_REQUIRE(std::isfinite(g->xres) && g->xres > 0.0 && std::isfinite(g->yres) && g->yres > 0.0, "%s: the %s grid's cell size must be finite and positive", fn, which);
    RS_REQUIRE(std::isfinite(g->xmin) && std::isfinite(g->ymax), "%s: the %s grid's origin must be finite", fn, which);
    *o = RsGrid{g->xmin, g->ymax, g->xres, g->yres, (int)g->nrow, (int)g->ncol};
    return MHS_OK;
}

// the source of a call: every check of grid and stack, before any device call
inline int rs_check_src(const char *fn, const mhs_grid *sg, const mhs_stack *ss, RsSrc *S) {
    RsGrid g;
    if (int rc = rs_check_grid(fn, "source", sg, &g)) return rc;
    RS_REQUIRE(ss, "%s: NULL argument (source stack)", fn);
    RS_REQUIRE(ss->data, "%s: the source stack's data is NULL", fn);
    RS_REQUIRE(ss->dtype == MHS_F64 || ss->dtype == MHS_F32 || ss->dtype == MHS_I16, "%s: bad stack dtype", fn);
    RS_REQUIRE(ss->n_layers >= 1, "%s: the source stack has no layer", fn);
    RS_REQUIRE(ss->ld >= sg->ncol && (ss->n_layers == 1 || ss->plane_stride >= ss->ld * (sg->nrow - 1) + sg->ncol), "%s: stack strides smaller than the source grid", fn);
    *S = RsSrc{ss->data, ss->ld, ss->plane_stride, ss->n_layers, 0, g.nrow, ss->nodata, !std::isnan(ss->nodata), g};
    return MHS_OK;
}

}  // namespace mhs
