/* .Call() shim: binds R to the C ABI of include/machisplin_hip.h.  UNTESTED HERE (no R in the
 * build image); it is mechanically derived from the header: every SEXP is unpacked with
 * REAL()/INTEGER(), the library is called, a non-zero status becomes Rf_error() AFTER all C
 * resources are released, handles are external pointers with finalizers.
 *
 * Build inside the R package:  PKG_CPPFLAGS=-I<repo>/include  PKG_LIBS=-L<repo>/machisplin_amd -lmachisplin_hip
 */
#include <R.h>
#include <Rinternals.h>
#include <stdint.h>
#include <string.h>
#include "machisplin_hip.h"

static void chk(int rc) { if (rc != MHS_OK) Rf_error("machisplin_hip: %s", mhs_last_error()); }

static mhs_grid grid_from(SEXP geom) { /* c(xmin, ymax, xres, yres, nrow, ncol) */
    double *g = REAL(geom);
    mhs_grid out = { g[0], g[1], g[2], g[3], (int64_t)g[4], (int64_t)g[5] };
    return out;
}

static void tps_finalizer(SEXP p) { mhs_tps_free((mhs_tps *)R_ExternalPtrAddr(p)); R_ClearExternalPtr(p); }
static void model_finalizer(SEXP p) { mhs_model_free((mhs_model *)R_ExternalPtrAddr(p)); R_ClearExternalPtr(p); }
static SEXP wrap(void *h, R_CFinalizer_t fin) {
    SEXP p = PROTECT(R_MakeExternalPtr(h, R_NilValue, R_NilValue));
    R_RegisterCFinalizerEx(p, fin, TRUE);
    UNPROTECT(1);
    return p;
}

SEXP mhsr_init(SEXP device) { chk(mhs_init(Rf_asInteger(device))); return R_NilValue; }
/* 0 = by cost (default), 1 = direct sum (predict.Krig's own loop; bit-identical across windows), 2 = far-field-
   interpolated sum; see mhs_tps_eval_mode in machisplin_hip.h */
SEXP mhsr_tps_eval_mode(SEXP mode) { chk(mhs_tps_eval_mode(Rf_asInteger(mode))); return R_NilValue; }
/* the standard errors' limit on distinct stations (returns the value it replaces) and where Q = -M^-1 is built
   (0 auto, 1 host, 2 device); see mhs_tps_se_max_n / mhs_tps_se_build_mode in machisplin_hip.h */
SEXP mhsr_tps_se_max_n(SEXP n) {
    int64_t prev = 0;
    chk(mhs_tps_se_max_n((int64_t)Rf_asReal(n), &prev));
    return Rf_ScalarReal((double)prev);
}
SEXP mhsr_tps_se_build_mode(SEXP mode) { chk(mhs_tps_se_build_mode(Rf_asInteger(mode))); return R_NilValue; }

/* fields::Tps(x, Y)  (V73:722, V73:751).  xy: n x 2 numeric matrix, lambda NA => GCV */
SEXP mhsr_tps_fit(SEXP xy, SEXP y, SEXP lambda, SEXP mode) {
    mhs_tps *t = NULL;
    double lam = Rf_asReal(lambda);
    chk(mhs_tps_fit(REAL(xy), REAL(y), (int64_t)Rf_length(y), ISNA(lam) ? R_NaN : lam, Rf_asInteger(mode), &t));
    return wrap(t, tps_finalizer);
}

/* lapply(seq_along(xs), function(k) fields::Tps(xs[[k]], ys[[k]])) in ONE library call (the tiles of V73:690-738, or the
 * response layers of one station table): xs a list of n_k x 2 numeric matrices, ys a list of numeric vectors.  Every fit with
 * 8..256 distinct locations is done by one kernel launch, a workgroup per fit (mhs_tps_fit_many).  Returns a list of external
 * pointers, NULL where a fit failed (collinear stations, ...). */
SEXP mhsr_tps_fit_many(SEXP xs, SEXP ys, SEXP lambda, SEXP mode) {
    const R_xlen_t k = Rf_xlength(xs);
    double lam = Rf_asReal(lambda);
    const double **px = (const double **)R_alloc((size_t)(k ? k : 1), sizeof(double *));
    const double **py = (const double **)R_alloc((size_t)(k ? k : 1), sizeof(double *));
    int64_t *n = (int64_t *)R_alloc((size_t)(k ? k : 1), sizeof(int64_t));
    mhs_tps **h = (mhs_tps **)R_alloc((size_t)(k ? k : 1), sizeof(mhs_tps *));
    int *st = (int *)R_alloc((size_t)(k ? k : 1), sizeof(int));
    if (Rf_xlength(ys) != k) Rf_error("mhsr_tps_fit_many: xs and ys have different lengths");
    for (R_xlen_t i = 0; i < k; ++i) {
        SEXP x = VECTOR_ELT(xs, i), y = VECTOR_ELT(ys, i);
        if (Rf_xlength(x) != 2 * Rf_xlength(y)) Rf_error("mhsr_tps_fit_many: element %d: x must be an n x 2 matrix beside n values", (int)i + 1);
        px[i] = REAL(x); py[i] = REAL(y); n[i] = (int64_t)Rf_xlength(y); h[i] = NULL;
    }
    SEXP out = PROTECT(Rf_allocVector(VECSXP, k));
    int rc = mhs_tps_fit_many(px, py, n, (int64_t)k, ISNA(lam) ? R_NaN : lam, Rf_asInteger(mode), h, st);
    /* every handle gets its owner BEFORE an error can unwind: nothing leaks */
    for (R_xlen_t i = 0; i < k; ++i)
        if (h[i]) SET_VECTOR_ELT(out, i, wrap(h[i], tps_finalizer));
    UNPROTECT(1);
    chk(rc);
    return out;
}

/* predict(tps, xy): the spline at arbitrary points -- what terra::interpolate feeds an S3 predict method
 * block by block; xy is an n x 2 numeric matrix */
SEXP mhsr_tps_predict_points(SEXP tps, SEXP xy) {
    R_xlen_t n = Rf_xlength(xy) / 2;
    SEXP out = PROTECT(Rf_allocVector(REALSXP, n));
    int rc = mhs_tps_predict_points((mhs_tps *)R_ExternalPtrAddr(tps), REAL(xy), (int64_t)n, REAL(out));
    UNPROTECT(1);
    chk(rc);
    return out;
}

/* terra::interpolate(terra::rast(rb), tps)  (V73:726, V73:753): values in terra cell order */
SEXP mhsr_tps_predict_grid(SEXP tps, SEXP geom, SEXP win) {
    mhs_grid g = grid_from(geom);
    int *w = INTEGER(win); /* r0, r1, c0, c1 (0-based, half-open) */
    SEXP out = PROTECT(Rf_allocVector(REALSXP, (R_xlen_t)(w[1] - w[0]) * (w[3] - w[2])));
    int rc = mhs_tps_predict_grid((mhs_tps *)R_ExternalPtrAddr(tps), &g, w[0], w[1], w[2], w[3], REAL(out));
    UNPROTECT(1);
    chk(rc);
    return out;
}

/* Step 3 + Step 4 in one call (V73:636-897) */
SEXP mhsr_tps_surface(SEXP geom, SEXP xy, SEXP resid, SEXP cov1, SEXP tile_edge, SEXP lambda, SEXP mode) {
    mhs_grid g = grid_from(geom);
    double lam = Rf_asReal(lambda);
    SEXP out = PROTECT(Rf_allocVector(REALSXP, (R_xlen_t)g.nrow * g.ncol));
    int rc = mhs_tps_surface(&g, REAL(xy), REAL(resid), (int64_t)Rf_length(resid),
                             Rf_isNull(cov1) ? NULL : REAL(cov1), (int64_t)Rf_asInteger(tile_edge),
                             ISNA(lam) ? R_NaN : lam, Rf_asInteger(mode), REAL(out), NULL);
    UNPROTECT(1);
    chk(rc);
    return out;
}

/* fields::predictSE.Krig (machisplin_hip.h "TPS standard errors"); sigma2 NA => the fit's own sigma^2 hat */
static double sigma2_from(SEXP sigma2) {
    double s = Rf_asReal(sigma2);
    return ISNA(s) ? R_NaN : s;
}
SEXP mhsr_tps_sigma2(SEXP tps) {
    double s2 = 0;
    chk(mhs_tps_sigma2((mhs_tps *)R_ExternalPtrAddr(tps), &s2));
    return Rf_ScalarReal(s2);
}
/* predictSE(fit, x) */
SEXP mhsr_tps_predict_se_points(SEXP tps, SEXP xy, SEXP sigma2) {
    R_xlen_t n = Rf_xlength(xy) / 2;
    SEXP out = PROTECT(Rf_allocVector(REALSXP, n));
    int rc = mhs_tps_predict_se_points((mhs_tps *)R_ExternalPtrAddr(tps), REAL(xy), (int64_t)n, sigma2_from(sigma2), REAL(out));
    UNPROTECT(1);
    chk(rc);
    return out;
}
/* terra::interpolate(r, fit, fun = predictSE): values in terra cell order */
SEXP mhsr_tps_predict_se_grid(SEXP tps, SEXP geom, SEXP win, SEXP sigma2) {
    mhs_grid g = grid_from(geom);
    int *w = INTEGER(win); /* r0, r1, c0, c1 (0-based, half-open) */
    SEXP out = PROTECT(Rf_allocVector(REALSXP, (R_xlen_t)(w[1] - w[0]) * (w[3] - w[2])));
    int rc = mhs_tps_predict_se_grid((mhs_tps *)R_ExternalPtrAddr(tps), &g, w[0], w[1], w[2], w[3], sigma2_from(sigma2), REAL(out));
    UNPROTECT(1);
    chk(rc);
    return out;
}
/* the SE plane of Step 3 + Step 4 (mhsr_tps_surface's arguments) */
SEXP mhsr_tps_surface_se(SEXP geom, SEXP xy, SEXP resid, SEXP cov1, SEXP tile_edge, SEXP lambda, SEXP mode) {
    mhs_grid g = grid_from(geom);
    double lam = Rf_asReal(lambda);
    SEXP out = PROTECT(Rf_allocVector(REALSXP, (R_xlen_t)g.nrow * g.ncol));
    int rc = mhs_tps_surface_se(&g, REAL(xy), REAL(resid), (int64_t)Rf_length(resid),
                                Rf_isNull(cov1) ? NULL : REAL(cov1), (int64_t)Rf_asInteger(tile_edge),
                                ISNA(lam) ? R_NaN : lam, Rf_asInteger(mode), REAL(out), NULL);
    UNPROTECT(1);
    chk(rc);
    return out;
}

/* model loaders: flat arrays pulled out of the fitted objects by R/backend_hip.R */
SEXP mhsr_lm_load(SEXP coef) {
    mhs_model *m = NULL;
    chk(mhs_lm_load(REAL(coef), Rf_length(coef) - 1, &m));
    return wrap(m, model_finalizer);
}
SEXP mhsr_nnet_load(SEXP wts, SEXP p, SEXP size, SEXP scale, SEXP shift) {
    mhs_model *m = NULL;
    chk(mhs_nnet_load(REAL(wts), Rf_asInteger(p), Rf_asInteger(size), Rf_asReal(scale), Rf_asReal(shift), &m));
    return wrap(m, model_finalizer);
}
SEXP mhsr_earth_load(SEXP coef, SEXP dirs_rowmajor, SEXP cuts_rowmajor, SEXP p) {
    mhs_model *m = NULL;
    chk(mhs_earth_load(REAL(coef), INTEGER(dirs_rowmajor), REAL(cuts_rowmajor), Rf_length(coef), Rf_asInteger(p), &m));
    return wrap(m, model_finalizer);
}
SEXP mhsr_svr_load(SEXP alpha, SEXP sv_rowmajor, SEXP p, SEXP b, SEXP sigma, SEXP xc, SEXP xs, SEXP yc, SEXP ys) {
    mhs_model *m = NULL;
    chk(mhs_svr_load(REAL(alpha), REAL(sv_rowmajor), (int64_t)Rf_length(alpha), Rf_asInteger(p), Rf_asReal(b),
                     Rf_asReal(sigma), REAL(xc), REAL(xs), Rf_asReal(yc), Rf_asReal(ys), &m));
    return wrap(m, model_finalizer);
}
SEXP mhsr_gbm_load(SEXP initF, SEXP offsets /* numeric, n.trees+1 */, SEXP var, SEXP val, SEXP left, SEXP right,
                   SEXP missing, SEXP p) {
    R_xlen_t nt = Rf_xlength(offsets) - 1;
    int64_t *off = (int64_t *)R_alloc((size_t)nt + 1, sizeof(int64_t));
    for (R_xlen_t i = 0; i <= nt; ++i) off[i] = (int64_t)REAL(offsets)[i];
    mhs_model *m = NULL;
    chk(mhs_gbm_load(Rf_asReal(initF), (int64_t)nt, off, INTEGER(var), REAL(val), INTEGER(left), INTEGER(right),
                     INTEGER(missing), Rf_asInteger(p), &m));
    return wrap(m, model_finalizer);
}
SEXP mhsr_rf_load(SEXP offsets, SEXP left, SEXP right, SEXP status, SEXP bestvar, SEXP split, SEXP nodepred, SEXP p) {
    R_xlen_t nt = Rf_xlength(offsets) - 1;
    int64_t *off = (int64_t *)R_alloc((size_t)nt + 1, sizeof(int64_t));
    for (R_xlen_t i = 0; i <= nt; ++i) off[i] = (int64_t)REAL(offsets)[i];
    mhs_model *m = NULL;
    chk(mhs_rf_load((int64_t)nt, off, INTEGER(left), INTEGER(right), INTEGER(status), INTEGER(bestvar), REAL(split),
                    REAL(nodepred), Rf_asInteger(p), &m));
    return wrap(m, model_finalizer);
}

/* the Step-2 raster loop (V73:447-619).  covars: terra::values(covar.ras), an ncell x C numeric
 * matrix -- column-major, i.e. already planar; NA_real_ is a NaN and is treated as NA */
SEXP mhsr_ensemble_predict(SEXP models, SEXP weights, SEXP wt_total, SEXP geom, SEXP covars) {
    mhs_grid g = grid_from(geom);
    int n = Rf_length(models);
    const mhs_model **h = (const mhs_model **)R_alloc((size_t)n, sizeof(*h));
    for (int i = 0; i < n; ++i) h[i] = (const mhs_model *)R_ExternalPtrAddr(VECTOR_ELT(models, i));
    mhs_stack st = { REAL(covars), Rf_ncols(covars), MHS_F64, (int64_t)g.nrow * g.ncol, g.ncol, R_NaN };
    SEXP out = PROTECT(Rf_allocVector(REALSXP, (R_xlen_t)g.nrow * g.ncol));
    int rc = mhs_ensemble_predict(h, REAL(weights), n, Rf_asReal(wt_total), &g, &st, 0, g.nrow, 0, g.ncol, REAL(out));
    UNPROTECT(1);
    chk(rc);
    return out;
}

/* dismo::mess(covar.ras, ref, full = TRUE) (machisplin_hip.h "MESS extrapolation map").  ref: n_ref x V numeric matrix, the
 * stations' covariate columns (V = C) or those plus LONG and LAT (V = C + 2); covars: terra::values(covar.ras), ncell x C.
 * Returns list(mess, mod) in terra cell order: the MESS values (NaN at NA cells) and the integer most dissimilar
 * variable, 0-based as the library counts it, -1 at NA cells. */
SEXP mhsr_mess_grid(SEXP ref, SEXP geom, SEXP covars) {
    mhs_grid g = grid_from(geom);
    mhs_mess *m = NULL;
    mhs_stack st = { REAL(covars), Rf_ncols(covars), MHS_F64, (int64_t)g.nrow * g.ncol, g.ncol, R_NaN };
    if ((int64_t)Rf_nrows(covars) != g.nrow * g.ncol) Rf_error("mhsr_mess_grid: covars must have one row per cell");
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 2));
    SEXP mess = PROTECT(Rf_allocVector(REALSXP, (R_xlen_t)g.nrow * g.ncol));
    SEXP mod = PROTECT(Rf_allocVector(INTSXP, (R_xlen_t)g.nrow * g.ncol));
    /* the handle lives only between here and mhs_mess_free: no R call in between can unwind past it */
    int rc = mhs_mess_create(REAL(ref), (int64_t)Rf_nrows(ref), Rf_ncols(ref), &m);
    if (rc == MHS_OK) rc = mhs_mess_grid(m, &g, &st, 0, g.nrow, 0, g.ncol, REAL(mess), INTEGER(mod));
    mhs_mess_free(m);
    SET_VECTOR_ELT(out, 0, mess);
    SET_VECTOR_ELT(out, 1, mod);
    UNPROTECT(3);
    chk(rc);
    return out;
}

/* Topographic covariates from a DEM (machisplin_hip.h "terrain"): what the package's README sends its users to SAGA, GRASS and
 * terra for.  dem: terra::values(dem.ras), one double per cell (NA_real_ = NA); units: c(dx, dy, z_factor); dx_row: NULL or
 * one cell width per row (a lon/lat raster: made in R, the library never calls cos).  All three run on the HOST entry points. */
static mhs_terrain_units units_from(SEXP units, SEXP dx_row, const mhs_grid *g, const char *who) {
    if (Rf_length(units) != 3) Rf_error("%s: units must be c(dx, dy, z_factor)", who);
    if (!Rf_isNull(dx_row) && (int64_t)Rf_length(dx_row) != g->nrow) Rf_error("%s: dx_row must have one width per row", who);
    mhs_terrain_units u = { REAL(units)[0], Rf_isNull(dx_row) ? NULL : REAL(dx_row), REAL(units)[1], REAL(units)[2] };
    return u;
}
static mhs_stack dem_from(SEXP dem, const mhs_grid *g, const char *who) {
    if ((int64_t)Rf_xlength(dem) != g->nrow * g->ncol) Rf_error("%s: dem must have one value per cell", who);
    mhs_stack st = { REAL(dem), 1, MHS_F64, (int64_t)g->nrow * g->ncol, g->ncol, R_NaN };
    return st;
}
static int mask_planes(int mask) { int n = 0; for (unsigned m = (unsigned)mask; m; m &= m - 1) ++n; return n; }

/* the 3 x 3 variables of the bit mask vars (bit 0 dzdx ... bit 9 roughness): an ncell x n matrix, columns in ascending bit order */
SEXP mhsr_terrain(SEXP geom, SEXP dem, SEXP units, SEXP dx_row, SEXP vars) {
    mhs_grid g = grid_from(geom);
    mhs_stack st = dem_from(dem, &g, "mhsr_terrain");
    mhs_terrain_units u = units_from(units, dx_row, &g, "mhsr_terrain");
    int mask = Rf_asInteger(vars), n = mask_planes(mask);
    if (mask == NA_INTEGER || mask < 0) Rf_error("mhsr_terrain: vars must be a bit mask");
    SEXP out = PROTECT(Rf_allocMatrix(REALSXP, (int)(g.nrow * g.ncol), n > 0 ? n : 1));
    int rc = mhs_terrain(&g, &st, 0, &u, 0, g.nrow, 0, g.ncol, (unsigned)mask, REAL(out), MHS_F64);
    UNPROTECT(1);
    chk(rc);
    return out;
}

/* relief in a circular window of `radius` cells, the statistics of the bit mask stats (1 above_min, 2 below_max, 4 minus_mean) */
SEXP mhsr_relief(SEXP geom, SEXP dem, SEXP z_factor, SEXP radius, SEXP stats) {
    mhs_grid g = grid_from(geom);
    mhs_stack st = dem_from(dem, &g, "mhsr_relief");
    mhs_terrain_units u = { 0.0, NULL, 0.0, Rf_asReal(z_factor) };
    int mask = Rf_asInteger(stats), n = mask_planes(mask);
    if (mask == NA_INTEGER || mask < 0) Rf_error("mhsr_relief: stats must be a bit mask");
    SEXP out = PROTECT(Rf_allocMatrix(REALSXP, (int)(g.nrow * g.ncol), n > 0 ? n : 1));
    int rc = mhs_relief(&g, &st, 0, &u, Rf_asInteger(radius), 0, g.nrow, 0, g.ncol, (unsigned)mask, REAL(out), MHS_F64);
    UNPROTECT(1);
    chk(rc);
    return out;
}

/* geomorphons: an integer vector of the forms 1 .. 10 in terra cell order, NA_integer_ at NA cells */
SEXP mhsr_geomorphon(SEXP geom, SEXP dem, SEXP units, SEXP dx_row, SEXP search, SEXP flat_deg) {
    mhs_grid g = grid_from(geom);
    mhs_stack st = dem_from(dem, &g, "mhsr_geomorphon");
    mhs_terrain_units u = units_from(units, dx_row, &g, "mhsr_geomorphon");
    R_xlen_t n = (R_xlen_t)g.nrow * g.ncol;
    SEXP out = PROTECT(Rf_allocVector(INTSXP, n));
    int16_t *forms = (int16_t *)R_alloc((size_t)(n ? n : 1), sizeof(int16_t));
    int rc = mhs_geomorphon(&g, &st, 0, &u, Rf_asInteger(search), Rf_asReal(flat_deg), 0, g.nrow, 0, g.ncol, forms);
    if (rc == MHS_OK)
        for (R_xlen_t k = 0; k < n; ++k) INTEGER(out)[k] = forms[k] == -32768 ? NA_INTEGER : (int)forms[k];
    UNPROTECT(1);
    chk(rc);
    return out;
}

/* Solar covariates of the DEM (machisplin_hip.h "solar"): products is a bit mask (1 svf, 2 direct, 4 sun_hours, 8 horizon), search
 * the length of the sixteen rays in cells.  tables: NULL (horizon alone) or list(entries, start, omega, tab_row) -- entries an
 * n x 8 numeric matrix with the columns t, tan_h, ux, uy, uz, w, d, pad, start n_tab * 16 + 1 offsets into its rows (0-based,
 * numeric or integer), omega n_tab * 16 weights, tab_row NULL or one 0-based table index per row of the raster (integer).
 * Returns an ncell x n matrix in terra cell order, columns in ascending bit order, horizon as sixteen columns N, NNE, ... NNW;
 * NaN at NA cells.  Runs on the HOST entry point. */
SEXP mhsr_solar(SEXP geom, SEXP dem, SEXP units, SEXP dx_row, SEXP search, SEXP products, SEXP tables) {
    mhs_grid g = grid_from(geom);
    mhs_stack st = dem_from(dem, &g, "mhsr_solar");
    mhs_terrain_units u = units_from(units, dx_row, &g, "mhsr_solar");
    int mask = Rf_asInteger(products);
    if (mask == NA_INTEGER || mask < 1 || mask > 15) Rf_error("mhsr_solar: products must be a bit mask of 1 svf, 2 direct, 4 sun_hours, 8 horizon");
    int n = mask_planes(mask & 7) + ((mask & 8) ? 16 : 0);
    mhs_sun_tables t = { 0, NULL, NULL, NULL, NULL };
    if (!Rf_isNull(tables)) {
        if (TYPEOF(tables) != VECSXP || Rf_length(tables) != 4) Rf_error("mhsr_solar: tables must be list(entries, start, omega, tab_row)");
        SEXP entries = VECTOR_ELT(tables, 0), start = VECTOR_ELT(tables, 1), omega = VECTOR_ELT(tables, 2), tab_row = VECTOR_ELT(tables, 3);
        if (!Rf_isReal(entries) || !Rf_isMatrix(entries) || Rf_ncols(entries) != 8) Rf_error("mhsr_solar: entries must be a numeric matrix of 8 columns");
        if (!Rf_isReal(omega) || Rf_length(omega) < 16 || Rf_length(omega) % 16) Rf_error("mhsr_solar: omega must hold 16 weights per table");
        int n_tab = Rf_length(omega) / 16, n_ent = Rf_nrows(entries), n_start = n_tab * 16 + 1;
        if (Rf_length(start) != n_start) Rf_error("mhsr_solar: start must hold 16 offsets per table and one more");
        int64_t *s64 = (int64_t *)R_alloc((size_t)n_start, sizeof(int64_t));
        for (int k = 0; k < n_start; ++k) {
            double v = TYPEOF(start) == INTSXP ? (double)INTEGER(start)[k] : REAL(start)[k];
            if (!(v >= 0.0 && v <= (double)n_ent)) Rf_error("mhsr_solar: start[%d] is not an offset into the %d rows of entries", k + 1, n_ent);
            s64[k] = (int64_t)v;
        }
        mhs_sun_entry *e = (mhs_sun_entry *)R_alloc((size_t)(n_ent ? n_ent : 1), sizeof(mhs_sun_entry));
        const double *m = REAL(entries);                 /* column-major */
        for (int i = 0; i < n_ent; ++i) {
            mhs_sun_entry r = { m[i], m[i + (size_t)n_ent], m[i + 2 * (size_t)n_ent], m[i + 3 * (size_t)n_ent], m[i + 4 * (size_t)n_ent],
                                m[i + 5 * (size_t)n_ent], m[i + 6 * (size_t)n_ent], 0.0 };
            e[i] = r;
        }
        if (!Rf_isNull(tab_row) && (TYPEOF(tab_row) != INTSXP || (int64_t)Rf_length(tab_row) != g.nrow))
            Rf_error("mhsr_solar: tab_row must be NULL or one integer table index per row");
        t.n_tab = n_tab; t.start = s64; t.entries = e; t.omega = REAL(omega);
        t.tab_row = Rf_isNull(tab_row) ? NULL : (const int32_t *)INTEGER(tab_row);
    }
    SEXP out = PROTECT(Rf_allocMatrix(REALSXP, (int)(g.nrow * g.ncol), n));
    int rc = mhs_solar(&g, &st, 0, &u, Rf_asInteger(search), Rf_isNull(tables) ? NULL : &t, 0, g.nrow, 0, g.ncol, (unsigned)mask, REAL(out), MHS_F64);
    UNPROTECT(1);
    chk(rc);
    return out;
}

/* Hydrology of the DEM (machisplin_hip.h "hydrology"): the bundled TWI.tif's recipe.  products: bit mask (1 filled, 2 flowdir,
 * 4 flowacc, 8 twi); opts: c(min_slope_tan, max_passes).  Returns list(filled, flowdir, flowacc, twi, info) in terra cell order,
 * NULL where a plane was not asked for: numeric vectors (NaN at NA cells), flowdir an integer vector (0 .. 7 = E, SE, S, SW, W,
 * NW, N, NE, -1 the water leaves, NA_integer_ at NA cells), info = c(passes_fill, passes_flat, passes_acc, n_valid, n_raised,
 * n_sinks).  Runs on the HOST entry point: the whole plane goes up, there are no row bands. */
SEXP mhsr_hydro(SEXP geom, SEXP dem, SEXP units, SEXP dx_row, SEXP products, SEXP opts) {
    mhs_grid g = grid_from(geom);
    mhs_stack st = dem_from(dem, &g, "mhsr_hydro");
    mhs_terrain_units u = units_from(units, dx_row, &g, "mhsr_hydro");
    int mask = Rf_asInteger(products);
    if (mask == NA_INTEGER || mask < 1 || mask > 15) Rf_error("mhsr_hydro: products must be a bit mask of 1 filled, 2 flowdir, 4 flowacc, 8 twi");
    if (Rf_length(opts) != 2) Rf_error("mhsr_hydro: opts must be c(min_slope_tan, max_passes)");
    if (!(REAL(opts)[1] >= 0.0 && REAL(opts)[1] <= 2147483647.0)) Rf_error("mhsr_hydro: max_passes must be 0 (the default cap) or a positive count");
    R_xlen_t n = (R_xlen_t)g.nrow * g.ncol;
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 5));
    SEXP plane[4] = { R_NilValue, R_NilValue, R_NilValue, R_NilValue };
    int n_protect = 1;
    for (int k = 0; k < 4; ++k)
        if (mask & (1 << k)) { plane[k] = PROTECT(Rf_allocVector(k == 1 ? INTSXP : REALSXP, n)); ++n_protect; }
    int8_t *dirs = (mask & 2) ? (int8_t *)R_alloc((size_t)(n ? n : 1), sizeof(int8_t)) : NULL;
    mhs_hydro_out o = { (mask & 1) ? REAL(plane[0]) : NULL, dirs, (mask & 4) ? REAL(plane[2]) : NULL, (mask & 8) ? REAL(plane[3]) : NULL };
    mhs_hydro_info info = { 0 };
    int rc = mhs_hydro(&g, &st, 0, &u, REAL(opts)[0], (int)REAL(opts)[1], &o, MHS_F64, &info);
    if (rc == MHS_OK) {
        if (dirs)
            for (R_xlen_t k = 0; k < n; ++k) INTEGER(plane[1])[k] = dirs[k] == -2 ? NA_INTEGER : (int)dirs[k];
        SEXP inf = PROTECT(Rf_allocVector(REALSXP, 6)); ++n_protect;
        REAL(inf)[0] = info.passes_fill; REAL(inf)[1] = info.passes_flat; REAL(inf)[2] = info.passes_acc;
        REAL(inf)[3] = (double)info.n_valid; REAL(inf)[4] = (double)info.n_raised; REAL(inf)[5] = (double)info.n_sinks;
        for (int k = 0; k < 4; ++k) SET_VECTOR_ELT(out, k, plane[k]);
        SET_VECTOR_ELT(out, 4, inf);
    }
    UNPROTECT(n_protect);
    chk(rc);
    return out;
}

/* The same with multiple flow direction (machisplin_hip.h "hydrology, multiple flow direction": what SAGA makes the bundled
 * TWI.tif with).  products: bit mask (1 filled, 2 flowacc, 4 twi); opts: c(min_slope_tan, max_passes, exponent).  Returns
 * list(filled, flowacc, twi, info), NULL where a plane was not asked for; info as mhsr_hydro's, passes_acc of the MFD
 * accumulation. */
SEXP mhsr_hydro_mfd(SEXP geom, SEXP dem, SEXP units, SEXP dx_row, SEXP products, SEXP opts) {
    mhs_grid g = grid_from(geom);
    mhs_stack st = dem_from(dem, &g, "mhsr_hydro_mfd");
    mhs_terrain_units u = units_from(units, dx_row, &g, "mhsr_hydro_mfd");
    int mask = Rf_asInteger(products);
    if (mask == NA_INTEGER || mask < 1 || mask > 7) Rf_error("mhsr_hydro_mfd: products must be a bit mask of 1 filled, 2 flowacc, 4 twi");
    if (Rf_length(opts) != 3) Rf_error("mhsr_hydro_mfd: opts must be c(min_slope_tan, max_passes, exponent)");
    if (!(REAL(opts)[1] >= 0.0 && REAL(opts)[1] <= 2147483647.0)) Rf_error("mhsr_hydro_mfd: max_passes must be 0 (the default cap) or a positive count");
    R_xlen_t n = (R_xlen_t)g.nrow * g.ncol;
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 4));
    SEXP plane[3] = { R_NilValue, R_NilValue, R_NilValue };
    int n_protect = 1;
    for (int k = 0; k < 3; ++k)
        if (mask & (1 << k)) { plane[k] = PROTECT(Rf_allocVector(REALSXP, n)); ++n_protect; }
    mhs_hydro_mfd_out o = { (mask & 1) ? REAL(plane[0]) : NULL, (mask & 2) ? REAL(plane[1]) : NULL, (mask & 4) ? REAL(plane[2]) : NULL };
    mhs_hydro_info info = { 0 };
    int rc = mhs_hydro_mfd(&g, &st, 0, &u, REAL(opts)[0], (int)REAL(opts)[1], REAL(opts)[2], &o, MHS_F64, &info);
    if (rc == MHS_OK) {
        SEXP inf = PROTECT(Rf_allocVector(REALSXP, 6)); ++n_protect;
        REAL(inf)[0] = info.passes_fill; REAL(inf)[1] = info.passes_flat; REAL(inf)[2] = info.passes_acc;
        REAL(inf)[3] = (double)info.n_valid; REAL(inf)[4] = (double)info.n_raised; REAL(inf)[5] = (double)info.n_sinks;
        for (int k = 0; k < 3; ++k) SET_VECTOR_ELT(out, k, plane[k]);
        SET_VECTOR_ELT(out, 3, inf);
    }
    UNPROTECT(n_protect);
    chk(rc);
    return out;
}

/* Rasters onto one grid (machisplin_hip.h "resample"): what the package's README sends its users to terra::crop, terra::resample
 * and terra::extract for.  planes: terra::values(src.ras), an ncell x C numeric matrix (or a vector for one layer; NA_real_ =
 * NA); nodata: a value that also means NA, or NA_real_; method: 0 near, 1 bilinear, 2 cubic, 3 mean, 4 min, 5 max, 6 sum,
 * 7 count.  Both run on the HOST entry points. */
static mhs_stack planes_from(SEXP planes, SEXP nodata, const mhs_grid *g, const char *who) {
    if (!Rf_isReal(planes)) Rf_error("%s: planes must be numeric (terra::values)", who);
    int C = Rf_isMatrix(planes) ? Rf_ncols(planes) : 1;
    if (C < 1 || (int64_t)Rf_xlength(planes) != g->nrow * g->ncol * C) Rf_error("%s: planes must have one row per cell", who);
    mhs_stack st = { REAL(planes), C, MHS_F64, (int64_t)g->nrow * g->ncol, g->ncol, Rf_asReal(nodata) };
    return st;
}

/* every layer on the grid geom_dst: an ncell(dst) x C matrix in terra cell order, NaN where the method gives NA */
SEXP mhsr_resample(SEXP geom_src, SEXP planes, SEXP nodata, SEXP geom_dst, SEXP method) {
    mhs_grid gs = grid_from(geom_src), gd = grid_from(geom_dst);
    mhs_stack st = planes_from(planes, nodata, &gs, "mhsr_resample");
    if (!(gd.nrow > 0 && gd.ncol > 0 && (double)gd.nrow * (double)gd.ncol <= 2147483647.0)) Rf_error("mhsr_resample: bad target dimension");
    SEXP out = PROTECT(Rf_allocMatrix(REALSXP, (int)(gd.nrow * gd.ncol), st.n_layers));
    int rc = mhs_resample(&gs, &st, &gd, 0, gd.nrow, 0, gd.ncol, Rf_asInteger(method), REAL(out), MHS_F64);
    UNPROTECT(1);
    chk(rc);
    return out;
}

/* terra::extract(src.ras, xy, method =): xy an n x 2 numeric matrix (x, y); method 0 simple, 1 bilinear, 2 cubic.  An n x C matrix. */
SEXP mhsr_extract(SEXP geom, SEXP planes, SEXP nodata, SEXP xy, SEXP method) {
    mhs_grid g = grid_from(geom);
    mhs_stack st = planes_from(planes, nodata, &g, "mhsr_extract");
    if (!Rf_isReal(xy) || !Rf_isMatrix(xy) || Rf_ncols(xy) != 2) Rf_error("mhsr_extract: xy must be a numeric matrix of 2 columns");
    int n = Rf_nrows(xy);
    SEXP out = PROTECT(Rf_allocMatrix(REALSXP, n, st.n_layers));
    int rc = mhs_extract_points(&g, &st, REAL(xy), (int64_t)n, Rf_asInteger(method), REAL(out));
    UNPROTECT(1);
    chk(rc);
    return out;
}

/* Every layer on the grid geom_dst of ANOTHER coordinate system (machisplin_hip.h "warp") through a control lattice the caller has
 * made (R has PROJ through terra): step a power of two, sx and sy the source coordinates of the target-grid points
 * (xmin + b step xres, ymax - a step yres), ROW-MAJOR vectors of (ceil(nrow / step) + 1) x (ceil(ncol / step) + 1) nodes (NA_real_
 * where the transform has no value: those cells come out NA).  method: 0 near, 1 bilinear, 2 cubic.  An ncell(dst) x C matrix in
 * terra cell order.  Runs on the HOST entry point mhs_warp: the whole stack goes up in one piece. */
SEXP mhsr_warp(SEXP geom_src, SEXP planes, SEXP nodata, SEXP geom_dst, SEXP step, SEXP sx, SEXP sy, SEXP method) {
    mhs_grid gs = grid_from(geom_src), gd = grid_from(geom_dst);
    mhs_stack st = planes_from(planes, nodata, &gs, "mhsr_warp");
    if (!(gd.nrow > 0 && gd.ncol > 0 && (double)gd.nrow * (double)gd.ncol <= 2147483647.0)) Rf_error("mhsr_warp: bad target dimension");
    int K = Rf_asInteger(step);
    if (K < 1 || K > 1024 || (K & (K - 1)) != 0) Rf_error("mhsr_warp: step must be a power of two in 1 .. 1024");
    int64_t nr = (gd.nrow + K - 1) / K + 1, nc = (gd.ncol + K - 1) / K + 1;
    if (!Rf_isReal(sx) || !Rf_isReal(sy) || (int64_t)Rf_xlength(sx) != nr * nc || (int64_t)Rf_xlength(sy) != nr * nc)
        Rf_error("mhsr_warp: sx and sy must be numeric with (ceil(nrow / step) + 1) x (ceil(ncol / step) + 1) = %d x %d nodes", (int)nr, (int)nc);
    mhs_warp_lattice lat = { K, nr, nc, REAL(sx), REAL(sy) };
    SEXP out = PROTECT(Rf_allocMatrix(REALSXP, (int)(gd.nrow * gd.ncol), st.n_layers));
    int rc = mhs_warp(&gs, &st, &gd, 0, gd.nrow, 0, gd.ncol, &lat, Rf_asInteger(method), REAL(out), MHS_F64);
    UNPROTECT(1);
    chk(rc);
    return out;
}

/* Window statistics of one layer at any radius (machisplin_hip.h "focal"): terra::focal for sums, moments, min and max.  planes,
 * nodata: as for mhsr_resample; opts: c(layer, shape, fill_na, offset) with layer 0-based, shape 0 square / 1 circle and offset the
 * constant the values are centred by (NA_real_: 0); radii: 1 .. 8 integers; stats: bit mask (1 count, 2 sum, 4 mean, 8 sd, 16 min,
 * 32 max, 64 range, 128 minus_mean, 256 above_min, 512 below_max, 1024 dev).  An ncell x (length(radii) * statistics) matrix in terra
 * cell order, radius after radius, the statistics in ascending bit order.  Runs on the HOST entry point mhs_focal (row bands). */
SEXP mhsr_focal(SEXP geom, SEXP planes, SEXP nodata, SEXP opts, SEXP radii, SEXP stats) {
    mhs_grid g = grid_from(geom);
    mhs_stack st = planes_from(planes, nodata, &g, "mhsr_focal");
    if (!Rf_isReal(opts) || Rf_length(opts) != 4) Rf_error("mhsr_focal: opts must be c(layer, shape, fill_na, offset)");
    const double *o = REAL(opts);
    if (TYPEOF(radii) != INTSXP || Rf_length(radii) < 1 || Rf_length(radii) > MHS_FOCAL_MAX_RADII)
        Rf_error("mhsr_focal: radii must be 1 .. %d integers", MHS_FOCAL_MAX_RADII);
    int mask = Rf_asInteger(stats), n = mask_planes(mask), nrad = Rf_length(radii);
    if (mask == NA_INTEGER || mask < 1 || mask > 2047) Rf_error("mhsr_focal: stats must be a bit mask of 1 count ... 1024 dev");
    if ((double)g.nrow * (double)g.ncol > 2147483647.0) Rf_error("mhsr_focal: bad dimension");
    SEXP out = PROTECT(Rf_allocMatrix(REALSXP, (int)(g.nrow * g.ncol), n * nrad));
    int rc = mhs_focal(&g, &st, (int)o[0], INTEGER(radii), nrad, (int)o[1], (unsigned)mask, o[2] != 0.0, ISNAN(o[3]) ? 0.0 : o[3], 0, g.nrow, 0, g.ncol,
                       REAL(out), MHS_F64);
    UNPROTECT(1);
    chk(rc);
    return out;
}

/* Distance to the nearest feature cell (machisplin_hip.h "proximity"): what terra::distance and terra::gridDist are used for.
 * planes, nodata: as for mhsr_resample; opts: c(layer, where, threshold, value_layer, unit) with layer and value_layer 0-based
 * (value_layer is read only for the value product) and where 0 na, 1 valid, 2 lt, 3 le, 4 gt, 5 ge, 6 eq, 7 ne; products: bit
 * mask (1 d2, 2 index, 4 dist, 8 dir_x, 16 dir_y, 32 value).  Returns list(d2, index, dist, dir_x, dir_y, value, info) in terra
 * cell order, NULL where a plane was not asked for: d2 and index integer vectors -- index the nearest feature's terra cell
 * NUMBER (1-based), both NA_integer_ where the raster has no feature --, the others numeric (NaN there); info = c(n_features,
 * max_d2).  Runs on the HOST entry point: the whole plane goes up, there are no row bands. */
SEXP mhsr_proximity(SEXP geom, SEXP planes, SEXP nodata, SEXP opts, SEXP products) {
    mhs_grid g = grid_from(geom);
    mhs_stack st = planes_from(planes, nodata, &g, "mhsr_proximity");
    int mask = Rf_asInteger(products);
    if (mask == NA_INTEGER || mask < 1 || mask > 63) Rf_error("mhsr_proximity: products must be a bit mask of 1 d2, 2 index, 4 dist, 8 dir_x, 16 dir_y, 32 value");
    if (!Rf_isReal(opts) || Rf_length(opts) != 5) Rf_error("mhsr_proximity: opts must be c(layer, where, threshold, value_layer, unit)");
    const double *o = REAL(opts);
    if (!(o[0] >= 0.0 && o[0] <= 2147483647.0)) Rf_error("mhsr_proximity: layer must be a 0-based layer number");
    if (!(o[1] >= 0.0 && o[1] <= 7.0)) Rf_error("mhsr_proximity: where must be 0 .. 7");
    int value_layer = (o[3] >= 0.0 && o[3] <= 2147483647.0) ? (int)o[3] : -1;
    if (!(g.nrow > 0 && g.ncol > 0 && (double)g.nrow * (double)g.ncol <= 2147483647.0)) Rf_error("mhsr_proximity: bad grid dimension");
    R_xlen_t n = (R_xlen_t)g.nrow * g.ncol;
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 7));
    SEXP plane[6] = { R_NilValue, R_NilValue, R_NilValue, R_NilValue, R_NilValue, R_NilValue };
    int n_protect = 1;
    for (int k = 0; k < 6; ++k)
        if (mask & (1 << k)) { plane[k] = PROTECT(Rf_allocVector(k < 2 ? INTSXP : REALSXP, n)); ++n_protect; }
    mhs_proximity_out po = { (mask & 1) ? (int32_t *)INTEGER(plane[0]) : NULL, (mask & 2) ? (int32_t *)INTEGER(plane[1]) : NULL,
                             (mask & 4) ? REAL(plane[2]) : NULL, (mask & 8) ? REAL(plane[3]) : NULL, (mask & 16) ? REAL(plane[4]) : NULL,
                             (mask & 32) ? REAL(plane[5]) : NULL };
    mhs_proximity_info info = { 0 };
    int rc = mhs_proximity(&g, &st, (int)o[0], (int)o[1], o[2], value_layer, o[4], &po, MHS_F64, &info);
    if (rc == MHS_OK) {
        if (mask & 1)
            for (R_xlen_t k = 0; k < n; ++k) if (INTEGER(plane[0])[k] < 0) INTEGER(plane[0])[k] = NA_INTEGER;
        if (mask & 2)
            for (R_xlen_t k = 0; k < n; ++k) INTEGER(plane[1])[k] = INTEGER(plane[1])[k] < 0 ? NA_INTEGER : INTEGER(plane[1])[k] + 1;
        SEXP inf = PROTECT(Rf_allocVector(REALSXP, 2)); ++n_protect;
        REAL(inf)[0] = (double)info.n_features; REAL(inf)[1] = (double)info.max_d2;
        for (int k = 0; k < 6; ++k) SET_VECTOR_ELT(out, k, plane[k]);
        SET_VECTOR_ELT(out, 6, inf);
    }
    UNPROTECT(n_protect);
    chk(rc);
    return out;
}

/* Connected patches of the feature cells (machisplin_hip.h "patches"): what terra::patches and a size filter (a sieve) are used
 * for.  planes, nodata: as for mhsr_resample; opts: c(layer, where, threshold, connectivity, min_size, max_size, edge_rule) with
 * layer 0-based, where 0 .. 7 as for mhsr_proximity, connectivity 4 or 8, max_size NA or Inf = no limit, edge_rule 0 any,
 * 1 touching, 2 interior; products: bit mask (1 label, 2 id, 4 size, 8 edge, 16 keep).  Returns list(label, id, size, edge, keep,
 * info) in terra cell order, NULL where a plane was not asked for, all integer vectors: label the terra cell NUMBER (1-based) of
 * the patch's first cell, NA_integer_ at a non-feature cell, the others 0 there; info = c(n_features, n_patches, n_kept_patches,
 * n_kept_cells, max_size).  Runs on the HOST entry point: the whole plane goes up, there are no row bands. */
SEXP mhsr_patches(SEXP geom, SEXP planes, SEXP nodata, SEXP opts, SEXP products) {
    mhs_grid g = grid_from(geom);
    mhs_stack st = planes_from(planes, nodata, &g, "mhsr_patches");
    int mask = Rf_asInteger(products);
    if (mask == NA_INTEGER || mask < 1 || mask > 31) Rf_error("mhsr_patches: products must be a bit mask of 1 label, 2 id, 4 size, 8 edge, 16 keep");
    if (!Rf_isReal(opts) || Rf_length(opts) != 7)
        Rf_error("mhsr_patches: opts must be c(layer, where, threshold, connectivity, min_size, max_size, edge_rule)");
    const double *o = REAL(opts);
    if (!(o[0] >= 0.0 && o[0] <= 2147483647.0)) Rf_error("mhsr_patches: layer must be a 0-based layer number");
    if (!(o[1] >= 0.0 && o[1] <= 7.0)) Rf_error("mhsr_patches: where must be 0 .. 7");
    if (!(o[3] == 4.0 || o[3] == 8.0)) Rf_error("mhsr_patches: connectivity must be 4 or 8");
    if (!(o[4] >= 1.0 && o[4] <= 2147483647.0)) Rf_error("mhsr_patches: min_size must be a whole number of cells >= 1");
    if (!(o[6] >= 0.0 && o[6] <= 2.0)) Rf_error("mhsr_patches: edge_rule must be 0 any, 1 touching or 2 interior");
    if (!(g.nrow > 0 && g.ncol > 0 && (double)g.nrow * (double)g.ncol <= 2147483647.0)) Rf_error("mhsr_patches: bad grid dimension");
    int64_t max_size = (ISNAN(o[5]) || o[5] >= 2147483647.0) ? INT64_MAX : o[5] < 1.0 ? 0 : (int64_t)o[5];       /* below min_size: the library refuses */
    R_xlen_t n = (R_xlen_t)g.nrow * g.ncol;
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 6));
    SEXP plane[5] = { R_NilValue, R_NilValue, R_NilValue, R_NilValue, R_NilValue };
    uint8_t *byte[5] = { NULL, NULL, NULL, NULL, NULL };
    int n_protect = 1;
    for (int k = 0; k < 5; ++k)
        if (mask & (1 << k)) {
            plane[k] = PROTECT(Rf_allocVector(INTSXP, n)); ++n_protect;
            if (k >= 3) byte[k] = (uint8_t *)R_alloc((size_t)n, 1);                            /* edge and keep come down as bytes */
        }
    mhs_patches_out po = { (mask & 1) ? (int32_t *)INTEGER(plane[0]) : NULL, (mask & 2) ? (int32_t *)INTEGER(plane[1]) : NULL,
                           (mask & 4) ? (int32_t *)INTEGER(plane[2]) : NULL, byte[3], byte[4] };
    mhs_patches_info info = { 0 };
    int rc = mhs_patches(&g, &st, (int)o[0], (int)o[1], o[2], (int)o[3], (int64_t)o[4], max_size, (int)o[6], &po, &info);
    if (rc == MHS_OK) {
        if (mask & 1)
            for (R_xlen_t k = 0; k < n; ++k) INTEGER(plane[0])[k] = INTEGER(plane[0])[k] < 0 ? NA_INTEGER : INTEGER(plane[0])[k] + 1;
        for (int j = 3; j < 5; ++j)
            if (byte[j])
                for (R_xlen_t k = 0; k < n; ++k) INTEGER(plane[j])[k] = byte[j][k];
        SEXP inf = PROTECT(Rf_allocVector(REALSXP, 5)); ++n_protect;
        REAL(inf)[0] = (double)info.n_features; REAL(inf)[1] = (double)info.n_patches; REAL(inf)[2] = (double)info.n_kept_patches;
        REAL(inf)[3] = (double)info.n_kept_cells; REAL(inf)[4] = (double)info.max_size;
        for (int k = 0; k < 5; ++k) SET_VECTOR_ELT(out, k, plane[k]);
        SET_VECTOR_ELT(out, 5, inf);
    }
    UNPROTECT(n_protect);
    chk(rc);
    return out;
}

/* Zonal statistics (machisplin_hip.h "zonal"): what terra::zonal is used for, and the statistics put back on the cells.  planes,
 * nodata: as for mhsr_resample; zones: an integer vector of one zone number per cell in terra cell order, NA_integer_ or a
 * negative number = no zone; opts: c(layer, n_zones, quantum, present) with layer 0-based, n_zones 0 = max(zone) + 1, quantum 0 =
 * the library's choice, present 1 = only the zones that have a cell; stats: bit mask of the table's statistics (1 count, 2 sum,
 * 4 mean, 8 sd, 16 min, 32 max, 64 range, 2048 cells), 0 for no table; planes_mask: bit mask of the planes (those and 128
 * minus_mean, 256 above_min, 512 below_max, 1024 dev), 0 for none.  Returns list(table, planes, info): table = list(zone, count,
 * sum, mean, sd, min, max, range, cells), numeric vectors of one row per zone (zone: integer, NULL for a dense table), NULL where
 * not asked for; planes = a list of 12 by bit number, numeric (count and cells integer), NULL where not asked for; info =
 * c(n_zones, n_present, n_cells_in_zones, n_contributing, n_nonfinite, n_inexact, quantum).  Runs on the HOST entry point: the
 * layer and the zone plane go up whole.  A dense table whose n_zones is to be measured costs a first call for the info. */
SEXP mhsr_zonal(SEXP geom, SEXP planes, SEXP nodata, SEXP zones, SEXP opts, SEXP stats, SEXP planes_mask) {
    mhs_grid g = grid_from(geom);
    mhs_stack st = planes_from(planes, nodata, &g, "mhsr_zonal");
    int ts = Rf_asInteger(stats), ps = Rf_asInteger(planes_mask);
    if (ts == NA_INTEGER || ts < 0 || (ts & ~0x87f)) Rf_error("mhsr_zonal: stats must be a bit mask of 1 count, 2 sum, 4 mean, 8 sd, 16 min, 32 max, 64 range, 2048 cells");
    if (ps == NA_INTEGER || ps < 0 || ps > 4095) Rf_error("mhsr_zonal: planes_mask must be a bit mask of the twelve statistics (1 count ... 2048 cells)");
    if (!ts && !ps) Rf_error("mhsr_zonal: no output: stats and planes_mask are both 0");
    if (!Rf_isReal(opts) || Rf_length(opts) != 4) Rf_error("mhsr_zonal: opts must be c(layer, n_zones, quantum, present)");
    const double *o = REAL(opts);
    if (!(o[0] >= 0.0 && o[0] <= 2147483647.0)) Rf_error("mhsr_zonal: layer must be a 0-based layer number");
    if (!(o[1] >= 0.0 && o[1] <= 2147483647.0)) Rf_error("mhsr_zonal: n_zones must be 0 (measure it) or in 1 .. 2^31 - 1");
    if (!(o[2] >= 0.0)) Rf_error("mhsr_zonal: quantum must be 0 (the library's choice) or a power of two");
    if (!(g.nrow > 0 && g.ncol > 0 && (double)g.nrow * (double)g.ncol <= 2147483647.0)) Rf_error("mhsr_zonal: bad grid dimension");
    R_xlen_t n = (R_xlen_t)g.nrow * g.ncol;
    if (TYPEOF(zones) != INTSXP || Rf_xlength(zones) != n) Rf_error("mhsr_zonal: zones must be an integer vector of one zone per cell");
    const int present = o[3] != 0.0;
    int64_t n_zones = (int64_t)o[1];
    double quantum = o[2];
    mhs_zonal_info info = { 0 };
    if (ts && !present && n_zones == 0) {                          /* the library measures n_zones before the dense table is sized */
        chk(mhs_zonal(&g, &st, (int)o[0], (const int32_t *)INTEGER(zones), 0, quantum, 0, NULL, NULL, &info));
        n_zones = info.n_zones;
        quantum = info.quantum;
    }
    R_xlen_t rows = !ts ? 0 : !present ? (R_xlen_t)n_zones : (n_zones && n_zones < n) ? (R_xlen_t)n_zones : n;
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 3));
    SEXP tab = PROTECT(Rf_allocVector(VECSXP, 9)), pl = PROTECT(Rf_allocVector(VECSXP, 12));
    int n_protect = 3;
    for (int k = 0; k < 9; ++k) SET_VECTOR_ELT(tab, k, R_NilValue);
    for (int k = 0; k < 12; ++k) SET_VECTOR_ELT(pl, k, R_NilValue);
    /* the library's arrays hold `rows` rows in transient storage; the R vectors are made once the number of rows is known */
    mhs_zonal_table zt = { (int64_t)rows, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL };
    double **slot[6] = { &zt.sum, &zt.mean, &zt.sd, &zt.min, &zt.max, &zt.range };
    if (ts && rows > 0) {
        if (present) zt.zone = (int32_t *)R_alloc((size_t)rows, sizeof(int32_t));
        if (ts & 1) zt.count = (int64_t *)R_alloc((size_t)rows, sizeof(int64_t));
        if (ts & 2048) zt.cells = (int64_t *)R_alloc((size_t)rows, sizeof(int64_t));
        for (int k = 1; k < 7; ++k)
            if (ts & (1 << k)) *slot[k - 1] = (double *)R_alloc((size_t)rows, sizeof(double));
    }
    mhs_zonal_planes zp = { { NULL }, { 0 }, MHS_F64 };
    for (int k = 0; k < 12; ++k)
        if (ps & (1 << k)) {
            const int is_int = k == 0 || k == 11;
            SET_VECTOR_ELT(pl, k, Rf_allocVector(is_int ? INTSXP : REALSXP, n));
            zp.plane[k] = is_int ? (void *)INTEGER(VECTOR_ELT(pl, k)) : (void *)REAL(VECTOR_ELT(pl, k));
            zp.ld[k] = g.ncol;
        }
    const int with_table = ts && rows > 0;
    int rc = MHS_OK;
    if (with_table || ps) rc = mhs_zonal(&g, &st, (int)o[0], (const int32_t *)INTEGER(zones), n_zones, quantum, 0, with_table ? &zt : NULL, ps ? &zp : NULL, &info);
    if (rc == MHS_OK) {
        const R_xlen_t k_rows = !with_table ? 0 : present ? (R_xlen_t)info.n_present : rows;
        if (ts) {
            if (present) {
                SET_VECTOR_ELT(tab, 0, Rf_allocVector(INTSXP, k_rows));
                for (R_xlen_t k = 0; k < k_rows; ++k) INTEGER(VECTOR_ELT(tab, 0))[k] = zt.zone[k];
            }
            for (int j = 0; j < 8; ++j) {                          /* count, sum .. range, cells: bits 0 .. 6 and 11 */
                if (!(ts & (1 << (j == 7 ? 11 : j)))) continue;
                SET_VECTOR_ELT(tab, 1 + j, Rf_allocVector(REALSXP, k_rows));
                double *dst = REAL(VECTOR_ELT(tab, 1 + j));
                for (R_xlen_t k = 0; k < k_rows; ++k)
                    dst[k] = j == 0 ? (double)zt.count[k] : j == 7 ? (double)zt.cells[k] : (*slot[j - 1])[k];
            }
        }
        SEXP inf = PROTECT(Rf_allocVector(REALSXP, 7)); ++n_protect;
        REAL(inf)[0] = (double)info.n_zones; REAL(inf)[1] = (double)info.n_present; REAL(inf)[2] = (double)info.n_cells_in_zones;
        REAL(inf)[3] = (double)info.n_contributing; REAL(inf)[4] = (double)info.n_nonfinite; REAL(inf)[5] = (double)info.n_inexact;
        REAL(inf)[6] = info.quantum;
        SET_VECTOR_ELT(out, 0, tab);
        SET_VECTOR_ELT(out, 1, pl);
        SET_VECTOR_ELT(out, 2, inf);
    }
    UNPROTECT(n_protect);
    chk(rc);
    return out;
}

/* Zonal quantiles (section "zonal quantiles" of machisplin_hip.h) through the host entry mhs_zonal_quantile.  planes, nodata: as
 * for mhsr_zonal; zones: an integer vector of one zone per cell, or NULL; target: NULL or the geometry c(xmin, ymax, xres, yres,
 * nrow, ncol) of the grid whose cells are the zones (zones must then be NULL); both NULL: the whole layer.  opts: c(layer,
 * n_zones, quantum, present, table, planes) with layer 0-based, n_zones and quantum 0 = the library's choice, table != 0 a table,
 * planes a bit mask of 1 q, 2 below, 4 frac_below.  probs: 1 .. 16 probabilities.  Returns list(table = list(zone, count, q)
 * with q a vector of rows x n_probs values, row-major; planes = list(q = a list of one plane per probability, below, frac_below);
 * info = c(n_zones, n_present, n_cells_in_zones, n_contributing, n_nonfinite, n_inexact, quantum, passes_run)). */
SEXP mhsr_zonal_quantile(SEXP geom, SEXP planes, SEXP nodata, SEXP zones, SEXP target, SEXP opts, SEXP probs) {
    mhs_grid g = grid_from(geom);
    mhs_stack st = planes_from(planes, nodata, &g, "mhsr_zonal_quantile");
    if (!Rf_isReal(opts) || Rf_length(opts) != 6) Rf_error("mhsr_zonal_quantile: opts must be c(layer, n_zones, quantum, present, table, planes)");
    const double *o = REAL(opts);
    if (!(o[0] >= 0.0 && o[0] <= 2147483647.0)) Rf_error("mhsr_zonal_quantile: layer must be a 0-based layer number");
    if (!(o[1] >= 0.0 && o[1] <= 2147483647.0)) Rf_error("mhsr_zonal_quantile: n_zones must be 0 (measure it) or in 1 .. 2^31 - 1");
    if (!(o[2] >= 0.0)) Rf_error("mhsr_zonal_quantile: quantum must be 0 (the library's choice) or a power of two");
    if (!(o[5] >= 0.0 && o[5] <= 7.0)) Rf_error("mhsr_zonal_quantile: planes must be a bit mask of 1 q, 2 below, 4 frac_below");
    if (!Rf_isReal(probs) || Rf_length(probs) < 1 || Rf_length(probs) > MHS_QUANTILE_MAX_PROBS) Rf_error("mhsr_zonal_quantile: probs must hold 1 .. 16 probabilities");
    if (!(g.nrow > 0 && g.ncol > 0 && (double)g.nrow * (double)g.ncol <= 2147483647.0)) Rf_error("mhsr_zonal_quantile: bad grid dimension");
    const R_xlen_t n = (R_xlen_t)g.nrow * g.ncol;
    const int have_zones = !Rf_isNull(zones), have_target = !Rf_isNull(target);
    if (have_zones && have_target) Rf_error("mhsr_zonal_quantile: zones and target are both given");
    if (have_zones && (TYPEOF(zones) != INTSXP || Rf_xlength(zones) != n)) Rf_error("mhsr_zonal_quantile: zones must be NULL or an integer vector of one zone per cell");
    if (!have_zones && o[1] != 0.0) Rf_error("mhsr_zonal_quantile: n_zones goes with a zone plane");
    mhs_grid tg = g;
    if (have_target) {
        tg = grid_from(target);
        if (!(tg.nrow > 0 && tg.ncol > 0 && (double)tg.nrow * (double)tg.ncol <= 2147483647.0)) Rf_error("mhsr_zonal_quantile: bad target dimension");
    }
    const int n_probs = Rf_length(probs), present = o[3] != 0.0, want_table = o[4] != 0.0, ps = (int)o[5];
    if (!want_table && !ps) Rf_error("mhsr_zonal_quantile: no output: neither a table nor a plane is asked for");
    const int32_t *zp = have_zones ? (const int32_t *)INTEGER(zones) : NULL;
    const mhs_grid *tp = have_target ? &tg : NULL;
    int64_t n_zones = (int64_t)o[1];
    double quantum = o[2];
    mhs_quantile_info info = { 0 };
    if (!have_zones) n_zones = have_target ? tg.nrow * tg.ncol : 1;
    else if (want_table && !present && n_zones == 0) {             /* the library measures n_zones before the dense table is sized */
        chk(mhs_zonal_quantile(&g, &st, (int)o[0], zp, 0, quantum, 0, REAL(probs), n_probs, tp, NULL, NULL, &info));
        n_zones = info.n_zones;
        quantum = info.quantum;
    }
    const R_xlen_t rows = !want_table ? 0 : !present ? (R_xlen_t)n_zones : (n_zones && n_zones < n) ? (R_xlen_t)n_zones : n;
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 3));
    SEXP tab = PROTECT(Rf_allocVector(VECSXP, 3)), pl = PROTECT(Rf_allocVector(VECSXP, 3));
    int n_protect = 3;
    for (int k = 0; k < 3; ++k) { SET_VECTOR_ELT(tab, k, R_NilValue); SET_VECTOR_ELT(pl, k, R_NilValue); }
    mhs_quantile_table qt = { (int64_t)rows, NULL, NULL, NULL };
    const int with_table = want_table && rows > 0;
    if (with_table) {
        if (present) qt.zone = (int32_t *)R_alloc((size_t)rows, sizeof(int32_t));
        qt.count = (int64_t *)R_alloc((size_t)rows, sizeof(int64_t));
        qt.q = (double *)R_alloc((size_t)rows * (size_t)n_probs, sizeof(double));
    }
    mhs_quantile_planes qp = { { NULL }, { 0 }, NULL, 0, NULL, 0, MHS_F64 };
    if (ps & 1) {
        SET_VECTOR_ELT(pl, 0, Rf_allocVector(VECSXP, n_probs));
        for (int j = 0; j < n_probs; ++j) {
            SET_VECTOR_ELT(VECTOR_ELT(pl, 0), j, Rf_allocVector(REALSXP, n));
            qp.q[j] = REAL(VECTOR_ELT(VECTOR_ELT(pl, 0), j));
            qp.ld_q[j] = g.ncol;
        }
    }
    if (ps & 2) { SET_VECTOR_ELT(pl, 1, Rf_allocVector(INTSXP, n)); qp.below = (int32_t *)INTEGER(VECTOR_ELT(pl, 1)); qp.ld_below = g.ncol; }
    if (ps & 4) { SET_VECTOR_ELT(pl, 2, Rf_allocVector(REALSXP, n)); qp.frac_below = REAL(VECTOR_ELT(pl, 2)); qp.ld_frac_below = g.ncol; }
    int rc = MHS_OK;
    if (with_table || ps)
        rc = mhs_zonal_quantile(&g, &st, (int)o[0], zp, have_zones ? n_zones : 0, quantum, 0, REAL(probs), n_probs, tp, with_table ? &qt : NULL, ps ? &qp : NULL, &info);
    if (rc == MHS_OK) {
        const R_xlen_t k_rows = !with_table ? 0 : present ? (R_xlen_t)info.n_present : rows;
        if (want_table) {
            if (present) {
                SET_VECTOR_ELT(tab, 0, Rf_allocVector(INTSXP, k_rows));
                for (R_xlen_t k = 0; k < k_rows; ++k) INTEGER(VECTOR_ELT(tab, 0))[k] = qt.zone[k];
            }
            SET_VECTOR_ELT(tab, 1, Rf_allocVector(REALSXP, k_rows));
            SET_VECTOR_ELT(tab, 2, Rf_allocVector(REALSXP, k_rows * n_probs));
            for (R_xlen_t k = 0; k < k_rows; ++k) REAL(VECTOR_ELT(tab, 1))[k] = (double)qt.count[k];
            for (R_xlen_t k = 0; k < k_rows * n_probs; ++k) REAL(VECTOR_ELT(tab, 2))[k] = qt.q[k];
        }
        SEXP inf = PROTECT(Rf_allocVector(REALSXP, 8)); ++n_protect;
        REAL(inf)[0] = (double)info.n_zones; REAL(inf)[1] = (double)info.n_present; REAL(inf)[2] = (double)info.n_cells_in_zones;
        REAL(inf)[3] = (double)info.n_contributing; REAL(inf)[4] = (double)info.n_nonfinite; REAL(inf)[5] = (double)info.n_inexact;
        REAL(inf)[6] = info.quantum; REAL(inf)[7] = (double)info.passes_run;
        SET_VECTOR_ELT(out, 0, tab);
        SET_VECTOR_ELT(out, 1, pl);
        SET_VECTOR_ELT(out, 2, inf);
    }
    UNPROTECT(n_protect);
    chk(rc);
    return out;
}

/* the class list and frac_of of the two class entries: integer vectors, or NULL (classes: measure them; frac_of: all classes) */
static int class_codes(SEXP v, const char *who, const char *what, const int32_t **out) {
    *out = NULL;
    if (v == R_NilValue) return 0;
    if (TYPEOF(v) != INTSXP || Rf_xlength(v) < 1 || Rf_xlength(v) > MHS_CLASS_MAX) Rf_error("%s: %s must be NULL or an integer vector of 1 .. 256 codes", who, what);
    *out = (const int32_t *)INTEGER(v);
    return (int)Rf_xlength(v);
}
static SEXP class_info_vec(const mhs_class_info *info) {          /* c(K, n_zones, n_valid, n_na, n_other) */
    SEXP inf = Rf_allocVector(REALSXP, 5);
    REAL(inf)[0] = (double)info->K; REAL(inf)[1] = (double)info->n_zones; REAL(inf)[2] = (double)info->n_valid;
    REAL(inf)[3] = (double)info->n_na; REAL(inf)[4] = (double)info->n_other;
    return inf;
}
static SEXP class_codes_vec(const mhs_class_info *info) {
    SEXP codes = Rf_allocVector(INTSXP, info->K);
    for (int k = 0; k < info->K; ++k) INTEGER(codes)[k] = info->codes[k];
    return codes;
}

/* Class counts, fractions and mode per zone (machisplin_hip.h "classes"): what terra::crosstab is used for, and mhs_zonal's missing
 * mode.  planes, nodata, zones: as for mhsr_zonal; opts: c(layer, n_zones) with layer 0-based and n_zones 0 = max(zone) + 1;
 * classes: integer vector of the class codes, NULL = the codes present in the layer; frac_of: integer vector of the codes whose
 * frac is wanted, NULL = all; stats: bit mask of the table's statistics (1 counts, 2 n, 4 other, 8 cells, 16 mode, 32 mode_frac,
 * 64 variety, 128 simpson, 256 frac), 0 for no table; planes_mask: bit mask of the planes (1 mode, 2 mode_frac, 4 variety,
 * 8 simpson, 16 n, 32 frac), 0 for none.  Returns list(table, planes, info, codes): table = a list of 9 in that order, one entry per
 * zone (counts: an integer matrix K x n_zones, frac: a numeric matrix n_frac x n_zones -- a zone is a COLUMN), NULL where not asked
 * for; planes = a list of 6 in that order, one entry per cell in terra cell order (frac: a matrix ncell x n_frac); info = c(K,
 * n_zones, n_valid, n_na, n_other); codes = the class codes in force, ascending.  Runs on the HOST entry point.  Measured classes
 * or n_zones cost a first call for the info. */
SEXP mhsr_class_crosstab(SEXP geom, SEXP planes, SEXP nodata, SEXP zones, SEXP opts, SEXP classes, SEXP frac_of, SEXP stats, SEXP planes_mask) {
    mhs_grid g = grid_from(geom);
    mhs_stack st = planes_from(planes, nodata, &g, "mhsr_class_crosstab");
    int ts = Rf_asInteger(stats), ps = Rf_asInteger(planes_mask);
    if (ts == NA_INTEGER || ts < 0 || ts > 511) Rf_error("mhsr_class_crosstab: stats must be a bit mask of 1 counts, 2 n, 4 other, 8 cells, 16 mode, 32 mode_frac, 64 variety, 128 simpson, 256 frac");
    if (ps == NA_INTEGER || ps < 0 || ps > 63) Rf_error("mhsr_class_crosstab: planes_mask must be a bit mask of 1 mode, 2 mode_frac, 4 variety, 8 simpson, 16 n, 32 frac");
    if (!ts && !ps) Rf_error("mhsr_class_crosstab: no output: stats and planes_mask are both 0");
    if (!Rf_isReal(opts) || Rf_length(opts) != 2) Rf_error("mhsr_class_crosstab: opts must be c(layer, n_zones)");
    const double *o = REAL(opts);
    if (!(o[0] >= 0.0 && o[0] <= 2147483647.0)) Rf_error("mhsr_class_crosstab: layer must be a 0-based layer number");
    if (!(o[1] >= 0.0 && o[1] <= 2147483647.0)) Rf_error("mhsr_class_crosstab: n_zones must be 0 (measure it) or in 1 .. 2^31 - 1");
    if (!(g.nrow > 0 && g.ncol > 0 && (double)g.nrow * (double)g.ncol <= 2147483647.0)) Rf_error("mhsr_class_crosstab: bad grid dimension");
    R_xlen_t n = (R_xlen_t)g.nrow * g.ncol;
    if (TYPEOF(zones) != INTSXP || Rf_xlength(zones) != n) Rf_error("mhsr_class_crosstab: zones must be an integer vector of one zone per cell");
    const int32_t *cl, *fo;
    int K = class_codes(classes, "mhsr_class_crosstab", "classes", &cl);
    const int nf_given = class_codes(frac_of, "mhsr_class_crosstab", "frac_of", &fo);
    int64_t n_zones = (int64_t)o[1];
    mhs_class_info info;
    int32_t measured[MHS_CLASS_MAX];
    memset(&info, 0, sizeof(info));
    if (K == 0 || n_zones == 0) {                                  /* the library measures the codes and n_zones before the outputs are sized */
        chk(mhs_class_crosstab(&g, &st, (int)o[0], (const int32_t *)INTEGER(zones), n_zones, cl, K, NULL, 0, NULL, NULL, &info));
        n_zones = info.n_zones;
        K = info.K;
        memcpy(measured, info.codes, sizeof(measured));
        cl = measured;
    }
    const int nf = nf_given ? nf_given : K;
    const R_xlen_t rows = (R_xlen_t)n_zones;
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 4));
    SEXP tab = PROTECT(Rf_allocVector(VECSXP, 9)), pl = PROTECT(Rf_allocVector(VECSXP, 6));
    for (int k = 0; k < 9; ++k) SET_VECTOR_ELT(tab, k, R_NilValue);
    for (int k = 0; k < 6; ++k) SET_VECTOR_ELT(pl, k, R_NilValue);
    mhs_class_table ct;
    mhs_class_planes cp;
    memset(&ct, 0, sizeof(ct));
    memset(&cp, 0, sizeof(cp));
    ct.capacity = (int64_t)rows;
    for (int k = 0; k < 9; ++k) {
        if (!(ts & (1 << k))) continue;
        const int is_int = k < 5 || k == 6;
        SEXP v = k == 0 ? Rf_allocMatrix(INTSXP, K, (int)rows) : k == 8 ? Rf_allocMatrix(REALSXP, nf, (int)rows) : Rf_allocVector(is_int ? INTSXP : REALSXP, rows);
        SET_VECTOR_ELT(tab, k, v);
        void *p = is_int ? (void *)INTEGER(v) : (void *)REAL(v);
        if (k == 0) ct.counts = p; else if (k == 1) ct.n = p; else if (k == 2) ct.other = p; else if (k == 3) ct.cells = p; else if (k == 4) ct.mode = p;
        else if (k == 5) ct.mode_frac = p; else if (k == 6) ct.variety = p; else if (k == 7) ct.simpson = p; else ct.frac = p;
    }
    cp.dtype = MHS_F64;
    for (int k = 0; k < 6; ++k) {
        if (!(ps & (1 << k))) continue;
        const int is_int = k == 0 || k == 2 || k == 4;
        SEXP v = k == 5 ? Rf_allocMatrix(REALSXP, (int)n, nf) : Rf_allocVector(is_int ? INTSXP : REALSXP, n);
        SET_VECTOR_ELT(pl, k, v);
        void *p = is_int ? (void *)INTEGER(v) : (void *)REAL(v);
        if (k == 0) cp.mode = p; else if (k == 1) cp.mode_frac = p; else if (k == 2) cp.variety = p; else if (k == 3) cp.simpson = p; else if (k == 4) cp.n = p;
        else cp.frac = p;
    }
    const int with_table = ts && rows > 0;
    int rc = MHS_OK;
    if (with_table || ps) rc = mhs_class_crosstab(&g, &st, (int)o[0], (const int32_t *)INTEGER(zones), n_zones, cl, K, fo, nf_given, with_table ? &ct : NULL, ps ? &cp : NULL, &info);
    if (rc == MHS_OK) {
        SET_VECTOR_ELT(out, 0, tab);
        SET_VECTOR_ELT(out, 1, pl);
        SET_VECTOR_ELT(out, 2, class_info_vec(&info));
        SET_VECTOR_ELT(out, 3, class_codes_vec(&info));
    }
    UNPROTECT(3);
    chk(rc);
    return out;
}

/* Class fractions and mode per cell of another grid (machisplin_hip.h "classes"): terra::aggregate(fun = "modal"), and class cover
 * when land cover is finer than the model grid.  geom_src, planes, nodata, geom_dst: as for mhsr_resample; opts: c(layer), 0-based;
 * classes, frac_of: as for mhsr_class_crosstab; products: bit mask of 1 mode, 2 variety, 4 n, 8 mode_frac, 16 simpson, 32 frac.
 * Returns list(planes, info, codes): planes = a list of 6 in that order, one entry per cell of dst in terra cell order (frac: a
 * matrix ncell x n_frac), NULL where not asked for.  Runs on the HOST entry point. */
SEXP mhsr_class_aggregate(SEXP geom_src, SEXP planes, SEXP nodata, SEXP geom_dst, SEXP opts, SEXP classes, SEXP frac_of, SEXP products) {
    mhs_grid gs = grid_from(geom_src), gd = grid_from(geom_dst);
    mhs_stack st = planes_from(planes, nodata, &gs, "mhsr_class_aggregate");
    const int pm = Rf_asInteger(products);
    if (pm == NA_INTEGER || pm < 1 || pm > 63) Rf_error("mhsr_class_aggregate: products must be a bit mask of 1 mode, 2 variety, 4 n, 8 mode_frac, 16 simpson, 32 frac, and not 0");
    if (!Rf_isReal(opts) || Rf_length(opts) != 1) Rf_error("mhsr_class_aggregate: opts must be c(layer)");
    const double *o = REAL(opts);
    if (!(o[0] >= 0.0 && o[0] <= 2147483647.0)) Rf_error("mhsr_class_aggregate: layer must be a 0-based layer number");
    if (!(gd.nrow > 0 && gd.ncol > 0 && (double)gd.nrow * (double)gd.ncol <= 2147483647.0)) Rf_error("mhsr_class_aggregate: bad target dimension");
    const R_xlen_t n = (R_xlen_t)gd.nrow * gd.ncol;
    const int32_t *cl, *fo;
    int K = class_codes(classes, "mhsr_class_aggregate", "classes", &cl);
    const int nf_given = class_codes(frac_of, "mhsr_class_aggregate", "frac_of", &fo);
    mhs_class_info info;
    int32_t measured[MHS_CLASS_MAX];
    memset(&info, 0, sizeof(info));
    if (K == 0) {                                                  /* the library measures the codes before frac is sized */
        chk(mhs_class_aggregate(&gs, &st, (int)o[0], &gd, NULL, 0, NULL, 0, NULL, &info));
        K = info.K;
        memcpy(measured, info.codes, sizeof(measured));
        cl = measured;
    }
    const int nf = nf_given ? nf_given : K;
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 3));
    SEXP pl = PROTECT(Rf_allocVector(VECSXP, 6));
    for (int k = 0; k < 6; ++k) SET_VECTOR_ELT(pl, k, R_NilValue);
    mhs_class_planes cp;
    memset(&cp, 0, sizeof(cp));
    cp.dtype = MHS_F64;
    for (int k = 0; k < 6; ++k) {
        if (!(pm & (1 << k))) continue;
        const int is_int = k < 3;
        SEXP v = k == 5 ? Rf_allocMatrix(REALSXP, (int)n, nf) : Rf_allocVector(is_int ? INTSXP : REALSXP, n);
        SET_VECTOR_ELT(pl, k, v);
        void *p = is_int ? (void *)INTEGER(v) : (void *)REAL(v);
        if (k == 0) cp.mode = p; else if (k == 1) cp.variety = p; else if (k == 2) cp.n = p; else if (k == 3) cp.mode_frac = p; else if (k == 4) cp.simpson = p;
        else cp.frac = p;
    }
    const int rc = mhs_class_aggregate(&gs, &st, (int)o[0], &gd, cl, K, fo, nf_given, &cp, &info);
    if (rc == MHS_OK) {
        SET_VECTOR_ELT(out, 0, pl);
        SET_VECTOR_ELT(out, 1, class_info_vec(&info));
        SET_VECTOR_ELT(out, 2, class_codes_vec(&info));
    }
    UNPROTECT(2);
    chk(rc);
    return out;
}

/* Vector features burned onto the grid (machisplin_hip.h "rasterize"): what terra::rasterize is used for.  coords: a V x 2 numeric
 * matrix (x, y) in the grid's coordinate system; part_offsets: integer vector of P + 1 0-based vertex numbers (a part is a ring of
 * a polygon, a polyline, a run of points); feature_offsets: integer vector of F + 1 0-based part numbers; values: numeric vector of
 * one value per feature, or NULL; opts: c(kind, rule, touches, scratch_budget) with kind 0 point, 1 line, 2 polygon, rule 0 last,
 * 1 first, 2 max, 3 min, scratch_budget 0 = the library's 256 MiB; products: bit mask of 1 index, 2 count, 4 value.  Returns
 * list(index, count, value, info): index (integer, the winning feature 0-based, -1 for none) and count (integer) and value
 * (numeric, NaN for none), one per cell in terra cell order, NULL where not asked for; info = c(n_features, n_parts, n_vertices,
 * n_edges, n_items, n_batches, n_burned, n_outside).  Runs on the HOST entry point: the products come down whole. */
SEXP mhsr_rasterize(SEXP geom, SEXP coords, SEXP part_offsets, SEXP feature_offsets, SEXP values, SEXP opts, SEXP products) {
    mhs_grid g = grid_from(geom);
    if (!Rf_isReal(coords) || !Rf_isMatrix(coords) || Rf_ncols(coords) != 2) Rf_error("mhsr_rasterize: coords must be a numeric matrix of two columns (x, y)");
    if (TYPEOF(part_offsets) != INTSXP || Rf_xlength(part_offsets) < 1) Rf_error("mhsr_rasterize: part_offsets must be an integer vector of n_parts + 1 vertex numbers");
    if (TYPEOF(feature_offsets) != INTSXP || Rf_xlength(feature_offsets) < 1) Rf_error("mhsr_rasterize: feature_offsets must be an integer vector of n_features + 1 part numbers");
    const R_xlen_t nv = Rf_nrows(coords), np = Rf_xlength(part_offsets) - 1, nf = Rf_xlength(feature_offsets) - 1;
    if (values != R_NilValue && (!Rf_isReal(values) || Rf_xlength(values) != nf)) Rf_error("mhsr_rasterize: values must be NULL or a numeric vector of one value per feature");
    if (!Rf_isReal(opts) || Rf_length(opts) != 4) Rf_error("mhsr_rasterize: opts must be c(kind, rule, touches, scratch_budget)");
    const double *o = REAL(opts);
    if (!(o[0] >= 0.0 && o[0] <= 2.0)) Rf_error("mhsr_rasterize: kind must be 0 (point), 1 (line) or 2 (polygon)");
    if (!(o[1] >= 0.0 && o[1] <= 3.0)) Rf_error("mhsr_rasterize: rule must be 0 (last), 1 (first), 2 (max) or 3 (min)");
    if (!(o[3] >= 0.0 && o[3] <= 9007199254740992.0)) Rf_error("mhsr_rasterize: scratch_budget must be 0 (the library's choice) or a number of bytes");
    int pm = Rf_asInteger(products);
    if (pm == NA_INTEGER || pm < 1 || pm > 7) Rf_error("mhsr_rasterize: products must be a bit mask of 1 index, 2 count, 4 value, and not 0");
    if (!(g.nrow > 0 && g.ncol > 0 && (double)g.nrow * (double)g.ncol <= 2147483647.0)) Rf_error("mhsr_rasterize: bad grid dimension");
    R_xlen_t n = (R_xlen_t)g.nrow * g.ncol;
    /* R's matrix is column-major and its offsets are int: the library takes x, y pairs and int64 */
    double *xy = (double *)R_alloc((size_t)(nv ? 2 * nv : 1), sizeof(double));
    int64_t *po = (int64_t *)R_alloc((size_t)(np + 1), sizeof(int64_t)), *fo = (int64_t *)R_alloc((size_t)(nf + 1), sizeof(int64_t));
    for (R_xlen_t v = 0; v < nv; ++v) { xy[2 * v] = REAL(coords)[v]; xy[2 * v + 1] = REAL(coords)[nv + v]; }
    for (R_xlen_t i = 0; i <= np; ++i) po[i] = INTEGER(part_offsets)[i] == NA_INTEGER ? -1 : INTEGER(part_offsets)[i];
    for (R_xlen_t i = 0; i <= nf; ++i) fo[i] = INTEGER(feature_offsets)[i] == NA_INTEGER ? -1 : INTEGER(feature_offsets)[i];
    mhs_features ft = { (int)o[0], (int64_t)nv, (int64_t)np, (int64_t)nf, xy, po, fo, values == R_NilValue ? NULL : REAL(values) };
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 4));
    for (int k = 0; k < 4; ++k) SET_VECTOR_ELT(out, k, R_NilValue);
    if (pm & 1) SET_VECTOR_ELT(out, 0, Rf_allocVector(INTSXP, n));
    if (pm & 2) SET_VECTOR_ELT(out, 1, Rf_allocVector(INTSXP, n));
    if (pm & 4) SET_VECTOR_ELT(out, 2, Rf_allocVector(REALSXP, n));
    mhs_rasterize_out ro = { (pm & 1) ? (int32_t *)INTEGER(VECTOR_ELT(out, 0)) : NULL, (pm & 2) ? (int32_t *)INTEGER(VECTOR_ELT(out, 1)) : NULL,
                             (pm & 4) ? (void *)REAL(VECTOR_ELT(out, 2)) : NULL, g.ncol, g.ncol, g.ncol, MHS_F64 };
    mhs_rasterize_info info = { 0 };
    int rc = mhs_rasterize(&g, &ft, (int)o[1], o[2] != 0.0, &ro, (int64_t)o[3], &info);
    if (rc == MHS_OK) {
        SET_VECTOR_ELT(out, 3, Rf_allocVector(REALSXP, 8));
        double *inf = REAL(VECTOR_ELT(out, 3));
        inf[0] = (double)info.n_features; inf[1] = (double)info.n_parts; inf[2] = (double)info.n_vertices; inf[3] = (double)info.n_edges;
        inf[4] = (double)info.n_items; inf[5] = (double)info.n_batches; inf[6] = (double)info.n_burned; inf[7] = (double)info.n_outside;
    }
    UNPROTECT(1);
    chk(rc);
    return out;
}

/* Along the D8 flow paths (machisplin_hip.h "flow paths"): height above and distance to the first target cell a cell's own water
 * meets, catchment labels.  flowdir: the integer vector mhsr_hydro returns (0 .. 7, -1 the water leaves, NA_integer_ at NA
 * cells), one per cell; planes, nodata: as for mhsr_resample; opts: c(layer, where, threshold, value_layer, flags, dx, dy) with
 * layer and value_layer 0-based (value_layer is read only for value and drop), where 0 .. 7 as for mhsr_proximity or 8 = outlet,
 * flags 1 = the root counts where a path meets no target, 2 = without the local phase; products: bit mask (1 index, 2 steps,
 * 4 dist, 8 value, 16 drop).  Returns list(index, steps, dist, value, drop, info) in terra cell order, NULL where a plane was
 * not asked for: index the terra cell NUMBER (1-based) of the path's end and steps integer vectors, NA_integer_ where the cell
 * is unreached or NA, the others numeric (NaN there); info = c(n_valid, n_targets, n_roots, n_unreached, max_steps, rounds).
 * Runs on the HOST entry point: the whole plane goes up, there are no row bands. */
SEXP mhsr_flowpath(SEXP geom, SEXP flowdir, SEXP planes, SEXP nodata, SEXP opts, SEXP products) {
    mhs_grid g = grid_from(geom);
    mhs_stack st = planes_from(planes, nodata, &g, "mhsr_flowpath");
    int mask = Rf_asInteger(products);
    if (mask == NA_INTEGER || mask < 1 || mask > 31) Rf_error("mhsr_flowpath: products must be a bit mask of 1 index, 2 steps, 4 dist, 8 value, 16 drop");
    if (!Rf_isReal(opts) || Rf_length(opts) != 7) Rf_error("mhsr_flowpath: opts must be c(layer, where, threshold, value_layer, flags, dx, dy)");
    const double *o = REAL(opts);
    if (!(o[0] >= 0.0 && o[0] <= 2147483647.0)) Rf_error("mhsr_flowpath: layer must be a 0-based layer number");
    if (!(o[1] >= 0.0 && o[1] <= 8.0)) Rf_error("mhsr_flowpath: where must be 0 .. 8");
    if (!(o[4] >= 0.0 && o[4] <= 3.0)) Rf_error("mhsr_flowpath: flags must be 0 .. 3");
    int value_layer = (o[3] >= 0.0 && o[3] <= 2147483647.0) ? (int)o[3] : -1;
    if (!(g.nrow > 0 && g.ncol > 0 && (double)g.nrow * (double)g.ncol <= 2147483647.0)) Rf_error("mhsr_flowpath: bad grid dimension");
    R_xlen_t n = (R_xlen_t)g.nrow * g.ncol;
    if (TYPEOF(flowdir) != INTSXP || Rf_xlength(flowdir) != n) Rf_error("mhsr_flowpath: flowdir must be an integer vector of one code per cell");
    int8_t *dirs = (int8_t *)R_alloc((size_t)n, sizeof(int8_t));
    for (R_xlen_t k = 0; k < n; ++k) {
        int d = INTEGER(flowdir)[k];
        dirs[k] = d == NA_INTEGER ? -2 : (d < -1 || d > 7) ? 127 : (int8_t)d;      /* 127: a code the library refuses (-2 is NA's alone) */
    }
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 6));
    SEXP plane[5] = { R_NilValue, R_NilValue, R_NilValue, R_NilValue, R_NilValue };
    int n_protect = 1;
    for (int k = 0; k < 5; ++k)
        if (mask & (1 << k)) { plane[k] = PROTECT(Rf_allocVector(k < 2 ? INTSXP : REALSXP, n)); ++n_protect; }
    mhs_flowpath_out po = { (mask & 1) ? (int32_t *)INTEGER(plane[0]) : NULL, (mask & 2) ? (int32_t *)INTEGER(plane[1]) : NULL,
                            (mask & 4) ? REAL(plane[2]) : NULL, (mask & 8) ? REAL(plane[3]) : NULL, (mask & 16) ? REAL(plane[4]) : NULL };
    mhs_flowpath_info info = { 0 };
    int rc = mhs_flowpath(&g, dirs, g.ncol, &st, (int)o[0], (int)o[1], o[2], value_layer, (int)o[4], o[5], o[6], &po, MHS_F64, &info);
    if (rc == MHS_OK) {
        if (mask & 1)
            for (R_xlen_t k = 0; k < n; ++k) INTEGER(plane[0])[k] = INTEGER(plane[0])[k] < 0 ? NA_INTEGER : INTEGER(plane[0])[k] + 1;
        if (mask & 2)
            for (R_xlen_t k = 0; k < n; ++k) if (INTEGER(plane[1])[k] < 0) INTEGER(plane[1])[k] = NA_INTEGER;
        SEXP inf = PROTECT(Rf_allocVector(REALSXP, 6)); ++n_protect;
        REAL(inf)[0] = (double)info.n_valid; REAL(inf)[1] = (double)info.n_targets; REAL(inf)[2] = (double)info.n_roots;
        REAL(inf)[3] = (double)info.n_unreached; REAL(inf)[4] = (double)info.max_steps; REAL(inf)[5] = (double)info.rounds;
        for (int k = 0; k < 5; ++k) SET_VECTOR_ELT(out, k, plane[k]);
        SET_VECTOR_ELT(out, 5, inf);
    }
    UNPROTECT(n_protect);
    chk(rc);
    return out;
}

/* predict(model, data.frame) at the stations (V73:477, 501, 525, 586, 608) */
SEXP mhsr_predict_points(SEXP model, SEXP X) {
    SEXP out = PROTECT(Rf_allocVector(REALSXP, Rf_nrows(X)));
    int rc = mhs_predict_points((const mhs_model *)R_ExternalPtrAddr(model), REAL(X), (int64_t)Rf_nrows(X), REAL(out));
    UNPROTECT(1);
    chk(rc);
    return out;
}

/* mgcv::gam(mod.form, data) with the parametric formula (V73:252, V73:600): X = as.matrix(data[, predictors]) */
SEXP mhsr_lm_fit(SEXP X, SEXP y) {
    SEXP out = PROTECT(Rf_allocVector(REALSXP, Rf_ncols(X) + 1));
    int rc = mhs_lm_fit(REAL(X), REAL(y), (int64_t)Rf_nrows(X), Rf_ncols(X), REAL(out));
    UNPROTECT(1);
    chk(rc);
    return out;
}

/* kernlab::ksvm(mod.form, data) (V73:251, V73:560) with kpar = list(sigma = sigma): returns list(beta[n], b,
 * x.center[p], x.scale[p], y.center, y.scale, iterations); the support vectors are the rows with beta != 0 */
SEXP mhsr_svr_fit(SEXP X, SEXP y, SEXP sigma, SEXP C, SEXP epsilon, SEXP tol) {
    if (!Rf_isReal(X) || !Rf_isMatrix(X) || !Rf_isReal(y)) Rf_error("mhsr_svr_fit: X must be a double matrix and y a double vector");
    int n = Rf_nrows(X), p = Rf_ncols(X);
    if (Rf_length(y) != n) Rf_error("mhsr_svr_fit: length(y) = %d but X has %d rows", Rf_length(y), n);
    if (p < 1 || p > 12) Rf_error("mhsr_svr_fit: 1..12 predictors supported, got %d", p);
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 7));
    SEXP beta = PROTECT(Rf_allocVector(REALSXP, n)), xc = PROTECT(Rf_allocVector(REALSXP, p)), xs = PROTECT(Rf_allocVector(REALSXP, p));
    double b = 0, yc = 0, ys = 0;
    int64_t it = 0;
    int rc = mhs_svr_fit(REAL(X), REAL(y), (int64_t)n, p, Rf_asReal(sigma), Rf_asReal(C), Rf_asReal(epsilon), Rf_asReal(tol), 0,
                         REAL(beta), &b, REAL(xc), REAL(xs), &yc, &ys, &it);
    if (rc == 0) {
        SET_VECTOR_ELT(out, 0, beta); SET_VECTOR_ELT(out, 1, Rf_ScalarReal(b)); SET_VECTOR_ELT(out, 2, xc); SET_VECTOR_ELT(out, 3, xs);
        SET_VECTOR_ELT(out, 4, Rf_ScalarReal(yc)); SET_VECTOR_ELT(out, 5, Rf_ScalarReal(ys)); SET_VECTOR_ELT(out, 6, Rf_ScalarReal((double)it));
    }
    UNPROTECT(4);
    chk(rc);
    return out;
}

/* nnet::nnet(mod.form, data = trainNN, size = 10, linout = TRUE, maxit = maxit) (V73:249, V73:463) from the initial
 * weights wts0 (nnet's own: runif(length, -0.7, 0.7)); y already scaled as V73:455-459.
 * returns list(wts, value, counts[2], fail) */
SEXP mhsr_nnet_fit(SEXP X, SEXP y, SEXP wts0, SEXP maxit) {
    if (!Rf_isReal(X) || !Rf_isMatrix(X) || !Rf_isReal(y) || !Rf_isReal(wts0)) Rf_error("mhsr_nnet_fit: X must be a double matrix, y and wts0 double vectors");
    int nw = Rf_length(wts0);
    if (Rf_ncols(X) < 1 || Rf_ncols(X) > 12) Rf_error("mhsr_nnet_fit: 1..12 predictors supported, got %d", Rf_ncols(X));
    if (Rf_length(y) != Rf_nrows(X)) Rf_error("mhsr_nnet_fit: length(y) = %d but X has %d rows", Rf_length(y), Rf_nrows(X));
    if (nw != (Rf_ncols(X) + 1) * 10 + 11) Rf_error("mhsr_nnet_fit: wts0 must hold (ncol(X) + 1) * 10 + 11 = %d weights, got %d", (Rf_ncols(X) + 1) * 10 + 11, nw);
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 4));
    SEXP w = PROTECT(Rf_allocVector(REALSXP, nw)), counts = PROTECT(Rf_allocVector(INTSXP, 2));
    for (int i = 0; i < nw; ++i) REAL(w)[i] = REAL(wts0)[i];
    double value = 0;
    int fail = 0;
    int rc = mhs_nnet_fit(REAL(X), REAL(y), (int64_t)Rf_nrows(X), Rf_ncols(X), 10, REAL(w), Rf_asInteger(maxit), 1e-4, 1e-8,
                          &value, INTEGER(counts), &fail);
    if (rc == 0) {
        SET_VECTOR_ELT(out, 0, w); SET_VECTOR_ELT(out, 1, Rf_ScalarReal(value)); SET_VECTOR_ELT(out, 2, counts);
        SET_VECTOR_ELT(out, 3, Rf_ScalarInteger(fail));
    }
    UNPROTECT(3);
    chk(rc);
    return out;
}

/* gbm::gbm / gbm::gbm.more inside machisplin.gbm.step (V73:1772, 1908, 2101; called at V73:247, 493) for several models in one
 * device call: Xs, ys = lists of double matrices / vectors (one per model, same ncol), bags = list of INTEGER matrices
 * bag_size x n_new (column t = the 1-based rows tree t is grown on, e.g. replicate(n_new, sample.int(n, bag_size)): R's own
 * RNG draws them), Fs = NULL for the first trees or the list of $F vectors a previous call returned (gbm.more).
 * returns a list with, per model, list(F, init_f, tree_offsets, SplitVar, SplitCodePred, LeftNode, RightNode, MissingNode)
 * in mhs_gbm_load's layout (0-based, tree-local children); init_f is NA on a gbm.more call */
SEXP mhsr_gbm_grow(SEXP Xs, SEXP ys, SEXP bags, SEXP depth, SEXP minobs, SEXP shrinkage, SEXP Fs) {
    if (TYPEOF(Xs) != VECSXP || TYPEOF(ys) != VECSXP || TYPEOF(bags) != VECSXP) Rf_error("mhsr_gbm_grow: Xs, ys and bags must be lists");
    int count = Rf_length(Xs), first = Rf_isNull(Fs), d = Rf_asInteger(depth);
    if (count < 1 || Rf_length(ys) != count || Rf_length(bags) != count || (!first && (TYPEOF(Fs) != VECSXP || Rf_length(Fs) != count)))
        Rf_error("mhsr_gbm_grow: need one y, one bag matrix (and one F) per X");
    if (d == NA_INTEGER || d < 1 || d > 64) Rf_error("mhsr_gbm_grow: interaction.depth must be 1..64");
    int p = Rf_ncols(VECTOR_ELT(Xs, 0)), n_new = Rf_ncols(VECTOR_ELT(bags, 0));
    if (n_new < 1) Rf_error("mhsr_gbm_grow: the bag matrices have no columns");
    const double **X = (const double **)R_alloc((size_t)count, sizeof(*X)), **y = (const double **)R_alloc((size_t)count, sizeof(*y));
    const int32_t **b = (const int32_t **)R_alloc((size_t)count, sizeof(*b));
    int64_t *n = (int64_t *)R_alloc((size_t)count, sizeof(*n)), *bs = (int64_t *)R_alloc((size_t)count, sizeof(*bs));
    for (int k = 0; k < count; ++k) {
        SEXP Xk = VECTOR_ELT(Xs, k), yk = VECTOR_ELT(ys, k), bk = VECTOR_ELT(bags, k);
        if (!Rf_isReal(Xk) || !Rf_isMatrix(Xk) || Rf_ncols(Xk) != p || !Rf_isReal(yk) || Rf_length(yk) != Rf_nrows(Xk))
            Rf_error("mhsr_gbm_grow: model %d: X must be a double matrix with %d columns and y a double vector of nrow(X)", k + 1, p);
        if (TYPEOF(bk) != INTSXP || !Rf_isMatrix(bk) || Rf_ncols(bk) != n_new || Rf_nrows(bk) < 1 || Rf_nrows(bk) > Rf_nrows(Xk))
            Rf_error("mhsr_gbm_grow: model %d: bags must be an integer matrix bag_size x %d with bag_size <= nrow(X)", k + 1, n_new);
        if (!first && (!Rf_isReal(VECTOR_ELT(Fs, k)) || Rf_length(VECTOR_ELT(Fs, k)) != Rf_nrows(Xk)))
            Rf_error("mhsr_gbm_grow: model %d: F must be a double vector of nrow(X)", k + 1);
        n[k] = Rf_nrows(Xk); bs[k] = Rf_nrows(bk);
        X[k] = REAL(Xk); y[k] = REAL(yk);
        int32_t *z = (int32_t *)R_alloc((size_t)bs[k] * n_new, sizeof(int32_t));
        for (R_xlen_t e = 0; e < (R_xlen_t)bs[k] * n_new; ++e) {
            if (INTEGER(bk)[e] == NA_INTEGER) Rf_error("mhsr_gbm_grow: model %d: NA in bags", k + 1);
            z[e] = INTEGER(bk)[e] - 1;
        }
        b[k] = z;
    }
    const size_t cap = (size_t)n_new * (3 * (size_t)d + 1);
    double **F = (double **)R_alloc((size_t)count, sizeof(*F)), **val = (double **)R_alloc((size_t)count, sizeof(*val));
    double *init = (double *)R_alloc((size_t)count, sizeof(double));
    int64_t **off = (int64_t **)R_alloc((size_t)count, sizeof(*off));
    int32_t **iv[4];
    for (int a = 0; a < 4; ++a) iv[a] = (int32_t **)R_alloc((size_t)count, sizeof(int32_t *));
    SEXP out = PROTECT(Rf_allocVector(VECSXP, count));
    for (int k = 0; k < count; ++k) {
        SEXP Fk = PROTECT(Rf_allocVector(REALSXP, (R_xlen_t)n[k]));
        if (!first) for (int64_t i = 0; i < n[k]; ++i) REAL(Fk)[i] = REAL(VECTOR_ELT(Fs, k))[i];
        SEXP mk = PROTECT(Rf_allocVector(VECSXP, 8));
        SET_VECTOR_ELT(mk, 0, Fk);
        SET_VECTOR_ELT(out, k, mk);
        UNPROTECT(2);
        F[k] = REAL(Fk);
        off[k] = (int64_t *)R_alloc((size_t)n_new + 1, sizeof(int64_t));
        val[k] = (double *)R_alloc(cap, sizeof(double));
        for (int a = 0; a < 4; ++a) iv[a][k] = (int32_t *)R_alloc(cap, sizeof(int32_t));
    }
    int rc = mhs_gbm_grow_many(count, X, y, n, p, b, bs, n_new, d, Rf_asInteger(minobs), Rf_asReal(shrinkage), first, F, init, off,
                               iv[0], val, iv[1], iv[2], iv[3]);
    if (rc == 0)
        for (int k = 0; k < count; ++k) {
            SEXP mk = VECTOR_ELT(out, k);
            const R_xlen_t nn = (R_xlen_t)off[k][n_new];
            SEXP o = PROTECT(Rf_allocVector(REALSXP, n_new + 1)), v = PROTECT(Rf_allocVector(REALSXP, nn));
            for (int t = 0; t <= n_new; ++t) REAL(o)[t] = (double)off[k][t];
            for (R_xlen_t e = 0; e < nn; ++e) REAL(v)[e] = val[k][e];
            SET_VECTOR_ELT(mk, 1, Rf_ScalarReal(first ? init[k] : R_NaReal)); SET_VECTOR_ELT(mk, 2, o); SET_VECTOR_ELT(mk, 4, v);
            UNPROTECT(2);
            static const int slot[4] = {3, 5, 6, 7};
            for (int a = 0; a < 4; ++a) {
                SEXP w = PROTECT(Rf_allocVector(INTSXP, nn));
                for (R_xlen_t e = 0; e < nn; ++e) INTEGER(w)[e] = iv[a][k][e];
                SET_VECTOR_ELT(mk, slot[a], w);
                UNPROTECT(1);
            }
        }
    UNPROTECT(1);
    chk(rc);
    return out;
}

/* randomForest::randomForest(mod.form, data = train) (V73:248 per CV fold, V73:517 final) on the device: X = double matrix
 * n x p, y = double vector, inbag = INTEGER matrix n x ntree (column t = how many times every row is in tree t's bootstrap,
 * e.g. tabulate(sample.int(n, n, replace = TRUE), n): R's own RNG draws it), seeds = double vector, one whole number in
 * [0, 2^53) per tree (e.g. floor(runif(ntree) * 2^53)) that drives the per-node variable draw.
 * returns list(handle, tree_offsets, leftDaughter, rightDaughter, nodestatus, bestvar, xbestsplit, nodepred, predicted,
 * oob.times, mse, rsq, IncNodePurity): the $forest arrays per tree concatenated (mhs_rf_load's layout), the out-of-bag
 * predictions (NA where no tree left the row out) and mse / rsq over the rows some tree left out */
SEXP mhsr_rf_fit(SEXP X, SEXP y, SEXP inbag, SEXP seeds, SEXP mtry, SEXP nodesize) {
    if (!Rf_isReal(X) || !Rf_isMatrix(X) || !Rf_isReal(y) || Rf_length(y) != Rf_nrows(X))
        Rf_error("mhsr_rf_fit: X must be a double matrix and y a double vector of nrow(X)");
    const int n = Rf_nrows(X), p = Rf_ncols(X);
    if (TYPEOF(inbag) != INTSXP || !Rf_isMatrix(inbag) || Rf_nrows(inbag) != n || Rf_ncols(inbag) < 1)
        Rf_error("mhsr_rf_fit: inbag must be an integer matrix nrow(X) x ntree");
    const int nt = Rf_ncols(inbag);
    if (!Rf_isReal(seeds) || Rf_length(seeds) != nt) Rf_error("mhsr_rf_fit: seeds must be a double vector of ntree whole numbers");
    uint64_t *sd = (uint64_t *)R_alloc((size_t)nt, sizeof(uint64_t));
    for (int t = 0; t < nt; ++t) {
        const double v = REAL(seeds)[t];
        if (!(v >= 0.0 && v < 9007199254740992.0)) Rf_error("mhsr_rf_fit: seeds must lie in [0, 2^53)");
        sd[t] = (uint64_t)v;
    }
    for (R_xlen_t e = 0; e < (R_xlen_t)n * nt; ++e)
        if (INTEGER(inbag)[e] == NA_INTEGER) Rf_error("mhsr_rf_fit: NA in inbag");
    const double *Xp = REAL(X), *yp = REAL(y);
    const int32_t *bp = INTEGER(inbag);
    const uint64_t *sp = sd;
    int64_t nn64 = n, nodes = 0;
    mhs_model *m = NULL;
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 13));
    SEXP pred = PROTECT(Rf_allocVector(REALSXP, n)), times = PROTECT(Rf_allocVector(INTSXP, n)), pur = PROTECT(Rf_allocVector(REALSXP, p));
    SET_VECTOR_ELT(out, 8, pred); SET_VECTOR_ELT(out, 9, times); SET_VECTOR_ELT(out, 12, pur);
    UNPROTECT(3);
    double *predp = REAL(pred), *purp = REAL(pur);
    int32_t *timesp = INTEGER(times);
    int rc = mhs_rf_fit_many(1, &Xp, &yp, &nn64, p, nt, Rf_asInteger(mtry), Rf_asInteger(nodesize), &bp, &sp, &m, &predp, &timesp, &purp);
    if (rc == 0) {
        SET_VECTOR_ELT(out, 0, wrap(m, model_finalizer));
        rc = mhs_rf_get(m, &nodes, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
    }
    if (rc == 0) {
        SEXP off = PROTECT(Rf_allocVector(REALSXP, nt + 1)), l = PROTECT(Rf_allocVector(INTSXP, (R_xlen_t)nodes));
        SEXP r = PROTECT(Rf_allocVector(INTSXP, (R_xlen_t)nodes)), st = PROTECT(Rf_allocVector(INTSXP, (R_xlen_t)nodes));
        SEXP bv = PROTECT(Rf_allocVector(INTSXP, (R_xlen_t)nodes)), xs = PROTECT(Rf_allocVector(REALSXP, (R_xlen_t)nodes));
        SEXP np = PROTECT(Rf_allocVector(REALSXP, (R_xlen_t)nodes));
        SET_VECTOR_ELT(out, 1, off); SET_VECTOR_ELT(out, 2, l); SET_VECTOR_ELT(out, 3, r); SET_VECTOR_ELT(out, 4, st);
        SET_VECTOR_ELT(out, 5, bv); SET_VECTOR_ELT(out, 6, xs); SET_VECTOR_ELT(out, 7, np);
        UNPROTECT(7);
        int64_t *to = (int64_t *)R_alloc((size_t)nt + 1, sizeof(int64_t));
        rc = mhs_rf_get(m, &nodes, INTEGER(l), INTEGER(r), INTEGER(st), INTEGER(bv), REAL(xs), REAL(np), to);
        for (int t = 0; t <= nt && rc == 0; ++t) REAL(off)[t] = (double)to[t];
        double se = 0.0, sy = 0.0, ss = 0.0;
        int seen = 0;
        for (int i = 0; i < n; ++i)
            if (timesp[i] > 0) { const double d = yp[i] - predp[i]; se += d * d; sy += yp[i]; ++seen; }
        for (int i = 0; i < n; ++i)
            if (timesp[i] > 0) { const double d = yp[i] - sy / seen; ss += d * d; }
        for (int i = 0; i < n; ++i)
            if (timesp[i] == 0) predp[i] = R_NaReal;
        SET_VECTOR_ELT(out, 10, Rf_ScalarReal(seen ? se / seen : R_NaReal));
        SET_VECTOR_ELT(out, 11, Rf_ScalarReal(seen ? 1.0 - se / ss : R_NaReal));
    }
    UNPROTECT(1);
    chk(rc);
    return out;
}

/* gbm::predict.gbm(model, x.data[pred.mask, ], n.trees = k * step) for k = 1 .. in one pass (V73:1843, 1919): returns the
 * n x stages matrix machisplin.gbm.step's hold-out deviance curve is computed from */
SEXP mhsr_gbm_staged_points(SEXP model, SEXP X, SEXP step, SEXP n_trees) {
    const mhs_model *m = (const mhs_model *)R_ExternalPtrAddr(model);
    int kind = -1, p = 0, st = Rf_asInteger(step);
    int64_t trees = 0;
    chk(mhs_model_info(m, &kind, &p, &trees));
    if (kind != 4) Rf_error("mhsr_gbm_staged_points: the handle is not a gbm model");
    if (st == NA_INTEGER || st < 1) Rf_error("mhsr_gbm_staged_points: step must be >= 1");
    if (!Rf_isReal(X) || !Rf_isMatrix(X) || Rf_ncols(X) != p) Rf_error("mhsr_gbm_staged_points: X must be a double matrix with %d columns", p);
    /* the library walks the trees the HANDLE holds and writes n x (trees / step) values: the matrix is sized from the
     * handle, and a caller whose n.trees disagrees with it is told so instead of being overrun */
    if (Rf_asInteger(n_trees) != NA_INTEGER && (int64_t)Rf_asInteger(n_trees) != trees)
        Rf_error("mhsr_gbm_staged_points: n.trees = %d but the loaded model has %lld trees", Rf_asInteger(n_trees), (long long)trees);
    int n = Rf_nrows(X), stages = (int)(trees / st);
    SEXP out = PROTECT(Rf_allocMatrix(REALSXP, n, stages));
    int rc = stages > 0 && n > 0 ? mhs_gbm_staged_points(m, REAL(X), (int64_t)n, st, REAL(out)) : 0;
    UNPROTECT(1);
    chk(rc);
    return out;
}

/* machisplin.tiles.merge (V73:1392-1546): tiles = list of numeric vectors (terra::values of each
 * rast.in[[h]] in cell order), win = integer matrix 4 x n (r0, r1, c0, c1 per tile, 0-based) */
SEXP mhsr_tiles_merge(SEXP geom, SEXP tiles, SEXP win, SEXP in_ncol, SEXP in_nrow) {
    mhs_grid g = grid_from(geom);
    int n = Rf_length(tiles);
    const double **h = (const double **)R_alloc((size_t)n, sizeof(*h));
    int64_t *w = (int64_t *)R_alloc((size_t)4 * n, sizeof(int64_t));
    for (int i = 0; i < n; ++i) h[i] = REAL(VECTOR_ELT(tiles, i));
    for (int i = 0; i < 4 * n; ++i) w[i] = (int64_t)INTEGER(win)[i];
    SEXP out = PROTECT(Rf_allocVector(REALSXP, (R_xlen_t)g.nrow * g.ncol));
    int rc = mhs_mosaic_feather(&g, Rf_asInteger(in_nrow), Rf_asInteger(in_ncol), w, h, 1, REAL(out));
    UNPROTECT(1);
    chk(rc);
    return out;
}

/* bracket of the layer loop of machisplin.mltps (V73:176-957): fits of later layers reuse the tiles' reductions */
SEXP mhsr_tps_reduction_cache(SEXP enable) {
    chk(mhs_tps_reduction_cache(Rf_asInteger(enable)));
    return enable;
}

/* ---- several devices from the one R process (include/machisplin_hip.h, "several devices") ---- */

/* mhs_init_devices: n device slots on the devices `ids` (NULL = 0 .. n - 1) */
SEXP mhsr_init_devices(SEXP n, SEXP ids) {
    int nn = Rf_asInteger(n);
    if (nn == NA_INTEGER || nn < 1 || nn > 16) Rf_error("mhsr_init_devices: n must be 1..16");
    if (!Rf_isNull(ids) && Rf_length(ids) != nn) Rf_error("mhsr_init_devices: length(ids) must equal n");
    chk(mhs_init_devices(nn, Rf_isNull(ids) ? NULL : INTEGER(ids)));
    int slots = 0;
    chk(mhs_device_slots(&slots, NULL));
    return Rf_ScalarInteger(slots);
}

/* mhs_multi_trim: give back the device buffers, arenas and pinned rings the two host-plane calls keep between calls */
SEXP mhsr_multi_trim(void) {
    chk(mhs_multi_trim());
    return R_NilValue;
}

static const mhs_model **model_handles(SEXP models, int *n) {
    *n = Rf_length(models);
    const mhs_model **h = (const mhs_model **)R_alloc((size_t)(*n > 0 ? *n : 1), sizeof(*h));
    for (int i = 0; i < *n; ++i) {
        h[i] = (const mhs_model *)R_ExternalPtrAddr(VECTOR_ELT(models, i));
        if (!h[i]) Rf_error("machisplin_hip: a model handle has been freed");
    }
    return h;
}

/* machisplin.mltps Steps 2-5 for one response layer (V73:447-930) over every device slot in ONE call: covars =
 * terra::values(covar.ras) (ncell x C, planar as it stands), X = as.matrix(dat_tps[, predictors]) (n x p: covariates, LONG,
 * LAT), resp the response column.  Returns list(final (terra cell order), rsq.model, rsq.final, lambda, used.tps,
 * n.slots, slot0.share for the next call). */
SEXP mhsr_mltps_grid_multi(SEXP models, SEXP weights, SEXP wt_total, SEXP geom, SEXP covars, SEXP X, SEXP resp, SEXP tile_edge,
                           SEXP lambda, SEXP mode, SEXP slot0_share) {
    mhs_grid g = grid_from(geom);
    int n = 0;
    const mhs_model **h = model_handles(models, &n);
    if (!Rf_isReal(covars) || !Rf_isMatrix(covars) || (int64_t)Rf_nrows(covars) != g.nrow * g.ncol)
        Rf_error("mhsr_mltps_grid_multi: covars must be terra::values(covar.ras), an ncell x layers double matrix");
    if (!Rf_isReal(X) || !Rf_isMatrix(X) || Rf_ncols(X) != Rf_ncols(covars) + 2 || Rf_length(resp) != Rf_nrows(X))
        Rf_error("mhsr_mltps_grid_multi: X must be n x (layers + 2) and resp of length n");
    if (Rf_length(weights) != n) Rf_error("mhsr_mltps_grid_multi: one weight per model");
    mhs_stack st = { REAL(covars), Rf_ncols(covars), MHS_F64, (int64_t)g.nrow * g.ncol, g.ncol, R_NaN };
    double lam = Rf_asReal(lambda), share = Rf_asReal(slot0_share);
    mhs_mltps_info info;
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 7));
    SEXP fin = PROTECT(Rf_allocVector(REALSXP, (R_xlen_t)g.nrow * g.ncol));
    int rc = mhs_mltps_grid_multi(h, REAL(weights), n, Rf_asReal(wt_total), &g, &st, REAL(X), REAL(resp), (int64_t)Rf_nrows(X),
                                  (int64_t)Rf_asInteger(tile_edge), ISNA(lam) ? R_NaN : lam, Rf_asInteger(mode),
                                  ISNA(share) ? R_NaN : share, REAL(fin), &info);
    if (rc == 0) {
        SET_VECTOR_ELT(out, 0, fin); SET_VECTOR_ELT(out, 1, Rf_ScalarReal(info.rsq_model)); SET_VECTOR_ELT(out, 2, Rf_ScalarReal(info.rsq_final));
        SET_VECTOR_ELT(out, 3, Rf_ScalarReal(info.lambda)); SET_VECTOR_ELT(out, 4, Rf_ScalarInteger(info.used_tps));
        SET_VECTOR_ELT(out, 5, Rf_ScalarInteger(info.n_slots)); SET_VECTOR_ELT(out, 6, Rf_ScalarReal(info.suggested_slot0_share));
    }
    UNPROTECT(2);
    chk(rc);
    return out;
}

/* machisplin.tiles.create -> machisplin.mltps Steps 2-5 per (tile, layer) -> machisplin.tiles.merge (README.md:157-215,
 * V73:1165-1256, 1392-1548) over every device slot in ONE call.  units: list of length n.layers * n.tiles, layer-major
 * (unit (l - 1) * n.tiles + t), each list(models, weights, wt.total, X, resp) of that tile's fits and station table.
 * Returns list(planes = list over layers of numeric vectors in terra cell order, rsq = 2 x n.units matrix). */
SEXP mhsr_tiles_units_multi(SEXP geom, SEXP covars, SEXP out_ncol, SEXP out_nrow, SEXP feather_d, SEXP units, SEXP n_layers,
                            SEXP tps, SEXP tile_edge, SEXP lambda, SEXP mode) {
    mhs_grid g = grid_from(geom);
    int L = Rf_asInteger(n_layers), nc = Rf_asInteger(out_ncol), nr = Rf_asInteger(out_nrow);
    if (L == NA_INTEGER || L < 1 || nc < 1 || nr < 1) Rf_error("mhsr_tiles_units_multi: bad layout");
    int nu = Rf_length(units);
    if (nu != L * nc * nr) Rf_error("mhsr_tiles_units_multi: need n.layers * out.ncol * out.nrow = %d units, got %d", L * nc * nr, nu);
    if (!Rf_isReal(covars) || !Rf_isMatrix(covars) || (int64_t)Rf_nrows(covars) != g.nrow * g.ncol)
        Rf_error("mhsr_tiles_units_multi: covars must be terra::values(covar.ras), an ncell x layers double matrix");
    mhs_unit *u = (mhs_unit *)R_alloc((size_t)nu, sizeof(*u));
    for (int i = 0; i < nu; ++i) {
        SEXP e = VECTOR_ELT(units, i);
        if (TYPEOF(e) != VECSXP || Rf_length(e) != 5) Rf_error("mhsr_tiles_units_multi: unit %d must be list(models, weights, wt.total, X, resp)", i + 1);
        int nm = 0;
        u[i].models = model_handles(VECTOR_ELT(e, 0), &nm);
        u[i].n_models = nm; u[i].reserved_ = 0;
        if (Rf_length(VECTOR_ELT(e, 1)) != nm) Rf_error("mhsr_tiles_units_multi: unit %d: one weight per model", i + 1);
        u[i].weights = REAL(VECTOR_ELT(e, 1));
        u[i].wt_total = Rf_asReal(VECTOR_ELT(e, 2));
        SEXP X = VECTOR_ELT(e, 3), y = VECTOR_ELT(e, 4);
        if (!Rf_isReal(X) || !Rf_isMatrix(X) || Rf_ncols(X) != Rf_ncols(covars) + 2 || Rf_length(y) != Rf_nrows(X))
            Rf_error("mhsr_tiles_units_multi: unit %d: X must be n x (layers + 2) and resp of length n", i + 1);
        u[i].X = REAL(X); u[i].resp = REAL(y); u[i].n = (int64_t)Rf_nrows(X);
    }
    mhs_stack st = { REAL(covars), Rf_ncols(covars), MHS_F64, (int64_t)g.nrow * g.ncol, g.ncol, R_NaN };
    double lam = Rf_asReal(lambda);
    SEXP out = PROTECT(Rf_allocVector(VECSXP, 2));
    SEXP planes = PROTECT(Rf_allocVector(VECSXP, L));
    SEXP rsq = PROTECT(Rf_allocMatrix(REALSXP, 2, nu));
    double **ptr = (double **)R_alloc((size_t)L, sizeof(*ptr));
    for (int l = 0; l < L; ++l) {
        SEXP v = PROTECT(Rf_allocVector(REALSXP, (R_xlen_t)g.nrow * g.ncol));
        SET_VECTOR_ELT(planes, l, v);
        UNPROTECT(1);
        ptr[l] = REAL(v);
    }
    int rc = mhs_tiles_units_multi(&g, &st, nc, nr, Rf_asReal(feather_d), L, u, Rf_asInteger(tps), (int64_t)Rf_asInteger(tile_edge),
                                   ISNA(lam) ? R_NaN : lam, Rf_asInteger(mode), ptr, REAL(rsq), NULL);
    if (rc == 0) { SET_VECTOR_ELT(out, 0, planes); SET_VECTOR_ELT(out, 1, rsq); }
    UNPROTECT(3);
    chk(rc);
    return out;
}

/* library.dynam.unload / R exit: the library's streams go while the HIP runtime is still whole (mhs_init also registers
 * an atexit handler, so this is belt and braces) */
void R_unload_machisplin_hip(DllInfo *info) {
    (void)info;
    (void)mhs_shutdown();
}
