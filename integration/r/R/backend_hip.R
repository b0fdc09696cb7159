# R side of the drop-in (UNTESTED HERE: no R in the build image).  Each helper replaces one
# call site of machisplin.mltps (V73 = R/ensemble.machine.learning.thin.plate.splines.V73.R)
# and returns the same kind of object the caller consumes (a SpatRaster), so the 7 exported
# functions and their return structure are unchanged.  Selected with
#   options(machisplin.backend = "hip")
# and falling back to the original CRAN call when the library cannot be initialised.

.mhs_geom <- function(r) c(terra::xmin(r), terra::ymax(r), terra::res(r)[1], terra::res(r)[2], nrow(r), ncol(r))

.mhs_ready <- function() {
  if (!identical(getOption("machisplin.backend", "cpu"), "hip")) return(FALSE)
  isTRUE(tryCatch({ .Call("mhsr_init", 0L); TRUE }, error = function(e) FALSE))
}

# ---- flat parameter arrays of the fitted members (loaders in include/machisplin_hip.h) ----
.mhs_model <- function(k, mod, n.covars, max2.resp.f = 1, min.resp.f = 0) {
  p <- n.covars
  switch(k,
    g = .Call("mhsr_lm_load", as.numeric(mod$coefficients)),
    n = .Call("mhsr_nnet_load", as.numeric(mod$wts), p, as.integer(mod$n[2]), max2.resp.f, min.resp.f),
    m = { sel <- mod$selected.terms
          .Call("mhsr_earth_load", as.numeric(mod$coefficients), as.integer(t(mod$dirs[sel, , drop = FALSE])),
                as.numeric(t(mod$cuts[sel, , drop = FALSE])), p) },
    v = { sc <- kernlab::scaling(mod)
          .Call("mhsr_svr_load", as.numeric(unlist(kernlab::coef(mod))), as.numeric(t(kernlab::xmatrix(mod))), p,
                kernlab::b(mod), kernlab::kpar(kernlab::kernelf(mod))$sigma,
                sc$x.scale$`scaled:center`, sc$x.scale$`scaled:scale`,
                sc$y.scale$`scaled:center`, sc$y.scale$`scaled:scale`) },
    b = { nt <- mod$gbm.call$best.trees; tr <- mod$trees[seq_len(nt)]
          cnt <- vapply(tr, function(t) length(t[[1]]), 1L)
          .Call("mhsr_gbm_load", mod$initF, as.numeric(c(0, cumsum(cnt))),
                as.integer(unlist(lapply(tr, `[[`, 1))), as.numeric(unlist(lapply(tr, `[[`, 2))),
                as.integer(unlist(lapply(tr, `[[`, 3))), as.integer(unlist(lapply(tr, `[[`, 4))),
                as.integer(unlist(lapply(tr, `[[`, 5))), p) },
    r = { f <- mod$forest; nb <- f$ndbigtree
          pick <- function(m) unlist(lapply(seq_len(f$ntree), function(t) m[seq_len(nb[t]), t]))
          .Call("mhsr_rf_load", as.numeric(c(0, cumsum(nb))), as.integer(pick(f$leftDaughter)),
                as.integer(pick(f$rightDaughter)), as.integer(pick(f$nodestatus)), as.integer(pick(f$bestvar)),
                as.numeric(pick(f$xbestsplit)), as.numeric(pick(f$nodepred)), p) })
}

# ---- Step 2: pred.elev over the whole raster (replaces the six terra::predict calls and the
#      weighted accumulation, V73:447-619) --------------------------------------------------
mhs_ensemble_raster <- function(covar.ras, handles, OptX.mfit.wt, OptX.mfit.wt.tot) {
  v <- .Call("mhsr_ensemble_predict", handles, as.numeric(OptX.mfit.wt), OptX.mfit.wt.tot,
             .mhs_geom(covar.ras), terra::values(covar.ras))
  terra::setValues(covar.ras[[1]], v)
}

# ---- Step 3 + 4: final.TPS (replaces V73:636-897) ------------------------------------------
mhs_tps_surface <- function(rast_stack, dat, res.FINAL, n.covars, tile.edge = 1500L, lambda = NA_real_) {
  xy <- as.matrix(dat[, c(n.covars, n.covars + 1)])          # LONG, LAT columns (V73:688,751)
  v <- .Call("mhsr_tps_surface", .mhs_geom(rast_stack), xy, as.numeric(res.FINAL), as.numeric(dat[, 2]),
             as.integer(tile.edge), lambda, 0L)
  terra::setValues(terra::rast(rast_stack[[1]]), v)
}

# How terra::interpolate's replacement sums the knots: "auto" (by cost), "direct" (predict.Krig's own loop, results
# bit-identical across windows -- use it when comparing against captured fields output) or "far.field".
mhs_tps_eval_mode <- function(mode = c("auto", "direct", "far.field")) {
  mode <- match.arg(mode)
  invisible(.Call("mhsr_tps_eval_mode", match(mode, c("auto", "direct", "far.field")) - 1L))
}


# ---- a drop-in for the fields::Tps object itself (keeps the R loop of V73:690-753 as it is) ----
# mhs_Tps(xy, y) returns an object of class "machisplin_tps"; terra::interpolate(rast, obj) then works through
# the predict method below (points, block by block), and mhs_interpolate() is the whole-grid fast path.
mhs_Tps <- function(x, Y, lambda = NA_real_) {
  structure(list(handle = .Call("mhsr_tps_fit", as.matrix(x), as.numeric(unlist(Y)), lambda, 0L)),
            class = "machisplin_tps")
}
# lapply(seq_along(xs), function(k) fields::Tps(xs[[k]], Ys[[k]])) in ONE library call: the tiles of V73:690-738 (or the
# response layers of one station table); every fit with 8..256 distinct locations is one workgroup of one kernel launch.
# Returns a list of "machisplin_tps" objects, NULL where a fit failed (the loop of V73:707-738 skips such a tile's spline).
mhs_Tps_many <- function(xs, Ys, lambda = NA_real_) {
  hs <- .Call("mhsr_tps_fit_many", lapply(xs, as.matrix), lapply(Ys, function(y) as.numeric(unlist(y))), lambda, 0L)
  lapply(hs, function(h) if (is.null(h)) NULL else structure(list(handle = h), class = "machisplin_tps"))
}
predict.machisplin_tps <- function(object, x, ...) .Call("mhsr_tps_predict_points", object$handle, as.matrix(x))
mhs_interpolate <- function(r, object) {
  v <- .Call("mhsr_tps_predict_grid", object$handle, .mhs_geom(r), c(0L, nrow(r), 0L, ncol(r)))
  terra::setValues(terra::rast(r), v)
}
# fields::predictSE(fit, x) for the GPU handle: var = (sigma2 / lambda) z' (-M^-1) z, i.e. predictSE.Krig with
# rho = sigma2 / lambda.  sigma2 = NA takes the fit's own sigma^2 hat (fields' shat.GCV^2, mhs_tps_sigma2()); to
# reproduce predictSE of a real fields object pass sigma2 = fit$best.model[2].  At most 2048 distinct stations unless
# mhs_tps_se_max_n() raises the limit (up to 20000): above 2048, Q = -M^-1 is built on the device.
predictSE.machisplin_tps <- function(object, x, sigma2 = NA, ...)
  .Call("mhsr_tps_predict_se_points", object$handle, as.matrix(x), as.numeric(sigma2))
mhs_tps_sigma2 <- function(object) .Call("mhsr_tps_sigma2", object$handle)
# the limit on distinct stations (returns the previous one), and where Q is built: "auto" = host up to 2048, device above
mhs_tps_se_max_n <- function(n) .Call("mhsr_tps_se_max_n", as.numeric(n))
mhs_tps_se_build_mode <- function(mode = c("auto", "host", "device")) {
  mode <- match.arg(mode)
  invisible(.Call("mhsr_tps_se_build_mode", match(mode, c("auto", "host", "device")) - 1L))
}
# terra::interpolate(r, fit, fun = predictSE): the SE at every cell centre of r
mhs_interpolate_se <- function(r, object, sigma2 = NA) {
  v <- .Call("mhsr_tps_predict_se_grid", object$handle, .mhs_geom(r), c(0L, nrow(r), 0L, ncol(r)), as.numeric(sigma2))
  terra::setValues(terra::rast(r), v)
}
# The SE plane of mhs_tps_surface (same arguments): each tile's SE with its own sigma^2 hat, blended by the same mosaic
# and seam feathering (an upper bound on the SE of the blended estimate); NA where only zero tiles reach.
mhs_tps_surface_se <- function(rast_stack, dat, res.FINAL, n.covars, tile.edge = 1500L, lambda = NA_real_) {
  xy <- as.matrix(dat[, c(n.covars, n.covars + 1)])
  v <- .Call("mhsr_tps_surface_se", .mhs_geom(rast_stack), xy, as.numeric(res.FINAL), as.numeric(dat[, 2]),
             as.integer(tile.edge), lambda, 0L)
  terra::setValues(terra::rast(rast_stack[[1]]), v)
}

# ---- where the learners extrapolate: dismo::mess(covar.ras, <the stations' covariates>, full = TRUE) ----------------------
# The MESS extrapolation map (Elith, Kearney & Phillips 2010) of covar.ras against the stations of dat (a dat_tps[[i]]:
# response, the covariates in columns 2 .. n.covars - 1, LONG and LAT in columns n.covars and n.covars + 1; n.covars =
# nlyr(covar.ras) + 2 as at V73:123).  Returns a two-layer SpatRaster: "mess" (negative where at least one covariate is
# outside the stations' range, NA where a covariate is NA) and "mod", the 1-based most dissimilar variable.  lonlat = TRUE
# also places the cell centres' LONG and LAT among the stations' (variables n.covars - 1 and n.covars of "mod").
mhs_mess <- function(covar.ras, dat, n.covars, lonlat = FALSE) {
  ref <- as.matrix(dat[, 2:(if (lonlat) n.covars + 1 else n.covars - 1), drop = FALSE])
  storage.mode(ref) <- "double"
  v <- .Call("mhsr_mess_grid", ref, .mhs_geom(covar.ras), terra::values(covar.ras))
  out <- c(terra::setValues(terra::rast(covar.ras[[1]]), v[[1]]),
           terra::setValues(terra::rast(covar.ras[[1]]), ifelse(v[[2]] < 0L, NA_integer_, v[[2]] + 1L)))
  names(out) <- c("mess", "mod")
  out
}

# ---- topographic covariates from the DEM: what the README's "Need help with the high-resolution topography data?" sends to
# SAGA, GRASS and terra ------------------------------------------------------------------------------------------------
# v: any of .mhs_terrain_vars (3 x 3 window), "above_min" / "below_max" / "minus_mean" (relief in a circular window of `radius`
# cells; above_min is the bundled relative_elevation500m at radius = 17 on 30 m cells) and "geomorphon" (search length `search`
# cells, flatness `flat.deg` degrees; forms 1 flat .. 10 pit).  Returns a SpatRaster with one layer per entry of v.  A lon/lat
# raster gets its cell sizes in metres on the sphere -- the cosine is taken here, the library never calls cos.
.mhs_terrain_vars <- c("dzdx", "dzdy", "slope_tan", "slope_deg", "eastness", "northness", "aspect_deg", "tpi", "tri", "roughness")
.mhs_relief_stats <- c("above_min", "below_max", "minus_mean")
mhs_terrain <- function(dem.ras, v = "slope_deg", radius = 17L, search = 10L, flat.deg = 1, z.factor = 1,
                        lonlat = terra::is.lonlat(dem.ras)) {
  bad <- setdiff(v, c(.mhs_terrain_vars, .mhs_relief_stats, "geomorphon"))
  if (length(bad)) stop("mhs_terrain: unknown variable ", paste(bad, collapse = ", "))
  geom <- .mhs_geom(dem.ras)
  z <- as.numeric(terra::values(dem.ras[[1]]))
  res <- terra::res(dem.ras)
  if (isTRUE(lonlat)) {
    lat <- terra::yFromRow(dem.ras, seq_len(terra::nrow(dem.ras)))
    dx.row <- res[1] * (pi / 180) * 6378137 * cos(lat * (pi / 180))
    units <- c(NA_real_, res[2] * (pi / 180) * 6378137, z.factor)
  } else {
    dx.row <- NULL
    units <- c(res[1], res[2], z.factor)
  }
  layers <- list()
  tv <- intersect(.mhs_terrain_vars, v)                      # ascending bit order: the order of the columns that come back
  if (length(tv)) {
    m <- .Call("mhsr_terrain", geom, z, units, dx.row, as.integer(sum(2^(match(tv, .mhs_terrain_vars) - 1))))
    for (k in seq_along(tv)) layers[[tv[k]]] <- m[, k]
  }
  rs <- intersect(.mhs_relief_stats, v)
  if (length(rs)) {
    m <- .Call("mhsr_relief", geom, z, as.numeric(z.factor), as.integer(radius), as.integer(sum(2^(match(rs, .mhs_relief_stats) - 1))))
    for (k in seq_along(rs)) layers[[rs[k]]] <- m[, k]
  }
  if ("geomorphon" %in% v)
    layers[["geomorphon"]] <- .Call("mhsr_geomorphon", geom, z, units, dx.row, as.integer(search), as.numeric(flat.deg))
  out <- do.call(c, lapply(v, function(n) terra::setValues(terra::rast(dem.ras[[1]]), layers[[n]])))
  names(out) <- v
  out
}

# ---- the topographic wetness index of the DEM (the package bundles a TWI.tif and sends its users to SAGA or GRASS for
# their own) and what it is made from --------------------------------------------------------------------------------------
# v: any of "filled" (the flat-filled surface), "flowdir" (D8: 0 .. 7 = E, SE, S, SW, W, NW, N, NE, -1 where the water leaves
# the raster), "flowacc" (cells draining through the cell, itself included) and "twi" = log(flowacc * sqrt(dx * dy) /
# max(slope of the filled surface, tan(min.slope.deg))).  Always the whole raster: flow accumulation is not local.  Returns a
# SpatRaster with one layer per entry of v; attr(, "info") holds the passes each phase took and the counts of valid, raised
# and sink cells.  max.passes = 0 is the library's cap on the passes of a phase (an error names the phase that reaches it).
.mhs_hydro_products <- c("filled", "flowdir", "flowacc", "twi")
mhs_hydro <- function(dem.ras, v = "twi", min.slope.deg = 0.1, max.passes = 0L, z.factor = 1, lonlat = terra::is.lonlat(dem.ras)) {
  bad <- setdiff(v, .mhs_hydro_products)
  if (length(bad) || !length(v)) stop("mhs_hydro: v must name some of ", paste(.mhs_hydro_products, collapse = ", "))
  res <- terra::res(dem.ras)
  if (isTRUE(lonlat)) {
    lat <- terra::yFromRow(dem.ras, seq_len(terra::nrow(dem.ras)))
    dx.row <- res[1] * (pi / 180) * 6378137 * cos(lat * (pi / 180))
    units <- c(NA_real_, res[2] * (pi / 180) * 6378137, z.factor)
  } else {
    dx.row <- NULL
    units <- c(res[1], res[2], z.factor)
  }
  h <- .Call("mhsr_hydro", .mhs_geom(dem.ras), as.numeric(terra::values(dem.ras[[1]])), units, dx.row,
             as.integer(sum(2^(match(unique(v), .mhs_hydro_products) - 1))), c(tan(min.slope.deg * (pi / 180)), as.numeric(max.passes)))
  out <- do.call(c, lapply(v, function(n) terra::setValues(terra::rast(dem.ras[[1]]), h[[match(n, .mhs_hydro_products)]])))
  names(out) <- v
  attr(out, "info") <- stats::setNames(h[[5]], c("passes_fill", "passes_flat", "passes_acc", "n_valid", "n_raised", "n_sinks"))
  out
}

# The same with MULTIPLE FLOW DIRECTION, what SAGA's catchment area and the bundled TWI.tif use: a cell shares its water among
# all its lower neighbours in proportion to slope ^ convergence (Freeman 1991, Holmgren 1994; 1.1 is SAGA's default) instead of
# sending it to the steepest one -- no parallel one-cell streaks on hillslopes.  v: any of "filled", "flowacc" (a real number
# >= 1) and "twi"; everything else as mhs_hydro.
.mhs_hydro_mfd_products <- c("filled", "flowacc", "twi")
mhs_hydro_mfd <- function(dem.ras, v = "twi", convergence = 1.1, min.slope.deg = 0.1, max.passes = 0L, z.factor = 1,
                          lonlat = terra::is.lonlat(dem.ras)) {
  bad <- setdiff(v, .mhs_hydro_mfd_products)
  if (length(bad) || !length(v)) stop("mhs_hydro_mfd: v must name some of ", paste(.mhs_hydro_mfd_products, collapse = ", "))
  res <- terra::res(dem.ras)
  if (isTRUE(lonlat)) {
    lat <- terra::yFromRow(dem.ras, seq_len(terra::nrow(dem.ras)))
    dx.row <- res[1] * (pi / 180) * 6378137 * cos(lat * (pi / 180))
    units <- c(NA_real_, res[2] * (pi / 180) * 6378137, z.factor)
  } else {
    dx.row <- NULL
    units <- c(res[1], res[2], z.factor)
  }
  h <- .Call("mhsr_hydro_mfd", .mhs_geom(dem.ras), as.numeric(terra::values(dem.ras[[1]])), units, dx.row,
             as.integer(sum(2^(match(unique(v), .mhs_hydro_mfd_products) - 1))),
             c(tan(min.slope.deg * (pi / 180)), as.numeric(max.passes), as.numeric(convergence)))
  out <- do.call(c, lapply(v, function(n) terra::setValues(terra::rast(dem.ras[[1]]), h[[match(n, .mhs_hydro_mfd_products)]])))
  names(out) <- v
  attr(out, "info") <- stats::setNames(h[[4]], c("passes_fill", "passes_flat", "passes_acc", "n_valid", "n_raised", "n_sinks"))
  out
}

# ---- solar covariates of the DEM: what SAGA's "Potential Incoming Solar Radiation" / "Sky View Factor" and GRASS's r.horizon +
# r.sun are used for ----------------------------------------------------------------------------------------------------
# v: any of "svf" (the sky-view factor), "direct" (potential direct insolation on the tilted cell, shadowed by the relief, in
# the units of the tables' w), "sun_hours" (the units of the tables' d) and "horizon" (sixteen layers: the tangent of the
# horizon along N, NNE, NE, ... NNW within `search` cells).  tables: list(entries = n x 8 matrix with the columns t, tan_h, ux,
# uy, uz, w, d, pad; start = 16 offsets per table into its rows and one more, 0-based; omega = 16 weights per table; tab_row =
# NULL or one table number per row of the raster, 1-based) -- section "solar" of machisplin_hip.h says what they mean.  The
# library does no trigonometry: the tables carry the sun.  Making them (the Python package's sun_tables) is not restated in R;
# write them from Python or build them with the formulas of that section.  tables = NULL serves v = "horizon" alone.
.mhs_solar_products <- c("svf", "direct", "sun_hours", "horizon")
.mhs_solar_dirs <- c("N", "NNE", "NE", "ENE", "E", "ESE", "SE", "SSE", "S", "SSW", "SW", "WSW", "W", "WNW", "NW", "NNW")
mhs_solar <- function(dem.ras, search = 10L, tables = NULL, v = "svf", z.factor = 1, lonlat = terra::is.lonlat(dem.ras)) {
  bad <- setdiff(v, .mhs_solar_products)
  if (length(bad) || !length(v)) stop("mhs_solar: v must name some of ", paste(.mhs_solar_products, collapse = ", "))
  res <- terra::res(dem.ras)
  if (isTRUE(lonlat)) {
    lat <- terra::yFromRow(dem.ras, seq_len(terra::nrow(dem.ras)))
    dx.row <- res[1] * (pi / 180) * 6378137 * cos(lat * (pi / 180))
    units <- c(NA_real_, res[2] * (pi / 180) * 6378137, z.factor)
  } else {
    dx.row <- NULL
    units <- c(res[1], res[2], z.factor)
  }
  if (!is.null(tables)) {
    entries <- as.matrix(tables$entries); storage.mode(entries) <- "double"
    tables <- list(entries, as.numeric(tables$start), as.numeric(tables$omega),
                   if (is.null(tables$tab_row)) NULL else as.integer(tables$tab_row) - 1L)
  }
  v <- unique(v)
  pv <- intersect(.mhs_solar_products, v)                     # ascending bit order: the order of the columns that come back
  m <- .Call("mhsr_solar", .mhs_geom(dem.ras), as.numeric(terra::values(dem.ras[[1]])), units, dx.row, as.integer(search),
             as.integer(sum(2^(match(pv, .mhs_solar_products) - 1))), tables)
  first <- cumsum(c(1L, ifelse(pv == "horizon", 16L, 1L)))
  layers <- list()
  for (n in v) {
    k <- first[match(n, pv)]
    cols <- if (n == "horizon") k:(k + 15L) else k
    for (j in seq_along(cols)) {
      r <- terra::setValues(terra::rast(dem.ras[[1]]), m[, cols[j]])
      names(r) <- if (n == "horizon") paste0("horizon_", .mhs_solar_dirs[j]) else n
      layers <- c(layers, list(r))
    }
  }
  do.call(c, layers)
}

# ---- rasters onto one grid: what the README's "All rasters must be the same: resolution, projection and extent" leaves to
# terra::crop, terra::resample and terra::extract ---------------------------------------------------------------------------
# x: a SpatRaster in the coordinate system of y (no reprojection); y: the SpatRaster whose grid the result takes.  method: "near",
# "bilinear", "cubic" interpolate at y's cell centres; "mean", "min", "max", "sum", "count" take x's cells whose centre lies
# in y's cell (a 30 m product onto the 1 km grid the stations were sampled from).  Every layer of x goes through one call.
# Section "resample" of machisplin_hip.h states the rules; they are the library's own, not terra's bit for bit.
.mhs_resample_methods <- c("near", "bilinear", "cubic", "mean", "min", "max", "sum", "count")
mhs_resample <- function(x, y, method = "bilinear") {
  m <- match(method, .mhs_resample_methods)
  if (length(method) != 1L || is.na(m)) stop("mhs_resample: method must be one of ", paste(.mhs_resample_methods, collapse = ", "))
  v <- terra::values(x); storage.mode(v) <- "double"
  out <- .Call("mhsr_resample", .mhs_geom(x), v, NA_real_, .mhs_geom(y), as.integer(m - 1L))
  r <- terra::rast(y[[1]], nlyrs = terra::nlyr(x))
  r <- terra::setValues(r, out)
  names(r) <- names(x)
  r
}
# terra::extract(x, xy, method = ) for a matrix of coordinates: "simple" (the cell that holds the point), "bilinear", "cubic"
mhs_extract <- function(x, xy, method = "simple") {
  m <- match(method, c("simple", "bilinear", "cubic"))
  if (length(method) != 1L || is.na(m)) stop("mhs_extract: method must be simple, bilinear or cubic")
  xy <- as.matrix(xy[, 1:2]); storage.mode(xy) <- "double"
  v <- terra::values(x); storage.mode(v) <- "double"
  out <- .Call("mhsr_extract", .mhs_geom(x), v, NA_real_, xy, as.integer(m - 1L))
  colnames(out) <- names(x)
  out
}

# ---- rasters into another coordinate system: the README's "projection" ---------------------------------------------------------
# x: a SpatRaster; y: the SpatRaster whose grid (in ANOTHER coordinate system) the result takes; lattice: list(step, sx, sy) made by
# the caller -- step a power of two, sx and sy matrices of (ceil(nrow(y) / step) + 1) x (ceil(ncol(y) / step) + 1) nodes, node
# [a + 1, b + 1] the coordinates IN x's SYSTEM of y's grid point (xmin(y) + b step xres(y), ymax(y) - a step yres(y)), e.g. by
# terra::project(cbind(X, Y), from = terra::crs(y), to = terra::crs(x)); NA where the transform has no value.  The library
# interpolates the lattice at y's cell centres and takes x there by "near", "bilinear" or "cubic" (section "warp" of
# machisplin_hip.h; the rules are mhs_resample's).  How far the lattice is from the exact transform is the caller's to check: halve
# step until the midpoints of the lattice cells agree with PROJ to the tolerance wanted (the Python side's project.lattice_from
# does this; an R restatement is out of scope, as for sun_tables).  A much coarser y: mhs_resample(x, ., "mean") first.
mhs_warp <- function(x, y, lattice, method = "bilinear") {
  m <- match(method, c("near", "bilinear", "cubic"))
  if (length(method) != 1L || is.na(m)) stop("mhs_warp: method must be near, bilinear or cubic (aggregate with mhs_resample in x's system first)")
  step <- as.integer(lattice$step)
  nodes <- c(ceiling(terra::nrow(y) / step) + 1, ceiling(terra::ncol(y) / step) + 1)
  sx <- as.matrix(lattice$sx); sy <- as.matrix(lattice$sy)
  if (!all(dim(sx) == nodes) || !all(dim(sy) == nodes)) stop("mhs_warp: lattice$sx and lattice$sy must be ", nodes[1], " x ", nodes[2], " matrices")
  v <- terra::values(x); storage.mode(v) <- "double"
  out <- .Call("mhsr_warp", .mhs_geom(x), v, NA_real_, .mhs_geom(y), step, as.double(t(sx)), as.double(t(sy)), as.integer(m - 1L))
  r <- terra::rast(y[[1]], nlyrs = terra::nlyr(x))
  r <- terra::setValues(r, out)
  names(r) <- names(x)
  r
}

# ---- terra::focal at any radius (machisplin_hip.h "focal"): the multi-scale covariates -- TPI and DEV over kilometres, the sd of
# elevation, the smoothed terrain -- that mhs_terrain's relief, limited to 45 cells, stops short of -------------------------------
# x: a SpatRaster (layer `layer` is used); radius: 1 .. 8 radii in cells, each up to max(nrow, ncol); stats: any of .mhs_focal_stats;
# shape "square" (every statistic) or "circle" (count, sum, mean, sd, minus_mean, dev); fill.na: make the statistics that do not
# use the centre at NA cells too; offset: what the values are centred by before they are squared and summed (default: the layer's
# rounded mean).  Returns a SpatRaster with one layer per radius and statistic, named <stat><radius>.
.mhs_focal_stats <- c("count", "sum", "mean", "sd", "min", "max", "range", "minus_mean", "above_min", "below_max", "dev")
mhs_focal <- function(x, radius, stats = "mean", layer = 1L, shape = "square", fill.na = FALSE, offset = NULL) {
  bad <- setdiff(stats, .mhs_focal_stats)
  if (length(bad)) stop("mhs_focal: unknown statistic ", paste(bad, collapse = ", "))
  s <- match(shape, c("square", "circle"))
  if (length(shape) != 1L || is.na(s)) stop("mhs_focal: shape must be square or circle")
  if (s == 2L && any(stats %in% c("min", "max", "range", "above_min", "below_max")))
    stop("mhs_focal: a circle gives the sum family only; mhs_terrain has above_min and below_max in a circle for radius <= 45, shape = \"square\" beyond")
  v <- terra::values(x[[layer]])
  if (is.null(offset)) offset <- round(mean(v, na.rm = TRUE))
  if (!is.finite(offset)) offset <- 0
  st <- intersect(.mhs_focal_stats, stats)                   # ascending bit order: the order of the columns that come back
  m <- .Call("mhsr_focal", .mhs_geom(x), as.numeric(v), NA_real_, c(0, s - 1, as.numeric(isTRUE(fill.na)), as.numeric(offset)),
             as.integer(radius), as.integer(sum(2^(match(st, .mhs_focal_stats) - 1))))
  cols <- as.vector(outer(seq_along(st), (seq_along(radius) - 1L) * length(st), "+"))
  names.all <- as.vector(outer(st, as.integer(radius), paste0))
  want <- as.vector(outer(stats, as.integer(radius), paste0))
  out <- terra::rast(x[[layer]], nlyrs = length(want))
  terra::values(out) <- m[, cols[match(want, names.all)], drop = FALSE]
  names(out) <- want
  out
}

# ---- distance-to-feature covariates: what terra::distance and terra::gridDist are used for ---------------------------------
# x: a SpatRaster with square cells.  A cell is a feature where layer `layer` is NA (where = "na": the sea of a land-only DEM),
# not NA ("valid"), or "lt" "le" "gt" "ge" "eq" "ne" `threshold`.  v: any of "d2" (squared distance in cells, exact), "index"
# (the nearest feature's cell number; ties go to the smaller row, then the smaller column), "dist" (sqrt(d2) * unit), "dir_x",
# "dir_y" (the unit vector towards the feature, y to the north) and "value" (layer `value.layer` at the nearest feature).
# unit = NULL takes the cell width.  Section "proximity" of machisplin_hip.h states the rule; geodesic distance on lon/lat
# rasters, cost distance and a search radius are out of scope.
.mhs_proximity_where <- c("na", "valid", "lt", "le", "gt", "ge", "eq", "ne")
.mhs_proximity_products <- c("d2", "index", "dist", "dir_x", "dir_y", "value")
mhs_proximity <- function(x, where = "na", threshold = NA_real_, v = "dist", layer = 1L, value.layer = NA_integer_, unit = NULL) {
  w <- match(where, .mhs_proximity_where)
  if (length(where) != 1L || is.na(w)) stop("mhs_proximity: where must be one of ", paste(.mhs_proximity_where, collapse = ", "))
  if (w > 2L && is.na(threshold)) stop("mhs_proximity: where = \"", where, "\" needs a threshold")
  bad <- setdiff(v, .mhs_proximity_products)
  if (length(bad) || !length(v)) stop("mhs_proximity: v must name some of ", paste(.mhs_proximity_products, collapse = ", "))
  if ("value" %in% v && is.na(value.layer)) stop("mhs_proximity: the value product needs value.layer")
  res <- terra::res(x)
  if (is.null(unit)) {
    if (abs(res[1] - res[2]) > 1e-9 * max(res)) stop("mhs_proximity: the cells are not square; resample x (mhs_resample) or give unit")
    unit <- res[1]
  }
  v <- unique(v)
  pv <- match(v, .mhs_proximity_products)
  vals <- terra::values(x); storage.mode(vals) <- "double"
  out <- .Call("mhsr_proximity", .mhs_geom(x), vals, NA_real_,
               c(layer - 1, w - 1, if (w > 2L) threshold else 0, if (is.na(value.layer)) -1 else value.layer - 1, unit),
               as.integer(sum(2^(pv - 1))))
  layers <- lapply(seq_along(v), function(j) {
    r <- terra::setValues(terra::rast(x[[1]]), out[[pv[j]]])
    names(r) <- v[j]
    r
  })
  r <- do.call(c, layers)
  attr(r, "info") <- stats::setNames(out[[7]], c("n_features", "max_d2"))
  r
}

# ---- connected patches of a mask: what terra::patches and a size filter (a sieve) are used for ------------------------------
# x: a SpatRaster.  A cell is a feature by `where` and `threshold` as for mhs_proximity (default "valid": the cells that are not
# NA).  Two feature cells are neighbours under directions = 4 or 8 (terra::patches' name for it).  v: any of "label" (the cell
# number of the patch's first cell, NA off the features), "id" (1 .. K in that order: terra::patches' numbering; 0 off the
# features), "size", "edge" (1 where the patch touches the raster's edge) and "keep" (1 where min.size <= size <= max.size and
# the patch meets edge = "any", "touching" or "interior").  mhs_proximity(r[["keep"]], where = "ne", threshold = 0) then measures
# to the patches that were kept.  Section "patches" of machisplin_hip.h states the rule; patches of equal value and wrap-around
# at the date line are out of scope; the statistics of another layer per patch are mhs_zonal below.
.mhs_patches_products <- c("label", "id", "size", "edge", "keep")
.mhs_patches_edge <- c("any", "touching", "interior")
mhs_patches <- function(x, where = "valid", threshold = NA_real_, directions = 8L, v = "id", min.size = 1, max.size = Inf, edge = "any",
                        layer = 1L) {
  w <- match(where, .mhs_proximity_where)
  if (length(where) != 1L || is.na(w)) stop("mhs_patches: where must be one of ", paste(.mhs_proximity_where, collapse = ", "))
  if (w > 2L && is.na(threshold)) stop("mhs_patches: where = \"", where, "\" needs a threshold")
  if (length(directions) != 1L || !(directions %in% c(4, 8))) stop("mhs_patches: directions must be 4 or 8")
  bad <- setdiff(v, .mhs_patches_products)
  if (length(bad) || !length(v)) stop("mhs_patches: v must name some of ", paste(.mhs_patches_products, collapse = ", "))
  if (is.na(min.size) || min.size < 1 || min.size != floor(min.size)) stop("mhs_patches: min.size must be a whole number >= 1")
  if (is.na(max.size) || max.size < min.size) stop("mhs_patches: max.size must not be below min.size")
  e <- match(edge, .mhs_patches_edge)
  if (length(edge) != 1L || is.na(e)) stop("mhs_patches: edge must be one of ", paste(.mhs_patches_edge, collapse = ", "))
  v <- unique(v)
  pv <- match(v, .mhs_patches_products)
  vals <- terra::values(x); storage.mode(vals) <- "double"
  out <- .Call("mhsr_patches", .mhs_geom(x), vals, NA_real_,
               c(layer - 1, w - 1, if (w > 2L) threshold else 0, directions, min.size, max.size, e - 1),
               as.integer(sum(2^(pv - 1))))
  layers <- lapply(seq_along(v), function(j) {
    r <- terra::setValues(terra::rast(x[[1]]), out[[pv[j]]])
    names(r) <- v[j]
    r
  })
  r <- do.call(c, layers)
  attr(r, "info") <- stats::setNames(out[[6]], c("n_features", "n_patches", "n_kept_patches", "n_kept_cells", "max_size"))
  r
}

# ---- zonal statistics: what terra::zonal is used for, and the statistics put back on the cells --------------------------------
# x: a SpatRaster whose layer `layer` holds the values.  z: a one-layer SpatRaster of whole zone numbers >= 0 on the same grid --
# mhs_patches(v = "id") (its 0 off the features is then a zone of its own: subtract 1 or mask it), the "index" layer of
# mhs_flowpath(where = "outlet"), a land-cover raster; NA or a negative number = no zone.  stats: the table's statistics, any of
# count sum mean sd min max range cells (NULL: no table); planes: the statistics wanted on the cells, any of those and
# minus_mean above_min below_max dev.  present = TRUE gives only the zones that have a cell (the form for cell-number labels).
# n.zones = NULL and quantum = NULL leave both to the library.  Returns list(table = a data.frame with the column zone, planes = a
# SpatRaster or NULL, info).  Section "zonal" of machisplin_hip.h states the rule: the values are quantised to whole multiples of
# `quantum`, a power of two, and every sum is an exact integer; info[["n_inexact"]] = 0 says the statistics are those of the
# input itself.  Median and mode, zones given as fractions and cell-area weights are out of scope.
.mhs_zonal_stats <- c("count", "sum", "mean", "sd", "min", "max", "range", "minus_mean", "above_min", "below_max", "dev", "cells")
.mhs_zonal_table <- c("count", "sum", "mean", "sd", "min", "max", "range", "cells")
mhs_zonal <- function(x, z, stats = "mean", planes = NULL, present = TRUE, n.zones = NULL, quantum = NULL, layer = 1L) {
  if (length(setdiff(stats, .mhs_zonal_table))) stop("mhs_zonal: stats must name some of ", paste(.mhs_zonal_table, collapse = ", "))
  if (length(setdiff(planes, .mhs_zonal_stats))) stop("mhs_zonal: planes must name some of ", paste(.mhs_zonal_stats, collapse = ", "))
  if (!length(stats) && !length(planes)) stop("mhs_zonal: no output: stats and planes are both empty")
  if (terra::ncell(z) != terra::ncell(x) || terra::ncol(z) != terra::ncol(x)) stop("mhs_zonal: shape mismatch: z is not on the grid of x")
  if (!is.null(n.zones) && (is.na(n.zones) || n.zones < 1 || n.zones > 2147483647)) stop("mhs_zonal: n.zones must be in 1 .. 2^31 - 1")
  if (!is.null(quantum) && (is.na(quantum) || quantum <= 0 || log2(quantum) != floor(log2(quantum)))) stop("mhs_zonal: quantum must be a power of two")
  stats <- unique(stats); planes <- unique(planes)
  zv <- terra::values(z[[1]])[, 1]
  if (any(zv != floor(zv), na.rm = TRUE)) stop("mhs_zonal: zones given as fractions are out of scope")
  vals <- terra::values(x); storage.mode(vals) <- "double"
  bits <- function(v) as.integer(sum(2^(match(v, .mhs_zonal_stats) - 1)))
  out <- .Call("mhsr_zonal", .mhs_geom(x), vals, NA_real_, as.integer(zv),
               c(layer - 1, if (is.null(n.zones)) 0 else n.zones, if (is.null(quantum)) 0 else quantum, as.numeric(isTRUE(present))),
               bits(stats), bits(planes))
  table <- NULL
  if (length(stats)) {
    cols <- stats::setNames(out[[1]][1L + match(stats, .mhs_zonal_table)], stats)
    zone <- if (isTRUE(present)) out[[1]][[1]] else seq_along(cols[[1]]) - 1L
    table <- data.frame(zone = zone, cols)
  }
  r <- NULL
  if (length(planes)) {
    layers <- lapply(planes, function(p) {
      l <- terra::setValues(terra::rast(x[[1]]), out[[2]][[match(p, .mhs_zonal_stats)]])
      names(l) <- p
      l
    })
    r <- do.call(c, layers)
  }
  list(table = table, planes = r,
       info = stats::setNames(out[[3]], c("n_zones", "n_present", "n_cells_in_zones", "n_contributing", "n_nonfinite", "n_inexact", "quantum")))
}

# ---- zonal quantiles: the median (any quantile) per zone, per coarser cell, of the whole layer -------------------------------------
# Section "zonal quantiles" of machisplin_hip.h: R's type 7 quantile (stats::quantile's default) of the quantised values, from a
# deterministic device sort.  z = NULL: the whole layer (terra::global).  planes: some of "q", "below", "frac_below".
# Returns list(table = data.frame(zone, count, q<p> ...), planes = SpatRaster or NULL, info).
mhs_zonal_quantile <- function(x, z = NULL, probs = 0.5, planes = NULL, present = TRUE, n.zones = NULL, quantum = NULL, layer = 1L) {
  .mhs_quantile_planes <- c("q", "below", "frac_below")
  if (!length(probs) || length(probs) > 16 || any(is.na(probs)) || any(probs < 0 | probs > 1)) stop("mhs_zonal_quantile: probs must be 1 .. 16 probabilities in [0, 1]")
  if (length(setdiff(planes, .mhs_quantile_planes))) stop("mhs_zonal_quantile: planes must name some of q, below, frac_below")
  if (!is.null(z) && (terra::ncell(z) != terra::ncell(x) || terra::ncol(z) != terra::ncol(x))) stop("mhs_zonal_quantile: shape mismatch: z is not on the grid of x")
  if (!is.null(n.zones) && (is.null(z) || is.na(n.zones) || n.zones < 1 || n.zones > 2147483647)) stop("mhs_zonal_quantile: n.zones goes with z and must be in 1 .. 2^31 - 1")
  if (!is.null(quantum) && (is.na(quantum) || quantum <= 0 || log2(quantum) != floor(log2(quantum)))) stop("mhs_zonal_quantile: quantum must be a power of two")
  zv <- NULL
  if (!is.null(z)) {
    zv <- terra::values(z[[1]])[, 1]
    if (any(zv != floor(zv), na.rm = TRUE)) stop("mhs_zonal_quantile: zones given as fractions are out of scope")
    zv <- as.integer(zv)
  }
  vals <- terra::values(x); storage.mode(vals) <- "double"
  planes <- unique(planes)
  out <- .Call("mhsr_zonal_quantile", .mhs_geom(x), vals, NA_real_, zv, NULL,
               c(layer - 1, if (is.null(n.zones)) 0 else n.zones, if (is.null(quantum)) 0 else quantum, as.numeric(isTRUE(present)), 1,
                 sum(2^(match(planes, .mhs_quantile_planes) - 1))),
               as.numeric(probs))
  q <- matrix(out[[1]][[3]], ncol = length(probs), byrow = TRUE)
  colnames(q) <- paste0("q", probs)
  zone <- if (isTRUE(present)) out[[1]][[1]] else seq_len(nrow(q)) - 1L
  table <- data.frame(zone = zone, count = out[[1]][[2]], q, check.names = FALSE)
  r <- NULL
  if (length(planes)) {
    layers <- list()
    if ("q" %in% planes) for (j in seq_along(probs)) {
      l <- terra::setValues(terra::rast(x[[1]]), out[[2]][[1]][[j]]); names(l) <- paste0("q", probs[j]); layers <- c(layers, l)
    }
    if ("below" %in% planes) { l <- terra::setValues(terra::rast(x[[1]]), out[[2]][[2]]); names(l) <- "below"; layers <- c(layers, l) }
    if ("frac_below" %in% planes) { l <- terra::setValues(terra::rast(x[[1]]), out[[2]][[3]]); names(l) <- "frac_below"; layers <- c(layers, l) }
    r <- do.call(c, layers)
  }
  list(table = table, planes = r,
       info = stats::setNames(out[[3]], c("n_zones", "n_present", "n_cells_in_zones", "n_contributing", "n_nonfinite", "n_inexact", "quantum", "passes_run")))
}

# terra::aggregate(x, fun = median) and its quantiles onto the grid of y (same coordinate system, any resolution, origin and
# extent): a cell of y takes the cells of x whose centre lies in it, resample's footprints.  Returns a SpatRaster on y's grid with
# one layer per probability and the layer "count".
mhs_aggregate_quantile <- function(x, y, probs = 0.5, quantum = NULL, layer = 1L) {
  if (!length(probs) || length(probs) > 16 || any(is.na(probs)) || any(probs < 0 | probs > 1)) stop("mhs_aggregate_quantile: probs must be 1 .. 16 probabilities in [0, 1]")
  if (!is.null(quantum) && (is.na(quantum) || quantum <= 0 || log2(quantum) != floor(log2(quantum)))) stop("mhs_aggregate_quantile: quantum must be a power of two")
  vals <- terra::values(x); storage.mode(vals) <- "double"
  out <- .Call("mhsr_zonal_quantile", .mhs_geom(x), vals, NA_real_, NULL, .mhs_geom(y),
               c(layer - 1, 0, if (is.null(quantum)) 0 else quantum, 0, 1, 0), as.numeric(probs))
  q <- matrix(out[[1]][[3]], ncol = length(probs), byrow = TRUE)
  layers <- lapply(seq_along(probs), function(j) { l <- terra::setValues(terra::rast(y[[1]]), q[, j]); names(l) <- paste0("q", probs[j]); l })
  cnt <- terra::setValues(terra::rast(y[[1]]), out[[1]][[2]]); names(cnt) <- "count"
  do.call(c, c(layers, cnt))
}

# ---- categorical layers: class counts, fractions and mode per zone and per coarser cell -------------------------------------------
# What terra::crosstab and terra::aggregate(fun = "modal") are used for, and how a land-cover raster enters a covariate stack: as
# class fractions.  Section "classes" of machisplin_hip.h states the rule: a value is the class whose code it equals exactly, every
# other valid value is `other`, every accumulator is an exact integer count, and a tie of the mode goes to the SMALLER code (terra's
# modal takes the first occurrence).  classes: the class codes, whole numbers in 0 .. 65535, at most 256 (NULL: the codes present in
# the layer); frac.of: the codes whose fraction is wanted (NULL: all).
#
# mhs_class_crosstab: x, z, n.zones as for mhs_zonal.  stats: any of counts n other cells mode mode_frac variety simpson frac (NULL: no
# table); planes: any of mode mode_frac variety simpson n frac.  Returns list(table = a data.frame with the column zone -- counts and
# frac as one column per code, counts_<code> and frac_<code> --, planes = a SpatRaster or NULL, info, codes).  The table is dense:
# renumber cell-number labels first -- mhs_patches(v = "label") by its "id" layer minus 1; the "index" layer of mhs_flowpath (basins) by
# match(v, sort(unique(v))) - 1, NOT through mhs_patches, which would merge basins that touch.
.mhs_class_table <- c("counts", "n", "other", "cells", "mode", "mode_frac", "variety", "simpson", "frac")
.mhs_class_planes <- c("mode", "mode_frac", "variety", "simpson", "n", "frac")
.mhs_class_products <- c("mode", "variety", "n", "mode_frac", "simpson", "frac")
.mhs_class_codes <- function(who, what, v) {
  if (is.null(v)) return(NULL)
  if (!length(v) || length(v) > 256L || anyNA(v) || any(v != floor(v)) || any(v < 0 | v > 65535)) stop(who, ": ", what, " must hold 1 .. 256 whole numbers in 0 .. 65535")
  if (anyDuplicated(v)) stop(who, ": ", what, " names a code twice")
  as.integer(v)
}
.mhs_class_layers <- function(template, lst, names.all, wanted, codes) {
  layers <- lapply(wanted, function(p) {
    v <- lst[[match(p, names.all)]]
    l <- terra::setValues(terra::rast(template[[1]], nlyrs = if (is.matrix(v)) ncol(v) else 1L), v)
    names(l) <- if (is.matrix(v)) paste0("frac_", codes) else p
    l
  })
  do.call(c, layers)
}
mhs_class_crosstab <- function(x, z, classes = NULL, stats = "counts", planes = NULL, frac.of = NULL, n.zones = NULL, layer = 1L) {
  who <- "mhs_class_crosstab"
  if (length(setdiff(stats, .mhs_class_table))) stop(who, ": stats must name some of ", paste(.mhs_class_table, collapse = ", "))
  if (length(setdiff(planes, .mhs_class_planes))) stop(who, ": planes must name some of ", paste(.mhs_class_planes, collapse = ", "))
  if (!length(stats) && !length(planes)) stop(who, ": no output: stats and planes are both empty")
  if (terra::ncell(z) != terra::ncell(x) || terra::ncol(z) != terra::ncol(x)) stop(who, ": shape mismatch: z is not on the grid of x")
  if (!is.null(n.zones) && (is.na(n.zones) || n.zones < 1 || n.zones > 2147483647)) stop(who, ": n.zones must be in 1 .. 2^31 - 1")
  classes <- .mhs_class_codes(who, "classes", classes); frac.of <- .mhs_class_codes(who, "frac.of", frac.of)
  if (!is.null(classes) && length(setdiff(frac.of, classes))) stop(who, ": frac.of names a code that is not in classes")
  stats <- unique(stats); planes <- unique(planes)
  zv <- terra::values(z[[1]])[, 1]
  if (any(zv != floor(zv), na.rm = TRUE)) stop(who, ": zones given as fractions are out of scope")
  vals <- terra::values(x); storage.mode(vals) <- "double"
  bits <- function(v, all) as.integer(sum(2^(match(v, all) - 1)))
  out <- .Call("mhsr_class_crosstab", .mhs_geom(x), vals, NA_real_, as.integer(zv), c(layer - 1, if (is.null(n.zones)) 0 else n.zones),
               classes, frac.of, bits(stats, .mhs_class_table), bits(planes, .mhs_class_planes))
  codes <- out[[4]]
  fcodes <- if (is.null(frac.of)) codes else frac.of
  table <- NULL
  if (length(stats)) {
    cols <- lapply(stats, function(s) {
      v <- out[[1]][[match(s, .mhs_class_table)]]
      if (!is.matrix(v)) return(stats::setNames(data.frame(v), s))
      stats::setNames(as.data.frame(t(v)), paste0(s, "_", if (s == "counts") codes else fcodes))       # a zone is a column of the shim's matrix
    })
    table <- do.call(cbind, c(list(data.frame(zone = seq_len(out[[3]][2]) - 1L)), cols))
  }
  list(table = table, planes = if (length(planes)) .mhs_class_layers(x, out[[2]], .mhs_class_planes, planes, fcodes) else NULL,
       info = stats::setNames(out[[3]], c("K", "n_zones", "n_valid", "n_na", "n_other")), codes = codes)
}
# mhs_class_aggregate: every product of layer `layer` of x on the grid of y (one coordinate system), the unit of a cell of y being the
# cells of x whose centre lies in it (mhs_resample's aggregates).  v: any of mode variety n mode_frac simpson frac.  A SpatRaster with
# one layer per entry of v (frac: one per code, frac_<code>); attr(, "info") and attr(, "codes").  A cell of y that holds no centre of
# a cell of x has n = 0, mode NA.
mhs_class_aggregate <- function(x, y, classes = NULL, v = "mode", frac.of = NULL, layer = 1L) {
  who <- "mhs_class_aggregate"
  if (!length(v) || length(setdiff(v, .mhs_class_products))) stop(who, ": v must name some of ", paste(.mhs_class_products, collapse = ", "))
  classes <- .mhs_class_codes(who, "classes", classes); frac.of <- .mhs_class_codes(who, "frac.of", frac.of)
  if (!is.null(classes) && length(setdiff(frac.of, classes))) stop(who, ": frac.of names a code that is not in classes")
  v <- unique(v)
  vals <- terra::values(x); storage.mode(vals) <- "double"
  out <- .Call("mhsr_class_aggregate", .mhs_geom(x), vals, NA_real_, .mhs_geom(y), c(layer - 1), classes, frac.of,
               as.integer(sum(2^(match(v, .mhs_class_products) - 1))))
  if ("mode" %in% v) out[[1]][[1]][out[[1]][[1]] < 0L] <- NA_integer_
  r <- .mhs_class_layers(y, out[[1]], .mhs_class_products, v, if (is.null(frac.of)) out[[3]] else frac.of)
  attr(r, "info") <- stats::setNames(out[[2]], c("K", "n_zones", "n_valid", "n_na", "n_other"))
  attr(r, "codes") <- out[[3]]
  r
}

# ---- rasterize: points, lines and polygons burned onto the grid (what terra::rasterize is used for) --------------------------
# x: a SpatRaster that gives the grid.  coords: a numeric matrix of two columns (x, y) in the grid's coordinate system;
# part.offsets: 0-based vertex numbers that cut it into parts (a ring of a polygon, a polyline, a run of points), one more than
# there are parts; feature.offsets: 0-based part numbers that group the parts into features, one more than there are features --
# with terra, g <- terra::geom(v) gives coords = g[, c("x", "y")], the parts from the runs of (geom, part, hole) and the features
# from the runs of geom.  values: one number per feature (a field of the vector), or NULL.  v: the layers wanted, any of "index"
# (the winning feature, 1-based as a row of the vector; NA for none -- minus 1 it is a zone plane for mhs_zonal), "count" (the
# number of features on the cell; for points the number of points in it) and "value" (values[index]; NA for none -- what
# mhs_proximity(where = "valid") takes).  rule: which feature wins where several cover a cell, "last" or "first" in the vector's
# order, "max" or "min" of values.  touches = TRUE adds every cell that a polygon's ring passes through to the centre rule.
# Section "rasterize" of machisplin_hip.h states the rule; partial-coverage fractions, sums of overlapping values, line width and
# buffers, and validity repair are out of scope.
.mhs_rasterize_kinds <- c("point", "line", "polygon")
.mhs_rasterize_rules <- c("last", "first", "max", "min")
.mhs_rasterize_products <- c("index", "count", "value")
mhs_rasterize <- function(x, coords, part.offsets, feature.offsets, values = NULL, kind = "polygon", v = "index", rule = "last", touches = FALSE,
                          scratch.budget = NULL) {
  if (!kind %in% .mhs_rasterize_kinds) stop("mhs_rasterize: kind must be one of ", paste(.mhs_rasterize_kinds, collapse = ", "))
  if (!rule %in% .mhs_rasterize_rules) stop("mhs_rasterize: rule must be one of ", paste(.mhs_rasterize_rules, collapse = ", "))
  if (!length(v) || length(setdiff(v, .mhs_rasterize_products))) stop("mhs_rasterize: v must name some of ", paste(.mhs_rasterize_products, collapse = ", "))
  if (is.null(values) && ("value" %in% v || rule %in% c("max", "min"))) stop("mhs_rasterize: values is missing: \"value\", \"max\" and \"min\" need it")
  if (!is.null(scratch.budget) && (is.na(scratch.budget) || scratch.budget < 1)) stop("mhs_rasterize: scratch.budget must be a positive number of bytes")
  v <- unique(v)
  coords <- as.matrix(coords); storage.mode(coords) <- "double"
  out <- .Call("mhsr_rasterize", .mhs_geom(x), coords, as.integer(part.offsets), as.integer(feature.offsets),
               if (is.null(values)) NULL else as.numeric(values),
               c(match(kind, .mhs_rasterize_kinds) - 1, match(rule, .mhs_rasterize_rules) - 1, as.numeric(isTRUE(touches)),
                 if (is.null(scratch.budget)) 0 else scratch.budget),
               as.integer(sum(2^(match(v, .mhs_rasterize_products) - 1))))
  layers <- lapply(v, function(p) {
    vals <- out[[match(p, .mhs_rasterize_products)]]
    if (p == "index") vals <- ifelse(vals < 0L, NA_integer_, vals + 1L)
    l <- terra::setValues(terra::rast(x[[1]]), vals)
    names(l) <- p
    l
  })
  r <- do.call(c, layers)
  attr(r, "info") <- stats::setNames(out[[4]], c("n_features", "n_parts", "n_vertices", "n_edges", "n_items", "n_batches", "n_burned", "n_outside"))
  r
}

# ---- flow-path covariates: HAND, SAGA's vertical / horizontal distance to channel network, catchment labels ------------------
# flowdir: the one-layer SpatRaster of D8 directions that the hydrology call makes (0 .. 7 = E, SE, S, SW, W, NW, N, NE, -1 the
# water leaves, NA).  x: a SpatRaster on the same grid whose layer `layer` defines the targets -- `where` as for mhs_proximity,
# or "outlet": no targets, every path runs to its root -- and whose layer `value.layer` supplies values.  v: any of "index" (the
# cell number of the first target on the cell's own flow path; with "outlet" a catchment label), "steps", "dist" (the path's
# length; dx, dy default to the cell size), "value" (layer value.layer there) and "drop" (that layer at the cell minus there:
# the height above the drainage when it is the DEM).  root.is.target: a path that meets no target ends at its root; otherwise
# its cells are NA.  Section "flow paths" of machisplin_hip.h states the rule; lon/lat rasters are out of scope for "dist".
.mhs_flowpath_where <- c(.mhs_proximity_where, "outlet")
.mhs_flowpath_products <- c("index", "steps", "dist", "value", "drop")
mhs_flowpath <- function(flowdir, x, where = "outlet", threshold = NA_real_, v = "index", layer = 1L, value.layer = NA_integer_,
                         root.is.target = TRUE, dx = NULL, dy = NULL) {
  w <- match(where, .mhs_flowpath_where)
  if (length(where) != 1L || is.na(w)) stop("mhs_flowpath: where must be one of ", paste(.mhs_flowpath_where, collapse = ", "))
  if (w > 2L && w < 9L && is.na(threshold)) stop("mhs_flowpath: where = \"", where, "\" needs a threshold")
  bad <- setdiff(v, .mhs_flowpath_products)
  if (length(bad) || !length(v)) stop("mhs_flowpath: v must name some of ", paste(.mhs_flowpath_products, collapse = ", "))
  if (any(c("value", "drop") %in% v) && is.na(value.layer)) stop("mhs_flowpath: the value and drop products need value.layer")
  if ("dist" %in% v && terra::is.lonlat(x, perhaps = TRUE, warn = FALSE) && (is.null(dx) || is.null(dy)))
    stop("mhs_flowpath: dist on a lon/lat raster is out of scope; project x or give dx and dy")
  res <- terra::res(x)
  if (is.null(dx)) dx <- res[1]
  if (is.null(dy)) dy <- res[2]
  v <- unique(v)
  pv <- match(v, .mhs_flowpath_products)
  vals <- terra::values(x); storage.mode(vals) <- "double"
  dirs <- as.integer(terra::values(flowdir[[1]]))
  out <- .Call("mhsr_flowpath", .mhs_geom(x), dirs, vals, NA_real_,
               c(layer - 1, w - 1, if (w > 2L && w < 9L) threshold else 0, if (is.na(value.layer)) -1 else value.layer - 1,
                 if (root.is.target) 1 else 0, dx, dy),
               as.integer(sum(2^(pv - 1))))
  layers <- lapply(seq_along(v), function(j) {
    r <- terra::setValues(terra::rast(x[[1]]), out[[pv[j]]])
    names(r) <- v[j]
    r
  })
  r <- do.call(c, layers)
  attr(r, "info") <- stats::setNames(out[[6]], c("n_valid", "n_targets", "n_roots", "n_unreached", "max_steps", "rounds"))
  r
}

# ---- learner fits on the device (SURVEY.md 8f rank 4); every one keeps the CRAN call as its fallback -----------------
# kernlab::ksvm(mod.form, data = dat) (V73:251, V73:560).  sigma: kernlab draws it with sigest() from a random half
# of the rows -- do the same here so that the two backends see the same kernel width.
.mhs_ksvm <- function(dat, sigma = mean(kernlab::sigest(as.matrix(dat[, -1]), scaled = TRUE)[c(1, 3)])) {
  X <- as.matrix(dat[, -1]); p <- ncol(X)
  f <- .Call("mhsr_svr_fit", X, as.numeric(dat[, 1]), sigma, 1.0, 0.1, 0.001)
  sv <- which(f[[1]] != 0)
  Z <- sweep(sweep(X[sv, , drop = FALSE], 2, f[[3]]), 2, f[[4]], "/")
  list(handle = .Call("mhsr_svr_load", as.numeric(f[[1]][sv]), as.numeric(t(Z)), p, f[[2]], sigma, f[[3]], f[[4]], f[[5]], f[[6]]),
       beta = f[[1]], b = f[[2]], sigma = sigma, iterations = f[[7]])
}
# nnet::nnet(mod.form, data = trainNN, size = 10, linout = TRUE, maxit = 10000) (V73:249, V73:463); trainNN$resp is
# already (resp - min) / max (V73:455-459)
.mhs_nnet <- function(trainNN, max2.resp.f, min.resp.f, maxit = 10000L) {
  X <- as.matrix(trainNN[, -1]); p <- ncol(X)
  f <- .Call("mhsr_nnet_fit", X, as.numeric(trainNN[, 1]), runif((p + 1) * 10 + 11, -0.7, 0.7), as.integer(maxit))
  list(handle = .Call("mhsr_nnet_load", f[[1]], p, 10L, max2.resp.f, min.resp.f), wts = f[[1]], value = f[[2]], convergence = f[[4]])
}
# gbm::gbm / gbm::gbm.more inside machisplin.gbm.step (V73:1772 per fold, V73:1908 per stage, V73:2101 final): n.new more trees
# for ALL the given models in one device call.  Xs / ys: lists (one per fold model: x.data[model.mask, ], y.data[model.mask]);
# state: NULL for the first trees, else what the previous call returned.  The bags are drawn HERE with R's RNG
# (sample.int without replacement, floor(bag.fraction * n) rows per tree), so set.seed() governs them as it governs gbm's.
.mhs_gbm_grow <- function(Xs, ys, n.new, state = NULL, tree.complexity = 25L, learning.rate = 0.01, bag.fraction = 0.5,
                          n.minobsinnode = 10L) {
  Xs <- lapply(Xs, as.matrix); ys <- lapply(ys, as.numeric)
  bags <- lapply(Xs, function(X) { b <- replicate(n.new, sample.int(nrow(X), floor(bag.fraction * nrow(X)))); storage.mode(b) <- "integer"; b })
  Fs <- if (is.null(state)) NULL else lapply(state, function(s) s[[1]])
  .Call("mhsr_gbm_grow", Xs, ys, bags, as.integer(tree.complexity), as.integer(n.minobsinnode), learning.rate, Fs)
}
# randomForest::randomForest(mod.form, data = train) (V73:248 per CV fold, V73:517 final), regression defaults, grown on the
# device.  The bootstrap counts and the per-tree seeds of the variable draws are drawn HERE with R's RNG, so set.seed() governs
# them; they are not randomForest's own C-level draws, so the forest is randomForest's for these bags and draws, not for the
# same seed (and the random tie-break of recent releases is not reproduced).  Returns the handle for the "r" slot plus the
# $forest arrays, the OOB predictions, mse and rsq.
.mhs_rf <- function(dat, ntree = 500L, mtry = max(floor((ncol(dat) - 1) / 3), 1), nodesize = 5L) {
  X <- as.matrix(dat[, -1, drop = FALSE]); storage.mode(X) <- "double"
  n <- nrow(X)
  inbag <- replicate(ntree, tabulate(sample.int(n, n, replace = TRUE), n)); storage.mode(inbag) <- "integer"
  f <- .Call("mhsr_rf_fit", X, as.numeric(dat[, 1]), inbag, floor(runif(ntree) * 2^53), as.integer(mtry), as.integer(nodesize))
  names(f) <- c("handle", "tree_offsets", "leftDaughter", "rightDaughter", "nodestatus", "bestvar", "xbestsplit", "nodepred",
                "predicted", "oob.times", "mse", "rsq", "IncNodePurity")
  f
}
# inside machisplin.gbm.step's loop (V73:1843, 1919): the hold-out predictions of fold model i for every stage at once,
# instead of one predict.gbm per gbm.more
.mhs_gbm_holdout_stages <- function(handle, x.holdout, step.size, n.fitted)
  .Call("mhsr_gbm_staged_points", handle, as.matrix(x.holdout), as.integer(step.size), as.integer(n.fitted))


# ---- Step 2 as it is threaded through machisplin.mltps (V73:442-619), all six members -----------------------------------
# The loop  for(k in mods.run)  keeps its fits, its variable-importance lines and its station residuals (O(stations) work in
# the packages); only the raster side of each  if (k=="x")  block -- the terra::predict(rast_stack, model) pair and the
# pred.elev accumulation -- is replaced by ONE call that records the fitted member, and the division by the weight total
# after the loop by ONE call that evaluates all recorded members in a single pass over the raster.  The edit list, by V73
# line (INTEGRATION.md section 2 repeats it):
#   before V73:447   hip <- .mhs_ready(); S2 <- .mhs_step2_new()
#   V73:468-475 (n)  if (hip) S2 <- .mhs_step2_member(S2, "n", mod.nn.tps.FINAL,   OptX.mfit.wt[[iter.mod]], n.covars, max2.resp.f, min.resp.f) else { <the eight lines> }
#   V73:497-499 (b)  if (hip) S2 <- .mhs_step2_member(S2, "b", mod.brt.tps.FINAL,  OptX.mfit.wt[[iter.mod]], n.covars) else { <the three lines> }
#   V73:521-523 (r)  if (hip) S2 <- .mhs_step2_member(S2, "r", mod.rf.tps.FINAL,   OptX.mfit.wt[[iter.mod]], n.covars) else { ... }
#   V73:543-545 (m)  if (hip) S2 <- .mhs_step2_member(S2, "m", mod.MARS.tps.FINAL, OptX.mfit.wt[[iter.mod]], n.covars) else { ... }
#   V73:582-584 (v)  if (hip) S2 <- .mhs_step2_member(S2, "v", mod.SVM.tps.FINAL,  OptX.mfit.wt[[iter.mod]], n.covars) else { ... }
#   V73:604-606 (g)  if (hip) S2 <- .mhs_step2_member(S2, "g", mod.GAM.tps.FINAL,  OptX.mfit.wt[[iter.mod]], n.covars) else { ... }
#   V73:619          pred.elev <- if (hip) .mhs_step2_finish(S2, covar.ras, OptX.mfit.wt.tot) else (pred.elev/OptX.mfit.wt.tot)
# The members are summed in the loop's order (mods.run), each times its weight, then divided by the unrounded total -- the
# arithmetic of V73:471-475 ... 606 and 619.
.mhs_step2_new <- function() list(handles = list(), wts = numeric(0))
.mhs_step2_member <- function(S2, k, mod, wt, n.covars, max2.resp.f = 1, min.resp.f = 0) {
  S2$handles[[length(S2$handles) + 1L]] <- .mhs_model(k, mod, n.covars, max2.resp.f, min.resp.f)
  S2$wts <- c(S2$wts, as.numeric(wt))
  S2
}
.mhs_step2_finish <- function(S2, covar.ras, OptX.mfit.wt.tot) mhs_ensemble_raster(covar.ras, S2$handles, S2$wts, OptX.mfit.wt.tot)
