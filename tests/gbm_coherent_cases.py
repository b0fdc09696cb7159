"""Inputs of the coherent gbm kernel's bit tests (tests/test_gbm_coherent_parent_gpu.py) and of the tool that records the
parent commit's planes (tools/make_gbm_coherent_golden.py).  Built on the host from a seeded generator's draws and IEEE's
basic operations only (no libm call), so that the same bits come out on every machine: a recorded plane is only a yardstick
for inputs that are bit for bit the recorded ones, and the SHA-256 stored beside each plane tells the two apart.

The kernel classifies every tree against a wave's tile of 16 x 16 cells (anchored to the grid at multiples of 16): a split
STRADDLES when some cell of the tile lies left of it and some cell right.  straddle_histogram() counts on the host, from
the cells' ranks among the model's thresholds, how many (tile, tree) pairs have 0 .. 5 straddling levels; `rough` (the
white-noise share of a plane) is what moves a case between the classes."""
import functools
import hashlib

import numpy as np

TILE = 16
NROW, NCOL = 40, 1100
CENTER = (1500.0, 400.0, -20.0, 180.0, 0.0, 0.5)
SCALE = (900.0, 300.0, 120.0, 150.0, 40.0, 0.4)

# key: dtype, layers, trees, n_splits, window (None: (0, NROW, 0, 1000)), rough, nodata_frac, grid (nrow, ncol), forced
CASES = {
    "smooth_f32_900":   dict(dtype="f32", C=3, trees=900, n_splits=5, window=None, rough=0.0, nodata_frac=0.0),
    "fast_f32_na":      dict(dtype="f32", C=3, trees=900, n_splits=5, window=None, rough=0.6, nodata_frac=0.01),
    "f64_clipped":      dict(dtype="f64", C=3, trees=900, n_splits=5, window=(3, 37, 40, 1040), rough=0.25, nodata_frac=0.01),
    "i16_three_splits": dict(dtype="i16", C=3, trees=900, n_splits=3, window=None, rough=0.1, nodata_frac=0.01),
    "one_split":        dict(dtype="f32", C=3, trees=900, n_splits=1, window=(0, 40, 0, 1000), rough=0.1, nodata_frac=0.01),
    "trees_64":         dict(dtype="f32", C=3, trees=64, n_splits=5, window=None, rough=0.05, nodata_frac=0.0),
    "trees_70":         dict(dtype="f32", C=3, trees=70, n_splits=5, window=None, rough=0.4, nodata_frac=0.0),
    "p8":               dict(dtype="f32", C=6, trees=300, n_splits=5, window=(0, 48, 0, 1000), rough=0.15, nodata_frac=0.01,
                             grid=(48, 1100)),
    "probe_2p20":       dict(dtype="f32", C=3, trees=300, n_splits=5, window=(0, 1024, 0, 1024), rough=0.0, nodata_frac=0.0,
                             grid=(1024, 1024), forced=False, smooth_scale=4.0),
}


def case_names():
    return list(CASES)


def _spec(name):
    d = dict(grid=(NROW, NCOL), forced=True, smooth_scale=1.0)
    d.update(CASES[name])
    if d["window"] is None:
        d["window"] = (0, d["grid"][0], 0, 1000)
    return d


def planes(nrow, ncol, C, dtype, rough, nodata_frac, smooth_scale=1.0, seed=17):
    """(C, nrow, ncol) planes as numpy and the NoData value: a smooth polynomial field per layer (a 16-cell tile spans a
    fraction of a percent of its range) plus `rough` x uniform noise over the field's whole range; NoData on the same
    `nodata_frac` of cells in every layer."""
    rng = np.random.default_rng(seed)
    u = np.arange(ncol, dtype=np.float64)[None, :] / (8192.0 * smooth_scale)
    v = np.arange(nrow, dtype=np.float64)[:, None] / (2048.0 * smooth_scale)
    z = np.empty((C, nrow, ncol))
    for k in range(C):
        a, b, c = 0.3 + 0.2 * k, 1.0 - 0.15 * k, 0.2 * (k % 3)
        f = a * u * (1.0 - u) * 4.0 + b * v * (1.0 - 0.5 * v) + c * (u - 0.4) * (v + 0.1) * 6.0 - 0.5
        z[k] = CENTER[k % 6] + SCALE[k % 6] * ((1.0 - rough) * f + rough * (rng.random((nrow, ncol)) - 0.5))
    na = rng.random((nrow, ncol)) < nodata_frac
    if dtype == "i16":
        z = np.rint(z)
        z[:, na] = -32768.0
        return z.astype(np.int16), -32768.0
    z[:, na] = np.nan
    return z.astype(np.float32 if dtype == "f32" else np.float64), float("nan")


def host_predictors(geom, pl, nodata):
    """n x p float64 predictors (the covariates, LONG, LAT) of every cell, NoData as NaN."""
    from oracle import ensemble as oe
    from oracle import tps as otps
    host = pl.astype(np.float64)
    if not np.isnan(nodata):
        host[host == nodata] = np.nan
    x, y = otps.cell_centres(geom.xmin, geom.ymax, geom.xres, geom.yres, geom.nrow, geom.ncol)
    return oe.stack_predictors(host, (x, y))


def digest(pl, prm):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(pl).tobytes())
    for key in ("tree_offsets", "split_var", "left", "right", "missing"):
        h.update(np.ascontiguousarray(prm[key], dtype=np.int64).tobytes())
    h.update(np.ascontiguousarray(prm["split_val"], dtype=np.float64).tobytes())
    h.update(np.array([prm["init_f"], float(prm["p"])]).tobytes())
    return h.hexdigest()


def plane_digest(plane):
    """SHA-256 of a predicted plane's float64 bits (NaN pattern included): the planes are too large to be stored whole."""
    return hashlib.sha256(np.ascontiguousarray(plane, dtype=np.float64).tobytes()).hexdigest()


def sample(plane):
    """The cells of a plane that are stored beside its digest (every row, every 13th column: all 16 tile columns occur),
    so that a failing digest can be told from a failing everything."""
    return np.ascontiguousarray(plane[:, 5::13] if plane.shape[0] <= 64 else plane[7::29, 5::13])


@functools.lru_cache(maxsize=None)
def build(name):
    """(geometry, planes, nodata, model parameters, window, forced) of a case."""
    from machisplin_amd import synth
    d = _spec(name)
    nrow, ncol = d["grid"]
    geom = synth.grid(nrow, ncol)
    pl, nodata = planes(nrow, ncol, d["C"], d["dtype"], d["rough"], d["nodata_frac"], d["smooth_scale"])
    X = host_predictors(geom, pl, nodata)
    rng = np.random.default_rng(29)
    ok = np.flatnonzero(~np.isnan(X).any(axis=1))
    idx = rng.choice(ok, 1500, replace=False)
    Xs = X[idx]
    uu, vv = (idx % ncol + 0.5) / ncol, (idx // ncol + 0.5) / nrow
    ys = 250.0 - 0.0055 * Xs[:, 0] + 12.0 * uu * (1.0 - uu) + 2.0 * vv * vv + (rng.random(idx.size) - 0.5)
    prm = synth.gbm_params(Xs, ys, 3, n_trees=d["trees"], n_splits=d["n_splits"])
    return geom, pl, nodata, prm, d["window"], d["forced"]


def straddle_histogram(name):
    """Counts of (tile, tree) pairs with 0 .. 5 straddling levels over the case's window, from the cells' ranks among the
    sorted distinct thresholds of each predictor (rank = thresholds <= value; a split with threshold rank c sends rank < c
    left): a level straddles when min rank < c <= max rank over the tile's cells that are not NoData."""
    geom, pl, nodata, prm, win, _ = build(name)
    p = prm["p"]
    nrow, ncol = geom.nrow, geom.ncol
    X = host_predictors(geom, pl, nodata).reshape(nrow, ncol, p)
    na = np.isnan(X).any(axis=2)
    r0, r1, c0, c1 = win
    var = prm["split_var"].reshape(len(prm["tree_offsets"]) - 1, -1)
    val = prm["split_val"].reshape(var.shape)
    hist = np.zeros(6, dtype=np.int64)
    ranks, cthr = [], np.zeros(var.shape, dtype=np.int64)
    for j in range(p):
        sv = np.unique(val[var == j])
        ranks.append(np.searchsorted(sv, X[:, :, j], side="right"))
        cthr[var == j] = np.searchsorted(sv, val[var == j], side="left") + 1
    inner = var >= 0
    for tr in range(r0 - r0 % TILE, r1, TILE):
        for tc in range(c0 - c0 % TILE, c1, TILE):
            rs, cs = slice(max(tr, r0), min(tr + TILE, r1)), slice(max(tc, c0), min(tc + TILE, c1))
            live = ~na[rs, cs]
            if not live.any():
                continue
            mn = np.array([ranks[j][rs, cs][live].min() for j in range(p)])
            mx = np.array([ranks[j][rs, cs][live].max() for j in range(p)])
            vv = np.where(inner, var, 0)
            strad = inner & (mn[vv] < cthr) & (cthr <= mx[vv])
            hist += np.bincount(strad.sum(axis=1), minlength=6)[:6]
    return hist


def predict(hip, name, env=()):
    """The case's plane through hip.predict, with the given environment switches set for the call."""
    import os
    geom, pl, nodata, prm, win, forced = build(name)
    stack = hip.RasterStack(geom, pl, nodata)
    model = hip.models.from_param_dict(prm)
    keys = tuple(env) + (("MHS_GBM_FORCE_COHERENT",) if forced and "MHS_GBM_NO_COHERENT" not in env else ())
    for k in keys:
        os.environ[k] = "1"
    try:
        return hip.predict(stack, model, window=win).cpu().numpy(), model
    finally:
        for k in keys:
            del os.environ[k]


def probe_last(model):
    """(cost, count) of the model's last probe launch."""
    import ctypes as C
    from machisplin_amd import _lib
    cst, cnt = C.c_longlong(0), C.c_longlong(0)
    _lib.check(_lib.lib().mhs_gbm_probe_last(model._h, C.byref(cst), C.byref(cnt)))
    return int(cst.value), int(cnt.value)
