"""Inputs of the ksvm row-tile tests (tests/test_ksvm_resident_gpu.py) and of the tool that records the parent commit's
planes (tools/make_ksvm_rowtile_golden.py).  Built on the host from a seeded generator's uniform draws and IEEE's basic
operations only (no libm call), so that the same bits come out on every machine: a recorded plane is only a yardstick for inputs that are bit for bit the recorded ones."""
import hashlib

import numpy as np

GOLDEN_NCOLS = (2688, 2689, 2753, 2817)     # live columns of a row's last tile: 192, 1 (one live lane), 65, 129
GOLDEN_NROW = 5
TILE = 192
CENTER = (1500.0, 40.0, -20.0)
SCALE = (600.0, 25.0, 90.0)


def planes(nrow, ncol, dtype="f32", seed=11, special=True):
    """(3, nrow, ncol) planes as numpy and the NoData value.  With `special` (nrow >= 4): row 1 has an all-NA tile (the
    fourth), row 2 has NA cells inside its LAST tile, row 3 has a spike of 60 scale units on three cells of its LAST tile
    (q = sigma |x|^2 / 700 then spreads 0.3 * 60^2 / 700 = 1.5 > 0.5 over that wave: it must not fold)."""
    rng = np.random.default_rng(seed)
    u = np.arange(ncol, dtype=np.float64)[None, :] / 4096.0
    v = np.arange(nrow, dtype=np.float64)[:, None] / 512.0
    f = [4.0 * u * (1.0 - u) - 0.5 + 0.25 * v, (2.0 * u - 0.7) * (1.0 - v), (u - 0.3) * (u - 0.3) * 4.0 - 0.5 * v]
    z = np.empty((3, nrow, ncol))
    for k in range(3):
        z[k] = CENTER[k] + SCALE[k] * (f[k] + 0.5 * (rng.random((nrow, ncol)) - 0.5))
    last = ((ncol - 1) // TILE) * TILE
    if special and nrow >= 4:
        z[1, 3, last:last + 3] += 60.0 * SCALE[1]      # plane 1: 1 500 units, inside int16
    if dtype == "i16":
        z = np.rint(z)
    na = np.zeros((nrow, ncol), dtype=bool)
    if special and nrow >= 4:
        na[1, 3 * TILE:4 * TILE] = True
        na[2, last::7] = True
        na[2, ncol - 1] = True
    nodata = float("nan")
    if dtype == "i16":
        nodata = -32768.0
        z[:, na] = nodata
        out = z.astype(np.int16)
    else:
        z[:, na] = np.nan
        out = z.astype(np.float32 if dtype == "f32" else np.float64)
    return out, nodata


def host_predictors(geom, pl, nodata):
    """n x 5 float64 predictors (three covariates, LONG, LAT) of every cell, NoData as NaN: what the oracle takes."""
    from oracle import ensemble as oe
    from oracle import tps as otps
    host = pl.astype(np.float64)
    if not np.isnan(nodata):
        host[host == nodata] = np.nan
    x, y = otps.cell_centres(geom.xmin, geom.ymax, geom.xres, geom.yres, geom.nrow, geom.ncol)
    return oe.stack_predictors(host, (x, y))


def svr_params(geom, nsv=37, npos=None, seed=3):
    """A ksvm model for the grid: p = 5, `nsv` support vectors of both signs, `npos` of them with alpha > 0 (default:
    as drawn).  Centres and scales are constants near the planes' own, LONG / LAT scaled to the grid's extent."""
    rng = np.random.default_rng(seed)
    w, h = geom.ncol * geom.xres, geom.nrow * geom.yres
    center = np.array([*CENTER, geom.xmin + w / 2.0, geom.ymax - h / 2.0])
    scale = np.array([*SCALE, w / 4.0, h / 4.0])
    sv = (rng.random((nsv, 5)) - 0.5) * 3.0
    alpha = rng.random(nsv) * 2.0 - 1.0
    alpha[np.abs(alpha) < 0.01] = 0.5
    if npos is not None:
        alpha = np.abs(alpha)
        alpha[npos:] *= -1.0
        alpha = alpha[rng.permutation(nsv)]
    k = int((alpha > 0).sum())
    assert 0 < k < nsv
    return {"kind": "svr", "alpha": alpha, "sv": sv, "b": 0.125, "sigma": 0.3, "x_center": center, "x_scale": scale,
            "y_center": 240.0, "y_scale": 7.5}


def digest(pl, prm):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(pl).tobytes())
    for key in ("alpha", "sv", "x_center", "x_scale"):
        h.update(np.ascontiguousarray(prm[key], dtype=np.float64).tobytes())
    h.update(np.array([prm["b"], prm["sigma"], prm["y_center"], prm["y_scale"]]).tobytes())
    return h.hexdigest()


def golden_cases():
    """(key, ncol, nsv, npos) of the recorded planes: the four widths with 37 support vectors, and the one-live-lane width
    with 131 of which 129 have alpha > 0 -- the kernel stages the support vectors of ONE sign 128 at a time, so it is the
    positive range that has to pass 128 for a second chunk (of one vector: the loop's tail) to exist."""
    return [(f"w{nc}", nc, 37, None) for nc in GOLDEN_NCOLS] + [("w2689_sv131", 2689, 131, 129)]


def row_tile_plane(hip, geom, pl, nodata, prm):
    stack = hip.RasterStack(geom, pl, nodata)
    return hip.predict(stack, hip.models.from_param_dict(prm)).cpu().numpy()
