"""The resampling rules of include/machisplin_hip.h, section "resample", restated in numpy: what the GPU tests compare the
library with, bit for bit.  Every operation stands in the header's order and is rounded once; sums are made by explicit loops
over the taps and over the footprint's columns and rows (never np.sum, whose pairwise order is not the rule's), vectorised only
ACROSS target cells, which are independent.

Geometries are anything with xmin, ymax, xres, yres, nrow, ncol (machisplin_amd.Geometry).  A source is a 2-D array of int16,
float32 or float64 with the stack's nodata; outputs are float64 with NaN for NA."""
import numpy as np

METHODS = ("near", "bilinear", "cubic", "mean", "min", "max", "sum", "count")


def to_double(z, nodata):
    """the plane converted exactly to double, NA (NaN or nodata) as NaN"""
    a = np.array(z, dtype=np.float64)
    if not np.isnan(nodata):
        a[a == nodata] = np.nan
    return a


def cell_x(T, c):
    return T.xmin + (np.asarray(c, dtype=np.float64) + 0.5) * T.xres


def cell_y(T, r):
    return T.ymax - (np.asarray(r, dtype=np.float64) + 0.5) * T.yres


def _cell_from(v, lo, hi, res, n, from_hi):
    """colFromX (from_hi False: v - lo) / rowFromY (from_hi True: hi - v): the far edge belongs to the last cell, -1 outside"""
    with np.errstate(invalid="ignore"):
        q = np.floor(((hi - v) if from_hi else (v - lo)) / res)
        q = np.where(q < n - 1, q, n - 1)
        far = (v == lo) if from_hi else (v == hi)
        inside = (v >= lo) & (v <= hi)
    q = np.where(far, n - 1, q)
    return np.where(inside, q, -1).astype(np.int64)


def col_from_x(S, x):
    x = np.asarray(x, dtype=np.float64)
    return _cell_from(x, S.xmin, S.xmin + float(S.ncol) * S.xres, S.xres, S.ncol, False)


def row_from_y(S, y):
    y = np.asarray(y, dtype=np.float64)
    return _cell_from(y, S.ymax - float(S.nrow) * S.yres, S.ymax, S.yres, S.nrow, True)


def axis(d, res, n):
    """f = d / res - 0.5 held in [-4, n + 4]; (i0 = floor(f), t = f - i0)"""
    with np.errstate(invalid="ignore"):
        f = d / res - 0.5
        f = np.where(f >= -4.0, f, -4.0)
        f = np.where(f > n + 4.0, n + 4.0, f)
    fl = np.floor(f)
    return fl.astype(np.int64), f - fl


def cubic_weights(t):
    return [((-0.5 * t + 1.0) * t - 0.5) * t, ((1.5 * t - 2.5) * t) * t + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t, ((0.5 * t - 0.5) * t) * t]


def _get(z, i, j):
    """(has a value, the value or 0) of the cells (i, j)"""
    nr, nc = z.shape
    ok = (i >= 0) & (i < nr) & (j >= 0) & (j < nc)
    v = z[np.clip(i, 0, nr - 1), np.clip(j, 0, nc - 1)]
    ok = ok & ~np.isnan(v)
    return ok, np.where(ok, v, 0.0)


def interp_points(z, S, method, x, y):
    """NEAR / BILINEAR / CUBIC of the double plane z (NaN = NA) on S at the points (x, y): arrays of one shape"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    jn, in_ = col_from_x(S, x), row_from_y(S, y)
    inside = (jn >= 0) & (in_ >= 0)
    if method == "near":
        ok, v = _get(z, in_, jn)
        return np.where(inside & ok, v, np.nan)
    j0, tx = axis(x - S.xmin, S.xres, S.ncol)
    i0, ty = axis(S.ymax - y, S.yres, S.nrow)
    wx, wy = [1.0 - tx, tx], [1.0 - ty, ty]
    num, den = np.zeros(x.shape), np.zeros(x.shape)
    for i in range(2):
        for j in range(2):
            w = wy[i] * wx[j]
            ok, v = _get(z, i0 + i, j0 + j)
            use = ok & (w != 0.0)
            num = np.where(use, num + w * v, num)
            den = np.where(use, den + w, den)
    with np.errstate(invalid="ignore", divide="ignore"):
        val = np.where(den > 0.0, num / den, np.nan)
    if method == "cubic":
        cx, cy = cubic_weights(tx), cubic_weights(ty)
        fail = np.zeros(x.shape, dtype=bool)
        rowv = []
        for i in range(4):
            zs = []
            for j in range(4):
                ok, v = _get(z, i0 - 1 + i, j0 - 1 + j)
                fail |= ~ok & (cx[j] != 0.0) & (cy[i] != 0.0)
                zs.append(v)
            rowv.append(((cx[0] * zs[0] + cx[1] * zs[1]) + cx[2] * zs[2]) + cx[3] * zs[3])
        cub = ((cy[0] * rowv[0] + cy[1] * rowv[1]) + cy[2] * rowv[2]) + cy[3] * rowv[3]
        val = np.where(fail, val, cub)
    elif method != "bilinear":
        raise ValueError(method)
    return np.where(inside, val, np.nan)


def edge(d, res, n):
    """ceil(d / res - 0.5) held in [0, n]"""
    q = np.ceil(d / res - 0.5)
    q = np.where(q > 0.0, q, 0.0)
    return np.where(q < n, q, n).astype(np.int64)


def foot_cols(S, T, c):
    """first source column of the footprint of target column c (its end is foot_cols(c + 1))"""
    return edge((T.xmin + np.asarray(c, dtype=np.float64) * T.xres) - S.xmin, S.xres, S.ncol)


def foot_rows(S, T, r):
    return edge(S.ymax - (T.ymax - np.asarray(r, dtype=np.float64) * T.yres), S.yres, S.nrow)


def aggregate(z, S, T, method, rows, cols):
    """the aggregate of the double plane z over the footprints of the target cells rows x cols: a sum of row sums"""
    rows, cols = np.asarray(rows), np.asarray(cols)
    jl, jh = foot_cols(S, T, cols), foot_cols(S, T, cols + 1)
    il, ih = foot_rows(S, T, rows), foot_rows(S, T, rows + 1)
    ns, nt_c, nt_r = S.nrow, cols.size, rows.size
    psum, pcnt = np.zeros((ns, nt_c)), np.zeros((ns, nt_c), dtype=np.int64)
    pmn, pmx = np.zeros((ns, nt_c)), np.zeros((ns, nt_c))
    with np.errstate(invalid="ignore"):
        for k in range(int((jh - jl).max(initial=0))):             # every footprint row west to east from 0
            j = jl + k
            v = z[:, np.clip(j, 0, S.ncol - 1)]
            ok = (j < jh)[None, :] & ~np.isnan(v)
            v = np.where(ok, v, 0.0)
            psum = np.where(ok, psum + v, psum)
            pmn = np.where(ok & ((pcnt == 0) | (v < pmn)), v, pmn)
            pmx = np.where(ok & ((pcnt == 0) | (v > pmx)), v, pmx)
            pcnt = pcnt + ok
        csum, ccnt = np.zeros((nt_r, nt_c)), np.zeros((nt_r, nt_c), dtype=np.int64)
        cmn, cmx = np.zeros((nt_r, nt_c)), np.zeros((nt_r, nt_c))
        for k in range(int((ih - il).max(initial=0))):             # the row sums north to south from 0
            i = il + k
            use = (i < ih)[:, None]
            ii = np.clip(i, 0, ns - 1)
            csum = np.where(use, csum + psum[ii], csum)
            has = use & (pcnt[ii] > 0)
            cmn = np.where(has & ((ccnt == 0) | (pmn[ii] < cmn)), pmn[ii], cmn)
            cmx = np.where(has & ((ccnt == 0) | (pmx[ii] > cmx)), pmx[ii], cmx)
            ccnt = ccnt + np.where(has, pcnt[ii], 0)
        if method == "sum":
            return csum
        if method == "count":
            return ccnt.astype(np.float64)
        none = ccnt == 0
        val = csum / ccnt.astype(np.float64) if method == "mean" else cmn if method == "min" else cmx
    return np.where(none, np.nan, val)


def resample(src, nodata, S, T, method, window=None):
    """the source plane `src` (2-D) on grid S onto the window (r0, r1, c0, c1) of grid T: float64, NaN = NA"""
    z = to_double(src, nodata)
    assert z.shape == (S.nrow, S.ncol)
    r0, r1, c0, c1 = window if window is not None else (0, T.nrow, 0, T.ncol)
    rows, cols = np.arange(r0, r1), np.arange(c0, c1)
    if method in ("near", "bilinear", "cubic"):
        y, x = np.meshgrid(cell_y(T, rows), cell_x(T, cols), indexing="ij")
        return interp_points(z, S, method, x, y)
    return aggregate(z, S, T, method, rows, cols)


def extract(src, nodata, S, xy, method):
    """the interpolating methods at the points xy (n x 2); "simple" is "near" """
    xy = np.asarray(xy, dtype=np.float64)
    return interp_points(to_double(src, nodata), S, "near" if method == "simple" else method, xy[:, 0], xy[:, 1])
