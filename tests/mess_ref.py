"""The MESS rule of include/machisplin_hip.h restated in numpy: np.sort, searchsorted(side="right") and the rule's
operations in its order, each one rounded once (numpy never contracts a multiply and an add), plus MoD by argmin over the
variables in order.  What the device planes must equal bit for bit."""
import numpy as np


def similarity(ref_col, p):
    """s of the values p (any shape, float64, NaN = NA) against ONE variable's reference values."""
    r = np.sort(np.asarray(ref_col, dtype=np.float64))
    p = np.asarray(p, dtype=np.float64)
    n = r.size
    mn, mx = r[0], r[-1]
    with np.errstate(invalid="ignore"):
        i = np.searchsorted(r, p, side="right")          # NaN sorts last: i == n, overwritten below
        f = (100.0 * i.astype(np.float64)) / np.float64(n)
        s = np.where(f <= 50.0, 2.0 * f, 200.0 - 2.0 * f)
        s = np.where(i == 0, (100.0 * (p - mn)) / (mx - mn), s)
        s = np.where(i == n, (100.0 * (mx - p)) / (mx - mn), s)
    return np.where(np.isnan(p), np.nan, s)


def mess(ref, values):
    """ref: n_ref x V; values: V arrays of one shape (NaN = NA).  Returns (MESS float64, MoD int32) of that shape."""
    ref = np.asarray(ref, dtype=np.float64)
    s = np.stack([similarity(ref[:, v], values[v]) for v in range(ref.shape[1])])
    na = np.isnan(s).any(axis=0)
    filled = np.where(np.isnan(s), np.inf, s)
    mod = np.argmin(filled, axis=0).astype(np.int32)      # the lowest variable that attains the minimum
    out = np.min(filled, axis=0)
    return np.where(na, np.nan, out), np.where(na, np.int32(-1), mod).astype(np.int32)


def grid_values(geom, planes, nodata, n_vars, window=None):
    """The V variables of every cell of the window as float64 planes: the stack's layers (nodata -> NaN), then -- when
    n_vars is two more -- LONG and LAT of the cell centres on absolute grid indices."""
    r0, r1, c0, c1 = window if window is not None else (0, geom.nrow, 0, geom.ncol)
    planes = np.asarray(planes)
    vals = []
    for k in range(planes.shape[0]):
        v = planes[k, r0:r1, c0:c1].astype(np.float64)
        if not np.isnan(nodata):
            v = np.where(v == nodata, np.nan, v)
        vals.append(v)
    if n_vars == planes.shape[0] + 2:
        x = geom.xmin + (np.arange(c0, c1, dtype=np.float64) + 0.5) * geom.xres
        y = geom.ymax - (np.arange(r0, r1, dtype=np.float64) + 0.5) * geom.yres
        vals.append(np.broadcast_to(x[None, :], (r1 - r0, c1 - c0)))
        vals.append(np.broadcast_to(y[:, None], (r1 - r0, c1 - c0)))
    assert len(vals) == n_vars
    return vals
