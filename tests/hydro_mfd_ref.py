"""The multiple-flow-direction rules of include/machisplin_hip.h (section "hydrology, multiple flow direction", rules 6 - 8)
restated by ANOTHER algorithm than the library's tile sweeps: the shares vectorised in numpy over the whole plane, the
accumulation by ONE walk through the cells in topological order ((W, D) descending), every cell pulling from its donors in k
order.  W and D come from tests/hydro_ref.py (priority flood, breadth-first search).  Every arithmetic operation stands in
the header's order and is rounded once; with the exponent 1 nothing but subtraction, division, multiplication and sums occur,
so the device planes must equal these bit for bit.  For another exponent the shares go through pow (numpy's here).

Also the two planes the MFD tests add to hydro_ref.PLANES: a ramp on which every cell has one receiver (MFD = D8), and a cone
from whose apex the water diverges (where the two differ most)."""
import numpy as np

import hydro_ref as hr
import terrain_ref as tr

EXPONENTS = (1.0, 1.1, 8.0)
EXTRA = [("ramp", (1, 70)), ("cone", (97, 130))]
PLANES = list(hr.PLANES) + EXTRA
EPS = float(np.finfo(np.float64).eps)
# the accumulation over the cells without receivers against n_valid, relative: at most three roundings per step (product, add,
# and the share's own), the longest path on these planes is the spiral's 9 216 cells: 3 * 9216 * 1.1e-16 = 3e-12
SINK_SUM_RTOL = 1e-11


def plane(kind, shape):
    """the test planes by name: those of hydro_ref, the ramp and the cone"""
    if kind == "spiral":
        return hr.spiral(shape[0])
    if kind in ("ramp", "cone"):
        nr, nc = shape
        r, c = np.meshgrid(np.arange(nr, dtype=np.float64), np.arange(nc, dtype=np.float64), indexing="ij")
        if kind == "ramp":                                   # z = column: one receiver, the west neighbour
            return c.copy()
        return -np.floor(0.5 * np.hypot(r - 48.0, c - 65.0))  # a cone with its apex up: the water diverges
    return hr.plane(kind, shape)


def shares(W, D, dx, dy, x, dx_row=None):
    """rule 6 over the whole plane: f (8, nr, nc), f[k] = the share a cell sends to its neighbour k (0 where none, and at NA
    cells), and `has` = the cells with receivers"""
    dxr = tr._dx(W, dx, dx_row)
    g = np.sqrt(dxr * dxr + np.float64(dy) * np.float64(dy))
    dist = (dxr, g, np.float64(dy), g, dxr, g, np.float64(dy), g)
    wp, dp = hr._pad(W, np.nan), hr._pad(D, 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.stack([(W - hr._shift(wp, k)) / dist[k] for k in range(8)])
        pos = s > 0.0                                                  # false for a NaN: no neighbour
        s_max = np.where(pos, s, 0.0).max(axis=0)
        steep = s_max > 0.0
        p = np.where(pos & steep, s / np.where(steep, s_max, 1.0), 0.0)
        if x != 1.0:
            p = np.power(p, np.float64(x))
        S = p[0].copy()
        for k in range(1, 8):
            S = S + p[k]
        f = np.where(steep, p / np.where(steep, S, 1.0), 0.0)
        along = np.stack([~steep & (D > 0) & (hr._shift(wp, k) == W) & (hr._shift(dp, k) == D - 1) for k in range(8)])
        m = along.sum(axis=0)
        f = np.where(along, 1.0 / np.where(m > 0, m, 1).astype(np.float64), f)
    return f, steep | (m > 0)


def incoming(f):
    """fin (8, nr, nc): fin[k] = the share neighbour k sends to the cell = that cell's f[(k + 4) & 7]"""
    return np.stack([hr._shift(hr._pad(f[(k + 4) & 7], 0.0), k) for k in range(8)])


def accumulation(W, D, fin):
    """rule 7 by one walk in topological order: sorted by (W, D) descending every cell comes after all its donors, and pulls
    from them in k order -- product, then add, Python floats (doubles, each operation rounded once)"""
    nr, nc = W.shape
    pc = nc + 2
    A = [float("nan")] * ((nr + 2) * pc)
    offs = [hr.K_DR[k] * pc + hr.K_DC[k] for k in range(8)]
    flat = [hr._pad(fin[k], 0.0).ravel().tolist() for k in range(8)]
    rows, cols = np.nonzero(~np.isnan(W))
    order = np.lexsort((-D[rows, cols].astype(np.int64), -W[rows, cols]))
    for i in ((rows[order] + 1) * pc + cols[order] + 1).tolist():
        a = 1.0
        for k in range(8):
            fk = flat[k][i]
            if fk > 0.0:
                a = a + fk * A[i + offs[k]]
        A[i] = a
    return np.array(A).reshape(nr + 2, pc)[1:-1, 1:-1].copy()


def jacobi(W, fin, max_sweeps=20000):
    """rule 7 the way a tile solve does it: sweeps over the whole plane from A = 1, every cell from the values of the sweep
    before, until one changes nothing.  Returns A and the number of sweeps; asserts that no sweep lowers a value."""
    A = np.where(np.isnan(W), np.nan, 1.0)
    for sweep in range(max_sweeps):
        ap = hr._pad(A, np.nan)
        new = np.where(np.isnan(W), np.nan, 1.0)
        for k in range(8):
            new = np.where(fin[k] > 0.0, new + fin[k] * hr._shift(ap, k), new)
        with np.errstate(invalid="ignore"):
            assert not (new < A).any()
        if np.array_equal(new, A, equal_nan=True):
            return A, sweep + 1
        A = new
    raise AssertionError("no fixed point")


def hydro_mfd(z_plane, nodata, dx, dy, x, z_factor=1.0, dx_row=None, min_slope_tan=np.tan(np.deg2rad(0.1)), base=None):
    """dict: filled, dist, shares (f), incoming (fin), receivers, flowacc (float64, NaN at NA cells), twi_arg, twi and the
    counts; `base` = hydro_ref.hydro of the same plane and units, where the caller has it already"""
    z = tr.to_double(z_plane, nodata)
    h = base if base is not None else hr.hydro(z_plane, nodata, dx, dy, z_factor, dx_row, min_slope_tan)
    W, D = h["filled"], h["dist"]
    f, has = shares(W, D, dx, dy, x, dx_row)
    fin = incoming(f)
    acc = accumulation(W, D, fin)
    t = tr.terrain(W, np.nan, dx, dy, z_factor, dx_row)["slope_tan"]
    dxr = tr._dx(z, dx, dx_row)
    with np.errstate(invalid="ignore"):
        arg = (acc * np.sqrt(dxr * np.float64(dy))) / np.where(t > min_slope_tan, t, np.where(np.isnan(t), np.nan, min_slope_tan))
        twi = np.log(arg)
    valid = ~np.isnan(z)
    return {"filled": W, "dist": D, "shares": f, "incoming": fin, "receivers": has, "flowacc": acc, "twi_arg": arg, "twi": twi,
            "n_valid": h["n_valid"], "n_raised": h["n_raised"], "n_sinks": int((valid & ~has).sum())}


def check_invariants(z, m, d8):
    """every positive share goes to a strictly smaller (W, D); the shares of a cell with receivers sum to 1 within 4 ulp; the
    cells without receivers are D8's -1 cells; A >= 1; the accumulation over them is the number of valid cells"""
    W, D, f, A = m["filled"], m["dist"], m["shares"], m["flowacc"]
    valid = ~np.isnan(z)
    wp, dp = hr._pad(W, np.nan), hr._pad(D, 0)
    assert (f >= 0.0).all() and not f[:, ~valid].any()
    for k in range(8):
        to = f[k] > 0.0
        wk, dk = hr._shift(wp, k), hr._shift(dp, k)
        assert not np.isnan(wk[to]).any()                                       # a receiver is a valid cell of the raster
        assert ((wk[to] < W[to]) | ((wk[to] == W[to]) & (dk[to] < D[to]))).all(), k
    total = f[0].copy()
    for k in range(1, 8):
        total = total + f[k]
    has = m["receivers"]
    assert np.array_equal(has, (f > 0.0).any(axis=0)) and (np.abs(total[has] - 1.0) <= 4 * EPS).all()
    assert np.array_equal(valid & ~has, d8 == hr.DIR_OUT) and m["n_sinks"] == int((d8 == hr.DIR_OUT).sum())
    assert np.array_equal(np.isnan(A), ~valid) and (A[valid] >= 1.0).all()
    n_valid = int(valid.sum())
    if n_valid:
        out_sum = float(A[valid & ~has].sum())
        assert abs(out_sum - n_valid) <= SINK_SUM_RTOL * n_valid, (out_sum, n_valid)
