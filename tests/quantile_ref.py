"""The quantile rule of include/machisplin_hip.h, section "zonal quantiles", restated: ``np.sort`` per zone and the rule's operations
in ``np.float64`` one by one, ``below`` by ``np.searchsorted``, the aggregate's zones from ``resample_ref``'s footprints.  The
input, NA, membership and the quantisation are ``zonal_ref``'s.  The device's tables and planes must equal these bit for bit.
``loop`` is a second, plain restatement (Python lists and floats) that the CPU tests hold against this one."""
import math

import numpy as np

import resample_ref as rr
import zonal_ref as zr

NAN = float("nan")
INFO = ("n_zones", "n_present", "n_cells_in_zones", "n_contributing", "n_nonfinite", "n_inexact", "quantum")
U = 2.0 ** -53


def bound(s, quantum):
    """the header's bound on |Q - exact type 7| for the ascending s"""
    d = float(int(s[-1]) - int(s[0]))
    m = max(abs(float(s[0])), abs(float(s[-1])))
    return U * (s.size * d + d + m) * quantum


def quantise(values, zones, nodata=None, n_zones=None, quantum=None):
    """(q int64, contributing mask, zones int64, n_zones, quantum, info without n_present)"""
    v, na = zr.na_mask(values, nodata)
    zones = np.asarray(zones).astype(np.int64)
    assert v.shape == zones.shape and v.ndim == 2
    if n_zones is None:
        n_zones = int(zones.max()) + 1 if zones.size and zones.max() >= 0 else 0
    assert zones.max() < n_zones or n_zones == 0
    if quantum is None:
        quantum = zr.default_quantum(values, nodata)
    finite = np.isfinite(v)
    assert (np.abs(v[~na & finite]) <= 2.0 ** 30 * quantum).all()
    inz = zones >= 0
    con = inz & ~na & finite
    q = np.zeros(v.shape, dtype=np.int64)
    q[con] = np.rint(v[con] / quantum).astype(np.int64)
    info = {"n_zones": n_zones, "n_cells_in_zones": int(inz.sum()), "n_contributing": int(con.sum()), "n_nonfinite": int((inz & ~na & ~finite).sum()),
            "n_inexact": int((q[con].astype(np.float64) * quantum != v[con]).sum()), "quantum": quantum}
    return q, con, zones, n_zones, quantum, info


def quantile(values, zones=None, probs=(0.5,), nodata=None, n_zones=None, quantum=None, f32=False):
    """(table, planes, info): the DENSE table {"q": [n_zones, n_probs], "count"}, the planes q [n_probs, nrow, ncol], below,
    frac_below, and the info's fields.  zones None: the whole layer is zone 0."""
    values = np.asarray(values)
    if zones is None:
        zones, n_zones = np.zeros(values.shape, dtype=np.int32), 1
    q, con, zones, n_zones, quantum, info = quantise(values, zones, nodata, n_zones, quantum)
    probs = [float(p) for p in probs]
    tq = np.full((n_zones, len(probs)), NAN)
    count = np.zeros(n_zones, dtype=np.int64)
    below = np.full(values.shape, -1, dtype=np.int32)
    frac = np.full(values.shape, NAN)
    zc, qc = zones[con], q[con]
    order = np.lexsort((qc, zc))
    zs, qs = zc[order], qc[order]
    starts = np.searchsorted(zs, np.arange(n_zones + 1))
    where = np.argwhere(con)
    count[:] = np.diff(starts)
    have = np.flatnonzero(count)
    for j, p in enumerate(probs):                                          # the rule's operations one by one, on all present zones at once
        h = (count[have] - 1).astype(np.float64) * np.float64(p)
        lo = np.floor(h).astype(np.int64)
        g = h - lo.astype(np.float64)
        hi = np.minimum(lo + 1, count[have] - 1)
        a, b = qs[starts[have] + lo], qs[starts[have] + hi]
        tq[have, j] = (a.astype(np.float64) + g * (b - a).astype(np.float64)) * np.float64(quantum)
    if zc.size:
        # the cells of a zone with a smaller q: the first place of (zone, q) among the sorted pairs, less the zone's first place
        b = np.searchsorted(zs * 2 ** 32 + (qs + 2 ** 30), zc * 2 ** 32 + (qc + 2 ** 30), side="left") - starts[zc]
        below[where[:, 0], where[:, 1]] = b
        frac[where[:, 0], where[:, 1]] = b.astype(np.float64) / count[zc].astype(np.float64)
    inz = (zones >= 0) & (n_zones > 0)
    zi = np.where(inz, zones, 0)
    qp = np.full((len(probs),) + values.shape, NAN)
    if n_zones:
        for j in range(len(probs)):
            qp[j] = np.where(inz, tq[zi, j], NAN)
    planes = {"q": qp, "below": below, "frac_below": frac}
    if f32:
        planes = {k: p if p.dtype == np.int32 else p.astype(np.float32) for k, p in planes.items()}
    info = dict(info, n_present=int((count > 0).sum()))
    return {"q": tq, "count": count}, planes, info


def present(table):
    """the present form of a dense table: the rows with n > 0 and their zone numbers"""
    keep = np.flatnonzero(table["count"] > 0)
    return {"zone": keep.astype(np.int32), "q": table["q"][keep], "count": table["count"][keep]}


def target_zones(S, T):
    """the zone plane of "aggregate": target row * T.ncol + target column of the footprint that holds the source cell, -1 for none"""
    row = np.full(S.nrow, -1, dtype=np.int64)
    col = np.full(S.ncol, -1, dtype=np.int64)
    r_edge = rr.foot_rows(S, T, np.arange(T.nrow + 1))
    c_edge = rr.foot_cols(S, T, np.arange(T.ncol + 1))
    for r in range(T.nrow):
        row[r_edge[r]:r_edge[r + 1]] = r
    for c in range(T.ncol):
        col[c_edge[c]:c_edge[c + 1]] = c
    z = row[:, None] * T.ncol + col[None, :]
    return np.where((row[:, None] < 0) | (col[None, :] < 0), -1, z).astype(np.int32)


def aggregate_quantile(values, S, T, probs=(0.5,), nodata=None, quantum=None):
    """(planes [n_probs, T.nrow, T.ncol], count [T.nrow, T.ncol] int64, info)"""
    table, _, info = quantile(values, target_zones(S, T), probs, nodata, n_zones=T.nrow * T.ncol, quantum=quantum)
    return table["q"].T.reshape(len(probs), T.nrow, T.ncol).copy(), table["count"].reshape(T.nrow, T.ncol), info


def loop(values, zones, probs, nodata=None, n_zones=None, quantum=None):
    """the dense table by a plain loop over the cells: Python lists, sorted(), floats"""
    v, na = zr.na_mask(values, nodata)
    zones = np.asarray(zones)
    if n_zones is None:
        n_zones = max(int(zones.max()) + 1, 0)
    if quantum is None:
        quantum = zr.default_quantum(values, nodata)
    cells = [[] for _ in range(n_zones)]
    for z, x, bad in zip(zones.ravel().tolist(), v.ravel().tolist(), na.ravel().tolist()):
        if z < 0 or bad or math.isinf(x):
            continue
        cells[z].append(int(np.rint(x / quantum)))
    tq = np.full((n_zones, len(probs)), NAN)
    for z, c in enumerate(cells):
        s = sorted(c)
        n = len(s)
        for j, p in enumerate(probs):
            if n:
                h = float(n - 1) * float(p)
                lo = int(math.floor(h))
                g = h - float(lo)
                hi = min(lo + 1, n - 1)
                tq[z, j] = (float(s[lo]) + g * float(s[hi] - s[lo])) * quantum
    return {"q": tq, "count": np.array([len(c) for c in cells], dtype=np.int64).reshape(n_zones)}
