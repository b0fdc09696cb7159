"""The zonal rule of include/machisplin_hip.h, section "zonal", restated: S1 and S2 are Python ints, everything else numpy, and
every statistic repeats the header's operations in the header's order, so the device's tables and planes must equal these bit
for bit.  ``loop`` is a second, plain restatement (a Python loop over the cells, no two-word S2) that the CPU tests hold against
this one."""
import math

import numpy as np

STATS = ("count", "sum", "mean", "sd", "min", "max", "range", "minus_mean", "above_min", "below_max", "dev", "cells")
TABLE_STATS = STATS[:7] + ("cells",)
INFO = ("n_zones", "n_present", "n_cells_in_zones", "n_contributing", "n_nonfinite", "n_inexact", "quantum")
NAN = float("nan")


def na_mask(values, nodata=None):
    v = np.asarray(values).astype(np.float64)
    na = np.isnan(v)
    if nodata is not None and not np.isnan(nodata):
        na |= v == nodata
    return v, na


def default_quantum(values, nodata=None):
    """the smallest power of two (not below 2^-1022) with max|v| <= 2^30 * quantum over the valid finite cells; 1 for int16"""
    if np.asarray(values).dtype == np.int16:
        return 1.0
    v, na = na_mask(values, nodata)
    ok = ~na & np.isfinite(v)
    m = float(np.abs(v[ok]).max()) if ok.any() else 0.0
    if m == 0.0:
        return 1.0
    f, e = math.frexp(m)
    return math.ldexp(1.0, max((e - 1 if f == 0.5 else e) - 30, -1022))


def _D(x):
    return float(x >> 64) * 2.0 ** 64 + float(x & (2 ** 64 - 1))


def finalise(n, S1, S2, qmin, qmax, quantum):
    """the six float statistics of one zone, by the header's lines"""
    if n == 0:
        return (NAN,) * 6
    total = float(S1) * quantum
    mean = (float(S1) / float(n)) * quantum
    sd = math.sqrt(_D(n * S2 - S1 * S1) / (float(n) * float(n - 1))) * quantum if n >= 2 else NAN
    mn, mx = float(qmin) * quantum, float(qmax) * quantum
    return total, mean, sd, mn, mx, mx - mn


def zonal(values, zones, nodata=None, n_zones=None, quantum=None, f32=False):
    """(table, planes, info): the DENSE table of every statistic of TABLE_STATS, every plane of STATS, the info's fields"""
    v, na = na_mask(values, nodata)
    zones = np.asarray(zones).astype(np.int64)
    assert v.shape == zones.shape and v.ndim == 2
    if n_zones is None:
        n_zones = int(zones.max()) + 1 if zones.size and zones.max() >= 0 else 0
    assert zones.max() < n_zones or n_zones == 0
    if quantum is None:
        quantum = default_quantum(values, nodata)
    finite = np.isfinite(v)
    assert (np.abs(v[~na & finite]) <= 2.0 ** 30 * quantum).all()
    inz = zones >= 0
    con = inz & ~na & finite
    q = np.zeros(v.shape, dtype=np.int64)
    q[con] = np.rint(v[con] / quantum).astype(np.int64)
    zc, qc = zones[con], q[con]
    cells = np.bincount(zones[inz], minlength=n_zones).astype(np.int64)
    n = np.bincount(zc, minlength=n_zones).astype(np.int64)
    S1 = np.zeros(n_zones, dtype=np.int64)
    np.add.at(S1, zc, qc)
    sq = qc * qc                                                       # <= 2^60
    L = np.zeros(n_zones, dtype=np.int64)
    H = np.zeros(n_zones, dtype=np.int64)
    np.add.at(L, zc, sq & 0xffffffff)                                  # <= 2^31 * 2^32
    np.add.at(H, zc, sq >> 32)
    qmin = np.full(n_zones, 2 ** 31 - 1, dtype=np.int64)
    qmax = np.full(n_zones, -2 ** 31, dtype=np.int64)
    np.minimum.at(qmin, zc, qc)
    np.maximum.at(qmax, zc, qc)
    fl = np.full((6, n_zones), NAN)
    for z in np.flatnonzero(n):
        fl[:, z] = finalise(int(n[z]), int(S1[z]), (int(H[z]) << 32) + int(L[z]), int(qmin[z]), int(qmax[z]), quantum)
    table = {"count": n, "cells": cells}
    for k, name in enumerate(STATS[1:7]):
        table[name] = fl[k]
    table = {k: table[k] for k in TABLE_STATS}
    zi = np.where(inz, zones, 0)
    planes = {}
    for name in TABLE_STATS:
        if name in ("count", "cells"):
            planes[name] = np.where(inz, table[name][zi] if n_zones else 0, 0).astype(np.int32)
        else:
            planes[name] = np.where(inz, table[name][zi] if n_zones else NAN, NAN)
    if n_zones:
        e = q.astype(np.float64) * quantum
        mean, sd, mn, mx = (table[k][zi] for k in ("mean", "sd", "min", "max"))
        with np.errstate(invalid="ignore", divide="ignore"):
            mm = e - mean
            planes["minus_mean"] = np.where(con, mm, NAN)
            planes["above_min"] = np.where(con, e - mn, NAN)
            planes["below_max"] = np.where(con, mx - e, NAN)
            planes["dev"] = np.where(con & ~np.isnan(sd) & (sd != 0.0), mm / np.where(sd == 0.0, 1.0, sd), NAN)
    else:
        for name in STATS[7:11]:
            planes[name] = np.full(v.shape, NAN)
    planes = {k: planes[k] for k in STATS}
    if f32:
        planes = {k: p if p.dtype == np.int32 else p.astype(np.float32) for k, p in planes.items()}
    info = {"n_zones": n_zones, "n_present": int((cells > 0).sum()), "n_cells_in_zones": int(inz.sum()), "n_contributing": int(con.sum()),
            "n_nonfinite": int((inz & ~na & ~finite).sum()), "n_inexact": int((q[con].astype(np.float64) * quantum != v[con]).sum()),
            "quantum": quantum}
    return table, planes, info


def present(table):
    """the present form of a dense table: the rows with cells > 0 and their zone numbers"""
    keep = np.flatnonzero(table["cells"] > 0)
    return {"zone": keep.astype(np.int32), **{k: a[keep] for k, a in table.items()}}


def loop(values, zones, nodata=None, n_zones=None, quantum=None):
    """the dense table by a plain loop over the cells: Python ints, one S2, no numpy reduction"""
    v, na = na_mask(values, nodata)
    zones = np.asarray(zones)
    if n_zones is None:
        n_zones = max(int(zones.max()) + 1, 0)
    if quantum is None:
        quantum = default_quantum(values, nodata)
    acc = [[0, 0, 0, 0, None, None] for _ in range(n_zones)]           # cells, n, S1, S2, qmin, qmax
    for z, x, bad in zip(zones.ravel().tolist(), v.ravel().tolist(), na.ravel().tolist()):
        if z < 0:
            continue
        a = acc[z]
        a[0] += 1
        if bad or math.isinf(x):
            continue
        q = int(np.rint(x / quantum))
        a[1] += 1
        a[2] += q
        a[3] += q * q
        a[4] = q if a[4] is None else min(a[4], q)
        a[5] = q if a[5] is None else max(a[5], q)
    table = {k: np.full(n_zones, NAN) for k in TABLE_STATS}
    table["count"] = np.array([a[1] for a in acc], dtype=np.int64).reshape(n_zones)
    table["cells"] = np.array([a[0] for a in acc], dtype=np.int64).reshape(n_zones)
    for z, a in enumerate(acc):
        if a[1]:
            for name, x in zip(STATS[1:7], finalise(a[1], a[2], a[3], a[4], a[5], quantum)):
                table[name][z] = x
    return table
