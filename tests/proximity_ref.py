"""numpy restatements of the proximity rule (include/machisplin_hip.h, section "proximity"), independent of the library.

Two of them: :func:`brute` goes over all features for every cell (tiny grids), :func:`two_stage` does a row scan with
``np.maximum.accumulate`` / ``np.minimum.accumulate`` and then, per column, the full minimum over the rows -- ``argmin``'s first
occurrence is the smaller row.  O(nrow^2 ncol): fine up to a few hundred rows (a plane of one column or one row costs
nothing).  Both return (d2, index) as int64 arrays; :func:`products` makes every plane of the rule from them.
"""
import numpy as np

WHERE = ("na", "valid", "lt", "le", "gt", "ge", "eq", "ne")
BIG = np.int64(1) << 40


def features(z, nodata, where, threshold=None):
    """the boolean feature mask of the plane z"""
    v = np.asarray(z).astype(np.float64)
    na = np.isnan(v)
    if nodata is not None and not np.isnan(nodata):
        na |= v == nodata
    if where == "na":
        return na
    if where == "valid":
        return ~na
    t = np.float64(threshold)
    with np.errstate(invalid="ignore"):
        cmp = {"lt": v < t, "le": v <= t, "gt": v > t, "ge": v >= t, "eq": v == t, "ne": v != t}[where]
    return cmp & ~na


def brute(mask):
    """(d2, index) by going over every feature, in the order of their cell numbers: a strictly smaller d2 replaces"""
    mask = np.asarray(mask, dtype=bool)
    nrow, ncol = mask.shape
    d2 = np.full((nrow, ncol), -1, dtype=np.int64)
    idx = np.full((nrow, ncol), -1, dtype=np.int64)
    r, c = np.meshgrid(np.arange(nrow, dtype=np.int64), np.arange(ncol, dtype=np.int64), indexing="ij")
    for fr, fc in zip(*np.nonzero(mask)):                   # row-major: ascending cell number
        d = (r - fr) ** 2 + (c - fc) ** 2
        better = (d2 < 0) | (d < d2)
        d2[better] = d[better]
        idx[better] = fr * ncol + fc
    return d2, idx


def row_nearest(mask):
    """the column of the nearest feature in each cell's own row, the left one on a tie, -1 where the row has none"""
    mask = np.asarray(mask, dtype=bool)
    nrow, ncol = mask.shape
    cols = np.broadcast_to(np.arange(ncol, dtype=np.int64), (nrow, ncol))
    left = np.maximum.accumulate(np.where(mask, cols, -1), axis=1)
    right = np.minimum.accumulate(np.where(mask, cols, BIG)[:, ::-1], axis=1)[:, ::-1]
    take_left = (left >= 0) & ((right >= BIG) | (cols - left <= right - cols))
    near = np.where(take_left, left, np.where(right < BIG, right, -1))
    return near


def two_stage(mask):
    """(d2, index): the row scan, then per column the full minimum over the rows"""
    mask = np.asarray(mask, dtype=bool)
    nrow, ncol = mask.shape
    near = row_nearest(mask)
    cols = np.arange(ncol, dtype=np.int64)[None, :]
    h = np.where(near >= 0, (cols - near) ** 2, BIG)                         # (nrow, ncol), by the feature's row
    d2 = np.empty((nrow, ncol), dtype=np.int64)
    fr = np.empty((nrow, ncol), dtype=np.int64)
    rows = np.arange(nrow, dtype=np.int64)
    for r in range(nrow):
        cost = (rows - r)[:, None] ** 2 + h                                   # cost[r', c]
        k = np.argmin(cost, axis=0)                                           # the first minimum: the smaller row
        fr[r] = k
        d2[r] = cost[k, np.arange(ncol)]
    none = d2 >= BIG
    fc = near[fr, np.broadcast_to(np.arange(ncol), (nrow, ncol))]
    idx = np.where(none, -1, fr * ncol + fc)
    return np.where(none, -1, d2), idx


def products(d2, idx, ncol, unit=1.0, value_plane=None, nodata=None, f32=False):
    """the six planes of the rule from (d2, index): a dict.  f32: the float planes converted once to float32"""
    d2 = np.asarray(d2, dtype=np.int64)
    idx = np.asarray(idx, dtype=np.int64)
    nrow = d2.shape[0]
    none = idx < 0
    r, c = np.meshgrid(np.arange(nrow, dtype=np.int64), np.arange(ncol, dtype=np.int64), indexing="ij")
    fr, fc = np.where(none, 0, idx // ncol), np.where(none, 0, idx % ncol)
    s = np.sqrt(np.where(none, 0, d2).astype(np.float64))
    dist = s * np.float64(unit)
    with np.errstate(invalid="ignore", divide="ignore"):
        dx = np.where(d2 == 0, 0.0, (fc - c).astype(np.float64) / s)
        dy = np.where(d2 == 0, 0.0, (r - fr).astype(np.float64) / s)
    out = {"d2": d2.astype(np.int32), "index": idx.astype(np.int32)}
    flo = {"dist": dist, "dir_x": dx, "dir_y": dy}
    if value_plane is not None:
        v = np.asarray(value_plane).astype(np.float64)
        na = np.isnan(v)
        if nodata is not None and not np.isnan(nodata):
            na |= v == nodata
        v = np.where(na, np.nan, v)
        flo["value"] = v[fr, fc]
    for k, a in flo.items():
        a = np.where(none, np.nan, a)
        out[k] = a.astype(np.float32) if f32 else a
    return out


def proximity(z, nodata=None, where="na", threshold=None, unit=1.0, value_plane=None, f32=False, search=two_stage):
    """every plane of the rule for the plane z"""
    mask = features(z, nodata, where, threshold)
    d2, idx = search(mask)
    return products(d2, idx, mask.shape[1], unit, value_plane, nodata, f32)
