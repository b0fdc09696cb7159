"""numpy restatement of include/machisplin_hip.h, section "classes": the class of a cell by np.searchsorted in the ascending
list, the exact integer counts of every unit by np.bincount of unit * (K + 3) + slot, and the derived values by the header's
handful of operations -- what the GPU tests compare the library with, bit for bit.  The units: the zones of an int32 plane
(crosstab), the footprints of resample_ref (aggregate), the windows of focal_ref (focal).  And the plain loops with
collections.Counter that the restatement is held against."""
from collections import Counter

import numpy as np

import focal_ref as fr
import resample_ref as rr

MAX_K = 256
MAX_CODE = 65535
NAN = float("nan")


def valid(values, nodata=NAN):
    """(the plane as double, the cells that are not NA)"""
    z = np.asarray(values, dtype=np.float64)
    ok = ~np.isnan(z)
    if nodata == nodata:
        ok &= z != nodata
    return z, ok


def codes_of(values, nodata=NAN):
    """the code of every cell: the integer value in 0 .. 65 535, -1 where the cell is valid without one, -2 where it is NA"""
    z, ok = valid(values, nodata)
    with np.errstate(invalid="ignore"):
        has = ok & (z >= 0.0) & (z <= MAX_CODE) & (np.floor(z) == z)
    code = np.full(z.shape, -1, dtype=np.int64)
    code[has] = z[has].astype(np.int64)
    code[~ok] = -2
    return code


def measure(values, nodata=NAN):
    """classes=None: the codes present, ascending, and the info's counts"""
    code = codes_of(values, nodata)
    present = np.unique(code[code >= 0])
    if present.size > MAX_K:
        raise ValueError(f"{present.size} distinct codes")
    return [int(c) for c in present]


def slots(values, classes, nodata=NAN):
    """(the sorted class list, the slot of every cell: k, K for `other`, K + 1 for NA)"""
    classes = np.array(sorted(int(c) for c in classes), dtype=np.int64)
    assert 1 <= classes.size <= MAX_K and np.all(np.diff(classes) > 0) and classes[0] >= 0 and classes[-1] <= MAX_CODE
    K = classes.size
    code = codes_of(values, nodata)
    k = np.searchsorted(classes, code)
    hit = (code >= 0) & (k < K) & (classes[np.minimum(k, K - 1)] == code)
    slot = np.where(hit, k, K)
    slot[code == -2] = K + 1
    return classes, slot


def info(values, classes, nodata=NAN):
    classes, slot = slots(values, classes, nodata)
    K = classes.size
    return {"K": K, "codes": [int(c) for c in classes], "n_valid": int((slot <= K).sum()), "n_na": int((slot == K + 1).sum()),
            "n_other": int((slot == K).sum())}


def finish(counts, other, classes, frac_of=()):
    """the derived values of units whose class counts are the rows of `counts` (U x K) and `other` (U): a dict of arrays"""
    counts = np.asarray(counts, dtype=np.int64)
    other = np.asarray(other, dtype=np.int64)
    classes = np.asarray(classes, dtype=np.int64)
    K = classes.size
    n = counts.sum(axis=1) + other
    assert n.max(initial=0) <= 2 ** 31 - 1
    best = counts.argmax(axis=1)                                           # the first largest: the smaller code on a tie
    best_count = counts[np.arange(counts.shape[0]), best]
    none = best_count == 0
    nd = n.astype(np.float64)
    # the numerator is below 2^62: exact in uint64 (and in Python ints, which is what checks it)
    num = n.astype(np.uint64) * n.astype(np.uint64) - (counts.astype(np.uint64) ** 2).sum(axis=1).astype(np.uint64) - other.astype(np.uint64) ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        out = {"n": n.astype(np.int32), "other": other.astype(np.int32), "counts": counts.astype(np.int32),
               "mode": np.where(none, -1, classes[best]).astype(np.int32), "variety": (counts > 0).sum(axis=1).astype(np.int32),
               "mode_frac": np.where(none, np.nan, best_count.astype(np.float64) / nd),
               "simpson": np.where(n == 0, np.nan, num.astype(np.float64) / (nd * nd))}
        sel = [int(np.searchsorted(classes, c)) for c in frac_of] if len(frac_of) else list(range(K))
        for c, k in zip(frac_of, sel):
            assert classes[k] == c, f"frac_of code {c} is not in the list"
        out["frac"] = np.where((n == 0)[:, None], np.nan, counts[:, sel].astype(np.float64) / nd[:, None])
    return out


def unit_counts(unit, slot, n_units, K):
    """np.bincount of unit * (K + 3) + slot over the cells with unit >= 0: (counts U x K, other U, na U)"""
    W = K + 3
    use = unit >= 0
    t = np.bincount(unit[use].astype(np.int64) * W + slot[use], minlength=n_units * W).reshape(n_units, W)
    return t[:, :K], t[:, K], t[:, K + 1]


def crosstab(values, zones, classes=None, nodata=NAN, n_zones=None, frac_of=(), with_planes=True):
    """(table, planes, info): dicts of every table statistic and of every plane (frac as (F, nrow, ncol)), float64 / int32;
    with_planes False leaves the planes out (a large grid with many classes)"""
    zones = np.asarray(zones)
    if classes is None:
        classes = measure(values, nodata)
    classes, slot = slots(values, classes, nodata)
    K = classes.size
    if n_zones is None:
        n_zones = int(max(zones.max(initial=-1), -1)) + 1
    assert zones.max(initial=-1) < n_zones and n_zones * (K + 3) <= 2 ** 31 - 1
    counts, other, na = unit_counts(zones.ravel(), slot.ravel(), n_zones, K)
    table = finish(counts, other, classes, frac_of)
    table["cells"] = (table["n"].astype(np.int64) + na).astype(np.int32)
    inz = zones >= 0
    zi = np.where(inz, zones, 0)
    planes = {}
    for name in ("mode", "variety", "n") if with_planes else ():
        planes[name] = np.where(inz, table[name][zi] if n_zones else 0, -1).astype(np.int32)
    for name in ("mode_frac", "simpson") if with_planes else ():
        planes[name] = np.where(inz, table[name][zi] if n_zones else 0.0, np.nan)
    F = table["frac"].shape[1] if with_planes else 0
    planes["frac"] = np.stack([np.where(inz, table["frac"][zi, j] if n_zones else 0.0, np.nan) for j in range(F)]) if F else np.zeros((0,) + zones.shape)
    inf = info(values, classes, nodata)
    inf["n_zones"] = n_zones
    return table, planes, inf


def target_cells(S, T):
    """the number r * T.ncol + c of the target cell whose footprint holds each source cell, -1 where none does"""
    ce, re = rr.foot_cols(S, T, np.arange(T.ncol + 1)), rr.foot_rows(S, T, np.arange(T.nrow + 1))
    j, i = np.arange(S.ncol), np.arange(S.nrow)
    tc = np.searchsorted(ce, j, side="right") - 1                          # ce[tc] <= j < ce[tc + 1]; empty footprints are skipped
    tr = np.searchsorted(re, i, side="right") - 1
    tc = np.where((j >= ce[0]) & (j < ce[-1]), tc, -1)
    tr = np.where((i >= re[0]) & (i < re[-1]), tr, -1)
    unit = tr[:, None] * T.ncol + tc[None, :]
    return np.where((tr[:, None] >= 0) & (tc[None, :] >= 0), unit, -1)


def aggregate(values, S, T, classes=None, nodata=NAN, frac_of=()):
    """(planes, info): every product on T's cells"""
    if classes is None:
        classes = measure(values, nodata)
    classes, slot = slots(values, classes, nodata)
    K = classes.size
    counts, other, _ = unit_counts(target_cells(S, T).ravel(), slot.ravel(), T.nrow * T.ncol, K)
    out = finish(counts, other, classes, frac_of)
    shape = (T.nrow, T.ncol)
    planes = {name: out[name].reshape(shape) for name in ("mode", "variety", "n", "mode_frac", "simpson")}
    planes["frac"] = np.ascontiguousarray(out["frac"].T).reshape((-1,) + shape)
    return planes, info(values, classes, nodata)


def window_count(x, R, shape):
    """the number of cells with x != 0 in every cell's window (focal_ref's windows), exact in int64"""
    P = fr.blocked_prefix(np.asarray(x, dtype=np.int64), 1)
    if shape == "square":
        return fr.window_sum(fr.blocked_prefix(fr.window_sum(P, R, 1), 0), R, 0)
    nrow = P.shape[0]
    out = np.zeros(P.shape, dtype=np.int64)
    for dr in range(-R, R + 1):
        lo, hi = max(0, -dr), min(nrow, nrow - dr)
        if lo >= hi:
            continue
        out[lo:hi] += fr.window_sum(P, fr.half_width(R, abs(dr)), 1)[lo + dr:hi + dr]
    return out


def focal(values, R, classes=None, nodata=NAN, frac_of=(), shape="square"):
    """(planes, info): frac (F, nrow, ncol), mode, mode_frac, variety, n; NA (-1) where the centre is NA"""
    if classes is None:
        classes = measure(values, nodata)
    classes, slot = slots(values, classes, nodata)
    K = classes.size
    centre = slot <= K
    counts = np.stack([window_count(slot == k, R, shape) for k in range(K)], axis=-1).reshape(-1, K)
    n = window_count(centre, R, shape).ravel()
    out = finish(counts, n - counts.sum(axis=1), classes, frac_of)
    sh = slot.shape
    planes = {name: np.where(centre, out[name].reshape(sh), -1).astype(np.int32) for name in ("mode", "variety", "n")}
    planes["mode_frac"] = np.where(centre, out["mode_frac"].reshape(sh), np.nan)
    planes["frac"] = np.where(centre[None], np.ascontiguousarray(out["frac"].T).reshape((-1,) + sh), np.nan)
    return planes, info(values, classes, nodata)


# ---- the plain loops

def loop_units(values, unit, classes, nodata=NAN):
    """per unit number: (Counter of code -> cells for listed codes, other, na), by a Python loop over the cells"""
    z, ok = valid(values, nodata)
    listed = set(int(c) for c in classes)
    out = {}
    for v, good, u in zip(z.ravel().tolist(), ok.ravel().tolist(), np.asarray(unit).ravel().tolist()):
        if u < 0:
            continue
        cnt = out.setdefault(u, [Counter(), 0, 0])
        if not good:
            cnt[2] += 1
        elif v == int(v) if abs(v) < 1e18 else False:
            if int(v) in listed:
                cnt[0][int(v)] += 1
            else:
                cnt[1] += 1
        else:
            cnt[1] += 1
    return out


def loop_finish(counter, other, classes):
    """(n, mode, mode_frac, variety, simpson, fracs) of one unit with Python ints and one division each"""
    n = sum(counter.values()) + other
    best, mode = 0, -1
    for c in sorted(classes):
        if counter.get(c, 0) > best:
            best, mode = counter[c], c
    num = n * n - sum(v * v for v in counter.values()) - other * other
    return (n, mode, best / n if mode >= 0 else NAN, sum(1 for v in counter.values() if v > 0), float(num) / (float(n) * float(n)) if n else NAN,
            [counter.get(c, 0) / n if n else NAN for c in sorted(classes)])
