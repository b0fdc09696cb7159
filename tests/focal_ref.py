"""numpy restatement of include/machisplin_hip.h, section "focal": the blocked prefix sums (np.cumsum over the axis reshaped
to blocks of B), the row-window sums, the column prefixes of a square window, the row-by-row sum of a circular one, and
the statistics -- every operation in the header's order, so the planes equal the library's bit for bit.  And the brute-force
window loops the restatement and the library are held against."""
import numpy as np

B = 64
STATS = ("count", "sum", "mean", "sd", "min", "max", "range", "minus_mean", "above_min", "below_max", "dev")
U = 2.0 ** -53


def valid(z, nodata):
    z = np.asarray(z, dtype=np.float64)
    ok = ~np.isnan(z)
    if nodata == nodata:
        ok &= z != nodata
    return z, ok


def blocked_prefix(x, axis):
    """P of the header: sequential inside aligned blocks of B, the blocks' offsets the sequential running sum of their totals"""
    x = np.moveaxis(np.asarray(x), axis, -1)
    n = x.shape[-1]
    nb = -(-n // B)
    pad = np.zeros(x.shape[:-1] + (nb * B - n,), dtype=x.dtype)
    blocks = np.concatenate([x, pad], axis=-1).reshape(x.shape[:-1] + (nb, B))
    inblock = np.cumsum(blocks, axis=-1)                                   # sequential: p[i] = p[i - 1] + x[i]
    totals = inblock[..., -1]
    zero = np.zeros(totals.shape[:-1] + (1,), dtype=x.dtype)
    offsets = np.cumsum(np.concatenate([zero, totals[..., :-1]], axis=-1), axis=-1)      # O[0] = 0, O[k] = O[k - 1] + T[k - 1]
    P = (offsets[..., None] + inblock).reshape(x.shape[:-1] + (nb * B,))[..., :n]
    return np.moveaxis(P, -1, axis)


def window_sum(P, w, axis):
    """P[min(i + w, n - 1)] - P[max(i - w, 0) - 1] along ``axis``, P[-1] = 0; ``w`` a scalar"""
    P = np.moveaxis(P, axis, -1)
    n = P.shape[-1]
    i = np.arange(n)
    hi, lo = np.minimum(i + w, n - 1), np.maximum(i - w, 0)
    below = np.where(lo > 0, P[..., np.maximum(lo - 1, 0)], np.zeros((), dtype=P.dtype))
    return np.moveaxis(P[..., hi] - below, -1, axis)


def half_width(R, dr):
    rem = R * R - dr * dr
    d = int(np.sqrt(float(rem)))
    while d * d > rem:
        d -= 1
    while (d + 1) * (d + 1) <= rem:
        d += 1
    return d


def sums(z, nodata, R, shape, offset):
    """(n, S1, S2) of every cell's window by the header's order"""
    z, ok = valid(z, nodata)
    zc = z - offset
    a = np.where(ok, zc, 0.0)
    b = np.where(ok, zc * zc, 0.0)
    P = [blocked_prefix(a, 1), blocked_prefix(b, 1), blocked_prefix(ok.astype(np.int64), 1)]
    nrow = z.shape[0]
    if shape == "square":
        return tuple(window_sum(blocked_prefix(window_sum(p, R, 1), 0), R, 0) for p in (P[2], P[0], P[1]))
    out = [np.zeros(z.shape, dtype=np.int64), np.zeros(z.shape), np.zeros(z.shape)]
    for dr in range(-R, R + 1):
        lo, hi = max(0, -dr), min(nrow, nrow - dr)                        # the centre rows whose row r + dr is in the raster
        if lo >= hi:
            continue
        w = half_width(R, abs(dr))
        for k, p in enumerate((P[2], P[0], P[1])):
            out[k][lo:hi] = out[k][lo:hi] + window_sum(p, w, 1)[lo + dr:hi + dr]
    return tuple(out)


def minmax(z, nodata, R):
    """(min, max) of the valid cells of every cell's square window, +-inf where it has none: a running minimum along the rows, then
    down the columns (exact in any order)"""
    z, ok = valid(z, nodata)
    out = []
    for sign in (1.0, -1.0):
        m = np.where(ok, sign * z, np.inf)
        for axis in (1, 0):
            n = m.shape[axis]
            src = np.moveaxis(m, axis, -1)
            acc = src.copy()
            for d in range(1, min(R, n - 1) + 1):
                acc[..., d:] = np.minimum(acc[..., d:], src[..., :-d])
                acc[..., :-d] = np.minimum(acc[..., :-d], src[..., d:])
            m = np.moveaxis(acc, -1, axis)
        out.append(sign * m)
    return out[0], out[1]


def statistics(n, S1, S2, z, ok, offset, fill_na, mn=None, mx=None):
    """the header's formulas: a dict of planes by name (the min / max family where mn, mx are given)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        dn = n.astype(np.float64)
        some = n > 0
        mean = np.where(some, offset + S1 / dn, np.nan)
        var = (S2 - S1 * S1 / dn) / (dn - 1.0)
        sd = np.where(n >= 2, np.sqrt(np.where(var > 0.0, var, 0.0)), np.nan)
        d = np.where(ok & some, z - mean, np.nan)
        out = {"count": dn, "sum": np.where(some, S1 + dn * offset, np.nan), "mean": mean, "sd": sd, "minus_mean": d,
               "dev": np.where(sd > 0.0, d / sd, np.nan)}
        if mn is not None:
            out.update({"min": np.where(some, mn, np.nan), "max": np.where(some, mx, np.nan), "range": np.where(some, mx - mn, np.nan),
                        "above_min": np.where(ok & some, z - mn, np.nan), "below_max": np.where(ok & some, mx - z, np.nan)})
    for name in out:
        if name in ("minus_mean", "above_min", "below_max", "dev") or not fill_na:
            out[name] = np.where(ok, out[name], np.nan)
    return out


def focal(z, nodata, R, names, shape="square", fill_na=False, offset=0.0, window=None):
    """the planes ``names`` (len(names), rows, cols) of the header's rule"""
    zz, ok = valid(z, nodata)
    n, S1, S2 = sums(z, nodata, R, shape, offset)
    mn, mx = minmax(z, nodata, R) if shape == "square" and any(k in ("min", "max", "range", "above_min", "below_max") for k in names) else (None, None)
    st = statistics(n, S1, S2, zz, ok, offset, fill_na, mn, mx)
    out = np.stack([st[k] for k in names])
    if window is not None:
        r0, r1, c0, c1 = window
        out = out[:, r0:r1, c0:c1]
    return out


def brute(z, nodata, R, shape="square", offset=0.0, dtype=np.float64):
    """(n, S1, S2, min, max) of every cell's window by a plain loop over the window's offsets, row-major -- so every cell's sums are
    the sequential row-major sums of its window -- in ``dtype`` (np.longdouble: the reference of the bound)"""
    z, ok = valid(z, nodata)
    nr, nc = z.shape
    n = np.zeros(z.shape, dtype=np.int64)
    S1, S2 = np.zeros(z.shape, dtype=dtype), np.zeros(z.shape, dtype=dtype)
    mn, mx = np.full(z.shape, np.inf), np.full(z.shape, -np.inf)
    zc = np.where(ok, z - offset, 0.0).astype(dtype)                      # the rounded terms the library sums
    for dr in range(-min(R, nr - 1), min(R, nr - 1) + 1):
        w = R if shape == "square" else half_width(R, abs(dr))
        for dc in range(-min(w, nc - 1), min(w, nc - 1) + 1):
            dst = (slice(max(0, -dr), min(nr, nr - dr)), slice(max(0, -dc), min(nc, nc - dc)))
            src = (slice(max(0, dr), min(nr, nr + dr)), slice(max(0, dc), min(nc, nc + dc)))
            n[dst] += ok[src]
            S1[dst] = S1[dst] + zc[src]
            S2[dst] = S2[dst] + zc[src] * zc[src]
            mn[dst] = np.minimum(mn[dst], np.where(ok[src], z[src], np.inf))
            mx[dst] = np.maximum(mx[dst], np.where(ok[src], z[src], -np.inf))
    return n, S1, S2, mn, mx


def depth(n):
    """d(n) of the header's bound: the additions a term of a blocked prefix of n elements passes through at most"""
    return B + -(-n // B)


def bound(z, nodata, R, shape, offset, power=1):
    """the header's bound on |S^ - S| for S1 (power 1) or S2 (power 2), with A taken over the whole raster"""
    zz, ok = valid(z, nodata)
    A = float(np.sum(np.abs(np.where(ok, zz - offset, 0.0)) ** power))
    d = depth(zz.shape[1]) + (depth(zz.shape[0]) if shape == "square" else R) + 1
    return 2.02 * U * d * A
