"""The terrain rules of include/machisplin_hip.h (section "terrain") restated in numpy, every operation in the header's order
and rounded once (numpy never contracts a multiply and an add): the 3 x 3 terrain variables, relief in a circular window,
geomorphons.  What the device planes must equal bit for bit -- but for slope_deg, aspect_deg and the geomorphons' angles,
which go through atan / atan2."""
import numpy as np

VARS = ("dzdx", "dzdy", "slope_tan", "slope_deg", "eastness", "northness", "aspect_deg", "tpi", "tri", "roughness")
STATS = ("above_min", "below_max", "minus_mean")
FL, PK, RI, SH, SP, SL, HO, FS, VL, PT = range(1, 11)
GEOMORPHON_NA = -32768
#        plus: 0   1   2   3   4   5   6   7   8
FORM = np.array([[FL, FL, FL, FS, FS, VL, VL, VL, PT],       # minus 0
                 [FL, FL, FS, FS, FS, VL, VL, VL, 0],
                 [FL, SH, SL, SL, HO, HO, VL, 0, 0],
                 [SH, SH, SL, SL, SL, HO, 0, 0, 0],
                 [SH, SH, SP, SL, SL, 0, 0, 0, 0],
                 [RI, RI, SP, SP, 0, 0, 0, 0, 0],
                 [RI, RI, RI, 0, 0, 0, 0, 0, 0],
                 [RI, RI, 0, 0, 0, 0, 0, 0, 0],
                 [PK, 0, 0, 0, 0, 0, 0, 0, 0]], dtype=np.int16)
DEG = 180.0 / np.pi
RAD = np.pi / 180.0


def to_double(plane, nodata):
    """the plane as float64 with NaN at every NA cell (NaN, or equal to the stack's nodata)"""
    z = np.asarray(plane).astype(np.float64)
    if not np.isnan(nodata):
        z = np.where(z == nodata, np.nan, z)
    return z


def _padded(z, h):
    zp = np.full((z.shape[0] + 2 * h, z.shape[1] + 2 * h), np.nan)        # cells outside the raster count as NA
    zp[h:h + z.shape[0], h:h + z.shape[1]] = z
    return zp


def _dx(z, dx, dx_row):
    return np.full((z.shape[0], 1), float(dx)) if dx_row is None else np.asarray(dx_row, dtype=np.float64).reshape(-1, 1)


def terrain(plane, nodata, dx, dy, z_factor=1.0, dx_row=None):
    """dict of the ten 3 x 3 variables (float64, NaN where any of the nine cells is NA)"""
    z = to_double(plane, nodata)
    nr, nc = z.shape
    zp = _padded(z, 1)
    a, b, c = zp[0:nr, 0:nc], zp[0:nr, 1:nc + 1], zp[0:nr, 2:nc + 2]
    d, e, f = zp[1:nr + 1, 0:nc], zp[1:nr + 1, 1:nc + 1], zp[1:nr + 1, 2:nc + 2]
    g, h, i = zp[2:nr + 2, 0:nc], zp[2:nr + 2, 1:nc + 1], zp[2:nr + 2, 2:nc + 2]
    nine = (a, b, c, d, e, f, g, h, i)
    na = np.zeros(z.shape, dtype=bool)
    for x in nine:
        na |= np.isnan(x)
    dxr, zf, dy = _dx(z, dx, dx_row), np.float64(z_factor), np.float64(dy)
    out = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        dzdx = (((c + 2.0 * f) + i) - ((a + 2.0 * d) + g)) * zf / (8.0 * dxr)
        dzdy = (((g + 2.0 * h) + i) - ((a + 2.0 * b) + c)) * zf / (8.0 * dy)
        st = np.sqrt(dzdx * dzdx + dzdy * dzdy)
        flat = st == 0.0
        out["dzdx"], out["dzdy"], out["slope_tan"] = dzdx, dzdy, st
        out["slope_deg"] = np.arctan(st) * DEG
        out["eastness"] = np.where(flat, 0.0, -dzdx / st)
        out["northness"] = np.where(flat, 0.0, dzdy / st)
        deg = np.arctan2(-dzdx, dzdy) * DEG
        out["aspect_deg"] = np.where(flat, -1.0, np.where(deg < 0.0, deg + 360.0, deg))
        out["tpi"] = (e - (((((((a + b) + c) + d) + f) + g) + h) + i) / 8.0) * zf
        ab = [np.abs(x - e) for x in (a, b, c, d, f, g, h, i)]
        out["tri"] = (((((((ab[0] + ab[1]) + ab[2]) + ab[3]) + ab[4]) + ab[5]) + ab[6]) + ab[7]) / 8.0 * zf
        mn, mx = a, a
        for x in nine[1:]:
            mn, mx = np.where(x < mn, x, mn), np.where(x > mx, x, mx)
        out["roughness"] = (mx - mn) * zf
    return {k: np.where(na, np.nan, v) for k, v in out.items()}


def relief(plane, nodata, radius, z_factor=1.0):
    """dict of the three relief statistics in the circular window of `radius` cells (NaN where the centre is NA)"""
    z = to_double(plane, nodata)
    nr, nc = z.shape
    R = int(radius)
    zp = _padded(z, R)
    mn, mx = np.full(z.shape, np.inf), np.full(z.shape, -np.inf)
    total, count = np.zeros(z.shape), np.zeros(z.shape)
    for dr in range(-R, R + 1):                          # row-major over the offsets
        for dc in range(-R, R + 1):
            if dr * dr + dc * dc > R * R:
                continue
            x = zp[R + dr:R + dr + nr, R + dc:R + dc + nc]
            ok = ~np.isnan(x)
            with np.errstate(invalid="ignore"):
                mn = np.where(ok & (x < mn), x, mn)
                mx = np.where(ok & (x > mx), x, mx)
                total = np.where(ok, total + x, total)
            count = count + ok
    zf = np.float64(z_factor)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = {"above_min": (z - mn) * zf, "below_max": (mx - z) * zf, "minus_mean": (z - total / count) * zf}
    return {k: np.where(np.isnan(z), np.nan, v) for k, v in out.items()}


DIRECTIONS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))        # N NE E SE S SW W NW


def geomorphon(plane, nodata, search, flat_deg, dx, dy, z_factor=1.0, dx_row=None):
    """(forms int16 with -32768 at NA cells, margin): margin = the smallest | |D| - t | over every direction of every cell
    that is not NA, D = atan(a) + atan(b) -- how far the nearest decision is from its threshold, in radians.  Directions
    with a == b == 0 (a level ray) are left out of it: atan(0) is 0 exactly in every math library, so their D is 0 exactly."""
    z = to_double(plane, nodata)
    nr, nc = z.shape
    L = int(search)
    zp = _padded(z, L)
    dxr, zf, dy = _dx(z, dx, dx_row), np.float64(z_factor), np.float64(dy)
    diag = np.sqrt(dy * dy + dxr * dxr)
    t = np.float64(flat_deg) * RAD
    na = np.isnan(z)
    plus, minus = np.zeros(z.shape, dtype=np.int64), np.zeros(z.shape, dtype=np.int64)
    deltas = []
    for dr, dc in DIRECTIONS:
        step = dy if dc == 0 else dxr if dr == 0 else diag
        alive = ~np.isnan(z)
        have = np.zeros(z.shape, dtype=bool)
        a, b = np.zeros(z.shape), np.zeros(z.shape)
        for k in range(1, L + 1):
            x = zp[L + k * dr:L + k * dr + nr, L + k * dc:L + k * dc + nc]
            ok = alive & ~np.isnan(x)                   # a ray stops at the first NA or outside cell
            with np.errstate(invalid="ignore"):
                s = ((x - z) * zf) / (np.float64(k) * step)
                a = np.where(ok & (~have | (s > a)), s, a)
                b = np.where(ok & (~have | (s < b)), s, b)
            have |= ok
            alive = ok
        na = na | ~have
        delta = np.arctan(a) + np.arctan(b)
        plus += delta > t
        minus += delta < -t
        deltas.append(np.where((a == 0.0) & (b == 0.0), np.inf, delta))
    forms = FORM[np.where(na, 0, minus), np.where(na, 0, plus)]
    forms = np.where(na, np.int16(GEOMORPHON_NA), forms).astype(np.int16)
    d = np.stack(deltas)[:, ~na]
    margin = float(np.abs(np.abs(d) - t).min()) if d.size else np.inf
    return forms, margin
