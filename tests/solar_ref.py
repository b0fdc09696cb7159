"""The solar rules of include/machisplin_hip.h (section "solar") restated in numpy, every operation in the header's order and
rounded once (numpy never contracts a multiply and an add): the sixteen horizon tangents, the sky-view factor, potential direct
insolation and sun hours from host-made sun tables.  No operation goes through a math library's atan, sin or cos, so the
device planes must equal these bit for bit, every product included.

Two restatements: `solar`, vectorised over the cells, and `solar_scalar`, written independently with plain loops per cell,
direction and step for small planes.  Tables are anything with the attributes of machisplin_amd.terrain.SunTables: n_tab, start,
entries (n, 8: t, tan_h, ux, uy, uz, w, d, pad), omega, tab_row (or None)."""
import math

import numpy as np

import terrain_ref as tr

SOLAR = ("svf", "direct", "sun_hours", "horizon")
# clockwise from north: (rows south, columns east)
DIRECTIONS = ((-1, 0), (-2, 1), (-1, 1), (-1, 2), (0, 1), (1, 2), (1, 1), (2, 1),
              (1, 0), (2, -1), (1, -1), (1, -2), (0, -1), (-1, -2), (-1, -1), (-2, -1))


def horizon(plane, nodata, search, dx, dy, z_factor=1.0, dx_row=None):
    """(16, nr, nc) horizon tangents, NaN where the centre is NA"""
    z = tr.to_double(plane, nodata)
    nr, nc = z.shape
    L = int(search)
    zp = tr._padded(z, L)
    dxr, zf, dy = tr._dx(z, dx, dx_row), np.float64(z_factor), np.float64(dy)
    H = np.zeros((16,) + z.shape)
    for j, (dr, dc) in enumerate(DIRECTIONS):
        ry, rx = np.float64(abs(dr)) * dy, np.float64(abs(dc)) * dxr
        length = np.sqrt(ry * ry + rx * rx)
        h = np.zeros(z.shape)
        for m in range(1, L // max(abs(dr), abs(dc)) + 1):
            x = zp[L + m * dr:L + m * dr + nr, L + m * dc:L + m * dc + nc]       # NaN outside the raster and at NA cells: skipped
            with np.errstate(invalid="ignore"):
                s = ((x - z) * zf) / (np.float64(m) * length)
                h = np.where(s > h, s, h)
        H[j] = h
    H[:, np.isnan(z)] = np.nan
    return H


def solar(plane, nodata, search, tables, dx, dy, z_factor=1.0, dx_row=None):
    """dict of svf, direct, sun_hours (nr, nc) and horizon (16, nr, nc), float64 with NaN at NA cells, and "counts": the
    numbers of lit and shadowed (cell, entry) pairs over the cells with a valid centre and of pairs with c <= 0 over the cells
    with a valid slope -- what a test needs to know that its case exercises every branch."""
    z = tr.to_double(plane, nodata)
    H = horizon(plane, nodata, search, dx, dy, z_factor, dx_row)
    out = {"horizon": H}
    if tables is None:
        return out
    nr = z.shape[0]
    tab_row = np.zeros(nr, dtype=np.int64) if tables.tab_row is None else np.asarray(tables.tab_row, dtype=np.int64)
    omega = np.asarray(tables.omega, dtype=np.float64)[tab_row * 16 + np.arange(16)[:, None]]        # (16, nr)
    svf = np.zeros(z.shape)
    with np.errstate(invalid="ignore"):
        for j in range(16):
            svf = svf + omega[j][:, None] / (1.0 + H[j] * H[j])
    t3 = tr.terrain(plane, nodata, dx, dy, z_factor, dx_row)
    dzdx, dzdy = t3["dzdx"], t3["dzdy"]
    with np.errstate(invalid="ignore"):
        nrm = np.sqrt((1.0 + dzdx * dzdx) + dzdy * dzdy)
    acc, hrs = np.zeros(z.shape), np.zeros(z.shape)
    start = np.asarray(tables.start, dtype=np.int64)
    E = np.asarray(tables.entries, dtype=np.float64).reshape(-1, 8)
    n_lit = n_shadow = n_cneg = 0
    valid, has_slope = ~np.isnan(z), ~np.isnan(dzdx)
    for b in range(int(tables.n_tab)):
        rows = np.nonzero(tab_row == b)[0]
        if rows.size == 0:
            continue
        Hb, gx, gy = H[:, rows], dzdx[rows], dzdy[rows]
        a, h = acc[rows], hrs[rows]
        for j in range(16):
            h0, h1 = Hb[j], Hb[(j + 1) & 15]
            for i in range(start[16 * b + j], start[16 * b + j + 1]):
                t, tan_h, ux, uy, uz, w, d = E[i, :7]
                with np.errstate(invalid="ignore"):
                    hs = h0 + t * (h1 - h0)
                    lit = tan_h > hs
                    c = (uz - gx * ux) + gy * uy
                    a = np.where(lit & (c > 0.0), a + w * c, a)
                    h = np.where(lit, h + d, h)
                n_lit += int((lit & valid[rows]).sum())
                n_shadow += int((~lit & valid[rows]).sum())
                n_cneg += int((~(c > 0.0) & has_slope[rows]).sum())
        acc[rows], hrs[rows] = a, h
    with np.errstate(invalid="ignore"):
        direct = acc / nrm
    out["svf"] = np.where(valid, svf, np.nan)
    out["direct"] = np.where(has_slope, direct, np.nan)
    out["sun_hours"] = np.where(valid, hrs, np.nan)
    out["counts"] = {"lit": n_lit, "shadow": n_shadow, "c_neg": n_cneg}
    return out


def planes(res, names):
    """the planes of `names` one behind the other as the library lays them out (horizon: sixteen)"""
    return np.concatenate([res[n] if n == "horizon" else res[n][None] for n in names])


def solar_scalar(plane, nodata, search, tables, dx, dy, z_factor=1.0, dx_row=None):
    """the same dict (without "counts"), cell by cell with Python floats: an independent restatement for small planes"""
    z = np.asarray(plane).astype(np.float64)
    nr, nc = z.shape
    L, zf, dy = int(search), float(z_factor), float(dy)

    def na(v):
        return v != v or (not math.isnan(nodata) and v == nodata)

    out = {"svf": np.full((nr, nc), np.nan), "direct": np.full((nr, nc), np.nan), "sun_hours": np.full((nr, nc), np.nan),
           "horizon": np.full((16, nr, nc), np.nan)}
    for r in range(nr):
        dxc = float(dx) if dx_row is None else float(dx_row[r])
        b = 0 if tables is None or tables.tab_row is None else int(tables.tab_row[r])
        for c in range(nc):
            e = float(z[r, c])
            if na(e):
                continue
            H = []
            for dr, dc in DIRECTIONS:
                length = math.sqrt((abs(dr) * dy) * (abs(dr) * dy) + (abs(dc) * dxc) * (abs(dc) * dxc))
                best, m = 0.0, 1
                while max(abs(m * dr), abs(m * dc)) <= L and 0 <= r + m * dr < nr and 0 <= c + m * dc < nc:
                    v = float(z[r + m * dr, c + m * dc])
                    if not na(v):
                        s = ((v - e) * zf) / (float(m) * length)
                        if s > best:
                            best = s
                    m += 1
                H.append(best)
            out["horizon"][:, r, c] = H
            if tables is None:
                continue
            svf = 0.0
            for j in range(16):
                svf = svf + float(tables.omega[16 * b + j]) / (1.0 + H[j] * H[j])
            out["svf"][r, c] = svf
            slope = None
            if 1 <= r < nr - 1 and 1 <= c < nc - 1:
                n9 = [float(z[r + i, c + k]) for i in (-1, 0, 1) for k in (-1, 0, 1)]
                if not any(na(v) for v in n9):
                    a_, b_, c_, d_, _, f_, g_, h_, i_ = n9
                    slope = ((((c_ + 2.0 * f_) + i_) - ((a_ + 2.0 * d_) + g_)) * zf / (8.0 * dxc),
                             (((g_ + 2.0 * h_) + i_) - ((a_ + 2.0 * b_) + c_)) * zf / (8.0 * dy))
            acc = hrs = 0.0
            for j in range(16):
                for i in range(int(tables.start[16 * b + j]), int(tables.start[16 * b + j + 1])):
                    t, tan_h, ux, uy, uz, w, d = (float(v) for v in tables.entries[i][:7])
                    hs = H[j] + t * (H[(j + 1) & 15] - H[j])
                    if tan_h > hs:
                        hrs = hrs + d
                        if slope is not None:
                            cc = (uz - slope[0] * ux) + slope[1] * uy
                            if cc > 0.0:
                                acc = acc + w * cc
            out["sun_hours"][r, c] = hrs
            if slope is not None:
                out["direct"][r, c] = acc / math.sqrt((1.0 + slope[0] * slope[0]) + slope[1] * slope[1])
    return out
