"""The warp rule of include/machisplin_hip.h, section "warp", restated in numpy: the lattice formula, every operation in the
header's order and rounded once, then resample_ref.interp_points at the point it gives.  What the GPU tests compare the
library with, bit for bit.

A lattice is anything with step, sx, sy (machisplin_amd.project.Lattice); geometries as in resample_ref."""
import numpy as np

import resample_ref as rr


def node_counts(T, K):
    return -(-T.nrow // K) + 1, -(-T.ncol // K) + 1


def source_points(lat, rows, cols):
    """(sx, sy) of the target cells rows x cols (2-D arrays), NaN where one of the eight node values is not finite"""
    K = int(lat.step)
    r, c = np.meshgrid(np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64), indexing="ij")
    a, b = r // K, c // K
    tv = ((r - a * K).astype(np.float64) + 0.5) / float(K)
    tu = ((c - b * K).astype(np.float64) + 0.5) / float(K)
    u0, v0 = 1.0 - tu, 1.0 - tv
    out, finite = [], np.ones(r.shape, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for P in (np.asarray(lat.sx, dtype=np.float64), np.asarray(lat.sy, dtype=np.float64)):
            p00, p01, p10, p11 = P[a, b], P[a, b + 1], P[a + 1, b], P[a + 1, b + 1]
            finite &= np.isfinite(p00) & np.isfinite(p01) & np.isfinite(p10) & np.isfinite(p11)
            top = u0 * p00 + tu * p01
            bot = u0 * p10 + tu * p11
            out.append(v0 * top + tv * bot)
    return np.where(finite, out[0], np.nan), np.where(finite, out[1], np.nan)


def warp(src, nodata, S, T, lat, method, window=None):
    """the source plane `src` (2-D) on grid S onto the window (r0, r1, c0, c1) of grid T through the lattice: float64, NaN = NA"""
    assert (np.asarray(lat.sx).shape == node_counts(T, int(lat.step))) and np.asarray(lat.sy).shape == np.asarray(lat.sx).shape
    z = rr.to_double(src, nodata)
    assert z.shape == (S.nrow, S.ncol)
    r0, r1, c0, c1 = window if window is not None else (0, T.nrow, 0, T.ncol)
    sx, sy = source_points(lat, np.arange(r0, r1), np.arange(c0, c1))
    return rr.interp_points(z, S, method, sx, sy)
