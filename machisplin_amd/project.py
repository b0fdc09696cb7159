"""Rasters onto a grid in another coordinate system: lon/lat to UTM and back.

The reference package's README says "All rasters must be the same: resolution, projection and extent".  ``resample`` closes
resolution and extent; this module closes projection.  The rasters the package is used with are lon/lat (SRTM, WorldClim, the
stations' ``long`` / ``lat``), while ``proximity``, ``flowpath`` and the ``dist_*`` / ``hand`` covariates want a metric grid:
``project`` brings a stack onto one, ``transform_points`` the stations, ``io.write_geotiff(..., epsg=)`` stamps the result.

The device never sees a projection (include/machisplin_hip.h, section "warp", states the rule).  This module evaluates the
transform from target to source coordinates in numpy on a CONTROL LATTICE of the target grid, one node every K cells, and
MEASURES the lattice's interpolation error against the exact transform (:func:`lattice_from` keeps the largest K within
``tol`` source cells and returns the measured error with the lattice); csrc/warp.hip interpolates the lattice at each cell
centre and applies the resample rule there.  So a warped cell equals ``resample.extract`` at the lattice's point, bit for bit.

Coordinate systems: :data:`LONLAT` (degrees, WGS 84) and transverse Mercator (:func:`tmerc`, :func:`utm`) by the Krueger
series in the third flattening n through n^6 (Karney 2011, "Transverse Mercator with an accuracy of a few nanometers"), the
conformal latitude inverted by Newton iteration.  Any other transform (pyproj, say) plugs in through :func:`lattice_from`.

Only the interpolating methods warp.  A much coarser target is made by ``resample.resample(..., "mean")`` in the source
system first, then a warp.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .raster import Geometry, RasterStack

WGS84_A = 6378137.0
WGS84_F = 1.0 / 298.257223563
TMERC_MAX_DLON = 15.0            # degrees of longitude from the central meridian beyond which a transverse Mercator gives NaN
METHODS = ("near", "bilinear", "cubic")             # MHS_RS_NEAR, MHS_RS_BILINEAR, MHS_RS_CUBIC
STEPS = (256, 128, 64, 32, 16, 8, 4, 2, 1)
# where a lattice cell is checked, as fractions of the cell: its centre, the four edge midpoints (where each second derivative's
# term of the bilinear error peaks) and the quarter points between them -- 21 points, the corners (error 0) left out
_CHECK_T = tuple((tu, tv) for tv in (0.0, 0.25, 0.5, 0.75, 1.0) for tu in (0.0, 0.25, 0.5, 0.75, 1.0) if not (tu in (0.0, 1.0) and tv in (0.0, 1.0)))
_CHECK_CHUNK = 1 << 21           # points of one evaluation of the exact transform


@dataclass(frozen=True)
class Crs:
    """A coordinate system: ``kind`` "lonlat" (x = longitude, y = latitude, degrees) or "tmerc" (metres)."""
    kind: str
    lon0: float = 0.0
    lat0: float = 0.0
    k0: float = 1.0
    x0: float = 0.0
    y0: float = 0.0
    a: float = WGS84_A
    f: float = WGS84_F
    epsg: int | None = None


LONLAT = Crs("lonlat", epsg=4326)


def tmerc(lon0, lat0=0.0, k0=0.9996, x0=500000.0, y0=0.0, a=WGS84_A, f=WGS84_F) -> Crs:
    """Transverse Mercator about the central meridian ``lon0`` (degrees), origin latitude ``lat0``, scale ``k0`` on the meridian,
    false easting and northing ``x0``, ``y0`` (metres), on the ellipsoid (``a``, ``f``)."""
    return Crs("tmerc", float(lon0), float(lat0), float(k0), float(x0), float(y0), float(a), float(f), None)


def utm(zone: int, south: bool = False) -> Crs:
    """WGS 84 / UTM zone ``zone`` (1 .. 60): EPSG 326zz north, 327zz south (false northing 10 000 000 m)."""
    zone = int(zone)
    if not 1 <= zone <= 60:
        raise ValueError("a UTM zone is 1 .. 60")
    return Crs("tmerc", -183.0 + 6.0 * zone, 0.0, 0.9996, 500000.0, 1.0e7 if south else 0.0, WGS84_A, WGS84_F, (32700 if south else 32600) + zone)


def utm_zone(lon, lat=0.0) -> int:
    """The UTM zone of a point, with the exceptions of southern Norway (32V) and Svalbard (31X, 33X, 35X, 37X)."""
    lon = (float(lon) + 180.0) % 360.0 - 180.0
    zone = min(60, int(math.floor((lon + 180.0) / 6.0)) + 1)
    if 56.0 <= lat < 64.0 and 3.0 <= lon < 12.0:
        zone = 32
    if 72.0 <= lat <= 84.0 and 0.0 <= lon < 42.0:
        zone = 31 if lon < 9.0 else 33 if lon < 21.0 else 35 if lon < 33.0 else 37
    return zone


def from_epsg(code: int) -> Crs:
    """4326, or a WGS 84 / UTM code 32601 .. 32660 (north), 32701 .. 32760 (south)."""
    code = int(code)
    if code == 4326:
        return LONLAT
    if 32601 <= code <= 32660:
        return utm(code - 32600)
    if 32701 <= code <= 32760:
        return utm(code - 32700, south=True)
    raise ValueError(f"EPSG:{code} is not supported: 4326, 32601 .. 32660 (WGS 84 / UTM north), 32701 .. 32760 (UTM south)")


def _series(crs: Crs):
    """third flattening n, rectifying radius A, the forward (alpha) and inverse (beta) coefficients of the Krueger series"""
    n = crs.f / (2.0 - crs.f)
    n2, n3, n4, n5, n6 = n * n, n ** 3, n ** 4, n ** 5, n ** 6
    A = crs.a / (1.0 + n) * (1.0 + n2 / 4.0 + n4 / 64.0 + n6 / 256.0)
    alpha = (n / 2 - 2 * n2 / 3 + 5 * n3 / 16 + 41 * n4 / 180 - 127 * n5 / 288 + 7891 * n6 / 37800,
             13 * n2 / 48 - 3 * n3 / 5 + 557 * n4 / 1440 + 281 * n5 / 630 - 1983433 * n6 / 1935360,
             61 * n3 / 240 - 103 * n4 / 140 + 15061 * n5 / 26880 + 167603 * n6 / 181440,
             49561 * n4 / 161280 - 179 * n5 / 168 + 6601661 * n6 / 7257600,
             34729 * n5 / 80640 - 3418889 * n6 / 1995840,
             212378941 * n6 / 319334400)
    beta = (n / 2 - 2 * n2 / 3 + 37 * n3 / 96 - n4 / 360 - 81 * n5 / 512 + 96199 * n6 / 604800,
            n2 / 48 + n3 / 15 - 437 * n4 / 1440 + 46 * n5 / 105 - 1118711 * n6 / 3870720,
            17 * n3 / 480 - 37 * n4 / 840 - 209 * n5 / 4480 + 5569 * n6 / 90720,
            4397 * n4 / 161280 - 11 * n5 / 504 - 830251 * n6 / 7257600,
            4583 * n5 / 161280 - 108847 * n6 / 3991680,
            20648693 * n6 / 638668800)
    return n, A, alpha, beta


def _taup(tau, e):
    """tangent of the conformal latitude from the tangent of the geographic latitude"""
    sig = np.sinh(e * np.arctanh(e * tau / np.sqrt(1.0 + tau * tau)))
    return tau * np.sqrt(1.0 + sig * sig) - sig * np.sqrt(1.0 + tau * tau)


def _xi0(crs: Crs) -> float:
    """rectifying latitude of the origin latitude (0 for lat0 = 0)"""
    if crs.lat0 == 0.0:
        return 0.0
    _, _, alpha, _ = _series(crs)
    e = math.sqrt(crs.f * (2.0 - crs.f))
    xp = float(np.arctan(_taup(np.tan(np.radians(np.float64(crs.lat0))), e)))
    return xp + sum(al * math.sin(2 * (j + 1) * xp) for j, al in enumerate(alpha))


def _tmerc_forward(crs: Crs, lon, lat):
    _, A, alpha, _ = _series(crs)
    e = math.sqrt(crs.f * (2.0 - crs.f))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dlon = np.remainder(lon - crs.lon0 + 180.0, 360.0) - 180.0
        ok = (np.abs(dlon) <= TMERC_MAX_DLON) & (np.abs(lat) <= 90.0)
        lam, phi = np.radians(np.where(ok, dlon, 0.0)), np.radians(np.where(ok, lat, 0.0))
        tp = _taup(np.tan(phi), e)
        xip = np.arctan2(tp, np.cos(lam))
        etap = np.arcsinh(np.sin(lam) / np.hypot(tp, np.cos(lam)))
        xi, eta = xip.copy(), etap.copy()
        for j, al in enumerate(alpha):
            m = 2.0 * (j + 1)
            xi = xi + al * np.sin(m * xip) * np.cosh(m * etap)
            eta = eta + al * np.cos(m * xip) * np.sinh(m * etap)
        x = crs.x0 + crs.k0 * A * eta
        y = crs.y0 + crs.k0 * A * (xi - _xi0(crs))
    return np.where(ok, x, np.nan), np.where(ok, y, np.nan)


def _tmerc_inverse(crs: Crs, x, y):
    _, A, _, beta = _series(crs)
    e2 = crs.f * (2.0 - crs.f)
    e = math.sqrt(e2)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        xi = (y - crs.y0) / (crs.k0 * A) + _xi0(crs)
        eta = (x - crs.x0) / (crs.k0 * A)
        ok = np.isfinite(xi) & np.isfinite(eta) & (np.abs(eta) < 1.0)
        xi, eta = np.where(ok, xi, 0.0), np.where(ok, eta, 0.0)
        xip, etap = xi.copy(), eta.copy()
        for j, be in enumerate(beta):
            m = 2.0 * (j + 1)
            xip = xip - be * np.sin(m * xi) * np.cosh(m * eta)
            etap = etap - be * np.cos(m * xi) * np.sinh(m * eta)
        ok &= np.abs(xip) <= 0.5 * math.pi                         # beyond a pole
        sh, cx = np.sinh(etap), np.cos(xip)
        lam = np.arctan2(sh, cx)
        tp = np.sin(xip) / np.hypot(sh, cx)
        tau = tp.copy()
        for _ in range(6):                                         # Newton on taup(tau) = tp: quadratic, 3 rounds reach rounding
            ti = _taup(tau, e)
            tau = tau + (tp - ti) / np.sqrt(1.0 + ti * ti) * (1.0 + (1.0 - e2) * tau * tau) / ((1.0 - e2) * np.sqrt(1.0 + tau * tau))
        dlon, lat = np.degrees(lam), np.degrees(np.arctan(tau))
        ok &= np.abs(dlon) <= TMERC_MAX_DLON
        lon = np.remainder(crs.lon0 + dlon + 180.0, 360.0) - 180.0
    return np.where(ok, lon, np.nan), np.where(ok, lat, np.nan)


def transform(src: Crs, dst: Crs, x, y):
    """(x, y) of ``src`` in ``dst``: float64 arrays of one shape.  NaN where a transverse Mercator is asked for a point more
    than :data:`TMERC_MAX_DLON` degrees of longitude from its central meridian, or beyond a pole -- never garbage."""
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    if src == dst:
        return x.copy(), y.copy()
    lon, lat = (x, y) if src.kind == "lonlat" else _tmerc_inverse(src, x, y)
    if dst.kind == "lonlat":
        with np.errstate(invalid="ignore"):
            return np.array(lon, dtype=np.float64), np.where(np.abs(lat) <= 90.0, lat, np.nan)
    return _tmerc_forward(dst, lon, lat)


def transform_points(xy, src: Crs, dst: Crs) -> np.ndarray:
    """The stations on the new grid: ``xy`` (n x 2: x, y) of ``src`` as an n x 2 array of ``dst``."""
    xy = np.asarray(xy, dtype=np.float64)
    if xy.ndim != 2 or xy.shape[1] != 2:
        raise ValueError("xy must be n x 2")
    return np.column_stack(transform(src, dst, xy[:, 0], xy[:, 1]))


@dataclass
class Lattice:
    """The control lattice of a target grid (struct mhs_warp_lattice): node (a, b) holds the source coordinates of the
    target-grid point (xmin + b step xres, ymax - a step yres).  ``max_error``: the largest distance, in source cells, between
    the exact transform and the lattice's interpolation over the ``n_checked`` points it was measured at; ``n_skipped``: the
    check points left out of the measure because the transform or a node of their lattice cell has no value there (the cells
    of such a lattice cell come out NA).  The last, partial lattice cell of a row or column reaches beyond the grid: if the
    transform has no value at ITS far nodes (next to :data:`TMERC_MAX_DLON` or a pole), the grid's cells in it are NA although
    the exact transform has a value at them -- ``n_skipped`` > 0 says that this can be the case.
    ``sx`` and ``sy`` may be edited (holes, say): a warp uploads them again whenever their contents have changed."""
    step: int
    sx: np.ndarray
    sy: np.ndarray
    max_error: float = float("nan")
    n_checked: int = 0
    n_skipped: int = 0
    _dev: dict = field(default_factory=dict, repr=False, compare=False)

    def device_arrays(self, device):
        """(sx, sy) on the device, uploaded once per device and again when the host arrays' contents change"""
        import torch
        sx, sy = np.ascontiguousarray(self.sx, dtype=np.float64), np.ascontiguousarray(self.sy, dtype=np.float64)
        if sx.ndim != 2 or sx.shape != sy.shape:
            raise ValueError("a lattice's sx and sy must be 2-D arrays of one shape")
        key, stamp = str(device), (sx.shape, hash(sx.tobytes()), hash(sy.tobytes()))
        if key not in self._dev or self._dev[key][0] != stamp:
            self._dev[key] = (stamp, torch.from_numpy(sx).to(device), torch.from_numpy(sy).to(device))
        return self._dev[key][1:]


def node_counts(geom: Geometry, step: int):
    return -(-geom.nrow // step) + 1, -(-geom.ncol // step) + 1


def _bilerp(p00, p01, p10, p11, tu, tv):
    """the section's formula, in its order"""
    u0, v0 = 1.0 - tu, 1.0 - tv
    top = u0 * p00 + tu * p01
    bot = u0 * p10 + tu * p11
    return v0 * top + tv * bot


def _lattice_at(fn, geom: Geometry, src_geom: Geometry, K: int) -> Lattice:
    nr, nc = node_counts(geom, K)
    X = geom.xmin + (np.arange(nc, dtype=np.float64) * K) * geom.xres
    Y = geom.ymax - (np.arange(nr, dtype=np.float64) * K) * geom.yres
    Yg, Xg = np.meshgrid(Y, X, indexing="ij")
    sx, sy = fn(Xg, Yg)
    sx, sy = np.ascontiguousarray(sx, dtype=np.float64), np.ascontiguousarray(sy, dtype=np.float64)
    if sx.shape != (nr, nc) or sy.shape != (nr, nc):
        raise ValueError("fn(X, Y) must return two arrays of X's shape")
    worst, n_checked, n_skipped = 0.0, 0, 0
    rows_per = max(1, _CHECK_CHUNK // max(1, (nc - 1) * len(_CHECK_T)))
    bcol = np.arange(nc - 1, dtype=np.float64)
    for a0 in range(0, nr - 1, rows_per):
        a1 = min(nr - 1, a0 + rows_per)
        arow = np.arange(a0, a1, dtype=np.float64)
        sl, sr = slice(a0, a1), slice(a0 + 1, a1 + 1)
        for tu, tv in _CHECK_T:
            Yc, Xc = np.meshgrid(geom.ymax - ((arow + tv) * K) * geom.yres, geom.xmin + ((bcol + tu) * K) * geom.xres, indexing="ij")
            ex, ey = fn(Xc, Yc)
            ix = _bilerp(sx[sl, :-1], sx[sl, 1:], sx[sr, :-1], sx[sr, 1:], tu, tv)
            iy = _bilerp(sy[sl, :-1], sy[sl, 1:], sy[sr, :-1], sy[sr, 1:], tu, tv)
            with np.errstate(invalid="ignore"):
                err = np.maximum(np.abs(ix - ex) / src_geom.xres, np.abs(iy - ey) / src_geom.yres)
            good = np.isfinite(err)
            n_checked += int(good.sum())
            n_skipped += int(good.size - good.sum())
            if good.any():
                worst = max(worst, float(err[good].max()))
    return Lattice(K, sx, sy, worst, n_checked, n_skipped)


def lattice_from(fn, geom: Geometry, src_geom: Geometry, tol: float = 0.01, step: int | None = None) -> Lattice:
    """The control lattice of the target grid ``geom`` for the transform ``fn(X, Y) -> (sx, sy)`` from target to source
    coordinates (float64 arrays in, arrays of the same shape out; NaN where the transform has no value: those cells come out NA).
    Tries the steps 256, 128, ..., 1 and keeps the largest whose MEASURED error is at most ``tol`` source cells -- the largest
    of |sx - fn's| / src_geom.xres and |sy - fn's| / src_geom.yres between the section's interpolation formula and ``fn`` itself at
    21 points of every lattice cell (its centre, its edge midpoints, the quarter points between) -- and raises if step 1 fails.
    A check point at which ``fn`` or a node of its lattice cell is not finite cannot be measured: it is counted in
    ``n_skipped``, not in ``n_checked`` (see :class:`Lattice` for what that means at the grid's far edges).
    ``step`` forces one step (still measured, still held to ``tol``).  With pyproj:
    ``lattice_from(lambda X, Y: Transformer.from_crs(dst, src, always_xy=True).transform(X, Y), geom, src_geom)``."""
    if not tol > 0.0:
        raise ValueError("tol must be positive")
    if step is not None and (int(step) not in STEPS and int(step) not in (512, 1024)):
        raise ValueError("step must be a power of two in 1 .. 1024")
    lat = None
    for K in ((int(step),) if step is not None else STEPS):
        lat = _lattice_at(fn, geom, src_geom, K)
        if lat.max_error <= tol:
            return lat
    raise ValueError(f"the lattice misses tol = {tol} source cells even at step {lat.step}: measured {lat.max_error:.3g}")


def lattice(src_crs: Crs, dst_crs: Crs, geom: Geometry, src_geom: Geometry, tol: float = 0.01, step: int | None = None) -> Lattice:
    """:func:`lattice_from` with this module's transform from ``dst_crs`` (the target grid ``geom``) back to ``src_crs``."""
    return lattice_from(lambda X, Y: transform(dst_crs, src_crs, X, Y), geom, src_geom, tol, step)


def suggest_geometry(src_geom: Geometry, src_crs: Crs, dst_crs: Crs, res: float | None = None) -> Geometry:
    """A target grid for ``src_geom`` in ``dst_crs``: the bounding box of the source's boundary (41 points a side) transformed,
    square cells of ``res`` -- default: the box's diagonal divided by the source's diagonal cell count, GDAL's rule -- and an
    origin snapped outward to multiples of ``res``."""
    t = np.linspace(0.0, 1.0, 41)
    xs = src_geom.xmin + t * (src_geom.ncol * src_geom.xres)
    ys = src_geom.ymax - t * (src_geom.nrow * src_geom.yres)
    bx = np.concatenate([xs, xs, np.full(t.size, xs[0]), np.full(t.size, xs[-1])])
    by = np.concatenate([np.full(t.size, ys[0]), np.full(t.size, ys[-1]), ys, ys])
    X, Y = transform(src_crs, dst_crs, bx, by)
    if not (np.isfinite(X).all() and np.isfinite(Y).all()):
        raise ValueError("part of the source's boundary has no coordinates in the target system")
    x_lo, x_hi, y_lo, y_hi = X.min(), X.max(), Y.min(), Y.max()
    if res is None:
        res = math.hypot(x_hi - x_lo, y_hi - y_lo) / math.hypot(src_geom.ncol, src_geom.nrow)
    res = float(res)
    if not (res > 0.0 and math.isfinite(res)):
        raise ValueError("res must be positive")
    xmin, ymax = math.floor(x_lo / res) * res, math.ceil(y_hi / res) * res
    ncol, nrow = max(1, math.ceil((x_hi - xmin) / res)), max(1, math.ceil((ymax - y_lo) / res))
    while xmin + ncol * res < x_hi:                                # the rounding of the quotient must not lose the last point
        ncol += 1
    while ymax - nrow * res > y_lo:
        nrow += 1
    return Geometry(xmin, ymax, res, res, int(nrow), int(ncol))


def _method(method) -> int:
    if method not in METHODS:
        raise ValueError(f"unknown or aggregate method {method!r}: a warp takes one of {', '.join(METHODS)} "
                         "(for a much coarser target, resample.resample(..., 'mean') in the source system first)")
    return METHODS.index(method)


def warp(stack: RasterStack, geom: Geometry, lattice: Lattice, method="bilinear", out_dtype=None, window=None, out=None, stream=None) -> RasterStack:
    """Every layer of ``stack`` on the grid ``geom`` of another coordinate system, in one launch, through the control lattice
    ``lattice`` of ``geom`` (:func:`lattice`, :func:`lattice_from`).  ``method``: ``near``, ``bilinear`` or ``cubic``.
    ``out_dtype``, ``window`` and ``out`` as in ``resample.resample``: a window gives those cells of the whole-grid result bit
    for bit.  NaN where the lattice's point is outside the source, where a node is not finite and where the method gives NA."""
    import torch
    code = _method(method)
    r0, r1, c0, c1 = (int(x) for x in window) if window is not None else (0, geom.nrow, 0, geom.ncol)
    if out_dtype is None:
        out_dtype = out.dtype if out is not None else torch.float64 if stack.planes.dtype == torch.float64 else torch.float32
    if out_dtype not in (torch.float64, torch.float32):
        raise ValueError("out_dtype must be torch.float64 or torch.float32")
    shape = (stack.n_layers, r1 - r0, c1 - c0)
    if out is None:
        out = torch.empty(shape, dtype=out_dtype, device=stack.planes.device)
    if out.dtype != out_dtype or not out.is_cuda or out.dim() != 3 or tuple(out.shape) != shape or (out.numel() and out.stride(2) != 1):
        raise ValueError("out must be a device tensor (layers, rows, cols) of out_dtype with unit column stride")
    st = stream if stream is not None else torch.cuda.current_stream(stack.planes.device).cuda_stream
    lx, ly = lattice.device_arrays(stack.planes.device)
    lat = _lib.WarpLattice(int(lattice.step), lx.shape[0], lx.shape[1], lx.data_ptr(), ly.data_ptr())
    sg, ss, tg = stack.geom.c_struct(), stack.c_struct(), geom.c_struct()
    _lib.check(_lib.lib().mhs_warp_dev(C.byref(sg), C.byref(ss), C.byref(tg), r0, r1, c0, c1, C.byref(lat), code, out.data_ptr(), out.stride(1),
                                       out.stride(0), _lib.F64 if out_dtype == torch.float64 else _lib.F32, st))
    res = RasterStack.__new__(RasterStack)          # keeps `out` as it is: RasterStack() would copy a padded tensor
    res.planes, res.geom, res.nodata = out, geom.window(r0, r1, c0, c1) if window is not None else geom, float("nan")
    return res


def project(stack: RasterStack, src_crs: Crs, dst_crs: Crs, geom: Geometry | None = None, res: float | None = None, method="bilinear",
            tol: float = 0.01):
    """``stack`` (on a grid of ``src_crs``) in ``dst_crs``: ``(RasterStack, Lattice)``.  ``geom``: the target grid, default
    :func:`suggest_geometry` with ``res``.  The lattice carries the measured error (``max_error`` <= ``tol`` source cells)."""
    if geom is None:
        geom = suggest_geometry(stack.geom, src_crs, dst_crs, res)
    lat = lattice(src_crs, dst_crs, geom, stack.geom, tol)
    return warp(stack, geom, lat, method), lat
