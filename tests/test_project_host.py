"""CPU: the host side of the warp (machisplin_amd/project.py; include/machisplin_hip.h, section "warp").  The transverse
Mercator series is held against its DEFINITIONS in extended precision (mpmath), not against remembered constants; the lattice
keeps its tolerance over every cell of a target; mhs_warp_dev refuses bad arguments before it touches a device; the rule header
the kernel is built from (csrc/warp_rule.h) gives the hand-worked table in a plain C++ program under AddressSanitizer + UBSan;
the GeoTIFF writer's coordinate system comes back."""
import ctypes as C
import math
import os
import subprocess

import mpmath
import numpy as np
import pytest
from PIL import Image

import warp_ref as wr
from machisplin_amd import _lib, io as mio, project as pj
from machisplin_amd.raster import Geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


# ---------------------------------------------------------------- the series against its definitions

@pytest.fixture(scope="module")
def definitions():
    """From the ellipsoid alone, in 30 digits: the rectifying radius A = (2 / pi) x the quarter meridian, by quadrature of the
    meridian arc, and the first four alpha_j = the Fourier sine coefficients of mu(chi) - chi (rectifying minus conformal
    latitude, which is what the Krueger series is on the central meridian), by quadrature over the latitude."""
    mp = mpmath
    mp.mp.dps = 30
    a, f = mp.mpf(pj.WGS84_A), mp.mpf(1) / mp.mpf("298.257223563")
    e2 = f * (2 - f)
    e = mp.sqrt(e2)

    def arc(phi):                                                  # meridian arc from the equator
        return mp.quad(lambda p: a * (1 - e2) / (1 - e2 * mp.sin(p) ** 2) ** 1.5, [0, phi])

    quarter = arc(mp.pi / 2)
    A = 2 * quarter / mp.pi

    def chi(phi):                                                  # conformal latitude, from the isometric latitude
        psi = mp.atanh(mp.sin(phi)) - e * mp.atanh(e * mp.sin(phi))
        return mp.asin(mp.tanh(psi))

    def dchi(phi):                                                 # d chi / d phi = cos chi (1 - e^2) / ((1 - e^2 sin^2 phi) cos phi)
        return mp.cos(chi(phi)) * (1 - e2) / ((1 - e2 * mp.sin(phi) ** 2) * mp.cos(phi))

    def alpha(j):                                                  # (4 / pi) int_0^{pi/2} (mu - chi) sin(2 j chi) d chi, over phi
        lim = mp.pi / 2 - mp.mpf("1e-12")                          # the integrand is O(1e-15) there: mu - chi vanishes at the pole
        return 4 / mp.pi * mp.quad(lambda p: (mp.pi / 2 * arc(p) / quarter - chi(p)) * mp.sin(2 * j * chi(p)) * dchi(p), [0, lim / 2, lim])

    return mp, a, e, A, [alpha(j) for j in (1, 2, 3, 4)]


def _forward_by_definition(defs, crs, lon, lat):
    """Gauss-Schreiber from the conformal latitude, then the four-term series with the coefficients derived above"""
    mp, _, e, A, alphas = defs
    lam, phi = mp.radians(mp.mpf(lon) - mp.mpf(crs.lon0)), mp.radians(mp.mpf(lat))
    psi = mp.atanh(mp.sin(phi)) - e * mp.atanh(e * mp.sin(phi))
    taup = mp.sinh(psi)                                            # tan of the conformal latitude
    xip = mp.atan2(taup, mp.cos(lam))
    etap = mp.asinh(mp.sin(lam) / mp.sqrt(taup ** 2 + mp.cos(lam) ** 2))
    z = mp.mpc(xip, etap)
    w = z + sum(al * mp.sin(2 * (j + 1) * z) for j, al in enumerate(alphas))
    return crs.x0 + crs.k0 * A * w.imag, crs.y0 + crs.k0 * A * w.real


def test_series_constants_are_what_the_definitions_give(definitions):
    mp, _, _, A, alphas = definitions
    n, A_mod, alpha_mod, _ = pj._series(pj.utm(31))
    assert abs(float(A) - A_mod) < 1e-8                            # metres: 2 ulp of 6.4e6 is 1.9e-9
    for j, (want, got) in enumerate(zip(alphas, alpha_mod)):
        # a coefficient is applied to A cosh(2 j eta) <= 6.4e6 x 2.6 (eta <= 0.21 at 12 degrees): 1e-14 of error is 2e-7 m
        assert abs(float(want) - got) < 1e-14, (j, float(want), got)


def test_forward_and_round_trip_against_the_definitions(definitions):
    """200 random points within 12 degrees of the central meridian and 84 degrees of the equator.  Bound (set by the issue): 1e-6 m
    for forward positions and for forward -> inverse -> forward.  Measured with this module's n^6 series: forward 1.38e-7 m --
    that is the four-term REFERENCE's own truncation: the fifth coefficient it leaves out, 5.7e-15, is worth
    A alpha_5 cosh(10 eta) <= 1.5e-7 m at 12 degrees (test_series_constants_... holds the module's alpha_1 .. alpha_4 to the
    quadrature's within 1e-14) -- and
    round trip 4.66e-9 m (float64 rounds 1e7 m to 1.9e-9).  A scratch fourth-order implementation measured 2.3e-7 m and 1.9e-7 m."""
    rng = np.random.default_rng(11)
    crs = pj.utm(31)
    lon = crs.lon0 + rng.uniform(-12.0, 12.0, 200)
    lat = rng.uniform(-84.0, 84.0, 200)
    x, y = pj.transform(pj.LONLAT, crs, lon, lat)
    assert np.isfinite(x).all() and np.isfinite(y).all()
    worst = 0.0
    for i in range(200):
        wx, wy = _forward_by_definition(definitions, crs, lon[i], lat[i])
        worst = max(worst, abs(float(wx - definitions[0].mpf(x[i]))), abs(float(wy - definitions[0].mpf(y[i]))))
    print(f"forward against the definitions: {worst:.3g} m")
    assert worst <= 1e-6
    lon2, lat2 = pj.transform(crs, pj.LONLAT, x, y)
    x2, y2 = pj.transform(pj.LONLAT, crs, lon2, lat2)
    trip = max(np.abs(x2 - x).max(), np.abs(y2 - y).max())
    print(f"forward -> inverse -> forward: {trip:.3g} m")
    assert trip <= 1e-6
    # and the inverse lands on the point it came from: 1e-6 m is 9e-12 degrees of latitude
    assert np.abs(lat2 - lat).max() < 1e-10 and np.abs(lon2 - lon).max() < 1e-9


# ---------------------------------------------------------------- fixed facts

def test_fixed_facts_of_utm():
    for zone in (1, 18, 31, 60):
        crs = pj.utm(zone)
        assert crs.lon0 == -183.0 + 6.0 * zone and crs.epsg == 32600 + zone
        x, y = pj.transform(pj.LONLAT, crs, crs.lon0, 0.0)
        assert float(x) == 500000.0 and float(y) == 0.0
        xs, ys = pj.transform(pj.LONLAT, pj.utm(zone, south=True), crs.lon0, 0.0)
        assert float(xs) == 500000.0 and float(ys) == 1.0e7
    north, south = pj.utm(18), pj.utm(18, south=True)
    assert south.epsg == 32718
    xn, yn = pj.transform(pj.LONLAT, north, [-77.3, -74.0], [-12.5, -3.0])
    xs, ys = pj.transform(pj.LONLAT, south, [-77.3, -74.0], [-12.5, -3.0])
    assert np.array_equal(xn, xs) and np.allclose(ys - yn, 1.0e7, rtol=0, atol=2e-9)
    # the scale on the central meridian is k0: a degree of latitude at the equator is k0 x 110 574.4 m (the meridian arc)
    _, y1 = pj.transform(pj.LONLAT, north, -75.0, 1.0)
    assert abs(float(y1) / 0.9996 - 110574.3886) < 1e-3
    # a transverse Mercator of its own: origin latitude, false origin
    crs = pj.tmerc(9.0, lat0=48.0, k0=1.0, x0=0.0, y0=0.0)
    x, y = pj.transform(pj.LONLAT, crs, 9.0, 48.0)
    assert float(x) == 0.0 and abs(float(y)) < 1e-8 and crs.epsg is None
    lon, lat = pj.transform(crs, pj.LONLAT, 1234.5, -987.25)
    x, y = pj.transform(pj.LONLAT, crs, lon, lat)
    assert abs(float(x) - 1234.5) < 1e-6 and abs(float(y) + 987.25) < 1e-6


def test_utm_zone_and_from_epsg():
    assert [pj.utm_zone(lon, 0.0) for lon in (-180.0, -177.0, -174.0, -75.0, 0.0, 3.0, 179.9, 180.0)] == [1, 1, 2, 18, 31, 31, 60, 1]
    assert pj.utm_zone(5.0, 60.0) == 32 and pj.utm_zone(5.0, 50.0) == 31                   # southern Norway
    assert [pj.utm_zone(lon, 78.0) for lon in (5.0, 10.0, 25.0, 35.0)] == [31, 33, 35, 37]  # Svalbard
    assert pj.from_epsg(4326) is pj.LONLAT and pj.LONLAT.epsg == 4326
    assert pj.from_epsg(32618) == pj.utm(18) and pj.from_epsg(32760) == pj.utm(60, south=True)
    for bad in (3857, 32600, 32661, 32700, 32761, 0):
        with pytest.raises(ValueError, match="4326, 32601 .. 32660"):
            pj.from_epsg(bad)
    with pytest.raises(ValueError):
        pj.utm(0)
    with pytest.raises(ValueError):
        pj.utm(61)


def test_nan_beyond_the_domain_never_garbage():
    assert pj.TMERC_MAX_DLON >= 12.0
    crs = pj.utm(31)                                               # central meridian 3
    d = pj.TMERC_MAX_DLON
    lon = np.array([3.0 + d - 1e-9, 3.0 + d + 1e-6, 3.0 - d - 1e-6, 100.0, -177.0, 3.0, 3.0, 3.0, NAN])
    lat = np.array([10.0, 10.0, 10.0, 10.0, 10.0, 90.0, 90.0001, -91.0, 10.0])
    x, y = pj.transform(pj.LONLAT, crs, lon, lat)
    assert np.isfinite(x[[0, 5]]).all() and np.isfinite(y[[0, 5]]).all()
    assert np.isnan(x[[1, 2, 3, 4, 6, 7, 8]]).all() and np.isnan(y[[1, 2, 3, 4, 6, 7, 8]]).all()
    # the inverse: an easting that far from the meridian, a northing beyond the pole, non-finite input
    xe, _ = pj.transform(pj.LONLAT, crs, 3.0 + d - 1e-6, 0.0)
    lon, lat = pj.transform(crs, pj.LONLAT, [float(xe), float(xe) + 10000.0, 500000.0, 500000.0, NAN, 1e300], [0.0, 0.0, 9.9e6, 1.1e7, 0.0, 0.0])
    assert np.isfinite(lon[[0, 2]]).all() and np.isfinite(lat[[0, 2]]).all()
    assert np.isnan(lon[[1, 3, 4, 5]]).all() and np.isnan(lat[[1, 3, 4, 5]]).all()
    # across the date line the distance from the meridian is what counts
    x, _ = pj.transform(pj.LONLAT, pj.utm(1), [179.5, -179.5], [0.0, 0.0])          # central meridian -177
    assert np.isfinite(x).all() and x[0] < x[1] < 500000.0
    pts = pj.transform_points([[3.0, 0.0], [4.0, 45.0]], pj.LONLAT, crs)
    assert pts.shape == (2, 2) and pts[0, 0] == 500000.0
    with pytest.raises(ValueError):
        pj.transform_points([1.0, 2.0], pj.LONLAT, crs)


# ---------------------------------------------------------------- the lattice

SRC_1S = Geometry(5.5, 45.3, 1.0 / 3600.0, 1.0 / 3600.0, 1200, 1800)          # 1 arc second, at the east edge of zone 31


def _utm_target(n=300, res=30.0):
    x, y = pj.transform(pj.LONLAT, pj.utm(31), 5.75, 45.15)
    return Geometry(math.floor(float(x) / res) * res - (n // 2) * res, math.floor(float(y) / res) * res + (n // 2) * res, res, res, n, n)


@pytest.mark.parametrize("tol", [0.01, 0.001, 0.0001])
def test_lattice_keeps_its_tolerance_over_every_cell(tol):
    T = _utm_target()
    lat = pj.lattice(pj.LONLAT, pj.utm(31), T, SRC_1S, tol=tol)
    assert lat.step in pj.STEPS and lat.max_error <= tol and lat.n_checked >= 5 * (lat.sx.shape[0] - 1) * (lat.sx.shape[1] - 1)
    assert lat.sx.shape == wr.node_counts(T, lat.step) == pj.node_counts(T, lat.step)
    fn = lambda X, Y: pj.transform(pj.utm(31), pj.LONLAT, X, Y)
    if lat.step < 256:                                             # the largest step that meets tol
        assert pj._lattice_at(fn, T, SRC_1S, 2 * lat.step).max_error > tol
    # node (a, b) is the transform of the grid point (xmin + b K xres, ymax - a K yres)
    ex, ey = fn(T.xmin + (1 * lat.step) * T.xres, T.ymax - (1 * lat.step) * T.yres)
    assert lat.sx[1, 1] == float(ex) and lat.sy[1, 1] == float(ey)
    # the contract: ALL cell centres, interpolated by the section's formula, within tol source cells of the exact transform
    sx, sy = wr.source_points(lat, np.arange(T.nrow), np.arange(T.ncol))
    Y, X = np.meshgrid(T.ymax - (np.arange(T.nrow) + 0.5) * T.yres, T.xmin + (np.arange(T.ncol) + 0.5) * T.xres, indexing="ij")
    ex, ey = fn(X, Y)
    err = np.maximum(np.abs(sx - ex) / SRC_1S.xres, np.abs(sy - ey) / SRC_1S.yres)
    print(f"tol {tol}: step {lat.step}, measured {lat.max_error:.3g} at {lat.n_checked} points, over all cells {err.max():.3g}")
    assert np.isfinite(err).all() and err.max() <= tol


def test_lattice_steps_differ_with_the_tolerance_and_a_forced_step_is_held_to_it():
    T = _utm_target()
    steps = [pj.lattice(pj.LONLAT, pj.utm(31), T, SRC_1S, tol=t).step for t in (0.01, 0.001, 0.0001)]
    assert steps[0] > steps[1] > steps[2] >= 1, steps               # the error scales as K^2: a tenth of the tolerance, a third of the step
    assert pj.lattice(pj.LONLAT, pj.utm(31), T, SRC_1S, tol=0.01, step=4).step == 4
    with pytest.raises(ValueError, match="misses tol"):
        pj.lattice(pj.LONLAT, pj.utm(31), T, SRC_1S, tol=1e-4, step=256)
    with pytest.raises(ValueError, match="power of two"):
        pj.lattice(pj.LONLAT, pj.utm(31), T, SRC_1S, step=48)
    with pytest.raises(ValueError, match="misses tol"):             # step 1 fails: a transform that jumps inside every cell
        pj.lattice_from(lambda X, Y: (np.floor(X / 7.0) * 7.0, Y), T, SRC_1S, tol=0.01)


def test_lattice_of_an_affine_map_is_exact_to_rounding():
    """A bilinear lattice reproduces an affine map; what is left is rounding.  The source coordinates stay below 2^20 (ulp
    2.4e-10) and a value goes through fewer than ten rounded operations, so with unit source cells 1e-8 cells bounds it."""
    T = Geometry(1000.0, 9000.0, 7.0, 7.0, 333, 517)
    S = Geometry(0.0, 4000.0, 1.0, 1.0, 4000, 4000)
    c, s = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
    lat = pj.lattice_from(lambda X, Y: (0.9 * c * X - 0.9 * s * Y + 0.2 * Y + 3000.0, 0.9 * s * X + 0.9 * c * Y - 4000.0), T, S)
    assert lat.step == 256 and 0.0 <= lat.max_error < 1e-8 and lat.n_checked == 21 * 2 * 3


def test_a_lattice_made_by_hand_must_have_sx_and_sy_of_one_shape():
    with pytest.raises(ValueError, match="one shape"):
        pj.Lattice(4, np.zeros((3, 3)), np.zeros((2, 3))).device_arrays("cpu")
    with pytest.raises(ValueError, match="one shape"):
        pj.Lattice(4, np.zeros(9), np.zeros(9)).device_arrays("cpu")


def test_a_transform_without_a_value_gives_nan_nodes_not_an_error():
    T = _utm_target()
    wide = Geometry(T.xmin, T.ymax, 30000.0, 30000.0, 40, 120)      # 3 600 km east: past the domain
    lat = pj.lattice(pj.LONLAT, pj.utm(31), wide, SRC_1S, tol=1e9)
    assert np.isnan(lat.sx).any() and np.isfinite(lat.sx).any() and np.array_equal(np.isnan(lat.sx), np.isnan(lat.sy))
    assert lat.n_skipped > 0 and lat.n_checked + lat.n_skipped == 21 * (lat.sx.shape[0] - 1) * (lat.sx.shape[1] - 1)
    assert pj.lattice(pj.LONLAT, pj.utm(31), T, SRC_1S).n_skipped == 0


# ---------------------------------------------------------------- suggest_geometry

@pytest.mark.parametrize("res", [None, 30.0, 250.0])
def test_suggest_geometry_holds_the_boundary_and_snaps_its_origin(res):
    S = Geometry(-75.5, -11.75, 1.0 / 1200.0, 1.0 / 1200.0, 700, 900)
    crs = pj.utm(18, south=True)
    G = pj.suggest_geometry(S, pj.LONLAT, crs, res)
    assert G.xres == G.yres and (res is None or G.xres == res)
    def boundary(n):
        t = np.linspace(0.0, 1.0, n)
        xs, ys = S.xmin + t * (S.ncol * S.xres), S.ymax - t * (S.nrow * S.yres)
        bx = np.concatenate([xs, xs, np.full(n, xs[0]), np.full(n, xs[-1])])
        by = np.concatenate([np.full(n, ys[0]), np.full(n, ys[-1]), ys, ys])
        return pj.transform(pj.LONLAT, crs, bx, by)

    X, Y = boundary(41)                                            # the densified boundary it is made from: held exactly
    assert X.min() >= G.xmin and X.max() <= G.xmax and Y.min() >= G.ymin and Y.max() <= G.ymax
    X, Y = boundary(1001)                                          # between those points a side bulges by far less than a cell
    slack = 0.01 * G.xres
    assert X.min() >= G.xmin - slack and X.max() <= G.xmax + slack and Y.min() >= G.ymin - slack and Y.max() <= G.ymax + slack
    for q in (G.xmin / G.xres, G.ymax / G.yres):                   # a multiple of res, up to the rounding of the product
        assert abs(q - round(q)) <= 4 * np.spacing(abs(q))
    # no more than the snap and the last partial cell beyond the box
    assert X.min() - G.xmin < G.xres + slack and G.xmax - X.max() < G.xres + slack
    if res is None:                                                # GDAL's rule: the diagonal in cells is kept
        assert abs(math.hypot(G.nrow, G.ncol) - math.hypot(S.nrow, S.ncol)) < 3.0
    # and back: a UTM grid in lon/lat
    B = pj.suggest_geometry(G, crs, pj.LONLAT)
    assert B.xmin <= S.xmin and B.xmax >= S.xmax and B.ymin <= S.ymin and B.ymax >= S.ymax


# ---------------------------------------------------------------- refusals

class _Call:
    """mhs_warp_dev and mhs_warp on HOST arrays that are never read: every refusal comes before the first device call"""

    def __init__(self, fn="mhs_warp_dev"):
        self.fn = fn
        self.lib = _lib.load()
        self.src = _lib.Grid(0.0, 10.0, 1.0, 1.0, 10, 12)
        self.dst = _lib.Grid(500.0, 900.0, 2.0, 2.0, 9, 21)
        self.z = np.zeros((2, 10, 12), dtype=np.float32)
        self.stack = _lib.Stack(self.z.ctypes.data, 2, _lib.F32, 120, 12, NAN)
        self.out = np.zeros((2, 9, 21))
        self.nodes = np.zeros((2, 40, 40))

    def lattice(self, step=4, rows=None, cols=None, sx="default", sy="default"):
        rows = -(-9 // step) + 1 if rows is None and step > 0 else rows
        cols = -(-21 // step) + 1 if cols is None and step > 0 else cols
        return _lib.WarpLattice(step, rows or 0, cols or 0, self.nodes[0].ctypes.data if sx == "default" else sx,
                                self.nodes[1].ctypes.data if sy == "default" else sy)

    def __call__(self, src="default", stack="default", dst="default", window=(0, 9, 0, 21), lat="default", method=1, out="default",
                 out_dtype=_lib.F64, ld=21, plane_stride=189):
        g = C.byref(self.src) if src == "default" else src
        s = C.byref(self.stack) if stack == "default" else stack
        t = C.byref(self.dst) if dst == "default" else dst
        o = self.out.ctypes.data if out == "default" else out
        self._keep = self.lattice() if lat == "default" else lat
        la = C.byref(self._keep) if self._keep is not None else None
        if self.fn == "mhs_warp":
            rc = self.lib.mhs_warp(g, s, t, *window, la, method, o, out_dtype)
        else:
            rc = self.lib.mhs_warp_dev(g, s, t, *window, la, method, o, ld, plane_stride, out_dtype, None)
        return rc, self.lib.mhs_last_error().decode()


@pytest.mark.parametrize("fn", ["mhs_warp_dev", "mhs_warp"])
def test_refusals_come_before_any_device_call(fn):
    call = _Call(fn)

    def refused(needle, **kw):
        rc, msg = call(**kw)
        assert rc == _lib.ERR_INVALID and needle in msg and msg.startswith(fn + ":"), (kw, rc, msg)

    refused("NULL", src=None)
    refused("NULL", stack=None)
    refused("NULL", dst=None)
    refused("NULL", out=None)
    refused("NULL argument (lattice)", lat=None)
    refused("sx or sy", lat=call.lattice(sx=None))
    refused("sx or sy", lat=call.lattice(sy=None))
    refused("data is NULL", stack=C.byref(_lib.Stack(None, 2, _lib.F32, 120, 12, NAN)))
    refused("bad stack dtype", stack=C.byref(_lib.Stack(call.z.ctypes.data, 2, 7, 120, 12, NAN)))
    refused("strides", stack=C.byref(_lib.Stack(call.z.ctypes.data, 2, _lib.F32, 120, 11, NAN)))
    refused("source grid's cell size", src=C.byref(_lib.Grid(0.0, 10.0, 0.0, 1.0, 10, 12)))
    refused("target grid's cell size", dst=C.byref(_lib.Grid(500.0, 900.0, 2.0, NAN, 9, 21)))
    refused("target grid dimension", dst=C.byref(_lib.Grid(500.0, 900.0, 2.0, 2.0, 0, 21)))
    for step in (0, -1, -4, 3, 5, 6, 12, 48, 100, 1023, 1025, 2048, 4096, 1 << 20):
        refused("not a power of two in 1 .. 1024", lat=call.lattice(step=step, rows=4, cols=7))
    # the kernel reads nodes a + 1 and b + 1: a lattice one short, one long, or made for another step never reaches it
    want = {1: (10, 22), 2: (6, 12), 4: (4, 7), 8: (3, 4), 16: (2, 3), 32: (2, 2), 1024: (2, 2)}
    for step, (nr, nc) in want.items():
        for rows, cols in ((nr - 1, nc), (nr, nc - 1), (nr + 1, nc), (nr, nc + 1), (nc, nr), (0, 0), (-1, nc)):
            if (rows, cols) != (nr, nc):
                refused("node counts", lat=call.lattice(step=step, rows=rows, cols=cols))
        rc, msg = call(lat=call.lattice(step=step, rows=nr, cols=nc), window=(1, 1, 2, 2))
        assert rc in (_lib.OK, _lib.ERR_NODEVICE), (step, msg)
    for w in ((0, 10, 0, 21), (0, 9, 2, 22), (3, 2, 0, 21), (-1, 9, 0, 21), (0, 9, 5, 4)):
        refused("window outside the target", window=w)
    refused("unknown method", method=8)
    refused("unknown method", method=-1)
    for m in range(3, 8):
        refused("aggregate method", method=m)
    for bad in (_lib.I16, 5, -1):
        refused("out_dtype", out_dtype=bad)
    if fn == "mhs_warp_dev":
        refused("out_ld smaller", ld=20)
        refused("out_plane_stride", plane_stride=188)
    for m in range(3):                                             # every interpolating method passes the checks
        rc, msg = call(method=m, window=(1, 1, 2, 2))
        assert rc in (_lib.OK, _lib.ERR_NODEVICE), (m, msg)


def test_python_refuses_an_aggregate_method_by_name():
    with pytest.raises(ValueError, match="aggregate method 'mean'.*near, bilinear, cubic"):
        pj._method("mean")
    with pytest.raises(ValueError, match="near, bilinear, cubic"):
        pj._method("lanczos")
    assert [pj._method(m) for m in ("near", "bilinear", "cubic")] == [0, 1, 2]


# ---------------------------------------------------------------- the rule header, stand-alone

# Worked by hand on the 3 x 3 plane 1 2 3 / 4 5 6 / 7 8 10 of test_resample_host.py (unit cells, north-west corner (0, 3)).
# K = 1, a 2 x 2 target: 3 x 3 nodes, sx = 1.25, 2.25, 3.25 along b and sy = 1.75, 0.75, -0.25 along a.  Cell (0, 0): tu = tv = 0.5,
#   top = 0.5 * 1.25 + 0.5 * 2.25 = 1.75 = bot, sx = 0.5 * 1.75 + 0.5 * 1.75 = 1.75; sy = 0.5 * 1.75 + 0.5 * 0.75 = 1.25: the point
#   (1.75, 1.25) of the resample table: bilinear 6.0625, cubic falls back to it, near 5.  Cell (1, 1): (2.75, 0.25), in cell (2, 2) = 10;
#   bilinear fx = fy = 2.25: of the taps (2, 2), (2, 3), (3, 2), (3, 3) only the first is inside, 0.5625 * 10 / 0.5625 = 10.
# K = 4, a 6 x 5 target: ceil(6 / 4) + 1 = 3 by ceil(5 / 4) + 1 = 3 nodes, sx = 0.5, 2.5, 4.5 and sy = 3, 1, -1.  Column 1: tu = 1.5 / 4;
#   row 5: a = 1, tv = 1.5 / 4.  Cell (2, 1): tu = 0.375, tv = 0.625; sx = 0.625 * 0.5 + 0.375 * 2.5 = 1.25 in both rows;
#   sy = 0.375 * 3 + 0.625 * 1 = 1.75.  At (1.25, 1.75): fx = fy = 0.75, weights 0.0625, 0.1875, 0.1875, 0.5625 on 1, 2, 4, 5:
#   0.0625 + 0.375 + 0.75 + 2.8125 = 4.  Cell (5, 4), the last partial lattice cell (a = b = 1): tu = 0.125, tv = 0.375;
#   sx = 0.875 * 2.5 + 0.125 * 4.5 = 2.75, sy = 0.625 * 1 + 0.375 * -1 = 0.25: cell (2, 2) again.
# Node (2, 2) NaN: the cells of a = b = 1 (rows 4, 5 of column 4) are NA, cell (2, 1) keeps 4.  Node (0, 0) infinite: cell (2, 1) is NA,
#   cell (5, 4) keeps 10.  All 30 cells' points lie inside the source (sx in [0.75, 2.75], sy in [0.25, 2.75]).
HAND = {"k1_nodes": 33.0, "k1_ok_00": 1.0, "k1_sx_00": 1.75, "k1_sy_00": 1.25, "k1_bilinear_00": 6.0625, "k1_cubic_00": 6.0625, "k1_near_00": 5.0,
        "k1_near_11": 10.0, "k1_bilinear_11": 10.0, "k4_nodes": 33.0, "k4_tu_c1": 0.375, "k4_tv_r5": 0.375, "k4_node_r5": 1.0, "k4_sx_21": 1.25,
        "k4_sy_21": 1.75, "k4_bilinear_21": 4.0, "k4_last_sx": 2.75, "k4_last_sy": 0.25, "k4_last_near": 10.0, "k4_last_bilinear": 10.0,
        "nan_node_is_na": 1.0, "nan_node_elsewhere": 4.0, "inf_node_is_na": 1.0, "inf_node_elsewhere": 10.0, "nodes_8_by_4": 3.0,
        "nodes_9_by_4": 4.0, "nodes_1_by_1024": 2.0, "steps": 1.0, "k4_cells_with_a_value": 30.0}

S3 = Geometry(0.0, 3.0, 1.0, 1.0, 3, 3)
Z3 = np.array([[1.0, 2, 3], [4, 5, 6], [7, 8, 10]])


class _Lat:
    def __init__(self, T, K, xo, xs, yo, ys):
        nr, nc = wr.node_counts(T, K)
        self.step = K
        self.sx = np.tile(xo + np.arange(nc) * xs, (nr, 1))
        self.sy = np.tile((yo - np.arange(nr) * ys)[:, None], (1, nc))


def _restated():
    T1, T4 = Geometry(0.0, 2.0, 1.0, 1.0, 2, 2), Geometry(0.0, 6.0, 1.0, 1.0, 6, 5)
    l1, l4 = _Lat(T1, 1, 1.25, 1.0, 1.75, 1.0), _Lat(T4, 4, 0.5, 2.0, 3.0, 2.0)
    got = {"k1_nodes": l1.sx.shape[0] * 10.0 + l1.sx.shape[1], "k4_nodes": l4.sx.shape[0] * 10.0 + l4.sx.shape[1]}
    sx, sy = wr.source_points(l1, np.arange(2), np.arange(2))
    got.update(k1_ok_00=float(np.isfinite(sx[0, 0])), k1_sx_00=sx[0, 0], k1_sy_00=sy[0, 0])
    w1 = {m: wr.warp(Z3, NAN, S3, T1, l1, m) for m in ("near", "bilinear", "cubic")}
    got.update(k1_bilinear_00=w1["bilinear"][0, 0], k1_cubic_00=w1["cubic"][0, 0], k1_near_00=w1["near"][0, 0], k1_near_11=w1["near"][1, 1],
               k1_bilinear_11=w1["bilinear"][1, 1])
    sx, sy = wr.source_points(l4, np.arange(6), np.arange(5))
    w4 = {m: wr.warp(Z3, NAN, S3, T4, l4, m) for m in ("near", "bilinear", "cubic")}
    got.update(k4_tu_c1=(1 - (1 // 4) * 4 + 0.5) / 4.0, k4_tv_r5=(5 - (5 // 4) * 4 + 0.5) / 4.0, k4_node_r5=float(5 // 4), k4_sx_21=sx[2, 1], k4_sy_21=sy[2, 1],
               k4_bilinear_21=w4["bilinear"][2, 1], k4_last_sx=sx[5, 4], k4_last_sy=sy[5, 4], k4_last_near=w4["near"][5, 4],
               k4_last_bilinear=w4["bilinear"][5, 4], k4_cells_with_a_value=float((~np.isnan(w4["cubic"])).sum()))
    lnan = _Lat(T4, 4, 0.5, 2.0, 3.0, 2.0); lnan.sx[2, 2] = np.nan
    bn, nn = wr.warp(Z3, NAN, S3, T4, lnan, "bilinear"), wr.warp(Z3, NAN, S3, T4, lnan, "near")
    got.update(nan_node_is_na=float(np.isnan(bn[5, 4]) and np.isnan(nn[4, 4])), nan_node_elsewhere=bn[2, 1])
    linf = _Lat(T4, 4, 0.5, 2.0, 3.0, 2.0); linf.sy[0, 0] = np.inf
    got.update(inf_node_is_na=float(np.isnan(wr.warp(Z3, NAN, S3, T4, linf, "bilinear")[2, 1])), inf_node_elsewhere=wr.warp(Z3, NAN, S3, T4, linf, "near")[5, 4])
    G = lambda n: Geometry(0.0, 1.0, 1.0, 1.0, n, n)
    got.update(nodes_8_by_4=float(wr.node_counts(G(8), 4)[0]), nodes_9_by_4=float(wr.node_counts(G(9), 4)[0]), nodes_1_by_1024=float(wr.node_counts(G(1), 1024)[0]))
    got["steps"] = 1.0                                             # a property of the C header alone
    return {k: float(v) for k, v in got.items()}


def test_restatement_gives_the_hand_worked_table():
    got = _restated()
    assert got.keys() == HAND.keys()
    for name, want in HAND.items():
        assert got[name] == want, (name, got[name], want)


def test_rule_header_in_a_plain_cpp_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "warp_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "machisplin_amd", "csrc"),
           os.path.join(ROOT, "tests", "warp_check.cpp"), "-o", exe]
    pr = subprocess.run(cmd, capture_output=True, text=True)
    assert pr.returncode == 0, pr.stderr
    pr = subprocess.run([exe], capture_output=True, text=True)       # stand-alone: the sanitizer runtimes are linked into it
    assert pr.returncode == 0, pr.stdout + pr.stderr
    lines = pr.stdout.split("\n")
    assert lines[len(HAND)] == "OK"
    got = {ln.split()[0]: float(ln.split()[1]) for ln in lines[:len(HAND)]}
    assert got.keys() == HAND.keys()
    restated = _restated()
    for name, want in HAND.items():
        assert got[name] == float(want) == restated[name], (name, got[name], want, restated[name])


# ---------------------------------------------------------------- the coordinate system of a GeoTIFF

def test_epsg_round_trip_through_the_host_writer(tmp_path):
    lib = _lib.load()
    g = Geometry(500010.0, 8700030.0, 30.0, 30.0, 7, 9)
    data = np.arange(63, dtype=np.float32).reshape(7, 9)
    data[2, 3] = np.nan
    old, new, utm = (str(tmp_path / n) for n in ("old.tif", "new.tif", "utm.tif"))
    cg = g.c_struct()
    for comp in (1, 8):
        filled = np.where(np.isnan(data), np.float32(-9999.0), data)
        assert lib.mhs_tiff_write_f32_host(os.fsencode(old), C.byref(cg), filled.ctypes.data, -9999.0, comp) == _lib.OK
        mio.write_geotiff(new, g, data, nodata=-9999.0, compress=comp == 8)           # epsg = 4326 by default
        assert open(old, "rb").read() == open(new, "rb").read()                       # today's file, byte for byte
        assert mio.read_crs(new) == 4326
    mio.write_geotiff(utm, g, data, nodata=-9999.0, epsg=32718)
    assert mio.read_crs(utm) == 32718 and pj.from_epsg(mio.read_crs(utm)) == pj.utm(18, south=True)
    with Image.open(utm) as im:
        keys = tuple(im.tag_v2[34735])
        assert im.size == (9, 7)
    assert keys == (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32718)
    assert mio.geometry_of(utm) == g and np.array_equal(mio.read_host(utm), np.where(np.isnan(data), np.float32(-9999.0), data))
    with Image.open(new) as im:
        assert tuple(im.tag_v2[34735]) == (1, 1, 0, 3, 1024, 0, 1, 2, 1025, 0, 1, 1, 2048, 0, 1, 4326)
    for bad in (3857, 32600, 32661, 32761, 0, -1, 70000):
        with pytest.raises(_lib.MhsError, match="epsg must be 4326"):
            mio.write_geotiff(str(tmp_path / "bad.tif"), g, data, epsg=bad)
        assert not os.path.exists(str(tmp_path / "bad.tif"))
    # the device writer makes the same check before it asks for a device
    rc = lib.mhs_tiff_write_f32_dev_crs(os.fsencode(str(tmp_path / "bad.tif")), C.byref(cg), data.ctypes.data, 9, NAN, 8, None, 3857)
    assert rc == _lib.ERR_INVALID and "epsg must be 4326" in lib.mhs_last_error().decode()


def test_read_crs_of_a_file_without_a_geokey_directory(tmp_path):
    path = str(tmp_path / "plain.tif")
    Image.fromarray(np.zeros((4, 5), dtype=np.float32)).save(path)
    assert mio.read_crs(path) is None
    with pytest.raises(_lib.MhsError):
        mio.read_crs(str(tmp_path / "missing.tif"))
