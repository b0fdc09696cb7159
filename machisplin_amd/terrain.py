"""Topographic covariates from an elevation model: slope, aspect, relief, geomorphons.

What the reference package's README sends its users to SAGA, GRASS and terra for ("Need help with the high-resolution
topography data?"): the covariate rasters derived from the DEM -- ``slope``, ``rel_alt`` / ``relative_elevation500m`` and
their kin -- and ``TWI``, with the filled surface, the D8 flow direction and the flow accumulation it is made from
(:func:`hydro`), or with the multiple-flow-direction accumulation SAGA makes it from (:func:`hydro_mfd`).
And the radiation covariates such a study makes with SAGA or GRASS's r.sun: the local horizon, the sky-view factor, potential
direct insolation and sun hours (:func:`solar`, with the sun's positions from :func:`sun_tables`).
include/machisplin_hip.h, sections "terrain", "solar", "hydrology" and "hydrology, multiple flow direction", states the rules.
All arithmetic on the cells runs in libmachisplin_hip.so (csrc/terrain.hip, csrc/hydro.hip); this module only marshals
arguments -- and, for a lon/lat raster, makes the rows' ground widths with numpy, because the library never calls cos (nor tan:
the slope floor of the wetness index is made here too; nor any trigonometry for the sun: the sun tables are made here).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .raster import RasterStack

VARS = ("dzdx", "dzdy", "slope_tan", "slope_deg", "eastness", "northness", "aspect_deg", "tpi", "tri", "roughness")
STATS = ("above_min", "below_max", "minus_mean")
FORMS = ("flat", "peak", "ridge", "shoulder", "spur", "slope", "hollow", "footslope", "valley", "pit")       # codes 1 .. 10
HYDRO = ("filled", "flowdir", "flowacc", "twi")                     # the planes of mhs_hydro_out, in its order
HYDRO_SPEC = {"twi": ("twi", False), "log_flowacc": ("flowacc", True)}      # covariates(): spec name -> (product, take its log)
HYDRO_MFD = ("filled", "flowacc", "twi")                            # the planes of mhs_hydro_mfd_out, in its order
HYDRO_MFD_SPEC = {"twi_mfd": ("twi", False), "log_flowacc_mfd": ("flowacc", True)}      # the same, made by hydro_mfd at its defaults
DIST_SPEC = {"dist_na": "na", "dist_le": "le", "dist_ge": "ge"}          # covariates(): spec name -> the predicate of proximity
STREAM_SPEC = {"dist_stream": "dist", "above_stream": "value"}          # covariates(): spec name -> the product of proximity
PATCH_DIST_SPEC = {"dist_na_edge": ("na", 0), "dist_na_min": ("na", 1), "dist_le_min": ("le", 2)}      # covariates(): spec name -> the predicate of patches, its arguments
BASIN_SPEC = {"basin_mean": "mean", "basin_minus_mean": "minus_mean", "basin_dev": "dev"}      # covariates(): spec name -> the plane of zonal
ZONE_SPEC = {"zone_mean": "mean", "zone_minus_mean": "minus_mean", "zone_dev": "dev"}      # covariates(): spec name -> the plane of zonal, zones from vector features
BASIN_QUANTILE_SPEC = {"basin_median": "q", "basin_frac_below": "frac_below"}      # covariates(): spec name -> the plane of zonal.quantile at p = 0.5
ZONE_QUANTILE_SPEC = {"zone_median": "q", "zone_frac_below": "frac_below"}         # ... zones from vector features
DIST_FEATURES = "dist_features"                                         # covariates(): the distance to vector features
CLASS_SPEC = {"class_frac": 4, "class_cover": 3}                         # covariates(): spec name -> the entry's length (classes.focal / classes.aggregate)
FLOW_SPEC = {"hand": "drop", "flowdist_stream": "dist"}                 # covariates(): spec name -> the product of flowpath
FLOW_OUTLET = "flowdist_outlet"                                         # covariates(): the path length to the root
FOCAL_SPEC = {"focal_mean": "mean", "focal_sd": "sd", "tpi_scale": "minus_mean", "dev": "dev"}      # covariates(): spec name -> the statistic of focal
SOLAR = ("svf", "direct", "sun_hours", "horizon")                   # the products of mhs_solar, in its order; horizon is 16 planes
# the sixteen ray directions of section "solar", clockwise from north: (rows south, columns east)
SOLAR_DIRECTIONS = ((-1, 0), (-2, 1), (-1, 1), (-1, 2), (0, 1), (1, 2), (1, 1), (2, 1),
                    (1, 0), (2, -1), (1, -1), (1, -2), (0, -1), (-1, -2), (-1, -1), (-2, -1))
SOLAR_CONSTANT = 1367.0                                             # W / m^2
GEOMORPHON_NA = -32768
EARTH_RADIUS = 6378137.0


def max_radius() -> int:
    """MHS_TERRAIN_MAX_RADIUS of the loaded library: the largest relief radius and geomorphon search length, in cells."""
    return int(_lib.load().mhs_terrain_max_radius())


def ground_units(geom, lonlat=False, z_factor=1.0, dx=None, dy=None, dx_row=None):
    """(dx, dx_row, dy, z_factor) of a raster: its resolution as it stands, or -- ``lonlat=True``, degrees -- metres on the
    sphere: dx_row = xres (pi / 180) 6378137 cos(latitude of the row's centre), dy = yres (pi / 180) 6378137.  ``dx``,
    ``dy`` and ``dx_row`` (one width per row of the whole grid) override."""
    if dx_row is not None:
        dx_row = np.ascontiguousarray(dx_row, dtype=np.float64)
        if dx_row.shape != (geom.nrow,):
            raise ValueError("dx_row must hold one width per row of the whole grid")
    elif lonlat and dx is None:
        lat = geom.y_from_row(np.arange(geom.nrow))
        dx_row = np.ascontiguousarray(geom.xres * (np.pi / 180.0) * EARTH_RADIUS * np.cos(lat * (np.pi / 180.0)))
    if dy is None:
        dy = geom.yres * (np.pi / 180.0) * EARTH_RADIUS if lonlat else geom.yres
    if dx is None:
        dx = geom.xres
    return float(dx), dx_row, float(dy), float(z_factor)


def _c_units(units):
    dx, dx_row, dy, zf = units
    return _lib.TerrainUnits(dx, dx_row.ctypes.data if dx_row is not None else None, dy, zf)


def _window(stack, window):
    g = stack.geom
    return tuple(int(x) for x in window) if window is not None else (0, g.nrow, 0, g.ncol)


def _mask(names, table, what):
    one = isinstance(names, str)
    names = (names,) if one else tuple(names)
    for n in names:
        if n not in table:
            raise ValueError(f"unknown {what} {n!r}: one of {', '.join(table)}")
    if not names or len(set(names)) != len(names):
        raise ValueError(f"give every {what} once")
    mask = 0
    for n in names:
        mask |= 1 << table.index(n)
    order = sorted(names, key=table.index)            # the library's plane order: ascending bit
    return one, names, mask, [order.index(n) for n in names]


def _planes(stack, shape, n, out_dtype, out):
    import torch
    if out_dtype not in (torch.float64, torch.float32):
        raise ValueError("out_dtype must be torch.float64 or torch.float32")
    if out is None:
        out = torch.empty((n,) + shape, dtype=out_dtype, device=stack.planes.device)
    if out.dtype != out_dtype or not out.is_cuda or out.dim() != 3 or out.stride(2) != 1 or tuple(out.shape) != (n,) + shape:
        raise ValueError("out must be a device tensor (n, rows, cols) of out_dtype with unit column stride")
    return out, (_lib.F64 if out_dtype == torch.float64 else _lib.F32)


def _stream(stack, stream):
    import torch
    return stream if stream is not None else torch.cuda.current_stream(stack.planes.device).cuda_stream


def terrain(stack: RasterStack, layer=0, v=("slope_deg",), lonlat=False, z_factor=1.0, window=None, out_dtype=None, out=None,
            stream=None, dx=None, dy=None, dx_row=None):
    """3 x 3 terrain variables of layer ``layer``: ``v`` names some of :data:`VARS`; every one of them comes out of one pass.
    A device tensor (len(v), rows, cols) in the order of ``v`` -- or (rows, cols) when ``v`` is a single name -- NaN where
    any of the nine cells is NA (so on the raster's outer ring).  aspect_deg is degrees clockwise from north, downslope,
    -1 at flat cells.  ``window`` = (r0, r1, c0, c1) gives those cells of the whole-grid result bit for bit.  ``out``: a
    pre-allocated tensor for the planes in the LIBRARY's order (ascending position in :data:`VARS`)."""
    import torch
    one, names, mask, order = _mask(v, VARS, "variable")
    r0, r1, c0, c1 = _window(stack, window)
    units = ground_units(stack.geom, lonlat, z_factor, dx, dy, dx_row)
    out, code = _planes(stack, (r1 - r0, c1 - c0), len(names), out_dtype or torch.float64, out)
    g, s, u = stack.geom.c_struct(), stack.c_struct(), _c_units(units)
    _lib.check(_lib.lib().mhs_terrain_dev(C.byref(g), C.byref(s), int(layer), C.byref(u), r0, r1, c0, c1, mask, out.data_ptr(), code,
                                          out.stride(1), out.stride(0), _stream(stack, stream)))
    if one:
        return out[0]
    return out if order == list(range(len(names))) else out[order]


def relief(stack: RasterStack, radius, stat="above_min", layer=0, z_factor=1.0, window=None, out_dtype=None, out=None, stream=None):
    """Relief of layer ``layer`` in a circular window of ``radius`` cells (1 .. :func:`max_radius`), NA cells and cells
    outside the raster skipped: ``stat`` names some of :data:`STATS` -- above_min is the bundled ``relative_elevation500m``
    (radius 17 at 30 m).  Shapes, ``window`` and ``out`` as in :func:`terrain`; NaN where the centre is NA."""
    import torch
    one, names, mask, order = _mask(stat, STATS, "statistic")
    r0, r1, c0, c1 = _window(stack, window)
    units = ground_units(stack.geom, False, z_factor)
    out, code = _planes(stack, (r1 - r0, c1 - c0), len(names), out_dtype or torch.float64, out)
    g, s, u = stack.geom.c_struct(), stack.c_struct(), _c_units(units)
    _lib.check(_lib.lib().mhs_relief_dev(C.byref(g), C.byref(s), int(layer), C.byref(u), int(radius), r0, r1, c0, c1, mask, out.data_ptr(),
                                         code, out.stride(1), out.stride(0), _stream(stack, stream)))
    if one:
        return out[0]
    return out if order == list(range(len(names))) else out[order]


def geomorphon(stack: RasterStack, search, flat_deg=1.0, layer=0, lonlat=False, z_factor=1.0, window=None, out=None, stream=None,
               dx=None, dy=None, dx_row=None):
    """Geomorphons (Jasiewicz & Stepinski 2013) of layer ``layer``: search length ``search`` cells (1 .. :func:`max_radius`),
    flatness threshold ``flat_deg`` degrees.  An int16 device tensor (rows, cols) of the codes 1 .. 10 (:data:`FORMS`),
    -32768 where the centre is NA or one of the eight rays has no valid step (so on the raster's outer ring)."""
    import torch
    r0, r1, c0, c1 = _window(stack, window)
    units = ground_units(stack.geom, lonlat, z_factor, dx, dy, dx_row)
    shape = (r1 - r0, c1 - c0)
    if out is None:
        out = torch.empty(shape, dtype=torch.int16, device=stack.planes.device)
    if out.dtype != torch.int16 or not out.is_cuda or out.dim() != 2 or out.stride(1) != 1 or tuple(out.shape) != shape:
        raise ValueError("out must be an int16 device tensor of the window's shape with unit column stride")
    g, s, u = stack.geom.c_struct(), stack.c_struct(), _c_units(units)
    _lib.check(_lib.lib().mhs_geomorphon_dev(C.byref(g), C.byref(s), int(layer), C.byref(u), int(search), float(flat_deg), r0, r1, c0, c1,
                                             out.data_ptr(), out.stride(0), _stream(stack, stream)))
    return out


class SunTables:
    """The sun tables of a solar call (struct mhs_sun_tables; include/machisplin_hip.h, section "solar", (c)), as host
    arrays: ``start`` int64 (n_tab * 16 + 1), ``entries`` float64 (n, 8) with the columns t, tan_h, ux, uy, uz, w, d, pad,
    ``omega`` float64 (n_tab * 16), ``tab_row`` int32 (one table index per row of the whole grid) or None.  ``phi``
    (n_tab, 16) holds the directions' azimuths the tables were made with, radians clockwise from north (None when the
    tables did not come from :func:`sun_tables`)."""

    def __init__(self, start, entries, omega, tab_row=None, phi=None):
        self.start = np.ascontiguousarray(start, dtype=np.int64)
        self.entries = np.ascontiguousarray(entries, dtype=np.float64).reshape(-1, 8)
        self.omega = np.ascontiguousarray(omega, dtype=np.float64).ravel()
        self.tab_row = None if tab_row is None else np.ascontiguousarray(tab_row, dtype=np.int32)
        self.phi = phi
        if self.omega.size % 16 or self.omega.size == 0 or self.start.shape != (self.omega.size + 1,):
            raise ValueError("omega must hold 16 weights per table and start one offset more")
        self.n_tab = self.omega.size // 16

    def c_struct(self):
        """the struct; it points into this object's arrays, which must outlive the call"""
        return _lib.SunTablesC(self.n_tab, self.start.ctypes.data, self.entries.ctypes.data, self.omega.ctypes.data,
                               None if self.tab_row is None else self.tab_row.ctypes.data)


def _sun_table(lat_deg, dx, dy, days, step_minutes, transmittance):
    """one table: (entries (n, 8) grouped by sector, the 17 offsets, omega (16), phi (16))"""
    two_pi = 2.0 * np.pi
    phi = np.array([np.arctan2(dc * dx, -dr * dy) for dr, dc in SOLAR_DIRECTIONS]) % two_pi       # ascending: the rays go clockwise
    width = (np.roll(phi, -1) - phi) % two_pi                       # of the sector from direction j to j + 1
    omega = 0.5 * ((np.roll(phi, -1) - np.roll(phi, 1)) % two_pi) / two_pi
    lat = np.deg2rad(float(lat_deg))
    dt = float(step_minutes) / 60.0
    hours = (np.arange(int(round(24.0 / dt))) + 0.5) * dt           # local solar time at the midpoints of the steps
    rows = []
    for n in days:
        delta = np.deg2rad(23.45) * np.sin(two_pi * (284.0 + float(n)) / 365.0)           # Cooper (1969)
        om = np.deg2rad(15.0) * (hours - 12.0)
        up = np.sin(lat) * np.sin(delta) + np.cos(lat) * np.cos(delta) * np.cos(om)
        north = np.cos(lat) * np.sin(delta) - np.sin(lat) * np.cos(delta) * np.cos(om)
        east = -np.cos(delta) * np.sin(om)
        k = up > 0.0
        up, north, east = up[k], north[k], east[k]
        az = np.arctan2(east, north) % two_pi
        j = np.clip(np.searchsorted(phi, az, side="right") - 1, 0, 15)
        t = np.clip(((az - phi[j]) % two_pi) / width[j], 0.0, 1.0)
        with np.errstate(divide="ignore"):
            tan_h = np.minimum(up / np.sqrt(east * east + north * north), 1e12)           # the sun in the zenith: finite
        w = SOLAR_CONSTANT * float(transmittance) ** (1.0 / up) * dt / len(days)
        d = np.full(up.shape, dt / len(days))
        rows.append(np.column_stack([t, tan_h, east, north, up, w, d, np.zeros(up.shape), j]))
    rows = np.concatenate(rows) if rows else np.zeros((0, 9))
    order = np.argsort(rows[:, 8], kind="stable")                   # by sector; within one, the days and times in order
    rows = rows[order]
    start = np.searchsorted(rows[:, 8], np.arange(17), side="left").astype(np.int64)
    return np.ascontiguousarray(rows[:, :8]), start, omega, phi


def sun_tables(geom, days=(80, 172, 266, 355), step_minutes=30, lonlat=False, lat=None, transmittance=0.7, lat_step=0.25, dx=None,
               dy=None) -> SunTables:
    """The sun tables :func:`solar` hands to the library, made here with numpy (the library never calls sin, cos or atan).
    For every day ``n`` of ``days`` (day of the year) and every step of ``step_minutes`` of local solar time, at the step's
    midpoint: declination delta = 23.45 deg sin(2 pi (284 + n) / 365) (Cooper), hour angle 15 deg (time - 12), and at
    latitude phi  up = sin phi sin delta + cos phi cos delta cos omega,  north = cos phi sin delta - sin phi cos delta
    cos omega,  east = -cos delta sin omega.  An entry where up > 0: tan_h = up / sqrt(east^2 + north^2), its azimuth
    atan2(east, north) placed between the two of the sixteen ray directions it lies between -- their azimuths
    atan2(dc dx, -dr dy) come from the table's own ``dx``, ``dy`` --, the energy weight w = 1367 transmittance ** (1 / up)
    dt / len(days) (the mean daily W h / m^2 on a surface facing the beam) and the time weight d = dt / len(days) (hours).
    omega_j = half the angle between direction j's two neighbours over 2 pi.

    A projected grid has one table at latitude ``lat`` degrees (required).  ``lonlat=True``: one table per band of
    ``lat_step`` degrees, counted from the grid's northern edge, made at the band's centre latitude with that latitude's
    ``dx``, and ``tab_row`` from the rows' latitudes.  The library's rays use each row's OWN dx (``dx_row``) while the
    sectors' azimuths come from the band's: that mismatch, at most half a ``lat_step`` of latitude, is this wrapper's
    approximation, not the library's."""
    days = tuple(days)
    if not days or not 0.0 < float(step_minutes) <= 720.0 or not 0.0 < float(transmittance) <= 1.0:
        raise ValueError("days must not be empty, step_minutes in (0, 720], transmittance in (0, 1]")
    if not lonlat:
        if lat is None:
            raise ValueError("a projected grid needs lat, the latitude in degrees the sun tables are made for")
        e, start, omega, phi = _sun_table(lat, dx if dx is not None else geom.xres, dy if dy is not None else geom.yres, days,
                                          step_minutes, transmittance)
        return SunTables(start, e, omega, None, phi[None])
    if not float(lat_step) > 0.0:
        raise ValueError("lat_step must be positive")
    lats = np.asarray(geom.y_from_row(np.arange(geom.nrow)), dtype=np.float64)
    tab_row = np.floor((geom.ymax - lats) / float(lat_step)).astype(np.int32)
    tab_row -= tab_row.min()
    n_tab = int(tab_row.max()) + 1
    first = int(np.floor((geom.ymax - lats[0]) / float(lat_step)))
    ents, starts, omegas, phis, n = [], [np.zeros(1, dtype=np.int64)], [], [], 0
    for b in range(n_tab):
        centre = geom.ymax - (first + b + 0.5) * float(lat_step) if lat is None else float(lat)
        bdx = dx if dx is not None else geom.xres * (np.pi / 180.0) * EARTH_RADIUS * np.cos(np.deg2rad(centre))
        bdy = dy if dy is not None else geom.yres * (np.pi / 180.0) * EARTH_RADIUS
        e, start, omega, phi = _sun_table(centre, bdx, bdy, days, step_minutes, transmittance)
        ents.append(e); starts.append(start[1:] + n); omegas.append(omega); phis.append(phi)
        n += len(e)
    return SunTables(np.concatenate(starts), np.concatenate(ents), np.concatenate(omegas), tab_row, np.stack(phis))


def solar(stack: RasterStack, search, products=("svf",), tables=None, layer=0, lonlat=False, lat=None, z_factor=1.0, window=None,
          out_dtype=None, out=None, stream=None, dx=None, dy=None, dx_row=None):
    """Solar covariates of layer ``layer`` (include/machisplin_hip.h, section "solar"): ``products`` names some of
    :data:`SOLAR` -- ``svf`` the sky-view factor, ``direct`` the potential direct insolation on the tilted cell, shadowed by
    the horizon (in the units of the tables' ``w``: mean daily W h / m^2 with :func:`sun_tables`), ``sun_hours`` (the units of
    ``d``: mean hours per day) and ``horizon``, the SIXTEEN planes of the horizon's tangent along the rays N, NNE, NE, ... NNW
    within ``search`` cells (1 .. :func:`max_radius`).  Shapes, ``window``, ``out`` and the plane order as in :func:`terrain`;
    ``horizon`` contributes 16 planes, so a single ``"horizon"`` returns (16, rows, cols).  ``tables``: a :class:`SunTables`;
    None makes them with :func:`sun_tables` at its defaults (``lonlat``, ``lat``, ``dx``, ``dy`` passed on) when a product
    needs them -- ``horizon`` alone needs none.  NaN where the centre is NA; ``direct`` also where any of the nine cells is."""
    import torch
    one, names, mask, _ = _mask(products, SOLAR, "product")
    r0, r1, c0, c1 = _window(stack, window)
    units = ground_units(stack.geom, lonlat, z_factor, dx, dy, dx_row)
    if tables is None and mask & 7:
        tables = sun_tables(stack.geom, lonlat=lonlat, lat=lat, dx=dx, dy=dy)
    width = {n: 16 if n == "horizon" else 1 for n in SOLAR}
    lib_order = sorted(names, key=SOLAR.index)
    first, n_planes = {}, 0
    for n in lib_order:
        first[n] = n_planes
        n_planes += width[n]
    out, code = _planes(stack, (r1 - r0, c1 - c0), n_planes, out_dtype or torch.float64, out)
    g, s, u = stack.geom.c_struct(), stack.c_struct(), _c_units(units)
    t = tables.c_struct() if tables is not None else None
    _lib.check(_lib.lib().mhs_solar_dev(C.byref(g), C.byref(s), int(layer), C.byref(u), int(search), C.byref(t) if t is not None else None,
                                        r0, r1, c0, c1, mask, out.data_ptr(), code, out.stride(1), out.stride(0), _stream(stack, stream)))
    if one:
        return out if names[0] == "horizon" else out[0]
    if list(names) == lib_order:
        return out
    return out[[first[n] + k for n in names for k in range(width[n])]]


class HydroResult(dict):
    """what :func:`hydro` returns for several products: the planes by name, and ``.info``"""
    info = None


def hydro(stack: RasterStack, layer=0, products=("twi",), lonlat=False, z_factor=1.0, min_slope_deg=0.1, max_passes=0, out_dtype=None,
          stream=None, dx=None, dy=None, dx_row=None):
    """Hydrology of layer ``layer`` (include/machisplin_hip.h, section "hydrology"): ``products`` names some of
    :data:`HYDRO` -- ``filled`` (the flat-filled surface), ``flowdir`` (int8: 0 .. 7 = E, SE, S, SW, W, NW, N, NE, -1 the
    water leaves, -2 NA), ``flowacc`` (cells draining through the cell, itself included) and ``twi`` =
    log(flowacc sqrt(dx dy) / max(slope_tan of the filled surface, tan(min_slope_deg))).  Always the whole plane: there is no
    window, flow accumulation is not local.  Returns ``(planes, info)``: a dict of device tensors by name (``.info`` too) --
    or the single tensor when ``products`` is one name -- and the call's counts, a dict of the fields of mhs_hydro_info.
    ``max_passes`` = 0 is the library's cap on the passes of a phase; MhsError (ERR_NUMERIC) when a phase reaches it.
    The call synchronises ``stream`` once per pass."""
    return _hydro(stack, layer, products, None, lonlat, z_factor, min_slope_deg, max_passes, out_dtype, stream, dx, dy, dx_row)


def hydro_mfd(stack: RasterStack, layer=0, products=("twi",), exponent=1.1, lonlat=False, z_factor=1.0, min_slope_deg=0.1, max_passes=0,
              out_dtype=None, stream=None, dx=None, dy=None, dx_row=None):
    """Hydrology of layer ``layer`` with MULTIPLE FLOW DIRECTION (include/machisplin_hip.h, section "hydrology, multiple
    flow direction"): a cell shares its water among all its lower neighbours in proportion to slope ** ``exponent`` (Freeman
    1991, Holmgren 1994; 1.1 is SAGA's default, 0 < exponent <= 64) where :func:`hydro` sends all of it to the steepest.
    ``products`` names some of :data:`HYDRO_MFD`: ``filled``, ``flowacc`` (a real number >= 1) and ``twi``.  Everything
    else, and what is returned, as in :func:`hydro`; the info's ``*_acc`` fields refer to the MFD accumulation."""
    return _hydro(stack, layer, products, float(exponent), lonlat, z_factor, min_slope_deg, max_passes, out_dtype, stream, dx, dy, dx_row)


def _hydro(stack, layer, products, exponent, lonlat, z_factor, min_slope_deg, max_passes, out_dtype, stream, dx, dy, dx_row):
    """:func:`hydro` (``exponent`` None: mhs_hydro_dev) and :func:`hydro_mfd` (mhs_hydro_mfd_dev)"""
    import torch
    table = HYDRO if exponent is None else HYDRO_MFD
    one = isinstance(products, str)
    names = (products,) if one else tuple(products)
    for n in names:
        if n not in table:
            raise ValueError(f"unknown product {n!r}: one of {', '.join(table)}")
    if not names or len(set(names)) != len(names):
        raise ValueError("give every product once")
    out_dtype = out_dtype or torch.float64
    if out_dtype not in (torch.float64, torch.float32):
        raise ValueError("out_dtype must be torch.float64 or torch.float32")
    if not min_slope_deg > 0.0:
        raise ValueError("min_slope_deg must be positive")
    g = stack.geom
    units = ground_units(g, lonlat, z_factor, dx, dy, dx_row)
    planes = {n: torch.empty((g.nrow, g.ncol), dtype=torch.int8 if n == "flowdir" else out_dtype, device=stack.planes.device) for n in names}
    ptrs = [planes[n].data_ptr() if n in planes else None for n in table]
    info = _lib.HydroInfo()
    cg, cs, cu = g.c_struct(), stack.c_struct(), _c_units(units)
    head = (C.byref(cg), C.byref(cs), int(layer), C.byref(cu), float(np.tan(np.deg2rad(min_slope_deg))), int(max_passes))
    tail = (_lib.F64 if out_dtype == torch.float64 else _lib.F32, g.ncol, _stream(stack, stream), C.byref(info))
    if exponent is None:
        out = _lib.HydroOut(*ptrs)
        _lib.check(_lib.lib().mhs_hydro_dev(*head, C.byref(out), *tail))
    else:
        out = _lib.HydroMfdOut(*ptrs)
        _lib.check(_lib.lib().mhs_hydro_mfd_dev(*head, exponent, C.byref(out), *tail))
    info = {k: getattr(info, k) for k, _ in _lib.HydroInfo._fields_}          # counts are ints, the phases' ms floats
    if one:
        return planes[names[0]], info
    res = HydroResult(planes)
    res.info = info
    return res, info


def _stream_layers(dem_stack, demf, flowacc, thresholds, spec):
    """the ("dist_stream", A) and ("above_stream", A) layers of :func:`covariates`: one proximity call per threshold A on a
    float64 stack of the D8 flow accumulation and the DEM (NA as NaN), which makes the distance and the DEM's value at the
    nearest stream cell; keyed (name, A)"""
    import torch
    from . import proximity as _prox
    pair = RasterStack(dem_stack.geom, torch.stack([flowacc.to(torch.float64), demf.to(torch.float64)]), float("nan"))
    out = {}
    for a in thresholds:
        want = tuple(dict.fromkeys(STREAM_SPEC[e[0]] for e in spec if len(e) == 2 and e[0] in STREAM_SPEC and float(e[1]) == a))
        got, _ = _prox.proximity(pair, 0, "ge", a, want, value_layer=1)
        if "dist" in got:
            out[("dist_stream", a)] = got["dist"].to(torch.float32)
        if "value" in got:
            out[("above_stream", a)] = (pair.planes[1] - got["value"]).to(torch.float32)
    return out


def _flow_layers(dem_stack, demf, flowdir, flowacc, thresholds, spec, layer):
    """the ("hand", A), ("flowdist_stream", A) and "flowdist_outlet" layers of :func:`covariates`: one flowpath call per threshold
    A on the stack :func:`_stream_layers` makes (the D8 flow accumulation and the DEM, float64, NA as NaN) follows every cell's
    own flow path to the first stream cell -- or to the root, where it meets none -- and one more call to the root; keyed
    (name, A) and by the name"""
    import torch
    from . import flowpath as _flow
    out = {}
    if thresholds:
        pair = RasterStack(dem_stack.geom, torch.stack([flowacc.to(torch.float64), demf.to(torch.float64)]), float("nan"))
    for a in thresholds:
        want = tuple(dict.fromkeys(FLOW_SPEC[e[0]] for e in spec if len(e) == 2 and e[0] in FLOW_SPEC and float(e[1]) == a))
        got, _ = _flow.flowpath(flowdir, pair, 0, "ge", a, want, value_layer=1, root_is_target=True)
        if "drop" in got:
            out[("hand", a)] = got["drop"].to(torch.float32)
        if "dist" in got:
            out[("flowdist_stream", a)] = got["dist"].to(torch.float32)
    if any(e[0] == FLOW_OUTLET for e in spec):
        out[FLOW_OUTLET] = _flow.flowpath(flowdir, dem_stack, layer, "outlet", None, "dist")[0].to(torch.float32)
    return out


def _quantile_planes(dem_stack, zones, n_zones, wanted, layer):
    """the planes ``wanted`` ("q": the zone's median, "frac_below") of one :func:`zonal.quantile` call at p = 0.5, float32"""
    import torch
    from . import zonal as _zonal
    _, planes, _ = _zonal.quantile(dem_stack, zones, (0.5,), layer, wanted, n_zones=n_zones, table=None, out_dtype=torch.float32)
    return {k: (v[0] if k == "q" else v) for k, v in planes.items()}


def _basin_layers(dem_stack, flowdir, wanted, layer, wanted_q=()):
    """the "basin_mean", "basin_minus_mean" and "basin_dev" layers of :func:`covariates`: the outlet labels of the D8 forest are
    the zones (a cell number per basin, -1 at NA cells), and one zonal call makes the planes; "basin_median" and
    "basin_frac_below" come from one :func:`zonal.quantile` call on the same labels; keyed by the spec's name"""
    import torch
    from . import flowpath as _flow
    from . import zonal as _zonal
    g = dem_stack.geom
    basin = _flow.flowpath(flowdir, dem_stack, layer, "outlet", None, "index")[0]
    out = {}
    if wanted:
        _, planes, _ = _zonal.zonal(dem_stack, basin, layer, stats=(), planes=wanted, n_zones=g.nrow * g.ncol, table=None, out_dtype=torch.float32)
        out.update({name: planes[plane] for name, plane in BASIN_SPEC.items() if plane in planes})
    if wanted_q:
        planes = _quantile_planes(dem_stack, basin, g.nrow * g.ncol, wanted_q, layer)
        out.update({name: planes[plane] for name, plane in BASIN_QUANTILE_SPEC.items() if plane in planes})
    return out


def _vector_layers(dem_stack, spec, layer):
    """the ("dist_features", feats) and ("zone_mean" | "zone_minus_mean" | "zone_dev", feats) layers of :func:`covariates`: the
    features are burned onto the DEM's grid (:func:`rasterize.rasterize`) -- with ``touches`` and as a value plane for the distance,
    which one proximity call then measures to; as an index plane for the zones, which one zonal call per distinct ``feats`` makes
    all three planes from; keyed (name, id(feats))"""
    import torch
    from . import proximity as _prox
    from . import rasterize as _rast
    from . import zonal as _zonal
    from .vector import Features
    g = dem_stack.geom
    dev = dem_stack.planes.device
    out = {}
    for feats in {id(e[1]): e[1] for e in spec if e[0] == DIST_FEATURES}.values():
        marked = Features(feats.kind, feats.coords, feats.part_offsets, feats.feature_offsets, np.zeros(feats.n_features))   # a NaN value would be no feature
        burned, _ = _rast.rasterize(marked, g, ("value",), touches=True, device=dev)
        out[(DIST_FEATURES, id(feats))] = _prox.proximity(RasterStack(g, burned["value"][None], float("nan")), 0, "valid", None, "dist",
                                                          out_dtype=torch.float32)[0]
    for feats in {id(e[1]): e[1] for e in spec if e[0] in ZONE_SPEC or e[0] in ZONE_QUANTILE_SPEC}.values():
        wanted = tuple(dict.fromkeys(ZONE_SPEC[e[0]] for e in spec if e[0] in ZONE_SPEC and e[1] is feats))
        wanted_q = tuple(dict.fromkeys(ZONE_QUANTILE_SPEC[e[0]] for e in spec if e[0] in ZONE_QUANTILE_SPEC and e[1] is feats))
        zones, _ = _rast.rasterize(feats, g, ("index",), device=dev)
        if wanted:
            _, planes, _ = _zonal.zonal(dem_stack, zones["index"], layer, stats=(), planes=wanted, n_zones=max(feats.n_features, 1), table=None,
                                        out_dtype=torch.float32)
            out.update({(name, id(feats)): planes[plane] for name, plane in ZONE_SPEC.items() if plane in planes})
        if wanted_q:                                  # the one rasterize call is shared; one quantile call per zone plane
            planes = _quantile_planes(dem_stack, zones["index"], max(feats.n_features, 1), wanted_q, layer)
            out.update({(name, id(feats)): planes[plane] for name, plane in ZONE_QUANTILE_SPEC.items() if plane in planes})
    return out


def _class_entry(e):
    """(categorical stack, layer, code[, radius]) of a "class_frac" / "class_cover" entry, checked"""
    if len(e) != CLASS_SPEC[e[0]]:
        raise ValueError(f"{e[0]!r} takes " + ("a categorical RasterStack (or (stack, layer)), a class code and the radius in cells" if e[0] == "class_frac"
                                               else "a categorical RasterStack (or (stack, layer)) and a class code"))
    cat, cat_layer = e[1] if isinstance(e[1], tuple) else (e[1], 0)
    if not isinstance(cat, RasterStack):
        raise ValueError(f"{e[0]!r}: the categorical raster must be a RasterStack or (RasterStack, layer)")
    if int(e[2]) != e[2] or not 0 <= int(e[2]) <= 65535:
        raise ValueError(f"{e[0]!r}: the class code must be an integer in 0 .. 65535, not {e[2]!r}")
    if e[0] == "class_frac" and int(e[3]) != e[3]:
        raise ValueError(f"'class_frac': the radius must be a whole number of cells, not {e[3]!r}")
    return (cat, int(cat_layer), int(e[2])) + ((int(e[3]),) if e[0] == "class_frac" else ())


def _class_layers(dem_stack, spec):
    """the ("class_frac", cat, code, R) and ("class_cover", cat, code) layers of :func:`covariates`: the share of class ``code`` of
    the categorical raster ``cat`` within R cells (:func:`classes.focal`; ``cat`` on the DEM's own grid) and in the DEM's cell
    (:func:`classes.aggregate`; ``cat`` on any grid of the same coordinate system).  Entries that share ``cat`` (and R) share one
    call, whose class list is their codes; keyed (name, id(cat), layer, code[, R])"""
    import torch
    from . import classes as _classes
    entries = [(e[0],) + _class_entry(e) for e in spec if e[0] in CLASS_SPEC]
    out = {}
    for name, cat, cat_layer, *rest in dict.fromkeys((n, c, l) + ((r[1],) if n == "class_frac" else ()) for n, c, l, *r in entries):
        codes = list(dict.fromkeys(en[3] for en in entries if en[:3] == (name, cat, cat_layer) and tuple(en[4:]) == tuple(rest)))
        if name == "class_frac":
            if cat.geom != dem_stack.geom:
                raise ValueError("'class_frac': the categorical raster must be on the DEM's own grid (classes.aggregate, or 'class_cover', brings another grid onto it)")
            planes, _ = _classes.focal(cat, rest[0], cat_layer, codes, ("frac",), codes, "square", out_dtype=torch.float32)
        else:
            planes, _ = _classes.aggregate(cat, dem_stack.geom, cat_layer, codes, ("frac",), codes, out_dtype=torch.float32)
        out.update({(name, id(cat), cat_layer, code) + tuple(rest): planes["frac"][j] for j, code in enumerate(codes)})
    return out


def covariates(dem_stack: RasterStack, spec=("slope_deg", ("above_min", 17)), layer=0, lonlat=False, z_factor=1.0, lat=None, sun=None):
    """A float32 covariate stack made from the DEM, ready for ``mltps``, ``mltps_predict`` and ``Mess``: the DEM first,
    then one layer per entry of ``spec`` --
      a name of :data:`VARS`                      that 3 x 3 variable (all of them in one pass)
      (a name of :data:`STATS`, radius)           that relief statistic in a window of ``radius`` cells
      ("geomorphon", search[, flat_deg])          the geomorphon code (1 .. 10)
      ("focal_mean" | "focal_sd" | "tpi_scale" | "dev", radius)
                                                  mean, sample sd, e - mean and (e - mean) / sd of the SQUARE window of ``radius``
                                                  cells, any radius up to max(nrow, ncol) (:func:`focal.focal`; one call per
                                                  distinct radius makes all of its layers)
      "twi"                                       the topographic wetness index (:func:`hydro`, its defaults)
      "log_flowacc"                               log of the flow accumulation, taken by torch on the float64 plane
      "twi_mfd", "log_flowacc_mfd"                the same two with multiple flow direction (:func:`hydro_mfd`, its defaults)
      ("svf" | "direct" | "sun_hours", search)    that solar product within ``search`` cells (:func:`solar`; one call per
                                                  distinct search length makes all of its layers) with the tables ``sun``, a
                                                  :class:`SunTables`, or those of :func:`sun_tables` at ``lat`` degrees
      "dist_na"                                   distance to the nearest NA cell of the DEM -- the sea, for a land-only DEM
                                                  (:func:`proximity.proximity`, in the geometry's cell width; square cells)
      ("dist_le" | "dist_ge", t)                  distance to the nearest cell whose elevation is <= t / >= t
      "dist_na_edge"                              distance to the nearest NA cell whose 8-connected patch of NA cells touches
                                                  the raster's edge (:func:`patches.sieve`, then proximity on that mask): the
                                                  sea without the voids and masked lakes inland
      ("dist_na_min", n)                          distance to the nearest NA cell in a patch of at least ``n`` NA cells
      ("dist_le_min", t, n)                       distance to the nearest cell <= t in a patch of at least ``n`` such cells
      ("dist_stream", A)                          distance to the nearest cell whose D8 ``flowacc`` is >= A (the one
                                                  :func:`hydro` call that makes ``twi`` / ``log_flowacc`` serves these too)
      ("above_stream", A)                         the DEM minus the DEM at that nearest stream cell, in elevation units:
                                                  Euclidean height above the nearest drainage
      ("hand", A)                                 the DEM minus the DEM at the first cell with D8 ``flowacc`` >= A on the cell's
                                                  OWN flow path (:func:`flowpath.flowpath`; the path's root where it meets
                                                  none): height above the nearest drainage along the flow
      ("flowdist_stream", A)                      the length of that path, in the geometry's cell width and height
      "flowdist_outlet"                           the length of the flow path to its root, where the water leaves the raster
                                                  (these three share the ``hydro`` call too, need metric cells and raise
                                                  ValueError for ``lonlat=True``; one flowpath call per distinct A)
      "basin_mean", "basin_minus_mean", "basin_dev"
                                                  the elevation against the cell's DRAINAGE BASIN, the cells that drain to the same
                                                  root of the D8 forest: the basin's mean elevation, the cell's elevation minus it,
                                                  and that over the basin's sample sd (the ``hydro`` call is shared again; one
                                                  :func:`flowpath.flowpath` call labels the basins, one :func:`zonal.zonal` call
                                                  makes all three)
      ("dist_features", feats)                    distance to the nearest cell that the :class:`vector.Features` ``feats`` -- a
                                                  digitised coastline, rivers, lakes, stations -- touch (:func:`rasterize.rasterize`
                                                  with ``touches=True``, then proximity; square cells)
      ("zone_mean" | "zone_minus_mean" | "zone_dev", feats)
                                                  the elevation against the polygon of ``feats`` that holds the cell's centre --
                                                  an administrative unit, a catchment: the zone's mean elevation, the cell's
                                                  elevation minus it, and that over the zone's sample sd (one rasterize call and
                                                  one :func:`zonal.zonal` call per distinct ``feats`` make all three; NaN outside)
      "basin_median", "basin_frac_below"          the MEDIAN elevation of the cell's drainage basin, and the share of the basin's cells
                                                  that lie below the cell -- its hypsometric position, a cold-air-pooling
                                                  covariate (the same ``hydro`` and ``flowpath`` calls as the basin layers above,
                                                  and one :func:`zonal.quantile` call)
      ("zone_median" | "zone_frac_below", feats)  the same two against the polygon of ``feats`` that holds the cell's centre (the
                                                  one rasterize call is shared with the zone layers above; one quantile call)
      ("class_frac", cat, code, R)                the share of class ``code`` among the valid cells of the categorical raster ``cat`` -- a
                                                  land-cover RasterStack on the DEM's own grid, or (stack, layer) -- within the square
                                                  window of R cells (:func:`classes.focal`'s ``frac``; NaN where ``cat`` is NA)
      ("class_cover", cat, code)                  the share of class ``code`` among the cells of ``cat`` -- on any grid of the same
                                                  coordinate system -- whose centre lies in the DEM's cell (:func:`classes.aggregate`'s
                                                  ``frac``; entries that share ``cat``, and R, share one call)
    NA cells are NaN (the stack's nodata is NaN).  The returned RasterStack carries the layers' names in ``.names``."""
    import torch
    spec = [(e,) if isinstance(e, str) else tuple(e) for e in spec]
    nr, nc = dem_stack.geom.nrow, dem_stack.geom.ncol
    planes = torch.empty((1 + len(spec), nr, nc), dtype=torch.float32, device=dem_stack.planes.device)
    dem = dem_stack.planes[layer]
    demf = dem.to(torch.float32)
    if not np.isnan(dem_stack.nodata):
        demf = torch.where(dem == dem_stack.nodata, torch.full_like(demf, float("nan")), demf)
    planes[0] = demf
    names = ["dem"]
    by_name = {}
    for e in spec:
        if e[0] in FLOW_SPEC or e[0] == FLOW_OUTLET:
            if len(e) != (2 if e[0] in FLOW_SPEC else 1):
                raise ValueError(f"{e[0]!r} takes " + ("one argument, the flow accumulation from which a cell is a stream" if e[0] in FLOW_SPEC
                                                       else "no argument"))
            if lonlat:
                raise ValueError(f"{e[0]!r} follows flow paths in metric cells: lonlat=True is out of scope (resample.resample onto a metric grid)")
        if (e[0] in BASIN_SPEC or e[0] in BASIN_QUANTILE_SPEC) and len(e) != 1:
            raise ValueError(f"{e[0]!r} takes no argument")
        if e[0] in ZONE_SPEC or e[0] in ZONE_QUANTILE_SPEC or e[0] == DIST_FEATURES:
            from .vector import Features
            if len(e) != 2 or not isinstance(e[1], Features):
                raise ValueError(f"{e[0]!r} takes one argument, a vector.Features in the DEM's coordinate system")
        if e[0] in STREAM_SPEC and len(e) != 2:
            raise ValueError(f"{e[0]!r} takes one argument, the flow accumulation from which a cell is a stream")
        if e[0] in DIST_SPEC and len(e) != (1 if e[0] == "dist_na" else 2):
            raise ValueError(f"{e[0]!r} takes {'no argument' if e[0] == 'dist_na' else 'one threshold'}")
        if e[0] in PATCH_DIST_SPEC:
            n_args = PATCH_DIST_SPEC[e[0]][1]
            if len(e) != 1 + n_args or (n_args and (int(e[-1]) != e[-1] or int(e[-1]) < 1)):
                raise ValueError(f"{e[0]!r} takes " + ("no argument", "one argument, the smallest patch in cells (a whole number >= 1)",
                                                       "a threshold and the smallest patch in cells (a whole number >= 1)")[n_args])
        if e[0] in CLASS_SPEC:
            _class_entry(e)
    stream_a = list(dict.fromkeys(float(e[1]) for e in spec if e[0] in STREAM_SPEC))
    flow_a = list(dict.fromkeys(float(e[1]) for e in spec if e[0] in FLOW_SPEC))
    basins = tuple(dict.fromkeys(BASIN_SPEC[e[0]] for e in spec if e[0] in BASIN_SPEC))
    basins_q = tuple(dict.fromkeys(BASIN_QUANTILE_SPEC[e[0]] for e in spec if e[0] in BASIN_QUANTILE_SPEC))
    flows = bool(flow_a) or any(e[0] == FLOW_OUTLET for e in spec) or bool(basins) or bool(basins_q)
    tv = [e[0] for e in spec if len(e) == 1 and e[0] not in HYDRO_SPEC and e[0] not in HYDRO_MFD_SPEC and e[0] not in DIST_SPEC and e[0] != FLOW_OUTLET
          and e[0] not in PATCH_DIST_SPEC and e[0] not in BASIN_SPEC and e[0] not in BASIN_QUANTILE_SPEC]
    if tv:
        got = terrain(dem_stack, layer, tuple(dict.fromkeys(tv)), lonlat, z_factor, out_dtype=torch.float32)
        by_name.update(zip(dict.fromkeys(tv), got))
    for table, call in ((HYDRO_SPEC, hydro), (HYDRO_MFD_SPEC, hydro_mfd)):
        hv = [e[0] for e in spec if len(e) == 1 and e[0] in table]
        extra = ("flowacc",) if (stream_a or flow_a) and call is hydro else ()          # the streams are cut from the D8 accumulation
        if flows and call is hydro:
            extra += ("flowdir",)                                                       # ... and the paths follow the D8 directions
        if hv or extra:                           # one hydrology call of a route makes all of its layers
            hp, _ = call(dem_stack, layer, tuple(dict.fromkeys([table[n][0] for n in hv] + list(extra))), lonlat=lonlat, z_factor=z_factor)
            if stream_a and call is hydro:
                by_name.update(_stream_layers(dem_stack, demf, hp["flowacc"], stream_a, spec))
            if flows and call is hydro:
                by_name.update(_flow_layers(dem_stack, demf, hp["flowdir"], hp.get("flowacc"), flow_a, spec, layer))
            if (basins or basins_q) and call is hydro:
                by_name.update(_basin_layers(dem_stack, hp["flowdir"], basins, layer, basins_q))
            for n in hv:
                product, log = table[n]
                by_name[n] = (torch.log(hp[product]) if log else hp[product]).to(torch.float32)
    sun_names = SOLAR[:3]
    for L in dict.fromkeys(int(e[1]) for e in spec if len(e) > 1 and e[0] in sun_names):
        sv = tuple(dict.fromkeys(e[0] for e in spec if len(e) > 1 and e[0] in sun_names and int(e[1]) == L))
        got = solar(dem_stack, L, sv, sun, layer, lonlat, lat, z_factor, out_dtype=torch.float32)
        by_name.update({(n, L): p for n, p in zip(sv, got)})
    for e in spec:
        if e[0] in FOCAL_SPEC and len(e) != 2:
            raise ValueError(f"{e[0]!r} takes one argument, the radius in cells")
    if any(e[0] in FOCAL_SPEC for e in spec):
        from . import focal as _focal
        off = _focal.default_offset(dem_stack, layer)
        for R in dict.fromkeys(int(e[1]) for e in spec if e[0] in FOCAL_SPEC):
            fv = tuple(dict.fromkeys(FOCAL_SPEC[e[0]] for e in spec if e[0] in FOCAL_SPEC and int(e[1]) == R))
            got = _focal.focal(dem_stack, R, fv, layer, "square", out_dtype=torch.float32, offset=off)
            by_name.update({(n, R): p for n, p in zip(fv, got)})
    from . import proximity as _prox
    for e in dict.fromkeys(e for e in spec if e[0] in DIST_SPEC):
        by_name[e] = _prox.proximity(dem_stack, layer, DIST_SPEC[e[0]], float(e[1]) if len(e) > 1 else None, "dist", out_dtype=torch.float32)[0]
    patch_specs = list(dict.fromkeys(e for e in spec if e[0] in PATCH_DIST_SPEC))
    if patch_specs:
        from . import patches as _patches
        g = dem_stack.geom
        if abs(g.xres - g.yres) > 1e-9 * max(abs(g.xres), abs(g.yres)):
            raise ValueError(f"{patch_specs[0][0]!r}: the cells are not square (xres {g.xres}, yres {g.yres}); bring the raster onto a square "
                             "grid with resample.resample")
        for e in patch_specs:
            where, n_args = PATCH_DIST_SPEC[e[0]]
            keep = _patches.sieve(dem_stack, layer, where, float(e[1]) if n_args == 2 else None, 8, min_size=int(e[-1]) if n_args else 1,
                                  edge="any" if n_args else "touching")
            by_name[e] = _prox.proximity(keep, products="dist", unit=g.xres, out_dtype=torch.float32)[0]
    if any(e[0] in ZONE_SPEC or e[0] in ZONE_QUANTILE_SPEC or e[0] == DIST_FEATURES for e in spec):
        by_name.update(_vector_layers(dem_stack, spec, layer))
    if any(e[0] in CLASS_SPEC for e in spec):
        by_name.update(_class_layers(dem_stack, spec))
    for k, e in enumerate(spec):
        if e[0] in CLASS_SPEC:
            cat, cat_layer, *rest = _class_entry(e)
            planes[1 + k] = by_name[(e[0], id(cat), cat_layer) + tuple(rest)]
            names.append(e[0] + "_".join(str(v) for v in rest))
        elif e[0] in ZONE_SPEC or e[0] in ZONE_QUANTILE_SPEC or e[0] == DIST_FEATURES:
            planes[1 + k] = by_name[(e[0], id(e[1]))]
            names.append(e[0])
        elif e[0] in PATCH_DIST_SPEC:
            planes[1 + k] = by_name[e]
            names.append(e[0] if len(e) == 1 else f"{e[0]}{int(e[1])}" if len(e) == 2 else f"dist_le{float(e[1]):g}_min{int(e[2])}")
        elif e[0] in DIST_SPEC or e[0] in STREAM_SPEC or e[0] in FLOW_SPEC:
            planes[1 + k] = by_name[e if e[0] in DIST_SPEC else (e[0], float(e[1]))]
            names.append(e[0] + (f"{float(e[1]):g}" if len(e) > 1 else ""))
        elif len(e) > 1 and e[0] in sun_names:
            planes[1 + k] = by_name[(e[0], int(e[1]))]
            names.append(f"{e[0]}{int(e[1])}")
        elif e[0] in FOCAL_SPEC:
            planes[1 + k] = by_name[(FOCAL_SPEC[e[0]], int(e[1]))]
            names.append(f"{e[0]}{int(e[1])}")
        elif len(e) == 1:
            planes[1 + k] = by_name[e[0]]
            names.append(e[0])
        elif e[0] == "geomorphon":
            f = geomorphon(dem_stack, e[1], e[2] if len(e) > 2 else 1.0, layer, lonlat, z_factor)
            planes[1 + k] = torch.where(f == GEOMORPHON_NA, torch.full((), float("nan"), device=f.device), f.to(torch.float32))
            names.append(f"geomorphon{int(e[1])}")
        else:
            planes[1 + k] = relief(dem_stack, e[1], e[0], layer, z_factor, out_dtype=torch.float32)
            names.append(f"{e[0]}{int(e[1])}")
    out = RasterStack(dem_stack.geom, planes, float("nan"))
    out.names = names
    return out
