"""CPU: the solar rules (include/machisplin_hip.h, section "solar").  The numpy restatement the GPU tests compare with
(tests/solar_ref.py) equals an independent scalar restatement bit for bit and gives the values that can be worked out by
hand (a flat plane, a wall south of a cell); the sun tables of machisplin_amd.terrain.sun_tables have the properties the rules
rely on; the entry points refuse bad arguments before they touch a device; and the rule header the kernel is built from
(csrc/solar_rule.h) gives the restatement's values in a plain C++ program compiled with gcc under AddressSanitizer + UBSan
and run stand-alone."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import solar_ref as sr
from machisplin_amd import _lib, synth, terrain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODATA = -32768.0


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _small_plane(shape, seed):
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(shape[0], dtype=np.float64), np.arange(shape[1], dtype=np.float64), indexing="ij")
    z = 500.0 + 9.0 * r - 4.0 * c + 30.0 * rng.standard_normal(shape)
    z[rng.integers(0, shape[0], 6), rng.integers(0, shape[1], 6)] = np.nan          # NA holes: NaN ...
    z[rng.integers(0, shape[0], 4), rng.integers(0, shape[1], 4)] = NODATA          # ... and the nodata value
    z[shape[0] // 2, shape[1] // 2] = 700.0                                         # a valid peak that casts shadows
    return z


def _two_tables(nrow, switch):
    """two tables at different latitudes, tab_row switching at row `switch`"""
    g = synth.grid(nrow, 8)
    a = terrain.sun_tables(g, lat=30.0, dx=30.0, dy=28.5, days=(355,), step_minutes=60)
    b = terrain.sun_tables(g, lat=60.0, dx=30.0, dy=28.5, days=(172, 355), step_minutes=60)
    start = np.concatenate([a.start, b.start[1:] + a.start[-1]])
    tab_row = (np.arange(nrow) >= switch).astype(np.int32)
    return terrain.SunTables(start, np.concatenate([a.entries, b.entries]), np.concatenate([a.omega, b.omega]), tab_row)


@pytest.mark.parametrize("search", [1, 2, 5])
@pytest.mark.parametrize("varying", [False, True], ids=["dx", "dx_row"])
def test_vectorised_restatement_equals_the_scalar_one_bit_for_bit(search, varying):
    shape = (12, 14)
    z = _small_plane(shape, 7 + search)
    rows = 30.0 * (1.0 - 0.3 * np.arange(shape[0]) / (shape[0] - 1)) if varying else None
    for tables in (terrain.sun_tables(synth.grid(*shape), lat=45.0, dx=30.0, dy=28.5), _two_tables(shape[0], 5)):
        kw = dict(dx=np.nan if varying else 30.0, dy=28.5, z_factor=0.3048, dx_row=rows)
        vec = sr.solar(z, NODATA, search, tables, **kw)
        sca = sr.solar_scalar(z, NODATA, search, tables, **kw)
        for name in sr.SOLAR:
            assert _same(vec[name], sca[name]), name
        na = np.isnan(sr.tr.to_double(z, NODATA))
        assert na.sum() >= 8 and np.array_equal(np.isnan(vec["svf"]), na) and np.array_equal(np.isnan(vec["sun_hours"]), na)
        assert np.isnan(vec["direct"][~na]).any() and not np.isnan(vec["direct"][1:-1, 1:-1]).all()
        assert vec["counts"]["lit"] > 0 and vec["counts"]["shadow"] > 0
    # horizon alone needs no tables
    assert _same(sr.solar(z, NODATA, search, None, **kw)["horizon"], vec["horizon"])


def test_flat_plane():
    tables = terrain.sun_tables(synth.grid(9, 11), lat=45.0, dx=30.0, dy=30.0)
    res = sr.solar(np.full((9, 11), 321.0), np.nan, 4, tables, 30.0, 30.0)
    E = tables.entries
    omega_sum = direct = hours = 0.0
    for j in range(16):
        omega_sum = omega_sum + tables.omega[j] / 1.0
    for i in range(len(E)):                            # c = uz on a level cell, nrm = 1
        direct = direct + E[i, 5] * E[i, 4]
        hours = hours + E[i, 6]
    assert (res["horizon"] == 0.0).all()
    assert (res["svf"] == omega_sum).all() and abs(omega_sum - 1.0) < 16e-15
    assert (res["sun_hours"] == hours).all() and hours > 0.0
    assert (res["direct"][1:-1, 1:-1] == direct).all() and np.isnan(res["direct"][0]).all() and np.isnan(res["direct"][:, -1]).all()
    assert res["counts"]["shadow"] == 0


def test_a_wall_south_of_a_cell_removes_exactly_the_entries_behind_it():
    """L = 1: the wall one row south is seen along S, SE and SW only, H = h / dy and h / sqrt(dy^2 + dx^2); the horizon in the
    sectors next to them is the linear blend.  The entries with tan_h <= Hs are counted from the table."""
    dx, dy, h = 30.0, 20.0, 9.0
    tables = terrain.sun_tables(synth.grid(9, 11), lat=45.0, days=(355, 80), dx=dx, dy=dy)
    z = np.zeros((9, 11))
    z[5] = h
    res = sr.solar(z, np.nan, 1, tables, dx, dy)
    H = np.zeros(16)
    H[8] = h / dy
    H[6] = H[10] = h / math.sqrt(dy * dy + dx * dx)
    assert np.array_equal(res["horizon"][:, 4, 5], H)
    hours, removed, kept = 0.0, 0, 0
    for j in range(16):
        for i in range(tables.start[j], tables.start[j + 1]):
            t, tan_h = tables.entries[i, 0], tables.entries[i, 1]
            if tan_h > H[j] + t * (H[(j + 1) & 15] - H[j]):
                hours, kept = hours + tables.entries[i, 6], kept + 1
            else:
                removed += 1
    assert removed > 0 and kept > 0 and removed + kept == len(tables.entries)
    assert res["sun_hours"][4, 5] == hours
    assert res["sun_hours"][4, 5] < res["sun_hours"][1, 5] == tables.entries[:, 6].sum()          # row 1 sees no wall
    # fewer entries reach the cell, and its 3 x 3 holds the wall: it tilts away from the winter sun
    assert res["direct"][4, 5] < res["direct"][1, 5]


def test_sun_tables_properties():
    g = synth.grid(40, 30)
    for lat, dx, dy in ((45.0, 30.0, 30.0), (-20.0, 25.0, 40.0), (70.0, 10.0, 31.0)):
        t = terrain.sun_tables(g, lat=lat, dx=dx, dy=dy)
        assert t.n_tab == 1 and t.tab_row is None and t.start[0] == 0 and t.start[-1] == len(t.entries) and (np.diff(t.start) >= 0).all()
        assert abs(t.omega.sum() - 1.0) <= 16e-15 and (t.omega > 0).all()
        phi = t.phi[0]
        want_phi = np.array([math.atan2(dc * dx, -dr * dy) for dr, dc in sr.DIRECTIONS]) % (2 * np.pi)
        assert np.abs(phi - want_phi).max() <= 1e-14 and (np.diff(phi) > 0).all()
        E = t.entries
        assert ((E[:, 0] >= 0) & (E[:, 0] <= 1)).all() and (E[:, 1] > 0).all() and (E[:, 5] >= 0).all() and (E[:, 6] > 0).all()
        assert np.abs(np.sqrt((E[:, 2:5] ** 2).sum(axis=1)) - 1.0).max() < 1e-12                 # unit vectors
        assert np.allclose(E[:, 1], E[:, 4] / np.hypot(E[:, 2], E[:, 3]), rtol=1e-14)
        # every entry's azimuth is rebuilt from (j, t) and phi_j
        for j in range(16):
            width = (phi[(j + 1) & 15] - phi[j]) % (2 * np.pi)
            for i in range(t.start[j], t.start[j + 1]):
                az = math.atan2(E[i, 2], E[i, 3]) % (2 * np.pi)
                diff = (phi[j] + E[i, 0] * width - az + np.pi) % (2 * np.pi) - np.pi
                assert abs(diff) <= 1e-12, (j, i, diff)
        assert (E[:, 5] <= terrain.SOLAR_CONSTANT * 0.5 / 4 + 1e-9).all()                         # w <= S0 dt / len(days)


@pytest.mark.parametrize("lat,day", [(0.0, 80), (60.0, 172)])
def test_sun_tables_day_length(lat, day):
    """the sum of d is the day length (24 / pi) acos(-tan(phi) tan(delta)) within 2 steps: a midpoint rule puts at most one
    step too many or too few at each end of the day"""
    step = 30
    t = terrain.sun_tables(synth.grid(5, 5), days=(day,), step_minutes=step, lat=lat, dx=30.0, dy=30.0)
    delta = math.radians(23.45) * math.sin(2 * math.pi * (284 + day) / 365)
    want = (24.0 / math.pi) * math.acos(-math.tan(math.radians(lat)) * math.tan(delta))
    got = t.entries[:, 6].sum()
    assert abs(got - want) <= 2 * step / 60.0, (got, want)
    # east is > 0 before noon: the sectors 0 .. 7 hold the morning.  Each half of the day has as many entries as the other.
    east = t.entries[:, 2]
    sector = np.repeat(np.arange(16), np.diff(t.start))
    assert (east[sector < 8] > 0).all() and (east[sector >= 8] < 0).all() and (sector < 8).sum() == (sector >= 8).sum() > 0


def test_sun_tables_lonlat_bands_and_projected_needs_lat():
    g = synth.grid(1000, 20)                          # 1000 rows of 1 / 1200 degree: 0.83 degrees from -5 southwards
    with pytest.raises(ValueError, match="lat"):
        terrain.sun_tables(g)
    t = terrain.sun_tables(g, lonlat=True, lat_step=0.25)
    lats = g.y_from_row(np.arange(g.nrow))
    assert t.n_tab == 4 and t.tab_row.dtype == np.int32 and t.tab_row.shape == (1000,)
    assert t.tab_row.min() == 0 and t.tab_row.max() == t.n_tab - 1
    order = np.argsort(lats)                          # ascending latitude: the table index does not increase
    assert (np.diff(t.tab_row[order]) <= 0).all()
    assert t.start.shape == (65,) and (np.diff(t.start) >= 0).all() and t.start[-1] == len(t.entries) and t.omega.shape == (64,)
    for b in range(4):                                # every row lies within half a step of its band's centre latitude
        centre = g.ymax - (b + 0.5) * 0.25
        assert np.abs(lats[t.tab_row == b] - centre).max() <= 0.125 + 1e-12
        one = terrain._sun_table(centre, g.xres * (np.pi / 180) * terrain.EARTH_RADIUS * math.cos(math.radians(centre)),
                                 g.yres * (np.pi / 180) * terrain.EARTH_RADIUS, (80, 172, 266, 355), 30, 0.7)
        assert np.array_equal(t.entries[t.start[16 * b]:t.start[16 * b + 16]], one[0]) and np.array_equal(t.omega[16 * b:16 * b + 16], one[2])


class _Call:
    """mhs_solar_dev and mhs_solar on HOST arrays that are never read: every refusal comes before the first device call"""

    def __init__(self):
        self.lib = _lib.load()
        self.grid = _lib.Grid(0.0, 10.0, 1.0, 1.0, 10, 12)
        self.z = np.zeros((10, 12), dtype=np.float32)
        self.stack = _lib.Stack(self.z.ctypes.data, 1, _lib.F32, 120, 12, float("nan"))
        self.out = np.zeros((19, 10, 12))
        self.tables = terrain.sun_tables(synth.grid(10, 12), lat=45.0)

    def __call__(self, fn, search=3, tables="default", mask=7, window=(0, 10, 0, 12), **edit):
        t = self.tables if tables == "default" else tables
        if edit:
            t = terrain.SunTables(t.start.copy(), t.entries.copy(), t.omega.copy(), np.zeros(10, dtype=np.int32))
            for k, (idx, v) in edit.items():
                getattr(t, k)[idx] = v
        ct = None if t is None else t.c_struct()
        u = _lib.TerrainUnits(30.0, None, 30.0, 1.0)
        tail = (self.out.ctypes.data, _lib.F64, 12, 120, None) if fn.endswith("_dev") else (self.out.ctypes.data, _lib.F64)
        rc = getattr(self.lib, fn)(C.byref(self.grid), C.byref(self.stack), 0, C.byref(u), search, None if ct is None else C.byref(ct),
                                   *window, mask, *tail)
        return rc, self.lib.mhs_last_error().decode()


@pytest.mark.parametrize("fn", ["mhs_solar_dev", "mhs_solar"])
def test_refusals_come_before_any_device_call(fn):
    call = _Call()
    limit = call.lib.mhs_terrain_max_radius()

    def refused(needle, **kw):
        rc, msg = call(fn, **kw)
        assert rc == _lib.ERR_INVALID and needle in msg and fn in msg, (kw, rc, msg)

    refused(f"search must be in 1 .. {limit}", search=0)
    refused(f"search must be in 1 .. {limit}", search=limit + 1)
    refused("products", mask=0)
    refused("products", mask=16)
    refused("window outside the grid", window=(0, 11, 0, 12))
    refused("tables is NULL", tables=None, mask=1)
    refused("tables is NULL", tables=None, mask=12)
    refused("entries[3].t", entries=((3, 0), 1.5))
    refused("entries[3].t", entries=((3, 0), -0.25))
    refused("entries[3].t", entries=((3, 0), float("nan")))
    refused("entries[2].tan_h", entries=((2, 1), 0.0))
    refused("entries[2].tan_h", entries=((2, 1), float("inf")))
    refused("entries[5].w", entries=((5, 5), -1.0))
    refused("entries[5].d", entries=((5, 6), -1.0))
    refused("entries[0].ux", entries=((0, 3), float("nan")))
    refused("start[4] decreases", start=(3, 5000))
    refused("start[0]", start=(0, 1))
    refused("omega[7]", omega=(7, -0.5))
    refused("tab_row[9]", tab_row=(9, 1))
    refused("tab_row[0]", tab_row=(0, -1))
    many = terrain.SunTables(np.concatenate([[0], np.full(16, 262145)]), np.zeros((1, 8)), np.full(16, 1 / 16))      # entries are never read
    refused("MHS_SOLAR_MAX_ENTRIES", tables=many)
    # good arguments pass every check: what is left is the device (present and initialised, or not)
    for kw in (dict(search=limit, window=(0, 0, 0, 0)), dict(tables=None, mask=8, window=(0, 0, 0, 0)), dict(tab_row=(9, 0), window=(2, 2, 0, 12))):
        rc, msg = call(fn, **kw)
        assert rc in (_lib.OK, _lib.ERR_NODEVICE), msg


def _check_inputs():
    """the plane and the tables of tests/solar_check.cpp, from the same formulas"""
    r, c = np.meshgrid(np.arange(50), np.arange(60), indexing="ij")
    z = ((r * 37 + c * 91 + r * c * 7) % 101).astype(np.float64) + 0.25 * r
    z[(r * 5 + c * 3 + 1) % 17 == 0] = np.nan
    entries, start, omega = [], [0], []
    for b in range(2):
        for j in range(16):
            for k in range(j % 3):
                entries.append([k / 4.0 + b / 8.0, 0.05 + 0.3 * j + b, (j - 8) / 16.0, (k - 1) / 4.0, 0.5, 1.0 + j, 0.5 + b, 0.0])
            start.append(len(entries))
            omega.append((1.0 + (j + b) % 4) / 40.0)
    rows = np.array([30.0 * (1.0 - 0.3 * i / 49) for i in range(50)])
    return z, terrain.SunTables(start, entries, omega, (np.arange(50) >= 20).astype(np.int32)), rows


def test_rule_header_in_a_plain_cpp_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "solar_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "machisplin_amd", "csrc"),
           os.path.join(ROOT, "tests", "solar_check.cpp"), "-o", exe]
    pr = subprocess.run(cmd, capture_output=True, text=True)
    assert pr.returncode == 0, pr.stderr
    pr = subprocess.run([exe], capture_output=True, text=True)       # stand-alone: the sanitizer runtimes are linked into it
    assert pr.returncode == 0, pr.stdout + pr.stderr
    lines = pr.stdout.split("\n")
    assert lines[-2] == "OK" and len(lines) == 4 * 9 * 19 + 2
    got = {ln.split()[0]: float(ln.split()[1]) for ln in lines[:-2]}
    z, tables, rows = _check_inputs()
    cells = ((0, 0), (0, 59), (49, 0), (49, 59), (0, 31), (49, 7), (23, 0), (24, 59), (25, 30))
    n_pos = 0
    for L in (1, 7, 44, 45):
        want = sr.solar(z, np.nan, L, tables, np.nan, 28.5, 0.3048, dx_row=rows)
        for r, c in cells:
            names = [(f"h{j}", want["horizon"][j, r, c]) for j in range(16)] + [(k, want[k][r, c]) for k in ("svf", "direct", "sun_hours")]
            for name, w in names:
                g = got[f"L{L}_r{r}_c{c}_{name}"]
                assert g == w or (np.isnan(g) and np.isnan(w)), (L, r, c, name, g, w)
                n_pos += w > 0
    assert n_pos > 4 * 9 * 4                            # more than the svf and sun hours alone: horizons are closed, beams arrive
