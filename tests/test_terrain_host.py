"""CPU: the terrain rules (include/machisplin_hip.h, section "terrain").  The numpy restatement the GPU tests compare with
(tests/terrain_ref.py) is itself checked against hand-computed values; every entry point refuses bad arguments with
MHS_ERR_INVALID before it touches a device; and the rule header the kernels are built from (csrc/terrain_rule.h) gives the same
table in a plain C++ program compiled with gcc under AddressSanitizer + UBSan and run stand-alone."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import terrain_ref as tr
from machisplin_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# z = 1 2 3 / 4 5 6 / 7 8 10, dx = 2, dy = 4, z_factor = 1, worked by hand:
#   dzdx = ((3 + 12 + 10) - (1 + 8 + 7)) / 16 = 9 / 16, dzdy = ((7 + 16 + 10) - (1 + 4 + 3)) / 32 = 25 / 32
#   tpi = 5 - 41 / 8, tri = (4 + 3 + 2 + 1 + 1 + 2 + 3 + 5) / 8, roughness = 10 - 1
_ST = math.sqrt(0.5625 * 0.5625 + 0.78125 * 0.78125)
HAND = {"hand_dzdx": 0.5625, "hand_dzdy": 0.78125, "hand_slope_tan": _ST, "hand_slope_deg": math.degrees(math.atan(_ST)),
        "hand_eastness": -0.5625 / _ST, "hand_northness": 0.78125 / _ST,
        "hand_aspect_deg": math.degrees(math.atan2(-0.5625, 0.78125)) + 360.0, "hand_tpi": -0.125, "hand_tri": 2.625, "hand_roughness": 9.0,
        "east_aspect_deg": 270.0, "east_eastness": -1.0, "east_northness": 0.0, "south_aspect_deg": 0.0,
        "flat_aspect_deg": -1.0, "flat_eastness": 0.0, "flat_northness": 0.0,
        # z = 5 r + c on 5 x 5, NA at (2, 3), R = 1.  Centre (2, 2): 7, 11, 12, 17 -> min 7, max 17, mean 47 / 4;
        # corner (0, 0): 0, 1, 5 -> min 0, max 5, mean 2
        "relief_centre_above_min": 5.0, "relief_centre_below_max": 5.0, "relief_centre_minus_mean": 0.25,
        "relief_corner_above_min": 0.0, "relief_corner_below_max": 5.0, "relief_corner_minus_mean": -2.0,
        "form_cone": tr.PK, "form_pit": tr.PT, "form_inclined": tr.SL, "form_constant": tr.FL, "form_roof": tr.RI, "form_vee": tr.VL,
        "form_border": tr.GEOMORPHON_NA}
ANGLES = ("hand_slope_deg", "hand_aspect_deg")          # through atan / atan2: equal to 1e-12 degrees, everything else exactly


def _close(name, got, want):
    return abs(got - want) <= 1e-12 if name in ANGLES else got == want


def test_restatement_3x3_gives_the_hand_computed_values():
    z = np.array([[1.0, 2, 3], [4, 5, 6], [7, 8, 10]])
    t = tr.terrain(z, np.nan, 2.0, 4.0)
    for k in tr.VARS:
        assert t[k].shape == (3, 3) and np.isnan(np.delete(t[k].ravel(), 4)).all()      # the outer ring is NA
        assert _close("hand_" + k, t[k][1, 1], HAND["hand_" + k]), k
    # z_factor multiplies every elevation difference, dx_row replaces dx row by row
    t2 = tr.terrain(z, np.nan, 99.0, 4.0, z_factor=3.0, dx_row=[7.0, 2.0, 5.0])
    assert t2["dzdx"][1, 1] == 3 * 0.5625 and t2["dzdy"][1, 1] == 3 * 0.78125 and t2["tpi"][1, 1] == -0.375 and t2["roughness"][1, 1] == 27.0
    # an NA (the nodata value) among the nine makes the cell NA
    zi = z.astype(np.int16); zi[0, 2] = -32768
    assert all(np.isnan(v).all() for v in tr.terrain(zi, -32768.0, 2.0, 4.0).values())


def test_restatement_aspect_conventions():
    cols, rows = np.meshgrid(np.arange(5.0), np.arange(5.0))
    east = tr.terrain(3.0 * cols, np.nan, 1.0, 1.0)
    assert east["aspect_deg"][2, 2] == 270.0 and east["eastness"][2, 2] == -1.0 and east["northness"][2, 2] == 0.0
    south = tr.terrain(3.0 * rows, np.nan, 1.0, 1.0)
    assert south["aspect_deg"][2, 2] == 0.0 and south["northness"][2, 2] == 1.0
    flat = tr.terrain(np.full((5, 5), 7.0), np.nan, 1.0, 1.0)
    assert flat["aspect_deg"][2, 2] == -1.0 and flat["eastness"][2, 2] == 0.0 and flat["northness"][2, 2] == 0.0 and flat["slope_deg"][2, 2] == 0.0


def _shapes():
    r, c = np.meshgrid(np.arange(21.0), np.arange(21.0), indexing="ij")
    d = np.sqrt((r - 10) ** 2 + (c - 10) ** 2)
    return {"cone": -d, "pit": d, "inclined": c, "constant": np.full((21, 21), 3.0), "roof": -np.abs(c - 10), "vee": np.abs(c - 10)}


def test_restatement_geomorphon_forms_of_six_shapes():
    for name, z in _shapes().items():
        forms, margin = tr.geomorphon(z, np.nan, 5, 1.0, 1.0, 1.0)
        assert forms.dtype == np.int16 and forms[10, 10] == HAND["form_" + name], name
        assert (forms[0, :] == tr.GEOMORPHON_NA).all() and (forms[:, -1] == tr.GEOMORPHON_NA).all()        # a ray with no step
        assert (forms[1:-1, 1:-1] != tr.GEOMORPHON_NA).all()
    # an NA stops a ray (the cells beyond are not seen) and an NA centre is NA
    z = _shapes()["pit"].copy()
    z[10, 12:] = -100.0                       # a cliff east of the centre ...
    assert tr.geomorphon(z, np.nan, 5, 1.0, 1.0, 1.0)[0][10, 10] != tr.PT
    z[10, 12] = np.nan                        # ... hidden behind an NA: the east ray ends at (10, 11)
    forms, _ = tr.geomorphon(z, np.nan, 5, 1.0, 1.0, 1.0)
    assert forms[10, 10] == tr.PT and forms[10, 12] == tr.GEOMORPHON_NA and forms[10, 11] == tr.GEOMORPHON_NA
    # flat_deg = 0: exact ties D == 0 are flat
    assert (tr.geomorphon(np.full((7, 7), 3.0), np.nan, 2, 0.0, 1.0, 1.0)[0][1:-1, 1:-1] == tr.FL).all()


def test_restatement_relief_with_one_na():
    z = 5.0 * np.arange(5.0)[:, None] + np.arange(5.0)[None, :]
    z[2, 3] = np.nan
    rel = tr.relief(z, np.nan, 1)
    for where, (r, c) in (("centre", (2, 2)), ("corner", (0, 0))):
        for s in tr.STATS:
            assert rel[s][r, c] == HAND[f"relief_{where}_{s}"], (where, s)
    assert all(np.isnan(rel[s][2, 3]) and np.isnan(rel[s]).sum() == 1 for s in tr.STATS)       # an NA centre, and only that
    # radius 2 has 13 offsets: 0 +- 2 on the axes, the 3 x 3 block
    assert tr.relief(np.arange(25.0).reshape(5, 5), np.nan, 2)["minus_mean"][2, 2] == 0.0


class _Call:
    """the six entry points on HOST arrays that are never read: every refusal comes before the first device call.  Where an
    earlier test of the session has initialised a device, a call with good arguments does run: a _dev entry then gets
    device planes (it would take the host arrays' addresses for device memory), a host entry keeps the host arrays."""

    def __init__(self, fn):
        self.lib = _lib.load()
        self.grid = _lib.Grid(0.0, 10.0, 1.0, 1.0, 10, 12)
        self.z = np.zeros((2, 10, 12), dtype=np.float32)
        self.out = np.zeros((10, 10, 12))
        zp, self.op = self.z.ctypes.data, self.out.ctypes.data
        if fn.endswith("_dev") and _lib._inited_device is not None:
            import torch
            dev = torch.device("cuda", _lib._inited_device)
            self.zd = torch.zeros((2, 10, 12), dtype=torch.float32, device=dev)
            self.od = torch.zeros((10, 10, 12), dtype=torch.float64, device=dev)
            zp, self.op = self.zd.data_ptr(), self.od.data_ptr()
        self.stack = _lib.Stack(zp, 2, _lib.F32, 120, 12, float("nan"))
        self.units = dict(dx=30.0, dx_row=None, dy=30.0, z_factor=1.0)

    def __call__(self, fn, grid=None, stack=None, layer=0, window=(0, 10, 0, 12), mask=1, out="default", out_dtype=_lib.F64, ld=12,
                 plane_stride=120, radius=3, flat_deg=1.0, units="default", **unit_kw):
        u = dict(self.units, **unit_kw)
        rows = None if u["dx_row"] is None else np.ascontiguousarray(u["dx_row"], dtype=np.float64)
        cu = _lib.TerrainUnits(u["dx"], None if rows is None else rows.ctypes.data, u["dy"], u["z_factor"])
        g = C.byref(grid or self.grid)
        s = C.byref(stack or self.stack)
        up = None if units is None else C.byref(cu)
        o = self.op if out == "default" else out
        dev = fn.endswith("_dev")
        tail = (o, out_dtype, ld, plane_stride, None) if dev else (o, out_dtype)
        f = getattr(self.lib, fn)
        if fn.startswith("mhs_terrain"):
            rc = f(g, s, layer, up, *window, mask, *tail)
        elif fn.startswith("mhs_relief"):
            rc = f(g, s, layer, up, radius, *window, mask, *tail)
        else:
            rc = f(g, s, layer, up, radius, flat_deg, *window, o, *((ld, None) if dev else ()))
        return rc, self.lib.mhs_last_error().decode()


ALL = ("mhs_terrain_dev", "mhs_relief_dev", "mhs_geomorphon_dev", "mhs_terrain", "mhs_relief", "mhs_geomorphon")


@pytest.mark.parametrize("fn", ALL)
def test_refusals_come_before_any_device_call(fn):
    call = _Call(fn)
    kind = fn.replace("_dev", "")

    def refused(needle, **kw):
        rc, msg = call(fn, **kw)
        assert rc == _lib.ERR_INVALID and needle in msg and fn in msg, (kw, rc, msg)

    refused("window outside the grid", window=(0, 11, 0, 12))
    refused("window outside the grid", window=(0, 10, 5, 13))
    refused("window outside the grid", window=(4, 3, 0, 12))
    refused("window outside the grid", window=(-1, 3, 0, 12))
    refused("layer 2", layer=2)
    refused("layer -1", layer=-1)
    refused("units", units=None)
    refused("dem data is NULL", stack=_lib.Stack(None, 2, _lib.F32, 120, 12, float("nan")))
    refused("bad dem dtype", stack=_lib.Stack(call.z.ctypes.data, 2, 7, 120, 12, float("nan")))
    refused("dem strides", stack=_lib.Stack(call.z.ctypes.data, 2, _lib.F32, 120, 11, float("nan")))
    refused("bad grid geometry", grid=_lib.Grid(0.0, 10.0, 1.0, 1.0, 0, 12))
    refused("out is NULL", out=None)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused("z_factor", z_factor=bad)
    if kind != "mhs_relief":
        for bad in (0.0, -30.0, float("nan"), float("inf")):
            refused("dy must be", dy=bad)
            refused("dx must be", dx=bad)
            rows = np.full(10, 30.0); rows[7] = bad
            refused("dx_row[7]", dx_row=rows, dx=float("nan"))          # dx is not looked at when dx_row is given
    else:
        rc, msg = call(fn, dx=float("nan"), dy=-1.0)                    # relief has no horizontal distance in it
        assert rc in (_lib.OK, _lib.ERR_NODEVICE), msg
    if kind != "mhs_terrain":
        what = "radius" if kind == "mhs_relief" else "search"
        limit = call.lib.mhs_terrain_max_radius()
        assert limit >= 32
        for bad in (0, -1, limit + 1):
            refused(f"{what} must be in 1 .. {limit}", radius=bad)
    if kind == "mhs_geomorphon":
        for bad in (-0.5, float("nan"), float("inf")):
            refused("flat_deg", flat_deg=bad)
    else:
        refused("mask", mask=0)
        refused("mask", mask=1 << (10 if kind == "mhs_terrain" else 3))
        refused("out_dtype", out_dtype=_lib.I16)
    if fn.endswith("_dev"):
        refused("ld smaller", ld=11)
        if kind != "mhs_geomorphon":
            refused("plane_stride", mask=3, plane_stride=119)
    # good arguments pass every check: what is left is the device (present and initialised, or not)
    rc, msg = call(fn, radius=call.lib.mhs_terrain_max_radius(), flat_deg=0.0, dx_row=np.full(10, 30.0), window=(0, 0, 0, 0))
    assert rc in (_lib.OK, _lib.ERR_NODEVICE), msg


def test_rule_header_in_a_plain_cpp_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "terrain_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "machisplin_amd", "csrc"),
           os.path.join(ROOT, "tests", "terrain_check.cpp"), "-o", exe]
    pr = subprocess.run(cmd, capture_output=True, text=True)
    assert pr.returncode == 0, pr.stderr
    pr = subprocess.run([exe], capture_output=True, text=True)       # stand-alone: the sanitizer runtimes are linked into it
    assert pr.returncode == 0, pr.stdout + pr.stderr
    lines = pr.stdout.split("\n")
    assert lines[len(HAND)] == "OK"
    got = {ln.split()[0]: float(ln.split()[1]) for ln in lines[:len(HAND)]}
    assert got.keys() == HAND.keys()
    for name, want in HAND.items():
        assert _close(name, got[name], float(want)), (name, got[name], want)
