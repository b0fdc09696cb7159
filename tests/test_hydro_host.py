"""CPU: the hydrology rules (include/machisplin_hip.h, section "hydrology").  The restatement the GPU tests compare with
(tests/hydro_ref.py: priority flood, breadth-first search, topological order) is itself checked against hand-worked cases and
against the rules' invariants on every test plane; both entry points refuse bad arguments with MHS_ERR_INVALID before they
touch a device; and the rule header the kernels are built from (csrc/hydro_rule.h) gives the same table in a plain C++ program
compiled with gcc under AddressSanitizer + UBSan and run stand-alone."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import hydro_ref as hr
from machisplin_amd import _lib

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
NAN = float("nan")


def _ring(nr, nc, ring, inside):
    z = np.full((nr, nc), float(inside))
    z[0], z[-1], z[:, 0], z[:, -1] = ring, ring, ring, ring
    return z


def _sink_sum(h):
    return float(np.nansum(h["flowacc"][h["flowdir"] == hr.DIR_OUT]))


# The cases, worked by hand (dx = dy = 1 unless said; neighbours k = 0 .. 7 = E, SE, S, SW, W, NW, N, NE):
#  pit    5 x 5, ring 5, inside 4, centre 1.  The ring cells are outlets (W = 5); every path from the inside ends on one, so
#         W = 5 inside: 9 cells raised.  Nothing is lower than anything: D = 0 on the ring, 1 beside it, 2 at the centre.  The
#         centre goes to the lowest k with D = 1: E.  (1, 1): E (1, 2) has D = 1, SE (2, 2) D = 2, S (2, 1) D = 1, SW (2, 0)
#         D = 0: k = 3.  (2, 3) receives the centre only: A = 2, and goes E to (2, 4): A = 3 ((1, 3) and (3, 3) go E too, to
#         their own ring cells).  The 16 ring cells have nothing lower: sinks, and their A sums to 25.
#  tilt   4 x 6, z = column.  Every cell but column 0 has its west neighbour 1 lower at distance 1 (SW, NW: 1 / sqrt 2): k = 4,
#         so every row is a chain: A = 6 - column; column 0 has nothing lower: 4 sinks.
#  const  5 x 7 of 17: D = rings to the border; the 20 ring cells are sinks; their A sums to 35.
#  nest   7 x 7: ring 9 but (3, 6) = 3; inside 6; rows 2 .. 4 x columns 2 .. 4 are 4, the centre (3, 3) is 2.  The lowest way out
#         of the inside is over (3, 5) = 6 to (3, 6): W = 6 on all 25 inner cells, 9 raised (the 4s and the 2).  (2, 5), (3, 5),
#         (4, 5) see (3, 6) below them: D = 0; from there D = 5 - column over the flat: centre 2, (1, 1) 4.  The centre goes E
#         (D = 1); (2, 5) goes SE to (3, 6).  The ring cells (9) see the inside (6) or (3, 6) below them, so everything ends in
#         (3, 6): A = 49 and it is the only sink.
#  hole   5 x 5: ring 5, inside 3, centre NA.  The 8 cells round the NA are outlets with nothing lower: sinks, direction -1;
#         the NA is -2.  (0, 0) has only (1, 1) lower: SE.  (1, 1) receives (0, 0), (0, 1) (S: 2 / 1 beats SE 2 / sqrt 2) and
#         (1, 0) (E): A = 4.  (1, 2) receives (0, 2) only ((0, 1) and (0, 3) go S): A = 2.  24 valid cells.
#  tie    3 x 3 of 4 with the centre 5: E, S, W, N all have s = 1: k = 0.  dx = 2: S and N 1, E and W 0.5: k = 2.  With E, S, W,
#         N level with the centre only the diagonals are lower: k = 1.
#  twi    the nine of the terrain table (1 2 3 / 4 5 6 / 7 8 10, dx = 2, dy = 4): slope_tan = sqrt(0.5625^2 + 0.78125^2);
#         A = 7, L = sqrt 8: log(7 sqrt 8 / slope_tan); with the floor 2 above the slope: log(7 sqrt 8 / 2).
_ST = math.sqrt(0.5625 * 0.5625 + 0.78125 * 0.78125)
HAND = {"pit_w_centre": 5.0, "pit_d_centre": 2, "pit_dir_centre": 0, "pit_dir_11": 3, "pit_a_24": 3.0, "pit_raised": 9, "pit_sinks": 16,
        "pit_sink_sum": 25.0,
        "tilt_all_west": 1, "tilt_ramp": 1, "tilt_raised": 0, "tilt_sinks": 4,
        "const_ring_distance": 1, "const_sinks": 20, "const_sink_sum": 35.0,
        "nest_w_centre": 6.0, "nest_d_centre": 2, "nest_d_11": 4, "nest_dir_centre": 0, "nest_dir_25": 1, "nest_a_gap": 49.0, "nest_raised": 9,
        "nest_sinks": 1,
        "hole_dir_centre": -2, "hole_dir_11": -1, "hole_dir_00": 1, "hole_a_11": 4.0, "hole_a_12": 2.0, "hole_sinks": 8, "hole_valid": 24,
        "hole_sink_sum": 24.0,
        "tie_dir_square": 0, "tie_dir_wide": 2, "tie_dir_diag": 1,
        "twi_hand": math.log(7.0 * math.sqrt(8.0) / _ST), "twi_floor": math.log(7.0 * math.sqrt(8.0) / 2.0)}
LOGS = ("twi_hand", "twi_floor")            # through log: equal to 1e-14, everything else exactly


def _close(name, got, want):
    return abs(got - want) <= 1e-14 if name in LOGS else got == want


def _restated():
    """the hand table from the restatement"""
    got = {}
    z = _ring(5, 5, 5, 4); z[2, 2] = 1
    h = hr.hydro(z, NAN, 1.0, 1.0)
    hr.check_invariants(z, h)
    got.update(pit_w_centre=h["filled"][2, 2], pit_d_centre=h["dist"][2, 2], pit_dir_centre=h["flowdir"][2, 2], pit_dir_11=h["flowdir"][1, 1],
               pit_a_24=h["flowacc"][2, 4], pit_raised=h["n_raised"], pit_sinks=h["n_sinks"], pit_sink_sum=_sink_sum(h))
    z = np.tile(np.arange(6.0), (4, 1))
    h = hr.hydro(z, NAN, 1.0, 1.0)
    hr.check_invariants(z, h)
    west = np.full((4, 6), 4); west[:, 0] = -1
    got.update(tilt_all_west=int(np.array_equal(h["flowdir"], west)), tilt_ramp=int(np.array_equal(h["flowacc"], 6.0 - z)),
               tilt_raised=h["n_raised"], tilt_sinks=h["n_sinks"])
    z = np.full((5, 7), 17.0)
    h = hr.hydro(z, NAN, 1.0, 1.0)
    hr.check_invariants(z, h)
    r, c = np.meshgrid(np.arange(5), np.arange(7), indexing="ij")
    got.update(const_ring_distance=int(np.array_equal(h["dist"], np.minimum(np.minimum(r, c), np.minimum(4 - r, 6 - c)))),
               const_sinks=h["n_sinks"], const_sink_sum=_sink_sum(h))
    z = _ring(7, 7, 9, 6); z[2:5, 2:5] = 4; z[3, 3] = 2; z[3, 6] = 3
    h = hr.hydro(z, NAN, 1.0, 1.0)
    hr.check_invariants(z, h)
    assert (h["filled"][1:6, 1:6] == 6.0).all()
    got.update(nest_w_centre=h["filled"][3, 3], nest_d_centre=h["dist"][3, 3], nest_d_11=h["dist"][1, 1], nest_dir_centre=h["flowdir"][3, 3],
               nest_dir_25=h["flowdir"][2, 5], nest_a_gap=h["flowacc"][3, 6], nest_raised=h["n_raised"], nest_sinks=h["n_sinks"])
    z = _ring(5, 5, 5, 3); z[2, 2] = NAN
    h = hr.hydro(z, NAN, 1.0, 1.0)
    hr.check_invariants(z, h)
    assert np.isnan(h["filled"][2, 2]) and np.isnan(h["flowacc"][2, 2]) and np.isnan(h["twi"]).all()      # every 3 x 3 holds the NA or leaves the raster
    got.update(hole_dir_centre=h["flowdir"][2, 2], hole_dir_11=h["flowdir"][1, 1], hole_dir_00=h["flowdir"][0, 0], hole_a_11=h["flowacc"][1, 1],
               hole_a_12=h["flowacc"][1, 2], hole_sinks=h["n_sinks"], hole_valid=h["n_valid"], hole_sink_sum=_sink_sum(h))
    z = np.full((3, 3), 4.0); z[1, 1] = 5
    got.update(tie_dir_square=hr.hydro(z, NAN, 1.0, 1.0)["flowdir"][1, 1], tie_dir_wide=hr.hydro(z, NAN, 2.0, 1.0)["flowdir"][1, 1])
    z[0, 1] = z[1, 0] = z[1, 2] = z[2, 1] = 5
    got.update(tie_dir_diag=hr.hydro(z, NAN, 1.0, 1.0)["flowdir"][1, 1])
    # the TWI of a plane whose centre has the hand nine around it: A there is what drains into it -- replace it by 7
    nine = np.array([[1.0, 2, 3], [4, 5, 6], [7, 8, 10]])
    st = hr.tr.terrain(nine, NAN, 2.0, 4.0)["slope_tan"][1, 1]
    assert st == _ST
    for name, floor in (("twi_hand", 0.001), ("twi_floor", 2.0)):
        got[name] = float(np.log((7.0 * np.sqrt(2.0 * 4.0)) / (st if st > floor else floor)))
    return got


def test_restatement_gives_the_hand_worked_values():
    got = _restated()
    assert got.keys() == HAND.keys()
    for name, want in HAND.items():
        assert _close(name, float(got[name]), float(want)), (name, got[name], want)


def test_restatement_twi_of_a_tilted_plane():
    """z = 2 column on 5 x 6, dx = 4, dy = 3: slope_tan = 2 * 8 / (8 * 4) = 0.5 inside; row r is a chain to the west, A = 6 -
    column; L = sqrt 12: twi = log((6 - column) sqrt 12 / 0.5), NaN on the outer ring.  z_factor 0.001 brings the slope under
    the floor tan(0.1 degree)."""
    z = np.tile(2.0 * np.arange(6.0), (5, 1))
    h = hr.hydro(z, NAN, 4.0, 3.0)
    want = np.full((5, 6), NAN)
    want[1:-1, 1:-1] = np.log(((6.0 - np.arange(6.0)) * np.sqrt(12.0) / 0.5))[None, 1:-1]
    assert np.array_equal(h["twi"], want, equal_nan=True)
    floor = np.tan(np.deg2rad(0.1))
    h = hr.hydro(z, NAN, 4.0, 3.0, z_factor=0.001)
    assert 0.0005 < floor and h["twi"][2, 2] == np.log(4.0 * np.sqrt(12.0) / floor)


@pytest.mark.parametrize("kind,shape", hr.PLANES, ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_invariants_on_the_test_planes(kind, shape):
    z = hr.spiral() if kind == "spiral" else hr.plane(kind, shape)
    h = hr.hydro(z, NAN, 30.0, 28.5)
    hr.check_invariants(z, h)
    if kind == "spiral":                       # the channel runs down to the border without a pit; the walls drain into it
        assert h["n_raised"] == 0 and z[0, 0] == 0.0 and z.max() == 10000.0
        chan = z < 10000.0
        assert chan[0].all() and not chan[1, 1:-2].any() and h["flowacc"].max() > 96 * 96 / 2
    if kind == "bowl" and shape[0] > 70:
        lake = h["filled"] > z
        assert lake.sum() > 2 * 32 * 64 and h["dist"].max() > 32           # a lake over several tiles, D grows across them
    if kind == "noise" and min(shape) > 2:
        assert h["n_raised"] > 0.05 * z.size


class _Call:
    """the two entry points on HOST arrays that are never read: every refusal comes before the first device call.  Where an
    earlier test of the session has initialised a device, a call with good arguments does run: the _dev entry then gets
    device planes (it would take the host arrays' addresses for device memory), the host entry keeps the host arrays."""

    def __init__(self, fn):
        self.lib = _lib.load()
        self.grid = _lib.Grid(0.0, 10.0, 1.0, 1.0, 10, 12)
        self.z = np.zeros((2, 10, 12), dtype=np.float32)
        self.planes = np.zeros((4, 10, 12))
        zp, self.pp = self.z.ctypes.data, [self.planes[k].ctypes.data for k in range(4)]
        if fn.endswith("_dev") and _lib._inited_device is not None:
            import torch
            dev = torch.device("cuda", _lib._inited_device)
            self.zd = torch.zeros((2, 10, 12), dtype=torch.float32, device=dev)
            self.pd = torch.zeros((4, 10, 12), dtype=torch.float64, device=dev)
            zp, self.pp = self.zd.data_ptr(), [self.pd[k].data_ptr() for k in range(4)]
        self.stack = _lib.Stack(zp, 2, _lib.F32, 120, 12, NAN)
        self.units = dict(dx=30.0, dx_row=None, dy=30.0, z_factor=1.0)

    def __call__(self, fn, grid=None, stack=None, layer=0, min_slope_tan=0.001, max_passes=0, out="default", which=(0, 1, 2, 3),
                 out_dtype=_lib.F64, ld=12, units="default", **unit_kw):
        u = dict(self.units, **unit_kw)
        rows = None if u["dx_row"] is None else np.ascontiguousarray(u["dx_row"], dtype=np.float64)
        cu = _lib.TerrainUnits(u["dx"], None if rows is None else rows.ctypes.data, u["dy"], u["z_factor"])
        o = _lib.HydroOut(*[self.pp[k] if k in which else None for k in range(4)])
        op = None if out is None else C.byref(o)
        info = _lib.HydroInfo()
        head = (C.byref(grid or self.grid), C.byref(stack or self.stack), layer, None if units is None else C.byref(cu), min_slope_tan,
                max_passes, op, out_dtype)
        if fn.endswith("_dev"):
            rc = self.lib.mhs_hydro_dev(*head, ld, None, C.byref(info))
        else:
            rc = self.lib.mhs_hydro(*head, C.byref(info))
        return rc, self.lib.mhs_last_error().decode()


@pytest.mark.parametrize("fn", ["mhs_hydro_dev", "mhs_hydro"])
def test_refusals_come_before_any_device_call(fn):
    call = _Call(fn)

    def refused(needle, **kw):
        rc, msg = call(fn, **kw)
        assert rc == _lib.ERR_INVALID and needle in msg and fn in msg, (kw, rc, msg)

    refused("out is NULL", out=None)
    refused("out names no plane", which=())
    refused("layer 2", layer=2)
    refused("layer -1", layer=-1)
    refused("units", units=None)
    refused("dem data is NULL", stack=_lib.Stack(None, 2, _lib.F32, 120, 12, NAN))
    refused("bad dem dtype", stack=_lib.Stack(call.z.ctypes.data, 2, 7, 120, 12, NAN))
    refused("dem strides", stack=_lib.Stack(call.z.ctypes.data, 2, _lib.F32, 120, 11, NAN))
    refused("bad grid geometry", grid=_lib.Grid(0.0, 10.0, 1.0, 1.0, 0, 12))
    # 2^29 x 2^29 cells: each side is admitted, the scratch planes' 22 bytes per cell would not fit a size_t
    refused("too many cells", grid=_lib.Grid(0.0, 10.0, 1.0, 1.0, 1 << 29, 1 << 29), stack=_lib.Stack(call.z.ctypes.data, 1, _lib.F32, 1 << 58, 1 << 29, NAN),
            ld=1 << 29)
    refused("out_dtype", out_dtype=_lib.I16)
    for bad in (0.0, -0.5, NAN, float("inf")):
        refused("min_slope_tan", min_slope_tan=bad)
        refused("z_factor", z_factor=bad)
        refused("dy must be", dy=bad)
        refused("dx must be", dx=bad)
        rows = np.full(10, 30.0); rows[7] = bad
        refused("dx_row[7]", dx_row=rows, dx=NAN)                 # dx is not looked at when dx_row is given
    refused("max_passes", max_passes=-1)
    if fn.endswith("_dev"):
        refused("ld smaller", ld=11)
    # good arguments pass every check: what is left is the device (present and initialised, or not)
    for which in ((0, 1, 2, 3), (3,), (1,)):
        rc, msg = call(fn, which=which, dx_row=np.full(10, 30.0), max_passes=7, out_dtype=_lib.F32)
        assert rc in (_lib.OK, _lib.ERR_NODEVICE), msg


def test_rule_header_in_a_plain_cpp_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "hydro_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "machisplin_amd", "csrc"),
           os.path.join(ROOT, "tests", "hydro_check.cpp"), "-o", exe]
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
