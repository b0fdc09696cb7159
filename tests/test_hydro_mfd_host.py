"""CPU: the multiple-flow-direction rules (include/machisplin_hip.h, section "hydrology, multiple flow direction").  The
restatement the GPU tests compare with (tests/hydro_mfd_ref.py: shares in numpy, accumulation by one walk in topological
order) is checked against the rules' invariants on every test plane and exponent; Jacobi sweeps from A = 1 -- what the
kernel's tile solves do -- reach the walk's value bit for bit and never lower a value, the property the kernel relies on; on a
ramp, where every cell has one receiver, MFD is D8; both entry points refuse bad arguments before they touch a device; and the
rule header the kernels are built from (csrc/hydro_rule.h) gives the walk's bits in a plain C++ program compiled with the host
compiler under AddressSanitizer + UBSan and run stand-alone."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import hydro_mfd_ref as mr
import hydro_ref as hr
from machisplin_amd import _lib

ROOT = os.path.dirname(os.path.abspath(os.path.dirname(__file__)))
NAN = float("nan")
DX, DY = 30.0, 28.5
PLANE_IDS = [f"{k}-{s[0]}x{s[1]}" for k, s in mr.PLANES]


@functools.lru_cache(maxsize=None)
def _base(kind, shape):
    z = mr.plane(kind, shape)
    z.setflags(write=False)
    return z, hr.hydro(z, NAN, DX, DY)


@pytest.mark.parametrize("kind,shape", mr.PLANES, ids=PLANE_IDS)
def test_invariants_on_the_test_planes(kind, shape):
    z, base = _base(kind, shape)
    for x in mr.EXPONENTS:
        m = mr.hydro_mfd(z, NAN, DX, DY, x, base=base)
        mr.check_invariants(z, m, base["flowdir"])
        if kind == "cone" and x == 1.0:
            # the water diverges from the apex: D8 leaves most of the slope at A = 1, MFD hardly a cell
            valid = ~np.isnan(z)
            assert (base["flowacc"][valid] == 1.0).mean() > 0.25 and (m["flowacc"][valid] == 1.0).mean() < 0.02


@pytest.mark.parametrize("kind,shape", mr.PLANES, ids=PLANE_IDS)
def test_jacobi_sweeps_reach_the_value_of_the_walk_bit_for_bit(kind, shape):
    z, base = _base(kind, shape)
    for x in mr.EXPONENTS:
        m = mr.hydro_mfd(z, NAN, DX, DY, x, base=base)
        A, sweeps = mr.jacobi(m["filled"], m["incoming"])              # asserts that no sweep lowers a value
        assert np.array_equal(A, m["flowacc"], equal_nan=True), (kind, shape, x)
        if kind == "spiral":
            assert sweeps > 96 * 96 / 2                                 # the channel is one path through half the plane


def test_the_ramp_equals_d8():
    z, base = _base("ramp", (1, 70))
    for x in mr.EXPONENTS:
        m = mr.hydro_mfd(z, NAN, DX, DY, x, base=base)
        assert np.array_equal(m["flowacc"], base["flowacc"]) and np.array_equal(m["flowacc"][0], 70.0 - np.arange(70.0))
        assert ((m["shares"] > 0.0).sum(axis=0) == (np.arange(70) > 0)).all() and (m["shares"][4, 0, 1:] == 1.0).all()


def test_hand_worked_shares():
    """3 x 3, dx = dy = 1, centre 5: E = 3, S = 4, SE = 3, the rest 5 or above.  s_E = 2, s_SE = 2 / sqrt 2, s_S = 1: p = 1,
    1 / sqrt 2, 0.5; with x = 2: 1, 0.5 (to rounding), 0.25."""
    z = np.array([[7.0, 6, 5], [6, 5, 3], [5, 4, 3]])
    h = hr.hydro(z, NAN, 1.0, 1.0)
    f, has = mr.shares(h["filled"], h["dist"], 1.0, 1.0, 1.0)
    p = np.array([1.0, (2.0 / np.sqrt(2.0)) / 2.0, 0.5])
    assert has[1, 1] and np.array_equal(f[:3, 1, 1], p / ((p[0] + p[1]) + p[2])) and not f[3:, 1, 1].any()
    f2, _ = mr.shares(h["filled"], h["dist"], 1.0, 1.0, 2.0)
    p2 = np.power(p, 2.0)
    assert np.array_equal(f2[:3, 1, 1], p2 / ((p2[0] + p2[1]) + p2[2])) and abs(f2[0, 1, 1] - 1.0 / 1.75) < 1e-15
    # a flat cell shares evenly among the neighbours one step nearer the exit: the centre of a 5 x 5 constant plane has D = 2
    # and eight neighbours at D = 1
    z = np.full((5, 5), 3.0)
    h = hr.hydro(z, NAN, 1.0, 1.0)
    f, has = mr.shares(h["filled"], h["dist"], 1.0, 1.0, 1.1)
    assert (f[:, 2, 2] == 0.125).all() and not has[0].any() and has[1:-1, 1:-1].all()


class _Call:
    """the two entry points on HOST arrays that are never read: every refusal comes before the first device call.  Where an
    earlier test of the session has initialised a device, a call with good arguments does run: the _dev entry then gets
    device planes (it would take the host arrays' addresses for device memory), the host entry keeps the host arrays."""

    def __init__(self, fn):
        self.lib = _lib.load()
        self.grid = _lib.Grid(0.0, 10.0, 1.0, 1.0, 10, 12)
        self.z = np.zeros((2, 10, 12), dtype=np.float32)
        self.planes = np.zeros((3, 10, 12))
        zp, self.pp = self.z.ctypes.data, [self.planes[k].ctypes.data for k in range(3)]
        if fn.endswith("_dev") and _lib._inited_device is not None:
            import torch
            dev = torch.device("cuda", _lib._inited_device)
            self.zd = torch.zeros((2, 10, 12), dtype=torch.float32, device=dev)
            self.pd = torch.zeros((3, 10, 12), dtype=torch.float64, device=dev)
            zp, self.pp = self.zd.data_ptr(), [self.pd[k].data_ptr() for k in range(3)]
        self.stack = _lib.Stack(zp, 2, _lib.F32, 120, 12, NAN)

    def __call__(self, fn, layer=0, min_slope_tan=0.001, max_passes=0, exponent=1.1, out="default", which=(0, 1, 2), out_dtype=_lib.F64,
                 ld=12, dx=30.0):
        cu = _lib.TerrainUnits(dx, None, 30.0, 1.0)
        o = _lib.HydroMfdOut(*[self.pp[k] if k in which else None for k in range(3)])
        info = _lib.HydroInfo()
        head = (C.byref(self.grid), C.byref(self.stack), layer, C.byref(cu), min_slope_tan, max_passes, exponent,
                None if out is None else C.byref(o), out_dtype)
        if fn.endswith("_dev"):
            rc = self.lib.mhs_hydro_mfd_dev(*head, ld, None, C.byref(info))
        else:
            rc = self.lib.mhs_hydro_mfd(*head, C.byref(info))
        return rc, self.lib.mhs_last_error().decode()


@pytest.mark.parametrize("fn", ["mhs_hydro_mfd_dev", "mhs_hydro_mfd"])
def test_refusals_come_before_any_device_call(fn):
    call = _Call(fn)

    def refused(needle, **kw):
        rc, msg = call(fn, **kw)
        assert rc == _lib.ERR_INVALID and needle in msg and fn in msg, (kw, rc, msg)

    for bad in (0.0, -1.0, 65.0, 64.000001, NAN, float("inf")):
        refused("exponent", exponent=bad)
    refused("out is NULL", out=None)
    refused("out names no plane (filled, flowacc, twi", which=())
    refused("layer 2", layer=2)
    refused("min_slope_tan", min_slope_tan=0.0)
    refused("dx must be", dx=-1.0)
    refused("max_passes", max_passes=-1)
    refused("out_dtype", out_dtype=_lib.I16)
    if fn.endswith("_dev"):
        refused("ld smaller", ld=11)
    # good arguments pass every check: what is left is the device (present and initialised, or not)
    for which, x in (((0, 1, 2), 1.0), ((2,), 64.0), ((1,), 1e-3)):
        rc, msg = call(fn, which=which, exponent=x, max_passes=7, out_dtype=_lib.F32)
        assert rc in (_lib.OK, _lib.ERR_NODEVICE), msg


def test_rule_header_in_a_plain_cpp_program_under_sanitizers(tmp_path):
    """the check program sweeps the rule header's functions to their fixed points on the 33 x 65 noise plane: at the exponent
    1 its accumulation is the walk's, bit for bit"""
    exe = str(tmp_path / "hydro_mfd_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "machisplin_amd", "csrc"),
           os.path.join(ROOT, "tests", "hydro_mfd_check.cpp"), "-o", exe]
    pr = subprocess.run(cmd, capture_output=True, text=True)
    assert pr.returncode == 0, pr.stderr
    kind, shape = "noise", (33, 65)
    z, base = _base(kind, shape)
    want = mr.hydro_mfd(z, NAN, DX, DY, 1.0, base=base)
    text = f"{shape[0]} {shape[1]} {DX!r} {DY!r} 1\n" + "\n".join(repr(float(v)) for v in z.ravel()) + "\n"
    pr = subprocess.run([exe], input=text, capture_output=True, text=True)       # stand-alone: the sanitizer runtimes are linked into it
    assert pr.returncode == 0, pr.stdout[-400:] + pr.stderr[-2000:]
    lines = pr.stdout.split("\n")
    n = shape[0] * shape[1]
    assert lines[0] == f"n_valid {want['n_valid']}" and lines[1] == f"n_sinks {want['n_sinks']}" and lines[3 + n] == "OK"
    got = np.array([float.fromhex(s) for s in lines[3:3 + n]]).reshape(shape)
    assert np.array_equal(got, want["flowacc"], equal_nan=True)
    assert 1 < int(lines[2].split()[1]) <= n                     # swept to a fixed point, not in one go
