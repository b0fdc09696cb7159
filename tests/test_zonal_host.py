"""CPU: the zonal rule (include/machisplin_hip.h, section "zonal").  The restatement the GPU tests compare with
(tests/zonal_ref.py) agrees with a plain per-zone loop, with scipy.ndimage and numpy, and with hand-worked cases; every entry
point refuses bad arguments before it touches a device, naming the argument; and the rule header the kernels are built from
(csrc/zonal_rule.h) gives the restatement's bits in a plain C++ program compiled with gcc under AddressSanitizer + UBSan and run
stand-alone.

The bound on sum and mean is the header's: with n_inexact = 0, sum is the exact sum rounded once, |sum - exact| <= u |exact|, and
|mean - exact / n| <= 3.01 u |exact / n|, u = 2^-53; the exact sum is formed here with fractions."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import zonal_ref as zr
from machisplin_amd import _lib
from machisplin_amd import zonal as zn
from machisplin_amd.raster import Geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
U = 2.0 ** -53


def bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _plane(seed, shape, n_zones, dtype):
    rng = np.random.default_rng(seed)
    if dtype == np.int16:
        v = rng.integers(-3000, 9000, shape).astype(np.int16)
        v[rng.random(shape) < 0.05] = -32768
        nodata = -32768.0
    else:
        v = (rng.integers(-40000, 90000, shape) / 16.0).astype(dtype)          # multiples of 1/16: exact at the default quantum
        v[rng.random(shape) < 0.05] = np.nan
        nodata = None
    zones = rng.integers(-1, n_zones, shape).astype(np.int32)
    return v, zones, nodata


@pytest.mark.parametrize("dtype", (np.float32, np.float64, np.int16), ids=("f32", "f64", "i16"))
def test_the_restatement_equals_a_plain_loop(dtype):
    for seed, shape, nz in ((1, (1, 1), 1), (2, (7, 9), 4), (3, (40, 50), 30), (4, (20, 20), 500)):
        v, zones, nodata = _plane(seed, shape, nz, dtype)
        table, _, info = zr.zonal(v, zones, nodata, n_zones=nz)
        want = zr.loop(v, zones, nodata, n_zones=nz)
        assert info["n_inexact"] == 0
        for k in zr.TABLE_STATS:
            assert bits_equal(table[k], want[k]), (dtype, shape, k)


def test_the_restatement_against_scipy_and_numpy():
    ndi = pytest.importorskip("scipy.ndimage")
    for dtype in (np.float32, np.int16):
        v, zones, nodata = _plane(11, (150, 170), 60, dtype)
        table, _, info = zr.zonal(v, zones, nodata, n_zones=60)
        assert info["n_inexact"] == 0
        x, na = zr.na_mask(v, nodata)
        ok = (zones >= 0) & ~na
        lab = np.where(ok, zones + 1, 0)
        idx = np.arange(1, 61)
        assert np.array_equal(table["count"], np.bincount(zones[ok], minlength=60))
        assert np.array_equal(table["cells"], np.bincount(zones[zones >= 0], minlength=60))
        assert bits_equal(table["min"], np.asarray(ndi.minimum(x, lab, idx), dtype=np.float64))
        assert bits_equal(table["max"], np.asarray(ndi.maximum(x, lab, idx), dtype=np.float64))
        # sum and mean: the header's bound against the exact sum, and scipy's float sums within their own bound of it
        for z in range(60):
            cell = x[ok & (zones == z)]
            exact = sum((Fraction(float(c)) for c in cell), Fraction(0))
            n = cell.size
            assert abs(Fraction(float(table["sum"][z])) - exact) <= Fraction(U) * abs(exact)
            assert abs(Fraction(float(table["mean"][z])) - exact / n) <= Fraction(3.01 * U) * abs(exact / n)
            slack = (n - 1) * U / (1 - (n - 1) * U) * float(np.abs(cell).sum())
            assert abs(Fraction(float(ndi.sum_labels(x, lab, z + 1))) - exact) <= Fraction(slack)
            assert abs(float(ndi.mean(x, lab, z + 1)) - float(table["mean"][z])) <= (slack / n + 4 * U * abs(float(exact / n)))


def test_hand_worked_cases():
    # two zones of three cells
    v = np.array([[1.0, 2.0, 3.0], [10.0, 20.0, 60.0]])
    zones = np.array([[0, 0, 0], [1, 1, 1]], dtype=np.int32)
    t, p, info = zr.zonal(v, zones, quantum=0.25)
    assert t["count"].tolist() == [3, 3] and t["sum"].tolist() == [6.0, 90.0] and t["mean"].tolist() == [2.0, 30.0]
    assert t["sd"][0] == 1.0 and t["sd"][1] == np.sqrt(700.0) and t["min"].tolist() == [1.0, 10.0] and t["max"].tolist() == [3.0, 60.0]
    assert t["range"].tolist() == [2.0, 50.0] and t["cells"].tolist() == [3, 3] and info["n_inexact"] == 0 and info["n_present"] == 2
    assert p["minus_mean"].tolist() == [[-1.0, 0.0, 1.0], [-20.0, -10.0, 30.0]] and p["dev"][0].tolist() == [-1.0, 0.0, 1.0]
    assert p["above_min"][1].tolist() == [0.0, 10.0, 50.0] and p["below_max"][0].tolist() == [2.0, 1.0, 0.0] and p["mean"][1].tolist() == [30.0] * 3
    # a zone with one contributing cell: sd is NA, dev too; a zone of NA values only: cells > 0, count 0, NA elsewhere; zone 2 absent
    v = np.array([[5.0, NAN, NAN, -9.0, 7.0]])
    zones = np.array([[0, 0, 1, 1, -1]], dtype=np.int32)
    t, p, info = zr.zonal(v, zones, nodata=-9.0, n_zones=3, quantum=1.0)
    assert t["count"].tolist() == [1, 0, 0] and t["cells"].tolist() == [2, 2, 0] and t["mean"][0] == 5.0 and np.isnan(t["sd"]).all()
    assert np.isnan(t["mean"][1:]).all() and np.isnan(t["min"][1:]).all() and np.isnan(t["sum"][1:]).all() and t["range"][0] == 0.0
    assert info["n_present"] == 2 and info["n_cells_in_zones"] == 4 and info["n_contributing"] == 1
    assert p["minus_mean"][0, 0] == 0.0 and np.isnan(p["minus_mean"][0, 1:]).all() and np.isnan(p["dev"]).all()
    assert p["count"].tolist() == [[1, 1, 0, 0, 0]] and p["cells"].tolist() == [[2, 2, 2, 2, 0]] and np.isnan(p["mean"][0, 2:]).all()
    assert zr.present(t)["zone"].tolist() == [0, 1]
    # constant values: sd 0, dev NA
    t, p, _ = zr.zonal(np.full((4, 4), 3.5), np.zeros((4, 4), np.int32), quantum=0.5)
    assert t["sd"][0] == 0.0 and t["mean"][0] == 3.5 and np.isnan(p["dev"]).all() and (p["minus_mean"] == 0.0).all()
    # an Inf is counted and otherwise NA; the inexact count; the default quantum
    v = np.array([[1.0, np.inf, 1.0 + 2.0 ** -40, 3.0]], dtype=np.float64)
    t, p, info = zr.zonal(v, np.zeros((1, 4), np.int32))
    assert info["quantum"] == 2.0 ** -28 and info["n_nonfinite"] == 1 and info["n_inexact"] == 1 and t["count"][0] == 3 and t["cells"][0] == 4
    assert zr.default_quantum(np.zeros((2, 2))) == 1.0 and zr.default_quantum(np.array([[2.0 ** 30]])) == 1.0
    assert zr.default_quantum(np.array([[-8848.86]])) == 2.0 ** -16 and zr.default_quantum(np.array([[7]], dtype=np.int16)) == 1.0


class _Call:
    """One of the two entry points on a 10 x 12 stack of two layers and a zone plane.  A refusal comes before the first device
    call and reads no plane.  The calls that PASS the checks end at MHS_ERR_NODEVICE on a machine without a GPU -- where there is
    one they run, so the arrays of the _dev entry are then device tensors."""

    def __init__(self, fn):
        import torch
        self.lib = _lib.load()
        if fn.endswith("_dev") and torch.cuda.is_available():
            self.z = torch.zeros((2, 10, 12), dtype=torch.float32, device="cuda")
            self.zones = torch.zeros((10, 12), dtype=torch.int32, device="cuda")
            self.tab = torch.zeros((9, 128), dtype=torch.float64, device="cuda")
            self.pl = torch.zeros((12, 10, 12), dtype=torch.float64, device="cuda")
            ptr = lambda t: t.data_ptr()                                      # noqa: E731
        else:
            self.z = np.zeros((2, 10, 12), dtype=np.float32)
            self.zones = np.zeros((10, 12), dtype=np.int32)
            self.tab = np.zeros((9, 128), dtype=np.float64)
            self.pl = np.zeros((12, 10, 12), dtype=np.float64)
            ptr = lambda a: a.ctypes.data                                     # noqa: E731
        self.zptr, self.qptr = ptr(self.z), ptr(self.zones)
        self.tptr, self.pptr = [ptr(self.tab[k]) for k in range(9)], [ptr(self.pl[k]) for k in range(12)]
        self.stack = _lib.Stack(self.zptr, 2, _lib.F32, 120, 12, NAN)
        self.table = _lib.ZonalTable(128, None, *self.tptr[1:])
        self.planes = _lib.ZonalPlanes()
        for k in range(12):
            self.planes.plane[k], self.planes.ld[k] = self.pptr[k], 12
        self.planes.dtype = _lib.F64
        self.info = _lib.ZonalInfo()

    def __call__(self, fn, grid=(10, 12), stack="default", layer=0, zones="default", ld_zones=12, n_zones=5, quantum=0.25, flags=0, table="default",
                 planes="default", info=None):
        g = C.byref(_lib.Grid(0.0, 10.0, 1.0, 1.0, *grid)) if grid is not None else None
        s = C.byref(self.stack) if stack == "default" else stack
        q = self.qptr if zones == "default" else zones
        t = C.byref(self.table) if table == "default" else table
        p = C.byref(self.planes) if planes == "default" else planes
        f = getattr(self.lib, fn)
        if fn.endswith("_dev"):
            rc = f(g, s, layer, q, ld_zones, n_zones, quantum, flags, t, p, None, info)
        else:
            rc = f(g, s, layer, q, n_zones, quantum, flags, t, p, info)
        return rc, self.lib.mhs_last_error().decode()


@pytest.mark.parametrize("fn", ("mhs_zonal_dev", "mhs_zonal"))
def test_refusals_of_the_library_come_before_any_device_call(fn):
    call = _Call(fn)

    def refused(needle, **kw):
        rc, msg = call(fn, **kw)
        assert rc == _lib.ERR_INVALID and needle in msg and fn in msg, (kw, rc, msg)

    refused("NULL", grid=None)
    refused("NULL", stack=None)
    refused("NULL", zones=None)
    refused("data is NULL", stack=C.byref(_lib.Stack(None, 2, _lib.F32, 120, 12, NAN)))
    refused("nrow, ncol", grid=(0, 12))
    refused("nrow * ncol", grid=(46341, 46341))
    refused("bad stack dtype", stack=C.byref(_lib.Stack(call.zptr, 2, 7, 120, 12, NAN)))
    refused("layer", layer=2)
    refused("layer", layer=-1)
    refused("strides", stack=C.byref(_lib.Stack(call.zptr, 2, _lib.F32, 120, 11, NAN)))     # the shapes do not match
    refused("n_zones", n_zones=2 ** 31)
    refused("n_zones", n_zones=-1)
    refused("capacity", n_zones=129)
    for bad in (3.0, 0.75, -1.0, float("inf"), NAN, 2.0 ** -1030):
        refused("quantum", quantum=bad)
    refused("flags", flags=2)
    refused("no output", table=None, planes=None)
    refused("no output", table=C.byref(_lib.ZonalTable()), planes=C.byref(_lib.ZonalPlanes()))
    refused("no statistic", table=C.byref(_lib.ZonalTable(128, call.tptr[0])), planes=None)
    refused("needs info", table=C.byref(_lib.ZonalTable(128, call.tptr[0], call.tptr[1])))
    refused("capacity", table=C.byref(_lib.ZonalTable(-1, None, call.tptr[1])))
    bad_dtype = _lib.ZonalPlanes()
    bad_dtype.plane[2], bad_dtype.ld[2], bad_dtype.dtype = call.pptr[2], 12, _lib.I16
    refused("dtype", planes=C.byref(bad_dtype))
    if fn.endswith("_dev"):
        refused("ld_zones", ld_zones=11)
        narrow = _lib.ZonalPlanes()
        narrow.plane[5], narrow.ld[5], narrow.dtype = call.pptr[5], 11, _lib.F64
        refused("ld of plane 5", planes=C.byref(narrow))
    only_mean = _lib.ZonalTable(128, None, None, None, call.tptr[3])
    for kw in (dict(), dict(table=C.byref(only_mean), planes=None), dict(table=None), dict(n_zones=0, quantum=0.0), dict(flags=1),
               dict(table=None, planes=None, info=C.byref(call.info)), dict(quantum=2.0 ** -1022), dict(n_zones=128)):
        rc, msg = call(fn, **kw)
        assert rc in (_lib.OK, _lib.ERR_NODEVICE), (kw, msg)


def _fake(nrow=10, ncol=12, n_layers=2):
    """what zonal() looks at before its first device call; touching the planes would be one"""
    class Stack:
        geom = Geometry(0.0, float(nrow), 1.0, 1.0, nrow, ncol)
        nodata = NAN

        @property
        def planes(self):
            raise AssertionError("the planes were touched before the refusal")
    s = Stack()
    s.n_layers = n_layers
    return s


def test_refusals_of_the_python_call_come_before_any_device_call():
    import torch
    zones = torch.zeros((10, 12), dtype=torch.int32)

    def refused(needle, *a, **kw):
        with pytest.raises(ValueError, match=needle):
            zn.zonal(*a, **kw)

    refused("shape mismatch", _fake(), torch.zeros((10, 13), dtype=torch.int32))
    refused("shape mismatch", _fake(12, 10), zones)
    refused("no output", _fake(), zones, stats=())
    refused("no output", _fake(), zones, table=None)
    refused("unknown statistic", _fake(), zones, stats=("median",))
    refused("unknown statistic", _fake(), zones, stats=("dev",))               # exists only as a plane
    refused("unknown statistic", _fake(), zones, planes=("mode",))
    refused("once", _fake(), zones, stats=("mean", "mean"))
    for bad in (3.0, 0.3, 0.0, -2.0, float("inf"), NAN):
        refused("quantum", _fake(), zones, quantum=bad)
    refused("n_zones", _fake(), zones, n_zones=2 ** 31)
    refused("n_zones", _fake(), zones, n_zones=0)
    refused("table", _fake(), zones, table="sparse")
    refused("integer tensor", _fake(), zones.double())
    refused("integer tensor", _fake(), zones[0])
    refused("layer", _fake(), zones, layer=2)
    refused(r"nrow \* ncol", _fake(46341, 46341), zones)
    refused("out_dtype", _fake(), zones, planes=("mean",), out_dtype=torch.float16)
    # a call that passes every check goes on to the planes
    with pytest.raises(AssertionError, match="planes were touched"):
        zn.zonal(_fake(), zones.long(), stats=("mean", "sd", "cells"), planes=("dev",), n_zones=4, table="present", quantum=0.125, out_dtype=torch.float32)


def _lcg_plane(k, nrow, ncol, nz):
    state = 9000 + k
    v = np.empty(nrow * ncol)
    zones = np.empty(nrow * ncol, dtype=np.int32)
    for i in range(nrow * ncol):
        state = (state * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        a = state >> 33
        state = (state * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        b = state >> 33
        v[i] = (1.0 if a % 2 else -1.0) * float(2 ** 30 - 1) * 0.25 if k == 3 else (float(a % 2001) - 1000.0) * 0.25
        zones[i] = b % (nz + 1) - 1
    return v.reshape(nrow, ncol), zones.reshape(nrow, ncol)


def test_rule_header_in_a_plain_cpp_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "zonal_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "machisplin_amd", "csrc"),
           os.path.join(ROOT, "tests", "zonal_check.cpp"), "-o", exe]
    run = subprocess.run(cmd, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    run = subprocess.run([exe], capture_output=True, text=True)       # stand-alone: the sanitizer runtimes are linked into it
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().split("\n")
    assert lines[-1] == "OK"
    n_case = n_zone = 0
    table = None
    for ln in lines[:-1]:
        w = ln.split()
        if w[0] == "case":
            k, nrow, ncol, nz, e = (int(x) for x in w[1:])
            v, zones = _lcg_plane(k, nrow, ncol, nz)
            table, _, info = zr.zonal(v, zones, n_zones=nz, quantum=2.0 ** e)
            assert info["n_inexact"] == 0
            n_case += 1
        else:
            assert w[0] == "zone", ln
            z, cells, n = (int(x) for x in w[1:4])
            got = np.array([int(x, 16) for x in w[4:]], dtype=np.uint64).view(np.float64)
            assert cells == table["cells"][z] and n == table["count"][z], ln
            want = np.array([table[name][z] for name in ("sum", "mean", "sd", "min", "max")])
            assert bits_equal(got, want), (ln, want)
            n_zone += 1
    assert n_case == 5 and n_zone == 1 + 3 + 40 + 1 + 9000
