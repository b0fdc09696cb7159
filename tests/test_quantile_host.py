"""CPU: the quantile rule (include/machisplin_hip.h, section "zonal quantiles").  The restatement the GPU tests compare with
(tests/quantile_ref.py) agrees with a plain per-zone loop, with numpy.median bit for bit where the quantisation is exact, with
zonal_ref's min, max and count at p = 0 and p = 1, and with numpy.quantile within the header's derived bound; every entry point
refuses bad arguments before it touches a device, naming the argument; and the rule header the kernels are built from
(csrc/quantile_rule.h) gives the restatement's bits in a plain C++ program compiled with gcc under AddressSanitizer + UBSan and
run stand-alone.

The bound (quantile_rule.h derives it): against the exact type 7 value of the same q, |Q - X| <= u (n D + D + M) quantum with
u = 2^-53, D = max q - min q of the zone, M = the larger magnitude of the two; numpy.quantile(method="linear") lies within the same
bound of X, so the two may differ by twice the bound."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import quantile_ref as qr
import zonal_ref as zr
from machisplin_amd import _lib
from machisplin_amd import zonal as zn
from machisplin_amd.raster import Geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
PROBS = (0.0, 0.05, 1.0 / 3.0, 0.5, 0.9, 1.0)


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


CASES = ((1, (1, 1), 1), (2, (7, 9), 4), (3, (40, 50), 30), (4, (20, 20), 500))


@pytest.mark.parametrize("dtype", (np.float32, np.float64, np.int16), ids=("f32", "f64", "i16"))
def test_the_restatement_equals_a_plain_loop_and_numpy(dtype):
    for seed, shape, nz in CASES:
        v, zones, nodata = _plane(seed, shape, nz, dtype)
        table, planes, info = qr.quantile(v, zones, PROBS, nodata, n_zones=nz)
        want = qr.loop(v, zones, PROBS, nodata, n_zones=nz)
        assert info["n_inexact"] == 0
        assert bits_equal(table["q"], want["q"]) and bits_equal(table["count"], want["count"]), (dtype, shape)
        # p = 0 and p = 1 are zonal's min and max, the count its count
        zt, _, zinfo = zr.zonal(v, zones, nodata, n_zones=nz)
        assert bits_equal(table["q"][:, 0], zt["min"]) and bits_equal(table["q"][:, 5], zt["max"]) and bits_equal(table["count"], zt["count"])
        assert {k: info[k] for k in qr.INFO if k != "n_present"} == {k: zinfo[k] for k in qr.INFO if k != "n_present"}
        assert info["n_present"] == int((zt["count"] > 0).sum())
        x, na = zr.na_mask(v, nodata)
        for z in range(nz):
            cell = x[(zones == z) & ~na]
            if cell.size == 0:
                assert np.isnan(table["q"][z]).all() and table["count"][z] == 0
                continue
            # the median: numpy's, bit for bit
            assert bits_equal(table["q"][z, 3], np.float64(np.median(cell))), (dtype, shape, z)
            # min <= Q <= max, and Q does not decrease with p
            assert (table["q"][z] >= cell.min()).all() and (table["q"][z] <= cell.max()).all() and (np.diff(table["q"][z]) >= 0).all()
            # numpy's linear quantile within twice the header's bound; the exact type 7 value within the bound
            s = np.sort(np.rint(cell / info["quantum"]).astype(np.int64))
            b = qr.bound(s, info["quantum"])
            for j in (1, 2, 4):
                assert abs(table["q"][z, j] - float(np.quantile(cell, PROBS[j], method="linear"))) <= 2 * b, (dtype, shape, z, j)
                H = Fraction(cell.size - 1) * Fraction(PROBS[j])
                lo = H.numerator // H.denominator
                hi = min(lo + 1, cell.size - 1)
                exact = (Fraction(int(s[lo])) + (H - lo) * (int(s[hi]) - int(s[lo]))) * Fraction(info["quantum"])
                assert abs(Fraction(float(table["q"][z, j])) - exact) <= Fraction(b), (dtype, shape, z, j)
        # the planes: a cell's zone's row; below counts the smaller values of the zone; frac_below = below / n
        con = (zones >= 0) & ~na
        for (r, c), inz in np.ndenumerate(zones >= 0):
            if inz:
                assert bits_equal(planes["q"][:, r, c], table["q"][zones[r, c]])
            else:
                assert np.isnan(planes["q"][:, r, c]).all()
            if con[r, c]:
                same = x[con & (zones == zones[r, c])]
                assert planes["below"][r, c] == int((same < x[r, c]).sum())
                assert planes["frac_below"][r, c] == np.float64(planes["below"][r, c]) / np.float64(same.size)
            else:
                assert planes["below"][r, c] == -1 and np.isnan(planes["frac_below"][r, c])


def test_hand_worked_cases():
    # n = 0 (zone 2 absent, zone 1 NA only), 1, 2, and an even n with a .5 median
    v = np.array([[5.0, NAN, -9.0, 7.0, 1.0, 2.0, 1.0, 2.0, 5.0, 9.0]])
    zones = np.array([[0, 1, 1, -1, 3, 3, 4, 4, 4, 4]], dtype=np.int32)
    t, p, info = qr.quantile(v, zones, (0.5, 0.0, 1.0, 0.25), nodata=-9.0, n_zones=5, quantum=0.25)
    assert t["count"].tolist() == [1, 0, 0, 2, 4] and info["n_present"] == 3 and info["n_cells_in_zones"] == 9 and info["n_contributing"] == 7
    assert t["q"][0].tolist() == [5.0, 5.0, 5.0, 5.0] and np.isnan(t["q"][1:3]).all()
    assert t["q"][3].tolist() == [1.5, 1.0, 2.0, 1.25] and t["q"][4].tolist() == [3.5, 1.0, 9.0, 1.75]
    assert p["below"].tolist() == [[0, -1, -1, -1, 0, 1, 0, 1, 2, 3]]
    assert p["frac_below"][0, [0, 4, 5, 9]].tolist() == [0.0, 0.0, 0.5, 0.75] and np.isnan(p["frac_below"][0, 1:4]).all()
    assert p["q"][0, 0].tolist()[:1] == [5.0] and np.isnan(p["q"][:, 0, 3]).all() and np.isnan(p["q"][:, 0, 1]).all() and p["q"][0, 0, 9] == 3.5
    assert qr.present(t)["zone"].tolist() == [0, 3, 4]
    # ties share the smallest rank
    t, p, _ = qr.quantile(np.array([[3.0, 1.0, 3.0, 3.0]]), None, (0.5,), quantum=1.0)
    assert t["q"].tolist() == [[3.0]] and p["below"].tolist() == [[1, 0, 1, 1]] and p["frac_below"].tolist() == [[0.25, 0.0, 0.25, 0.25]]
    # an Inf is counted and otherwise NA
    t, _, info = qr.quantile(np.array([[1.0, np.inf, 3.0]]), None, (0.5,))
    assert info["n_nonfinite"] == 1 and t["count"].tolist() == [2] and t["q"].tolist() == [[2.0]]
    # the aggregate's zones: a target of 2 x 2 cells over a 4 x 6 source, shifted: the footprints partition, the rest has no zone
    S, T = Geometry(0.0, 4.0, 1.0, 1.0, 4, 6), Geometry(0.75, 4.0, 2.0, 2.0, 2, 2)
    z = qr.target_zones(S, T)
    assert z.tolist() == [[-1, 0, 0, 1, 1, -1], [-1, 0, 0, 1, 1, -1], [-1, 2, 2, 3, 3, -1], [-1, 2, 2, 3, 3, -1]]


class _Call:
    """One of the two entry points on a 10 x 12 stack of two layers.  A refusal comes before the first device call and reads no
    plane.  The calls that PASS the checks end at MHS_ERR_NODEVICE on a machine without a GPU -- where there is one they run, so
    the arrays of the _dev entry are then device tensors."""

    def __init__(self, fn):
        import torch
        self.lib = _lib.load()
        if fn.endswith("_dev") and torch.cuda.is_available():
            self.z = torch.zeros((2, 10, 12), dtype=torch.float32, device="cuda")
            self.zones = torch.zeros((10, 12), dtype=torch.int32, device="cuda")
            self.tab = torch.zeros((3, 128 * 16), dtype=torch.float64, device="cuda")
            self.pl = torch.zeros((18, 10, 12), dtype=torch.float64, device="cuda")
            ptr = lambda t: t.data_ptr()                                      # noqa: E731
        else:
            self.z = np.zeros((2, 10, 12), dtype=np.float32)
            self.zones = np.zeros((10, 12), dtype=np.int32)
            self.tab = np.zeros((3, 128 * 16), dtype=np.float64)
            self.pl = np.zeros((18, 10, 12), dtype=np.float64)
            ptr = lambda a: a.ctypes.data                                     # noqa: E731
        self.zptr, self.qptr = ptr(self.z), ptr(self.zones)
        self.tptr, self.pptr = [ptr(self.tab[k]) for k in range(3)], [ptr(self.pl[k]) for k in range(18)]
        self.stack = _lib.Stack(self.zptr, 2, _lib.F32, 120, 12, NAN)
        self.table = _lib.QuantileTable(128, None, self.tptr[1], self.tptr[2])
        self.planes = self.make_planes(2)
        self.info = _lib.QuantileInfo()

    def make_planes(self, n_q, ld=12, dtype=_lib.F64):
        p = _lib.QuantilePlanes()
        for k in range(n_q):
            p.q[k], p.ld_q[k] = self.pptr[k], ld
        p.below, p.ld_below, p.frac_below, p.ld_frac_below, p.dtype = self.pptr[16], ld, self.pptr[17], ld, dtype
        return p

    def __call__(self, fn, grid=(10, 12), stack="default", layer=0, zones="default", ld_zones=12, n_zones=5, quantum=0.25, flags=0, probs=(0.5, 0.9),
                 n_probs=None, target=None, table="default", planes="default", info=None):
        g = C.byref(_lib.Grid(0.0, 10.0, 1.0, 1.0, *grid)) if grid is not None else None
        s = C.byref(self.stack) if stack == "default" else stack
        q = self.qptr if zones == "default" else zones
        t = C.byref(self.table) if table == "default" else table
        p = C.byref(self.planes) if planes == "default" else planes
        cp = (C.c_double * max(len(probs), 1))(*probs) if probs is not None else None
        n_probs = len(probs or ()) if n_probs is None else n_probs
        tg = C.byref(_lib.Grid(*target)) if target is not None else None
        f = getattr(self.lib, fn)
        if fn.endswith("_dev"):
            rc = f(g, s, layer, q, ld_zones, n_zones, quantum, flags, cp, n_probs, tg, t, p, None, info)
        else:
            rc = f(g, s, layer, q, n_zones, quantum, flags, cp, n_probs, tg, t, p, info)
        return rc, self.lib.mhs_last_error().decode()


@pytest.mark.parametrize("fn", ("mhs_zonal_quantile_dev", "mhs_zonal_quantile"))
def test_refusals_of_the_library_come_before_any_device_call(fn):
    call = _Call(fn)

    def refused(needle, **kw):
        rc, msg = call(fn, **kw)
        assert rc == _lib.ERR_INVALID and needle in msg and fn in msg, (kw, rc, msg)

    refused("NULL", grid=None)
    refused("NULL", stack=None)
    refused("data is NULL", stack=C.byref(_lib.Stack(None, 2, _lib.F32, 120, 12, NAN)))
    refused("nrow, ncol", grid=(0, 12))
    refused("nrow * ncol", grid=(46341, 46341))
    refused("bad stack dtype", stack=C.byref(_lib.Stack(call.zptr, 2, 7, 120, 12, NAN)))
    refused("layer", layer=2)
    refused("strides", stack=C.byref(_lib.Stack(call.zptr, 2, _lib.F32, 120, 11, NAN)))     # the shapes do not match
    refused("n_zones", n_zones=2 ** 31)
    refused("n_zones", n_zones=-1)
    refused("n_zones", zones=None, n_zones=5)                                  # without a zone plane it is not the caller's to give
    refused("capacity", n_zones=129)
    refused("capacity", zones=None, n_zones=0, target=(0.0, 10.0, 0.5, 0.5, 20, 24))
    refused("zones and target", target=(0.0, 10.0, 2.0, 2.0, 5, 6))
    refused("target", zones=None, n_zones=0, target=(0.0, 10.0, 2.0, 2.0, 0, 6))
    refused("target", zones=None, n_zones=0, target=(0.0, 10.0, 0.0, 2.0, 5, 6))
    refused("target", zones=None, n_zones=0, target=(0.0, 10.0, 2.0, 2.0, 46341, 46341))
    for bad in (3.0, 0.75, -1.0, float("inf"), NAN, 2.0 ** -1030):
        refused("quantum", quantum=bad)
    refused("flags", flags=1)
    refused("probs", probs=None)
    refused("probs", probs=(), n_probs=0)
    refused("probs", probs=(0.5,) * 17)
    refused("probs[1]", probs=(0.5, 1.5))
    refused("probs[0]", probs=(-0.01,))
    refused("probs[2]", probs=(0.0, 1.0, NAN))
    refused("no output", table=None, planes=None)
    refused("no output", table=C.byref(_lib.QuantileTable()), planes=C.byref(_lib.QuantilePlanes()))
    refused("only zone", table=C.byref(_lib.QuantileTable(128, call.tptr[0])), planes=None, info=C.byref(call.info))
    refused("needs info", table=C.byref(_lib.QuantileTable(128, call.tptr[0], call.tptr[1])))
    refused("capacity", table=C.byref(_lib.QuantileTable(-1, None, call.tptr[1])))
    refused("dtype", planes=C.byref(call.make_planes(2, dtype=_lib.I16)))
    refused("q[2]", planes=C.byref(call.make_planes(3)))                      # a plane without a probability
    if fn.endswith("_dev"):
        refused("ld_zones", ld_zones=11)
        refused("ld of plane q[0]", planes=C.byref(call.make_planes(2, ld=11)))
        only_below = _lib.QuantilePlanes()
        only_below.below, only_below.ld_below, only_below.dtype = call.pptr[16], 11, _lib.F64
        refused("ld of plane below", planes=C.byref(only_below))
    only_q = _lib.QuantileTable(128, None, None, call.tptr[2])
    for kw in (dict(), dict(table=C.byref(only_q), planes=None), dict(table=None), dict(n_zones=0, quantum=0.0),
               dict(table=None, planes=None, info=C.byref(call.info)), dict(quantum=2.0 ** -1022), dict(n_zones=128), dict(zones=None, n_zones=0),
               dict(zones=None, n_zones=0, target=(0.3, 9.9, 2.5, 3.0, 3, 4)), dict(probs=(1.0, 0.0, 0.5, 0.5), planes=None),
               dict(table=C.byref(_lib.QuantileTable(128, call.tptr[0], call.tptr[1], call.tptr[2])), info=C.byref(call.info))):
        rc, msg = call(fn, **kw)
        assert rc in (_lib.OK, _lib.ERR_NODEVICE), (kw, msg)


def test_refusals_of_the_sort_come_before_any_device_call():
    lib = _lib.load()

    def refused(needle, *a):
        rc = lib.mhs_sort_keys_dev(*a)
        assert rc == _lib.ERR_INVALID and needle in lib.mhs_last_error().decode(), (a, lib.mhs_last_error())

    buf = np.zeros(4, dtype=np.uint64)
    refused("n must", buf.ctypes.data, -1, 0, 64, None, None)
    refused("n must", buf.ctypes.data, 2 ** 31, 0, 64, None, None)
    refused("window", buf.ctypes.data, 4, 8, 7, None, None)
    refused("window", buf.ctypes.data, 4, 0, 65, None, None)
    refused("window", buf.ctypes.data, 4, -1, 8, None, None)
    refused("keys is NULL", None, 4, 0, 64, None, None)
    import torch
    with pytest.raises(ValueError, match="1-D uint64 or int64"):
        zn.sort_keys(torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="contiguous"):
        zn.sort_keys(torch.zeros(8, dtype=torch.int64)[::2])
    with pytest.raises(ValueError, match="bit_lo, bit_hi"):
        zn.sort_keys(torch.zeros(8, dtype=torch.int64), 9, 8)
    with pytest.raises(ValueError, match="device tensor"):
        zn.sort_keys(torch.zeros(8, dtype=torch.int64))


def _fake(nrow=10, ncol=12, n_layers=2):
    """what quantile() looks at before its first device call; touching the planes would be one"""
    class Stack:
        geom = Geometry(0.0, float(nrow), 1.0, 1.0, nrow, ncol)
        nodata = NAN

        @property
        def planes(self):
            raise AssertionError("the planes were touched before the refusal")
    s = Stack()
    s.n_layers = n_layers
    return s


def test_refusals_of_the_python_calls_come_before_any_device_call():
    import torch
    zones = torch.zeros((10, 12), dtype=torch.int32)

    def refused(needle, *a, **kw):
        with pytest.raises(ValueError, match=needle):
            zn.quantile(*a, **kw)

    refused("shape mismatch", _fake(), torch.zeros((10, 13), dtype=torch.int32))
    refused("shape mismatch", _fake(12, 10), zones)
    refused("probs", _fake(), zones, probs=())
    refused("probs", _fake(), zones, probs=(0.5,) * 17)
    refused("probs", _fake(), zones, probs=(0.5, 1.01))
    refused("probs", _fake(), zones, probs=(-0.5,))
    refused("probs", _fake(), zones, probs=(NAN,))
    refused("probs", _fake(), zones, probs=("a",))
    refused("no output", _fake(), zones, table=None)
    refused("unknown statistic", _fake(), zones, planes=("median",))
    refused("once", _fake(), zones, planes=("q", "q"))
    for bad in (3.0, 0.3, 0.0, -2.0, float("inf"), NAN):
        refused("quantum", _fake(), zones, quantum=bad)
    refused("n_zones", _fake(), zones, n_zones=2 ** 31)
    refused("n_zones", _fake(), zones, n_zones=0)
    refused("n_zones", _fake(), None, n_zones=3)
    refused("table", _fake(), zones, table="sparse")
    refused("integer tensor", _fake(), zones.double())
    refused("integer tensor", _fake(), zones[0])
    refused("layer", _fake(), zones, layer=2)
    refused(r"nrow \* ncol", _fake(46341, 46341), zones)
    refused("out_dtype", _fake(), zones, planes=("q",), out_dtype=torch.float16)
    for kw in (dict(probs=(0.5, 2.0)), dict(layer=3), dict(quantum=0.3), dict(out_dtype=torch.int32)):
        with pytest.raises(ValueError):
            zn.aggregate_quantile(_fake(), Geometry(0.0, 10.0, 2.0, 2.0, 5, 6), **kw)
    with pytest.raises(ValueError, match="geom"):
        zn.aggregate_quantile(_fake(), Geometry(0.0, 10.0, 2.0, 2.0, 0, 6))
    # a call that passes every check goes on to the planes
    for call in (lambda: zn.quantile(_fake(), zones.long(), probs=(0.0, 0.5, 0.5, 1.0), planes=("below", "q"), n_zones=4, table="present", quantum=0.125,
                                     out_dtype=torch.float32),
                 lambda: zn.quantile(_fake(), None, probs=0.5), lambda: zn.aggregate_quantile(_fake(), Geometry(0.0, 10.0, 2.0, 2.0, 5, 6))):
        with pytest.raises(AssertionError, match="planes were touched"):
            call()


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
    exe = str(tmp_path / "quantile_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "machisplin_amd", "csrc"),
           os.path.join(ROOT, "tests", "quantile_check.cpp"), "-o", exe]
    run = subprocess.run(cmd, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    run = subprocess.run([exe], capture_output=True, text=True)       # stand-alone: the sanitizer runtimes are linked into it
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().split("\n")
    assert lines[-1] == "OK"
    n_case = n_zone = 0
    table = below = zones = None
    for ln in lines[:-1]:
        w = ln.split()
        if w[0] == "case":
            k, nrow, ncol, nz, e = (int(x) for x in w[1:])
            v, zones = _lcg_plane(k, nrow, ncol, nz)
            table, planes, info = qr.quantile(v, zones, PROBS, n_zones=nz, quantum=2.0 ** e)
            below = planes["below"].astype(np.int64)
            assert info["n_inexact"] == 0
            n_case += 1
        else:
            assert w[0] == "zone", ln
            z, n = int(w[1]), int(w[2])
            got = np.array([int(x, 16) for x in w[3:9]], dtype=np.uint64).view(np.float64)
            assert n == table["count"][z], ln
            assert bits_equal(got, table["q"][z]), (ln, table["q"][z])
            assert int(w[9]) == int(below[(zones == z) & (below >= 0)].sum()), ln
            n_zone += 1
    assert n_case == 5 and n_zone == 1 + 3 + 40 + 1 + 9000
