"""CPU: the proximity rule (include/machisplin_hip.h, section "proximity").  The two numpy restatements the GPU tests compare
with (tests/proximity_ref.py) agree with each other, with scipy's exact Euclidean transform and with hand-worked cases; every
entry point refuses bad arguments before it touches a device, naming the argument; and the rule header the kernels are built
from (csrc/proximity_rule.h) gives the restatement's planes in a plain C++ program compiled with gcc under AddressSanitizer +
UBSan and run stand-alone.  Every comparison is exact equality, NaN matching NaN."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import proximity_ref as pr
from machisplin_amd import _lib
from machisplin_amd import proximity as px
from machisplin_amd.raster import Geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def test_the_two_restatements_agree_on_random_grids():
    rng = np.random.default_rng(5)
    for _ in range(200):
        nrow, ncol = (int(x) for x in rng.integers(1, 25, 2))
        mask = rng.random((nrow, ncol)) < rng.choice([0.0, 0.02, 0.1, 0.5, 1.0])
        b, t = pr.brute(mask), pr.two_stage(mask)
        assert np.array_equal(b[0], t[0]) and np.array_equal(b[1], t[1]), (nrow, ncol)


def test_d2_equals_scipys_exact_euclidean_transform():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(6)
    for shape, density in (((300, 300), 1e-3), ((300, 211), 0.05), ((97, 300), 0.5), ((1, 300), 0.01), ((300, 1), 0.01)):
        mask = rng.random(shape) < density
        mask[rng.integers(0, shape[0]), rng.integers(0, shape[1])] = True
        d2, _ = pr.two_stage(mask)
        want = np.rint(ndi.distance_transform_edt(~mask) ** 2).astype(np.int64)
        assert np.array_equal(d2, want), shape


def test_hand_worked_tie_rule():
    # two features mirrored about the cell (2, 2): (0, 2) and (4, 2) are both 4 away -> the smaller row
    m = np.zeros((5, 5), bool); m[0, 2] = m[4, 2] = True
    d2, idx = pr.two_stage(m)
    assert d2[2, 2] == 4 and idx[2, 2] == 0 * 5 + 2
    assert idx[1, 2] == 2 and idx[3, 2] == 22                   # off the mirror line the nearer one wins
    # mirrored about the cell in its own row: the smaller column
    m = np.zeros((1, 7), bool); m[0, 1] = m[0, 5] = True
    d2, idx = pr.two_stage(m)
    assert d2[0].tolist() == [1, 0, 1, 4, 1, 0, 1] and idx[0].tolist() == [1, 1, 1, 1, 5, 5, 5]
    # four features at the same distance 5 from (2, 2): (0, 1) has the smallest cell number; (1, 0) is in a smaller row than (3, 4)
    m = np.zeros((5, 5), bool); m[0, 1] = m[1, 0] = m[3, 4] = m[4, 3] = True
    d2, idx = pr.two_stage(m)
    assert d2[2, 2] == 5 and idx[2, 2] == 1
    m[0, 1] = False
    assert pr.two_stage(m)[1][2, 2] == 5 and pr.brute(m)[1][2, 2] == 5       # (1, 0) = cell 5
    # a smaller row beats a smaller column: (0, 4) and (4, 0) are both 8 away from (2, 2)
    m = np.zeros((5, 5), bool); m[0, 4] = m[4, 0] = True
    assert pr.two_stage(m)[1][2, 2] == 4 and pr.brute(m)[1][2, 2] == 4


def test_hand_worked_predicates_with_an_na_cell():
    z = np.array([[1.0, 2.0, NAN, 3.0, -9.0]])
    want = {"na": [0, 0, 1, 0, 1], "valid": [1, 1, 0, 1, 0], "lt": [1, 0, 0, 0, 0], "le": [1, 1, 0, 0, 0], "gt": [0, 0, 0, 1, 0],
            "ge": [0, 1, 0, 1, 0], "eq": [0, 1, 0, 0, 0], "ne": [1, 0, 0, 1, 0]}
    for where, w in want.items():
        assert pr.features(z, -9.0, where, 2.0)[0].astype(int).tolist() == w, where
    assert pr.features(z, None, "na")[0].astype(int).tolist() == [0, 0, 1, 0, 0]        # without a nodata value -9 is a value
    assert pr.features(z.astype(np.float32), -9.0, "lt", 2.0)[0].tolist() == [True, False, False, False, False]


def test_hand_worked_products():
    # one feature at (1, 3) of a 4 x 5 grid, unit 30: cell (3, 0) is 2 rows south and 3 columns west of it
    z = np.arange(20.0).reshape(4, 5)
    p = pr.proximity(z, None, "eq", 8.0, unit=30.0, value_plane=z * 10.0)
    assert p["d2"][3, 0] == 13 and p["index"][3, 0] == 8
    assert p["dist"][3, 0] == np.sqrt(13.0) * 30.0
    assert p["dir_x"][3, 0] == 3.0 / np.sqrt(13.0) and p["dir_y"][3, 0] == 2.0 / np.sqrt(13.0)       # the feature lies east and NORTH
    assert p["dir_x"][0, 4] == -1.0 / np.sqrt(2.0) and p["dir_y"][0, 4] == -1.0 / np.sqrt(2.0)      # west and south
    assert p["dir_x"][1, 3] == 0.0 and p["dir_y"][1, 3] == 0.0 and p["dist"][1, 3] == 0.0 and p["d2"][1, 3] == 0
    assert (p["value"] == 80.0).all()
    assert p["dir_y"][0, 3] == -1.0 and p["dir_x"][1, 0] == 1.0
    # the value plane's NA at the nearest feature is NaN
    v = z * 10.0; v[1, 3] = -9.0
    assert np.isnan(pr.proximity(z, -9.0, "eq", 8.0, value_plane=v)["value"]).all()
    # float32: the float64 value converted once
    p32 = pr.proximity(z, None, "eq", 8.0, unit=30.0, value_plane=z, f32=True)
    assert p32["dist"].dtype == np.float32 and p32["dist"][3, 0] == np.float32(np.sqrt(13.0) * 30.0)


def test_hand_worked_no_feature():
    p = pr.proximity(np.ones((3, 4)), None, "na", value_plane=np.ones((3, 4)))
    assert (p["d2"] == -1).all() and (p["index"] == -1).all() and p["d2"].dtype == np.int32
    for k in ("dist", "dir_x", "dir_y", "value"):
        assert np.isnan(p[k]).all(), k
    for search in (pr.brute, pr.two_stage):
        d2, idx = search(np.zeros((2, 2), bool))
        assert (d2 == -1).all() and (idx == -1).all()


class _Call:
    """One of the two entry points on a 10 x 12 stack of two layers.  A refusal comes before the first device call and reads no
    plane.  The calls that PASS the checks end at MHS_ERR_NODEVICE on a machine without a GPU -- but where there is one they run,
    so the planes of the _dev entry are then device tensors (a kernel must never be handed a host address) and those of the
    host entry are the host arrays it is made for."""

    def __init__(self, fn):
        import torch
        self.lib = _lib.load()
        if fn.endswith("_dev") and torch.cuda.is_available():
            self.z = torch.zeros((2, 10, 12), dtype=torch.float32, device="cuda")
            self.planes = torch.zeros((6, 10, 12), dtype=torch.float64, device="cuda")
            self.zptr, self.pptr = self.z.data_ptr(), [self.planes[k].data_ptr() for k in range(6)]
        else:
            self.z = np.zeros((2, 10, 12), dtype=np.float32)
            self.planes = np.zeros((6, 10, 12))
            self.zptr, self.pptr = self.z.ctypes.data, [self.planes[k].ctypes.data for k in range(6)]
        self.stack = _lib.Stack(self.zptr, 2, _lib.F32, 120, 12, NAN)
        self.out = _lib.ProximityOut(*self.pptr)

    def __call__(self, fn, grid=(10, 12), stack="default", layer=0, where=0, threshold=0.0, value_layer=1, unit=1.0, out="default",
                 out_dtype=_lib.F64, ld=12):
        g = C.byref(_lib.Grid(0.0, 10.0, 1.0, 1.0, *grid)) if grid is not None else None
        s = C.byref(self.stack) if stack == "default" else stack
        o = C.byref(self.out) if out == "default" else out
        f = getattr(self.lib, fn)
        head = (g, s, layer, where, threshold, value_layer, unit, o, out_dtype)
        rc = f(*head, ld, None, None) if fn.endswith("_dev") else f(*head, None)
        return rc, self.lib.mhs_last_error().decode()


@pytest.mark.parametrize("fn", ("mhs_proximity_dev", "mhs_proximity"))
def test_refusals_of_the_library_come_before_any_device_call(fn):
    call = _Call(fn)

    def refused(needle, **kw):
        rc, msg = call(fn, **kw)
        assert rc == _lib.ERR_INVALID and needle in msg and fn in msg, (kw, rc, msg)

    refused("NULL", grid=None)
    refused("NULL", stack=None)
    refused("NULL", out=None)
    refused("data is NULL", stack=C.byref(_lib.Stack(None, 2, _lib.F32, 120, 12, NAN)))
    refused("nrow, ncol", grid=(0, 12))
    refused("nrow, ncol", grid=(10, -1))
    refused("(nrow - 1)^2 + (ncol - 1)^2", grid=(1, 50000))                   # 49 999^2 passes the int32
    refused("(nrow - 1)^2 + (ncol - 1)^2", grid=(46342, 2))
    refused("(nrow - 1)^2 + (ncol - 1)^2", grid=(32768, 65536))               # nrow * ncol <= INT32_MAX follows from this limit
    refused("bad stack dtype", stack=C.byref(_lib.Stack(call.zptr, 2, 7, 120, 12, NAN)))
    refused("layer", layer=2)
    refused("layer", layer=-1)
    refused("strides", stack=C.byref(_lib.Stack(call.zptr, 2, _lib.F32, 120, 11, NAN)))
    refused("strides", stack=C.byref(_lib.Stack(call.zptr, 2, _lib.F32, 119, 12, NAN)))
    refused("where", where=8)
    refused("where", where=-1)
    refused("threshold", where=2, threshold=NAN)
    for bad in (0.0, -1.0, NAN, float("inf")):
        refused("unit", unit=bad)
    refused("no product", out=C.byref(_lib.ProximityOut()))
    refused("value_layer", value_layer=2)
    refused("value_layer", value_layer=-1)
    for bad in (_lib.I16, 5, -1):
        refused("out_dtype", out_dtype=bad)
    if fn.endswith("_dev"):
        refused("ld smaller", ld=11)
    # value_layer is looked at only when the value plane is asked for; NaN is a threshold like any other for na / valid
    only_dist = _lib.ProximityOut(None, None, call.pptr[2], None, None, None)
    for kw in (dict(value_layer=-1, out=C.byref(only_dist)), dict(threshold=NAN, where=1), dict()):
        rc, msg = call(fn, **kw)
        assert rc in (_lib.OK, _lib.ERR_NODEVICE), (kw, msg)
    for where in range(8):
        rc, msg = call(fn, where=where)
        assert rc in (_lib.OK, _lib.ERR_NODEVICE), (where, msg)


def _fake(nrow=10, ncol=12, xres=1.0, yres=1.0, n_layers=2):
    """what proximity() looks at before its first device call; touching the planes would be one"""
    class Stack:
        geom = Geometry(0.0, nrow * yres, xres, yres, nrow, ncol)
        nodata = NAN

        @property
        def planes(self):
            raise AssertionError("the planes were touched before the refusal")
    s = Stack()
    s.n_layers = n_layers
    return s


def test_refusals_of_the_python_call_come_before_any_device_call():
    def refused(needle, *a, **kw):
        with pytest.raises(ValueError, match=needle):
            px.proximity(*a, **kw)

    refused(r"\(nrow - 1\)\^2 \+ \(ncol - 1\)\^2", _fake(1, 50000))
    refused("unit.*not square.*resample", _fake(xres=30.0, yres=30.0001))
    refused("unit", _fake(), unit=0.0)
    refused("unit", _fake(), unit=-2.0)
    refused("unit", _fake(), unit=float("inf"))
    refused("unit", _fake(), unit=NAN)
    refused("where", _fake(), where="near")
    refused("threshold", _fake(), where="le")
    refused("threshold", _fake(), where="le", threshold=NAN)
    refused("value_layer", _fake(), products=("dist", "value"))
    refused("value_layer", _fake(), products="value", value_layer=2)
    refused("products", _fake(), products=())
    refused("products", _fake(), products=("dist", "dist"))
    refused("product", _fake(), products=("distance",))
    refused("layer", _fake(), layer=2)
    refused("out_dtype", _fake(), out_dtype=np.float32)
    import torch
    refused("tensor", torch.zeros((3, 3)))                       # a float tensor is no tensor of flags
    refused("tensor", torch.zeros((2, 3, 3), dtype=torch.bool))
    # an explicit unit skips the square-cell check: the call then goes on to the planes
    with pytest.raises(AssertionError, match="planes were touched"):
        px.proximity(_fake(xres=30.0, yres=31.0), unit=30.0)
    with pytest.raises(AssertionError, match="planes were touched"):
        px.proximity(_fake(xres=30.0, yres=30.0 * (1 + 5e-10)))


def _lcg_plane(k, nrow, ncol):
    state = 1000 + k
    z = np.empty(nrow * ncol)
    for i in range(nrow * ncol):
        state = (state * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        q = (state >> 33) % 23
        z[i] = NAN if q == 0 else -9.0 if q == 1 else float(q - 1) if q < 4 else 3.0
    return z.reshape(nrow, ncol)


def _bits(a):
    a = np.where(np.isnan(a), np.float64(np.nan), a).astype(np.float64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = np.uint64(0x7ff8000000000000)
    return b


def test_rule_header_in_a_plain_cpp_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "proximity_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "machisplin_amd", "csrc"),
           os.path.join(ROOT, "tests", "proximity_check.cpp"), "-o", exe]
    run = subprocess.run(cmd, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    run = subprocess.run([exe], capture_output=True, text=True)       # stand-alone: the sanitizer runtimes are linked into it
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().split("\n")
    assert lines[-1] == "OK"
    n_div = n_take = n_case = 0
    for ln in lines[:-1]:
        w = ln.split()
        if w[0] == "floor_div":
            a, b, q = (int(x) for x in w[1:])
            assert q == a // b, ln
            n_div += 1
        elif w[0] == "takeover":
            i, hi, u, hu, t = (int(x) for x in w[1:])
            nearer = lambda r: (r - u) ** 2 + hu < (r - i) ** 2 + hi          # noqa: E731
            assert nearer(t) and not nearer(t - 1), ln                          # the FIRST row at which the later row is strictly nearer
            n_take += 1
        elif w[0] == "compare":
            assert int(w[1]) == 70, ln                                          # w > f <=> n >= f d at the seven f around each w
        else:
            k, nrow, ncol, where, got = (int(x) for x in w[1:])
            z = _lcg_plane(k, nrow, ncol)
            p = pr.proximity(z, -9.0, pr.WHERE[where], 2.0, unit=2.5, value_plane=z)
            x = np.stack([p["d2"].astype(np.int64).view(np.uint64), p["index"].astype(np.int64).view(np.uint64), _bits(p["dist"]),
                          _bits(p["dir_x"]), _bits(p["dir_y"]), _bits(p["value"])], axis=-1).ravel()
            with np.errstate(over="ignore"):
                want = int((x * (2 * np.arange(x.size, dtype=np.uint64) + 1)).sum(dtype=np.uint64))
            assert got == want, ln
            assert same(pr.brute(pr.features(z, -9.0, pr.WHERE[where], 2.0))[1].astype(np.int32), p["index"]), ln
            n_case += 1
    assert n_div == 40 and n_take == 10 and n_case == 64
