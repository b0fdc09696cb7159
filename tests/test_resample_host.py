"""CPU: the resampling rules (include/machisplin_hip.h, section "resample").  The numpy restatement the GPU tests compare with
(tests/resample_ref.py) is itself checked against hand-computed values; every entry point refuses bad arguments with
MHS_ERR_INVALID before it touches a device; and the rule header the kernels are built from (csrc/resample_rule.h) gives the
same table in a plain C++ program compiled with gcc under AddressSanitizer + UBSan and run stand-alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import resample_ref as rr
from machisplin_amd import _lib
from machisplin_amd.raster import Geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")

S3 = Geometry(0.0, 3.0, 1.0, 1.0, 3, 3)
Z3 = np.array([[1.0, 2, 3], [4, 5, 6], [7, 8, 10]])
Z3NA = Z3.copy(); Z3NA[1, 2] = np.nan
S4 = Geometry(0.0, 4.0, 1.0, 1.0, 4, 4)
Z4 = np.tile(np.array([0.0, 1.0, 4.0, 9.0]), (4, 1))

# Worked by hand.  The point (1.75, 1.25) lies a quarter cell east and a quarter cell south of the centre (1.5, 1.5) of cell
# (1, 1) of the 3 x 3 plane 1 2 3 / 4 5 6 / 7 8 10:
#   fx = 1.75 / 1 - 0.5 = 1.25, j0 = 1, tx = 0.25; fy = (3 - 1.25) / 1 - 0.5 = 1.25, i0 = 1, ty = 0.25
#   w = 0.75 * 0.75, 0.75 * 0.25, 0.25 * 0.75, 0.25 * 0.25 = 0.5625, 0.1875, 0.1875, 0.0625 on z = 5, 6, 8, 10
#   num = 2.8125 + 1.125 + 1.5 + 0.625 = 6.0625, den = 1
#   with cell (1, 2) = 6 NA: num = 2.8125 + 1.5 + 0.625 = 4.9375, den = 0.8125, value 79 / 13
#   cubic there needs row 3 and column 3, which the plane does not have, with weights that are not 0: the bilinear value
# Cubic at t = 0.5: ((-0.25 + 1) 0.5 - 0.5) 0.5 = -1/16, ((0.75 - 2.5) 0.5) 0.5 + 1 = 9/16, ((-0.75 + 2) 0.5 + 0.5) 0.5 = 9/16,
#   ((0.25 - 0.5) 0.5) 0.5 = -1/16; on a row 0 1 4 9: -1/16 + 36/16 - 9/16 = 2.25 -- what x^2 gives at 1.5 -- and four such
#   rows under the same weights give 2.25 again; bilinear there is (1 + 4) / 2.
# Footprints of 10 unit columns under 3 columns of width 10 / 3: the edges 0, 3.33, 6.67, 10 give ceil(-0.5) = 0,
#   ceil(2.83) = 3, ceil(6.17) = 7, ceil(9.5) = 10: {0 1 2}, {3 4 5 6}, {7 8 9}, a partition of 0 .. 9.
# The 3 x 3 plane with (1, 2) NA under ONE target cell: row sums 6, 9, 25 -> 40 of 8 cells, mean 5, min 1, max 10.
HAND = {"bilinear_quarter": 6.0625, "cubic_fallback": 6.0625, "near_quarter": 5.0, "near_east_edge": 6.0, "near_south_edge": 7.0,
        "outside_is_na": 1.0, "bilinear_na_tap": 4.9375 / 0.8125, "bilinear_na_weight0": 5.0,
        "cubic_w0": -0.0625, "cubic_w1": 0.5625, "cubic_w2": 0.5625, "cubic_w3": -0.0625, "cubic_half": 2.25, "bilinear_half": 2.5,
        "foot_0": 0.0, "foot_1": 3.0, "foot_2": 7.0, "foot_3": 10.0,
        "agg_mean": 5.0, "agg_min": 1.0, "agg_max": 10.0, "agg_sum": 40.0, "agg_count": 8.0,
        "agg_empty_mean_is_na": 1.0, "agg_empty_count": 0.0, "agg_fine_hit": 5.0, "identity": 1.0}


def _at(z, S, method, x, y):
    return float(rr.extract(z, NAN, S, [[x, y]], method)[0])


def test_restatement_bilinear_cubic_and_near_give_the_hand_computed_values():
    assert _at(Z3, S3, "bilinear", 1.75, 1.25) == HAND["bilinear_quarter"]
    assert _at(Z3, S3, "cubic", 1.75, 1.25) == HAND["cubic_fallback"]
    assert _at(Z3, S3, "simple", 1.75, 1.25) == 5.0 and _at(Z3, S3, "near", 3.0, 1.5) == 6.0 and _at(Z3, S3, "near", 0.5, 0.0) == 7.0
    assert np.isnan(_at(Z3, S3, "bilinear", 3.0000001, 1.5)) and np.isnan(_at(Z3, S3, "near", 1.0, -0.1))
    assert [float(w) for w in rr.cubic_weights(np.float64(0.5))] == [-0.0625, 0.5625, 0.5625, -0.0625]
    assert _at(Z4, S4, "cubic", 2.0, 2.0) == 2.25 and _at(Z4, S4, "bilinear", 2.0, 2.0) == 2.5


def test_restatement_an_na_tap_renormalises_and_one_of_weight_zero_does_not_poison():
    assert _at(Z3NA, S3, "bilinear", 1.75, 1.25) == 4.9375 / 0.8125
    assert _at(Z3NA, S3, "bilinear", 1.5, 1.5) == 5.0 and _at(Z3NA, S3, "cubic", 1.5, 1.5) == 5.0
    assert np.isnan(_at(Z3NA, S3, "near", 2.5, 1.5))
    # the nodata value is NA as NaN is
    zi = Z3.astype(np.int16); zi[1, 2] = -32768
    assert float(rr.extract(zi, -32768.0, S3, [[1.75, 1.25]], "bilinear")[0]) == 4.9375 / 0.8125


def test_restatement_footprints_partition_the_source():
    S10, T3 = Geometry(0.0, 1.0, 1.0, 1.0, 1, 10), Geometry(0.0, 1.0, 10.0 / 3.0, 1.0, 1, 3)
    assert rr.foot_cols(S10, T3, np.arange(4)).tolist() == [0, 3, 7, 10]
    # shifted and 3.7 x coarser: footprints of 3 and 4 that vary, still a partition of the columns they cover
    T = Geometry(-1.3, 1.0, 3.7, 1.0, 1, 4)
    e = rr.foot_cols(S10, T, np.arange(5))
    assert e[0] == 0 and (np.diff(e) >= 0).all() and set(np.diff(e)[1:3]) <= {3, 4} and e[-1] == 10
    src = np.arange(10.0)[None]
    cnt = rr.resample(src, NAN, S10, T, "count")
    assert cnt.sum() == 10 and rr.resample(src, NAN, S10, T, "sum").sum() == 45.0


def test_restatement_aggregates_with_an_na_and_empty_footprints():
    T1 = Geometry(0.0, 3.0, 3.0, 3.0, 1, 1)
    for m in ("mean", "min", "max", "sum", "count"):
        assert float(rr.resample(Z3NA, NAN, S3, T1, m)[0, 0]) == HAND["agg_" + m], m
    Tf = Geometry(0.0, 3.0, 0.25, 0.25, 12, 12)                     # finer than the source: most footprints are empty
    mean, cnt, sm = (rr.resample(Z3, NAN, S3, Tf, m) for m in ("mean", "count", "sum"))
    assert np.isnan(mean[0, 0]) and cnt[0, 0] == 0.0 and sm[0, 0] == 0.0 and mean[6, 6] == 5.0
    assert cnt.sum() == 9 and (~np.isnan(mean)).sum() == 9


def test_restatement_is_the_identity_on_the_same_grid():
    for m in ("near", "bilinear", "cubic", "mean", "min", "max"):
        assert np.array_equal(rr.resample(Z3NA, NAN, S3, S3, m), Z3NA, equal_nan=True), m
    assert np.array_equal(rr.resample(Z3NA, NAN, S3, S3, "count"), (~np.isnan(Z3NA)).astype(float))
    assert np.array_equal(rr.resample(Z3, NAN, S3, S3, "bilinear", window=(1, 3, 0, 2)), Z3[1:3, 0:2])


class _Call:
    """the four entry points on HOST arrays that are never read: every refusal comes before the first device call"""

    def __init__(self):
        self.lib = _lib.load()
        self.src = _lib.Grid(0.0, 10.0, 1.0, 1.0, 10, 12)
        self.dst = _lib.Grid(0.5, 9.0, 2.0, 2.0, 4, 5)
        self.z = np.zeros((2, 10, 12), dtype=np.float32)
        self.stack = _lib.Stack(self.z.ctypes.data, 2, _lib.F32, 120, 12, NAN)
        self.out = np.zeros((2, 4, 5))
        self.xy = np.zeros((2, 7))
        self.pout = np.zeros((2, 7))

    def __call__(self, fn, src="default", stack="default", dst="default", window=(0, 4, 0, 5), method=1, out="default", out_dtype=_lib.F64,
                 ld=5, plane_stride=20, xy="default", n=7):
        g = C.byref(self.src) if src == "default" else src
        s = C.byref(self.stack) if stack == "default" else stack
        f = getattr(self.lib, fn)
        if "resample" in fn:
            t = C.byref(self.dst) if dst == "default" else dst
            o = self.out.ctypes.data if out == "default" else out
            rc = f(g, s, t, *window, method, o, ld, plane_stride, out_dtype, None) if fn.endswith("_dev") else f(g, s, t, *window, method, o, out_dtype)
        else:
            o = self.pout.ctypes.data if out == "default" else out
            p = self.xy.ctypes.data if xy == "default" else xy
            rc = f(g, s, p, n, method, o, None) if fn.endswith("_dev") else f(g, s, p, n, method, o)
        return rc, self.lib.mhs_last_error().decode()


ALL = ("mhs_resample_dev", "mhs_resample", "mhs_extract_points_dev", "mhs_extract_points")


@pytest.mark.parametrize("fn", ALL)
def test_refusals_come_before_any_device_call(fn):
    call = _Call()
    grid = "resample" in fn

    def refused(needle, **kw):
        rc, msg = call(fn, **kw)
        assert rc == _lib.ERR_INVALID and needle in msg and fn in msg, (kw, rc, msg)

    refused("NULL", src=None)
    refused("NULL", stack=None)
    refused("data is NULL", stack=C.byref(_lib.Stack(None, 2, _lib.F32, 120, 12, NAN)))
    refused("NULL", out=None)
    refused("bad stack dtype", stack=C.byref(_lib.Stack(call.z.ctypes.data, 2, 7, 120, 12, NAN)))
    refused("strides", stack=C.byref(_lib.Stack(call.z.ctypes.data, 2, _lib.F32, 120, 11, NAN)))
    refused("strides", stack=C.byref(_lib.Stack(call.z.ctypes.data, 2, _lib.F32, 119, 12, NAN)))
    refused("no layer", stack=C.byref(_lib.Stack(call.z.ctypes.data, 0, _lib.F32, 120, 12, NAN)))
    for bad in (0.0, -1.0, NAN, float("inf")):
        refused("source grid's cell size", src=C.byref(_lib.Grid(0.0, 10.0, bad, 1.0, 10, 12)))
        refused("source grid's cell size", src=C.byref(_lib.Grid(0.0, 10.0, 1.0, bad, 10, 12)))
    refused("source grid dimension", src=C.byref(_lib.Grid(0.0, 10.0, 1.0, 1.0, 0, 12)))
    refused("source grid dimension", src=C.byref(_lib.Grid(0.0, 10.0, 1.0, 1.0, 10, -3)))
    refused("origin", src=C.byref(_lib.Grid(NAN, 10.0, 1.0, 1.0, 10, 12)))
    refused("unknown method", method=8)
    refused("unknown method", method=-1)
    if grid:
        refused("NULL", dst=None)
        refused("target grid's cell size", dst=C.byref(_lib.Grid(0.5, 9.0, 0.0, 2.0, 4, 5)))
        refused("target grid's cell size", dst=C.byref(_lib.Grid(0.5, 9.0, 2.0, NAN, 4, 5)))
        refused("target grid dimension", dst=C.byref(_lib.Grid(0.5, 9.0, 2.0, 2.0, 4, 0)))
        for w in ((0, 5, 0, 5), (0, 4, 2, 6), (3, 2, 0, 5), (-1, 4, 0, 5)):
            refused("window outside the target", window=w)
        for bad in (_lib.I16, 5, -1):
            refused("out_dtype", out_dtype=bad)
        if fn.endswith("_dev"):
            refused("out_ld smaller", ld=4)
            refused("out_plane_stride", plane_stride=19)
        for m in range(8):                               # every method passes the checks
            rc, msg = call(fn, method=m, window=(1, 1, 2, 2))
            assert rc in (_lib.OK, _lib.ERR_NODEVICE), (m, msg)
    else:
        for m in range(3, 8):
            refused("aggregate method", method=m)
        refused("NULL", xy=None)
        refused("n is negative", n=-1)
        rc, msg = call(fn, n=0, xy=None, out=None)       # nothing to do needs no arrays
        assert rc in (_lib.OK, _lib.ERR_NODEVICE), msg


def test_rule_header_in_a_plain_cpp_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "resample_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "machisplin_amd", "csrc"),
           os.path.join(ROOT, "tests", "resample_check.cpp"), "-o", exe]
    pr = subprocess.run(cmd, capture_output=True, text=True)
    assert pr.returncode == 0, pr.stderr
    pr = subprocess.run([exe], capture_output=True, text=True)       # stand-alone: the sanitizer runtimes are linked into it
    assert pr.returncode == 0, pr.stdout + pr.stderr
    lines = pr.stdout.split("\n")
    assert lines[len(HAND)] == "OK"
    got = {ln.split()[0]: float(ln.split()[1]) for ln in lines[:len(HAND)]}
    assert got.keys() == HAND.keys()
    for name, want in HAND.items():
        assert got[name] == float(want), (name, got[name], want)
