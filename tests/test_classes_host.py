"""CPU: the rule of include/machisplin_hip.h, section "classes".  The numpy restatement (classes_ref) against plain Python loops
with collections.Counter for the three units, hand-worked cases with ties, the restatement against resample_ref and focal_ref
where the units are theirs, every refusal of the Python calls and of the C entries before any device call, and
classes_rule.h in a plain C++ program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import classes_ref as cr
import focal_ref as fr
import resample_ref as rr
from machisplin_amd import _lib
from machisplin_amd import classes as cl
from machisplin_amd.raster import Geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def land_cover(seed, shape, codes, dtype=np.float32, nodata=NAN, p_na=0.1, p_other=0.1):
    """a plane of the given codes with NA cells and `other` cells (an unlisted code, a half, a negative, a huge value)"""
    rng = np.random.default_rng(seed)
    z = rng.choice(np.asarray(codes), size=shape).astype(np.float64)
    if dtype == np.int16:
        stray = rng.choice(np.array([-5.0, 32000.0, 777.0]), size=shape)
    else:
        stray = rng.choice(np.array([0.5, -3.0, 70000.0, 65534.5, np.inf, 777.0]), size=shape)
    z = np.where(rng.random(shape) < p_other, stray, z)
    z = np.where(rng.random(shape) < p_na, -32768.0 if nodata == nodata else np.nan, z)
    return z.astype(dtype)


def check_units(planes_or_table, loop, classes, unit_ids, at):
    """the restatement's values of the units `unit_ids` (found at `at(u)`) against the loop's Counter per unit"""
    for u in unit_ids:
        counter, other, _ = loop.get(u, (Counter(), 0, 0))
        n, mode, mode_frac, variety, simpson, fracs = cr.loop_finish(counter, other, classes)
        i = at(u)
        assert planes_or_table["n"][i] == n and planes_or_table["mode"][i] == mode and planes_or_table["variety"][i] == variety, u
        assert bits_equal(planes_or_table["mode_frac"][i], mode_frac) and bits_equal(planes_or_table["simpson"][i], simpson), u
        assert bits_equal(np.array([planes_or_table["frac"][(j,) + i] if isinstance(i, tuple) else planes_or_table["frac"][i, j] for j in range(len(fracs))]),
                          np.array(fracs)), u


@pytest.mark.parametrize("dtype,nodata", [(np.float32, NAN), (np.int16, -32768.0), (np.float64, -32768.0)])
def test_the_restatement_of_crosstab_equals_a_plain_loop(dtype, nodata):
    classes = [41, 11, 90, 42]
    z = land_cover(1, (23, 37), classes + [21], dtype, nodata)
    zones = np.random.default_rng(2).integers(-1, 7, size=z.shape).astype(np.int32)
    table, planes, info = cr.crosstab(z, zones, classes, nodata, n_zones=8)
    loop = cr.loop_units(z, zones, classes, nodata)
    assert info["n_zones"] == 8 and len(table["n"]) == 8
    for u in range(8):
        counter, other, na = loop.get(u, (Counter(), 0, 0))
        assert [int(c) for c in table["counts"][u]] == [counter.get(c, 0) for c in sorted(classes)]
        assert table["other"][u] == other and table["cells"][u] == sum(counter.values()) + other + na == int((zones == u).sum())
    check_units(table, loop, classes, range(8), lambda u: u)
    # the planes carry the table's rows; -1 and NaN off the zones
    off = zones < 0
    assert off.any() and np.all(planes["mode"][off] == -1) and np.all(planes["n"][off] == -1) and np.all(np.isnan(planes["frac"][:, off]))
    on = ~off
    assert np.array_equal(planes["mode"][on], table["mode"][zones[on]]) and bits_equal(planes["simpson"][on], table["simpson"][zones[on]])
    assert bits_equal(planes["frac"][2][on], table["frac"][zones[on], 2])
    # the info, and the measured list
    zz, ok = cr.valid(z, nodata)
    assert info["n_valid"] == int(ok.sum()) and info["n_na"] == int((~ok).sum()) and info["K"] == 4 and info["codes"] == sorted(classes)
    assert info["n_other"] == sum(v[1] for v in cr.loop_units(z, np.zeros(z.shape, dtype=int), classes, nodata).values())
    want = sorted(set(int(v) for v, good in zip(zz.ravel(), ok.ravel()) if good and 0 <= v <= 65535 and v == int(v)))
    assert cr.measure(z, nodata) == want and 21 in want
    t2, _, i2 = cr.crosstab(z, zones, None, nodata)
    assert i2["codes"] == want and i2["n_zones"] == int(zones.max()) + 1
    k = [want.index(c) for c in sorted(classes)]
    assert np.array_equal(t2["counts"][:, k], table["counts"][:i2["n_zones"]])


def test_the_restatement_of_aggregate_equals_a_plain_loop_and_resample_ref():
    classes = [1, 2, 5]
    S = Geometry(10.0, 50.0, 0.1, 0.1, 41, 53)
    z = land_cover(3, (S.nrow, S.ncol), classes, np.float32)
    for T in (Geometry(10.037, 49.9, 0.25, 0.25, 14, 19), Geometry(9.0, 51.0, 0.3, 0.3, 20, 25), Geometry(10.0, 50.0, 0.04, 0.04, 30, 30)):
        planes, _ = cr.aggregate(z, S, T, classes)
        # the unit of a source cell by the rule's words: the target cell that holds its centre, through the footprints' edges
        unit = np.full(z.shape, -1)
        ce, re = rr.foot_cols(S, T, np.arange(T.ncol + 1)), rr.foot_rows(S, T, np.arange(T.nrow + 1))
        for r in range(T.nrow):
            for c in range(T.ncol):
                unit[re[r]:re[r + 1], ce[c]:ce[c + 1]] = r * T.ncol + c
        loop = cr.loop_units(z, unit, classes)
        check_units(planes, loop, classes, range(T.nrow * T.ncol), lambda u: divmod(u, T.ncol))
        # n is resample's count, frac its mean of the indicator, bit for bit
        count = rr.resample(z, NAN, S, T, "count")
        assert np.array_equal(planes["n"], count.astype(np.int32))
        zz, ok = cr.valid(z)
        for j, code in enumerate(sorted(classes)):
            ind = np.where(ok, (zz == code).astype(np.float64), np.nan)
            assert bits_equal(planes["frac"][j], rr.resample(ind, NAN, S, T, "mean"))
        assert (planes["n"] == 0).any() or T.xres > 0.2       # the finer and the partly outside targets have empty footprints
        empty = planes["n"] == 0
        assert np.all(planes["mode"][empty] == -1) and np.all(planes["variety"][empty] == 0) and np.all(np.isnan(planes["simpson"][empty]))


@pytest.mark.parametrize("shape,R", [("square", 1), ("square", 5), ("circle", 1), ("circle", 6), ("square", 40)])
def test_the_restatement_of_focal_equals_a_plain_loop_and_focal_ref(shape, R):
    classes = [3, 4, 9]
    z = land_cover(4, (17, 29), classes, np.int16, -32768.0)
    planes, _ = cr.focal(z, R, classes, -32768.0, shape=shape)
    zz, ok = cr.valid(z, -32768.0)
    for r in range(z.shape[0]):
        for c in range(z.shape[1]):
            if not ok[r, c]:
                assert planes["mode"][r, c] == -1 and planes["n"][r, c] == -1 and np.isnan(planes["frac"][:, r, c]).all() and np.isnan(planes["mode_frac"][r, c])
                continue
            counter, other = Counter(), 0
            for dr in range(-R, R + 1):
                w = R if shape == "square" else fr.half_width(R, abs(dr))
                for dc in range(-w, w + 1):
                    i, j = r + dr, c + dc
                    if 0 <= i < z.shape[0] and 0 <= j < z.shape[1] and ok[i, j]:
                        if zz[i, j] in classes:
                            counter[int(zz[i, j])] += 1
                        else:
                            other += 1
            n, mode, mode_frac, variety, _, fracs = cr.loop_finish(counter, other, classes)
            assert (planes["n"][r, c], planes["mode"][r, c], planes["variety"][r, c]) == (n, mode, variety), (r, c)
            assert bits_equal(planes["mode_frac"][r, c], mode_frac) and bits_equal(planes["frac"][:, r, c], np.array(fracs))
    for j, code in enumerate(sorted(classes)):
        ind = np.where(ok, (zz == code).astype(np.int16), -1).astype(np.int16)
        assert bits_equal(planes["frac"][j], fr.focal(ind, -1.0, R, ("mean",), shape=shape, offset=0.0)[0])
    assert np.array_equal(np.where(ok, planes["n"], 0), np.where(ok, fr.focal(z, -32768.0, R, ("count",), shape=shape)[0], 0).astype(np.int32))


def test_hand_worked_cases():
    z = np.array([[1, 1, 2, 2],
                  [1, 2, 2, 7],
                  [3, 3, NAN, 0.5]])
    zones = np.array([[0, 0, 0, 0],
                      [1, 1, 1, 1],
                      [2, 2, 2, -1]], dtype=np.int32)
    table, planes, info = cr.crosstab(z, zones, [3, 2, 1], n_zones=4)
    assert table["counts"].tolist() == [[2, 2, 0], [1, 2, 0], [0, 0, 2], [0, 0, 0]]
    assert table["n"].tolist() == [4, 4, 2, 0] and table["other"].tolist() == [0, 1, 0, 0] and table["cells"].tolist() == [4, 4, 3, 0]
    assert table["mode"].tolist() == [1, 2, 3, -1]                          # zone 0 is a tie of 1 and 2: the smaller code
    assert table["variety"].tolist() == [2, 2, 1, 0]
    assert bits_equal(table["mode_frac"], [0.5, 0.5, 1.0, NAN])
    assert bits_equal(table["simpson"], [(16 - 8) / 16, (16 - 1 - 4 - 1) / 16, 0.0, NAN])
    assert bits_equal(table["frac"], [[0.5, 0.5, 0.0], [0.25, 0.5, 0.0], [0.0, 0.0, 1.0], [NAN] * 3])
    assert info == {"K": 3, "codes": [1, 2, 3], "n_valid": 11, "n_na": 1, "n_other": 2, "n_zones": 4}
    assert planes["mode"].tolist() == [[1] * 4, [2] * 4, [3, 3, 3, -1]]
    # frac_of picks and orders the columns; a tie of three goes to the smallest, whatever the order of the list
    t2, _, _ = cr.crosstab(np.array([[9.0, 4.0, 6.0]]), np.zeros((1, 3), dtype=np.int32), [9, 6, 4], frac_of=(6, 9))
    assert t2["mode"].tolist() == [4] and bits_equal(t2["frac"], [[1 / 3, 1 / 3]]) and bits_equal(t2["simpson"], [6 / 9])
    # only `other`: n counts them, no listed class occurs
    t3, _, _ = cr.crosstab(np.array([[8.0, 8.5]]), np.zeros((1, 2), dtype=np.int32), [1])
    assert t3["n"].tolist() == [2] and t3["mode"].tolist() == [-1] and np.isnan(t3["mode_frac"][0]) and t3["simpson"].tolist() == [0.0]
    assert t3["frac"].tolist() == [[0.0]]
    # aggregate by 2: the 2 x 2 blocks
    S, T = Geometry(0.0, 4.0, 1.0, 1.0, 4, 4), Geometry(0.0, 4.0, 2.0, 2.0, 2, 2)
    lc = np.array([[1, 1, 2, 2], [1, 5, 2, 3], [NAN, NAN, 3, 2], [NAN, NAN, 2, 3]])
    p, _ = cr.aggregate(lc, S, T, [1, 2, 3])
    assert p["mode"].tolist() == [[1, 2], [-1, 2]] and p["n"].tolist() == [[4, 4], [0, 4]] and p["variety"].tolist() == [[1, 2], [0, 2]]
    assert bits_equal(p["mode_frac"], [[0.75, 0.75], [NAN, 0.5]]) and bits_equal(p["simpson"], [[(16 - 9 - 1) / 16, (16 - 9 - 1) / 16], [NAN, 0.5]])
    # a window of radius 1 on a row
    f, _ = cr.focal(np.array([[1.0, 2.0, 2.0, NAN, 1.0]]), 1, [1, 2])
    assert f["n"].tolist() == [[2, 3, 2, -1, 1]] and f["mode"].tolist() == [[1, 2, 2, -1, 1]]
    assert bits_equal(f["frac"], [[[0.5, 1 / 3, 0.0, NAN, 1.0]], [[0.5, 2 / 3, 1.0, NAN, 0.0]]])


class _Call:
    """the C entries with arguments that pass every check; host arrays, or device tensors for a _dev entry where there is a GPU"""

    def __init__(self, fn):
        import torch
        self.lib = _lib.load()
        self.fn = fn
        dev = fn.endswith("_dev") and torch.cuda.is_available()
        mk = (lambda shape, dt: torch.zeros(shape, dtype=getattr(torch, dt), device="cuda")) if dev else (lambda shape, dt: np.zeros(shape, dtype=dt))
        ptr = (lambda t: t.data_ptr()) if dev else (lambda a: a.ctypes.data)
        self.z, self.zones = mk((2, 10, 12), "float32"), mk((10, 12), "int32")
        self.ti, self.td, self.pi, self.pd = mk((6, 16 * 4), "int32"), mk((3, 16 * 4), "float64"), mk((3, 10, 12), "int32"), mk((6, 10, 12), "float64")
        self.zptr, self.qptr = ptr(self.z), ptr(self.zones)
        self.stack = _lib.Stack(self.zptr, 2, _lib.F32, 120, 12, NAN)
        self.table = _lib.ClassTable(16, *[ptr(self.ti[k]) for k in range(6)], *[ptr(self.td[k]) for k in range(3)])
        self.planes = _lib.ClassPlanes(*[ptr(self.pi[k]) for k in range(3)], ptr(self.pd[0]), ptr(self.pd[1]), ptr(self.pd[2]), 12, 120, _lib.F64)
        if "focal" in fn:
            self.planes.simpson = None
        self.info = _lib.ClassInfo()

    def __call__(self, grid=(10, 12), stack="default", layer=0, zones="default", ld_zones=12, n_zones=5, classes=(1, 2, 3, 4), n_classes=None,
                 frac_of=(), table="default", planes="default", info=None, dst=(5, 6), radius=2, shape=0):
        g = C.byref(_lib.Grid(0.0, 10.0, 1.0, 1.0, *grid)) if grid is not None else None
        t = C.byref(_lib.Grid(0.0, 10.0, 2.0, 2.0, *dst)) if dst is not None else None
        s = C.byref(self.stack) if stack == "default" else stack
        q = self.qptr if zones == "default" else zones
        tab = C.byref(self.table) if table == "default" else table
        p = C.byref(self.planes) if planes == "default" else planes
        cls = (C.c_int32 * len(classes))(*classes) if classes else None
        nk = len(classes or ()) if n_classes is None else n_classes
        fo = (C.c_int32 * len(frac_of))(*frac_of) if frac_of else None
        f = getattr(self.lib, self.fn)
        if self.fn == "mhs_class_crosstab_dev":
            rc = f(g, s, layer, q, ld_zones, n_zones, cls, nk, fo, len(frac_of), tab, p, None, info)
        elif self.fn == "mhs_class_crosstab":
            rc = f(g, s, layer, q, n_zones, cls, nk, fo, len(frac_of), tab, p, info)
        elif self.fn == "mhs_class_aggregate_dev":
            rc = f(g, s, layer, t, cls, nk, fo, len(frac_of), p, None, info)
        elif self.fn == "mhs_class_aggregate":
            rc = f(g, s, layer, t, cls, nk, fo, len(frac_of), p, info)
        else:
            rc = f(g, s, layer, radius, shape, cls, nk, fo, len(frac_of), p, None, info)
        return rc, self.lib.mhs_last_error().decode()


ENTRIES = ("mhs_class_crosstab_dev", "mhs_class_crosstab", "mhs_class_aggregate_dev", "mhs_class_aggregate", "mhs_class_focal_dev")


@pytest.mark.parametrize("fn", ENTRIES)
def test_refusals_of_the_library_come_before_any_device_call(fn):
    call = _Call(fn)

    def refused(needle, **kw):
        rc, msg = call(**kw)
        assert rc == _lib.ERR_INVALID and needle in msg and fn in msg, (kw, rc, msg)

    refused("NULL", grid=None)
    refused("NULL", stack=None)
    refused("NULL", stack=C.byref(_lib.Stack(None, 2, _lib.F32, 120, 12, NAN)))
    refused("nrow, ncol", grid=(0, 12))
    refused("bad stack dtype", stack=C.byref(_lib.Stack(call.zptr, 2, 7, 120, 12, NAN)))
    refused("layer", layer=2)
    refused("layer", layer=-1)
    refused("strides", stack=C.byref(_lib.Stack(call.zptr, 2, _lib.F32, 120, 11, NAN)))
    # the class list
    refused("K must be in 1 .. 256", classes=tuple(range(257)))
    refused("K = 0 is no list", classes=(1,), n_classes=0)
    refused("K must be in 1 .. 256", classes=(1,), n_classes=-1)
    refused("must be in 0 .. 65535", classes=(1, -1))
    refused("must be in 0 .. 65535", classes=(65536, 2))
    refused("twice", classes=(4, 2, 4))
    refused("frac_of[1] = 9 is not one of the 4 classes", frac_of=(2, 9))
    refused("must be in 0 .. 65535", frac_of=(-1,))
    refused("frac with measured classes", classes=None)
    refused("no output", table=None, planes=None)
    refused("no output", table=C.byref(_lib.ClassTable()), planes=C.byref(_lib.ClassPlanes()))
    bad = _lib.ClassPlanes(call.planes.mode)
    bad.ld, bad.dtype = 12, _lib.I16
    refused("dtype", planes=C.byref(bad))
    if fn.endswith("_dev"):
        narrow = _lib.ClassPlanes(call.planes.mode)
        narrow.ld, narrow.dtype = (5 if "aggregate" in fn else 11), _lib.F64
        refused("ld is smaller", planes=C.byref(narrow))
    if "crosstab" in fn:
        refused("NULL", zones=None)
        refused("nrow * ncol", grid=(46341, 46341))
        refused("n_zones", n_zones=2 ** 31)
        refused("n_zones", n_zones=-1)
        refused("capacity", n_zones=17)
        refused("n_zones * (K + 3) = 2147483653 passes 2^31 - 1", n_zones=306783379, table=None)      # K = 4: 7 words a zone
        refused("counts with measured classes", classes=None, frac_of=(1,))
        if fn.endswith("_dev"):
            refused("ld_zones", ld_zones=11)
        else:
            refused("needs n_zones", n_zones=0)
    if "aggregate" in fn:
        refused("NULL", dst=None)
        refused("target grid dimension", dst=(0, 6))
        refused("source grid dimension", grid=(2 ** 30, 1))
        call.dst_res = None
        for res in (0.0, -1.0, NAN, float("inf")):                                             # what resample refuses of a geometry
            g = _lib.Grid(0.0, 10.0, res, 2.0, 5, 6)
            rc = getattr(call.lib, fn)(C.byref(_lib.Grid(0.0, 10.0, 1.0, 1.0, 10, 12)), C.byref(call.stack), 0, C.byref(g), (C.c_int32 * 1)(1), 1, None, 0,
                                       C.byref(call.planes), *((None, None) if fn.endswith("_dev") else (None,)))
            assert rc == _lib.ERR_INVALID and "cell size must be finite and positive" in call.lib.mhs_last_error().decode()
    if "focal" in fn:
        refused("radius 0 is not in 1 .. max(nrow, ncol) = 12", radius=0)
        refused("radius 13", radius=13)
        refused("unknown shape", shape=2)
        refused("twice", frac_of=(2, 2))
        with_simpson = _lib.ClassPlanes(call.planes.mode, None, None, None, call.planes.mode_frac)
        with_simpson.ld, with_simpson.dtype = 12, _lib.F64
        refused("simpson is not a product of a window", planes=C.byref(with_simpson))
    only_mode = _lib.ClassPlanes(call.planes.mode)
    only_mode.ld, only_mode.dtype = 12, _lib.F64
    # Calls that pass every check; where there is a device they RUN, so each must fit the stand-in buffers: the table holds 16 rows of
    # 4 columns (counts, frac), and 4 frac planes lie behind planes.frac.  K = 256 therefore takes the mode plane alone and no table.
    passing = (dict(), dict(frac_of=(4, 1)), dict(table=None), dict(planes=C.byref(only_mode), table=None, classes=None),
               dict(classes=tuple(range(256)), planes=C.byref(only_mode), table=None),
               dict(table=None, planes=None, info=C.byref(call.info), classes=None), dict(classes=(0, 65535)))
    for kw in passing:
        k, nf = len(kw.get("classes", (1, 2, 3, 4)) or ()), len(kw.get("frac_of", ()))
        with_frac = kw.get("planes", "default") == "default"
        assert not with_frac or 1 <= (nf or k) <= 4, kw                                        # the frac planes (and columns) that exist
        assert kw.get("table", "default") is None or "crosstab" not in fn or 1 <= k <= 4, kw   # the counts columns that exist
        rc, msg = call(**kw)
        assert rc in (_lib.OK, _lib.ERR_NODEVICE), (kw, msg)


def _fake(nrow=10, ncol=12, n_layers=2, res=1.0):
    """what the calls look at before their first device call; touching the planes would be one"""
    class Stack:
        geom = Geometry(0.0, float(nrow), res, res, nrow, ncol)
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
    T = Geometry(0.0, 10.0, 2.0, 2.0, 5, 6)
    calls = {"crosstab": lambda **kw: cl.crosstab(kw.pop("stack", _fake()), kw.pop("zones", zones), **kw),
             "aggregate": lambda **kw: cl.aggregate(kw.pop("stack", _fake()), kw.pop("geom", T), **kw),
             "focal": lambda **kw: cl.focal(kw.pop("stack", _fake()), kw.pop("radius", 2), **kw)}

    def refused(name, needle, **kw):
        with pytest.raises(ValueError, match=needle):
            calls[name](**kw)

    for name in calls:
        refused(name, "K must be in 1 .. 256", classes=[])
        refused(name, "K must be in 1 .. 256", classes=list(range(257)))
        refused(name, "not in 0 .. 65535", classes=[1, -1])
        refused(name, "not in 0 .. 65535", classes=[65536])
        refused(name, "distinct", classes=[3, 4, 3])
        refused(name, "classes holds 41.5: a code must be a whole number", classes=[3, 41.5])
        refused(name, "frac_of holds 3.5", classes=[3, 4], frac_of=[3.5])
        refused(name, "whole number", classes=["a"])
        refused(name, "frac_of code 9 is not one of the 2 classes", classes=[3, 4], frac_of=[9])
        refused(name, "layer", classes=[1], layer=2)
        refused(name, r"nrow \* ncol", classes=[1], stack=_fake(46341, 46341), **({"zones": zones} if name == "crosstab" else {}))
        refused(name, "out_dtype", classes=[1], out_dtype=torch.float16)
        with pytest.raises(AssertionError, match="planes were touched"):                       # a call that passes every check goes on
            calls[name](classes=[2, 1], frac_of=[1], out_dtype=torch.float32)
    refused("crosstab", "unknown name", classes=[1], stats=("median",))
    refused("crosstab", "unknown name", classes=[1], planes=("counts",))
    refused("crosstab", "once", classes=[1], stats=("mode", "mode"))
    refused("crosstab", "no output", classes=[1], stats=())
    refused("crosstab", "shape mismatch", classes=[1], zones=torch.zeros((10, 13), dtype=torch.int32))
    refused("crosstab", "shape mismatch", classes=[1], stack=_fake(12, 10))
    refused("crosstab", "integer tensor", classes=[1], zones=zones.double())
    refused("crosstab", "n_zones", classes=[1], n_zones=0)
    refused("crosstab", "n_zones", classes=[1], n_zones=2 ** 31)
    refused("crosstab", r"n_zones \* \(K \+ 3\) = 2147483653", classes=[1, 2, 3, 4], n_zones=306783379)
    refused("aggregate", "unknown name", classes=[1], products=("cells",))
    refused("aggregate", "no output", classes=[1], products=())
    refused("aggregate", "Geometry", classes=[1], geom=(0, 1, 2))
    for bad in (Geometry(0.0, 10.0, 0.0, 2.0, 5, 6), Geometry(0.0, 10.0, 2.0, -2.0, 5, 6), Geometry(0.0, 10.0, NAN, 2.0, 5, 6)):
        refused("aggregate", "target grid's cell size", classes=[1], geom=bad)
    refused("aggregate", "target grid dimension", classes=[1], geom=Geometry(0.0, 10.0, 2.0, 2.0, 0, 6))
    refused("aggregate", "origin must be finite", classes=[1], geom=Geometry(float("inf"), 10.0, 2.0, 2.0, 5, 6))
    refused("aggregate", "source grid's cell size", classes=[1], stack=_fake(res=0.0))
    refused("focal", "unknown name", classes=[1], products=("simpson",))
    refused("focal", "unknown shape", classes=[1], shape="ring")
    refused("focal", "radius", classes=[1], radius=0)
    refused("focal", "radius", classes=[1], radius=13)
    refused("focal", "radius", classes=[1], radius=(1, 2))
    refused("focal", "radius", classes=[1], radius=2.5)
    refused("focal", "once", classes=[1, 2], frac_of=[2, 2])


def test_rule_header_in_a_plain_cpp_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "classes_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "machisplin_amd", "csrc"),
           os.path.join(ROOT, "tests", "classes_check.cpp"), "-o", exe]
    run = subprocess.run(cmd, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    run = subprocess.run([exe], capture_output=True, text=True)       # stand-alone: the sanitizer runtimes are linked into it
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().split("\n")
    assert lines[-1] == "OK"
    forms = [ln.split()[-1] for ln in lines if ln.startswith("index")]
    assert forms.count("bisect") >= 5 and forms.count("table+bisect") >= 7
    # the units it prints, against the restatement's finishing step
    n_unit, classes = 0, None
    for ln in lines[:-1]:
        w = ln.split()
        if w[0] == "case":
            K = int(w[2])
            classes = [5 + k * (200 if K == 256 else 7) for k in range(K)]
        elif w[0] == "unit":
            at = w.index("->")
            other, counts = int(w[1]), [int(x) for x in w[2:at]]
            n, mode, variety = (int(x) for x in w[at + 1:at + 4])
            got = np.array([int(x, 16) for x in w[at + 4:]], dtype=np.uint64).view(np.float64)
            want = cr.finish([counts], [other], classes)
            assert (n, mode, variety) == (want["n"][0], want["mode"][0], want["variety"][0]), ln
            assert bits_equal(got, [want["mode_frac"][0], want["simpson"][0]]), ln
            counter = Counter({c: v for c, v in zip(classes, counts)})
            assert (n, mode) == cr.loop_finish(counter, other, classes)[:2]
            n_unit += 1
    assert n_unit == 200
