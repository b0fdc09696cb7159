"""CPU: the flow-path rule (include/machisplin_hip.h, section "flow paths").  The two numpy restatements the GPU tests compare with
(tests/flowpath_ref.py: a sequential walk and Jacobi pointer doubling) agree with each other and with hand-worked cases; every
entry point refuses bad arguments before it touches a device, naming the argument; and the rule header the kernels are built
from (csrc/flowpath_rule.h) gives the restatement's planes in a plain C++ program compiled with gcc under AddressSanitizer +
UBSan and run stand-alone.  Every comparison is exact equality, NaN matching NaN."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import flowpath_ref as fr
import hydro_ref as hr
from machisplin_amd import _lib
from machisplin_amd import flowpath as fp
from machisplin_amd.raster import Geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
E, SE, S, SW, W, NW, N, NE, OUT, NA = 0, 1, 2, 3, 4, 5, 6, 7, -1, -2


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def agree(d, target):
    w = fr.walk(d, target)
    rounds = []
    j = fr.doubling(d, target, rounds)
    for a, b in zip(w, j):
        assert np.array_equal(a, b)
    longest = int((w[1] + w[2] + w[3]).max()) if w[0].size else 0
    assert rounds[0] == (int(np.ceil(np.log2(longest))) if longest > 1 else 0)            # a path of L steps resolves in ceil(log2 L) rounds
    return w


def test_the_two_restatements_agree_on_random_forests():
    rng = np.random.default_rng(11)
    for _ in range(200):
        nrow, ncol = (int(x) for x in rng.integers(1, 25, 2))
        d = fr.random_forest(rng, nrow, ncol, rng.choice([0.0, 0.1, 0.5]))
        target = (rng.random((nrow, ncol)) < rng.choice([0.0, 0.05, 0.5, 1.0])) & (d != NA)
        agree(d, target)


@pytest.mark.parametrize("kind,shape", [(k, s) for k, s in hr.PLANES if s[0] * s[1] <= 97 * 130])
def test_the_two_restatements_agree_on_the_hydrology_planes(kind, shape):
    _, d, acc = fr.hydro_plane(kind, shape)
    agree(d, np.zeros(shape, dtype=bool))
    with np.errstate(invalid="ignore"):
        agree(d, acc >= 20)


def test_serpentines_have_one_path_through_every_cell():
    for shape, steps, rounds in (((33, 65), 2144, 12), ((70, 130), 9099, 14)):
        d = fr.serpentine(*shape)
        got = []
        end, ew, ns, dg = fr.doubling(d, np.zeros(shape, dtype=bool), got)
        assert got == [rounds] and (ew + ns + dg).max() == steps and (dg == 0).all() and len(np.unique(end)) == 1


def test_hand_worked_channel():
    # a 1 x 5 channel flowing east to the root at its end; dx = 30, dy = 20
    d = np.array([[E, E, E, E, OUT]], dtype=np.int8)
    z = np.array([[9.0, 7.0, 4.0, 2.0, 1.0]])
    p, info = fr.flowpath(d, z, None, "outlet", dx=30.0, dy=20.0, value_plane=z)
    assert p["index"].tolist() == [[4] * 5] and p["steps"].tolist() == [[4, 3, 2, 1, 0]]
    assert p["dist"].tolist() == [[120.0, 90.0, 60.0, 30.0, 0.0]] and p["value"].tolist() == [[1.0] * 5]
    assert p["drop"].tolist() == [[8.0, 6.0, 3.0, 1.0, 0.0]]
    assert info == {"n_valid": 5, "n_targets": 0, "n_roots": 1, "n_unreached": 0, "max_steps": 4, "rounds": 2}
    # the first cell with z <= 4 is the target: a path whose start is a target has steps 0 and drop 0
    p, info = fr.flowpath(d, z, None, "le", 4.0, dx=30.0, dy=20.0, value_plane=z)
    assert p["index"].tolist() == [[2, 2, 2, 3, 4]] and p["steps"].tolist() == [[2, 1, 0, 0, 0]] and p["drop"].tolist() == [[5.0, 3.0, 0.0, 0.0, 0.0]]
    assert info["n_targets"] == 3 and info["max_steps"] == 2


def test_hand_worked_diagonal_and_vertical_steps():
    # (0, 0) -SE-> (1, 1) -S-> (2, 1) -E-> (2, 2), the root
    d = np.array([[SE, NA, NA], [NA, S, NA], [NA, E, OUT]], dtype=np.int8)
    z = np.arange(9.0).reshape(3, 3)
    p, _ = fr.flowpath(d, z, None, "outlet", dx=3.0, dy=4.0, value_plane=z)
    assert p["index"][0, 0] == 8 and p["steps"][0, 0] == 3
    assert p["dist"][0, 0] == (1.0 * 3.0 + 1.0 * 4.0) + 1.0 * 5.0 and p["dist"][1, 1] == 7.0 and p["dist"][2, 1] == 3.0
    assert p["index"][0, 1] == -1 and np.isnan(p["dist"][0, 1]) and np.isnan(p["drop"][1, 0])            # NA cells
    g = np.sqrt(np.float64(30.0) * 30.0 + np.float64(20.0) * 20.0)
    assert fr.flowpath(d, dx=30.0, dy=20.0)[0]["dist"][0, 0] == (30.0 + 20.0) + g


def test_hand_worked_na_value_at_the_target():
    d = np.array([[E, E, OUT]], dtype=np.int8)
    v = np.array([[5.0, -9.0, -9.0]])
    p, _ = fr.flowpath(d, v, -9.0, "outlet", value_plane=v)
    assert np.isnan(p["value"]).all() and np.isnan(p["drop"]).all() and p["index"].tolist() == [[2, 2, 2]]
    # the value is there but the cell's own is NA: value stands, drop is NaN
    v = np.array([[5.0, -9.0, 1.0]])
    p, _ = fr.flowpath(d, v, -9.0, "outlet", value_plane=v)
    assert p["value"].tolist() == [[1.0, 1.0, 1.0]] and p["drop"][0, 0] == 4.0 and np.isnan(p["drop"][0, 1]) and p["drop"][0, 2] == 0.0


def test_hand_worked_unreached_with_and_without_root_is_target():
    # two trees: the left one meets the target (0, 1), the right one meets none
    d = np.array([[E, E, OUT, E, OUT]], dtype=np.int8)
    z = np.array([[0.0, 1.0, 0.0, 0.0, 0.0]])
    p, info = fr.flowpath(d, z, None, "eq", 1.0, root_is_target=False)
    assert p["index"].tolist() == [[1, 1, -1, -1, -1]] and p["steps"].tolist() == [[1, 0, -1, -1, -1]] and np.isnan(p["dist"][0, 2:]).all()
    assert info["n_unreached"] == 3 and info["max_steps"] == 1
    p, info = fr.flowpath(d, z, None, "eq", 1.0, root_is_target=True)
    assert p["index"].tolist() == [[1, 1, 2, 4, 4]] and p["steps"].tolist() == [[1, 0, 0, 1, 0]] and info["n_unreached"] == 0
    p, info = fr.flowpath(d, z, None, "eq", 7.0, root_is_target=False)
    assert (p["index"] == -1).all() and info["max_steps"] == -1 and info["n_unreached"] == 5


def test_hand_worked_outlet_labels():
    rng = np.random.default_rng(3)
    d = fr.random_forest(rng, 20, 31)
    p, info = fr.flowpath(d, search=fr.walk)
    idx = p["index"]
    roots = np.flatnonzero(d.ravel() == OUT)
    assert set(np.unique(idx[idx >= 0])) == set(roots) and info["n_roots"] == len(roots)
    # a cell carries the label of the cell it points at
    for r, c in zip(*np.nonzero(d >= 0)):
        assert idx[r, c] == idx[r + hr.K_DR[d[r, c]], c + hr.K_DC[d[r, c]]]
    assert (idx.ravel()[roots] == roots).all() and ((idx == -1) == (d == NA)).all()


def test_malformed_planes_and_cycles_are_told_apart():
    for bad in ([[E, E]], [[8, OUT]], [[-3, OUT]], [[E, NA]], [[N, OUT]]):
        with pytest.raises(fr.Malformed):
            fr.flowpath(np.array(bad, dtype=np.int8))
    for search in (fr.walk, fr.doubling):
        with pytest.raises(fr.Cycle):
            fr.flowpath(np.array([[E, W]], dtype=np.int8), search=search)


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
            self.d = torch.full((10, 12), -1, dtype=torch.int8, device="cuda")
            self.planes = torch.zeros((5, 10, 12), dtype=torch.float64, device="cuda")
            self.zptr, self.dptr, self.pptr = self.z.data_ptr(), self.d.data_ptr(), [self.planes[k].data_ptr() for k in range(5)]
        else:
            self.z = np.zeros((2, 10, 12), dtype=np.float32)
            self.d = np.full((10, 12), -1, dtype=np.int8)
            self.planes = np.zeros((5, 10, 12))
            self.zptr, self.dptr, self.pptr = self.z.ctypes.data, self.d.ctypes.data, [self.planes[k].ctypes.data for k in range(5)]
        self.stack = _lib.Stack(self.zptr, 2, _lib.F32, 120, 12, NAN)
        self.out = _lib.FlowpathOut(*self.pptr)

    def __call__(self, fn, grid=(10, 12), flowdir="default", ld_dir=12, stack="default", layer=0, where=8, threshold=0.0, value_layer=1, flags=1,
                 dx=1.0, dy=1.0, out="default", out_dtype=_lib.F64, ld=12):
        g = C.byref(_lib.Grid(0.0, 10.0, 1.0, 1.0, *grid)) if grid is not None else None
        d = self.dptr if flowdir == "default" else flowdir
        s = C.byref(self.stack) if stack == "default" else stack
        o = C.byref(self.out) if out == "default" else out
        f = getattr(self.lib, fn)
        head = (g, d, ld_dir, s, layer, where, threshold, value_layer, flags, dx, dy, o, out_dtype)
        rc = f(*head, ld, None, None) if fn.endswith("_dev") else f(*head, None)
        return rc, self.lib.mhs_last_error().decode()


@pytest.mark.parametrize("fn", ("mhs_flowpath_dev", "mhs_flowpath"))
def test_refusals_of_the_library_come_before_any_device_call(fn):
    call = _Call(fn)

    def refused(needle, **kw):
        rc, msg = call(fn, **kw)
        assert rc == _lib.ERR_INVALID and needle in msg and fn in msg, (kw, rc, msg)

    refused("NULL", grid=None)
    refused("NULL", flowdir=None)
    refused("NULL", stack=None)
    refused("NULL", out=None)
    refused("data is NULL", stack=C.byref(_lib.Stack(None, 2, _lib.F32, 120, 12, NAN)))
    refused("nrow, ncol", grid=(0, 12))
    refused("nrow, ncol", grid=(10, -1))
    refused("nrow, ncol", grid=(2 ** 31, 1))
    refused("nrow * ncol", grid=(32768, 65536))                               # 2^31: one past INT32_MAX
    refused("nrow * ncol", grid=(46341, 46341))
    refused("ld_dir", ld_dir=11)
    refused("bad stack dtype", stack=C.byref(_lib.Stack(call.zptr, 2, 7, 120, 12, NAN)))
    refused("layer", layer=2)
    refused("layer", layer=-1)
    refused("strides", stack=C.byref(_lib.Stack(call.zptr, 2, _lib.F32, 120, 11, NAN)))
    refused("strides", stack=C.byref(_lib.Stack(call.zptr, 2, _lib.F32, 119, 12, NAN)))
    refused("where", where=9)
    refused("where", where=-1)
    refused("threshold", where=2, threshold=NAN)
    refused("flags", flags=4)
    refused("flags", flags=-1)
    for bad in (0.0, -1.0, NAN, float("inf")):
        refused("dx and dy", dx=bad)
        refused("dx and dy", dy=bad)
    refused("no product", out=C.byref(_lib.FlowpathOut()))
    refused("value_layer", value_layer=2)
    refused("value_layer", value_layer=-1)
    refused("value_layer", value_layer=-1, out=C.byref(_lib.FlowpathOut(None, None, None, None, call.pptr[4])))
    for bad in (_lib.I16, 5, -1):
        refused("out_dtype", out_dtype=bad)
    if fn.endswith("_dev"):
        refused("ld smaller", ld=11)
    # value_layer is looked at only for value and drop, dx and dy only for dist; NaN is a threshold like any other for na, valid, outlet
    only_index = _lib.FlowpathOut(call.pptr[0], None, None, None, None)
    for kw in (dict(value_layer=-1, dx=0.0, dy=NAN, out=C.byref(only_index)), dict(threshold=NAN, where=1), dict(threshold=NAN), dict(ld_dir=12)):
        rc, msg = call(fn, **kw)
        assert rc in (_lib.OK, _lib.ERR_NODEVICE), (kw, msg)
    for where in range(9):
        for flags in range(4):
            rc, msg = call(fn, where=where, flags=flags)
            assert rc in (_lib.OK, _lib.ERR_NODEVICE), (where, flags, msg)


def _fake(nrow=10, ncol=12, xres=1.0, yres=1.0, n_layers=2):
    """what flowpath() looks at before its first device call; touching the planes would be one"""
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
    import torch
    d = torch.full((10, 12), -1, dtype=torch.int8)

    def refused(needle, *a, **kw):
        with pytest.raises(ValueError, match=needle):
            fp.flowpath(*a, **kw)

    refused("flowdir", torch.zeros((10, 12)), _fake())
    refused("flowdir", torch.zeros((2, 10, 12), dtype=torch.int8), _fake())
    refused("flowdir", {"twi": d}, _fake())
    refused("flowdir is", d, _fake(10, 13))
    refused("nrow \\* ncol", torch.zeros((1, 1), dtype=torch.int8), _fake(46341, 46341))
    refused("where", d, _fake(), where="near")
    refused("threshold", d, _fake(), where="ge")
    refused("threshold", d, _fake(), where="ge", threshold=NAN)
    refused("value_layer", d, _fake(), products=("index", "value"))
    refused("value_layer", d, _fake(), products="drop")
    refused("value_layer", d, _fake(), products="drop", value_layer=2)
    refused("products", d, _fake(), products=())
    refused("products", d, _fake(), products=("dist", "dist"))
    refused("product", d, _fake(), products=("d2",))
    refused("layer", d, _fake(), layer=2)
    refused("lonlat", d, _fake(), products=("index", "dist"), lonlat=True)
    refused("dx and dy", d, _fake(), products="dist", dx=0.0)
    refused("dx and dy", d, _fake(), products="dist", dy=float("inf"))
    refused("out_dtype", d, _fake(), out_dtype=np.float32)
    # lonlat and the units matter to dist alone; a hydro result stands for its flowdir plane
    with pytest.raises(AssertionError, match="planes were touched"):
        fp.flowpath(d, _fake(), products=("index", "steps"), lonlat=True)
    with pytest.raises(AssertionError, match="planes were touched"):
        fp.flowpath({"flowdir": d}, _fake(xres=30.0, yres=20.0), products="dist")


def _hex(a):
    a = np.asarray(a, dtype=np.float64).ravel()
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = np.uint64(0x7ff8000000000000)
    return " ".join(format(int(x), "x") for x in b)


def _cases():
    """(flowdir, z, value plane, where, threshold, root_is_target, nodata, dx, dy) of the check program's run"""
    rng = np.random.default_rng(21)
    out = []
    for kind, shape in (("noise", (33, 65)), ("holes", (97, 130)), ("bowl", (33, 65)), ("constant", (70, 1)), ("all_na", (2, 2)), ("tilted", (1, 70)),
                        ("spiral", (96, 96))):
        z, d, acc = fr.hydro_plane(kind, shape)
        v = np.where(rng.random(shape) < 0.05, -9.0, z)
        out.append((d, acc, v, "ge", 20.0, True, -9.0, 30.0, 30.0))
        out.append((d, acc, v, "ge", 20.0, False, -9.0, 30.0, 20.0))
        out.append((d, acc, v, "outlet", 0.0, False, -9.0, 25.0, 30.0))
    for shape in ((33, 65), (70, 130)):
        d = fr.serpentine(*shape)
        z = rng.integers(0, 9, shape).astype(np.float64)
        out.append((d, z, z, "outlet", 0.0, True, -9.0, 1.0, 1.0))
        out.append((d, z, z, "eq", 3.0, False, -9.0, 2.0, 3.0))
    for _ in range(6):
        shape = tuple(int(x) for x in rng.integers(1, 80, 2))
        d = fr.random_forest(rng, *shape)
        z = rng.integers(0, 9, shape).astype(np.float64)
        z[rng.random(shape) < 0.1] = NAN
        out.append((d, z, z, fr.WHERE[int(rng.integers(0, 9))], 3.0, bool(rng.integers(0, 2)), 5.0, 30.0, 30.0))
    z = np.zeros((1, 2))
    out.append((np.array([[E, W]], dtype=np.int8), z, z, "outlet", 0.0, True, NAN, 1.0, 1.0))                       # the 2-cell cycle
    big = fr.serpentine(40, 70)
    big[39, 69] = N                                                                                                 # ... and a cycle that a path of
    big[38, 69] = W                                                                                                 # 2 700 cells runs into
    out.append((big, np.zeros((40, 70)), np.zeros((40, 70)), "outlet", 0.0, True, NAN, 1.0, 1.0))
    for code in (8, -3, 100, -128):
        d = fr.serpentine(5, 7)
        d[2, 3] = code
        out.append((d, np.zeros((5, 7)), np.zeros((5, 7)), "outlet", 0.0, True, NAN, 1.0, 1.0))
    d = fr.serpentine(5, 7); d[0, 6] = E                                                                            # out of the raster
    out.append((d, np.zeros((5, 7)), np.zeros((5, 7)), "outlet", 0.0, True, NAN, 1.0, 1.0))
    d = fr.serpentine(5, 7); d[1, 6] = NA                                                                           # (0, 6) points at an NA cell
    out.append((d, np.zeros((5, 7)), np.zeros((5, 7)), "valid", 0.0, True, NAN, 1.0, 1.0))
    return out


def test_rule_header_in_a_plain_cpp_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "flowpath_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "machisplin_amd", "csrc"),
           os.path.join(ROOT, "tests", "flowpath_check.cpp"), "-o", exe]
    run = subprocess.run(cmd, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    cases = _cases()
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.write(f"{len(cases)}\n")
        for d, z, v, where, thr, root, nodata, dx, dy in cases:
            f.write(f"{d.shape[0]} {d.shape[1]} {fr.WHERE.index(where)} {int(root)} {int(not np.isnan(nodata))} "
                    f"{_hex([thr])} {_hex([nodata])} {_hex([dx])} {_hex([dy])}\n")
            f.write(" ".join(str(int(x)) for x in d.ravel()) + "\n" + _hex(z) + "\n" + _hex(v) + "\n")
    run = subprocess.run([exe, path], capture_output=True, text=True)       # stand-alone: the sanitizer runtimes are linked into it
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.strip().split("\n")
    assert lines[-1] == "OK"
    at = 0
    n_ok = n_bad = n_cycle = 0
    for k, (d, z, v, where, thr, root, nodata, dx, dy) in enumerate(cases):
        w = lines[at].split()
        assert w[:2] == ["case", str(k)], lines[at]
        try:
            want, info = fr.flowpath(d, z, nodata, where, thr, root, dx, dy, v)
        except fr.Malformed:
            assert w[2] == "malformed", lines[at]
            at, n_bad = at + 1, n_bad + 1
            continue
        except fr.Cycle:
            assert w[2] == "cycle", lines[at]
            at, n_cycle = at + 1, n_cycle + 1
            continue
        assert w[2] == "ok", lines[at]
        got = [int(x) for x in w[3:]]
        assert got[:6] == [info[n] for n in ("n_valid", "n_targets", "n_roots", "n_unreached", "max_steps", "rounds")], (k, got, info)
        assert got[6] <= got[5]                                            # the local phase never adds a global round
        for j, name in enumerate(("index", "steps")):
            assert np.array_equal(np.array(lines[at + 1 + j].split(), dtype=np.int64).reshape(d.shape), want[name]), (k, name)
        for j, name in enumerate(("dist", "value", "drop")):
            bits = np.array([int(x, 16) for x in lines[at + 3 + j].split()], dtype=np.uint64)
            assert same(bits.view(np.float64).reshape(d.shape), want[name]), (k, name)
        at, n_ok = at + 6, n_ok + 1
    assert at == len(lines) - 1 and n_bad == 6 and n_cycle == 2 and n_ok == len(cases) - 8
