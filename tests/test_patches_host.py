"""CPU: the patches rule (include/machisplin_hip.h, section "patches").  The two numpy restatements the GPU tests compare with
(tests/patches_ref.py) agree with each other, with scipy's labelling and with hand-worked cases; every entry point refuses bad
arguments before it touches a device, naming the argument; and the rule header the kernels are built from
(csrc/patches_rule.h) gives the restatement's planes in a plain C++ program compiled with gcc under AddressSanitizer + UBSan and
run stand-alone: the sequential union-find, and the tile and border decomposition run tile by tile on the host.  Every
comparison is exact equality."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import patches_ref as pr
from machisplin_amd import _lib
from machisplin_amd import patches as pt
from machisplin_amd.raster import Geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def test_the_two_restatements_agree_on_random_grids():
    rng = np.random.default_rng(5)
    densities = (0.0, 0.1, 0.41, 0.6, 1.0)
    for k in range(200):
        nrow, ncol = (int(x) for x in rng.integers(1, 25, 2))
        mask = rng.random((nrow, ncol)) < densities[k % 5]
        for conn in (4, 8):
            assert np.array_equal(pr.flood(mask, conn), pr.propagate(mask, conn)), (nrow, ncol, conn)


def test_id_and_size_equal_scipys_labelling():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(6)
    for shape, density in (((150, 170), 0.5), ((97, 300), 0.41), ((300, 97), 0.59), ((1, 300), 0.5), ((300, 1), 0.5), ((40, 40), 0.0)):
        mask = rng.random(shape) < density
        for conn, structure in ((8, np.ones((3, 3))), (4, None)):
            want, k = ndi.label(mask, structure=structure)
            planes, info = pr.patches(mask, conn)
            assert np.array_equal(planes["id"], want) and info["n_patches"] == k, (shape, conn)
            assert np.array_equal(planes["size"], np.where(mask, np.bincount(want.ravel())[want], 0)), (shape, conn)


def test_hand_worked_diagonal_pair():
    m = np.zeros((3, 3), bool); m[0, 0] = m[1, 1] = True
    for search in (pr.flood, pr.propagate):
        p8, i8 = pr.patches(m, 8, search=search)
        p4, i4 = pr.patches(m, 4, search=search)
        assert i8["n_patches"] == 1 and p8["label"].tolist() == [[0, -1, -1], [-1, 0, -1], [-1, -1, -1]]
        assert p8["size"][1, 1] == 2 and p8["id"][1, 1] == 1
        assert i4["n_patches"] == 2 and p4["label"].tolist() == [[0, -1, -1], [-1, 4, -1], [-1, -1, -1]]
        assert p4["id"].tolist() == [[1, 0, 0], [0, 2, 0], [0, 0, 0]] and p4["size"].max() == 1
    # the anti-diagonal pair too
    m = np.zeros((2, 2), bool); m[0, 1] = m[1, 0] = True
    assert pr.patches(m, 8)[0]["label"].tolist() == [[-1, 1], [1, -1]] and pr.patches(m, 4)[0]["label"].tolist() == [[-1, 1], [2, -1]]


def _ring():
    """a 7 x 7 plane: a ring of values around a hole of two NA cells, NA outside the ring"""
    z = np.full((7, 7), NAN)
    z[1:6, 1:6] = 1.0
    z[3, 2:4] = NAN
    return z


def test_hand_worked_ring_around_a_hole():
    na = pr.features(_ring(), None, "na")
    p, info = pr.patches(na, 8)
    assert info["n_patches"] == 2 and info["n_features"] == 24 + 2 and info["max_size"] == 24
    assert p["label"][3, 2] == p["label"][3, 3] == 3 * 7 + 2 and p["edge"][3, 2] == 0 and p["size"][3, 3] == 2 and p["id"][3, 2] == 2
    assert p["label"][0, 0] == p["label"][6, 6] == 0 and p["edge"][6, 6] == 1 and p["size"][0, 3] == 24 and p["id"][6, 0] == 1
    assert (p["label"][1:6, 1:6][~na[1:6, 1:6]] == -1).all() and (p["size"][~na] == 0).all() and (p["edge"][~na] == 0).all()
    # the ring itself is one patch that does not touch the edge
    ring, rinfo = pr.patches(~na, 4)
    assert rinfo["n_patches"] == 1 and ring["size"].max() == 23 and ring["edge"].max() == 0


def test_hand_worked_keep_under_each_edge_rule_and_at_the_size_bounds():
    na = pr.features(_ring(), None, "na")
    hole, sea = (3, 2), (0, 0)
    keep = lambda **kw: pr.patches(na, 8, **kw)[0]["keep"]                   # noqa: E731
    assert keep()[hole] == 1 and keep()[sea] == 1 and keep().sum() == 26
    assert keep(edge="touching")[hole] == 0 and keep(edge="touching")[sea] == 1
    assert keep(edge="interior")[hole] == 1 and keep(edge="interior")[sea] == 0
    # size == min_size and size == max_size pass; one beyond does not
    assert keep(min_size=2)[hole] == 1 and keep(min_size=3)[hole] == 0 and keep(min_size=24)[sea] == 1 and keep(min_size=25).sum() == 0
    assert keep(max_size=24)[sea] == 1 and keep(max_size=23)[sea] == 0 and keep(max_size=2)[hole] == 1 and keep(max_size=1).sum() == 0
    assert keep(min_size=2, max_size=2).sum() == 2 and keep(min_size=3, max_size=23).sum() == 0
    _, info = pr.patches(na, 8, min_size=3, edge="touching")
    assert info["n_kept_patches"] == 1 and info["n_kept_cells"] == 24
    assert (keep()[~na] == 0).all()


class _Call:
    """One of the two entry points on a 10 x 12 stack of two layers.  A refusal comes before the first device call and reads no
    plane.  The calls that PASS the checks end at MHS_ERR_NODEVICE on a machine without a GPU -- but where there is one they run,
    so the planes of the _dev entry are then device tensors and those of the host entry are host arrays."""

    def __init__(self, fn):
        import torch
        self.lib = _lib.load()
        if fn.endswith("_dev") and torch.cuda.is_available():
            self.z = torch.zeros((2, 10, 12), dtype=torch.float32, device="cuda")
            self.planes = torch.zeros((5, 10, 12), dtype=torch.int32, device="cuda")
            self.zptr, self.pptr = self.z.data_ptr(), [self.planes[k].data_ptr() for k in range(5)]
        else:
            self.z = np.zeros((2, 10, 12), dtype=np.float32)
            self.planes = np.zeros((5, 10, 12), dtype=np.int32)
            self.zptr, self.pptr = self.z.ctypes.data, [self.planes[k].ctypes.data for k in range(5)]
        self.stack = _lib.Stack(self.zptr, 2, _lib.F32, 120, 12, NAN)
        self.out = _lib.PatchesOut(*self.pptr)

    def __call__(self, fn, grid=(10, 12), stack="default", layer=0, where=1, threshold=0.0, connectivity=8, min_size=1, max_size=2 ** 63 - 1,
                 edge_rule=0, out="default", ld=12):
        g = C.byref(_lib.Grid(0.0, 10.0, 1.0, 1.0, *grid)) if grid is not None else None
        s = C.byref(self.stack) if stack == "default" else stack
        o = C.byref(self.out) if out == "default" else out
        f = getattr(self.lib, fn)
        head = (g, s, layer, where, threshold, connectivity, min_size, max_size, edge_rule, o)
        rc = f(*head, ld, None, None) if fn.endswith("_dev") else f(*head, None)
        return rc, self.lib.mhs_last_error().decode()


@pytest.mark.parametrize("fn", ("mhs_patches_dev", "mhs_patches"))
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
    refused("nrow * ncol", grid=(46341, 46341))                               # 2 147 488 281 cells: one row and column past 2^31 - 1
    refused("nrow * ncol", grid=(2, 2 ** 30))
    refused("bad stack dtype", stack=C.byref(_lib.Stack(call.zptr, 2, 7, 120, 12, NAN)))
    refused("layer", layer=2)
    refused("layer", layer=-1)
    refused("strides", stack=C.byref(_lib.Stack(call.zptr, 2, _lib.F32, 120, 11, NAN)))
    refused("where", where=8)
    refused("where", where=-1)
    refused("threshold", where=2, threshold=NAN)
    for bad in (6, 0, 1, -8, 16):
        refused("connectivity", connectivity=bad)
    refused("min_size", min_size=0)
    refused("min_size", min_size=-3)
    refused("max_size", min_size=5, max_size=4)
    for bad in (3, -1):
        refused("edge_rule", edge_rule=bad)
    refused("no product", out=C.byref(_lib.PatchesOut()))
    if fn.endswith("_dev"):
        refused("ld smaller", ld=11)
    only_keep = _lib.PatchesOut(None, None, None, None, call.pptr[4])
    for kw in (dict(out=C.byref(only_keep)), dict(connectivity=4), dict(min_size=5, max_size=5), dict(edge_rule=2), dict(threshold=NAN, where=0)):
        rc, msg = call(fn, **kw)
        assert rc in (_lib.OK, _lib.ERR_NODEVICE), (kw, msg)
    for where in range(8):
        rc, msg = call(fn, where=where)
        assert rc in (_lib.OK, _lib.ERR_NODEVICE), (where, msg)


def _fake(nrow=10, ncol=12, n_layers=2):
    """what patches() looks at before its first device call; touching the planes would be one"""
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
    def refused(needle, *a, **kw):
        with pytest.raises(ValueError, match=needle):
            pt.patches(*a, **kw)

    refused("connectivity", _fake(), connectivity=6)
    refused("product", _fake(), products=("labels",))
    refused("products", _fake(), products=())
    refused("products", _fake(), products=("keep", "keep"))
    refused("min_size", _fake(), min_size=0)
    refused("max_size", _fake(), min_size=4, max_size=3)
    refused("edge", _fake(), edge="border")
    refused("threshold", _fake(), where="le")
    refused("threshold", _fake(), where="le", threshold=NAN)
    refused("where", _fake(), where="near")
    refused(r"nrow \* ncol", _fake(46341, 46341))
    refused("layer", _fake(), layer=2)
    import torch
    refused("tensor", torch.zeros((3, 3)))                       # a float tensor is no tensor of flags
    refused("tensor", torch.zeros((2, 3, 3), dtype=torch.bool))
    refused("tensor", torch.zeros((3, 3), dtype=torch.bool), where="na")
    with pytest.raises(ValueError, match="connectivity"):
        pt.sieve(_fake(), connectivity=6)
    # a call that passes every check goes on to the planes
    with pytest.raises(AssertionError, match="planes were touched"):
        pt.patches(_fake(), where="le", threshold=3, connectivity=4, products="keep", min_size=2, max_size=2, edge="interior")


def _lcg_mask(k, nrow, ncol, threshold):
    state = 7000 + k
    q = np.empty(nrow * ncol)
    for i in range(nrow * ncol):
        state = (state * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        q[i] = (state >> 33) % 100
    return q.reshape(nrow, ncol) < threshold


def test_rule_header_in_a_plain_cpp_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "patches_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "machisplin_amd", "csrc"),
           os.path.join(ROOT, "tests", "patches_check.cpp"), "-o", exe]
    run = subprocess.run(cmd, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    run = subprocess.run([exe], capture_output=True, text=True)       # stand-alone: the sanitizer runtimes are linked into it
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.strip().split("\n")
    assert lines[-1] == "OK"
    n_run = n_case = 0
    multi_tile = set()
    for ln in lines[:-1]:
        w = ln.split()
        if w[0] == "run":
            m, c, start, length = (int(x) for x in w[1:])
            bits = [(m >> b) & 1 for b in range(64)]
            assert bits[c] and all(bits[start:c + 1]) and (start == 0 or not bits[start - 1]), ln
            assert all(bits[c:c + length]) and (c + length == 64 or not bits[c + length]), ln
            n_run += 1
        else:
            assert w[0] == "case", ln
            k, nrow, ncol, where = (int(x) for x in w[1:5])
            threshold = float(w[5])
            conn, min_size, max_size, edge_rule = (int(x) for x in w[6:10])
            got = [int(x) for x in w[10:]]
            mask = _lcg_mask(k, nrow, ncol, threshold)
            p, info = pr.patches(mask, conn, min_size, max_size, pr.EDGE[edge_rule])
            x = np.stack([p[name].astype(np.int64).view(np.uint64) for name in pr.PRODUCTS], axis=-1).ravel()
            with np.errstate(over="ignore"):
                want = int((x * (2 * np.arange(x.size, dtype=np.uint64) + 1)).sum(dtype=np.uint64))
            assert got == [want, info["n_features"], info["n_patches"], info["n_kept_patches"], info["n_kept_cells"], info["max_size"]], ln
            assert np.array_equal(pr.propagate(mask, conn), p["label"]), ln
            if nrow > 64 and ncol > 128:
                multi_tile.add((threshold, conn))
            n_case += 1
    assert n_run == 1 + 1 + 64 + 29 + 62 + 32 and n_case == 8 * 5 * 2 and len(multi_tile) == 10
