"""GPU: categorical layers (include/machisplin_hip.h, section "classes"; csrc/classes.hip).  Every table, plane and info field of
classes.crosstab, classes.aggregate and classes.focal equals the numpy restatement of tests/classes_ref.py EXACTLY (the bytes are
compared, NaN included).

Shapes: the project's edge set -- the degenerate ones, one less than, exactly and one more than a tile of class_zone_kernel in
both dimensions, and 2 x 2 tiles and a bit.  Zone planes that stress the run logic and the LDS table: one zone, every cell its
own zone (runs of one, more (zone, class) pairs per strip than CLS_LDS_SLOTS: the global path), stripes, checkerboards of zones
and of classes, no zone, a zone in the first and the last tile only.  Class lists of K = 1, 2, 63, 64, 65, 256 in the dense
form that takes the direct table and in the spread form that takes the bisection.  Targets of aggregate one below, at and one
above the kernel's tile (computed here as aggregate_tile of classes.hip computes it, from the constants of classes_rule.h)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import classes_ref as cr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def _constant(name):
    text = open(os.path.join(ROOT, "machisplin_amd", "csrc", "classes_rule.h")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


TR, TC, SLOTS, STRIP = _constant("CLS_TILE_ROWS"), _constant("CLS_TILE_COLS"), _constant("CLS_LDS_SLOTS"), _constant("CLS_STRIP_TILES")
AGG_WORDS, AGG_SIDE, SPAN = _constant("CLS_AGG_WORDS"), _constant("CLS_AGG_SIDE"), _constant("CLS_TABLE_SPAN")
AGG_MIN_TILES, AGG_MIN_COLS = _constant("CLS_AGG_MIN_TILES"), _constant("CLS_AGG_MIN_COLS")
BIG = (2 * TR + 3, 2 * TC + 5)
SHAPES = [(1, 1), (1, TC + 1), (TR + 1, 1)] + [(r, c) for r in (TR - 1, TR, TR + 1) for c in (TC - 1, TC, TC + 1)] + [BIG]
TABLE_STATS = ("counts", "n", "other", "cells", "mode", "mode_frac", "variety", "simpson", "frac")
ZONE_PLANES = ("mode", "mode_frac", "variety", "simpson", "n", "frac")
AGG = ("mode", "variety", "n", "mode_frac", "simpson", "frac")
FOCAL = ("frac", "mode", "mode_frac", "variety", "n")
NLCD = [11, 21, 22, 23, 24, 31, 41, 42, 43, 52, 71, 81, 82, 90, 95]


def aggregate_tile(K, nrow, ncol):
    """(rows, columns) of class_aggregate_kernel's tile: aggregate_tile of csrc/classes.hip"""
    cap = AGG_WORDS // (K + 2)
    tc = min(ncol, cap, AGG_SIDE)
    tr = max(1, min(nrow, cap // tc, AGG_SIDE))
    tiles = lambda: -(-nrow // tr) * -(-ncol // tc)                        # noqa: E731
    while tr > 1 and tiles() < AGG_MIN_TILES:                              # few tiles: halved, rows first, then columns
        tr = (tr + 1) // 2
    while tc > AGG_MIN_COLS and tiles() < AGG_MIN_TILES:
        tc = (tc + 1) // 2
    return tr, tc


def class_list(K, form):
    """K codes; "table": max - min < CLS_TABLE_SPAN (the direct table), "bisect": spread over 0 .. 65 535"""
    if form == "table":
        return [100 + 3 * k for k in range(K)] if 3 * K < SPAN else list(range(700, 700 + K))
    if K == 1:
        return [65535]                                                     # a single code is always a table: its far end
    return [0] + [(k * 65535) // (K - 1) for k in range(1, K)]


def land_cover(shape, dtype, codes, seed=0, blobs=True, p_na=0.08, p_other=0.08):
    """(plane, nodata): coherent blobs (or speckle) of `codes`, with NA cells and cells that are `other`"""
    rng = np.random.default_rng(seed + 1000 * shape[0] + shape[1])
    nr, nc = shape
    if blobs:
        r, c = np.meshgrid(np.arange(nr), np.arange(nc), indexing="ij")
        field = np.sin(r / 5.0 + seed) + np.cos(c / 7.0) + 0.5 * np.sin((r + c) / 3.0)
        idx = np.digitize(field, np.linspace(field.min(), field.max() + 1e-9, len(codes) + 1)[1:-1])
    else:
        idx = rng.integers(0, len(codes), shape)
    z = np.asarray(codes, dtype=np.float64)[idx]
    if dtype == np.int16:
        z = np.where(z > 32767, z - 40000, z)                              # an int16 plane cannot hold the upper codes: they are `other`
        stray = rng.choice(np.array([-5.0, 32001.0, 777.0]), size=shape)
    else:
        stray = rng.choice(np.array([0.5, -3.0, 70000.0, 65534.5, np.inf, 777.0]), size=shape)
    z = np.where(rng.random(shape) < p_other, stray, z)
    nodata = -32768.0 if dtype == np.int16 else NAN
    z = np.where(rng.random(shape) < p_na, nodata, z)
    return z.astype(dtype), nodata


def zone_planes(nrow, ncol):
    """name -> (int32 zone plane, n_zones)"""
    r, c = np.meshgrid(np.arange(nrow), np.arange(ncol), indexing="ij")
    n = nrow * ncol
    cell = r * ncol + c
    ends = np.full((nrow, ncol), -1, dtype=np.int64)
    ends[0, :3] = 7
    ends[-1, -3:] = 5
    out = {"one": (np.zeros((nrow, ncol)), 1), "own": (cell, n), "columns": (c, ncol), "rows": (r, nrow), "checkerboard": ((r + c) % 2, 2),
           "none": (np.full((nrow, ncol), -1), 3), "ends": (ends, 9), "holes": (np.where((r * 7 + c * 3) % 5 == 0, -1, (r // 3) * 40 + c // 4), 40 * nrow)}
    return {k: (z.astype(np.int32), nz) for k, (z, nz) in out.items()}


def _bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _same(got, want, names, tag, f32=False):
    for k in names:
        g = got[k].cpu().numpy() if hasattr(got[k], "cpu") else got[k]
        w = want[k]
        if w.dtype == np.float64 and f32:
            w = w.astype(np.float32)
        assert _bits(np.ascontiguousarray(g), np.ascontiguousarray(w)), (tag, k, g, w)


def _info(got, want, tag):
    for k in want:
        assert got[k] == want[k], (tag, k, got[k], want[k])


def _stack(hip, plane, nodata=NAN, pad=0, geom=None):
    """a one-layer RasterStack; pad > 0: layer 1 of a tensor with `pad` more columns and one more layer"""
    import torch
    plane = np.asarray(plane)
    nr, nc = plane.shape
    st = hip.RasterStack(geom or hip.Geometry(1000.0, 5000.0, 30.0, 30.0, nr, nc), plane[None], nodata)
    if pad:
        big = torch.full((2, nr, nc + pad), 5, dtype=st.planes.dtype, device=st.planes.device)
        big[1, :, :nc] = st.planes[0]
        st.planes = big[:, :, :nc]
        assert st.planes.stride(1) == nc + pad
    return st


def _crosstab(hip, stack, zones, want, tag, **kw):
    import torch
    kw.setdefault("stats", TABLE_STATS)
    kw.setdefault("planes", ZONE_PLANES)
    f32 = kw.get("out_dtype") is torch.float32
    table, planes, info = hip.classes.crosstab(stack, torch.from_numpy(np.ascontiguousarray(zones)), **kw)
    wt, wp, wi = want
    _same(table, wt, kw["stats"], tag + " table")
    _same(planes, wp, kw["planes"], tag + " planes", f32)
    _info(info, wi, tag)
    return table, planes, info


# ---------------------------------------------------------------------------------------------------------------- crosstab

@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32", "i16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_crosstab_on_the_edge_grids_with_every_zone_plane(hip, shape, dtype):
    z, nodata = land_cover(shape, dtype, NLCD, blobs=shape[0] % 2 == 0)
    st = _stack(hip, z, nodata)
    for name, (zones, nz) in zone_planes(*shape).items():
        if nz * (len(NLCD) + 3) > 2 ** 31 - 1:
            continue
        want = cr.crosstab(z, zones, NLCD, nodata, n_zones=nz, frac_of=(41, 11, 95))
        _crosstab(hip, st, zones, want, f"{shape} {name}", classes=NLCD, n_zones=nz, frac_of=(41, 11, 95))


@pytest.mark.parametrize("form", ["table", "bisect"])
@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 256])
def test_crosstab_class_lists_that_force_each_class_index_form(hip, K, form):
    codes = class_list(K, form)
    assert len(set(codes)) == K and ((max(codes) - min(codes) < SPAN) == (form == "table" or K == 1))
    z, nodata = land_cover(BIG, np.float32, codes + [min(codes) + 1 if min(codes) + 1 not in codes else 699], seed=K, blobs=False)
    st = _stack(hip, z, nodata)
    zones = zone_planes(*BIG)["holes"][0]
    rng = np.random.default_rng(K)
    given = [int(c) for c in rng.permutation(codes)]                       # the library sorts the list
    want = cr.crosstab(z, zones, codes, nodata)
    table, _, info = _crosstab(hip, st, zones, want, f"K {K} {form}", classes=given)
    assert info["K"] == K and info["codes"] == sorted(codes) and table["counts"].shape == (info["n_zones"], K)


def test_crosstab_checkerboards_of_zones_and_classes_take_the_global_path(hip):
    nr, nc = BIG
    r, c = np.meshgrid(np.arange(nr), np.arange(nc), indexing="ij")
    z = np.where((r + c) % 2 == 0, 41.0, 42.0).astype(np.float32)          # every run has length 1
    st = _stack(hip, z)
    own = (r * nc + c).astype(np.int32)
    assert min(nr, TR * STRIP) * TC > SLOTS                                 # more (zone, class) pairs in a strip than LDS slots
    _crosstab(hip, st, own, cr.crosstab(z, own, [41, 42, 43]), "own zones, class checkerboard", classes=[41, 42, 43])
    board = ((r + c) % 2 + 2 * ((r // 2 + c) % 3)).astype(np.int32)        # a checkerboard of zones over a checkerboard of classes
    z3 = np.asarray([11.0, 21.0, 22.0], dtype=np.float32)[(r + 2 * c) % 3]
    _crosstab(hip, _stack(hip, z3), board, cr.crosstab(z3, board, [11, 21, 22]), "zone checkerboard", classes=[11, 21, 22])
    pairs = ((r * nc + c) // 2).astype(np.int32)
    _crosstab(hip, st, pairs, cr.crosstab(z, pairs, [41, 42]), "pairs", classes=[41, 42])


def test_crosstab_measured_against_given_and_degenerate_layers(hip):
    import torch
    shape = (TR + 1, TC + 1)
    z, nodata = land_cover(shape, np.float32, NLCD[:6], seed=3)
    zones, nz = zone_planes(*shape)["holes"]
    st = _stack(hip, z, nodata)
    codes = cr.measure(z, nodata)
    assert 777 in codes
    want = cr.crosstab(z, zones, None, nodata)
    a = _crosstab(hip, st, zones, want, "measured")                        # classes and n_zones measured
    b = _crosstab(hip, st, zones, want, "given", classes=codes, n_zones=want[2]["n_zones"])
    assert all(_bits(a[0][k].cpu().numpy(), b[0][k].cpu().numpy()) for k in TABLE_STATS) and a[2] == b[2]
    assert a[2]["n_other"] == int(((cr.codes_of(z, nodata)) == -1).sum()) > 0
    c = _crosstab(hip, st, zones, cr.crosstab(z, zones, codes, nodata, n_zones=nz), "n_zones above the largest zone", classes=codes, n_zones=nz)
    assert c[0]["n"].shape == (nz,)
    # all `other`, all NA
    other = np.full(shape, 0.5, dtype=np.float32)
    _crosstab(hip, _stack(hip, other), zones, cr.crosstab(other, zones, [1, 2]), "all other", classes=[1, 2])
    na = np.full(shape, NAN, dtype=np.float32)
    t, p, i = _crosstab(hip, _stack(hip, na), zones, cr.crosstab(na, zones, [1, 2]), "all NA", classes=[1, 2])
    assert int(t["n"].sum()) == 0 and int(t["cells"].sum()) == int((zones >= 0).sum()) and i["n_valid"] == 0 and bool(torch.isnan(t["simpson"]).all())
    # a tie in every zone: two cells of each of two classes per zone; the larger code first in the data
    rows = np.arange(shape[0])[:, None] + np.zeros(shape, dtype=int)
    tie = np.tile(np.array([9.0, 9.0, 4.0, 4.0], dtype=np.float32), (shape[0], shape[1] // 4 + 1))[:, :shape[1] // 4 * 4]
    tz = rows[:, :tie.shape[1]].astype(np.int32)
    t, _, _ = _crosstab(hip, _stack(hip, tie), tz, cr.crosstab(tie, tz, [9, 4]), "ties", classes=[9, 4])
    assert t["mode"].cpu().tolist() == [4] * shape[0] and t["mode_frac"].cpu().tolist() == [0.5] * shape[0]
    # float32 planes are the float64 values rounded once
    _crosstab(hip, st, zones, want, "float32 planes", out_dtype=torch.float32, stats=("mode",))


def test_crosstab_over_patches_ids_and_rasterize_index(hip):
    from machisplin_amd.vector import Features
    shape = BIG
    z, nodata = land_cover(shape, np.int16, NLCD, seed=5)
    st = _stack(hip, z, nodata)
    ids, pinfo = hip.patches.patches(st, 0, where="eq", threshold=float(NLCD[3]), products="id")
    zones = (ids - 1).cpu().numpy()                                        # id 1 .. K on the patches, 0 elsewhere: zones 0 .. K - 1, -1 elsewhere
    assert pinfo["n_patches"] > 1 and zones.max() == pinfo["n_patches"] - 1
    t, _, _ = _crosstab(hip, st, zones, cr.crosstab(z, zones, NLCD, nodata), "patches id", classes=NLCD)
    assert set(t["mode"].cpu().tolist()) == {NLCD[3]} and set(t["variety"].cpu().tolist()) == {1}
    g = st.geom
    rects = []
    for (x0, x1, y0, y1) in ((0.05, 0.4, 0.1, 0.9), (0.3, 0.8, 0.5, 0.95), (0.6, 0.97, 0.05, 0.45)):
        xs, ys = g.xmin + np.array([x0, x1, x1, x0, x0]) * g.ncol * g.xres, g.ymax - np.array([y0, y0, y1, y1, y0]) * g.nrow * g.yres
        rects.append([np.column_stack([xs, ys])])
    planes, _ = hip.rasterize.rasterize(Features.from_parts("polygon", rects, np.arange(3.0)), g, products=("index",))
    index = planes["index"].cpu().numpy()
    assert set(np.unique(index)) == {-1, 0, 1, 2}
    _crosstab(hip, st, index, cr.crosstab(z, index, NLCD, nodata), "rasterize index", classes=NLCD)


def test_crosstab_strided_stack_side_stream_host_entry_and_repeats(hip):
    import torch
    from machisplin_amd import _lib
    shape = BIG
    z, nodata = land_cover(shape, np.float32, NLCD, seed=7)
    zones, nz = zone_planes(*shape)["holes"]
    want = cr.crosstab(z, zones, NLCD, nodata, n_zones=nz)
    first = _crosstab(hip, _stack(hip, z, nodata), zones, want, "dense", classes=NLCD, n_zones=nz)
    second = _crosstab(hip, _stack(hip, z, nodata, pad=7), zones, want, "strided", classes=NLCD, n_zones=nz, layer=1)
    for k in TABLE_STATS:
        assert first[0][k].cpu().numpy().tobytes() == second[0][k].cpu().numpy().tobytes()
    # the identical call twice: the same bytes, table and planes (every accumulator is an integer, so no order of the atomics shows)
    st = _stack(hip, z, nodata)
    zt = torch.from_numpy(zones)
    once = hip.classes.crosstab(st, zt, classes=NLCD, n_zones=nz, stats=TABLE_STATS, planes=ZONE_PLANES)
    twice = hip.classes.crosstab(st, zt, classes=NLCD, n_zones=nz, stats=TABLE_STATS, planes=ZONE_PLANES)
    for a, b in ((once[0], twice[0]), (once[1], twice[1])):
        assert list(a) == list(b) and all(a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes() for k in a)
    assert once[2] == twice[2]
    T = hip.Geometry(1000.0, 5000.0, 75.0, 75.0, 27, 54)
    for call in (lambda: hip.classes.aggregate(st, T, classes=NLCD, products=AGG), lambda: hip.classes.focal(st, 5, classes=NLCD[:4], products=FOCAL)):
        (a, ia), (b, ib) = call(), call()
        assert all(a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes() for k in a) and ia == ib
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        st = _stack(hip, z, nodata)
        _crosstab(hip, st, zones, want, "side stream", classes=NLCD, n_zones=nz, stream=side.cuda_stream)
    side.synchronize()
    # the host entry: everything on the host
    K, n = len(NLCD), z.size
    lib = _lib.lib()
    zc = np.ascontiguousarray(z)
    ti = {k: np.full((nz, K) if k == "counts" else nz, -9, dtype=np.int32) for k in ("counts", "n", "other", "cells", "mode", "variety")}
    td = {k: np.full((nz, K) if k == "frac" else nz, -9.0) for k in ("mode_frac", "simpson", "frac")}
    pi = {k: np.full(shape, -9, dtype=np.int32) for k in ("mode", "variety", "n")}
    pd = {"mode_frac": np.full(shape, -9.0), "simpson": np.full(shape, -9.0), "frac": np.full((K,) + shape, -9.0)}
    tab = _lib.ClassTable(nz, *[ti[k].ctypes.data for k in ("counts", "n", "other", "cells", "mode", "variety")], td["mode_frac"].ctypes.data,
                          td["simpson"].ctypes.data, td["frac"].ctypes.data)
    pl = _lib.ClassPlanes(pi["mode"].ctypes.data, pi["variety"].ctypes.data, pi["n"].ctypes.data, pd["mode_frac"].ctypes.data, pd["simpson"].ctypes.data,
                          pd["frac"].ctypes.data, 0, 0, _lib.F64)
    info = _lib.ClassInfo()
    g = _lib.Grid(1000.0, 5000.0, 30.0, 30.0, *shape)
    cs = _lib.Stack(zc.ctypes.data, 1, _lib.F32, n, shape[1], nodata)
    cl = (C.c_int32 * K)(*NLCD)
    _lib.check(lib.mhs_class_crosstab(C.byref(g), C.byref(cs), 0, np.ascontiguousarray(zones).ctypes.data, nz, cl, K, None, 0, C.byref(tab), C.byref(pl),
                                      C.byref(info)))
    _same({**ti, **td}, want[0], TABLE_STATS, "host table")
    _same({**pi, **pd}, want[1], ZONE_PLANES, "host planes")
    assert info.K == K and info.n_zones == nz and info.n_other == want[2]["n_other"]


def test_crosstab_refuses_a_zone_beyond_n_zones_and_too_many_codes(hip):
    import torch
    from machisplin_amd import _lib
    shape = (TR + 1, TC + 1)
    z, nodata = land_cover(shape, np.float32, NLCD, seed=9)
    zones = zone_planes(*shape)["rows"][0].copy()
    zones[-1, -1] = 40
    st = _stack(hip, z, nodata)
    with pytest.raises(hip.MhsError, match="holds zone 40, which is not below n_zones 33"):
        hip.classes.crosstab(st, torch.from_numpy(zones), classes=NLCD, n_zones=33)
    # without an info nothing is measured: the accumulate kernel raises the device flag, and no later phase writes
    zd = torch.from_numpy(zones).cuda()
    n = torch.full((33,), -9, dtype=torch.int32, device="cuda")
    mode = torch.full(shape, -9, dtype=torch.int32, device="cuda")
    tab, pl = _lib.ClassTable(33, None, n.data_ptr()), _lib.ClassPlanes(mode.data_ptr())
    pl.ld, pl.dtype = shape[1], _lib.F64
    g, cs = st.geom.c_struct(), st.c_struct()
    cl = (C.c_int32 * len(NLCD))(*NLCD)
    rc = _lib.lib().mhs_class_crosstab_dev(C.byref(g), C.byref(cs), 0, zd.data_ptr(), shape[1], 33, cl, len(NLCD), None, 0, C.byref(tab), C.byref(pl), None, None)
    assert rc == _lib.ERR_INVALID and "not below n_zones 33" in _lib.lib().mhs_last_error().decode()
    torch.cuda.synchronize()
    assert bool((n == -9).all()) and bool((mode == -9).all())
    # 257 distinct codes with classes=None
    many = (np.arange(shape[0] * shape[1]) % 257 + 1000).reshape(shape).astype(np.float32)
    with pytest.raises(hip.MhsError, match="holds 257 distinct codes"):
        hip.classes.crosstab(_stack(hip, many), torch.from_numpy(zones))
    ok = np.where(many == 1256, NAN, many).astype(np.float32)              # 256 of them are fine
    _crosstab(hip, _stack(hip, ok), zones, cr.crosstab(ok, zones), "256 measured codes")


def test_crosstab_n_equals_zonal_count(hip):
    import torch
    z, nodata = land_cover(BIG, np.int16, NLCD, seed=11)
    zones, nz = zone_planes(*BIG)["holes"]
    st, zt = _stack(hip, z, nodata), torch.from_numpy(zones)
    table, _, _ = hip.classes.crosstab(st, zt, classes=NLCD, n_zones=nz, stats=("n", "cells"))
    ztab, _, _ = hip.zonal.zonal(st, zt, stats=("count", "cells"), n_zones=nz)
    assert torch.equal(table["n"].long(), ztab["count"]) and torch.equal(table["cells"].long(), ztab["cells"])


# --------------------------------------------------------------------------------------------------------------- aggregate

def _aggregate(hip, z, nodata, S, T, tag, classes=NLCD, **kw):
    import torch
    kw.setdefault("products", AGG)
    st = kw.pop("stack", None) or _stack(hip, z, nodata, geom=S)
    planes, info = hip.classes.aggregate(st, T, classes=classes, **kw)
    want, winfo = cr.aggregate(z, S, T, classes, nodata, kw.get("frac_of", ()))
    _same(planes, want, kw["products"], tag, kw.get("out_dtype") is torch.float32)
    _info(info, winfo, tag)
    return planes, want


@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32", "i16"])
def test_aggregate_factors_shifts_and_targets_off_the_source(hip, dtype):
    import torch
    S = hip.Geometry(500.0, 900.0, 2.0, 2.0, 77, 103)
    z, nodata = land_cover((S.nrow, S.ncol), dtype, NLCD, seed=13)
    st = _stack(hip, z, nodata, geom=S)
    cases = {"itself": S, "factor 2": hip.Geometry(500.0, 900.0, 4.0, 4.0, 39, 52), "factor 3": hip.Geometry(500.0, 900.0, 6.0, 6.0, 26, 35),
             "factor 25": hip.Geometry(500.0, 900.0, 50.0, 50.0, 4, 5), "factor 2.5 shifted": hip.Geometry(500.0 + 0.37 * 2.0, 900.0 - 0.37 * 2.0, 5.0, 5.0, 31, 41),
             "partly outside": hip.Geometry(450.0, 930.0, 8.0, 8.0, 20, 20), "wholly outside": hip.Geometry(2000.0, 900.0, 4.0, 4.0, 5, 7),
             "finer": hip.Geometry(520.0, 880.0, 0.7, 0.7, 50, 60)}
    for name, T in cases.items():
        planes, want = _aggregate(hip, z, nodata, S, T, name, stack=st, frac_of=(42, 11))
        if name == "itself":
            ok = cr.valid(z, nodata)[1]
            assert np.array_equal(want["n"], ok.astype(np.int32)) and np.array_equal(want["mode"][ok & (want["mode"] >= 0)], z[ok & (want["mode"] >= 0)].astype(np.int32))
        if name == "wholly outside":
            assert int(planes["n"].sum()) == 0 and bool((planes["mode"] == -1).all()) and bool(torch.isnan(planes["frac"]).all())
        if name == "finer":
            assert (want["n"] == 0).any() and (want["n"] == 1).any()
    _aggregate(hip, z, nodata, S, cases["factor 3"], "float32", stack=st, out_dtype=torch.float32)
    _aggregate(hip, z, nodata, S, cases["factor 2.5 shifted"], "measured", stack=st, classes=None)
    _aggregate(hip, z, nodata, S, cases["factor 3"], "strided", stack=_stack(hip, z, nodata, pad=5, geom=S), layer=1, products=("mode", "frac"))


@pytest.mark.parametrize("K", [1, 16, 256])
def test_aggregate_targets_around_the_tile_size(hip, K):
    codes = class_list(K, "table" if K != 256 else "bisect")
    tr, tc = aggregate_tile(K, 10 ** 6, 10 ** 6)                           # the tile that the LDS budget gives: a target of many tiles
    assert tr * tc * (K + 2) <= AGG_WORDS and (tr, tc) == {1: (64, 64), 16: (14, 64), 256: (1, 63)}[K]
    # a target of few tiles is cut into smaller ones: every tile shape on the way down, one below, at and one above
    shapes = [(tr - 1, tc), (tr, tc), (tr + 1, tc), (tr, tc - 1), (tr, tc + 1), (2 * tr + 1, 2 * tc + 1), (1, 1), (1, AGG_MIN_COLS + 1), (3, 2 * AGG_MIN_COLS)]
    seen = set()
    for nr, nc in shapes:
        if nr < 1 or nc < 1:
            continue
        seen.add(aggregate_tile(K, nr, nc))
        S = hip.Geometry(0.0, 2.0 * nr, 1.0, 1.0, 2 * nr, 2 * nc)
        T = hip.Geometry(0.0, 2.0 * nr, 2.0, 2.0, nr, nc)
        z, nodata = land_cover((S.nrow, S.ncol), np.float32, codes, seed=K, blobs=False)
        _aggregate(hip, z, nodata, S, T, f"K {K} target {nr}x{nc}", classes=codes, products=("mode", "n", "variety", "simpson"))
    assert len(seen) >= 3 and all(t[0] == 1 for t in seen)                 # these targets are small: one row of cells to a tile
    # a narrow target: the tile grows in rows
    S, T = hip.Geometry(0.0, 300.0, 1.0, 1.0, 300, 6), hip.Geometry(0.0, 300.0, 2.0, 2.0, 150, 3)
    z, nodata = land_cover((300, 6), np.int16, codes, seed=K)
    _aggregate(hip, z, nodata, S, T, f"K {K} narrow", classes=codes)


def test_aggregate_a_target_of_enough_tiles_keeps_the_full_tile(hip):
    K = 16
    codes = class_list(K, "table")
    tr, tc = aggregate_tile(K, 10 ** 6, 10 ** 6)
    for nr, nc in ((32 * tr + 1, 64 * tc + 1), (45 * tr, 45 * tc)):    # the second has too few tiles of that size: its tile rows are halved
        full = aggregate_tile(K, nr, nc) == (tr, tc)
        assert full == (-(-nr // tr) * -(-nc // tc) >= AGG_MIN_TILES)
        S = hip.Geometry(0.0, float(nr), 1.0, 1.0, nr, nc)                 # onto itself: every footprint is one cell
        z, nodata = land_cover((nr, nc), np.int16, codes, seed=3)
        _aggregate(hip, z, nodata, S, S, f"{nr}x{nc}", classes=codes, products=("mode", "n", "frac"), frac_of=(codes[2], codes[9]))


def test_aggregate_one_wide_and_tall_footprint_and_the_other_routes(hip):
    import torch
    S = hip.Geometry(0.0, 90.0, 1.0, 1.0, 90, 150)
    T = hip.Geometry(0.0, 90.0, 70.0, 40.0, 3, 3)                          # footprints 70 wide, 40 tall, and the clipped ones
    z, nodata = land_cover((S.nrow, S.ncol), np.float32, NLCD, seed=17)
    st = _stack(hip, z, nodata, geom=S)
    planes, want = _aggregate(hip, z, nodata, S, T, "70 x 40 footprints", stack=st)
    assert want["n"].max() > 64 * 32
    # the same units as zones: crosstab on the plane of target-cell numbers
    unit = cr.target_cells(S, T).astype(np.int32)
    table, _, _ = hip.classes.crosstab(st, torch.from_numpy(unit), classes=NLCD, n_zones=9, stats=("n", "mode", "mode_frac", "variety", "simpson", "frac"))
    for k in ("n", "mode", "mode_frac", "variety", "simpson"):
        assert _bits(table[k].reshape(3, 3).cpu().numpy(), planes[k].cpu().numpy()), k
    assert _bits(table["frac"].T.reshape(-1, 3, 3).contiguous().cpu().numpy(), planes["frac"].cpu().numpy())
    # n is resample's count and frac its mean of the indicator, on the device
    T2 = hip.Geometry(0.74, 89.26, 5.0, 5.0, 19, 31)
    p2, _ = _aggregate(hip, z, nodata, S, T2, "2.5 shifted", stack=st, products=("n", "frac"), frac_of=(41, 90))
    count = hip.resample.resample(st, T2, "count", out_dtype=torch.float64).planes[0]
    assert torch.equal(p2["n"].double(), count)
    zt = st.planes[0].double()
    for j, code in enumerate((41, 90)):
        ind = torch.where(torch.isnan(zt), zt, (zt == code).double())
        mean = hip.resample.resample(hip.RasterStack(S, ind[None]), T2, "mean", out_dtype=torch.float64).planes[0]
        assert _bits(p2["frac"][j].cpu().numpy(), mean.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------- focal

def _focal(hip, z, nodata, R, tag, classes, **kw):
    import torch
    kw.setdefault("products", FOCAL)
    st = kw.pop("stack", None) or _stack(hip, z, nodata)
    planes, info = hip.classes.focal(st, R, classes=classes, **kw)
    want, winfo = cr.focal(z, R, classes, nodata, kw.get("frac_of", ()), kw.get("shape", "square"))
    _same(planes, want, kw["products"], tag, kw.get("out_dtype") is torch.float32)
    _info(info, winfo, tag)
    return planes


@pytest.mark.parametrize("shape,R", [("square", 1), ("square", 31), ("square", 32), ("square", 33), ("square", BIG[1]), ("circle", 1), ("circle", 17)])
def test_focal_radii_and_shapes(hip, shape, R):
    import torch
    z, nodata = land_cover(BIG, np.int16, [11, 41, 82], seed=19)
    st = _stack(hip, z, nodata)
    planes = _focal(hip, z, nodata, R, f"{shape} {R}", [41, 11, 82], stack=st, shape=shape, frac_of=(82, 11))
    # frac is focal's mean of the indicator at offset 0
    zt = st.planes[0]
    for j, code in enumerate((82, 11)):
        ind = torch.where(zt == -32768, zt, (zt == code).to(torch.int16))
        mean = hip.focal.focal(hip.RasterStack(st.geom, ind[None], -32768.0), R, "mean", shape=shape, offset=0.0)
        assert _bits(planes["frac"][j].cpu().numpy(), mean.cpu().numpy())


@pytest.mark.parametrize("K", [1, 3, 256])
@pytest.mark.parametrize("grid", [(1, 1), (1, TC + 1), (TR + 1, 1), (TR + 1, TC + 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_focal_class_counts_and_grids(hip, K, grid):
    import torch
    codes = class_list(K, "bisect" if K == 256 else "table")
    z, nodata = land_cover(grid, np.float32, codes, seed=K, blobs=False)
    _focal(hip, z, nodata, 1, f"K {K} {grid}", codes)
    if K == 3:
        _focal(hip, z, nodata, max(grid), "largest radius, float32, measured", None, out_dtype=torch.float32, products=("mode", "frac", "n"))
        _focal(hip, z, nodata, min(2, max(grid)), "strided", codes, stack=_stack(hip, z, nodata, pad=3), layer=1, shape="circle")


# ------------------------------------------------------------------------------------------------------------ a larger case

def test_a_larger_land_cover_through_the_three_calls(hip):
    import torch
    nr, nc, K = 1500, 1700, 20
    codes = list(range(10, 10 + 5 * K, 5))
    r, c = np.meshgrid(np.arange(nr, dtype=np.float32), np.arange(nc, dtype=np.float32), indexing="ij")
    field = np.sin(r / 61.0) * np.cos(c / 47.0) + 0.6 * np.sin((r + 2 * c) / 97.0) + 0.25 * np.cos((3 * r - c) / 29.0)
    z = np.asarray(codes, dtype=np.int16)[np.digitize(field, np.linspace(field.min(), field.max() + 1e-6, K + 1)[1:-1])]
    rng = np.random.default_rng(23)
    z[rng.random(z.shape) < 0.02] = -32768
    z[rng.random(z.shape) < 0.01] = 7
    S = hip.Geometry(0.0, 1500.0, 1.0, 1.0, nr, nc)
    st = _stack(hip, z, -32768.0, geom=S)
    zones = ((np.arange(nr)[:, None] // 30) * 55 + np.arange(nc)[None, :] // 31).astype(np.int32)
    assert zones.max() + 1 == 2750
    table, _, info = hip.classes.crosstab(st, torch.from_numpy(zones), classes=codes, stats=("counts", "other", "cells", "mode", "simpson"))
    slot = np.searchsorted(codes, z)
    hit = (slot < K) & (np.asarray(codes)[np.minimum(slot, K - 1)] == z)
    flat = np.bincount(zones[hit].astype(np.int64) * K + slot[hit], minlength=2750 * K).reshape(2750, K)
    assert np.array_equal(table["counts"].cpu().numpy(), flat.astype(np.int32)) and info["n_zones"] == 2750
    want = cr.crosstab(z, zones, codes, -32768.0, with_planes=False)
    _same(table, want[0], ("counts", "other", "cells", "mode", "simpson"), "large crosstab")
    _info(info, want[2], "large crosstab")
    T = hip.Geometry(0.0, 1500.0, 25.0, 25.0, 60, 68)
    _aggregate(hip, z, -32768.0, S, T, "large aggregate", classes=codes, stack=st)
    # focal over all 20 classes; frac and n do not depend on the other classes of the list, so the restatement is made with two
    two = (codes[3], codes[11])
    planes, info = hip.classes.focal(st, 40, classes=codes, frac_of=two, products=("frac", "n"))
    want, _ = cr.focal(z, 40, two, -32768.0)
    _same(planes, want, ("frac", "n"), "large focal")
    assert info["K"] == K and info["n_other"] == int((z == 7).sum())


# -------------------------------------------------------------------------------------------------------------- covariates

def test_covariates_class_specs_and_an_old_spec_list_unchanged(hip):
    import torch
    g = hip.Geometry(1000.0, 5000.0, 30.0, 30.0, TR + 8, TC + 9)
    r, c = np.meshgrid(np.arange(g.nrow), np.arange(g.ncol), indexing="ij")
    dem = (300.0 + 40.0 * np.sin(r / 9.0) + 25.0 * np.cos(c / 11.0) + 0.5 * r).astype(np.float32)
    dem[5, 7] = NAN
    dem_stack = hip.RasterStack(g, dem[None])
    z, nodata = land_cover((g.nrow, g.ncol), np.int16, NLCD, seed=29)
    cat = _stack(hip, z, nodata, geom=g)
    fine = hip.Geometry(g.xmin - 45.0, g.ymax + 20.0, 10.0, 10.0, 3 * g.nrow + 10, 3 * g.ncol + 5)      # finer, shifted, partly off the DEM
    zf, nodata_f = land_cover((fine.nrow, fine.ncol), np.float32, NLCD, seed=31)
    two = hip.RasterStack(fine, np.stack([np.zeros_like(zf), zf]), nodata_f)
    old = ("slope_deg", ("above_min", 5), ("focal_mean", 9))
    spec = old + (("class_frac", cat, 41, 3), ("class_cover", (two, 1), 42), ("class_frac", cat, 11, 3), ("class_frac", cat, 41, 8),
                  ("class_cover", (two, 1), 90))
    before = hip.covariates(dem_stack, old)
    got = hip.covariates(dem_stack, spec)
    assert got.names == ["dem", "slope_deg", "above_min5", "focal_mean9", "class_frac41_3", "class_cover42", "class_frac11_3", "class_frac41_8", "class_cover90"]
    assert got.planes.dtype == torch.float32 and got.planes[:4].cpu().numpy().tobytes() == before.planes.cpu().numpy().tobytes()
    again = hip.covariates(dem_stack, old)
    assert again.names == before.names and again.planes.cpu().numpy().tobytes() == before.planes.cpu().numpy().tobytes()
    for k, (code, R) in ((4, (41, 3)), (6, (11, 3)), (7, (41, 8))):
        want, _ = cr.focal(z, R, [code], nodata)
        assert _bits(got.planes[k].cpu().numpy(), want["frac"][0].astype(np.float32)), (code, R)
    for k, code in ((5, 42), (8, 90)):
        want, _ = cr.aggregate(zf, fine, g, [code], nodata_f)
        assert _bits(got.planes[k].cpu().numpy(), want["frac"][0].astype(np.float32)), code
    with pytest.raises(ValueError, match="DEM's own grid"):
        hip.covariates(dem_stack, (("class_frac", two, 41, 3),))
    with pytest.raises(ValueError, match="class code"):
        hip.covariates(dem_stack, (("class_cover", cat, 41.5),))
    with pytest.raises(ValueError, match="'class_frac' takes"):
        hip.covariates(dem_stack, (("class_frac", cat, 41),))
