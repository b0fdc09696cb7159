"""GPU: rasters onto one grid (csrc/resample.hip, machisplin_amd/resample.py) against the numpy restatement of the rules
(tests/resample_ref.py), bit for bit, NaN where it is NaN: the library is built without contraction, the header fixes the
order of the operations and no method has a transcendental in it.

Sources: 37 x 83 and 70 x 131 cells of 30 x 28.5 units (origin and cell size make a cell centre's coordinate exact, so the same
grid must give the source back), built like the planes of test_terrain_gpu.py: seeded noise on a trend, a level patch, about 2 %
of the cells NA in clusters (the nodata -32768 everywhere, NaN too in float planes); int16, float32 and float64.  A stack is 3
layers cut out of a 4-layer tensor with 5 columns of padding, so neither its row stride nor its layer stride is the plane's.
One 150 x 300 source serves the 75 x coarser target, whose footprint of 5 625 cells is wider than a wave and larger than a
staged chunk."""
import ctypes as C
import functools

import numpy as np
import pytest

import resample_ref as rr

pytestmark = pytest.mark.gpu

NODATA = -32768.0
DX, DY = 30.0, 28.5
X0, Y0 = 1000.0, 5000.0
SHAPES = ((37, 83), (70, 131))
DTYPES = ("f64", "f32", "i16")
NP_DT = {"f64": np.float64, "f32": np.float32, "i16": np.int16}
WINDOW = (5, 29, 7, 60)
INTERP = ("near", "bilinear", "cubic")
AGGREGATES = ("mean", "min", "max", "sum", "count")
PLANES = [(s, d) for s in SHAPES for d in DTYPES]
PLANE_IDS = [f"{s[0]}x{s[1]}-{d}" for s, d in PLANES]


def _geom(shape):
    from machisplin_amd import Geometry
    return Geometry(X0, Y0, DX, DY, shape[0], shape[1])


@functools.lru_cache(maxsize=None)
def _planes(shape, dtype):
    """the 4 layers the stack is cut from, as the plane type holds them (numpy), built once"""
    nr, nc = shape
    out = []
    for layer in range(4):
        rng = np.random.default_rng(4000 * nr + 4 * nc + 16 * {"f64": 0, "f32": 1, "i16": 2}[dtype] + layer)
        r, c = np.meshgrid(np.arange(nr, dtype=np.float64), np.arange(nc, dtype=np.float64), indexing="ij")
        z = 800.0 + (6.0 - layer) * r - 3.5 * c + 40.0 * np.sin(r / 7.0) * np.cos(c / 9.0) + 25.0 * rng.standard_normal(shape)
        z[nr // 2:nr // 2 + 9, nc // 2:nc // 2 + 11] = 1234.0                  # a level patch: exact ties
        z = np.rint(z).astype(np.int16) if dtype == "i16" else z.astype(NP_DT[dtype])
        for k in range(max(2, int(0.02 * nr * nc / 6))):                       # about 2 % of the cells, in clusters of ~6
            r0, c0 = rng.integers(0, nr), rng.integers(0, nc)
            h, w = rng.integers(1, 4), rng.integers(1, 5)
            z[r0:r0 + h, c0:c0 + w] = np.nan if (dtype != "i16" and k % 2) else NP_DT[dtype](NODATA)
        out.append(z)
    return np.stack(out)


def _host(shape, dtype):
    """the stack's 3 layers on the host"""
    return _planes(shape, dtype)[1:4]


@functools.lru_cache(maxsize=None)
def _stack(shape, dtype):
    """layers 1 .. 3 of a 4-layer device tensor whose rows carry 5 columns of padding: ld = ncol + 5, layer stride nrow ld"""
    import torch
    import machisplin_amd as hip
    nr, nc = shape
    st = hip.RasterStack(_geom(shape), _host(shape, dtype), NODATA)
    big = torch.full((4, nr, nc + 5), -7, dtype=st.planes.dtype, device=st.planes.device)
    big[:, :, :nc] = torch.from_numpy(_planes(shape, dtype)).to(big.device)
    st.planes = big[1:4, :, :nc]
    assert st.c_struct().ld == nc + 5 and st.c_struct().plane_stride == nr * (nc + 5) != nr * nc
    return st


def _targets(shape):
    """the target grids of a source, by name"""
    from machisplin_amd import Geometry
    nr, nc = shape
    t = {
        "same": _geom(shape),
        # 3 x coarser, aligned; the last row and column of targets reach beyond the source
        "coarse3": Geometry(X0, Y0, 3 * DX, 3 * DY, -(-nr // 3), -(-nc // 3)),
        # 3.7 x coarser, shifted: footprints of 3 and 4 that vary; starts inside the source, ends beyond it
        "coarse3.7": Geometry(X0 + 1.3 * DX, Y0 - 0.7 * DY, 3.7 * DX, 3.7 * DY, int(nr / 3.7) + 1, int(nc / 3.7) + 1),
        # anisotropic: xres halved, yres times 2.5
        "aniso": Geometry(X0 - 1.25 * DX, Y0 + 0.4 * DY, 0.5 * DX, 2.5 * DY, int(nr / 2.5) + 2, 2 * nc + 6),
        # a ratio near 1 on the tile + 1 sizes
        "near1": Geometry(X0 + 0.2 * DX, Y0 - 0.45 * DY, 1.05 * DX, 0.97 * DY, *((33, 65) if shape == SHAPES[0] else (65, 129))),
        # 4.3 x finer, the origin shifted by 0.37 and 0.61 of a source cell, 5 source cells beyond the source on every side
        "fine4.3": Geometry(X0 - 5.37 * DX, Y0 + 5.61 * DY, DX / 4.3, DY / 4.3, int((nr + 10.9) * 4.3), int((nc + 10.9) * 4.3)),
    }
    return t


TARGET_NAMES = ("same", "coarse3", "coarse3.7", "aniso", "near1", "fine4.3")
CASES = [(s, d, t) for s, d in PLANES for t in TARGET_NAMES]
CASE_IDS = [f"{s[0]}x{s[1]}-{d}-{t}" for s, d, t in CASES]


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@functools.lru_cache(maxsize=None)
def _want(shape, dtype, target, method, window=None):
    S, T = _geom(shape), _targets(shape)[target]
    return np.stack([rr.resample(z, NODATA, S, T, method, window) for z in _host(shape, dtype)])


def _got(shape, dtype, target, method, **kw):
    import torch
    from machisplin_amd.resample import resample
    kw.setdefault("out_dtype", torch.float64)
    return resample(_stack(shape, dtype), _targets(shape)[target], method, **kw).planes.cpu().numpy()


@pytest.mark.parametrize("shape,dtype,target", CASES, ids=CASE_IDS)
def test_every_method_equals_the_restatement_bit_for_bit(hip, shape, dtype, target):
    for method in rr.METHODS:
        got, want = _got(shape, dtype, target, method), _want(shape, dtype, target, method)
        assert got.dtype == np.float64 and _same(got, want), method
    src = rr.to_double(_host(shape, dtype), NODATA)
    near = _want(shape, dtype, target, "near")
    if target == "same":
        for method in ("near", "bilinear", "cubic", "mean", "min", "max"):
            assert _same(_want(shape, dtype, target, method), src), method
        assert _same(_want(shape, dtype, target, "count"), (~np.isnan(src)).astype(np.float64))
    elif target == "fine4.3":
        T, S = _targets(shape)[target], _geom(shape)
        x, y = rr.cell_x(T, np.arange(T.ncol)), rr.cell_y(T, np.arange(T.nrow))
        outside = (y[:, None] > S.ymax) | (y[:, None] < S.ymin) | (x[None, :] < S.xmin) | (x[None, :] > S.xmax)
        assert outside.mean() > 0.15
        for method in INTERP:
            w = _want(shape, dtype, target, method)
            assert np.isnan(w[:, outside]).all() and 0.9 < (~np.isnan(w[:, ~outside])).mean() < 1.0, method
        assert (_want(shape, dtype, target, "count") <= 1.0).all() and np.isnan(_want(shape, dtype, target, "mean")).mean() > 0.9
    elif target == "coarse3" and dtype == "i16":
        # the aligned integer factor: the aggregates of an int16 plane are numpy's over the 3 x 3 blocks
        nr, nc = (shape[0] // 3) * 3, (shape[1] // 3) * 3
        blocks = src[:, :nr, :nc].reshape(3, nr // 3, 3, nc // 3, 3).transpose(0, 1, 3, 2, 4).reshape(3, nr // 3, nc // 3, 9)
        with np.errstate(all="ignore"):
            cnt = (~np.isnan(blocks)).sum(axis=3)
            mean = np.where(cnt > 0, np.nansum(blocks, axis=3) / cnt, np.nan)
            mn = np.where(cnt > 0, np.min(np.where(np.isnan(blocks), np.inf, blocks), axis=3), np.nan)
            mx = np.where(cnt > 0, np.max(np.where(np.isnan(blocks), -np.inf, blocks), axis=3), np.nan)
        for method, ref in (("mean", mean), ("min", mn), ("max", mx), ("count", cnt.astype(np.float64))):
            assert _same(_want(shape, dtype, target, method)[:, :nr // 3, :nc // 3], ref), method
    elif target == "coarse3.7":
        # the footprints partition the source: COUNT summed = the valid source cells whose centre lies in the target's extent
        T, S = _targets(shape)[target], _geom(shape)
        x, y = rr.cell_x(S, np.arange(S.ncol)), rr.cell_y(S, np.arange(S.nrow))
        inside = ((y <= T.ymax) & (y > T.ymin))[:, None] & ((x >= T.xmin) & (x < T.xmax))[None, :]
        cnt = _want(shape, dtype, target, "count")
        assert 0.5 < inside.mean() < 1.0 and set(np.unique(cnt)) >= {9.0, 12.0, 16.0}
        for k in range(3):
            assert cnt[k].sum() == (~np.isnan(src[k]) & inside).sum()
    assert np.isnan(near).any() and (~np.isnan(near)).any()


def test_large_footprint_75x_coarser(hip):
    """150 x 300 onto 2 x 4: a footprint of 75 x 75 = 5 625 cells, wider than a wave and larger than one staged chunk; the
    interpolating methods on the same target read their taps straight from global memory"""
    import torch
    from machisplin_amd import Geometry, RasterStack
    from machisplin_amd.resample import resample
    rng = np.random.default_rng(75)
    S = Geometry(X0, Y0, DX, DY, 150, 300)
    T = Geometry(X0, Y0, 75 * DX, 75 * DY, 2, 4)
    z = (500.0 + 100.0 * rng.standard_normal((2, 150, 300))).astype(np.float32)
    z[0, 10:40, 100:180] = np.nan
    z[1, rng.integers(0, 150, 500), rng.integers(0, 300, 500)] = NODATA
    stack = RasterStack(S, z, NODATA)
    for method in rr.METHODS:
        got = resample(stack, T, method, out_dtype=torch.float64).planes.cpu().numpy()
        want = np.stack([rr.resample(p, NODATA, S, T, method) for p in z])
        assert _same(got, want), method
    cnt = resample(stack, T, "count", out_dtype=torch.float64).planes.cpu().numpy()
    assert cnt[0].max() == 5625.0 and cnt[0].sum() == 150 * 300 - 30 * 80
    # a source narrower than its footprint chunking: one target cell over everything (a band 300 columns wide, 150 rows deep)
    T1 = Geometry(X0 - DX, Y0 + DY, 400 * DX, 400 * DY, 1, 1)
    for method in AGGREGATES:
        got = resample(stack, T1, method, out_dtype=torch.float64).planes.cpu().numpy()
        assert _same(got, np.stack([rr.resample(p, NODATA, S, T1, method) for p in z])), method


@pytest.mark.parametrize("dtype", DTYPES)
def test_window_float32_output_and_repeat(hip, dtype):
    import torch
    from machisplin_amd.resample import resample
    shape = SHAPES[0]
    stack = _stack(shape, dtype)
    r0, r1, c0, c1 = WINDOW
    for target in ("fine4.3", "coarse3.7"):
        T = _targets(shape)[target]
        win = WINDOW if target == "fine4.3" else (2, 9, 3, 20)
        for method in ("bilinear", "cubic", "near", "mean", "max"):
            whole = _got(shape, dtype, target, method)
            # a window equals that slice of the whole-grid call, and comes on the window's geometry
            res = resample(stack, T, method, out_dtype=torch.float64, window=win)
            assert res.geom == T.window(*win) and np.isnan(res.nodata)
            assert _same(res.planes.cpu().numpy(), whole[:, win[0]:win[1], win[2]:win[3]]), (target, method)
            assert _same(whole[:, win[0]:win[1], win[2]:win[3]], _want(shape, dtype, target, method, win)), (target, method)
            # a float32 output is the float64 result rounded once; the default type is float32 unless the source is float64
            got32 = _got(shape, dtype, target, method, out_dtype=torch.float32)
            assert _same(got32, whole.astype(np.float32)), (target, method)
            default = resample(stack, T, method).planes
            assert default.dtype == (torch.float64 if dtype == "f64" else torch.float32)
            # a repeat call gives the same bits
            assert _same(_got(shape, dtype, target, method), whole), (target, method)
    # a padded output keeps its padding
    T = _targets(shape)["fine4.3"]
    big = torch.full((3, r1 - r0, 71), -7.0, dtype=torch.float64, device=stack.planes.device)
    res = resample(stack, T, "cubic", window=WINDOW, out=big[:, :, :c1 - c0])
    assert res.planes.stride(1) == 71 and (big[:, :, c1 - c0:] == -7.0).all()
    assert _same(res.planes.cpu().numpy(), _got(shape, dtype, "fine4.3", "cubic")[:, r0:r1, c0:c1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_entry_equals_the_device_entry_with_several_bands(hip, monkeypatch, dtype):
    from machisplin_amd import _lib
    shape = SHAPES[1]
    z = np.ascontiguousarray(_host(shape, dtype))
    nr, nc = shape
    sg = _geom(shape).c_struct()
    ss = _lib.Stack(z.ctypes.data, 3, {"f64": _lib.F64, "f32": _lib.F32, "i16": _lib.I16}[dtype], nr * nc, nc, NODATA)
    for target, methods in (("near1", INTERP), ("coarse3.7", rr.METHODS), ("aniso", ("cubic", "mean"))):
        T = _targets(shape)[target]
        tg = T.c_struct()
        for bands in (None, "5"):
            if bands:
                monkeypatch.setenv("MHS_HOST_BANDS", bands)
            for method in methods:
                out = np.full((3, T.nrow, T.ncol), -7.0)
                _lib.check(_lib.lib().mhs_resample(C.byref(sg), C.byref(ss), C.byref(tg), 0, T.nrow, 0, T.ncol, rr.METHODS.index(method),
                                                   out.ctypes.data, _lib.F64))
                assert _same(out, _got(shape, dtype, target, method)), (target, bands, method)
            win = (3, T.nrow - 2, 1, T.ncol - 4)
            out32 = np.full((3, win[1] - win[0], win[3] - win[2]), -7.0, dtype=np.float32)
            _lib.check(_lib.lib().mhs_resample(C.byref(sg), C.byref(ss), C.byref(tg), *win, rr.METHODS.index(methods[-1]), out32.ctypes.data, _lib.F32))
            assert _same(out32, _got(shape, dtype, target, methods[-1])[:, win[0]:win[1], win[2]:win[3]].astype(np.float32)), (target, bands)
        monkeypatch.delenv("MHS_HOST_BANDS")


@pytest.mark.parametrize("shape,dtype", PLANES, ids=PLANE_IDS)
def test_extract_at_points(hip, shape, dtype):
    from machisplin_amd import _lib, mltps
    from machisplin_amd.resample import extract
    stack, S = _stack(shape, dtype), _geom(shape)
    src = rr.to_double(_host(shape, dtype), NODATA)
    # at all cell centres every method gives the plane
    cols, rows = np.meshgrid(np.arange(S.ncol), np.arange(S.nrow))
    centres = np.column_stack([S.x_from_col(cols.ravel()), S.y_from_row(rows.ravel())])
    for method in ("simple", "bilinear", "cubic"):
        assert _same(extract(stack, centres, method), src.reshape(3, -1).T.copy()), method
    # 500 seeded points, a tenth of them outside the extent, two on the far edges, one NaN
    rng = np.random.default_rng(500 + shape[0])
    xy = np.column_stack([rng.uniform(S.xmin, S.xmax, 500), rng.uniform(S.ymin, S.ymax, 500)])
    xy[:25, 0] = S.xmin - rng.uniform(0.01, 3.0, 25) * DX
    xy[25:50, 1] = S.ymax + rng.uniform(0.01, 3.0, 25) * DY
    xy[50] = (S.xmax, S.ymin)
    xy[51] = (S.xmin, S.ymax)
    xy[52, 0] = np.nan
    for method in ("simple", "bilinear", "cubic"):
        got = extract(stack, xy, method)
        want = np.column_stack([rr.extract(z, NODATA, S, xy, method) for z in _host(shape, dtype)])
        assert got.shape == (500, 3) and _same(got, want), method
        assert np.isnan(got[:50]).all() and np.isnan(got[52]).all() and (~np.isnan(got)).mean() > 0.8
        # the host entry point gives the same
        z = np.ascontiguousarray(_host(shape, dtype))
        ss = _lib.Stack(z.ctypes.data, 3, {"f64": _lib.F64, "f32": _lib.F32, "i16": _lib.I16}[dtype], z[0].size, shape[1], NODATA)
        sg, pts, out = S.c_struct(), np.ascontiguousarray(xy.T), np.full((3, 500), -7.0)
        _lib.check(_lib.lib().mhs_extract_points(C.byref(sg), C.byref(ss), pts.ctypes.data, 500, {"simple": 0, "bilinear": 1, "cubic": 2}[method],
                                                 out.ctypes.data))
        assert _same(out.T.copy(), want), method
    # "simple" is the cell lookup of the stations' predictors
    X, _, _ = mltps.station_predictors(stack, xy[53:])
    assert _same(extract(stack, xy[53:], "simple"), np.ascontiguousarray(X[:, :3]))


def test_align_three_stacks_on_different_grids(hip):
    import torch
    from machisplin_amd import Geometry, RasterStack, mltps
    from machisplin_amd.resample import align, resample
    first = _stack((70, 131), "i16")
    g = first.geom
    rng = np.random.default_rng(19)
    coarse_g = Geometry(X0 - 0.3 * DX, Y0 + 0.1 * DY, 3.7 * DX, 3.7 * DY, 19, 35)        # 3.7 x the cell size, shifted; ends short of the east edge
    coarse = RasterStack(coarse_g, (15.0 + 3.0 * rng.standard_normal((2, 19, 35))).astype(np.float32), float("nan"))
    part = RasterStack(Geometry(X0 + 20.5 * DX, Y0 - 11.25 * DY, 0.8 * DX, 0.8 * DY, 37, 83), _planes((37, 83), "f64")[:1], NODATA)
    out = align([first, coarse, part], methods=["near", "cubic", "bilinear"])
    assert isinstance(out, RasterStack) and out.geom == g and out.planes.dtype == torch.float32 and out.n_layers == 6 and np.isnan(out.nodata)
    planes = out.planes.cpu().numpy()
    # the first stack is on the target grid: its int16 values converted, NA as NaN
    assert _same(planes[:3], rr.to_double(_host((70, 131), "i16"), NODATA).astype(np.float32))
    # the others equal the single calls, and the restatement
    assert _same(planes[3:5], resample(coarse, g, "cubic", out_dtype=torch.float32).planes.cpu().numpy())
    assert _same(planes[5:], resample(part, g, "bilinear", out_dtype=torch.float32).planes.cpu().numpy())
    want = rr.resample(_planes((37, 83), "f64")[0], NODATA, part.geom, g, "bilinear").astype(np.float32)
    assert _same(planes[5], want) and 0.1 < np.isnan(want).mean() < 0.9                  # it covers only part of the extent
    assert 0.0 < np.isnan(planes[3:5]).mean() < 0.05
    # one method for all, a target grid of its own
    T = _targets((70, 131))["near1"]
    both = align([first, coarse], T, "bilinear")
    assert both.geom == T and both.n_layers == 5
    assert _same(both.planes.cpu().numpy()[:3], _got((70, 131), "i16", "near1", "bilinear", out_dtype=torch.float32))
    # ... and goes straight into the stations' predictors and Mess
    xy = np.column_stack([rng.uniform(g.xmin, g.xmax, 200), rng.uniform(g.ymin, g.ymax, 200)])
    X, _, _ = mltps.station_predictors(out, xy)
    keep = ~np.isnan(X).any(axis=1)
    assert X.shape == (200, 8) and 10 < keep.sum() < 200
    mess = hip.Mess(X[keep][:, :6]).grid(out).cpu().numpy()
    assert np.array_equal(np.isnan(mess), np.isnan(planes).any(axis=0))
    with pytest.raises(ValueError):
        align([first, coarse], methods=["near"])

