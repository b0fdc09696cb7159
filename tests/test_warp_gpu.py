"""GPU: rasters onto a grid in another coordinate system (csrc/warp.hip, machisplin_amd/project.py) against the numpy
restatement of the section "warp" (tests/warp_ref.py: the lattice formula, then resample_ref.interp_points), bit for bit, NaN
where it is NaN: the library is built without contraction, the header fixes the order of the operations and the device runs no
transcendental.

Source: 70 x 90 cells of 1 / 1200 degree at the east side of UTM zone 31, built like the planes of test_resample_gpu.py: seeded
noise on a trend, a level patch, about 2 % of the cells NA in clusters (the nodata -32768 everywhere, NaN too in float planes);
int16, float32 and float64.  A stack is 3 layers cut out of a 4-layer tensor with 5 columns of padding.  The lattices:
  utm       a real project.lattice from UTM 31 (100 m cells) back to lon/lat onto 45 x 70: partial tiles on both axes, a band of
            the target beyond the source
  bend-K    33 x 130 cells under a gently curved map at K = 1, 4, 64, 256: the lattice cell smaller than a tile, as wide as a
            tile, larger than the grid (K = 1 and the nodes come from global memory, otherwise from LDS)
  rotated   an affine map turned by 30 degrees with shear: the staged rectangle is wide and skewed
  holes     a block of NaN nodes (and an infinite one), and a third of the target mapping outside the source
and, on a 700 x 900 source, a target cell of 20 source cells (no rectangle fits: every tile reads global memory) and one of 2.1
(float64: whole tiles do not fit, the partial tiles of the last column and row do)."""
import functools
import math

import numpy as np
import pytest

import resample_ref as rr
import warp_ref as wr

pytestmark = pytest.mark.gpu

NODATA = -32768.0
SHAPE = (70, 90)
DTYPES = ("f64", "f32", "i16")
NP_DT = {"f64": np.float64, "f32": np.float32, "i16": np.int16}
METHODS = ("near", "bilinear", "cubic")
WINDOW = (5, 40, 3, 67)
LATTICES = ("utm", "bend-1", "bend-4", "bend-64", "bend-256", "rotated", "holes")


def _geom():
    from machisplin_amd import Geometry
    return Geometry(5.625, 45.25, 1.0 / 1200.0, 1.0 / 1200.0, *SHAPE)


@functools.lru_cache(maxsize=None)
def _planes(shape, dtype):
    """the 4 layers a stack is cut from, as the plane type holds them (numpy), built once"""
    nr, nc = shape
    out = []
    for layer in range(4):
        rng = np.random.default_rng(7000 * nr + 4 * nc + 16 * {"f64": 0, "f32": 1, "i16": 2}[dtype] + layer)
        r, c = np.meshgrid(np.arange(nr, dtype=np.float64), np.arange(nc, dtype=np.float64), indexing="ij")
        z = 800.0 + (6.0 - layer) * r - 3.5 * c + 40.0 * np.sin(r / 7.0) * np.cos(c / 9.0) + 25.0 * rng.standard_normal(shape)
        z[nr // 2:nr // 2 + 9, nc // 2:nc // 2 + 11] = 1234.0                  # a level patch: exact ties
        z = np.rint(np.clip(z, -30000, 30000)).astype(np.int16) if dtype == "i16" else z.astype(NP_DT[dtype])
        for k in range(max(2, int(0.02 * nr * nc / 6))):                       # about 2 % of the cells, in clusters of ~6
            r0, c0 = rng.integers(0, nr), rng.integers(0, nc)
            h, w = rng.integers(1, 4), rng.integers(1, 5)
            z[r0:r0 + h, c0:c0 + w] = np.nan if (dtype != "i16" and k % 2) else NP_DT[dtype](NODATA)
        out.append(z)
    return np.stack(out)


def _host(dtype, shape=SHAPE):
    return _planes(shape, dtype)[1:4]


@functools.lru_cache(maxsize=None)
def _stack(dtype, geom=None, shape=SHAPE):
    """layers 1 .. 3 of a 4-layer device tensor whose rows carry 5 columns of padding: ld = ncol + 5, layer stride nrow ld"""
    import torch
    import machisplin_amd as hip
    nr, nc = shape
    st = hip.RasterStack(geom or _geom(), _host(dtype, shape), NODATA)
    big = torch.full((4, nr, nc + 5), -7, dtype=st.planes.dtype, device=st.planes.device)
    big[:, :, :nc] = torch.from_numpy(_planes(shape, dtype)).to(big.device)
    st.planes = big[1:4, :, :nc]
    assert st.c_struct().ld == nc + 5 and st.c_struct().plane_stride == nr * (nc + 5) != nr * nc
    return st


def _cells_map(S, T, col_of, row_of):
    """fn(X, Y) of a lattice from a map between CELL coordinates: u, v = the target's columns / rows as reals, col_of(u, v) and
    row_of(u, v) the source's"""
    def fn(X, Y):
        u, v = (X - T.xmin) / T.xres, (T.ymax - Y) / T.yres
        return S.xmin + col_of(u, v) * S.xres, S.ymax - row_of(u, v) * S.yres
    return fn


@functools.lru_cache(maxsize=None)
def _case(name):
    """(target geometry, lattice) by name; a lattice that is given its step is not held to a tolerance"""
    from machisplin_amd import Geometry, project as pj
    S = _geom()
    if name == "utm":
        crs = pj.utm(31)
        x, y = pj.transform(pj.LONLAT, crs, S.xmin + 0.5 * S.ncol * S.xres, S.ymax - 0.5 * S.nrow * S.yres)
        T = Geometry(math.floor(float(x) / 100.0) * 100.0 - 3500.0, math.floor(float(y) / 100.0) * 100.0 + 2200.0, 100.0, 100.0, 45, 70)
        lat = pj.lattice(pj.LONLAT, crs, T, S, tol=0.001)
        assert lat.step < 64                                       # several lattice cells under the one tile row
        return T, lat
    if name.startswith("bend-"):
        T = Geometry(0.0, 33.0, 1.0, 1.0, 33, 130)
        fn = _cells_map(S, T, lambda u, v: 2.0 + 0.6 * u + 0.0011 * u * v + 0.0004 * v * v, lambda u, v: 1.5 + 1.7 * v + 0.002 * u - 0.00007 * u * u)
        return T, pj.lattice_from(fn, T, S, tol=1e9, step=int(name[5:]))
    if name == "rotated":
        T = Geometry(0.0, 50.0, 1.0, 1.0, 50, 100)
        c, s = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
        fn = _cells_map(S, T, lambda u, v: 8.0 + 0.8 * (c * u + s * v) + 0.15 * v, lambda u, v: 40.0 + 0.8 * (-s * u + c * v))
        return T, pj.lattice_from(fn, T, S, tol=1e9, step=16)
    if name == "holes":
        T = Geometry(0.0, 45.0, 1.0, 1.0, 45, 70)
        fn = _cells_map(S, T, lambda u, v: -45.0 + 1.93 * u + 0.01 * v, lambda u, v: 3.0 + 1.4 * v)      # columns -45 .. 90: a third outside
        lat = pj.lattice_from(fn, T, S, tol=1e9, step=4)
        lat.sx[3:6, 11:14] = np.nan
        lat.sy[8, 2] = np.inf
        return T, lat
    raise KeyError(name)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@functools.lru_cache(maxsize=None)
def _want(dtype, name, method, window=None):
    T, lat = _case(name)
    return np.stack([wr.warp(z, NODATA, _geom(), T, lat, method, window) for z in _host(dtype)])


def _got(dtype, name, method, **kw):
    import torch
    from machisplin_amd import project as pj
    T, lat = _case(name)
    kw.setdefault("out_dtype", torch.float64)
    return pj.warp(_stack(dtype), T, lat, method, **kw).planes.cpu().numpy()


@pytest.mark.parametrize("name", LATTICES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_method_equals_the_restatement_bit_for_bit(hip, dtype, name):
    import torch
    for method in METHODS:
        want = _want(dtype, name, method)
        got = _got(dtype, name, method)
        assert got.dtype == np.float64 and _same(got, want), method
        got32 = _got(dtype, name, method, out_dtype=torch.float32)                 # MHS_F32: the float64 result rounded once
        assert got32.dtype == np.float32 and _same(got32, want.astype(np.float32)), method
    near = _want(dtype, name, "near")
    assert (~np.isnan(near)).mean() > 0.4
    T, lat = _case(name)
    sx, sy = wr.source_points(lat, np.arange(T.nrow), np.arange(T.ncol))
    S = _geom()
    if name == "holes":
        outside = (sx < S.xmin) | (sx > S.xmax)
        assert 0.3 < outside.mean() < 0.4 and np.isnan(near[:, outside]).all()
        hole = np.isnan(sx)
        assert hole[8:24, 40:56].all() and hole[28:36, 4:12].all() and hole.sum() == 16 * 16 + 8 * 8     # the lattice cells that read a bad node
        assert np.isnan(near[:, hole]).all() and (~np.isnan(near[:, ~hole & ~outside])).mean() > 0.9
    elif name == "utm":
        assert np.isnan(near).any()                                # the target reaches beyond the source
    elif name.startswith("bend-"):
        assert {"bend-1": (34, 131), "bend-4": (10, 34), "bend-64": (2, 4), "bend-256": (2, 2)}[name] == lat.sx.shape
    # cubic is not bilinear here, and the fallback is taken somewhere
    cub, bil = _want(dtype, name, "cubic"), _want(dtype, name, "bilinear")
    both = ~np.isnan(cub) & ~np.isnan(bil)
    assert 0.0 < (cub[both] == bil[both]).mean() < 0.5


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_warped_cell_is_extract_at_the_lattice_point(hip, dtype):
    """the new kernel against the existing one: mhs_extract_points at the restated (sx, sy)"""
    from machisplin_amd import resample
    T, lat = _case("utm")
    sx, sy = wr.source_points(lat, np.arange(T.nrow), np.arange(T.ncol))
    xy = np.column_stack([sx.ravel(), sy.ravel()])
    for method in METHODS:
        pts = resample.extract(_stack(dtype), xy, method)                          # (n, C)
        assert _same(_got(dtype, "utm", method), np.ascontiguousarray(pts.T).reshape(3, T.nrow, T.ncol)), method


@pytest.mark.parametrize("dtype", DTYPES)
def test_window_padded_out_and_repeat(hip, dtype):
    import torch
    from machisplin_amd import project as pj
    T, lat = _case("utm")
    r0, r1, c0, c1 = WINDOW
    for method in METHODS:
        whole = _want(dtype, "utm", method)
        assert _same(_want(dtype, "utm", method, WINDOW), whole[:, r0:r1, c0:c1])
        res = pj.warp(_stack(dtype), T, lat, method, out_dtype=torch.float64, window=WINDOW)
        assert res.geom == T.window(*WINDOW) and _same(res.planes.cpu().numpy(), whole[:, r0:r1, c0:c1]), method
        big = torch.full((3, r1 - r0 + 2, c1 - c0 + 9), -5.0, dtype=torch.float64, device=res.planes.device)
        out = big[:, 1:-1, 4:4 + c1 - c0]                                          # a padded row stride, an offset origin
        res2 = pj.warp(_stack(dtype), T, lat, method, window=WINDOW, out=out)
        assert res2.planes.data_ptr() == out.data_ptr() and _same(out.cpu().numpy(), whole[:, r0:r1, c0:c1]), method
        host = big.cpu().numpy()
        assert (host[:, 0] == -5.0).all() and (host[:, -1] == -5.0).all() and (host[:, :, :4] == -5.0).all() and (host[:, :, 4 + c1 - c0:] == -5.0).all()
        assert _same(_got(dtype, "utm", method), whole) and _same(_got(dtype, "utm", method), whole), method      # a second call, the same bits


BIG = (700, 900)


@pytest.mark.parametrize("ratio,dtype", [(20.0, "f32"), (20.0, "i16"), (2.1, "f64"), (2.1, "f32")])
def test_rectangles_that_do_not_fit_read_global_memory(hip, ratio, dtype):
    """A target cell of 20 source cells: a tile's rectangle is 640 x 1 280 cells, no tile fits the staging array.  Of 2.1: a whole
    tile's rectangle is about 71 x 138 = 9 800 cells -- float64 holds 6 144, so whole tiles read global memory while the partial
    tiles of the last tile column (16 cells wide) and row fit and are staged; float32 (12 288) stages them all."""
    import torch
    from machisplin_amd import Geometry, project as pj
    S = Geometry(5.0, 46.0, 1.0 / 1200.0, 1.0 / 1200.0, *BIG)
    nr, nc = (35, 45) if ratio == 20.0 else (300, 400)
    T = Geometry(0.0, float(nr), 1.0, 1.0, nr, nc)
    fn = _cells_map(S, T, lambda u, v: 3.0 + ratio * u + 0.02 * v, lambda u, v: 2.0 + ratio * v * 1.05 + 0.01 * u)
    lat = pj.lattice_from(fn, T, S, tol=1e9, step=16)
    if ratio == 2.1:
        assert nc % 64 == 16 and (31 * ratio * 1.05 + 4) * (63 * ratio + 4) > 6144 > (31 * ratio * 1.05 + 4) * (15 * ratio + 4)
    stack = _stack(dtype, S, BIG)
    layers = _host(dtype, BIG)
    for method in METHODS:
        got = pj.warp(stack, T, lat, method, out_dtype=torch.float64).planes.cpu().numpy()
        want = np.stack([wr.warp(z, NODATA, S, T, lat, method) for z in layers])
        assert _same(got, want), method
        assert 0.8 < (~np.isnan(want)).mean() < 1.0


@pytest.mark.parametrize("step", [1, 16])
def test_identity_lattice_is_resample(hip, step):
    """On grids whose origins and cell sizes are whole metres the lattice formula gives the cell centres exactly (K is a power of
    two, the nodes are small integers: every product and sum is exact), so a warp IS a resample, bit for bit."""
    import torch
    from machisplin_amd import Geometry, project as pj, resample
    S = Geometry(1000.0, 5000.0, 30.0, 28.0, *SHAPE)
    for T in (S, Geometry(1007.0, 4989.0, 45.0, 45.0, 40, 50), Geometry(700.0, 5300.0, 20.0, 21.0, 120, 170)):
        lat = pj.lattice_from(lambda X, Y: (X, Y), T, S, step=step)
        assert lat.step == step and lat.max_error == 0.0
        sx, sy = wr.source_points(lat, np.arange(T.nrow), np.arange(T.ncol))
        assert np.array_equal(sx[0], rr.cell_x(T, np.arange(T.ncol))) and np.array_equal(sy[:, 0], rr.cell_y(T, np.arange(T.nrow)))
        for dtype in DTYPES:
            stack = _stack(dtype, S)
            for method in METHODS:
                a = pj.warp(stack, T, lat, method, out_dtype=torch.float64).planes.cpu().numpy()
                b = resample.resample(stack, T, method, out_dtype=torch.float64).planes.cpu().numpy()
                assert _same(a, b), (dtype, method)
                if T is S:
                    assert _same(a, rr.to_double(_host(dtype), NODATA)), (dtype, method)


def test_project_end_to_end_on_a_linear_field(hip):
    """p lon + q lat on 200 x 200 cells of 1 / 1200 degree, projected to UTM at 30 m with bilinear.  Bilinear interpolation is
    exact for a linear field, so away from the border |value - (p lon* + q lat*)| <= (|p| xres + |q| yres) (max_error + 1e-6):
    the lattice contract plus rounding, (lon*, lat*) the exact inverse of the cell centre.  "Away from the border": a cell
    within half a source cell (46 m: 1.5 target cells) of the source's edge has taps outside the source, whose weights
    renormalise -- no longer the linear field.  So the cells left out are the restatement's NA cells and a ring of 2 cells
    around them, the target's outer ring of 2 included; the restatement alone decides which, and it keeps over 90 %."""
    import machisplin_amd as hip_
    from machisplin_amd import Geometry, project as pj
    p, q = 3.0, -2.0
    S = Geometry(3.9, 45.1, 1.0 / 1200.0, 1.0 / 1200.0, 200, 200)
    lon, lat_ = np.meshgrid(rr.cell_x(S, np.arange(200)), rr.cell_y(S, np.arange(200)))
    z = (p * lon + q * lat_)[None]
    crs = pj.utm(31)
    out, lattice = pj.project(hip_.RasterStack(S, z), pj.LONLAT, crs, res=30.0, method="bilinear")
    T = out.geom
    assert T.xres == T.yres == 30.0 and lattice.max_error <= 0.01 and out.planes.dtype.is_floating_point and out.planes.element_size() == 8
    got = out.planes.cpu().numpy()[0]
    want = wr.warp(z[0], float("nan"), S, T, lattice, "bilinear")
    assert _same(got, want)
    na = np.pad(np.isnan(want), 2, constant_values=True)
    near_na = np.zeros_like(na)
    for dr in range(-2, 3):
        for dc in range(-2, 3):
            near_na |= np.roll(np.roll(na, dr, axis=0), dc, axis=1)
    keep = ~near_na[2:-2, 2:-2]
    assert keep.mean() >= 0.9
    Y, X = np.meshgrid(rr.cell_y(T, np.arange(T.nrow)), rr.cell_x(T, np.arange(T.ncol)), indexing="ij")
    lon_s, lat_s = pj.transform(crs, pj.LONLAT, X, Y)
    err = np.abs(got - (p * lon_s + q * lat_s))[keep]
    bound = (abs(p) * S.xres + abs(q) * S.yres) * (lattice.max_error + 1e-6)
    print(f"step {lattice.step}, lattice error {lattice.max_error:.3g} cells, kept {keep.mean():.3f}, worst {err.max():.3g} of {bound:.3g}")
    assert err.max() <= bound
    # the stations go the same way
    pts = pj.transform_points(np.column_stack([lon[::50, ::50].ravel(), lat_[::50, ::50].ravel()]), pj.LONLAT, crs)
    assert (T.col_from_x(pts[:, 0]) >= 0).all() and (T.row_from_y(pts[:, 1]) >= 0).all()


def test_an_edited_lattice_goes_up_again(hip):
    import copy
    import torch
    from machisplin_amd import project as pj
    T, lat0 = _case("bend-4")
    lat = copy.deepcopy(lat0)
    first = pj.warp(_stack("f32"), T, lat, "bilinear", out_dtype=torch.float64).planes.cpu().numpy()
    assert _same(first, _want("f32", "bend-4", "bilinear"))
    lat.sx[2:4, 5:8] = np.nan                                      # after the first call: the cached device copy is stale
    second = pj.warp(_stack("f32"), T, lat, "bilinear", out_dtype=torch.float64).planes.cpu().numpy()
    want = np.stack([wr.warp(z, NODATA, _geom(), T, lat, "bilinear") for z in _host("f32")])
    assert _same(second, want) and np.isnan(second[:, 4:16, 16:32]).all() and not _same(first, second)


def test_python_refuses_what_the_library_would(hip):
    from machisplin_amd import _lib, project as pj
    T, lat = _case("bend-4")
    with pytest.raises(ValueError, match="aggregate method 'mean'"):
        pj.warp(_stack("f32"), T, lat, "mean")
    other = _case("utm")[0]                                        # a lattice made for another grid: its node counts differ
    with pytest.raises(_lib.MhsError, match="node counts"):
        pj.warp(_stack("f32"), other, lat, "near")
    with pytest.raises(_lib.MhsError, match="window outside"):
        pj.warp(_stack("f32"), T, lat, "near", window=(0, 34, 0, 130))
