"""GPU: topographic covariates from a DEM (csrc/terrain.hip, machisplin_amd/terrain.py) against the numpy restatement of the
rules (tests/terrain_ref.py).  Everything that does not go through atan / atan2 must equal the restatement bit for bit (NaN
where it is NaN): the library is built without contraction and the header fixes the order of the operations.

Planes: 37 x 83 and 70 x 131 cells (no multiple of the kernels' 32 x 64 tile: several workgroups, partly filled tiles) and
33 x 65 (the tile + 1 in both directions); seeded noise on a trend, a level patch, about 2 % of the cells NA in clusters (the
nodata -32768 everywhere, NaN too in float planes); int16, float32 and float64; a constant cell width and one that varies by
30 % over the rows; z_factor 0.3048.

slope_deg and aspect_deg differ from numpy only through atan and atan2 on bit-identical arguments.  No OCML accuracy
table comes with the ROCm installation, so the bound is measured: the largest difference on these planes was 1.421e-14
degrees (slope_deg) and 5.684e-14 degrees (aspect_deg) -- one ulp of a value in [64, 128) and in [256, 512) -- on every plane, type
and width; the tolerance is 4 x that, absolute."""
import ctypes as C
import functools

import numpy as np
import pytest

import terrain_ref as tr

pytestmark = pytest.mark.gpu

NODATA = -32768.0
ZF = 0.3048
DX, DY = 30.0, 28.5
SHAPES = ((37, 83), (70, 131), (33, 65))
DTYPES = ("f64", "f32", "i16")
NP_DT = {"f64": np.float64, "f32": np.float32, "i16": np.int16}
WINDOW = (5, 29, 7, 60)
EXACT = ("dzdx", "dzdy", "slope_tan", "eastness", "northness", "tpi", "tri", "roughness")
# 4 x the largest difference measured against the restatement on these planes, in degrees (module docstring)
TOL_DEG = {"slope_deg": 4 * 1.421e-14, "aspect_deg": 4 * 5.684e-14}
PLANES = [(s, d) for s in SHAPES for d in DTYPES]
PLANE_IDS = [f"{s[0]}x{s[1]}-{d}" for s, d in PLANES]


def _rmax():
    from machisplin_amd import terrain
    return terrain.max_radius()


@functools.lru_cache(maxsize=None)
def _plane(shape, dtype):
    """the DEM as the plane type holds it (numpy), built once"""
    nr, nc = shape
    rng = np.random.default_rng(1000 * nr + nc + {"f64": 0, "f32": 1, "i16": 2}[dtype])
    r, c = np.meshgrid(np.arange(nr, dtype=np.float64), np.arange(nc, dtype=np.float64), indexing="ij")
    z = 800.0 + 6.0 * r - 3.5 * c + 40.0 * np.sin(r / 7.0) * np.cos(c / 9.0) + 25.0 * rng.standard_normal(shape)
    z[nr // 2:nr // 2 + 9, nc // 2:nc // 2 + 11] = 1234.0                  # a level patch: exact ties, flat cells
    z = np.rint(z).astype(np.int16) if dtype == "i16" else z.astype(NP_DT[dtype])
    n_clusters = max(2, int(0.02 * nr * nc / 6))                           # about 2 % of the cells, in clusters of ~6
    for k in range(n_clusters):
        r0, c0 = rng.integers(0, nr), rng.integers(0, nc)
        h, w = rng.integers(1, 4), rng.integers(1, 5)
        z[r0:r0 + h, c0:c0 + w] = np.nan if (dtype != "i16" and k % 2) else NP_DT[dtype](NODATA)
    z[nr // 2 + 3:nr // 2 + 6, nc // 2 + 3:nc // 2 + 7] = NP_DT[dtype](1234)   # keep the middle of the patch
    return z


def _units(shape, varying):
    """constant dx, or a dx_row that varies by 30 % over the rows"""
    if not varying:
        return dict(dx=DX, dy=DY), dict(dx=DX, dy=DY, dx_row=None)
    rows = DX * (1.0 - 0.3 * np.arange(shape[0]) / (shape[0] - 1))
    return dict(dx_row=rows, dy=DY), dict(dx=np.nan, dy=DY, dx_row=rows)


@functools.lru_cache(maxsize=None)
def _stack(shape, dtype):
    import machisplin_amd as hip
    from machisplin_amd import synth
    return hip.RasterStack(synth.grid(*shape), _plane(shape, dtype)[None], NODATA)


@functools.lru_cache(maxsize=None)
def _want_terrain(shape, dtype, varying):
    return tr.terrain(_plane(shape, dtype), NODATA, z_factor=ZF, **_units(shape, varying)[1])


@functools.lru_cache(maxsize=None)
def _got_terrain(shape, dtype, varying):
    from machisplin_amd import terrain
    got = terrain.terrain(_stack(shape, dtype), v=tr.VARS, z_factor=ZF, **_units(shape, varying)[0])
    return dict(zip(tr.VARS, got.cpu().numpy()))


@functools.lru_cache(maxsize=None)
def _want_relief(shape, dtype, radius):
    return tr.relief(_plane(shape, dtype), NODATA, radius, ZF)


@functools.lru_cache(maxsize=None)
def _want_geo(shape, dtype, varying, search, flat_deg):
    return tr.geomorphon(_plane(shape, dtype), NODATA, search, flat_deg, z_factor=ZF, **_units(shape, varying)[1])


def _same(a, b):
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("varying", [False, True], ids=["dx", "dx_row"])
@pytest.mark.parametrize("shape,dtype", PLANES, ids=PLANE_IDS)
def test_terrain_planes_equal_the_restatement(hip, shape, dtype, varying):
    want, got = _want_terrain(shape, dtype, varying), _got_terrain(shape, dtype, varying)
    na = np.isnan(want["dzdx"])
    assert na[0].all() and na[-1].all() and na[:, 0].all() and na[:, -1].all() and 0.03 < na[1:-1, 1:-1].mean() < 0.6
    flat = want["slope_tan"] == 0.0
    assert flat.any()                                            # the level patch
    for k in tr.VARS:
        assert got[k].dtype == np.float64 and np.array_equal(np.isnan(got[k]), na), k          # the NA mask of every output
    for k in EXACT:
        assert _same(got[k], want[k]), k
    for k, tol in TOL_DEG.items():
        diff = np.abs(got[k] - want[k])[~na]
        print(f"{k} {shape} {dtype} dx_row={varying}: largest difference {diff.max():.3e} degrees (tolerance {tol:.3e})")
        assert diff.max() <= tol, k
    assert (got["aspect_deg"][flat] == -1.0).all() and (got["eastness"][flat] == 0.0).all() and (got["northness"][flat] == 0.0).all()
    assert (got["slope_deg"][flat] == 0.0).all()
    ok = ~na & ~flat
    assert (got["aspect_deg"][ok] >= 0.0).all() and (got["aspect_deg"][ok] <= 360.0).all()


@pytest.mark.parametrize("shape,dtype", PLANES, ids=PLANE_IDS)
def test_relief_planes_equal_the_restatement_bit_for_bit(hip, shape, dtype):
    from machisplin_amd import terrain
    stack = _stack(shape, dtype)
    assert _rmax() >= 32 and _rmax() > 37
    for radius in (1, 2, 17, _rmax()):                           # the largest radius exceeds the 37-row raster
        want = _want_relief(shape, dtype, radius)
        got = terrain.relief(stack, radius, tr.STATS, z_factor=ZF).cpu().numpy()
        for k, s in enumerate(tr.STATS):
            assert np.array_equal(np.isnan(got[k]), np.isnan(tr.to_double(_plane(shape, dtype), NODATA))), (radius, s)
            assert _same(got[k], want[s]), (radius, s)


@pytest.mark.parametrize("varying", [False, True], ids=["dx", "dx_row"])
@pytest.mark.parametrize("shape,dtype", PLANES, ids=PLANE_IDS)
def test_geomorphon_forms_equal_the_restatement(hip, shape, dtype, varying):
    from machisplin_amd import terrain
    stack = _stack(shape, dtype)
    for search in (1, 5, _rmax()):
        want, margin = _want_geo(shape, dtype, varying, search, 1.0)
        assert margin > 1e-9, (search, margin)                   # no decision sits within an atan rounding error of its threshold
        got = terrain.geomorphon(stack, search, 1.0, z_factor=ZF, **_units(shape, varying)[0]).cpu().numpy()
        assert _same(got, want), search
        valid = want[want != tr.GEOMORPHON_NA]
        assert valid.size > 0.3 * want.size and valid.min() >= 1 and valid.max() <= 10 and len(np.unique(valid)) >= 6
        assert (want[0] == tr.GEOMORPHON_NA).all() and (want[:, -1] == tr.GEOMORPHON_NA).all()


@pytest.mark.parametrize("shape,dtype", [p for p in PLANES if p[1] != "i16"], ids=[i for i in PLANE_IDS if "i16" not in i])
def test_geomorphon_flat_deg_zero_ties_are_flat(hip, shape, dtype):
    """flat_deg = 0: on the level patch D == 0 exactly in all eight directions and the cell must be FL; everywhere else no
    D is within 1e-9 of 0 (float noise; an int16 plane has exact opposite tangents by the thousand and is left out)."""
    from machisplin_amd import terrain
    for search in (1, 5):
        want, margin = _want_geo(shape, dtype, False, search, 0.0)
        assert margin > 1e-9, (search, margin)
        nr, nc = shape
        assert want[nr // 2 + 4, nc // 2 + 4] == tr.FL if search == 1 else True
        got = terrain.geomorphon(_stack(shape, dtype), search, 0.0, z_factor=ZF, dx=DX, dy=DY).cpu().numpy()
        assert _same(got, want), search


def _one_plane(shape, dtype="f64", seed=3):
    import machisplin_amd as hip
    from machisplin_amd import synth
    z = (np.random.default_rng(seed).standard_normal(shape) * 50.0 + 300.0).astype(NP_DT[dtype])
    return z, hip.RasterStack(synth.grid(*shape), z[None], NODATA)


@pytest.mark.parametrize("shape", [(1, 70), (70, 1), (2, 2), (3, 3)], ids=["1xN", "Nx1", "2x2", "3x3"])
def test_degenerate_shapes(hip, shape):
    from machisplin_amd import terrain
    z, stack = _one_plane(shape)
    got = terrain.terrain(stack, v=tr.VARS, dx=DX, dy=DY).cpu().numpy()
    want = tr.terrain(z, NODATA, DX, DY)
    n_valid = 1 if shape == (3, 3) else 0                         # 3 x 3: one valid terrain cell; thinner: none
    for k, name in enumerate(tr.VARS):
        assert (~np.isnan(got[k])).sum() == n_valid, name
        if name in EXACT:
            assert _same(got[k], want[name]), name
    forms = terrain.geomorphon(stack, 3, 1.0, dx=DX, dy=DY).cpu().numpy()
    assert _same(forms, tr.geomorphon(z, NODATA, 3, 1.0, DX, DY)[0]) and (forms != tr.GEOMORPHON_NA).sum() == n_valid
    for radius in (1, 4):
        rel = terrain.relief(stack, radius, tr.STATS).cpu().numpy()
        want_r = tr.relief(z, NODATA, radius)
        assert not np.isnan(rel).any()                            # relief is valid wherever the centre is
        for k, s in enumerate(tr.STATS):
            assert _same(rel[k], want_r[s]), (radius, s)


@pytest.mark.parametrize("dtype", DTYPES)
def test_window_with_padding_equals_the_whole_grid_slice(hip, dtype):
    import torch
    from machisplin_amd import terrain
    shape = SHAPES[0]
    stack = _stack(shape, dtype)
    r0, r1, c0, c1 = WINDOW
    nr, nc = r1 - r0, c1 - c0
    dev = stack.planes.device
    u = _units(shape, True)[0]
    whole = terrain.terrain(stack, v=tr.VARS, z_factor=ZF, **u)
    big = torch.full((len(tr.VARS), nr, 71), -7.0, dtype=torch.float64, device=dev)             # ld = 71 > 53 = the width
    win = terrain.terrain(stack, v=tr.VARS, z_factor=ZF, window=WINDOW, out=big[:, :, :nc], **u)
    assert win.stride(1) == 71 and torch.equal(win.nan_to_num(nan=-5.0), whole[:, r0:r1, c0:c1].nan_to_num(nan=-5.0))
    assert (big[:, :, nc:] == -7.0).all()                                                       # the padding keeps its sentinel
    for radius in (2, 17):
        whole = terrain.relief(stack, radius, tr.STATS, z_factor=ZF)
        big.fill_(-7.0)
        win = terrain.relief(stack, radius, tr.STATS, z_factor=ZF, window=WINDOW, out=big[:3, :, :nc])
        assert torch.equal(win.nan_to_num(nan=-5.0), whole[:, r0:r1, c0:c1].nan_to_num(nan=-5.0)) and (big[:3, :, nc:] == -7.0).all()
    for search in (1, 5, _rmax()):
        whole = terrain.geomorphon(stack, search, 1.0, z_factor=ZF, **u)
        bigi = torch.full((nr, 64), -7, dtype=torch.int16, device=dev)
        win = terrain.geomorphon(stack, search, 1.0, z_factor=ZF, window=WINDOW, out=bigi[:, :nc], **u)
        assert torch.equal(win, whole[r0:r1, c0:c1]) and (bigi[:, nc:] == -7).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_float32_output_subset_order_and_repeat(hip, dtype):
    import torch
    from machisplin_amd import terrain
    shape = SHAPES[1]
    stack = _stack(shape, dtype)
    got = _got_terrain(shape, dtype, False)
    # a float32 output is the float64 result rounded once
    got32 = terrain.terrain(stack, v=tr.VARS, z_factor=ZF, dx=DX, dy=DY, out_dtype=torch.float32).cpu().numpy()
    for k, name in enumerate(tr.VARS):
        assert _same(got32[k], got[name].astype(np.float32)), name
    rel = terrain.relief(stack, 17, tr.STATS, z_factor=ZF)
    rel32 = terrain.relief(stack, 17, tr.STATS, z_factor=ZF, out_dtype=torch.float32)
    assert _same(rel32.cpu().numpy(), rel.cpu().numpy().astype(np.float32))
    # any subset, in the caller's order, gives the same planes as the all-variables pass; a single name gives one plane
    pick = ("roughness", "slope_deg", "dzdx")
    sub = terrain.terrain(stack, v=pick, z_factor=ZF, dx=DX, dy=DY).cpu().numpy()
    assert sub.shape == (3,) + shape and all(_same(sub[k], got[name]) for k, name in enumerate(pick))
    assert _same(terrain.terrain(stack, v="aspect_deg", z_factor=ZF, dx=DX, dy=DY).cpu().numpy(), got["aspect_deg"])
    assert _same(terrain.relief(stack, 17, "minus_mean", z_factor=ZF).cpu().numpy(), rel[2].cpu().numpy())
    # a repeat call gives the same bits
    again = terrain.terrain(stack, v=tr.VARS, z_factor=ZF, dx=DX, dy=DY).cpu().numpy()
    assert all(_same(again[k], got[name]) for k, name in enumerate(tr.VARS))
    assert torch.equal(terrain.geomorphon(stack, 5, 1.0, dx=DX, dy=DY), terrain.geomorphon(stack, 5, 1.0, dx=DX, dy=DY))
    assert _same(terrain.relief(stack, 17, tr.STATS, z_factor=ZF).cpu().numpy(), rel.cpu().numpy())


def _host_calls(lib, shape, dtype, varying):
    """the three host entry points on the numpy plane, whole grid: (terrain planes, relief planes (R = 17), forms (L = 5))"""
    from machisplin_amd import _lib, synth
    z = np.ascontiguousarray(_plane(shape, dtype))
    nr, nc = shape
    g = synth.grid(*shape).c_struct()
    s = _lib.Stack(z.ctypes.data, 1, {"f64": _lib.F64, "f32": _lib.F32, "i16": _lib.I16}[dtype], nr * nc, nc, NODATA)
    rows = _units(shape, varying)[1]["dx_row"]
    rows = None if rows is None else np.ascontiguousarray(rows)
    u = _lib.TerrainUnits(DX, None if rows is None else rows.ctypes.data, DY, ZF)
    t = np.full((len(tr.VARS), nr, nc), -7.0)
    _lib.check(lib.mhs_terrain(C.byref(g), C.byref(s), 0, C.byref(u), 0, nr, 0, nc, (1 << len(tr.VARS)) - 1, t.ctypes.data, _lib.F64))
    r = np.full((3, nr, nc), -7.0, dtype=np.float32)
    _lib.check(lib.mhs_relief(C.byref(g), C.byref(s), 0, C.byref(u), 17, 0, nr, 0, nc, 7, r.ctypes.data, _lib.F32))
    f = np.full((nr, nc), -7, dtype=np.int16)
    _lib.check(lib.mhs_geomorphon(C.byref(g), C.byref(s), 0, C.byref(u), 5, 1.0, 0, nr, 0, nc, f.ctypes.data))
    return t, r, f


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_entries_equal_the_device_entries(hip, monkeypatch, dtype):
    import torch
    from machisplin_amd import _lib, terrain
    shape, varying = SHAPES[0], True
    stack = _stack(shape, dtype)
    u = _units(shape, varying)[0]
    want_t = terrain.terrain(stack, v=tr.VARS, z_factor=ZF, **u).cpu().numpy()
    want_r = terrain.relief(stack, 17, tr.STATS, z_factor=ZF, out_dtype=torch.float32).cpu().numpy()
    want_f = terrain.geomorphon(stack, 5, 1.0, z_factor=ZF, **u).cpu().numpy()
    for bands in (None, "5"):                  # 5 bands of 8 rows: every seam falls inside the 17-row halo of its neighbours
        if bands:
            monkeypatch.setenv("MHS_HOST_BANDS", bands)
        t, r, f = _host_calls(_lib.lib(), shape, dtype, varying)
        assert _same(t, want_t) and _same(r, want_r) and _same(f, want_f), bands


def test_covariates_feed_mess_and_mltps_predict(hip):
    import torch
    from machisplin_amd import mltps, synth, terrain
    g = synth.grid(70, 131)
    dem = hip.RasterStack(g, _plane((70, 131), "i16")[None], NODATA)
    spec = ("slope_deg", ("above_min", 17), "tpi", ("geomorphon", 5), ("minus_mean", 2), ("geomorphon", 3, 0.5))
    stack = hip.covariates(dem, spec, z_factor=ZF, lonlat=True)
    assert isinstance(stack, hip.RasterStack) and stack.planes.dtype == torch.float32 and stack.n_layers == 7 and np.isnan(stack.nodata)
    assert stack.names == ["dem", "slope_deg", "above_min17", "tpi", "geomorphon5", "minus_mean2", "geomorphon3"]
    planes = stack.planes.cpu().numpy()
    # its planes equal those of the single calls
    assert _same(planes[0], tr.to_double(_plane((70, 131), "i16"), NODATA).astype(np.float32))
    t = terrain.terrain(dem, v=("slope_deg", "tpi"), lonlat=True, z_factor=ZF, out_dtype=torch.float32).cpu().numpy()
    assert _same(planes[1], t[0]) and _same(planes[3], t[1])
    assert _same(planes[2], terrain.relief(dem, 17, "above_min", z_factor=ZF, out_dtype=torch.float32).cpu().numpy())
    assert _same(planes[5], terrain.relief(dem, 2, "minus_mean", z_factor=ZF, out_dtype=torch.float32).cpu().numpy())
    for k, (search, flat) in ((4, (5, 1.0)), (6, (3, 0.5))):
        f = terrain.geomorphon(dem, search, flat, lonlat=True, z_factor=ZF).cpu().numpy()
        assert _same(planes[k], np.where(f == tr.GEOMORPHON_NA, np.nan, f).astype(np.float32))
    # lonlat: the wrapper's own widths, cos taken by numpy
    lat = g.y_from_row(np.arange(g.nrow))
    rows = g.xres * (np.pi / 180.0) * 6378137.0 * np.cos(lat * (np.pi / 180.0))
    want = tr.terrain(_plane((70, 131), "i16"), NODATA, np.nan, g.yres * (np.pi / 180.0) * 6378137.0, ZF, dx_row=rows)
    assert _same(planes[3], want["tpi"].astype(np.float32))
    assert _same(terrain.terrain(dem, v="dzdx", lonlat=True, z_factor=ZF).cpu().numpy(), want["dzdx"])
    # ... and go straight into Mess and mltps_predict
    xy, rows_s, cols_s, uv = synth.stations(g, 200, 23)
    X, _, _ = mltps.station_predictors(stack, xy)
    keep = ~np.isnan(X).any(axis=1)
    assert X.shape[1] == 9 and 60 < keep.sum() < 200                 # the outer ring and the NA clusters drop some stations
    mess = hip.Mess(X[keep][:, :7]).grid(stack).cpu().numpy()
    assert np.array_equal(np.isnan(mess), np.isnan(planes).any(axis=0)) and (mess[~np.isnan(mess)] <= 100.0).all()
    resp = synth.response(np.nan_to_num(X), uv, 23)
    models = [hip.models.from_param_dict(p) for p in synth.ensemble_params(X[keep], resp[keep], 23, which="g")]
    res = hip.mltps_predict(stack, xy, resp, models, [1.0], 1.0, tile_edge=None, mess=True)
    final = res["final"].cpu().numpy()
    assert final.shape == (70, 131) and np.isfinite(final[~np.isnan(planes).any(axis=0)]).all() and res["n_stations"] == keep.sum()
    assert _same(res["mess"].cpu().numpy(), mess)
