"""GPU: solar covariates from a DEM (solar_kernel of csrc/terrain.hip, machisplin_amd.terrain.solar) against the numpy
restatement of the rules (tests/solar_ref.py).  No trigonometry runs on the device, so EVERY product must equal the
restatement bit for bit (NaN where it is NaN).

Planes: those of test_terrain_gpu (37 x 83, 70 x 131, 33 x 65: ragged tiles, several workgroups, the tile + 1; noise on a
trend, a level patch, NA clusters as nodata and NaN; int16, float32, float64) with an NA strip one cell wide added, which the
rays must step over.  Two sun tables with tab_row switching at row 20 -- inside a tile and inside a wave's eight rows: table 0
is sun_tables at latitude 45 (its northern sectors are empty), table 1 holds entries in ONE sector only."""
import ctypes as C
import functools

import numpy as np
import pytest

import solar_ref as sr
import terrain_ref as tr
from test_terrain_gpu import DTYPES, DX, DY, NODATA, NP_DT, PLANE_IDS, PLANES, SHAPES, WINDOW, ZF, _same, _units
from test_terrain_gpu import _plane as _terrain_plane

pytestmark = pytest.mark.gpu

SWITCH = 20


def _rmax():
    from machisplin_amd import terrain
    return terrain.max_radius()


@functools.lru_cache(maxsize=None)
def _plane(shape, dtype):
    z = _terrain_plane(shape, dtype).copy()
    z[3:shape[0] - 2, 11] = NP_DT[dtype](NODATA)                     # an NA strip
    return z


@functools.lru_cache(maxsize=None)
def _stack(shape, dtype):
    import machisplin_amd as hip
    from machisplin_amd import synth
    return hip.RasterStack(synth.grid(*shape), _plane(shape, dtype)[None], NODATA)


@functools.lru_cache(maxsize=None)
def _tables(nrow):
    """table 0: latitude 45, four days, hourly; table 1: the winter entries of latitude 60 that fall into sector 7 (SSE .. S)"""
    from machisplin_amd import synth, terrain
    g = synth.grid(nrow, 8)
    a = terrain.sun_tables(g, lat=45.0, dx=DX, dy=DY, step_minutes=60)
    b = terrain.sun_tables(g, lat=60.0, dx=DX, dy=DY, days=(355, 20), step_minutes=10)
    only = b.entries[b.start[7]:b.start[8]]
    assert len(only) >= 4 and (np.diff(a.start) == 0).any()          # a sector with no entries in table 0
    start_b = a.start[-1] + np.where(np.arange(1, 17) >= 8, len(only), 0)
    tab_row = (np.arange(nrow) >= SWITCH).astype(np.int32) if nrow > SWITCH else None
    return terrain.SunTables(np.concatenate([a.start, start_b]), np.concatenate([a.entries, only]), np.concatenate([a.omega, b.omega]), tab_row)


@functools.lru_cache(maxsize=None)
def _want(shape, dtype, varying, search):
    return sr.solar(_plane(shape, dtype), NODATA, search, _tables(shape[0]), z_factor=ZF, **_units(shape, varying)[1])


def _got(shape, dtype, varying, search, products=sr.SOLAR, **kw):
    from machisplin_amd import terrain
    return terrain.solar(_stack(shape, dtype), search, products, _tables(shape[0]), z_factor=ZF, **_units(shape, varying)[0], **kw)


@pytest.mark.parametrize("varying", [False, True], ids=["dx", "dx_row"])
@pytest.mark.parametrize("shape,dtype", PLANES, ids=PLANE_IDS)
def test_every_product_equals_the_restatement_bit_for_bit(hip, shape, dtype, varying):
    import torch
    na = np.isnan(tr.to_double(_plane(shape, dtype), NODATA))
    assert 0.01 < na.mean() < 0.2 and na[3:shape[0] - 2, 11].all()
    for search in (1, 7, _rmax()):                                   # 7: the knight rays take 3 steps
        want = _want(shape, dtype, varying, search)
        counts = want["counts"]
        print(f"{shape} {dtype} dx_row={varying} L={search}: {counts}")
        # the case has shadowed and lit (cell, entry) pairs and cells facing away from the sun: every branch is taken
        assert counts["lit"] > 100 and counts["shadow"] > 100 and counts["c_neg"] > 0, (search, counts)
        assert (want["horizon"][:, ~na] > 0).any() and (want["horizon"][:, ~na] == 0).any()
        got = _got(shape, dtype, varying, search).cpu().numpy()
        assert got.dtype == np.float64 and got.shape == (19,) + shape
        assert _same(got, sr.planes(want, sr.SOLAR)), [k for k in range(19) if not _same(got[k], sr.planes(want, sr.SOLAR)[k])]
        for k in (0, 2) + tuple(range(3, 19)):                       # only an NA centre makes a cell NA ...
            assert np.array_equal(np.isnan(got[k]), na), k
        assert np.array_equal(np.isnan(got[1]), np.isnan(tr.terrain(_plane(shape, dtype), NODATA, DX, DY)["dzdx"]))      # ... but in direct
        got32 = _got(shape, dtype, varying, search, out_dtype=torch.float32).cpu().numpy()
        assert _same(got32, got.astype(np.float32))                  # float32 is the float64 result rounded once


def _one_plane(shape, seed=3):
    import machisplin_amd as hip
    from machisplin_amd import synth
    z = np.random.default_rng(seed).standard_normal(shape) * 50.0 + 300.0
    return z, hip.RasterStack(synth.grid(*shape), z[None], NODATA)


@pytest.mark.parametrize("shape", [(1, 70), (70, 1), (2, 2), (3, 3)], ids=["1xN", "Nx1", "2x2", "3x3"])
def test_degenerate_shapes(hip, shape):
    from machisplin_amd import terrain
    z, stack = _one_plane(shape)
    tables = _tables(shape[0])
    for search in (1, 3, _rmax()):
        got = terrain.solar(stack, search, sr.SOLAR, tables, dx=DX, dy=DY).cpu().numpy()
        want = sr.solar(z, NODATA, search, tables, DX, DY)
        assert _same(got, sr.planes(want, sr.SOLAR)), search
        assert not np.isnan(got[0]).any() and not np.isnan(got[2:]).any()          # svf, sun_hours, horizon: every centre is valid
        assert (~np.isnan(got[1])).sum() == (1 if shape == (3, 3) else 0)           # direct needs the whole 3 x 3


@pytest.mark.parametrize("dtype", DTYPES)
def test_window_subset_order_repeat(hip, dtype):
    import torch
    from machisplin_amd import terrain
    shape = SHAPES[0]
    stack = _stack(shape, dtype)
    r0, r1, c0, c1 = WINDOW
    nr, nc = r1 - r0, c1 - c0
    for search in (7, _rmax()):
        whole = _got(shape, dtype, True, search)
        big = torch.full((19, nr, 71), -7.0, dtype=torch.float64, device=stack.planes.device)           # ld = 71 > 53 = the width
        win = _got(shape, dtype, True, search, window=WINDOW, out=big[:, :, :nc])
        assert win.stride(1) == 71 and torch.equal(win.nan_to_num(nan=-5.0), whole[:, r0:r1, c0:c1].nan_to_num(nan=-5.0))
        assert (big[:, :, nc:] == -7.0).all()                        # the padding keeps its sentinel
        w = whole.cpu().numpy()
        # a subset in the caller's order; single names; a repeat call
        sub = _got(shape, dtype, True, search, products=("sun_hours", "svf")).cpu().numpy()
        assert sub.shape == (2,) + shape and _same(sub[0], w[2]) and _same(sub[1], w[0])
        sub = _got(shape, dtype, True, search, products=("horizon", "direct")).cpu().numpy()
        assert sub.shape == (17,) + shape and _same(sub[:16], w[3:]) and _same(sub[16], w[1])
        assert _same(_got(shape, dtype, True, search, products="direct").cpu().numpy(), w[1])
        assert _same(_got(shape, dtype, True, search, products="svf").cpu().numpy(), w[0])
        hor = terrain.solar(stack, search, "horizon", None, z_factor=ZF, **_units(shape, True)[0]).cpu().numpy()        # needs no tables
        assert hor.shape == (16,) + shape and _same(hor, w[3:])
        assert _same(_got(shape, dtype, True, search).cpu().numpy(), w)


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_entry_equals_the_device_entry(hip, monkeypatch, dtype):
    from machisplin_amd import _lib, synth
    shape = SHAPES[1]
    nr, nc = shape
    want = _got(shape, dtype, True, 7).cpu().numpy()
    z = np.ascontiguousarray(_plane(shape, dtype))
    g = synth.grid(*shape).c_struct()
    s = _lib.Stack(z.ctypes.data, 1, {"f64": _lib.F64, "f32": _lib.F32, "i16": _lib.I16}[dtype], nr * nc, nc, NODATA)
    rows = np.ascontiguousarray(_units(shape, True)[1]["dx_row"])
    u = _lib.TerrainUnits(DX, rows.ctypes.data, DY, ZF)
    t = _tables(nr).c_struct()
    for bands in (None, "3"):                    # 3 bands of 24 rows: the seams fall inside the halo rows of their neighbours
        if bands:
            monkeypatch.setenv("MHS_HOST_BANDS", bands)
        out = np.full((19, nr, nc), -7.0)
        _lib.check(_lib.lib().mhs_solar(C.byref(g), C.byref(s), 0, C.byref(u), 7, C.byref(t), 0, nr, 0, nc, 15, out.ctypes.data, _lib.F64))
        assert _same(out, want), bands
    r0, r1, c0, c1 = 9, 61, 3, 100
    out = np.full((2, r1 - r0, c1 - c0), -7.0, dtype=np.float32)
    _lib.check(_lib.lib().mhs_solar(C.byref(g), C.byref(s), 0, C.byref(u), 7, C.byref(t), r0, r1, c0, c1, 6, out.ctypes.data, _lib.F32))
    assert _same(out, want[1:3, r0:r1, c0:c1].astype(np.float32))


def test_a_ridge_and_a_pit(hip):
    """physics, without the restatement: an east-west ridge at latitude 45 on day 355 -- the south face gets more direct light
    and more sun hours than the north face; a cell in a pit sees less sky than the plain"""
    import machisplin_amd as hip_
    from machisplin_amd import synth, terrain
    g = synth.grid(41, 31)
    r, c = np.meshgrid(np.arange(41.0), np.arange(31.0), indexing="ij")
    ridge = hip_.RasterStack(g, (300.0 - 15.0 * np.abs(r - 20.0))[None], float("nan"))
    tables = terrain.sun_tables(g, days=(355,), lat=45.0, dx=30.0, dy=30.0)
    direct, hours = terrain.solar(ridge, 10, ("direct", "sun_hours"), tables, dx=30.0, dy=30.0).cpu().numpy()
    assert direct[30, 15] > direct[10, 15] >= 0.0 and hours[30, 15] > hours[10, 15] >= 0.0
    assert (direct[25:36, 5:26] > direct[5:16, 5:26].max()).all() and hours[30, 15] == tables.entries[:, 6].sum()
    pit = hip_.RasterStack(g, (10.0 * np.minimum(np.hypot(r - 20.0, c - 15.0) - 6.0, 0.0))[None], float("nan"))
    svf = terrain.solar(pit, 10, "svf", tables, dx=30.0, dy=30.0).cpu().numpy()
    assert 0.0 < svf[20, 15] < 0.95 * svf[3, 3] and abs(svf[3, 3] - 1.0) < 1e-14


def test_refusals_name_the_argument_and_the_library_works_afterwards(hip):
    from machisplin_amd import _lib, terrain
    shape, dtype = SHAPES[2], "f32"
    stack, good = _stack(shape, dtype), _tables(shape[0])
    want = terrain.solar(stack, 5, sr.SOLAR, good, dx=DX, dy=DY).cpu().numpy()

    def edited(**edit):
        t = terrain.SunTables(good.start.copy(), good.entries.copy(), good.omega.copy(), good.tab_row.copy())
        for k, (idx, v) in edit.items():
            getattr(t, k)[idx] = v
        return t

    many = terrain.SunTables(np.concatenate([[0], np.full(16, 262145)]), np.zeros((1, 8)), np.full(16, 1 / 16))
    cases = [("search must be in 1 .. %d" % _rmax(), dict(search=0)), ("search must be in 1 .. %d" % _rmax(), dict(search=_rmax() + 1)),
             ("entries[3].t", dict(tables=edited(entries=((3, 0), 1.5)))), ("entries[3].t", dict(tables=edited(entries=((3, 0), -0.5)))),
             ("entries[2].tan_h", dict(tables=edited(entries=((2, 1), 0.0)))), ("entries[2].tan_h", dict(tables=edited(entries=((2, 1), -1.0)))),
             ("entries[5].w", dict(tables=edited(entries=((5, 5), -1.0)))), ("start[4] decreases", dict(tables=edited(start=(3, 5000)))),
             ("tab_row[9]", dict(tables=edited(tab_row=(9, 2)))), ("MHS_SOLAR_MAX_ENTRIES", dict(tables=many))]
    for needle, kw in cases:
        with pytest.raises(_lib.MhsError) as err:
            terrain.solar(stack, kw.get("search", 5), sr.SOLAR, kw.get("tables", good), dx=DX, dy=DY)
        assert err.value.code == _lib.ERR_INVALID and needle in str(err.value) and "mhs_solar_dev" in str(err.value), (needle, str(err.value))
    # NULL tables with svf: the wrapper would make tables, so the library is asked directly
    g, s, u = stack.geom.c_struct(), stack.c_struct(), _lib.TerrainUnits(DX, None, DY, 1.0)
    out = stack.planes.new_empty((1,) + shape, dtype=__import__("torch").float64)
    rc = _lib.lib().mhs_solar_dev(C.byref(g), C.byref(s), 0, C.byref(u), 5, None, 0, shape[0], 0, shape[1], 1, out.data_ptr(), _lib.F64, shape[1],
                                  shape[0] * shape[1], None)
    assert rc == _lib.ERR_INVALID and "tables is NULL" in _lib.lib().mhs_last_error().decode()
    assert _same(terrain.solar(stack, 5, sr.SOLAR, good, dx=DX, dy=DY).cpu().numpy(), want)
    assert _same(want, sr.planes(sr.solar(_plane(shape, dtype), NODATA, 5, good, DX, DY), sr.SOLAR))


def test_covariates_carry_the_names_and_feed_mess_and_mltps_predict(hip):
    import torch
    from machisplin_amd import mltps, synth, terrain
    g = synth.grid(70, 131)
    dem = hip.RasterStack(g, _plane((70, 131), "i16")[None], NODATA)
    stack = hip.covariates(dem, ("slope_deg", ("svf", 7), ("direct", 7)), lat=45.0)
    assert isinstance(stack, hip.RasterStack) and stack.planes.dtype == torch.float32 and stack.n_layers == 4 and np.isnan(stack.nodata)
    assert stack.names == ["dem", "slope_deg", "svf7", "direct7"]
    planes = stack.planes.cpu().numpy()
    one = terrain.solar(dem, 7, ("svf", "direct"), lat=45.0, out_dtype=torch.float32).cpu().numpy()
    assert _same(planes[2], one[0]) and _same(planes[3], one[1])
    tables = terrain.sun_tables(g, lat=45.0)
    want = sr.solar(_plane((70, 131), "i16"), NODATA, 7, tables, g.xres, g.yres)
    assert _same(planes[2], want["svf"].astype(np.float32)) and _same(planes[3], want["direct"].astype(np.float32))
    # several search lengths and sun_hours, each length one call; the caller's tables
    more = hip.covariates(dem, (("sun_hours", 3), ("svf", 7), ("svf", 3)), sun=tables)
    assert more.names == ["dem", "sun_hours3", "svf7", "svf3"] and _same(more.planes[2].cpu().numpy(), planes[2])
    assert _same(more.planes[1].cpu().numpy(), sr.solar(_plane((70, 131), "i16"), NODATA, 3, tables, g.xres, g.yres)["sun_hours"].astype(np.float32))
    # ... and go straight into Mess and mltps_predict
    xy, rows_s, cols_s, uv = synth.stations(g, 200, 23)
    X, _, _ = mltps.station_predictors(stack, xy)
    keep = ~np.isnan(X).any(axis=1)
    assert X.shape[1] == 6 and 60 < keep.sum() < 200
    mess = hip.Mess(X[keep][:, :4]).grid(stack).cpu().numpy()
    assert np.array_equal(np.isnan(mess), np.isnan(planes).any(axis=0)) and (mess[~np.isnan(mess)] <= 100.0).all()
    resp = synth.response(np.nan_to_num(X), uv, 23)
    models = [hip.models.from_param_dict(p) for p in synth.ensemble_params(X[keep], resp[keep], 23, which="g")]
    res = hip.mltps_predict(stack, xy, resp, models, [1.0], 1.0, tile_edge=None, mess=True)
    final = res["final"].cpu().numpy()
    assert final.shape == (70, 131) and np.isfinite(final[~np.isnan(planes).any(axis=0)]).all() and res["n_stations"] == keep.sum()
    assert _same(res["mess"].cpu().numpy(), mess)
