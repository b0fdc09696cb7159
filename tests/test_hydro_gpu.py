"""GPU: the hydrology of a DEM (csrc/hydro.hip, machisplin_amd/terrain.py: hydro) against the restatement of the rules by
other algorithms (tests/hydro_ref.py: priority flood, breadth-first search, topological order).  The filled surface, the
direction and the accumulation must equal the restatement bit for bit: only min, max and sums of integers go into them, and the
monotone tile sweeps reach the same fixed point whatever the schedule.

Planes of integer-valued heights, so that int16 (nodata -32768), float32 and float64 hold the same plane and share one
restatement; shapes below, at and beyond the kernels' 32 x 64 tile, with ragged last tiles.

The TWI differs from numpy only through log on bit-identical arguments.  No OCML accuracy table comes with the ROCm
installation, so the bound is measured: the largest difference on these planes, types and widths was 3.553e-15 (the spiral,
whose channel gathers thousands of cells) -- one ulp of a value in [16, 32) -- and 1.776e-15 on every other plane; the
tolerance is 4 x the largest, absolute."""
import ctypes as C
import functools

import numpy as np
import pytest

import hydro_ref as hr

pytestmark = pytest.mark.gpu

DX, DY, ZF = 30.0, 28.5, 0.3048
DTYPES = ("i16", "f32", "f64")
PLANES = hr.PLANES                       # the planes whose restatement tests/test_hydro_host.py checks against the invariants
PLANE_IDS = [f"{k}-{s[0]}x{s[1]}" for k, s in PLANES]
TWI_SEEN = 3.553e-15                     # the largest |twi - np.log(the same argument)| seen on these planes (module docstring)
TWI_TOL = 4 * TWI_SEEN
MIN_SLOPE_TAN = float(np.tan(np.deg2rad(0.1)))


@functools.lru_cache(maxsize=None)
def _z(kind, shape):
    z = hr.spiral(shape[0]) if kind == "spiral" else hr.plane(kind, shape)
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def _want(kind, shape, varying=False):
    """the restatement, made once per plane and left unchanged"""
    return hr.hydro(_z(kind, shape), np.nan, DX, DY, ZF, dx_row=_rows(shape) if varying else None, min_slope_tan=MIN_SLOPE_TAN)


def _rows(shape):
    return DX * (1.0 - 0.3 * np.arange(shape[0]) / max(1, shape[0] - 1))      # 30 % narrower at the last row


def _stack(kind, shape, dtype):
    import machisplin_amd as hip
    from machisplin_amd import synth
    return hip.RasterStack(synth.grid(*shape), hr.as_dtype(_z(kind, shape), dtype)[None], hr.NODATA if dtype == "i16" else float("nan"))


def _same(a, b):
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def _cap(shape):
    return 16 * (-(-shape[0] // 32) + -(-shape[1] // 64)) + 64


def _check(got, info, want, shape, what):
    assert _same(got["filled"], want["filled"]), what
    assert got["flowdir"].dtype == np.int8 and np.array_equal(got["flowdir"], want["flowdir"]), what
    assert _same(got["flowacc"], want["flowacc"]), what
    assert all(info[k] == want[k] for k in ("n_valid", "n_raised", "n_sinks")), (what, info)
    assert all(1 <= info[k] <= _cap(shape) for k in ("passes_fill", "passes_flat", "passes_acc")), (what, info)
    assert np.array_equal(np.isnan(got["twi"]), np.isnan(want["twi"])), what
    ok = ~np.isnan(want["twi"])
    diff = float(np.abs(got["twi"] - want["twi"])[ok].max()) if ok.any() else 0.0
    print(f"twi {what}: largest difference from np.log {diff:.3e} (tolerance {TWI_TOL:.3e}), passes {info['passes_fill']} "
          f"{info['passes_flat']} {info['passes_acc']}")
    assert diff <= TWI_TOL, what
    return diff


@pytest.mark.parametrize("kind,shape", PLANES, ids=PLANE_IDS)
def test_planes_equal_the_restatement_bit_for_bit(hip, kind, shape):
    import torch
    from machisplin_amd import terrain
    want = _want(kind, shape)
    for dtype in DTYPES:
        stack = _stack(kind, shape, dtype)
        got, info = terrain.hydro(stack, products=terrain.HYDRO, z_factor=ZF, dx=DX, dy=DY)
        assert got.info == info
        got = {k: v.cpu().numpy() for k, v in got.items()}
        _check(got, info, want, shape, f"{kind} {shape} {dtype}")
        # a float32 output is the float64 one rounded once; the direction does not change
        got32, _ = terrain.hydro(stack, products=terrain.HYDRO, z_factor=ZF, dx=DX, dy=DY, out_dtype=torch.float32)
        for k in ("filled", "flowacc", "twi"):
            assert _same(got32[k].cpu().numpy(), got[k].astype(np.float32)), (k, dtype)
        assert np.array_equal(got32["flowdir"].cpu().numpy(), got["flowdir"])
    if kind == "bowl" and shape[0] > 70:
        assert want["n_raised"] > 2 * 32 * 64 and want["dist"].max() > 32      # a lake over several tiles, D grows across them
    if kind == "all_na":
        assert want["n_valid"] == 0 and (got["flowdir"] == hr.DIR_NA).all()


def test_single_products_and_a_repeat(hip):
    from machisplin_amd import terrain
    kind, shape = "noise", (97, 130)
    stack, want = _stack(kind, shape, "f32"), _want(kind, shape)
    for name in terrain.HYDRO:
        plane, info = terrain.hydro(stack, products=name, z_factor=ZF, dx=DX, dy=DY)
        assert tuple(plane.shape) == shape and info["n_raised"] == want["n_raised"]
        if name != "twi":
            assert np.array_equal(plane.cpu().numpy(), want[name], equal_nan=True), name
    a, _ = terrain.hydro(stack, products=("twi", "filled"), z_factor=ZF, dx=DX, dy=DY)
    b, _ = terrain.hydro(stack, products=("twi", "filled"), z_factor=ZF, dx=DX, dy=DY)
    assert list(a) == ["twi", "filled"] and all(_same(a[k].cpu().numpy(), b[k].cpu().numpy()) for k in a)
    # the default slope floor is tan(0.1 degree), made on the host
    c, _ = terrain.hydro(stack, products="twi", z_factor=ZF, dx=DX, dy=DY, min_slope_deg=0.1)
    assert _same(c.cpu().numpy(), a["twi"].cpu().numpy())
    with pytest.raises(ValueError):
        terrain.hydro(stack, products=("twi", "slope"))


def test_dx_row_varying_by_row(hip):
    from machisplin_amd import terrain
    kind, shape = "tilted", (97, 130)
    want = _want(kind, shape, True)
    assert not np.array_equal(want["flowdir"], _want(kind, shape)["flowdir"])          # the widths change directions
    got, info = terrain.hydro(_stack(kind, shape, "f32"), products=terrain.HYDRO, z_factor=ZF, dx_row=_rows(shape), dy=DY)
    _check({k: v.cpu().numpy() for k, v in got.items()}, info, want, shape, "dx_row")


def _direct(lib, fn, shape, stack_c, rows, outs, out_dtype, ld, max_passes=0):
    """mhs_hydro_dev / mhs_hydro through ctypes"""
    from machisplin_amd import _lib, synth
    g = synth.grid(*shape).c_struct()
    u = _lib.TerrainUnits(DX, None if rows is None else rows.ctypes.data, DY, ZF)
    o = _lib.HydroOut(*outs)
    info = _lib.HydroInfo()
    head = (C.byref(g), C.byref(stack_c), stack_c.n_layers - 1, C.byref(u), MIN_SLOPE_TAN, max_passes, C.byref(o), out_dtype)
    rc = getattr(lib, fn)(*head, *((ld, None) if fn.endswith("_dev") else ()), C.byref(info))
    return rc, {k: getattr(info, k) for k, _ in _lib.HydroInfo._fields_}


def test_strided_stack_and_padded_outputs(hip):
    """the second layer of a stack whose rows are 141 elements apart (ld > ncol), outputs with ld = 150: the padding keeps
    its sentinel"""
    import torch
    from machisplin_amd import _lib
    kind, shape = "holes", (97, 130)
    nr, nc = shape
    want = _want(kind, shape)
    dev = torch.device("cuda", _lib.init())
    big = torch.full((2, nr, 141), -5.0, dtype=torch.float32, device=dev)
    big[1, :, :nc] = torch.from_numpy(hr.as_dtype(_z(kind, shape), "f32")).to(dev)
    stack_c = _lib.Stack(big.data_ptr(), 2, _lib.F32, big.stride(0), big.stride(1), float("nan"))
    out = torch.full((3, nr, 150), -7.0, dtype=torch.float64, device=dev)
    d8 = torch.full((nr, 150), -7, dtype=torch.int8, device=dev)
    rc, info = _direct(_lib.lib(), "mhs_hydro_dev", shape, stack_c, None, (out[0].data_ptr(), d8.data_ptr(), out[1].data_ptr(), out[2].data_ptr()),
                       _lib.F64, 150)
    _lib.check(rc)
    torch.cuda.synchronize()
    assert (out[:, :, nc:] == -7.0).all() and (d8[:, nc:] == -7).all()
    got = {"filled": out[0, :, :nc].cpu().numpy(), "flowdir": d8[:, :nc].cpu().numpy(), "flowacc": out[1, :, :nc].cpu().numpy(),
           "twi": out[2, :, :nc].cpu().numpy()}
    _check(got, info, want, shape, "strided")


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_entry_equals_the_device_entry(hip, dtype):
    import torch
    from machisplin_amd import _lib, terrain
    kind, shape = "noise", (97, 130)
    nr, nc = shape
    dev_planes, dev_info = terrain.hydro(_stack(kind, shape, dtype), products=terrain.HYDRO, z_factor=ZF, dx_row=_rows(shape), dy=DY,
                                         out_dtype=torch.float32)
    z = np.ascontiguousarray(hr.as_dtype(_z(kind, shape), dtype))
    stack_c = _lib.Stack(z.ctypes.data, 1, {"f64": _lib.F64, "f32": _lib.F32, "i16": _lib.I16}[dtype], nr * nc, nc,
                         hr.NODATA if dtype == "i16" else float("nan"))
    out = np.full((3, nr, nc), -7.0, dtype=np.float32)
    d8 = np.full((nr, nc), -7, dtype=np.int8)
    rows = np.ascontiguousarray(_rows(shape))
    rc, info = _direct(_lib.lib(), "mhs_hydro", shape, stack_c, rows, (out[0].ctypes.data, d8.ctypes.data, out[1].ctypes.data, out[2].ctypes.data),
                       _lib.F32, nc)
    _lib.check(rc)
    for k, name in enumerate(("filled", "flowacc", "twi")):
        assert _same(out[k], dev_planes[name].cpu().numpy()), name
    assert np.array_equal(d8, dev_planes["flowdir"].cpu().numpy())
    assert all(info[k] == dev_info[k] for k in ("n_valid", "n_raised", "n_sinks"))
    # a subset on the host: only the TWI comes down
    only = np.full((nr, nc), -7.0, dtype=np.float32)
    rc, _ = _direct(_lib.lib(), "mhs_hydro", shape, stack_c, rows, (None, None, None, only.ctypes.data), _lib.F32, nc)
    _lib.check(rc)
    assert _same(only, out[2])


def test_the_pass_cap(hip):
    """The spiral with max_passes = 4 is refused with MHS_ERR_NUMERIC: a pass solves each of the plane's six tiles at most
    once, so four passes carry the outlets' heights over at most 24 tile borders in sequence, and the channel crosses about
    ninety on its way in.  The library stays usable: the same call at the default cap succeeds."""
    import machisplin_amd as mhs
    from machisplin_amd import _lib, terrain
    shape = (96, 96)
    stack = _stack("spiral", shape, "i16")
    with pytest.raises(mhs.MhsError) as ei:
        terrain.hydro(stack, products="twi", z_factor=ZF, dx=DX, dy=DY, max_passes=4)
    assert ei.value.code == _lib.ERR_NUMERIC and "fill" in str(ei.value) and "4 passes" in str(ei.value)
    got, info = terrain.hydro(stack, products=terrain.HYDRO, z_factor=ZF, dx=DX, dy=DY)
    _check({k: v.cpu().numpy() for k, v in got.items()}, info, _want("spiral", shape), shape, "spiral after the refusal")
    assert info["passes_fill"] > 4 and info["n_sinks"] == 1
    # a cap that is just enough is enough
    got2, info2 = terrain.hydro(stack, products="flowacc", z_factor=ZF, dx=DX, dy=DY,
                                max_passes=max(info["passes_fill"], info["passes_flat"], info["passes_acc"]) + 8)
    assert np.array_equal(got2.cpu().numpy(), got["flowacc"].cpu().numpy(), equal_nan=True)


def test_covariates_with_twi_feed_mess_and_mltps_predict(hip):
    import torch
    from machisplin_amd import mltps, synth, terrain
    kind, shape = "holes", (97, 130)
    g = synth.grid(*shape)
    dem = _stack(kind, shape, "i16")
    stack = hip.covariates(dem, ("slope_deg", "twi", "log_flowacc"), z_factor=ZF)
    assert isinstance(stack, hip.RasterStack) and stack.planes.dtype == torch.float32 and stack.names == ["dem", "slope_deg", "twi", "log_flowacc"]
    planes = stack.planes.cpu().numpy()
    hp, _ = terrain.hydro(dem, products=("twi", "flowacc"), z_factor=ZF)
    assert _same(planes[2], hp["twi"].cpu().numpy().astype(np.float32))
    assert _same(planes[3], torch.log(hp["flowacc"]).cpu().numpy().astype(np.float32))
    assert _same(planes[1], terrain.terrain(dem, v="slope_deg", z_factor=ZF, out_dtype=torch.float32).cpu().numpy())
    # a spec without the hydrology entries gives what it gave: the planes of the single calls
    plain = hip.covariates(dem, ("slope_deg", ("above_min", 5)), z_factor=ZF)
    assert plain.names == ["dem", "slope_deg", "above_min5"] and _same(plain.planes[1].cpu().numpy(), planes[1])
    # ... and ("slope_deg", "twi") goes straight into Mess and mltps_predict
    stack = hip.covariates(dem, ("slope_deg", "twi"), z_factor=ZF)
    planes = stack.planes.cpu().numpy()
    xy, _, _, uv = synth.stations(g, 200, 23)
    X, _, _ = mltps.station_predictors(stack, xy)
    keep = ~np.isnan(X).any(axis=1)
    assert X.shape[1] == 5 and 60 < keep.sum() <= 200
    mess = hip.Mess(X[keep][:, :3]).grid(stack).cpu().numpy()
    assert np.array_equal(np.isnan(mess), np.isnan(planes).any(axis=0)) and (mess[~np.isnan(mess)] <= 100.0).all()
    resp = synth.response(np.nan_to_num(X), uv, 23)
    models = [hip.models.from_param_dict(p) for p in synth.ensemble_params(X[keep], resp[keep], 23, which="g")]
    res = hip.mltps_predict(stack, xy, resp, models, [1.0], 1.0, tile_edge=None, mess=True)
    final = res["final"].cpu().numpy()
    assert final.shape == shape and np.isfinite(final[~np.isnan(planes).any(axis=0)]).all() and res["n_stations"] == keep.sum()
    assert _same(res["mess"].cpu().numpy(), mess)
