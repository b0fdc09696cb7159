"""GPU: the multiple-flow-direction hydrology of a DEM (csrc/hydro.hip, machisplin_amd/terrain.py: hydro_mfd) against the
restatement of the rules by other algorithms (tests/hydro_mfd_ref.py: shares in numpy, accumulation by one walk in
topological order; tests/hydro_ref.py for W and D).

With the exponent 1 only subtraction, division, multiplication and sums go into the accumulation, each rounded once, and the
monotone tile sweeps reach the one fixed point whatever the schedule: the filled surface and the accumulation must equal the
restatement BIT FOR BIT, on the int16, float32 and float64 stacks of every plane.  The TWI then differs from numpy only
through log on bit-identical arguments: the bound measured in tests/test_hydro_gpu.py applies, 4 x 3.553e-15 absolute.

With another exponent the shares go through pow, the device's against numpy's.  No OCML accuracy table comes with the ROCm
installation, so the bound is measured: the largest relative difference of the accumulation from the restatement on these
planes (float32 stacks) at the exponents 1.1 and 8 was ACC_SEEN = 1.527e-15 (the spiral at 1.1, whose channel carries the
shares of its walls through 9 216 cells; 1.069e-15 at 8, the bowl of 200 x 300); the tolerance is 4 x that, and the test also
asserts that the figure lies below 1e-11, the cap derived in tests/hydro_mfd_ref.py (three roundings per step along the
longest path, pow within a few ulp).  The TWI at those exponents gets that relative tolerance on top of the log bound: an
accumulation off by a relative e moves its log by e.

The pass cap: the issue's case (max_passes = 1 on the spiral) is refused with MHS_ERR_NUMERIC, but by the FILL phase, which
runs first under the same cap and cannot end in one pass on a plane whose fill changes anything; so that the message naming the
accumulation is checked too, the ramp of 1 x 70 (two tiles, every cell an outlet: fill and flat distance end in their first
pass, the accumulation crosses the tile border) is run at the same cap."""
import ctypes as C
import functools

import numpy as np
import pytest

import hydro_mfd_ref as mr
import hydro_ref as hr

pytestmark = pytest.mark.gpu

DX, DY, ZF = 30.0, 28.5, 0.3048
DTYPES = ("i16", "f32", "f64")
PLANES = mr.PLANES
PLANE_IDS = [f"{k}-{s[0]}x{s[1]}" for k, s in PLANES]
TWI_TOL = 4 * 3.553e-15                  # the log bound measured in tests/test_hydro_gpu.py
ACC_SEEN = 1.527e-15                     # the largest relative difference of flowacc at the exponents 1.1 and 8 (module docstring)
ACC_TOL = 4 * ACC_SEEN
ACC_CAP = 1e-11                          # what ACC_SEEN must stay below (tests/hydro_mfd_ref.py: SINK_SUM_RTOL's derivation)
MIN_SLOPE_TAN = float(np.tan(np.deg2rad(0.1)))


@functools.lru_cache(maxsize=None)
def _z(kind, shape):
    z = mr.plane(kind, shape)
    z.setflags(write=False)
    return z


def _rows(shape):
    return DX * (1.0 - 0.3 * np.arange(shape[0]) / max(1, shape[0] - 1))      # 30 % narrower at the last row


@functools.lru_cache(maxsize=None)
def _base(kind, shape, varying=False):
    return hr.hydro(_z(kind, shape), np.nan, DX, DY, ZF, dx_row=_rows(shape) if varying else None, min_slope_tan=MIN_SLOPE_TAN)


@functools.lru_cache(maxsize=None)
def _want(kind, shape, x, varying=False):
    """the restatement, made once per plane and exponent and left unchanged"""
    return mr.hydro_mfd(_z(kind, shape), np.nan, DX, DY, x, ZF, dx_row=_rows(shape) if varying else None, min_slope_tan=MIN_SLOPE_TAN,
                        base=_base(kind, shape, varying))


def _stack(kind, shape, dtype):
    import machisplin_amd as hip
    from machisplin_amd import synth
    return hip.RasterStack(synth.grid(*shape), hr.as_dtype(_z(kind, shape), dtype)[None], hr.NODATA if dtype == "i16" else float("nan"))


def _same(a, b):
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def _cap(shape):
    return 16 * (-(-shape[0] // 32) + -(-shape[1] // 64)) + 64


def _np(planes):
    return {k: v.cpu().numpy() for k, v in planes.items()}


def _check_counts(info, want, shape, what):
    assert all(info[k] == want[k] for k in ("n_valid", "n_raised", "n_sinks")), (what, info)
    assert all(1 <= info[k] <= _cap(shape) for k in ("passes_fill", "passes_flat", "passes_acc")), (what, info)


def _check_twi(got, want, tol, what):
    assert np.array_equal(np.isnan(got), np.isnan(want["twi"])), what
    ok = ~np.isnan(want["twi"])
    with np.errstate(invalid="ignore"):
        diff = float(np.abs(got - np.log(want["twi_arg"]))[ok].max()) if ok.any() else 0.0
    print(f"twi {what}: largest difference from np.log {diff:.3e} (tolerance {tol:.3e})")
    assert diff <= tol, what


def _check_exact(got, info, want, shape, what):
    """the exponent 1: everything but the log bit for bit"""
    assert _same(got["filled"], want["filled"]), what
    assert _same(got["flowacc"], want["flowacc"]), what
    _check_counts(info, want, shape, what)
    _check_twi(got["twi"], want, TWI_TOL, what)


def _rel(got, want):
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), ~ok)
    return float((np.abs(got - want)[ok] / want[ok]).max()) if ok.any() else 0.0


@pytest.mark.parametrize("kind,shape", PLANES, ids=PLANE_IDS)
def test_exponent_one_equals_the_restatement_bit_for_bit(hip, kind, shape):
    import torch
    from machisplin_amd import terrain
    want = _want(kind, shape, 1.0)
    for dtype in DTYPES:
        stack = _stack(kind, shape, dtype)
        got, info = terrain.hydro_mfd(stack, products=terrain.HYDRO_MFD, exponent=1.0, z_factor=ZF, dx=DX, dy=DY)
        assert got.info == info and list(got) == list(terrain.HYDRO_MFD)
        got = _np(got)
        _check_exact(got, info, want, shape, f"{kind} {shape} {dtype}")
        # a float32 output is the float64 one rounded once
        got32, _ = terrain.hydro_mfd(stack, products=terrain.HYDRO_MFD, exponent=1.0, z_factor=ZF, dx=DX, dy=DY, out_dtype=torch.float32)
        for k in terrain.HYDRO_MFD:
            assert _same(got32[k].cpu().numpy(), got[k].astype(np.float32)), (k, dtype)
    if kind == "all_na":
        assert want["n_valid"] == 0 and np.isnan(got["flowacc"]).all()
    if kind == "constant" and min(shape) > 2:
        assert want["n_raised"] == 0 and got["flowacc"].max() > 1.0            # flat sharing only


@pytest.mark.parametrize("kind,shape", PLANES, ids=PLANE_IDS)
def test_other_exponents_within_the_measured_bound(hip, kind, shape):
    from machisplin_amd import terrain
    assert ACC_SEEN < ACC_CAP
    stack = _stack(kind, shape, "f32")
    for x in (1.1, 8.0):
        want = _want(kind, shape, x)
        got, info = terrain.hydro_mfd(stack, products=terrain.HYDRO_MFD, exponent=x, z_factor=ZF, dx=DX, dy=DY)
        got = _np(got)
        assert _same(got["filled"], want["filled"])
        _check_counts(info, want, shape, f"{kind} {shape} x = {x}")
        rel = _rel(got["flowacc"], want["flowacc"])
        print(f"flowacc {kind} {shape} x = {x}: largest relative difference {rel:.3e} (tolerance {ACC_TOL:.3e})")
        assert rel <= ACC_TOL, (kind, shape, x, rel)
        _check_twi(got["twi"], want, TWI_TOL + ACC_TOL, f"{kind} {shape} x = {x}")


def test_dx_row_varying_by_row(hip):
    """a share uses the width of the DONOR's row: still bit for bit at the exponent 1"""
    from machisplin_amd import terrain
    kind, shape = "tilted", (97, 130)
    want = _want(kind, shape, 1.0, True)
    assert not np.array_equal(want["flowacc"], _want(kind, shape, 1.0)["flowacc"])          # the widths change the shares
    got, info = terrain.hydro_mfd(_stack(kind, shape, "f32"), products=terrain.HYDRO_MFD, exponent=1.0, z_factor=ZF, dx_row=_rows(shape), dy=DY)
    _check_exact(_np(got), info, want, shape, "dx_row")


def test_single_products_and_a_repeat(hip):
    from machisplin_amd import terrain
    kind, shape = "noise", (97, 130)
    stack, want = _stack(kind, shape, "f32"), _want(kind, shape, 1.0)
    for name in terrain.HYDRO_MFD:
        plane, info = terrain.hydro_mfd(stack, products=name, exponent=1.0, z_factor=ZF, dx=DX, dy=DY)
        assert tuple(plane.shape) == shape and info["n_raised"] == want["n_raised"]
        if name != "twi":
            assert np.array_equal(plane.cpu().numpy(), want[name], equal_nan=True), name
    a, _ = terrain.hydro_mfd(stack, products=("twi", "flowacc"), z_factor=ZF, dx=DX, dy=DY)
    b, _ = terrain.hydro_mfd(stack, products=("twi", "flowacc"), z_factor=ZF, dx=DX, dy=DY)
    assert list(a) == ["twi", "flowacc"] and all(_same(a[k].cpu().numpy(), b[k].cpu().numpy()) for k in a)
    c, _ = terrain.hydro_mfd(stack, products="twi", exponent=1.1, z_factor=ZF, dx=DX, dy=DY)        # 1.1 is the default
    assert _same(c.cpu().numpy(), a["twi"].cpu().numpy())
    with pytest.raises(ValueError):
        terrain.hydro_mfd(stack, products=("twi", "flowdir"))


def _direct(lib, fn, shape, stack_c, rows, outs, out_dtype, ld, x, max_passes=0):
    """mhs_hydro_mfd_dev / mhs_hydro_mfd through ctypes"""
    from machisplin_amd import _lib, synth
    g = synth.grid(*shape).c_struct()
    u = _lib.TerrainUnits(DX, None if rows is None else rows.ctypes.data, DY, ZF)
    o = _lib.HydroMfdOut(*outs)
    info = _lib.HydroInfo()
    head = (C.byref(g), C.byref(stack_c), stack_c.n_layers - 1, C.byref(u), MIN_SLOPE_TAN, max_passes, x, C.byref(o), out_dtype)
    rc = getattr(lib, fn)(*head, *((ld, None) if fn.endswith("_dev") else ()), C.byref(info))
    return rc, {k: getattr(info, k) for k, _ in _lib.HydroInfo._fields_}


def test_strided_stack_and_padded_outputs(hip):
    """the second layer of a stack whose rows are 141 elements apart (ld > ncol), outputs with ld = 150: the padding keeps
    its sentinel"""
    import torch
    from machisplin_amd import _lib
    kind, shape = "holes", (97, 130)
    nr, nc = shape
    want = _want(kind, shape, 1.0)
    dev = torch.device("cuda", _lib.init())
    big = torch.full((2, nr, 141), -5.0, dtype=torch.float32, device=dev)
    big[1, :, :nc] = torch.from_numpy(hr.as_dtype(_z(kind, shape), "f32")).to(dev)
    stack_c = _lib.Stack(big.data_ptr(), 2, _lib.F32, big.stride(0), big.stride(1), float("nan"))
    out = torch.full((3, nr, 150), -7.0, dtype=torch.float64, device=dev)
    rc, info = _direct(_lib.lib(), "mhs_hydro_mfd_dev", shape, stack_c, None, (out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr()),
                       _lib.F64, 150, 1.0)
    _lib.check(rc)
    torch.cuda.synchronize()
    assert (out[:, :, nc:] == -7.0).all()
    got = {"filled": out[0, :, :nc].cpu().numpy(), "flowacc": out[1, :, :nc].cpu().numpy(), "twi": out[2, :, :nc].cpu().numpy()}
    _check_exact(got, info, want, shape, "strided")


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_entry_equals_the_device_entry(hip, dtype):
    import torch
    from machisplin_amd import _lib, terrain
    kind, shape = "noise", (97, 130)
    nr, nc = shape
    dev_planes, dev_info = terrain.hydro_mfd(_stack(kind, shape, dtype), products=terrain.HYDRO_MFD, z_factor=ZF, dx_row=_rows(shape), dy=DY,
                                             out_dtype=torch.float32)
    z = np.ascontiguousarray(hr.as_dtype(_z(kind, shape), dtype))
    stack_c = _lib.Stack(z.ctypes.data, 1, {"f64": _lib.F64, "f32": _lib.F32, "i16": _lib.I16}[dtype], nr * nc, nc,
                         hr.NODATA if dtype == "i16" else float("nan"))
    out = np.full((3, nr, nc), -7.0, dtype=np.float32)
    rows = np.ascontiguousarray(_rows(shape))
    rc, info = _direct(_lib.lib(), "mhs_hydro_mfd", shape, stack_c, rows, (out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data), _lib.F32, nc, 1.1)
    _lib.check(rc)
    for k, name in enumerate(terrain.HYDRO_MFD):
        assert _same(out[k], dev_planes[name].cpu().numpy()), name
    assert all(info[k] == dev_info[k] for k in ("n_valid", "n_raised", "n_sinks"))
    # a subset on the host: only the TWI comes down
    only = np.full((nr, nc), -7.0, dtype=np.float32)
    rc, _ = _direct(_lib.lib(), "mhs_hydro_mfd", shape, stack_c, rows, (None, None, only.ctypes.data), _lib.F32, nc, 1.1)
    _lib.check(rc)
    assert _same(only, out[2])


def test_the_pass_cap(hip):
    """max_passes = 1: the spiral is refused by the fill, the ramp (fill and flat distance end in one pass) by the
    accumulation (module docstring); the library stays usable, and the spiral at the default cap equals the restatement."""
    import machisplin_amd as mhs
    from machisplin_amd import _lib, terrain
    shape = (96, 96)
    stack = _stack("spiral", shape, "i16")
    with pytest.raises(mhs.MhsError) as ei:
        terrain.hydro_mfd(stack, products="twi", exponent=1.0, z_factor=ZF, dx=DX, dy=DY, max_passes=1)
    assert ei.value.code == _lib.ERR_NUMERIC and "1 passes" in str(ei.value) and "phase" in str(ei.value)
    with pytest.raises(mhs.MhsError) as ei:
        terrain.hydro_mfd(_stack("ramp", (1, 70), "f32"), products="flowacc", exponent=1.0, z_factor=ZF, dx=DX, dy=DY, max_passes=1)
    assert ei.value.code == _lib.ERR_NUMERIC and "accumulation" in str(ei.value) and "1 passes" in str(ei.value)
    got, info = terrain.hydro_mfd(stack, products=terrain.HYDRO_MFD, exponent=1.0, z_factor=ZF, dx=DX, dy=DY)
    _check_exact(_np(got), info, _want("spiral", shape, 1.0), shape, "spiral after the refusal")
    assert info["passes_acc"] > 4 and info["n_sinks"] == 1


@pytest.mark.parametrize("bad", [0.0, 65.0, float("nan")])
def test_a_bad_exponent_is_refused(hip, bad):
    import machisplin_amd as mhs
    from machisplin_amd import _lib, terrain
    with pytest.raises(mhs.MhsError) as ei:
        terrain.hydro_mfd(_stack("noise", (2, 2), "f32"), exponent=bad)
    assert ei.value.code == _lib.ERR_INVALID and "exponent" in str(ei.value)


def test_the_ramp_equals_d8(hip):
    """every cell of the ramp has one receiver: MFD is D8, whatever the exponent"""
    from machisplin_amd import terrain
    stack = _stack("ramp", (1, 70), "f32")
    d8, _ = terrain.hydro(stack, products="flowacc", z_factor=ZF, dx=DX, dy=DY)
    for x in (1.0, 1.1, 8.0):
        got, _ = terrain.hydro_mfd(stack, products="flowacc", exponent=x, z_factor=ZF, dx=DX, dy=DY)
        assert _same(got.cpu().numpy(), d8.cpu().numpy()) and got[0, 0].item() == 70.0


def test_covariates_with_the_mfd_layers_feed_mess_and_mltps_predict(hip):
    import torch
    from machisplin_amd import mltps, synth, terrain
    kind, shape = "holes", (97, 130)
    g = synth.grid(*shape)
    dem = _stack(kind, shape, "i16")
    stack = hip.covariates(dem, ("twi_mfd", "log_flowacc_mfd", "twi"), z_factor=ZF)
    assert isinstance(stack, hip.RasterStack) and stack.planes.dtype == torch.float32
    assert stack.names == ["dem", "twi_mfd", "log_flowacc_mfd", "twi"]
    planes = stack.planes.cpu().numpy()
    hp, _ = terrain.hydro_mfd(dem, products=("twi", "flowacc"), z_factor=ZF)
    assert _same(planes[1], hp["twi"].cpu().numpy().astype(np.float32))
    assert _same(planes[2], torch.log(hp["flowacc"]).cpu().numpy().astype(np.float32))
    # the D8 layer is what covariates gives without the MFD entries, and what hydro gives
    assert _same(planes[3], hip.covariates(dem, ("twi",), z_factor=ZF).planes[1].cpu().numpy())
    assert _same(planes[3], terrain.hydro(dem, products="twi", z_factor=ZF)[0].cpu().numpy().astype(np.float32))
    assert not _same(planes[1], planes[3])
    xy, _, _, uv = synth.stations(g, 200, 23)
    X, _, _ = mltps.station_predictors(stack, xy)
    keep = ~np.isnan(X).any(axis=1)
    assert X.shape[1] == 6 and 60 < keep.sum() <= 200
    mess = hip.Mess(X[keep][:, :4]).grid(stack).cpu().numpy()
    assert np.array_equal(np.isnan(mess), np.isnan(planes).any(axis=0)) and (mess[~np.isnan(mess)] <= 100.0).all()
    resp = synth.response(np.nan_to_num(X), uv, 23)
    models = [hip.models.from_param_dict(p) for p in synth.ensemble_params(X[keep], resp[keep], 23, which="g")]
    res = hip.mltps_predict(stack, xy, resp, models, [1.0], 1.0, tile_edge=None, mess=True)
    final = res["final"].cpu().numpy()
    assert final.shape == shape and np.isfinite(final[~np.isnan(planes).any(axis=0)]).all() and res["n_stations"] == keep.sum()
    assert _same(res["mess"].cpu().numpy(), mess)
