"""GPU: the warp entry of the R .Call() shim (mhsr_warp -> the host entry point mhs_warp: the whole stack and the lattice go up in
one piece, the same kernel runs), executed through the stand-in R runtime of tests/rstub, equals the direct C call on device
planes (project.warp -> mhs_warp_dev) bit for bit.  Bad arguments come back as R errors."""
import ctypes as C
import math

import numpy as np
import pytest

import warp_ref as wr
from test_r_shim_exec import R  # noqa: F401  (the shim + stub runtime fixture)

pytestmark = pytest.mark.gpu


def test_shim_warp_equals_the_device_call_bit_for_bit(R, hip):  # noqa: F811
    import torch
    from machisplin_amd import Geometry, _lib, project as pj
    R.call("mhsr_init", R.int([0]))
    S = Geometry(5.625, 45.25, 1.0 / 1200.0, 1.0 / 1200.0, 45, 77)
    rng = np.random.default_rng(13)
    r, c = np.meshgrid(np.arange(45.0), np.arange(77.0), indexing="ij")
    z = np.stack([500.0 + 4.0 * r - 2.0 * c + 20.0 * rng.standard_normal((45, 77)), 10.0 + rng.standard_normal((45, 77))])
    z[0, rng.integers(0, 45, 60), rng.integers(0, 77, 60)] = np.nan                    # NA_real_ cells
    z[1, 20:24, 30:37] = -9999.0                                                       # ... and a nodata value
    stack = hip.RasterStack(S, z, -9999.0)
    values = z.reshape(2, -1).T                                                        # terra::values: ncell x C
    crs = pj.utm(31)
    x, y = pj.transform(pj.LONLAT, crs, S.xmin + 0.5 * S.ncol * S.xres, S.ymax - 0.5 * S.nrow * S.yres)
    T = Geometry(math.floor(float(x) / 50.0) * 50.0 - 3500.0, math.floor(float(y) / 50.0) * 50.0 + 2000.0, 50.0, 50.0, 75, 140)
    for tol in (0.01, 1e-4):                                                           # a coarse and a fine lattice
        lat = pj.lattice(pj.LONLAT, crs, T, S, tol=tol)
        for code, method in enumerate(("near", "bilinear", "cubic")):
            want = pj.warp(stack, T, lat, method, out_dtype=torch.float64).planes.cpu().numpy()
            got = R.values(R.call("mhsr_warp", R.geom(S), R.mat(values), R.num([-9999.0]), R.geom(T), R.int([lat.step]), R.num(lat.sx), R.num(lat.sy),
                                  R.int([code])))
            assert got.shape == (T.nrow * T.ncol, 2) and np.array_equal(got.T.reshape(2, T.nrow, T.ncol), want, equal_nan=True), (tol, method)
            assert np.array_equal(want, np.stack([wr.warp(p, -9999.0, S, T, lat, method) for p in z]), equal_nan=True)
            assert np.isnan(want).any() and (~np.isnan(want)).mean() > 0.5
    # the host entry point itself: a window, float32 output, a float32 stack with padded rows
    zf = np.full((2, 45, 80), -7.0, dtype=np.float32)
    zf[:, :, :77] = z.astype(np.float32)
    zf[np.isnan(zf)] = -9999.0
    st = _lib.Stack(zf.ctypes.data, 2, _lib.F32, 45 * 80, 80, -9999.0)
    cl = _lib.WarpLattice(lat.step, lat.sx.shape[0], lat.sx.shape[1], lat.sx.ctypes.data, lat.sy.ctypes.data)
    out = np.zeros((2, 60, 100), dtype=np.float32)
    sg, tg = S.c_struct(), T.c_struct()
    rc = _lib.lib().mhs_warp(C.byref(sg), C.byref(st), C.byref(tg), 10, 70, 30, 130, C.byref(cl), 2, out.ctypes.data, _lib.F32)
    assert rc == _lib.OK, _lib.lib().mhs_last_error()
    ref = np.stack([wr.warp(p, -9999.0, S, T, lat, "cubic", (10, 70, 30, 130)) for p in zf[:, :, :77]]).astype(np.float32)
    assert np.array_equal(out, ref, equal_nan=True)
    # one layer as a plain vector, NA_real_ for "no nodata value"
    got = R.values(R.call("mhsr_warp", R.geom(S), R.num(z[0]), R.num([np.nan]), R.geom(T), R.int([lat.step]), R.num(lat.sx), R.num(lat.sy), R.int([1])))
    assert np.array_equal(got.reshape(T.nrow, T.ncol), wr.warp(z[0], np.nan, S, T, lat, "bilinear"), equal_nan=True)
    # refusals of the library and of the shim come back as R errors
    args = lambda **kw: [kw.get("geom", R.geom(S)), kw.get("planes", R.mat(values)), R.num([np.nan]), R.geom(T), R.int([kw.get("step", lat.step)]),
                         kw.get("sx", R.num(lat.sx)), R.num(lat.sy), R.int([kw.get("method", 1)])]
    with pytest.raises(RuntimeError, match="aggregate method"):
        R.call("mhsr_warp", *args(method=3))
    with pytest.raises(RuntimeError, match="unknown method"):
        R.call("mhsr_warp", *args(method=8))
    with pytest.raises(RuntimeError, match="power of two"):
        R.call("mhsr_warp", *args(step=48))
    with pytest.raises(RuntimeError, match="nodes"):
        R.call("mhsr_warp", *args(sx=R.num(lat.sx[:-1])))
    with pytest.raises(RuntimeError, match="nodes"):
        R.call("mhsr_warp", *args(step=2 * lat.step if lat.step < 512 else lat.step // 2))
    with pytest.raises(RuntimeError, match="one row per cell"):
        R.call("mhsr_warp", *args(planes=R.mat(values[:-1])))
    with pytest.raises(RuntimeError, match="cell size"):
        R.call("mhsr_warp", *args(geom=R.geom(Geometry(0.0, 1.0, 0.0, 1.0, 45, 77))))
