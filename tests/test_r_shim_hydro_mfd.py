"""GPU: the multiple-flow-direction hydrology entry of the R .Call() shim (mhsr_hydro_mfd -> the host entry point
mhs_hydro_mfd on a double plane with the layout of terra::values), executed through the stand-in R runtime of tests/rstub,
equals the Python call on a device plane bit for bit, and at the exponent 1 the restatement (tests/hydro_mfd_ref.py).  Bad
arguments come back as R errors."""
import numpy as np
import pytest

import hydro_mfd_ref as mr
import hydro_ref as hr
from test_r_shim_exec import R  # noqa: F401  (the shim + stub runtime fixture)

pytestmark = pytest.mark.gpu


def test_shim_hydro_mfd_equals_the_device_call_bit_for_bit(R, hip):  # noqa: F811
    from machisplin_amd import synth, terrain
    R.call("mhsr_init", R.int([0]))
    shape = (45, 77)
    g = synth.grid(*shape)
    z = hr.plane("holes", shape)                                                       # NA_real_ cells
    stack = hip.RasterStack(g, z[None], float("nan"))
    rows = 30.0 * (1.0 - 0.3 * np.arange(45) / 44.0)
    floor = float(np.tan(np.deg2rad(0.25)))
    units = R.num([np.nan, 28.0, 2.5])
    for x in (1.0, 1.1):
        want, want_info = terrain.hydro_mfd(stack, products=terrain.HYDRO_MFD, exponent=x, z_factor=2.5, min_slope_deg=0.25, dx_row=rows, dy=28.0)
        want = {k: v.cpu().numpy() for k, v in want.items()}
        out = R.values(R.call("mhsr_hydro_mfd", R.geom(g), R.num(z), units, R.num(rows), R.int([7]), R.num([floor, 0, x])))
        assert len(out) == 4
        for k, name in enumerate(terrain.HYDRO_MFD):
            v = R.values(out[k])
            assert v.dtype == np.float64 and np.array_equal(v.reshape(shape), want[name], equal_nan=True), (name, x)
        info = R.values(out[3])
        assert list(info[3:]) == [want_info["n_valid"], want_info["n_raised"], want_info["n_sinks"]] and (info[:3] >= 1).all()
        if x == 1.0:
            ref = mr.hydro_mfd(z, np.nan, np.nan, 28.0, 1.0, 2.5, dx_row=rows, min_slope_tan=floor)
            assert all(np.array_equal(want[k], ref[k], equal_nan=True) for k in ("filled", "flowacc"))
            assert np.isnan(want["flowacc"]).sum() == np.isnan(z).sum() > 0
    # a subset: the planes not asked for are NULL; a constant width instead of dx_row
    out = R.values(R.call("mhsr_hydro_mfd", R.geom(g), R.num(z), R.num([30.0, 28.0, 2.5]), R.NULL, R.int([4]), R.num([floor, 0, 1.1])))
    assert out[0] == R.NULL and out[1] == R.NULL
    twi, _ = terrain.hydro_mfd(stack, products="twi", z_factor=2.5, min_slope_deg=0.25, dx=30.0, dy=28.0)
    assert np.array_equal(R.values(out[2]).reshape(shape), twi.cpu().numpy(), equal_nan=True)
    # refusals of the library and of the shim come back as R errors
    with pytest.raises(RuntimeError, match="exponent"):
        R.call("mhsr_hydro_mfd", R.geom(g), R.num(z), units, R.num(rows), R.int([7]), R.num([floor, 0, 65.0]))
    with pytest.raises(RuntimeError, match="min_slope_tan"):
        R.call("mhsr_hydro_mfd", R.geom(g), R.num(z), units, R.num(rows), R.int([7]), R.num([0.0, 0, 1.1]))
    with pytest.raises(RuntimeError, match="products must be a bit mask"):
        R.call("mhsr_hydro_mfd", R.geom(g), R.num(z), units, R.num(rows), R.int([8]), R.num([floor, 0, 1.1]))
    with pytest.raises(RuntimeError, match="opts must be"):
        R.call("mhsr_hydro_mfd", R.geom(g), R.num(z), units, R.num(rows), R.int([7]), R.num([floor, 0]))
    with pytest.raises(RuntimeError, match="max_passes"):
        R.call("mhsr_hydro_mfd", R.geom(g), R.num(z), units, R.num(rows), R.int([7]), R.num([floor, -1, 1.1]))
    with pytest.raises(RuntimeError, match="one value per cell"):
        R.call("mhsr_hydro_mfd", R.geom(g), R.num(z[:-1]), units, R.num(rows), R.int([7]), R.num([floor, 0, 1.1]))
    with pytest.raises(RuntimeError, match="one width per row"):
        R.call("mhsr_hydro_mfd", R.geom(g), R.num(z), units, R.num(rows[:-1]), R.int([7]), R.num([floor, 0, 1.1]))
