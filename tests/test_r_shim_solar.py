"""GPU: the solar entry of the R .Call() shim (mhsr_solar -> the host entry point mhs_solar on a double plane with the layout of
terra::values, the sun tables handed over as an R list), executed through the stand-in R runtime of tests/rstub, equals the
Python call on a device plane and the restatement (tests/solar_ref.py) bit for bit.  Bad arguments come back as R errors."""
import numpy as np
import pytest

import hydro_ref as hr
import solar_ref as sr
from test_r_shim_exec import R  # noqa: F401  (the shim + stub runtime fixture)

pytestmark = pytest.mark.gpu


def _r_tables(R, t, start_as_int=False):  # noqa: F811
    start = R.int(t.start) if start_as_int else R.num(t.start)
    return R.list([R.mat(t.entries), start, R.num(t.omega), R.NULL if t.tab_row is None else R.int(t.tab_row)])


def test_shim_solar_equals_the_device_call_bit_for_bit(R, hip):  # noqa: F811
    from machisplin_amd import synth, terrain
    R.call("mhsr_init", R.int([0]))
    shape = (45, 77)
    g = synth.grid(*shape)
    z = hr.plane("holes", shape)                                                       # NA_real_ cells
    assert 0 < np.isnan(z).sum() < z.size // 2
    stack = hip.RasterStack(g, z[None], float("nan"))
    rows = 30.0 * (1.0 - 0.3 * np.arange(45) / 44.0)
    a = terrain.sun_tables(g, lat=45.0, dx=30.0, dy=28.0, step_minutes=60)
    b = terrain.sun_tables(g, lat=10.0, dx=30.0, dy=28.0, days=(172,), step_minutes=60)
    two = terrain.SunTables(np.concatenate([a.start, b.start[1:] + a.start[-1]]), np.concatenate([a.entries, b.entries]),
                            np.concatenate([a.omega, b.omega]), (np.arange(45) >= 20).astype(np.int32))
    units = R.num([np.nan, 28.0, 2.5])
    want = terrain.solar(stack, 6, terrain.SOLAR, two, z_factor=2.5, dx_row=rows, dy=28.0).cpu().numpy()
    assert np.array_equal(want, sr.planes(sr.solar(z, np.nan, 6, two, np.nan, 28.0, 2.5, dx_row=rows), sr.SOLAR), equal_nan=True)
    for as_int in (False, True):
        out = R.values(R.call("mhsr_solar", R.geom(g), R.num(z), units, R.num(rows), R.int([6]), R.int([15]), _r_tables(R, two, as_int)))
        assert out.dtype == np.float64 and out.shape == (45 * 77, 19)
        assert np.array_equal(out.T.reshape((19,) + shape), want, equal_nan=True)
    # a subset, one table, a constant width; the horizon alone needs no tables
    out = R.values(R.call("mhsr_solar", R.geom(g), R.num(z), R.num([30.0, 28.0, 2.5]), R.NULL, R.int([6]), R.int([5]), _r_tables(R, a)))
    sub = terrain.solar(stack, 6, ("svf", "sun_hours"), a, z_factor=2.5, dx=30.0, dy=28.0).cpu().numpy()
    assert out.shape == (45 * 77, 2) and np.array_equal(out.T.reshape((2,) + shape), sub, equal_nan=True)
    out = R.values(R.call("mhsr_solar", R.geom(g), R.num(z), R.num([30.0, 28.0, 2.5]), R.NULL, R.int([6]), R.int([8]), R.NULL))
    hor = terrain.solar(stack, 6, "horizon", z_factor=2.5, dx=30.0, dy=28.0).cpu().numpy()
    assert out.shape == (45 * 77, 16) and np.array_equal(out.T.reshape((16,) + shape), hor, equal_nan=True)
    # refusals of the library and of the shim come back as R errors
    call = lambda *tail: R.call("mhsr_solar", R.geom(g), R.num(z), units, R.num(rows), *tail)  # noqa: E731
    with pytest.raises(RuntimeError, match="search must be in 1 .. 45"):
        call(R.int([46]), R.int([15]), _r_tables(R, two))
    with pytest.raises(RuntimeError, match="tables is NULL"):
        call(R.int([6]), R.int([1]), R.NULL)
    bad = terrain.SunTables(two.start, two.entries.copy(), two.omega, two.tab_row)
    bad.entries[4, 1] = 0.0
    with pytest.raises(RuntimeError, match=r"entries\[4\].tan_h"):
        call(R.int([6]), R.int([15]), _r_tables(R, bad))
    with pytest.raises(RuntimeError, match="products must be a bit mask"):
        call(R.int([6]), R.int([16]), _r_tables(R, two))
    with pytest.raises(RuntimeError, match="tables must be list"):
        call(R.int([6]), R.int([15]), R.list([R.mat(two.entries)]))
    with pytest.raises(RuntimeError, match="8 columns"):
        call(R.int([6]), R.int([15]), R.list([R.mat(two.entries[:, :7]), R.num(two.start), R.num(two.omega), R.NULL]))
    with pytest.raises(RuntimeError, match="start must hold"):
        call(R.int([6]), R.int([15]), R.list([R.mat(two.entries), R.num(two.start[:-1]), R.num(two.omega), R.NULL]))
    with pytest.raises(RuntimeError, match=r"start\[33\] is not an offset"):
        call(R.int([6]), R.int([15]), R.list([R.mat(two.entries), R.num(two.start + (np.arange(33) == 32)), R.num(two.omega), R.NULL]))
    with pytest.raises(RuntimeError, match="tab_row must be"):
        call(R.int([6]), R.int([15]), R.list([R.mat(two.entries), R.num(two.start), R.num(two.omega), R.int(two.tab_row[:-1])]))
    with pytest.raises(RuntimeError, match="one value per cell"):
        R.call("mhsr_solar", R.geom(g), R.num(z[:-1]), units, R.num(rows), R.int([6]), R.int([15]), _r_tables(R, two))
    with pytest.raises(RuntimeError, match="one width per row"):
        R.call("mhsr_solar", R.geom(g), R.num(z), units, R.num(rows[:-1]), R.int([6]), R.int([15]), _r_tables(R, two))
