"""GPU: the terrain entries of the R .Call() shim (mhsr_terrain, mhsr_relief, mhsr_geomorphon -> the host entry points
mhs_terrain, mhs_relief, mhs_geomorphon on a double plane with the layout of terra::values), executed through the stand-in R
runtime of tests/rstub, equal the Python calls on device planes bit for bit -- in one piece and with the plane going up in
several row bands.  Bad arguments come back as R errors."""
import numpy as np
import pytest

import terrain_ref as tr
from test_r_shim_exec import R  # noqa: F401  (the shim + stub runtime fixture)

pytestmark = pytest.mark.gpu

NA_INTEGER = -2**31


def test_shim_terrain_entries_equal_the_device_calls_bit_for_bit(R, hip, monkeypatch):  # noqa: F811
    from machisplin_amd import synth, terrain
    R.call("mhsr_init", R.int([0]))
    g = synth.grid(45, 77)
    rng = np.random.default_rng(11)
    r, c = np.meshgrid(np.arange(45.0), np.arange(77.0), indexing="ij")
    z = 500.0 + 4.0 * r - 2.0 * c + 20.0 * rng.standard_normal((45, 77))
    z[rng.integers(0, 45, 60), rng.integers(0, 77, 60)] = np.nan                      # NA_real_ cells
    stack = hip.RasterStack(g, z[None], float("nan"))
    rows = 30.0 * (1.0 - 0.3 * np.arange(45) / 44.0)
    pick = ("dzdy", "slope_deg", "aspect_deg", "tri")                                  # bits 1, 3, 6, 8, ascending
    mask = sum(1 << tr.VARS.index(n) for n in pick)
    want_t = terrain.terrain(stack, v=pick, z_factor=2.5, dx_row=rows, dy=28.0).cpu().numpy()
    want_r = terrain.relief(stack, 17, ("above_min", "minus_mean"), z_factor=2.5).cpu().numpy()
    want_f = terrain.geomorphon(stack, 6, 0.5, z_factor=2.5, dx_row=rows, dy=28.0).cpu().numpy()
    assert tr.terrain(z, np.nan, np.nan, 28.0, 2.5, dx_row=rows)["tri"].tobytes() == want_t[3].tobytes()
    units = R.num([np.nan, 28.0, 2.5])
    for bands in (None, "4"):
        if bands:
            monkeypatch.setenv("MHS_HOST_BANDS", bands)                                # four row bands, their halos overlapping
        t = R.values(R.call("mhsr_terrain", R.geom(g), R.num(z), units, R.num(rows), R.int([mask])))
        assert t.shape == (45 * 77, 4) and np.array_equal(t.T.reshape(4, 45, 77), want_t, equal_nan=True)
        rel = R.values(R.call("mhsr_relief", R.geom(g), R.num(z), R.num([2.5]), R.int([17]), R.int([1 | 4])))
        assert rel.shape == (45 * 77, 2) and np.array_equal(rel.T.reshape(2, 45, 77), want_r, equal_nan=True)
        f = R.values(R.call("mhsr_geomorphon", R.geom(g), R.num(z), units, R.num(rows), R.int([6]), R.num([0.5])))
        assert f.dtype == np.int32 and np.array_equal(np.where(f == NA_INTEGER, tr.GEOMORPHON_NA, f).reshape(45, 77), want_f)
        assert (f == NA_INTEGER).sum() == (want_f == tr.GEOMORPHON_NA).sum() > 0
    monkeypatch.delenv("MHS_HOST_BANDS")
    # a constant width instead of dx_row: units carry dx, dx_row is NULL
    flat_units = R.num([30.0, 28.0, 2.5])
    t = R.values(R.call("mhsr_terrain", R.geom(g), R.num(z), flat_units, R.NULL, R.int([1])))
    assert np.array_equal(t.T.reshape(1, 45, 77)[0], terrain.terrain(stack, v="dzdx", z_factor=2.5, dx=30.0, dy=28.0).cpu().numpy(), equal_nan=True)
    # refusals of the library and of the shim come back as R errors
    limit = terrain.max_radius()
    with pytest.raises(RuntimeError, match=f"radius must be in 1 .. {limit}"):
        R.call("mhsr_relief", R.geom(g), R.num(z), R.num([2.5]), R.int([limit + 1]), R.int([1]))
    with pytest.raises(RuntimeError, match=r"dx_row\[3\]"):
        bad = rows.copy(); bad[3] = -1.0
        R.call("mhsr_terrain", R.geom(g), R.num(z), units, R.num(bad), R.int([mask]))
    with pytest.raises(RuntimeError, match="mask"):
        R.call("mhsr_terrain", R.geom(g), R.num(z), units, R.num(rows), R.int([1 << 10]))
    with pytest.raises(RuntimeError, match="flat_deg"):
        R.call("mhsr_geomorphon", R.geom(g), R.num(z), units, R.num(rows), R.int([6]), R.num([-1.0]))
    with pytest.raises(RuntimeError, match="one value per cell"):
        R.call("mhsr_relief", R.geom(g), R.num(z[:-1]), R.num([2.5]), R.int([3]), R.int([1]))
    with pytest.raises(RuntimeError, match="one width per row"):
        R.call("mhsr_geomorphon", R.geom(g), R.num(z), units, R.num(rows[:-1]), R.int([6]), R.num([0.5]))
