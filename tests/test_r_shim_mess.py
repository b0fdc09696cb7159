"""GPU: the MESS entry of the R .Call() shim (mhsr_mess_grid -> mhs_mess_create + mhs_mess_grid on host planes with the
layout of terra::values), executed through the stand-in R runtime of tests/rstub, equals Mess.grid on device planes bit for
bit, MoD included -- in one piece and with the planes going up in several row bands."""
import numpy as np
import pytest

import mess_ref
from test_r_shim_exec import R  # noqa: F401  (the shim + stub runtime fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("lonlat", [False, True])
def test_shim_mess_grid_equals_the_device_call_bit_for_bit(R, hip, monkeypatch, lonlat):  # noqa: F811
    from machisplin_amd import synth
    R.call("mhsr_init", R.int([0]))
    g = synth.grid(131, 173)
    rng = np.random.default_rng(3 + lonlat)
    planes = rng.standard_normal((3, g.nrow, g.ncol)) * 40.0 + 100.0
    rr, cc = rng.integers(10, 120, size=150), rng.integers(10, 160, size=150)
    ref = np.column_stack([planes[k, rr, cc] for k in range(3)] + [g.x_from_col(cc), g.y_from_row(rr)])[:, :5 if lonlat else 3]
    planes[rng.integers(0, 3, 300), rng.integers(0, g.nrow, 300), rng.integers(0, g.ncol, 300)] = np.nan      # NA_real_ cells
    stack = hip.RasterStack(g, planes, float("nan"))
    want, want_mod = hip.Mess(ref).grid(stack, mod=True)
    want, want_mod = want.cpu().numpy(), want_mod.cpu().numpy()
    ref_m, ref_v = mess_ref.mess(ref, mess_ref.grid_values(g, planes, float("nan"), ref.shape[1]))
    assert np.array_equal(want, ref_m, equal_nan=True) and np.array_equal(want_mod, ref_v)
    values = planes.reshape(3, -1).T                                  # terra::values(covar.ras): ncell x C
    for bands in (None, "3"):
        if bands:
            monkeypatch.setenv("MHS_HOST_BANDS", bands)               # three row bands through the host pipeline's arena
        out = R.values(R.call("mhsr_mess_grid", R.mat(ref), R.geom(g), R.mat(values)))
        got, got_mod = R.values(out[0]), R.values(out[1])
        assert got.dtype == np.float64 and got_mod.dtype == np.int32
        assert np.array_equal(got.reshape(g.nrow, g.ncol), want, equal_nan=True)
        assert np.array_equal(got_mod.reshape(g.nrow, g.ncol), want_mod)
    monkeypatch.delenv("MHS_HOST_BANDS")
    # a refusal of the library comes back as an R error: a table that does not fit the stack, a table with an NA
    with pytest.raises(RuntimeError, match="two more"):
        R.call("mhsr_mess_grid", R.mat(ref[:, :2]), R.geom(g), R.mat(values))
    bad = ref.copy(); bad[7, 1] = np.nan
    with pytest.raises(RuntimeError, match="row 7 of variable 1"):
        R.call("mhsr_mess_grid", R.mat(bad), R.geom(g), R.mat(values))
