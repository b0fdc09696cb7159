"""GPU: the standard-error entries of the R .Call() shim (mhsr_tps_sigma2, mhsr_tps_predict_se_points,
mhsr_tps_predict_se_grid, mhsr_tps_surface_se), executed through the stand-in R runtime of tests/rstub, equal the
direct C-ABI calls bit for bit."""
import numpy as np
import pytest

from test_r_shim_exec import R  # noqa: F401  (the shim + stub runtime fixture)

pytestmark = pytest.mark.gpu


def test_shim_se_entries_equal_the_direct_c_abi_calls_bit_for_bit(R, hip):  # noqa: F811
    from machisplin_amd import synth
    R.call("mhsr_init", R.int([0]))
    g = synth.grid(120, 150)
    xy, rows, cols, uv = synth.stations(g, 260, 41)
    resid = synth.tps_residual(uv, 41)
    fit = hip.Tps(xy, resid)
    t = R.call("mhsr_tps_fit", R.mat(xy), R.num(resid), R.num([R.NA]), R.int([0]))
    assert R.values(R.call("mhsr_tps_sigma2", t))[0] == fit.sigma2
    pts = xy[:40] + 0.3 * g.xres
    assert np.array_equal(R.values(R.call("mhsr_tps_predict_se_points", t, R.mat(pts), R.num([R.NA]))), fit.predict_se(pts))
    assert np.array_equal(R.values(R.call("mhsr_tps_predict_se_points", t, R.mat(pts), R.num([0.25]))),
                          fit.predict_se(pts, sigma2=0.25))
    got = R.values(R.call("mhsr_tps_predict_se_grid", t, R.geom(g), R.int([0, g.nrow, 0, g.ncol]), R.num([R.NA])))
    assert np.array_equal(got.reshape(g.nrow, g.ncol), hip.interpolate_se(g, fit).cpu().numpy())
    for te in (60, 0):
        got = R.values(R.call("mhsr_tps_surface_se", R.geom(g), R.mat(xy), R.num(resid), R.NULL, R.int([te]),
                              R.num([R.NA]), R.int([0])))
        want = hip.mltps.tps_residual_surface_se(g, xy, resid, tile_edge=te or None).cpu().numpy()
        assert np.array_equal(got.reshape(g.nrow, g.ncol), want, equal_nan=True)
