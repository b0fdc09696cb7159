"""CPU: the extended-precision predictSE.Krig reference (tests/se_ref.py) agrees with itself -- the literal formula and
the quadratic form -rho z'M^-1 z are the same number for rho = sigma^2 / lambda -- and the standard-error entry points
refuse to run before mhs_init."""
import ctypes

import numpy as np
import pytest

import se_ref
from conftest import synth_stations
from oracle import tps as otps


@pytest.mark.parametrize("n,reps,lam", [(12, 0, 3e-3), (40, 6, 1e-2), (60, 0, None)])
def test_reference_forms_agree(n, reps, lam):
    xy, y = synth_stations(n, 7 + n)
    if reps:
        rng = np.random.default_rng(n)
        pick = rng.choice(n, reps, replace=False)
        xy = np.vstack([xy, xy[pick]])
        y = np.concatenate([y, y[pick] + 0.1 * rng.standard_normal(reps)])
    if lam is None:
        lam = otps.fit(xy, y)["lambda"]
    ref = se_ref.for_fit(xy, y, lam)
    p = ref.problem
    s2 = float(ref.sigma2(p["yM"], p["N"], p["pure_ss"]))
    assert s2 > 0
    rng = np.random.default_rng(1)
    lo, hi = xy.min(0), xy.max(0)
    pts = np.vstack([lo + (hi - lo) * rng.random((200, 2)), xy[:5]])
    vq = ref.var_quadratic(pts, s2)
    vl = ref.var_literal(pts, s2)
    assert np.all(vq > 0)
    assert float(np.max(np.abs(vq - vl) / np.abs(vl))) <= 1e-12
    # the oracle's float64 fit at the same lambda has the same residuals and effective degrees of freedom
    f = otps.fit(xy, y, lam=lam)
    fhat = otps.predict_points(f, f["xM"])
    rss = np.sum(f["weightsM"] * (f["yM"] - fhat) ** 2)
    s2_f64 = (rss + f["pure_ss"]) / (f["N"] - f["eff_df"])
    assert abs(s2_f64 - s2) <= 1e-8 * s2


def test_se_entry_points_refuse_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from machisplin_amd import _lib
    lib = _lib.load()
    a = np.zeros(64)
    out = ctypes.c_double()
    g = _lib.Grid(0.0, 1.0, 0.1, 0.1, 4, 4)
    assert lib.mhs_tps_sigma2(None, ctypes.byref(out)) == _lib.ERR_NODEVICE
    assert lib.mhs_tps_predict_se_points(None, a.ctypes.data, 4, float("nan"), a.ctypes.data) == _lib.ERR_NODEVICE
    assert lib.mhs_tps_predict_se_grid_dev(None, ctypes.byref(g), 0, 4, 0, 4, float("nan"), a.ctypes.data, 4,
                                           None) == _lib.ERR_NODEVICE
    nt = (ctypes.c_int64 * 2)()
    assert lib.mhs_tps_surface_se_dev(ctypes.byref(g), a.ctypes.data, a.ctypes.data, 12, None, 0, float("nan"), 0,
                                      a.ctypes.data, 4, nt, None) == _lib.ERR_NODEVICE
