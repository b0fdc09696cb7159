"""GPU: Q = -M^-1 of the TPS standard errors built on the device (mhs_tps_se_build_mode / mhs_tps_se_max_n) -- against
the extended-precision reference of tests/se_ref.py at every panel edge of the blocked inverse, for a from_coef handle,
bit for bit from build to build, past the host build's limit of 2 048 stations, and on the tiled surface."""
import numpy as np
import pytest

import se_ref
from conftest import synth_stations
from oracle import tps as otps

pytestmark = pytest.mark.gpu

# |v_gpu - v_ref| <= TAU_DEV * rho |z|'|M^-1||z| with Q built on the device: the largest ratio measured on the MI355X over
# the cases below, times at most 10 (summation order and box differences, as for TAU in test_tps_se_gpu.py)
TAU_DEV = 5e-14   # [5.9e-15, n = 12; the host build of the same spline: 6.0e-15]


@pytest.fixture(autouse=True)
def _restore_settings(hip):
    yield
    hip.se_build_mode(hip.SE_BUILD_AUTO)
    hip.se_max_n(2048)


def _with_replicates(xy, y, k, seed):
    rng = np.random.default_rng(seed)
    pick = rng.choice(xy.shape[0], k, replace=False)
    return np.vstack([xy, xy[pick]]), np.concatenate([y, y[pick] + 0.05 * rng.standard_normal(k)])


def _points(xy, m, seed):
    rng = np.random.default_rng(seed)
    lo, hi = xy.min(0), xy.max(0)
    span = hi - lo
    return np.vstack([lo - 0.05 * span + 1.1 * span * rng.random((m, 2)), xy[:7]])


def _grid(hip, xy):
    lo, hi = xy.min(0), xy.max(0)
    g = hip.Geometry(lo[0], hi[1], (hi[0] - lo[0]) / 37, (hi[1] - lo[1]) / 29, 29, 37)
    gx = g.xmin + (np.arange(2, 37) + 0.5) * g.xres
    gy = g.ymax - (np.arange(3, 29) + 0.5) * g.yres
    X, Y = np.meshgrid(gx, gy)
    return g, (3, 29, 2, 37), np.column_stack([X.ravel(), Y.ravel()])      # a 26 x 35 window


def _ratios(hip, ref, fit, s2, pts, g, win, cells):
    """Largest |v - v_ref| / bound and largest relative SE error over the points and the grid window."""
    se = np.concatenate([fit.predict_se(pts, sigma2=s2), hip.interpolate_se(g, fit, window=win, sigma2=s2).cpu().numpy().ravel()])
    allp = np.vstack([pts, cells])
    v_ref = ref.var_quadratic(allp, s2)
    ratio = float(np.max(np.abs(se.astype(np.longdouble) ** 2 - v_ref) / ref.bound(allp, s2)))
    sr = np.sqrt(v_ref.astype(np.float64))
    return ratio, float(np.max(np.abs(se - sr) / sr))


CASES = [(12, 3e-3, 0),      # m = 9, inside one padded panel
         (13, 3e-3, 0),      # n + 3 = 16: no Q padding
         (131, 3e-3, 0),     # m = 128, exactly one panel
         (132, 3e-3, 0),     # m = 129: two panels, 127 padded rows
         (200, None, 20),    # GCV, 20 replicates: weights != 1
         (290, None, 0),     # GCV, the band8 route
         (390, 3e-3, 0)]     # m = 387: four panels


@pytest.mark.parametrize("n,lam,reps", CASES)
def test_device_built_se_against_reference(hip, n, lam, reps):
    xy, y = synth_stations(n, 100 + n)
    if reps:
        xy, y = _with_replicates(xy, y, reps, reps)
    hip.se_build_mode(hip.SE_BUILD_DEVICE)
    fit = hip.Tps(xy, y, lambda_=lam)
    ref = se_ref.for_fit(xy, y, fit.lambda_)
    p = ref.problem
    s2_ref = float(ref.sigma2(p["yM"], p["N"], p["pure_ss"]))
    s2 = fit.sigma2
    assert fit.se_info()["built_on"] == hip.SE_BUILD_DEVICE
    assert fit.se_info()["q_bytes"] == 8 * ((fit.n + 3 + 15) // 16 * 16) ** 2
    pts = _points(xy, 300, 3)
    g, win, cells = _grid(hip, xy)
    ratio, rel = _ratios(hip, ref, fit, s2, pts, g, win, cells)
    # the host build of the same spline, for comparison only (same lambda: a fixed-lambda fit at the device handle's)
    hip.se_build_mode(hip.SE_BUILD_HOST)
    host = hip.Tps(xy, y, lambda_=fit.lambda_)
    s2_host = host.sigma2
    assert host.se_info()["built_on"] == hip.SE_BUILD_HOST
    ratio_h, rel_h = _ratios(hip, ref, host, s2, pts, g, win, cells)
    print(f"SE-DEV n={fit.n} reps={reps} lambda={fit.lambda_:.4g} sigma2={s2:.6g} (ref {s2_ref:.6g}, host {s2_host:.6g}) "
          f"ratio device={ratio:.3e} host={ratio_h:.3e} se_rel device={rel:.3e} host={rel_h:.3e} "
          f"build_ms device={fit.se_info()['build_ms']:.2f} host={host.se_info()['build_ms']:.2f}")
    assert abs(s2 - s2_ref) <= 1e-10 * s2_ref, (s2, s2_ref)
    assert ratio <= TAU_DEV, (ratio, ratio_h)
    assert rel <= 1e-6, rel


def test_from_coef_handle_on_the_device(hip):
    hip.se_build_mode(hip.SE_BUILD_DEVICE)
    xs, ys = synth_stations(30, 2)
    f = hip.Tps(xs, ys, lambda_=1e-2)
    fc = hip.Tps.from_coef(f.knots, f.c, f.d, f.lambda_, f.center, f.scale)
    pts = _points(xs, 50, 1)
    a, b = fc.predict_se(pts, sigma2=0.5), f.predict_se(pts, sigma2=0.5)
    assert fc.se_info()["built_on"] == hip.SE_BUILD_DEVICE and f.se_info()["built_on"] == hip.SE_BUILD_DEVICE
    np.testing.assert_allclose(a, b, rtol=1e-12)
    # a larger one, two panels
    xs, ys = synth_stations(150, 3)
    f = hip.Tps(xs, ys, lambda_=2e-3)
    fc = hip.Tps.from_coef(f.knots, f.c, f.d, f.lambda_, f.center, f.scale)
    pts = _points(xs, 50, 1)
    np.testing.assert_allclose(fc.predict_se(pts, sigma2=0.5), f.predict_se(pts, sigma2=0.5), rtol=1e-12)


def test_device_build_is_deterministic_and_data_independent(hip):
    hip.se_build_mode(hip.SE_BUILD_DEVICE)
    xy, y = synth_stations(300, 400)         # m = 297: three panels
    pts = _points(xy, 500, 9)
    g = hip.Geometry(-78.0, -5.0, 0.01, 0.01, 40, 50)
    s2 = 0.37
    a = hip.Tps(xy, y, lambda_=2e-3)
    b = hip.Tps(xy, y, lambda_=2e-3)
    c = hip.Tps(xy, np.cos(3 * y) + 0.3, lambda_=2e-3)
    pa, ga = a.predict_se(pts, sigma2=s2), hip.interpolate_se(g, a, sigma2=s2).cpu().numpy()
    assert a.se_info()["built_on"] == hip.SE_BUILD_DEVICE
    # two fresh handles on the same data: the same Q bit for bit (and the same sigma^2 hat)
    assert a.sigma2 == b.sigma2
    assert np.array_equal(pa, b.predict_se(pts, sigma2=s2))
    assert np.array_equal(ga, hip.interpolate_se(g, b, sigma2=s2).cpu().numpy())
    assert np.array_equal(a.predict_se(pts), b.predict_se(pts))
    # Q does not depend on the responses
    assert np.array_equal(pa, c.predict_se(pts, sigma2=s2))
    assert np.array_equal(ga, hip.interpolate_se(g, c, sigma2=s2).cpu().numpy())
    assert np.isfinite(pa).all() and (pa > 0).all()


def test_past_the_old_limit(hip):
    xy, y = synth_stations(2100, 5)
    fit = hip.Tps(xy, y)
    # nothing set: today's refusal
    with pytest.raises(hip.MhsError) as ei:
        fit.predict_se(xy[:3])
    assert ei.value.code == hip._lib.ERR_INVALID and "2048" in str(ei.value)
    with pytest.raises(hip.MhsError):
        fit.se_info()                       # no Q yet
    assert hip.se_max_n(4096) == 2048       # AUTO: above 2 048 stations the device builds
    xm, _, w, _ = otps.collapse_replicates(xy, y)
    pts = _points(xy, 300, 3)
    se_k, se_p = fit.predict_se(xm), fit.predict_se(pts)
    info = fit.se_info()
    assert info["built_on"] == hip.SE_BUILD_DEVICE and info["q_bytes"] == 8 * 2112 ** 2
    for se in (se_k, se_p):
        assert np.isfinite(se).all() and (se >= 0).all()
    # w_j var(u_j) / sigma^2 = A_jj, the hat diagonal: the knots' SEs sum to the effective degrees of freedom
    edf = float(np.sum(w * se_k ** 2) / fit.sigma2)
    print(f"SE-DEV n={fit.n} lambda={fit.lambda_:.4g} eff_df={fit.eff_df:.6f} sum w se^2 / sigma2={edf:.6f} "
          f"rel={abs(edf - fit.eff_df) / fit.eff_df:.3e} build_ms={info['build_ms']:.1f}")
    assert abs(edf - fit.eff_df) <= 1e-7 * fit.eff_df
    # the host build of the same spline
    hip.se_build_mode(hip.SE_BUILD_HOST)
    host = hip.Tps(xy, y, lambda_=fit.lambda_)
    hk, hp = host.predict_se(xm, sigma2=fit.sigma2), host.predict_se(pts, sigma2=fit.sigma2)
    assert host.se_info()["built_on"] == hip.SE_BUILD_HOST
    got, want = np.concatenate([se_k, se_p]), np.concatenate([hk, hp])
    print(f"SE-DEV n={fit.n} device vs host max rel {np.max(np.abs(got - want) / want):.3e} host build_ms={host.se_info()['build_ms']:.1f}")
    assert np.max(np.abs(got - want) / want) <= 1e-6
    # a limit below the handle's size refuses a NEW build and names itself; the handle that has its Q keeps it
    hip.se_max_n(2099)
    with pytest.raises(hip.MhsError) as ei:
        hip.Tps(xy, y, lambda_=fit.lambda_).predict_se(xy[:3])
    assert ei.value.code == hip._lib.ERR_INVALID and "2099" in str(ei.value)
    assert np.array_equal(fit.predict_se(pts), se_p)


def test_tiled_surface_under_device_builds(hip):
    # the smallest multi-tile geometry of test_tps_se_surface_gpu.py (one tile without a spline)
    from test_tps_se_surface_gpu import _stations
    g = hip.Geometry(-78.0, -5.0, 1.0 / 120, 1.0 / 120, 240, 240)
    xy, y = _stations(g, 500, 12, empty_box=(0, 100, 0, 100))
    default = hip.mltps.tps_residual_surface_se(g, xy, y, tile_edge=80).cpu().numpy()
    hip.se_build_mode(hip.SE_BUILD_DEVICE)
    dev = hip.mltps.tps_residual_surface_se(g, xy, y, tile_edge=80).cpu().numpy()
    nan = np.isnan(default)
    assert nan.any() and not nan.all()
    assert np.array_equal(np.isnan(dev), nan)
    rel = np.abs(dev[~nan] - default[~nan]) / default[~nan]
    print(f"SE-DEV tiled surface max rel {rel.max():.3e}")
    assert rel.max() <= 1e-6
