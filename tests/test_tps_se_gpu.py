"""GPU: prediction standard errors (fields::predictSE.Krig) of HIP splines -- points and grids -- against the
extended-precision reference of tests/se_ref.py, at the handle's own lambda and sigma^2 hat, on every fit route."""
import os

import numpy as np
import pytest

import se_ref
from conftest import synth_stations

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# |v_gpu - v_ref| <= TAU * rho |z|'|M^-1||z|: the largest ratio measured on the MI355X over these cases, times at most 10
TAU = 6e-14   # [6.0e-15, n = 12]


def _stations(name):
    if name.startswith("synth"):
        n = int(name[5:])
        return synth_stations(n, 100 + n)
    d = np.load(os.path.join(GOLDEN, f"tps_{name}.npz"))
    return d["xy"], d["y"]


def _with_replicates(xy, y, k, seed):
    rng = np.random.default_rng(seed)
    pick = rng.choice(xy.shape[0], k, replace=False)
    return np.vstack([xy, xy[pick]]), np.concatenate([y, y[pick] + 0.05 * rng.standard_normal(k)])


def _points(xy, m, seed):
    rng = np.random.default_rng(seed)
    lo, hi = xy.min(0), xy.max(0)
    span = hi - lo
    return np.vstack([lo - 0.05 * span + 1.1 * span * rng.random((m, 2)), xy[:7]])


def _check(hip, label, xy, y, fit, geom_cells=True):
    ref = se_ref.for_fit(xy, y, fit.lambda_)
    p = ref.problem
    s2_ref = float(ref.sigma2(p["yM"], p["N"], p["pure_ss"]))
    s2 = fit.sigma2
    assert abs(s2 - s2_ref) <= 1e-10 * s2_ref, (label, s2, s2_ref)
    pts = _points(xy, 300, 3)
    se = fit.predict_se(pts)
    v_ref = ref.var_quadratic(pts, s2)
    bound = ref.bound(pts, s2)
    ratio = float(np.max(np.abs(se.astype(np.longdouble) ** 2 - v_ref) / bound))
    rel = float(np.max(np.abs(se - np.sqrt(v_ref.astype(np.float64))) / np.sqrt(v_ref.astype(np.float64))))
    out = [ratio]
    if geom_cells:
        lo, hi = xy.min(0), xy.max(0)
        g = hip.Geometry(lo[0], hi[1], (hi[0] - lo[0]) / 37, (hi[1] - lo[1]) / 29, 29, 37)
        plane = hip.interpolate_se(g, fit, window=(3, 29, 2, 37)).cpu().numpy()
        gx = g.xmin + (np.arange(2, 37) + 0.5) * g.xres
        gy = g.ymax - (np.arange(3, 29) + 0.5) * g.yres
        X, Y = np.meshgrid(gx, gy)
        cells = np.column_stack([X.ravel(), Y.ravel()])
        vg = ref.var_quadratic(cells, s2)
        out.append(float(np.max(np.abs(plane.ravel().astype(np.longdouble) ** 2 - vg) / ref.bound(cells, s2))))
        rel = max(rel, float(np.max(np.abs(plane.ravel() - np.sqrt(vg.astype(np.float64))) / np.sqrt(vg.astype(np.float64)))))
        # the grid at the cell centres is the points call on those centres, to rounding
        pt = fit.predict_se(cells)
        assert np.max(np.abs(pt - plane.ravel()) / pt) < 1e-12, label
    print(f"SE {label} n={fit.n} lambda={fit.lambda_:.4g} sigma2={s2:.4g} ratio={max(out):.3e} se_rel={rel:.3e}")
    assert max(out) <= TAU, (label, out)
    assert rel <= 1e-6, (label, rel)


@pytest.mark.parametrize("name,lam,reps", [("synth12", 3e-3, 0), ("synth200", 3e-3, 0), ("synth200", None, 0),
                                           ("synth200", None, 20), ("sampling813", None, 0), ("sampling813", 1e-3, 30),
                                           ("synth290", None, 0)])
def test_se_against_reference_mhs_tps_fit(hip, name, lam, reps):
    """chol (fixed lambda), tri (GCV, m <= 256), band8 (290) and band32 (813) routes of mhs_tps_fit."""
    xy, y = _stations(name)
    if reps:
        xy, y = _with_replicates(xy, y, reps, reps)
    fit = hip.Tps(xy, y, lambda_=lam)
    _check(hip, f"{name}/{'gcv' if lam is None else 'fixed'}/reps={reps}", xy, y, fit)


def test_se_against_reference_fit_many(hip):
    """The batch route (a workgroup per spline) keeps what the SE needs as well."""
    sets = [_stations("synth12"), _stations("synth200"), _with_replicates(*_stations("synth200"), 15, 4)]
    fits = hip.tps.fit_many([a for a, _ in sets], [b for _, b in sets])
    for k, ((xy, y), f) in enumerate(zip(sets, fits)):
        _check(hip, f"fit_many[{k}]", xy, y, f, geom_cells=(k == 1))


def test_se_exact_properties(hip):
    xy, y = _stations("synth200")
    a = hip.Tps(xy, y, lambda_=2e-3)
    b = hip.Tps(xy, np.cos(3 * y) + 0.3, lambda_=2e-3)
    pts = _points(xy, 500, 9)
    s2 = 0.37
    # Q = -M^-1 does not depend on the data: bit-identical SE for two response vectors at the same lambda and sigma^2
    assert np.array_equal(a.predict_se(pts, sigma2=s2), b.predict_se(pts, sigma2=s2))
    # the SE scales with sigma
    s1, s4 = a.predict_se(pts, sigma2=s2), a.predict_se(pts, sigma2=4 * s2)
    assert np.all(np.abs(s4 - 2 * s1) <= np.spacing(2 * s1))
    g = hip.Geometry(-78.0, -5.0, 0.01, 0.01, 40, 50)
    ga, gb = hip.interpolate_se(g, a, sigma2=s2), hip.interpolate_se(g, b, sigma2=s2)
    assert bool((ga == gb).all())


def test_se_refusals(hip):
    xy, y = synth_stations(2100, 5)
    big = hip.Tps(xy, y, lambda_=1e-3)
    with pytest.raises(hip.MhsError) as ei:
        big.predict_se(xy[:3])
    assert ei.value.code == hip._lib.ERR_INVALID and "2048" in str(ei.value)
    xs, ys = synth_stations(30, 2)
    f = hip.Tps(xs, ys, lambda_=1e-2)
    fc = hip.Tps.from_coef(f.knots, f.c, f.d, f.lambda_, f.center, f.scale)
    with pytest.raises(hip.MhsError) as ei:
        fc.predict_se(xs[:3])
    assert ei.value.code == hip._lib.ERR_INVALID
    with pytest.raises(hip.MhsError) as ei:
        fc.sigma2
    assert ei.value.code == hip._lib.ERR_INVALID
    # with sigma^2 given, a from_coef handle (unit weights) gives the fitted handle's SE (no replicates here)
    pts = _points(xs, 50, 1)
    np.testing.assert_allclose(fc.predict_se(pts, sigma2=0.5), f.predict_se(pts, sigma2=0.5), rtol=1e-12)
