"""CPU: pin the TPS oracle against the committed golden vectors, against scipy's
independent RBF implementation, and against the analytic known-answer cases of
SURVEY.md section 8c (G1-G4).  (The reference has no tests of its own: parity unpinned.)"""
import glob
import os

import numpy as np
import pytest
from scipy.interpolate import RBFInterpolator

from oracle import tps

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLD, "tps_*.npz"))))
def test_oracle_reproduces_golden(path):
    z = np.load(path)
    m = tps.fit(z["xy"], z["y"], lam=float(z["lam"]))
    assert np.allclose(m["c"], z["c"], rtol=0, atol=1e-9 * np.abs(z["c"]).max())
    assert np.allclose(m["d"], z["d"], rtol=0, atol=1e-9 * np.abs(z["d"]).max())
    xmin, ymax, res, nrow, ncol = z["geom"]
    surf = tps.predict_grid(m, xmin, ymax, res, res, int(nrow), int(ncol))
    scale = np.abs(z["surf"]).max()
    assert np.abs(surf - z["surf"]).max() < 1e-10 * scale
    assert np.abs(surf - z["surf_scipy"]).max() < 1e-10 * scale  # independent implementation
    mg = tps.fit(z["xy"], z["y"])
    assert abs(mg["lambda"] - float(z["lam_gcv_fields"])) < 1e-8 * float(z["lam_gcv_fields"])
    mc = tps.fit(z["xy"], z["y"], gcv_mode="converged")
    assert abs(mc["lambda"] - float(z["lam_gcv_converged"])) < 1e-6 * float(z["lam_gcv_converged"])
    assert mc["gcv"] <= mg["gcv"] * (1 + 1e-12)  # the converged search is at least as low


def test_eigen_route_equals_direct_saddle_point_and_scipy():
    rng = np.random.default_rng(3)
    xy = rng.uniform(0, 5, (300, 2))
    y = np.cos(xy[:, 0]) + 0.05 * rng.standard_normal(300)
    m = tps.fit(xy, y)
    md = tps.fit_direct(xy, y, m["lambda"])
    assert np.abs(m["c"] - md["c"]).max() < 1e-10 * np.abs(m["c"]).max()
    assert np.abs(m["d"] - md["d"]).max() < 1e-10 * np.abs(m["d"]).max()
    pts = rng.uniform(0, 5, (1000, 2))
    rb = RBFInterpolator(m["knots"], y, kernel="thin_plate_spline", degree=1, smoothing=8 * np.pi * m["lambda"])
    ref = rb((pts - m["center"]) / m["scale"])
    assert np.abs(tps.predict_points(m, pts) - ref).max() < 1e-11 * np.abs(ref).max()
    assert np.abs(np.column_stack([np.ones(300), m["knots"]]).T @ m["c"]).max() < 1e-9  # T'c = 0


def test_linear_data_gives_plane():
    rng = np.random.default_rng(4)
    xy = rng.uniform(-1, 1, (60, 2))
    y = 1.0 + 2.0 * xy[:, 0] - 3.0 * xy[:, 1]
    m = tps.fit(xy, y, lam=1e-2)
    assert np.abs(m["c"]).max() < 1e-10
    pts = rng.uniform(-1, 1, (50, 2))
    assert np.abs(tps.predict_points(m, pts) - (1 + 2 * pts[:, 0] - 3 * pts[:, 1])).max() < 1e-10


def test_lambda_limits():
    rng = np.random.default_rng(5)
    xy = rng.uniform(0, 1, (80, 2))
    y = np.sin(4 * xy[:, 0]) + xy[:, 1] ** 2
    m0 = tps.fit(xy, y, lam=1e-12)
    assert np.abs(tps.predict_points(m0, xy) - y).max() < 1e-6  # interpolation
    minf = tps.fit(xy, y, lam=1e12)
    A = np.column_stack([np.ones(80), xy])
    plane = A @ np.linalg.lstsq(A, y, rcond=None)[0]
    assert np.abs(tps.predict_points(minf, xy) - plane).max() < 1e-6  # least-squares plane


def test_replicates_collapse_to_weighted_problem():
    rng = np.random.default_rng(6)
    xy = rng.uniform(0, 1, (50, 2))
    y = rng.standard_normal(50)
    xy2 = np.vstack([xy, xy[:4]])
    y2 = np.concatenate([y, y[:4] + 1.0])
    m = tps.fit(xy2, y2, lam=1e-2)
    assert m["knots"].shape == (50, 2) and m["N"] == 54
    assert np.allclose(m["weightsM"][:4], 2.0) and np.allclose(m["weightsM"][4:], 1.0)
    assert np.isclose(m["pure_ss"], 4 * 2 * 0.25)
    md = tps.fit_direct(xy2, y2, 1e-2)
    assert np.abs(m["c"] - md["c"]).max() < 1e-10 * np.abs(m["c"]).max()


def test_degenerate_inputs():
    x = np.linspace(0, 1, 20)
    with pytest.raises(ValueError):
        tps.fit(np.column_stack([x, x]), x)
    with pytest.raises(ValueError):
        tps.fit(np.array([[0, 0], [1, 0], [0, 1.0]]), np.arange(3.0))


def test_phi_floor_and_grid_convention():
    assert tps.radial_phi(np.array([0.0]))[0] == tps.radial_phi(np.array([1e-20]))[0]
    x, y = tps.cell_centres(-78.0, -5.0, 0.5, 0.25, 4, 3)
    assert np.allclose(x, [-77.75, -77.25, -76.75]) and np.allclose(y, [-5.125, -5.375, -5.625, -5.875])


# --- the extended-precision reference of the fixed-lambda system (refined_solution / backward_error) ---------------

def _saddle64(u, w, lam):
    n = u.shape[0]
    A = np.zeros((n + 3, n + 3))
    A[:n, :n] = tps.gram(u) + lam * np.diag(1.0 / w)
    A[:n, n:] = np.column_stack([np.ones(n), u])
    A[n:, :n] = A[:n, n:].T
    return A


def _manufactured(lam, seed, n=150, nrep=40):
    """Stations with `nrep` locations observed twice, and y = A x* for a chosen x* = (c*, d*), T'c* = 0, formed in long
    double and rounded to float64.  Returns xy, y, x*, and the exact solution for the rounded y (x* plus a float64
    correction far below the long-double error bound)."""
    rng = np.random.default_rng(seed)
    xy = np.column_stack([rng.uniform(-78, -76, n), rng.uniform(-7, -5, n)])
    center, scale = tps.range_scale(xy)
    u = (xy - center) / scale
    w = np.ones(n)
    w[:nrep] = 2.0
    T = np.column_stack([np.ones(n), u]).astype(np.longdouble)
    c = rng.standard_normal(n).astype(np.longdouble)
    for _ in range(2):   # project out the plane twice: T'c* = 0 to long-double rounding
        g = np.linalg.solve((T.T @ T).astype(np.float64), (T.T @ c).astype(np.float64))
        c = c - T @ g.astype(np.longdouble)
    x = np.concatenate([c, np.array([0.5, -1.25, 2.0], dtype=np.longdouble)])
    lam_w = np.longdouble(lam) / w.astype(np.longdouble)
    b = tps._saddle_apply_ld(u, lam_w, x)[0][:n]
    b64 = b.astype(np.float64)
    xy2 = np.vstack([xy, xy[:nrep]])
    y2 = np.concatenate([b64, b64[:nrep]])
    A = _saddle64(u, w, lam)
    dx = np.linalg.solve(A, np.concatenate([(b64.astype(np.longdouble) - b).astype(np.float64), np.zeros(3)]))
    return xy2, y2, x, x + dx.astype(np.longdouble), np.linalg.cond(A, np.inf), np.abs(dx).max()


@pytest.mark.parametrize("lam", [0.0, 1e-6, 1.0])
def test_refined_solution_recovers_a_manufactured_solution(lam):
    xy, y, xstar, xtrue, kappa, dxn = _manufactured(lam, 11 + int(lam * 7))
    ref = tps.refined_solution(xy, y, lam)
    assert ref["knots"].shape == (150, 2) and np.array_equal(ref["w"][:40], np.full(40, 2.0))
    assert ref["c"].dtype == np.longdouble and ref["d"].dtype == np.longdouble
    x = np.concatenate([ref["c"], ref["d"]])
    err = float(np.abs(x - xtrue).max())
    xn = float(np.abs(xstar).max())
    # long-double accuracy (kappa 2^-63) plus the float64 error of the correction for the rounding of y
    bound = 8 * kappa * 2.0 ** -63 * xn + 8 * kappa * 2.0 ** -53 * dxn
    assert err <= bound, (err, bound, kappa)
    # and far more accurate than the float64 solve once the system is ill-conditioned
    fd = tps.fit_direct(xy, y, lam)
    err64 = float(np.abs(np.concatenate([fd["c"], fd["d"]]) - xtrue).max())
    if kappa > 1e6:
        assert err < 1e-3 * err64, (err, err64, kappa)


@pytest.mark.parametrize("n,lam", [(300, 1e-3), (260, 1e-8)])
def test_refined_solution_agrees_with_fit_and_fit_direct(n, lam):
    from conftest import synth_stations
    xy, y = synth_stations(n, 40 + n)
    xy = np.vstack([xy, xy[:25]])
    y = np.concatenate([y, y[:25] + 0.1])
    ref = tps.refined_solution(xy, y, lam)
    x = np.concatenate([ref["c"], ref["d"]]).astype(np.float64)
    u, w = ref["knots"], ref["w"]
    kappa = np.linalg.cond(_saddle64(u, w, lam), np.inf)
    for m in (tps.fit(xy, y, lam=lam), tps.fit_direct(xy, y, lam)):
        assert np.array_equal(m["knots"], u) and np.array_equal(m["center"], ref["center"])
        assert np.array_equal(m["scale"], ref["scale"])
        err = np.abs(np.concatenate([m["c"], m["d"]]) - x).max()
        assert err <= 4 * kappa * 2.0 ** -53 * np.abs(x).max(), (err, kappa)


def test_backward_error_separates_long_double_from_float64():
    from conftest import synth_stations
    xy, y = synth_stations(400, 77)
    for lam in (0.0, 1e-3):
        ref = tps.refined_solution(xy, y, lam)
        comp, norm = tps.backward_error(xy, y, lam, ref["c"], ref["d"])
        assert comp < 2.0 ** -58 and norm <= comp                         # the long-double floor
        fd = tps.fit_direct(xy, y, lam)
        comp64, norm64 = tps.backward_error(xy, y, lam, fd["c"], fd["d"])
        assert 2.0 ** -58 < comp64 < 2.0 ** -45 and norm64 <= comp64      # float64 rounding, visible and small
        # one coefficient off by one part in 1e11 shows
        c = fd["c"].copy()
        c[7] *= 1 + 1e-11
        assert tps.backward_error(xy, y, lam, c, fd["d"])[0] > 10 * comp64


def test_refined_solution_of_an_exact_plane_has_zero_c():
    # dyadic stations spanning [0, 1] x [0, 1]: the knots equal the stations exactly and y is exactly a plane in them
    rng = np.random.default_rng(8)
    cells = rng.choice(65 * 65, size=200, replace=False)
    xy = np.column_stack([cells // 65, cells % 65]) / 64.0
    xy = np.vstack([xy, [[0, 0], [1, 1]]])
    y = 1.0 + 2.0 * xy[:, 0] - 3.0 * xy[:, 1]
    ref = tps.refined_solution(xy, y, 1e-2)
    assert np.array_equal(ref["knots"], xy)
    # zero to long-double rounding (the float64 solve leaves c at ~1e-12 here)
    assert np.abs(ref["c"]).max() < 1e-16
    assert np.abs(ref["d"] - np.array([1.0, 2.0, -3.0], dtype=np.longdouble)).max() < 1e-17


def test_radial_phi_long_double():
    d2 = np.array([0.0, 1e-30, 1e-20, 0.25, 1.0, 2.0], dtype=np.longdouble)
    p = tps._phi_ld(d2)
    assert p[0] == 0 and p[1] == p[2] and p[4] == 0
    assert abs(float(p[3]) - tps.radial_phi(np.array([0.25]))[0]) < 1e-17
    assert abs(tps.PI_LD - np.longdouble("3.14159265358979323846264338327950288")) < 1e-19
