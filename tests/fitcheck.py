"""Accuracy criteria for a fitted spline's coefficients against the extended-precision reference of its fixed-lambda
system (oracle.tps.refined_solution), shared by the GPU fit tests.

  B (backward error):  the componentwise backward error of (c, d), residual in long double, is at most TAU_B[route].
  F (forward error):   ||x_gpu - x*||_inf <= F_MAX[route] * max(||x_lapack - x*||_inf, 8 eps ||x*||_inf),
                       x* the refined solution, x_lapack fields' system solved by LAPACK in float64 (fit_direct).

F scales with the conditioning of the system: a fit is held to what a float64 solve achieves on the same problem, and
never to less than a few ulps of the coefficients.  Both thresholds are per route and were set from measurements on the
MI355X (largest value seen per route, times at most 10; see TAU_B below)."""
import hashlib

import numpy as np

from oracle import tps as otps

EPS = 2.0 ** -53

# Largest value measured per route on the MI355X over this suite's cases (in brackets), times at most 10.
# B sits at 1e-14 .. 9e-14 on every route, against 1e-16 for LAPACK on the same system: the device builds K with a table
# log good to ~2e-14 absolute per entry (devmath.h), a perturbation of A 100x larger than float64 rounding.  For the
# same reason F lands at 50 .. 1 600 on every route, GCV ones included -- not a property of one solver.  A wrong update
# (a skipped tile, a missing diagonal shift) moves B to 1e-5 .. 1e-2.
TAU_B = {
    "chol": 5e-13,        # [8.9e-14] fixed lambda: MFMA Cholesky of Q2'KQ2 + lambda I (tps_chol.hip)
    "gcv-tri": 4e-13,     # [4.5e-14] GCV, m <= 256: single-block tridiagonalisation
    "gcv-band8": 2.5e-13,  # [2.6e-14] GCV, 8-column band reduction
    "gcv-band32": 1.5e-13,  # [1.7e-14] GCV, 32-column band reduction
    "batch": 5e-13,       # [9.6e-14] fit_many: a workgroup per spline
}
F_MAX = {
    "chol": 2500.0,       # [524]
    "gcv-tri": 2500.0,    # [431]
    "gcv-band8": 1500.0,  # [211]
    "gcv-band32": 1500.0,  # [163]
    "batch": 2500.0,      # [1 579]
}

_REF = {}


def _key(xy, y, lam):
    h = hashlib.sha1(np.ascontiguousarray(xy, dtype=np.float64).tobytes())
    h.update(np.ascontiguousarray(y, dtype=np.float64).tobytes())
    return h.hexdigest(), float(lam)


def reference(xy, y, lam):
    """(refined solution, float64 LAPACK solution) of the stations' system at lam, cached for the session."""
    k = _key(xy, y, lam)
    if k not in _REF:
        _REF[k] = (otps.refined_solution(xy, y, lam), otps.fit_direct(xy, y, lam))
    return _REF[k]


def gcv_route(n_distinct):
    m = n_distinct - 3
    return "gcv-tri" if m <= 256 else ("gcv-band8" if m < 320 else "gcv-band32")


def measure(xy, y, lam, got):
    """(componentwise backward error, forward-error ratio of criterion F) of a fit `got` (c, d attributes)."""
    ref, lap = reference(xy, y, lam)
    xs = np.concatenate([ref["c"], ref["d"]])
    xg = np.concatenate([got.c, got.d]).astype(np.longdouble)
    xl = np.concatenate([lap["c"], lap["d"]]).astype(np.longdouble)
    be = otps.backward_error(xy, y, lam, got.c, got.d)[0]
    floor = max(float(np.abs(xl - xs).max()), 8 * EPS * float(np.abs(xs).max()))
    return be, float(np.abs(xg - xs).max()) / floor


def check(route, xy, y, lam, got, label=""):
    """Identity of the knots / transform with the oracle's, finite coefficients, then criteria B and F.
    Returns (backward error, F ratio); prints them for the record."""
    ref, _ = reference(xy, y, lam)
    assert np.array_equal(got.knots, ref["knots"]), label
    assert np.array_equal(got.center, ref["center"]) and np.array_equal(got.scale, ref["scale"]), label
    assert np.isfinite(got.c).all() and np.isfinite(got.d).all(), label
    be, fr = measure(xy, y, lam, got)
    print(f"CRITERIA route={route} n={got.n} lambda={lam:.6g} B={be:.3e} F={fr:.3f} {label}")
    assert be <= TAU_B[route], (route, label, be)
    assert fr <= F_MAX[route], (route, label, fr)
    return be, fr
