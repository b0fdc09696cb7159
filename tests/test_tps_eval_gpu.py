"""GPU parity: HIP thin-plate-spline evaluation (through the C ABI) vs the oracle's
predict.Krig restatement, same coefficients, same cell centres."""
import numpy as np
import pytest

import devmath_ref as R
from conftest import synth_stations
from oracle import tps as otps
from test_devmath_host import r2logr2_bound

pytestmark = pytest.mark.gpu

# |sum_j c_j phi_j| suffers cancellation (sum|terms| / |sum| ~ 1e2..1e3), so the bound is
# stated against the magnitude of the surface: 1e-10 of max|f| (north-star asks 1e-6).
RTOL = 1e-10


def _check(hip, n, nrow, ncol, seed, window=None, lam=None):
    g = hip.Geometry(-78.0, -5.0, 1.0 / 1200, 1.0 / 1200, nrow, ncol)
    xy, y = synth_stations(n, seed, g if n <= nrow * ncol else None)
    m = otps.fit(xy, y, lam=lam)
    t = hip.Tps.from_coef(m["knots"], m["c"], m["d"], m["lambda"], m["center"], m["scale"])
    r0, r1, c0, c1 = window or (0, nrow, 0, ncol)
    got = hip.interpolate(g, t, window=window).cpu().numpy()
    want = otps.predict_grid(m, g.xmin, g.ymax, g.xres, g.yres, nrow, ncol, r0, r1, c0, c1)
    assert got.shape == want.shape
    err = np.abs(got - want).max() / np.abs(want).max()
    assert err < RTOL, err
    return m, t


@pytest.mark.parametrize("n,nrow,ncol", [(12, 5, 7), (200, 48, 64), (813, 130, 257), (64, 1, 1)])
def test_grid_matches_oracle(hip, n, nrow, ncol):
    _check(hip, n, nrow, ncol, seed=n)


def test_window_and_strided_output(hip):
    import torch
    g = hip.Geometry(-78.0, -5.0, 1.0 / 1200, 1.0 / 1200, 300, 400)
    xy, y = synth_stations(150, 3, g)
    m = otps.fit(xy, y)
    t = hip.Tps.from_coef(m["knots"], m["c"], m["d"], m["lambda"], m["center"], m["scale"])
    hip.eval_mode(hip.EVAL_DIRECT)   # the far-field path tiles from the window origin: equal to rounding only
    try:
        full = hip.interpolate(g, t)
        big = torch.full((300, 512), float("nan"), dtype=torch.float64, device=full.device)
        win = (17, 203, 33, 390)
        hip.interpolate(g, t, window=win, out=big[17:203, 33:390])
        torch.cuda.synchronize()
    finally:
        hip.eval_mode(hip.EVAL_AUTO)
    assert torch.equal(big[17:203, 33:390], full[17:203, 33:390])  # same cells, same bits
    assert torch.isnan(big[:, :33]).all() and torch.isnan(big[:17]).all()
    assert torch.isnan(big[:, 390:]).all() and torch.isnan(big[203:]).all()


@pytest.mark.parametrize("n,nrow,ncol,xres,yres,window", [
    (813, 400, 600, 1.0 / 1200, 1.0 / 1200, None),           # square cells, stations spread over the grid
    (500, 700, 300, 1.0 / 600, 1.0 / 1200, None),            # anisotropic cells and a tall grid
    (300, 500, 500, 1.0 / 1200, 1.0 / 1200, (40, 371, 100, 437)),   # window: most knots lie outside it
])
def test_far_field_path_equals_direct_sum(hip, n, nrow, ncol, xres, yres, window):
    """The far-field-interpolated evaluation (csrc/tps_eval.hip) against the direct sum of the same handle
    and against the oracle: equal to rounding, not merely to the 1e-6 of the north star."""
    g = hip.Geometry(-78.0, -5.0, xres, yres, nrow, ncol)
    xy, y = synth_stations(n, n + 1, g)
    m = otps.fit(xy, y)
    t = hip.Tps.from_coef(m["knots"], m["c"], m["d"], m["lambda"], m["center"], m["scale"])
    try:
        hip.eval_mode(hip.EVAL_DIRECT)
        direct = hip.interpolate(g, t, window=window).cpu().numpy()
        hip.eval_mode(hip.EVAL_FAR_FIELD)
        far = hip.interpolate(g, t, window=window).cpu().numpy()
    finally:
        hip.eval_mode(hip.EVAL_AUTO)
    auto = hip.interpolate(g, t, window=window).cpu().numpy()
    r0, r1, c0, c1 = window or (0, nrow, 0, ncol)
    want = otps.predict_grid(m, g.xmin, g.ymax, g.xres, g.yres, nrow, ncol, r0, r1, c0, c1)
    scale = np.abs(want).max()
    assert not np.array_equal(far, direct)                     # really a different summation
    # the bound that holds for any coefficients is relative to S = sum_j |c_j phi_j| (a fitted spline's
    # terms cancel by 1e3..1e4), like the rounding error of the direct sum itself
    rr, cc = np.arange(r0, r1, 7), np.arange(c0, c1, 7)
    x = (g.xmin + (cc + 0.5) * g.xres - m["center"][0]) / m["scale"][0]
    yy = (g.ymax - (rr + 0.5) * g.yres - m["center"][1]) / m["scale"][1]
    S = 0.0
    for j in range(n):
        d2 = (x[None, :] - m["knots"][j, 0]) ** 2 + (yy[:, None] - m["knots"][j, 1]) ** 2
        with np.errstate(divide="ignore", invalid="ignore"):
            S = S + np.abs(m["c"][j]) * np.abs(np.where(d2 > 0, d2 * np.log(d2), 0.0)) * (0.5 / (8 * np.pi))
    # 1e-13 S: both paths carry the table log's absolute error per term, at different points -- up to 1.85e-13 on
    # log r2 near r2 = 1 (two roundings at e ln 2 ~ 709 and the rounded bias; the 2e-14 in devmath.h is log m alone:
    # tests/test_devmath_host.py derives the bound, profiles/devmath_bounds.txt holds the 1.7e-13 measured), which is
    # ~1e-13 of a term only where |log r2| >= 2, and the terms' errors do not add up in one direction; the interpolation
    # itself contributes 6e-15 S on square tiles and up to 8e-14 S at the ends of the accepted aspect window
    # (test_far_field_rule_at_its_worst_accepted_geometry)
    assert np.abs(far - direct).max() <= 1e-13 * S.max(), (np.abs(far - direct).max(), S.max())
    assert np.abs(far - direct).max() / scale < 1e-10
    assert np.abs(far - want).max() / scale < RTOL
    assert np.abs(auto - want).max() / scale < RTOL


def test_eval_mode_and_plan_reporting(hip):
    """mhs_tps_eval_mode / mhs_tps_eval_plan: small windows and few knots take the direct sum whatever the mode,
    the plan reports what the last evaluation did, bad modes are refused."""
    g = hip.Geometry(-78.0, -5.0, 1.0 / 1200, 1.0 / 1200, 512, 512)
    xy, y = synth_stations(400, 21, g)
    m = otps.fit(xy, y, lam=1e-3)
    t = hip.Tps.from_coef(m["knots"], m["c"], m["d"], m["lambda"], m["center"], m["scale"])
    try:
        hip.eval_mode(hip.EVAL_FAR_FIELD)
        hip.interpolate(g, t)
        tc, tr, node_pairs, cell_pairs = t.eval_plan()
        assert tc >= 64 and tc % 64 == 0 and tr >= 16 and tr % 16 == 0
        ntiles = -(-512 // tc) * -(-512 // tr)
        assert 0 < node_pairs <= ntiles * 256 * 400 and 0 < cell_pairs < 512 * 512 * 400
        hip.interpolate(g, t, window=(0, 512, 0, 40))          # narrower than one tile column block: direct
        assert t.eval_plan() == (0, 0, 0, 0)
        hip.eval_mode(hip.EVAL_DIRECT)
        hip.interpolate(g, t)
        assert t.eval_plan() == (0, 0, 0, 0)
        few = hip.Tps.from_coef(m["knots"][:20], m["c"][:20], m["d"], m["lambda"], m["center"], m["scale"])
        hip.eval_mode(hip.EVAL_FAR_FIELD)
        hip.interpolate(g, few)
        assert few.eval_plan() == (0, 0, 0, 0)                 # 20 knots: not worth tiling
        with pytest.raises(hip.MhsError):
            hip.eval_mode(7)
    finally:
        hip.eval_mode(hip.EVAL_AUTO)


def test_far_field_with_every_knot_outside_the_window(hip):
    """A band far from the stations: every knot sits in the rim bins, the whole sum is interpolated."""
    g = hip.Geometry(-78.0, -5.0, 1.0 / 1200, 1.0 / 1200, 1200, 400)
    rng = np.random.default_rng(8)
    rows, cols = rng.integers(0, 150, 300), rng.integers(0, 400, 300)          # stations in the top 150 rows only
    cells = np.unique(rows * 400 + cols)
    rows, cols = np.divmod(cells, 400)
    xy = np.column_stack([g.x_from_col(cols), g.y_from_row(rows)])
    y = np.sin(0.01 * cols) + 0.1 * rng.standard_normal(cells.size)
    m = otps.fit(xy, y, lam=1e-2)
    t = hip.Tps.from_coef(m["knots"], m["c"], m["d"], m["lambda"], m["center"], m["scale"])
    win = (900, 1200, 0, 400)
    try:
        hip.eval_mode(hip.EVAL_FAR_FIELD)
        far = hip.interpolate(g, t, window=win).cpu().numpy()
        assert t.eval_plan()[0] > 0 and t.eval_plan()[3] == 0              # no (cell, near knot) pair at all
    finally:
        hip.eval_mode(hip.EVAL_AUTO)
    want = otps.predict_grid(m, g.xmin, g.ymax, g.xres, g.yres, 1200, 400, *win)
    assert np.abs(far - want).max() / np.abs(want).max() < RTOL


@pytest.mark.parametrize("seed", range(6))
def test_far_field_equals_direct_on_random_geometries(hip, seed):
    """Random cell sizes (anisotropic), grid shapes, windows and station layouts (clustered, partly outside the
    window): the far-field-interpolated sum against the direct sum of the same handle."""
    rng = np.random.default_rng(1000 + seed)
    nrow, ncol = int(rng.integers(200, 900)), int(rng.integers(200, 900))
    xres, yres = 1.0 / rng.integers(300, 2400), 1.0 / rng.integers(300, 2400)
    g = hip.Geometry(-78.0, -5.0, xres, yres, nrow, ncol)
    n = int(rng.integers(60, 700))
    # clustered stations: a mixture of a uniform cloud and two blobs
    u = np.vstack([rng.uniform(0, 1, (n // 2, 2)), rng.normal([0.2, 0.7], 0.05, (n // 4, 2)),
                   rng.normal([0.8, 0.3], 0.1, (n - n // 2 - n // 4, 2))]).clip(0.001, 0.999)
    cells = np.unique((u[:, 1] * nrow).astype(int) * ncol + (u[:, 0] * ncol).astype(int))
    rows, cols = np.divmod(cells, ncol)
    xy = np.column_stack([g.x_from_col(cols), g.y_from_row(rows)])
    y = np.sin(5 * u[:len(cells), 0]) + rng.standard_normal(len(cells)) * 0.2
    t = hip.Tps(xy, y)
    r0 = int(rng.integers(0, nrow // 3)); r1 = int(rng.integers(2 * nrow // 3, nrow + 1))
    c0 = int(rng.integers(0, ncol // 3)); c1 = int(rng.integers(2 * ncol // 3, ncol + 1))
    win = (r0, r1, c0, c1)
    try:
        hip.eval_mode(hip.EVAL_DIRECT)
        direct = hip.interpolate(g, t, window=win).cpu().numpy()
        hip.eval_mode(hip.EVAL_FAR_FIELD)
        far = hip.interpolate(g, t, window=win).cpu().numpy()
        used = t.eval_plan()[0] > 0
    finally:
        hip.eval_mode(hip.EVAL_AUTO)
    assert np.isfinite(far).all()
    assert np.abs(far - direct).max() <= 1e-9 * np.abs(direct).max(), (used, t.eval_plan())


def test_points_match_oracle_and_knot_coincidence(hip):
    g = hip.Geometry(-78.0, -5.0, 1.0 / 1200, 1.0 / 1200, 200, 200)
    xy, y = synth_stations(300, 11, g)
    m = otps.fit(xy, y)
    t = hip.Tps.from_coef(m["knots"], m["c"], m["d"], m["lambda"], m["center"], m["scale"])
    rng = np.random.default_rng(5)
    pts = np.vstack([xy, np.column_stack([rng.uniform(-78.1, -77.7, 1000), rng.uniform(-5.3, -4.9, 1000)])])
    got = t.predict(pts)  # first 300 points sit exactly on knots (r2 == 0)
    want = otps.predict_points(m, pts)
    assert np.abs(got - want).max() / np.abs(want).max() < RTOL


def test_exactly_linear_residual_gives_plane(hip):
    """G4 analytic KAT: c == 0 => the surface is the plane d0 + d1 u + d2 v."""
    g = hip.Geometry(0.0, 10.0, 0.01, 0.01, 100, 120)
    rng = np.random.default_rng(1)
    kn = rng.uniform(0, 1, (50, 2))
    t = hip.Tps.from_coef(kn, np.zeros(50), [1.5, -2.0, 0.25], 0.0, [0.0, 9.0], [1.2, 1.0])
    got = hip.interpolate(g, t).cpu().numpy()
    u = (g.x_from_col(np.arange(120)) - 0.0) / 1.2
    v = (g.y_from_row(np.arange(100)) - 9.0) / 1.0
    want = 1.5 - 2.0 * u[None, :] + 0.25 * v[:, None]
    assert np.abs(got - want).max() < 1e-13


def test_bad_arguments_are_rejected(hip):
    g = hip.Geometry(0.0, 1.0, 0.1, 0.1, 10, 10)
    t = hip.Tps.from_coef(np.random.rand(5, 2), np.zeros(5), [0, 0, 0], 0.0, [0, 0], [1, 1])
    with pytest.raises(hip.MhsError):
        hip.interpolate(g, t, window=(0, 11, 0, 10))
    with pytest.raises(hip.MhsError):
        hip.Tps.from_coef(np.random.rand(5, 2), np.zeros(5), [0, 0, 0], 0.0, [0, 0], [0, 1])


def _term_bounds(knots, cw, u, v):
    """sum_j |cw_j| r2logr2_bound(|(u, v) - knot_j|^2) at the points u[None, :] x v[:, None]: the log bound of
    tests/test_devmath_host.py summed over the terms"""
    u, v = np.asarray(u)[None, :], np.asarray(v)[:, None]
    s = np.zeros((v.shape[0], u.shape[1]))
    for (ku, kv), w in zip(knots, cw):
        d2 = (u - ku) ** 2 + (v - kv) ** 2
        s = s + abs(w) * np.where(d2 > 0, r2logr2_bound(np.where(d2 > 0, d2, 1.0)), 0.0)
    return s


def far_field_worst_case(hip, k4, ty, lo=0.8, hi=1.25):
    """The body of test_far_field_rule_at_its_worst_accepted_geometry for the layout devmath_ref.far_layout(k4);
    returns the figures it asserted on."""
    e, ty_l, kn, c = R.far_layout(k4)
    assert ty_l == ty
    g = hip.Geometry(e.xmin, e.ymax, e.xres, e.yres, e.nr, e.nc)
    t = hip.Tps.from_coef(kn, c, [0.0, 0.0, 0.0], 0.0, [0.0, 0.0], [1.0, 1.0])
    try:
        hip.eval_mode(hip.EVAL_FAR_FIELD)
        far = hip.interpolate(g, t).cpu().numpy()
        tiles = t.eval_plan()[:2]
        hip.eval_mode(hip.EVAL_DIRECT)
        direct = hip.interpolate(g, t).cpu().numpy()
    finally:
        hip.eval_mode(hip.EVAL_AUTO)
    plan = R.far_plan_choose(kn, e, lo=lo, hi=hi)
    print("4 * aspect", k4, "device tiles", tiles, "restated plan", plan and (plan["tx"], plan["ty"], plan["tile_aspect"]))
    assert tiles == (64, ty)
    assert plan is not None and (plan["tx"], plan["ty"]) == tiles          # the restated far_plan_choose agrees
    share, fi, ni = R.far_method_error(e, plan, kn, c, 2, 2)
    print("method error, share of the far knots' sum:", share)
    assert len(fi) >= 32 and share <= 1e-10                                # what the aspect window has to keep
    rows, cols = slice(2 * ty, 3 * ty), slice(128, 192)
    want64, Lx, Ly, F = R.far_tile_f64(e, plan, kn, c, [0.0, 0.0, 0.0], 2, 2)
    uc, vc = R.cell_coords(e, range(128, 192), range(2 * ty, 3 * ty))
    exact = R.phi_sum_ld(kn, c, uc, vc)
    S_far = R.phi_sum_ld(kn[fi], c[fi], uc, vc, absolute=True).astype(np.float64)
    cw = c * R.TPS_KK
    un, vn = R.ff_node_coords(e, plan, 2, 2, R.cheb_points())
    lam = np.abs(Lx).sum(1).max() * np.abs(Ly).sum(1).max()                 # largest absolute row sums
    assert 1.0 < lam < 2.73 ** 2                                             # (2 / pi) ln 16 + 0.9625 per direction
    allow_far = lam * _term_bounds(kn[fi], cw[fi], un, vn).max()
    allow = allow_far + _term_bounds(kn[ni], cw[ni], uc, vc)
    allow_direct = _term_bounds(kn, cw, uc, vc)
    d64 = np.abs(far[rows, cols] - want64)
    dex = np.abs((far[rows, cols].astype(R.LD) - exact).astype(np.float64))
    ddi = np.abs((direct[rows, cols].astype(R.LD) - exact).astype(np.float64))
    method = 1.5 * share * S_far.max()
    out = {"far_vs_f64": (d64 / allow).max(), "far_vs_exact": (dex / (method + allow)).max(), "direct_vs_exact": (ddi / allow_direct).max(),
           "far_vs_exact_abs": dex.max(), "method_abs": share * S_far.max(), "allow": allow.max(), "S_far": S_far.max()}
    print(out)
    assert (d64 <= allow).all(), out                 # device far against the float64 restatement of the same interpolant
    assert (dex <= method + allow).all(), out        # device far against the exact sum
    assert (ddi <= allow_direct).all(), out          # device direct against the exact sum: the log bound alone
    other = np.ones(far.shape, dtype=bool)
    other[rows, cols] = False
    rest = np.abs(far - direct)[other].max()
    print("other cells, far - direct:", rest, "of max |direct|", rest / np.abs(direct).max())
    assert not np.array_equal(far, direct)
    assert rest <= 1e-9 * np.abs(direct).max()
    return out


@pytest.mark.parametrize("k4,ty", [(4.0, 64), (2.49, 32), (2.51, 48)])
def test_far_field_rule_at_its_worst_accepted_geometry(hip, k4, ty):
    """5 x 5 tiles of 64 columns by ty rows with 4 * aspect = 4.0, 2.49, 2.51 (tile aspect 1.0, 1.245, 0.837: the
    square tile and the two ends of far_plan_choose's window), 48 knots with positive c: 44 in the ring of bins at
    Chebyshev distance 2 from the centre tile, within a cell of the edge that faces it (some exactly on it), or
    collapsed onto the rim bins; 4 on the bin edges of the 3 x 3 block.  On the centre tile's cells:

      far - float64 restatement of the same interpolant (devmath_ref.far_tile_f64)   <= rounding allowance
      far - exact sum (long double)      <= 1.5 * the interpolant's own error in long double + rounding allowance
      direct - exact sum                 <= the log bound summed over the terms

    The rounding allowance is the log bound of tests/test_devmath_host.py (r2logr2_bound) summed over the terms: for
    the interpolated part the largest such sum over the tile's nodes times the product of the largest absolute row
    sums of Lx and Ly, for the near knots the cell's own sum.  The 1.5 covers float64 nodes against long-double nodes,
    nothing else.  The interpolant's own error must stay under 1e-10 of the far knots' sum.  On all other cells: far
    against direct at 1e-9 of the surface, as test_far_field_equals_direct_on_random_geometries has it."""
    far_field_worst_case(hip, k4, ty)


@pytest.mark.parametrize("k4,ty,aspect", [(1.26, 16, 1.26), (1.59, 32, 0.795)])
def test_far_field_rule_is_refused_just_outside_the_aspect_window(hip, k4, ty, aspect):
    """The same layout with tiles of aspect 1.26 and 0.795, just outside far_plan_choose's 0.8 .. 1.25: asked for the
    far-field path, the evaluation must still take the direct sum, as the restated far_plan_choose says, and give the
    direct sum's values.  (test_far_field_rule_at_its_worst_accepted_geometry holds the window's accepted ends; with
    this the window cannot widen unnoticed.)"""
    e, ty_l, kn, c = R.far_layout(k4)
    assert ty_l == ty and R.far_plan_choose(kn, e) is None
    wide = R.far_plan_choose(kn, e, lo=0.5, hi=2.0)                       # what a wider window would have tiled
    assert (wide["tx"], wide["ty"]) == (64, ty) and abs(wide["tile_aspect"] - aspect) < 1e-12
    g = hip.Geometry(e.xmin, e.ymax, e.xres, e.yres, e.nr, e.nc)
    t = hip.Tps.from_coef(kn, c, [0.0, 0.0, 0.0], 0.0, [0.0, 0.0], [1.0, 1.0])
    try:
        hip.eval_mode(hip.EVAL_FAR_FIELD)
        far = hip.interpolate(g, t).cpu().numpy()
        assert t.eval_plan() == (0, 0, 0, 0)
        hip.eval_mode(hip.EVAL_DIRECT)
        direct = hip.interpolate(g, t).cpu().numpy()
    finally:
        hip.eval_mode(hip.EVAL_AUTO)
    assert np.array_equal(far, direct)
