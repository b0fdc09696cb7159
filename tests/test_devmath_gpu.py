"""The table log, the table exp and nnet's sigmoid cut on the device, through one-term models, against their host
restatements (tests/devmath_ref.py; bounds and coverage: tests/test_devmath_host.py).  The library is built without
contraction and every device operation involved is correctly rounded, so device values EQUAL the restatement as
doubles; no last-bit allowance is needed."""
import math

import numpy as np
import pytest

import devmath_ref as R

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ table log --
@pytest.fixture(scope="module")
def one_knot(hip):
    """one knot at (0, 0), c = 1, d = 0, centre 0, scale 1: f(x, 0) = cw r2logr2(fl(x x)), cw = 1 * (0.5 / (8 pi))"""
    return hip.Tps.from_coef([[0.0, 0.0]], [1.0], [0.0, 0.0, 0.0], 0.0, [0.0, 0.0], [1.0, 1.0])


def test_table_log_points_kernel_equals_the_restatement(hip, one_knot):
    xs = R.log_sweep_points()
    assert 15000 < xs.size < 25000
    got = one_knot.predict(np.column_stack([xs, np.zeros_like(xs)]))
    want = np.array([R.tps_one_knot_point(float(x)) for x in xs])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, xs[bad[:5]], got[bad[:5]], want[bad[:5]])


def test_table_log_zero_and_subnormal_arguments(hip, one_knot):
    xs = np.array([0.0, 2.0 ** -520, 1.5 * 2.0 ** -530, 2.0 ** -537, 2.0 ** -600])      # d2 = 0, three subnormals, underflow to 0
    d2 = xs * xs
    assert d2[0] == 0.0 and (d2[1:4] > 0).all() and (d2[1:4] < 2.0 ** -1022).all() and d2[4] == 0.0
    got = one_knot.predict(np.column_stack([xs, np.zeros_like(xs)]))
    assert got[0] == 0.0 and got[4] == 0.0
    assert np.isfinite(got).all() and (np.abs(got) < 1e-300).all()
    assert np.array_equal(got, np.array([R.tps_one_knot_point(float(x)) for x in xs]))


def test_table_log_grid_kernel_agrees_with_the_points_kernel(hip, one_knot):
    """the same one-knot spline on a small grid (direct path: one knot), one cell centre exactly on the knot"""
    g = hip.Geometry(-2.5 * 0.375, 1.5 * 0.25, 0.375, 0.25, 5, 7)          # cell (row 1, col 2) is centred on (0, 0)
    assert g.x_from_col(2) == 0.0 and g.y_from_row(1) == 0.0
    grid = hip.interpolate(g, one_knot).cpu().numpy()
    assert one_knot.eval_plan()[:2] == (0, 0)
    xx, yy = np.meshgrid(g.x_from_col(np.arange(7)), g.y_from_row(np.arange(5)))
    pts = one_knot.predict(np.column_stack([xx.ravel(), yy.ravel()])).reshape(5, 7)
    assert grid[1, 2] == 0.0
    assert np.array_equal(grid, pts)
    # and both equal the restatement of the kernels' common arithmetic
    kn = [(0.0, 0.0, 1.0 * R.TPS_KK)]
    want = np.array([[0.0 + 0.0 * x + 0.0 * y + R.tps_accumulate(kn, [0], float(x), float(y), 0.0) for x in xx[0]] for y in yy[:, 0]])
    assert np.array_equal(grid, want)


# ------------------------------------------------------------------------------------------------ table exp --
SIGMA = 700.0          # sigma / 700 = 1: q = fl(fl(sigma / 700) * fl(t t)) = fl(t t), the sweep's u


def _one_vector(hip, sigma=SIGMA):
    return hip.models.Ksvm([1.0], [[0.0, 0.0, 0.0]], 0.0, sigma, [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], 0.0, 1.0)


def test_table_exp_svr_kernel_equals_the_restatement(hip):
    """one support vector at 0, alpha = 1, b = 0: the prediction at (t, 0, 0) is table_exp_neg_acc(clamp(q), 0)"""
    ts = R.exp_sweep_points()
    us = ts * ts
    assert (us == 0.0).any() and (us == 1.0).any() and (us > 1.0).sum() >= 3
    X = np.column_stack([ts, np.zeros_like(ts), np.zeros_like(ts)])
    got = _one_vector(hip).predict_points(X)
    want = np.array([R.table_exp_neg_acc(min(float(u), 1.0)) for u in us])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, ts[bad[:5]], got[bad[:5]], want[bad[:5]])
    assert got[us == 0.0][0] == 1.0
    floor = R.table_exp_neg_acc(1.0)
    assert (got[us >= 1.0] == floor).all() and abs(floor / math.exp(-700.0) - 1.0) < 4e-13
    # the whole model path restated (record, fma chain, clamp) gives the same, and so does another sigma
    sub = slice(0, None, 97)
    assert np.array_equal(got[sub], R.svr_predict([1.0], [[0.0, 0.0, 0.0]], 0.0, SIGMA, [0.0] * 3, [1.0] * 3, 0.0, 1.0, X[sub]))
    got2 = _one_vector(hip, 123.0).predict_points(X[sub])
    assert np.array_equal(got2, R.svr_predict([1.0], [[0.0, 0.0, 0.0]], 0.0, 123.0, [0.0] * 3, [1.0] * 3, 0.0, 1.0, X[sub]))


def test_table_exp_two_vectors_of_either_sign(hip):
    """a positive and a smaller negative alpha: ln(|alpha| / amax) in the record, the b_k of a vector off the origin,
    the second accumulator and its subtraction, the scaling back -- equal to the restatement"""
    alpha, sv = [1.75, -0.4], [[0.0, 0.0, 0.0], [0.25, -0.5, 0.125]]
    xc, xs = [0.1, -0.2, 0.3], [1.5, 0.75, 2.0]
    rng = np.random.default_rng(11)
    ts = R.exp_sweep_points()[::13]
    X = np.column_stack([ts * 25.0, rng.uniform(-1, 1, ts.size), rng.uniform(-2, 2, ts.size)])      # q up to the clamp and beyond
    X[::5, 1:] = 0.0
    # b = 0, y_center = 0: the difference of the two sums keeps its own relative precision down to 1e-300;
    # then with an offset and a centre, which swamp all but the largest terms
    for b, yc, distinct in ((0.0, 0.0, ts.size // 2), (0.3, 4.0, 16)):
        m = hip.models.Ksvm(alpha, sv, b, 1.9, xc, xs, yc, 2.5)
        got = m.predict_points(X)
        want = R.svr_predict(alpha, sv, b, 1.9, xc, xs, yc, 2.5, X)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (bad.size, X[bad[:3]], got[bad[:3]], want[bad[:3]])
        assert np.unique(got).size > distinct
        if b == 0.0:
            assert (got > 0).any() and (got < 0).any()              # either sum can be the larger one


def test_table_exp_row_tile_kernel_against_the_lane_per_cell_kernel(hip, monkeypatch):
    """svr_rt_kernel on a 1-layer stack of 6 rows by 384 columns (two waves of 192 cells per row) whose plane carries
    sqrt(u) of the exp sweep, one support vector, against svr_kernel (MHS_SVR_NO_ROWTILE=1) cell by cell and relative to
    the cell's own value.

    A wave whose q spread over more than 0.5 keeps the per-pair addition and must agree bit for bit.  A wave that folds
    evaluates table_exp(u + (S - q_c)) exp(700 (S - q_c)) with S the wave's largest q.  Rounded operations on the
    exponent path, each at most 2^-53 at a magnitude below 2 and each worth 700 times that in the result:
      lane-per-cell  q + A, the two fmas with b_k x_k, r inside the table exp                               4
      folded         A + S, the two fmas, r, S - q_c, 700 (S - q_c)                                         6
      both           the three roundings of NK = -700 * 4096 / ln 2, which now act on S - q_c as well      3
    m = 13.  (The folded waves here keep u + (S - q_c) below the clamp at 1: beyond it the folded form's floor is
    exp(-700 (1 - (S - q_c))) where the other kernel's is exp(-700), both far below 1e-150 of the largest term.)"""
    nrow, ncol = 6, 384
    g = hip.Geometry(0.0, 1.0, 2.0 ** -10, 2.0 ** -10, nrow, ncol)
    us = np.sort(np.unique(R.exp_sweep_points() ** 2))
    rng = np.random.default_rng(5)

    def pick(lo, hi):
        pool = us[(us >= lo) & (us <= hi)]
        assert pool.size >= 192
        return np.concatenate([pool[[0, -1]], rng.permutation(pool[1:-1])[:190]])       # the range's ends always
    spans = [[(0.0, 0.40), (0.45, 0.80)], [(0.20, 0.62), (0.0, 1.0)], [(0.30, 0.95), (0.70, 0.82)],
             [(0.0, 0.02), (0.30, 1.6)], [(0.001, 0.3), (0.5, 0.8)], [(0.0, 0.03), (0.35, 0.8)]]
    u = np.array([np.concatenate([pick(*w) for w in row]) for row in spans])
    plane = np.sqrt(u)
    stack = hip.RasterStack(g, plane[None].copy(), float("nan"))
    sv = [[0.05, 0.1, -0.2]]
    xc, xs = [0.0, 0.1875, 0.997], [1.0, 2.0 ** 4, 2.0 ** 4]
    m = hip.models.Ksvm([1.0], sv, 0.0, SIGMA, xc, xs, 0.0, 1.0)
    got = hip.predict(stack, m).cpu().numpy()
    monkeypatch.setenv("MHS_SVR_NO_ROWTILE", "1")
    plain = hip.predict(stack, m).cpu().numpy()
    monkeypatch.delenv("MHS_SVR_NO_ROWTILE")
    # the lane-per-cell kernel equals the restatement (LONG and LAT as the kernels generate them)
    X = np.column_stack([plane.ravel(), np.tile(g.x_from_col(np.arange(ncol)), nrow), np.repeat(g.y_from_row(np.arange(nrow)), ncol)])
    sub = np.arange(0, nrow * ncol, 7)
    assert np.array_equal(plain.ravel()[sub], R.svr_predict([1.0], sv, 0.0, SIGMA, xc, xs, 0.0, 1.0, X[sub]))
    Z = (X - xc) / xs
    q = (Z * Z).sum(1).reshape(nrow, ncol)
    M = 13
    folded = unfolded = 0
    for r in range(nrow):
        for w in range(2):
            sl = (r, slice(192 * w, 192 * (w + 1)))
            spread = q[sl].max() - q[sl].min()
            assert abs(spread - 0.5) > 0.02
            if spread > 0.5:
                unfolded += 1
                assert np.array_equal(got[sl], plain[sl]), (r, w)
            else:
                folded += 1
                arg = (((Z[:, None, :] - np.array(sv)[None]) ** 2).sum(-1)[:, 0]).reshape(nrow, ncol)[sl]
                assert (arg + (q[sl].max() - q[sl])).max() < 0.999          # below the clamp
                rel = np.abs(got[sl] / plain[sl] - 1.0).max()
                assert rel <= 700.0 * M * 2.0 ** -53, (r, w, rel)
    assert folded >= 6 and unfolded >= 3
    assert not np.array_equal(got, plain)                                   # the row-tile kernel did run


# ------------------------------------------------------------------------------------------------- nnet cut --
def test_nnet_sigmoid_cut_and_accuracy(hip):
    """one hidden unit with weight 1 on the first input, output weight 1: the prediction is nnet.c's sigmoid(z) --
    exactly 0 below -15, exactly 1 above 15, elsewhere within 2 ulp of 1 / (1 + exp(-z)) (the exponential, the sum and
    the quotient each round once)."""
    up, dn = lambda x: math.nextafter(x, math.inf), lambda x: math.nextafter(x, -math.inf)
    z = np.concatenate([np.linspace(-40.0, 40.0, 4001), [-15.0, dn(-15.0), up(-15.0), 15.0, dn(15.0), up(15.0), 0.0, -0.0, 1e-300, -1e-300]])
    m = hip.models.Nnet([0.0, 1.0, 0.0, 0.0, 1.0], 2, size=1)
    got = m.predict_points(np.column_stack([z, np.zeros_like(z)]))
    assert (got[z < -15.0] == 0.0).all() and (z < -15.0).sum() > 1000
    assert (got[z > 15.0] == 1.0).all() and (z > 15.0).sum() > 1000
    mid = (z >= -15.0) & (z <= 15.0)
    want = (R.LD(1.0) / (R.LD(1.0) + np.exp(-z[mid].astype(R.LD))))
    err = np.abs(got[mid].astype(R.LD) - want).astype(np.float64)
    ulps = err / np.array([math.ulp(float(w)) for w in want.astype(np.float64)])
    assert ulps.max() <= 2.0, (ulps.max(), z[mid][np.argmax(ulps)])
    assert got[z == -15.0][0] > 0.0 and got[z == 15.0][0] < 1.0 and got[z == dn(15.0)][0] < 1.0
